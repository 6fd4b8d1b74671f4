"""TEST INFRASTRUCTURE ONLY - torch fp32 autograd restatement of the reference's TD3+BC update.

Never imported by the product (`tianshou_amd/`).  TD3+BC is TD3 with one more term in the actor loss, so the networks, the target,
the n-step returns, the critic steps and the Adam restatement are oracle/oracle_sac.py's (TD3State, td3_target_q); only the update
is restated here.

Follows:
  update    TD3BC._update_with_batch imitation/td3_bc.py:102-127: both critics by _minimize_critic_squared_loss (ddpg.py:267-285),
            batch.weight = (td1 + td2) / 2; when _cnt % update_actor_freq == 0:
                lmbda = alpha / Q1(s, pi(s)).abs().mean().detach()
                actor_loss = -lmbda * Q1(s, pi(s)).mean() + mse_loss(pi(s), batch.act)
            Optimizer.step algorithm_base.py:484-500 (oracle_sac.Adam), the Polyak updates lagged_network.py:17-18
Tensors follow the parameters' dtype, so the same code in float64 is the reference of the kernel edge tests.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn.functional as F

from oracle import oracle_sac as OS


@dataclass
class TD3BCConfig(OS.TD3Config):
    alpha: float = 2.5


def actor_loss_terms(actor, critic1, obs, act, max_action: float, alpha: float):
    """td3_bc.py:114-117 -> (actor_loss with graph, lmbda, Q1(s, pi(s)) [B], pi(s) [B, A])."""
    pi = OS.det_actor_forward(actor, obs, max_action)
    q = OS.critic_forward(critic1, obs, pi)
    lmbda = alpha / q.abs().mean().detach()
    return -lmbda * q.mean() + F.mse_loss(pi, act), lmbda, q.flatten(), pi


def update_with_batch(st: OS.TD3State, cfg: TD3BCConfig, obs, act, returns, weight=None, collect=None):
    """td3_bc.py:102-127 -> dict(actor_loss, critic1_loss, critic2_loss, weight, lmbda); lmbda and actor_loss are those of the
    latest actor update (`st.last_actor_loss`, and `st.last_lmbda` set here)."""
    obs = torch.as_tensor(obs, dtype=torch.float32)
    act = torch.as_tensor(act, dtype=torch.float32)
    ret = torch.as_tensor(returns, dtype=torch.float32).flatten()
    w = 1.0 if weight is None else torch.as_tensor(weight, dtype=torch.float32)
    out, tds = {}, []
    for name, opt in (("critic1", st.opt_c1), ("critic2", st.opt_c2)):
        p = {k: v.clone().requires_grad_(True) for k, v in getattr(st, name).items()}
        td = OS.critic_forward(p, obs, act).flatten() - ret
        loss = (td.pow(2) * w).mean()
        g = OS._grads(loss, p)
        if collect is not None:
            collect[name + "_grads"] = g
        setattr(st, name, opt.apply(getattr(st, name), g))
        tds.append(td.detach())
        out[name + "_loss"] = float(loss.item())
    out["weight"] = (tds[0] + tds[1]) / 2.0
    if st.cnt % cfg.update_actor_freq == 0:
        p = {k: v.clone().requires_grad_(True) for k, v in st.actor.items()}
        actor_loss, lmbda, _, _ = actor_loss_terms(p, st.critic1, obs, act, cfg.max_action, cfg.alpha)
        g = OS._grads(actor_loss, p)
        if collect is not None:
            collect["actor_grads"] = g
        st.actor = st.opt_actor.apply(st.actor, g)
        st.last_actor_loss = float(actor_loss.item())
        st.last_lmbda = float(lmbda)
        for old, new in ((st.actor_old, st.actor), (st.critic1_old, st.critic1), (st.critic2_old, st.critic2)):
            for k in old:
                old[k] = cfg.tau * new[k] + (1 - cfg.tau) * old[k]
    st.cnt += 1
    out["actor_loss"] = st.last_actor_loss
    out["lmbda"] = getattr(st, "last_lmbda", 0.0)
    return out
