"""TEST INFRASTRUCTURE ONLY - torch autograd restatement of the reference's DiscreteSAC path on the Atari trunk.

Never imported by the product (`tianshou_amd/`).  Lives under tests/ next to the tests that use it; the buffer arithmetic
comes from oracle/oracle.py.

Follows:
  net       DiscreteActor(softmax_output=False), DiscreteCritic(last_size=n_act) twice: three single Linear heads on ONE
            DQNet(features_only=True, output_dim_added_layer=H) (examples/atari/atari_sac.py)
  target    discrete_sac.py:147-155: sum_j p_j min(Q1_old, Q2_old)_j + alpha H(p) on obs_next; p from the LIVE actor and
            trunk, the Qs from the lagged critics, each on its own lagged trunk copy (the two copies stay equal: one is kept)
  update    discrete_sac.py:157-196: THREE torch.optim.Adam instances, each over the shared trunk's eight tensors and its own
            head, stepped strictly in sequence -- critic 2's forward pass sees the trunk after critic 1's step, the actor's
            pass (which also evaluates both critics, without gradient) sees it after both; AutoAlpha.update (sac.py:203-209);
            Polyak of the lagged trunk and the two lagged heads
Gradients come from autograd.  Tensors follow the parameters' device and dtype, so the same code is the float64 yardstick of
the tolerances.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F
from torch.distributions import Categorical

from oracle import oracle_dqn as OD

TRUNK = ["conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc.w", "fc.b"]
HEADS = {"actor": ["a.w", "a.b"], "critic1": ["q1.w", "q1.b"], "critic2": ["q2.w", "q2.b"]}
# ModuleList([policy, critic, critic2]).named_parameters(): the shared trunk once (under the actor), then the three heads
PARAM_ORDER = TRUNK + HEADS["actor"] + HEADS["critic1"] + HEADS["critic2"]
LAGGED_ORDER = TRUNK + HEADS["critic1"] + HEADS["critic2"]
SETS = ("critic1", "critic2", "actor")                      # the engine's order of gradient / moment sets
_TRUNK_KEYS = ["preprocess.net.0.0.weight", "preprocess.net.0.0.bias", "preprocess.net.0.2.weight", "preprocess.net.0.2.bias",
               "preprocess.net.0.4.weight", "preprocess.net.0.4.bias", "preprocess.net.1.weight", "preprocess.net.1.bias"]
_HEAD_KEYS = ["last.model.0.weight", "last.model.0.bias"]
TIANSHOU_KEYS = ["0.actor." + k for k in _TRUNK_KEYS + _HEAD_KEYS] + ["1." + k for k in _HEAD_KEYS] + ["2." + k for k in _HEAD_KEYS]
STAT_NAMES = ("actor_loss", "critic1_loss", "critic2_loss", "alpha", "alpha_loss")


def set_order(which: str) -> list[str]:
    """The ten tensors one optimizer holds: the trunk and `which`'s head."""
    return TRUNK + HEADS[which]


@dataclass
class DSACConfig:
    gamma: float = 0.99
    tau: float = 0.005
    n_step: int = 1
    alpha: float = 0.2
    auto_alpha: bool = False
    target_entropy: float = 0.0
    log_alpha0: float = 0.0
    actor_lr: float = 1e-3
    critic_lr: float = 1e-3
    alpha_lr: float = 3e-4
    betas: tuple[float, float] = (0.9, 0.999)
    adam_eps: float = 1e-8


def feature_dim(h: int, w: int) -> int:
    oh, ow = OD.conv_out_hw(h, w)[-1]
    return 64 * oh * ow


def init_params(c: int, h: int, w: int, n_act: int, hidden: int = 512, seed: int = 0) -> dict[str, torch.Tensor]:
    """Same RNG consumption as `torch.manual_seed(seed)` + the example's construction: the DQNet trunk with its added layer,
    the actor's head, the two critics' heads (tools/gen_golden_dsac_cnn.py asserts the equality tensor by tensor)."""
    torch.manual_seed(seed)
    f = feature_dim(h, w)
    mods = {"conv1": torch.nn.Conv2d(c, 32, 8, 4), "conv2": torch.nn.Conv2d(32, 64, 4, 2), "conv3": torch.nn.Conv2d(64, 64, 3, 1),
            "fc": torch.nn.Linear(f, hidden), "a": torch.nn.Linear(hidden, n_act), "q1": torch.nn.Linear(hidden, n_act),
            "q2": torch.nn.Linear(hidden, n_act)}
    p = {}
    for name, m in mods.items():
        p[name + ".w"] = m.weight.detach().clone()
        p[name + ".b"] = m.bias.detach().clone()
    return p


def features(p, obs) -> torch.Tensor:
    ref = p["conv1.w"]
    x = torch.as_tensor(np.asarray(obs) if not isinstance(obs, torch.Tensor) else obs).to(ref.device, ref.dtype)
    x = F.relu(F.conv2d(x, p["conv1.w"], p["conv1.b"], stride=4))
    x = F.relu(F.conv2d(x, p["conv2.w"], p["conv2.b"], stride=2))
    x = F.relu(F.conv2d(x, p["conv3.w"], p["conv3.b"], stride=1))
    return F.relu(F.linear(x.flatten(1), p["fc.w"], p["fc.b"]))


def head(p, feat, which: str) -> torch.Tensor:
    return F.linear(feat, p[which + ".w"], p[which + ".b"])


def _on(x, like: torch.Tensor, dtype=None) -> torch.Tensor:
    x = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return x.to(device=like.device, dtype=dtype if dtype is not None else like.dtype)


# ---- the three head computations on raw arrays (what the per-sample kernels compute) --------------------------------------------
def target_from_heads(logits, q1_old, q2_old, alpha: float) -> torch.Tensor:
    """discrete_sac.py:150-155 -> [B]."""
    dist = Categorical(logits=logits)
    return (dist.probs * torch.min(q1_old, q2_old)).sum(dim=-1) + alpha * dist.entropy()


def critic_from_head(q, act, target, weight=None):
    """discrete_sac.py:163-165 -> (loss scalar with graph, td [B])."""
    act = _on(act, q, torch.int64).reshape(-1, 1)
    td = q.gather(1, act).flatten() - _on(target, q).flatten()
    w = 1.0 if weight is None else _on(weight, q).flatten()
    return (td.pow(2) * w).mean(), td


def actor_from_heads(logits, q1, q2, alpha: float):
    """discrete_sac.py:177-183 -> (loss scalar with graph, entropy [B])."""
    dist = Categorical(logits=logits)
    entropy = dist.entropy()
    q = torch.min(q1.detach(), q2.detach())
    return -(alpha * entropy + (dist.probs * q).sum(dim=-1)).mean(), entropy


class DSACState:
    """Live parameters (leaf tensors; the trunk's eight sit in all three optimizers), the lagged copy, log alpha."""

    def __init__(self, p: dict[str, torch.Tensor], cfg: DSACConfig):
        self.params = {k: p[k].detach().clone().requires_grad_(True) for k in PARAM_ORDER}
        lr = {"critic1": cfg.critic_lr, "critic2": cfg.critic_lr, "actor": cfg.actor_lr}
        self.opt = {s: torch.optim.Adam([self.params[k] for k in set_order(s)], lr=lr[s], betas=cfg.betas, eps=cfg.adam_eps)
                    for s in SETS}
        self.params_old = {k: p[k].detach().clone() for k in LAGGED_ORDER}
        ref = p["conv1.w"]
        self.log_alpha = torch.tensor(float(cfg.log_alpha0), dtype=ref.dtype, device=ref.device, requires_grad=True)
        self.alpha_opt = torch.optim.Adam([self.log_alpha], lr=cfg.alpha_lr, betas=cfg.betas, eps=cfg.adam_eps)
        self.steps = 0

    def moments(self, which_set: str, which: str) -> dict[str, torch.Tensor]:
        """which: "exp_avg" | "exp_avg_sq" -> per-tensor moments of one optimizer (zeros before the first step)."""
        o = self.opt[which_set]
        return {k: (o.state[self.params[k]][which] if o.state.get(self.params[k]) else torch.zeros_like(self.params[k]))
                for k in set_order(which_set)}


def make_state(p, cfg: DSACConfig) -> DSACState:
    return DSACState(p, cfg)


def alpha_of(st: DSACState, cfg: DSACConfig) -> float:
    """Alpha.value: a Python float (AutoAlpha: exp of the parameter in its own precision)."""
    return float(st.log_alpha.detach().exp().item()) if cfg.auto_alpha else float(cfg.alpha)


def policy_logits(p, obs) -> torch.Tensor:
    with torch.no_grad():
        return head(p, features(p, obs), "a")


def target_q(st: DSACState, cfg: DSACConfig, obs_next) -> torch.Tensor:
    """_target_q (ddpg.py:327-339) -> [B]."""
    with torch.no_grad():
        p = {k: v.detach() for k, v in st.params.items()}
        logits = head(p, features(p, obs_next), "a")
        fo = features(st.params_old, obs_next)
        return target_from_heads(logits, head(st.params_old, fo, "q1"), head(st.params_old, fo, "q2"), alpha_of(st, cfg))


def update_with_batch(st: DSACState, cfg: DSACConfig, obs, act, returns, weight=None, collect: dict | None = None,
                      apply: bool = True):
    """discrete_sac.py:157-196 -> ({actor_loss, critic1_loss, critic2_loss, alpha, alpha_loss} floats, (td1 + td2) / 2 [B]).
    apply=False: the three gradients at the unchanged parameters (collect["grads"][set][name]); nothing is stepped."""
    p = st.params
    grads: dict = {}

    def step(which: str, loss) -> None:
        names = set_order(which)
        g = torch.autograd.grad(loss, [p[k] for k in names])
        grads[which] = {k: x.detach().clone() for k, x in zip(names, g)}
        if apply:
            for k, x in zip(names, g):
                p[k].grad = x
            for grp in st.opt[which].param_groups:
                grp["lr"] = cfg.actor_lr if which == "actor" else cfg.critic_lr
            st.opt[which].step()
            for k in names:
                p[k].grad = None

    target = _on(returns, p["conv1.w"]).flatten()
    c1, td1 = critic_from_head(head(p, features(p, obs), "q1"), act, target, weight)
    step("critic1", c1)
    c2, td2 = critic_from_head(head(p, features(p, obs), "q2"), act, target, weight)
    step("critic2", c2)
    new_weight = ((td1 + td2) / 2.0).detach()
    alpha = alpha_of(st, cfg)
    feat = features(p, obs)
    logits = head(p, feat, "a")
    al, entropy = actor_from_heads(logits, head(p, feat, "q1"), head(p, feat, "q2"), alpha)
    step("actor", al)
    alpha_loss = 0.0
    if cfg.auto_alpha:
        a_loss = -(st.log_alpha * (cfg.target_entropy - entropy.detach())).mean()
        alpha_loss = float(a_loss.item())
        if apply:
            for grp in st.alpha_opt.param_groups:
                grp["lr"] = cfg.alpha_lr
            st.alpha_opt.zero_grad()
            a_loss.backward()
            st.alpha_opt.step()
    if apply:
        st.steps += 1
        with torch.no_grad():
            for k in LAGGED_ORDER:                          # lagged_network.py:17-18
                st.params_old[k] = cfg.tau * p[k].detach() + (1 - cfg.tau) * st.params_old[k]
    if collect is not None:
        collect.update(grads=grads, logits=logits.detach().clone(), entropy=entropy.detach().clone(), td1=td1.detach().clone(),
                       td2=td2.detach().clone())
    stats = {"actor_loss": float(al.item()), "critic1_loss": float(c1.item()), "critic2_loss": float(c2.item()),
             "alpha": alpha_of(st, cfg), "alpha_loss": alpha_loss}
    return stats, new_weight
