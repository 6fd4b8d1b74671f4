"""TEST INFRASTRUCTURE ONLY - torch fp32 autograd restatement of the reference's DiscreteCQL update on QRDQNet.

Never imported by the product (`tianshou_amd/`).  DiscreteCQL is QRDQN with one more term in the loss, so the network, the
target, the n-step returns and the Adam step are oracle/oracle_distq.py's (QR) and oracle/oracle_dqn.py's; only the update
is restated here.

Follows:
  update    DiscreteCQL._update_with_batch imitation/discrete_cql.py:80-113: QRDQN's quantile Huber loss and priorities
            (qrdqn.py:111-128), q = QRDQNPolicy.compute_q_value (mean over the quantiles, qrdqn.py:19-21),
            min_q_loss = q.logsumexp(1).mean() - q.gather(1, act).mean(), loss = qr_loss + min_q_loss * min_q_weight;
            periodic hard sync dqn.py:277-285, Optimizer.step algorithm_base.py:484-500 (oracle_dqn._adam)
Tensors follow the parameters' device, so the same code is the eager baseline of bench_cql.py on a GPU.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle_distq as OQ
from oracle import oracle_dqn as OD

warnings.filterwarnings("ignore", message="Using a target size")      # as qrdqn.py:92: the broadcast is intended


@dataclass
class DiscreteCQLConfig(OQ.DistQConfig):
    min_q_weight: float = 10.0


def loss_terms(p, cfg: DiscreteCQLConfig, obs, act, returns, n_act: int, weight=None):
    """discrete_cql.py:85-106 -> (loss, qr_loss, cql_loss: scalar tensors with graph, new batch.weight [B], dist [B, A, N])."""
    dev = p["conv1.w"].device
    x = torch.as_tensor(np.asarray(obs) if not isinstance(obs, torch.Tensor) else obs).to(dev)
    all_dist = OD.forward(p, x).view(-1, n_act, cfg.n_atoms)
    act_t = torch.as_tensor(np.asarray(act.cpu()) if isinstance(act, torch.Tensor) else np.asarray(act), dtype=torch.int64, device=dev)
    ret = torch.as_tensor(returns, dtype=torch.float32, device=dev)
    w = 1.0 if weight is None else torch.as_tensor(weight, dtype=torch.float32, device=dev)
    curr = all_dist[torch.arange(len(act_t), device=dev), act_t, :].unsqueeze(2)
    tgt = ret.unsqueeze(1)
    dist_diff = F.smooth_l1_loss(tgt, curr, reduction="none")
    th = OQ.tau_hat(cfg.n_atoms).to(dev).view(1, -1, 1)
    huber = (dist_diff * (th - (tgt - curr).detach().le(0.0).float()).abs()).sum(-1).mean(1)
    qr_loss = (huber * w).mean()
    prio = dist_diff.detach().abs().sum(-1).mean(1)
    q = all_dist.mean(2)
    dataset_expec = q.gather(1, act_t.unsqueeze(1)).mean()
    negative_sampling = q.logsumexp(1).mean()
    cql_loss = negative_sampling - dataset_expec
    loss = qr_loss + cql_loss * cfg.min_q_weight
    return loss, qr_loss, cql_loss, prio, all_dist


def update_with_batch(st: OD.DQNState, cfg: DiscreteCQLConfig, obs, act, returns, n_act: int, weight=None,
                      collect: dict | None = None):
    """discrete_cql.py:80-113 -> ((loss, qr_loss, cql_loss) floats, new batch.weight float32[B])."""
    if st.params_old is not None and st.iter % cfg.target_update_freq == 0:      # dqn.py:283-285
        st.params_old = {k: v.clone() for k, v in st.params.items()}
    st.iter += 1
    p = {k: v.clone().requires_grad_(True) for k, v in st.params.items()}
    loss, qr_loss, cql_loss, prio, d_all = loss_terms(p, cfg, obs, act, returns, n_act, weight)
    loss.backward()
    grads = {k: v.grad for k, v in p.items()}
    if collect is not None:
        collect["dist"] = d_all.detach().clone()
        collect["grads"] = {k: g.clone() for k, g in grads.items()}
    OD._adam(st, cfg.dqn(), grads)
    return (float(loss.item()), float(qr_loss.item()), float(cql_loss.item())), prio.clone()
