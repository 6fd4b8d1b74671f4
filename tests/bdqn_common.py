"""TEST INFRASTRUCTURE ONLY - what the BDQN tests share: the two recorded runs (tests/golden/bdqn_*.npz, written by
tools/gen_golden_bdqn.py from the unmodified reference), their batches, and the tolerances.

Tolerances (the sibling MLP-chain tests', tests/test_gpu_icm.py): per-sample outputs rtol 1e-5 (q with the atol 2e-6 that test
gives logits), gradients 1e-5 max|ref|, parameters rtol 1e-5 / atol 0.02 lr against the oracle and rtol 1e-4 / atol 0.02 lr
against the recorded run, moments rtol 1e-3.  The priority is a sum of D td errors that may cancel: atol 1e-5 max|td| D.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from tests import oracle_bdqn as OB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("double", "per")
STRIDE = 7
RTOL, Q_ATOL, GRAD_RTOL, PAR_RTOL, REC_RTOL, MOM_RTOL = 1e-5, 2e-6, 1e-5, 1e-5, 1e-4, 1e-3
PER_EPS = float(np.finfo(np.float32).eps)
_cache: dict = {}


def load(tag: str) -> dict:
    if tag not in _cache:
        _cache[tag] = dict(np.load(os.path.join(GOLDEN, f"bdqn_{tag}.npz")))
    return _cache[tag]


def dims_of(g) -> tuple:
    d = g["dims"]
    return (int(d[0]), tuple(int(x) for x in g["common"]), int(d[1]), int(d[2]), int(d[3]), int(d[4]), "relu" if d[15] else "tanh")


def cfg_of(g) -> dict:
    d = g["dims"]
    # (cfg = [lr, BDQN(gamma=...), the discount the reference's targets really use]: see tools/gen_golden_bdqn.py)
    return dict(gamma=float(g["cfg"][2]), target_update_freq=int(d[13]), is_double=bool(d[12]),
                optimizer="rmsprop" if d[14] else "adam", lr=float(g["cfg"][0]))


def n_updates(g) -> int:
    return int(g["dims"][9])


def init_params(g, dtype=torch.float32, device="cpu") -> dict:
    return {k: torch.as_tensor(g["init_" + k]).to(dtype).to(device) for k in OB.state_keys(dims_of(g))}


def batch_of(g, u: int, dtype=torch.float32, device="cpu") -> dict:
    """The rows update u sampled: obs, act [B, D], obs_next, rew, end, weight (None for the plain buffer)."""
    idx = g[f"u{u}_indices"]
    t = lambda x, dt=dtype: torch.as_tensor(np.asarray(x)).to(dt).to(device)  # noqa: E731
    return dict(obs=t(g["obs"][idx]), act=t(g["act"][idx], torch.int64), obs_next=t(g["obs_next"][idx]), rew=t(g["rew"][idx]),
                end=t(g[f"u{u}_end"], torch.bool), weight=t(g[f"u{u}_is_weight"]) if f"u{u}_is_weight" in g else None)


def max_td(g, u: int) -> float:
    """An upper bound of |td| in update u from recorded data alone (|ret| + max|q| is not recorded; |prio| <= D max|td|)."""
    return float(max(np.abs(g[f"u{u}_weight_out"]).max(), np.abs(g[f"u{u}_returns"]).max(), 1.0))


def prio_atol(g, u: int) -> float:
    return 1e-5 * max_td(g, u) * int(g["dims"][3])


def oracle_run(g, dtype=torch.float32, device="cpu"):
    """Drives tests/oracle_bdqn.Agent through the recorded run -> (agent, per-update dicts of ret, loss, prio, params, old)."""
    cfg = cfg_of(g)
    agent = OB.Agent(init_params(g, dtype, device), dims_of(g), **cfg)
    steps = []
    for u in range(n_updates(g)):
        b = batch_of(g, u, dtype, device)
        ret = agent.target_q(b["obs_next"], b["rew"], b["end"])
        val, prio = agent.update(b["obs"], b["act"], ret, b["weight"])
        steps.append(dict(ret=ret.cpu().numpy(), loss=float(val), prio=prio.cpu().numpy(), params=agent.cat().cpu().numpy(),
                          old=agent.cat(old=True).cpu().numpy() if agent.old is not None else None))
    return agent, steps


def expected_tree(g, u: int, prio: np.ndarray, alpha: float = 0.6) -> np.ndarray:
    """The sum tree after update u from the tree before it and the new priorities: leaf = (|prio| + eps) ** alpha at the sampled
    indices (the last occurrence of a repeated index wins), every inner node the sum of its two children."""
    tree = g[f"u{u}_tree_before"].copy()
    bound = tree.shape[0] // 2
    tree[bound + g[f"u{u}_indices"]] = (np.abs(prio.astype(np.float64)) + PER_EPS) ** alpha
    for i in range(bound - 1, 0, -1):
        tree[i] = tree[2 * i] + tree[2 * i + 1]
    return tree
