"""TEST INFRASTRUCTURE ONLY - loader of the behaviour-cloning fixtures (tools/gen_golden_bc.py), shared by
tests/test_oracle_bc.py and the GPU tests."""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np

from oracle import oracle_dqn as OD
from tests import oracle_bc as OB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("bc_atari.npz", "bc_cartpole.npz", "bc_d4rl.npz")
# case -> (file, key prefix, route of tests/oracle_bc.py)
CASES = {"atari": ("bc_atari.npz", "", "dqnet"), "cartpole": ("bc_cartpole.npz", "", "discrete"),
         "d4rl_a": ("bc_d4rl.npz", "a_", "continuous"), "d4rl_b": ("bc_d4rl.npz", "b_", "continuous")}
STRIDE = 61


def load(case: str) -> SimpleNamespace:
    """-> g (the npz), tag, route, batch, n_updates, seed, lr, max_action, obs / act (the buffer's columns), params0 (oracle
    parameter dict rebuilt from the seed), order (its flat order); dqnet: c, h, w, n_act; MLP routes: obs_dim, n_out, hidden."""
    fname, tag, route = CASES[case]
    g = np.load(os.path.join(GOLDEN, fname))
    cfg = dict(zip([str(k) for k in g["cfg_keys"]], [float(v) for v in g["cfg_vals"]]))
    d = [int(x) for x in g["dims"]]
    out = SimpleNamespace(g=g, tag=tag, route=route, lr=cfg["lr"], max_action=1.0)
    if route == "dqnet":
        _, _, _, out.c, out.h, out.w, out.n_act, out.batch, out.n_updates, out.seed = d
        out.obs, out.act = g["frames"], g["act"]
        out.params0, out.order = OD.init_params(out.c, out.h, out.w, out.n_act, out.seed), OD.PARAM_ORDER
        return out
    _, _, _, out.obs_dim, out.n_out, out.batch, out.n_updates, out.seed = d
    out.hidden = tuple(int(x) for x in g["hidden"])
    if route == "continuous":
        out.max_action = cfg[f"max_action_{tag[0]}"]
        out.obs, out.act = g[f"{tag}obs"], g[f"{tag}act"]
    else:
        out.obs, out.act = g["obs"], g["act"]
    out.params0, out.order = OB.init_mlp_params(out.obs_dim, out.n_out, out.hidden, out.seed), OB.mlp_order(len(out.hidden))
    return out


def flat(p: dict, order) -> np.ndarray:
    import torch

    return torch.cat([p[k].detach().reshape(-1).cpu() for k in order]).numpy()


def biases(p: dict, order) -> np.ndarray:
    import torch

    return torch.cat([p[k].detach().reshape(-1).cpu() for k in order if k.startswith("b") or k.endswith(".b")]).numpy()
