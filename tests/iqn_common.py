"""Shared by the IQN tests: the fixtures of tools/gen_golden_iqn.py (tests/golden/iqn_lagged.npz, iqn_single.npz)."""
import os

import numpy as np

from oracle import oracle as O
from tests import oracle_iqn as OI

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("lagged", "single")


def load_iqn(tag: str):
    g = np.load(os.path.join(GOLDEN, f"iqn_{tag}.npz"))
    E, slots, steps, c, h, w, n_act, n_online, n_target, batch, n_updates, seed = (int(x) for x in g["dims"])
    cd = dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist()))
    cfg = OI.IQNConfig(sample_size=9, online_sample_size=n_online, target_sample_size=n_target, gamma=cd["gamma"],
                       n_step=int(cd["n_step"]), target_update_freq=int(cd["target_update_freq"]), lr=cd["lr"])
    dims = dict(E=E, slots=slots, steps=steps, c=c, h=h, w=w, n_act=n_act, n_online=n_online, n_target=n_target, batch=batch,
                n_updates=n_updates, seed=seed)
    bstate = O.BufferState(g["buf_offset"], g["buf_last_index"], g["buf_lengths"], g["buf_insertion"],
                           g["rew"], g["terminated"], g["truncated"])
    return g, dims, cfg, bstate


def taus_of(g, u: int, lagged: bool):
    """The fractions of update u in the reference's call order -> (target pass: online, lagged or None; update pass)."""
    n = int(g[f"u{u}_n_taus"])
    assert n == (3 if lagged else 2)
    t = [g[f"u{u}_tau{i}"] for i in range(n)]
    return (t[0], t[1], t[2]) if lagged else (t[0], None, t[1])
