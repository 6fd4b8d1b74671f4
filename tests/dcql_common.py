"""Shared by the DiscreteCQL tests: the fixtures of tools/gen_golden_dcql.py (tests/golden/dcql_lagged.npz, dcql_single.npz)."""
import os

import numpy as np

from oracle import oracle as O
from tests import oracle_dcql as OC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("lagged", "single")


def load_dcql(tag: str):
    g = np.load(os.path.join(GOLDEN, f"dcql_{tag}.npz"))
    E, slots, steps, c, h, w, n_act, n_atoms, batch, n_updates, seed, prioritized = (int(x) for x in g["dims"])
    cd = dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist()))
    cfg = OC.DiscreteCQLConfig(n_atoms=n_atoms, gamma=cd["gamma"], n_step=int(cd["n_step"]),
                               target_update_freq=int(cd["target_update_freq"]), lr=cd["lr"], min_q_weight=cd["min_q_weight"])
    dims = dict(E=E, slots=slots, steps=steps, c=c, h=h, w=w, n_act=n_act, n_atoms=n_atoms, batch=batch, n_updates=n_updates,
                seed=seed, prioritized=bool(prioritized))
    bstate = O.BufferState(g["buf_offset"], g["buf_last_index"], g["buf_lengths"], g["buf_insertion"],
                           g["rew"], g["terminated"], g["truncated"])
    return g, dims, cfg, bstate


def is_weight(g, u: int, prioritized: bool):
    """The PER weights of update u (None for the plain buffer: the reference's batch carries no `weight`)."""
    return g[f"u{u}_is_weight"] if prioritized else None
