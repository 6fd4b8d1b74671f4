"""Shared by the DiscreteBCQ tests: the fixtures of tools/gen_golden_bcq.py (tests/golden/bcq_masked.npz, bcq_plain.npz)."""
import os

import numpy as np

from oracle import oracle as O
from tests import oracle_bcq as OB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("masked", "plain")
STRIDE = 61
LOSS_NAMES = ("loss", "q_loss", "i_loss", "reg_loss")


def load_bcq(tag: str):
    g = np.load(os.path.join(GOLDEN, f"bcq_{tag}.npz"))
    E, slots, steps, c, h, w, n_act, batch, n_updates, seed = (int(x) for x in g["dims"])
    cd = dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist()))
    cfg = OB.BCQConfig(gamma=cd["gamma"], n_step=int(cd["n_step"]), target_update_freq=int(cd["target_update_freq"]), lr=cd["lr"],
                       unlikely_action_threshold=cd["unlikely_action_threshold"],
                       imitation_logits_penalty=cd["imitation_logits_penalty"])
    dims = dict(E=E, slots=slots, steps=steps, c=c, h=h, w=w, n_act=n_act, batch=batch, n_updates=n_updates, seed=seed)
    bstate = O.BufferState(g["buf_offset"], g["buf_last_index"], g["buf_lengths"], g["buf_insertion"],
                           g["rew"], g["terminated"], g["truncated"])
    return g, dims, cfg, bstate
