"""TEST INFRASTRUCTURE ONLY - the edge inputs of the GAIL discriminator kernels, shared by tests/test_gail_edge_inputs_cpu.py
(which checks, on the oracle alone, the properties the GPU tests rely on) and tests/test_gpu_gail_edges.py.

Everything is drawn from seeded CPU generators, so both files see the same bits.
"""
from __future__ import annotations

import torch

from tests import oracle_gail as OG

MARGIN = 1e-4            # no float64-oracle logit of a case whose accuracies are compared exactly lies closer to 0 than this

# ---- the loss kernel alone: name -> (logits float32, n_pi, exact_zero) ---------------------------------------------------------
# exact_zero: the case places +0 / -0.0 on purpose (they count for neither accuracy); everywhere else the margin holds.


def _randn(n, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * scale


def loss_cases() -> dict:
    c = {}
    c["zeros"] = (torch.tensor([0.0, -0.0, 0.0, -0.0, 0.0, -0.0]), 3, True)            # both signs of zero on both sides
    c["zeros_mixed"] = (torch.tensor([0.0, -1.5, -0.0, 2.0, -0.0, 0.0, 0.75, -3.0]), 4, True)
    c["tiny"] = (torch.tensor([1e-6, -1e-6, 1e-6, -1e-6, -1e-6, 1e-6]), 3, False)      # |l| = 1e-6 -- see TINY below
    c["sat88"] = (torch.tensor([88.0, -88.0, 88.0, -88.0]), 2, False)                  # exp(88) is finite in float32 ...
    c["sat104"] = (torch.tensor([104.0, -104.0, 104.0, -104.0]), 2, False)             # ... exp(104) is not
    c["sat_one_sided"] = (torch.tensor([104.0, 88.0, 104.0, -104.0, -88.0]), 3, False)  # every row on its losing side
    c["n1_1"] = (torch.tensor([0.7, -0.3]), 1, False)
    c["n1_7"] = (torch.cat([torch.tensor([-1.25]), _randn(7, 11)]), 1, False)
    c["n5_3"] = (_randn(8, 12), 5, False)
    for rows in (255, 256, 257):                                                     # across the 256-row block boundary
        c[f"rows{rows}"] = (_randn(rows, 300 + rows), rows // 2, False)
        c[f"rows{rows}_pi_only_first_block"] = (_randn(rows, 200 + rows), 250, False)
    return c


TINY = ("tiny",)         # the margin condition is waived by the issue's own case list (logits at +-1e-6 are asked for); the signs
                         # are given, not computed, so the accuracies are still exact
SATURATED = ("sat88", "sat104", "sat_one_sided")

# ---- one discriminator step, gradient only: (obs_dim, act_dim, hidden, activation, N, disc_update_num, n_exp_rows, seed) -------
# total rows of the last step = (N - (steps - 1) bsz) + bsz; input width = obs_dim + act_dim
STEP_CASES = {
    # input widths 31 / 32 / 33: the k0 padding boundary and the one-launch route's limit
    "w31_64x64": (25, 6, (64, 64), "tanh", 33, 2, 40, 1),
    "w32_64x64": (26, 6, (64, 64), "tanh", 33, 2, 40, 2),
    "w33_64x64": (27, 6, (64, 64), "tanh", 33, 2, 40, 3),
    # total rows 31 / 32 / 33 / 2: the fused kernel's 32-sample tile edge (N = 31: 16 + 15, 32: 16 + 16, 33: 17 + 16, 1: 1 + 1)
    "rows31": (17, 6, (64, 64), "tanh", 31, 2, 9, 4),
    "rows32": (17, 6, (64, 64), "tanh", 32, 2, 9, 5),
    "rows33": (17, 6, (64, 64), "tanh", 33, 2, 9, 6),
    "rows2": (17, 6, (64, 64), "tanh", 1, 1, 3, 7),
    "rows70": (17, 6, (64, 64), "tanh", 70, 2, 50, 8),              # more than one tile per step
    # other trunks: per-layer route only
    "t32": (5, 3, (32,), "tanh", 33, 2, 9, 9),
    "relu3": (5, 3, (48, 80, 32), "relu", 38, 10, 7, 10),           # the odd fixture's shape: 12 steps, the last 5 against 3
    "relu3_rows2": (5, 3, (48, 80, 32), "relu", 1, 1, 2, 11),
}


def one_launch_shape(case) -> bool:
    od, ad, hidden, act = case[0], case[1], case[2], case[3]
    return tuple(hidden) == (64, 64) and act == "tanh" and od + ad <= 32


def step_case(name: str) -> dict:
    od, ad, hidden, act, n, num, n_exp_rows, seed = STEP_CASES[name]
    g = torch.Generator().manual_seed(1000 + seed)
    bsz, ch = OG.chunks(n, num)
    # a head scaled up so that the logits spread over a few units (an untrained head gives |l| ~ 0.1)
    t = OG.init_disc(od + ad, hidden, seed)
    t[-2] = t[-2] * 8.0
    return dict(name=name, obs_dim=od, act_dim=ad, hidden=list(hidden), activation=act, n=n, num=num, bsz=bsz, chunks=ch, t=t,
                obs=torch.randn(n, od, generator=g), act=torch.randn(n, ad, generator=g),
                obs_exp=torch.randn(n_exp_rows, od, generator=g) + 0.5, act_exp=torch.randn(n_exp_rows, ad, generator=g) - 0.5,
                perm=torch.randperm(n, generator=g), exp_index=torch.randint(0, n_exp_rows, (len(ch) * bsz,), generator=g))


def step_logits64(case: dict) -> list:
    """float64-oracle logits of every step at the case's (unchanged) parameters -> [(l_pi, l_exp)]."""
    t = [x.double() for x in case["t"]]
    ei = case["exp_index"].reshape(len(case["chunks"]), case["bsz"])
    out = []
    for k, (a, b) in enumerate(case["chunks"]):
        rows = case["perm"][a:b]
        out.append((OG.disc_forward(t, case["obs"][rows].double(), case["act"][rows].double(), case["activation"]),
                    OG.disc_forward(t, case["obs_exp"][ei[k]].double(), case["act_exp"][ei[k]].double(), case["activation"])))
    return out


def step_reference(case: dict, dtype=torch.float32):
    """Every step's statistics and gradient at the case's parameters (gradient only: nothing is applied) ->
    (stats [steps, 3], [per-step gradient lists])."""
    t = [x.to(dtype) for x in case["t"]]
    ei = case["exp_index"].reshape(len(case["chunks"]), case["bsz"])
    stats, grads = [], []
    for k, (a, b) in enumerate(case["chunks"]):
        rows = case["perm"][a:b]
        st, gs = OG.disc_grad(t, case["obs"][rows].to(dtype), case["act"][rows].to(dtype), case["obs_exp"][ei[k]].to(dtype),
                              case["act_exp"][ei[k]].to(dtype), case["activation"])
        stats.append(st)
        grads.append(gs)
    return torch.stack(stats), grads


# ---- the chunk rule: (N, disc_update_num) -> (bsz, steps, size of the last policy chunk) -------------------------------------
CHUNK_TABLE = {
    (38, 10): (3, 12, 5),
    (39, 10): (3, 13, 3),
    (27, 4): (6, 4, 9),
    (11, 4): (2, 5, 3),
    (7, 7): (1, 7, 1),           # N = num
    (8, 7): (1, 8, 1),           # N = num + 1
    (5, 1): (5, 1, 5),           # num = 1
}
