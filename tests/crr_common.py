"""Shared by the DiscreteCRR tests: the fixtures of tools/gen_golden_crr.py (tests/golden/crr_exp.npz, crr_binary.npz).

Tolerances.  The DiscreteBCQ figures for the same quantities are the starting point: rtol = 1e-5 on losses and targets,
rtol = 1e-5 with atol = 0.02 * lr on parameters after an update, 1e-5 / 2e-5 of the vector's largest magnitude on the Adam
moments m / v.  "exp" mode with beta = 0.05 amplifies rounding in adv by 1 / beta = 20, so every one of them was checked, not
against the kernel, but against the float32 CPU oracle's own deviation from a float64 run of the same oracle on the fixture
inputs (test_oracle_crr.py::test_float32_oracle_vs_float64 measures all of these again):

* losses and targets: crr_exp.npz 1.2e-6 (relative, the four losses of all updates) and 6.8e-7 (relative to the largest
  target), crr_binary.npz 6.1e-8 and 8.6e-8 (F32_VS_F64).  1e-5 is 8 and 15 times these: the BCQ tolerances stand.
* parameters (PARAM_DEV, per update: the fraction of ALL elements beyond the BCQ bar, the largest deviation in units of lr):
  crr_binary.npz 0 and 0.0022 lr in every update; crr_exp.npz 4.8e-6 (one element) and 0.040 lr in updates 0 to 3, but
  4.9e-3 and 0.61 lr in update 4: there float32 and float64 take different sides of a ReLU whose gradient is not small (the
  losses still agree to 1.2e-6; the value is continuous, the gradient is not), and the reference's own float32 run, which
  the fixture holds, differs from the float64 oracle in 20 of the 3,428 sampled parameters by up to 0.095 lr.
* Adam moments at the end (MOMENT_DEV): crr_binary.npz 3.1e-7 / 1.9e-7 of the largest magnitude, crr_exp.npz 1.2e-2 / 1.1e-3
  for the same reason.

The bar is TWICE the float32 oracle's deviation wherever that exceeds the BCQ figure, and the BCQ figure elsewhere.  Why two:
the fixture's numbers and the numbers under test are two float32 evaluations in different summation orders; each lies within
the measured deviation of the exact result, so they lie within twice that of each other.  In effect: the BCQ bars for
crr_binary.npz and for updates 0 to 3 of crr_exp.npz (twice 4.8e-6 of 3,428 sampled elements allows none); in update 4 of
crr_exp.npz at most 0.98 % of the sampled elements beyond the BCQ bar and none beyond 1.22 lr; moments of crr_exp.npz within
2.4e-2 / 2.2e-3.
"""
import os

import numpy as np

from oracle import oracle as O
from tests import oracle_crr as OC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("exp", "binary")
STRIDE = 61
LOSS_NAMES = ("loss", "actor_loss", "critic_loss", "cql_loss")
F32_VS_F64 = {"loss": 1.2e-6, "target": 6.8e-7}    # measured on the CPU, see the docstring
RTOL = 1e-5
ATOL_LR = 0.02
# float32 oracle vs float64 oracle, per update: (fraction of all parameters beyond rtol * |p| + ATOL_LR * lr, largest |diff| / lr)
PARAM_DEV = {"exp": [(4.8e-6, 0.040)] * 4 + [(4.9e-3, 0.61)], "binary": [(0.0, 0.0022)] * 3}
# ... and of the Adam moments after the last update, relative to the largest magnitude of each vector: (m, v)
MOMENT_DEV = {"exp": (1.2e-2, 1.1e-3), "binary": (3.1e-7, 1.9e-7)}
FACTOR = 2.0
ACTOR_OLD = list(range(10))                         # positions in the fourteen tensors of actor_old: trunk + actor head
CRITIC_OLD = list(range(6)) + [10, 11, 12, 13]      # ... of critic_old: trunk + critic head


def load_crr(tag: str):
    g = np.load(os.path.join(GOLDEN, f"crr_{tag}.npz"))
    E, slots, steps, c, h, w, n_act, batch, n_updates, seed = (int(x) for x in g["dims"])
    cd = dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist()))
    cfg = OC.CRRConfig(gamma=cd["gamma"], policy_improvement_mode=OC.MODES[int(cd["mode"])], beta=cd["beta"],
                       ratio_upper_bound=cd["ratio_upper_bound"], min_q_weight=cd["min_q_weight"],
                       target_update_freq=int(cd["target_update_freq"]), lr=cd["lr"])
    dims = dict(E=E, slots=slots, steps=steps, c=c, h=h, w=w, n_act=n_act, batch=batch, n_updates=n_updates, seed=seed)
    bstate = O.BufferState(g["buf_offset"], g["buf_last_index"], g["buf_lengths"], g["buf_insertion"],
                           g["rew"], g["terminated"], g["truncated"])
    return g, dims, cfg, bstate


def batch_of(g, u: int):
    """-> (obs, obs_next uint8 [B, c, h, w], act int64 [B], rew float32 [B], done uint8 [B]) of update u."""
    idx = g[f"u{u}_indices"]
    done = (g["terminated"][idx] | g["truncated"][idx]).astype(np.uint8)
    return g["frames"][idx], g["frames_next"][idx], g["act"][idx], g["rew"][idx].astype(np.float32), done


def check_params(got, ref, tag: str, u: int, lr: float, what: str = "parameters") -> None:
    """Sampled parameters after update u against the fixture: the BCQ bar (rtol = 1e-5, atol = 0.02 lr), widened only where
    the float32 oracle's own deviation from float64 (PARAM_DEV) exceeds it, to FACTOR times that deviation."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    frac, worst = PARAM_DEV[tag][u]
    diff = np.abs(got - ref)
    bad = diff > RTOL * np.abs(ref) + ATOL_LR * lr
    print(f"  {tag} u{u} {what}: {int(bad.sum())} of {bad.size} beyond the BCQ bar, largest deviation {diff.max() / lr:.3g} lr")
    assert bad.sum() <= int(FACTOR * frac * bad.size), (what, int(bad.sum()), bad.size)
    assert diff.max() <= max(FACTOR * worst, ATOL_LR) * lr + RTOL * np.abs(ref).max(), (what, diff.max() / lr)


def moment_bars(tag: str) -> tuple[float, float]:
    """-> the bars on (m, v) relative to each vector's largest magnitude: BCQ's 1e-5 / 2e-5, or FACTOR * MOMENT_DEV if larger."""
    m, v = MOMENT_DEV[tag]
    return max(1e-5, FACTOR * m), max(2e-5, FACTOR * v)
