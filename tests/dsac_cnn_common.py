"""Shared by the DiscreteSAC-on-the-Atari-trunk tests: the fixtures of tools/gen_golden_dsac_cnn.py
(tests/golden/dsac_cnn_fixed.npz, dsac_cnn_auto.npz), their loader and the tolerances.

Tolerances.  Where a quantity has a precedent the precedent stands (tests/test_gpu_bcq.py, tests/crr_common.py: the same trunk
and GEMM kernels): rtol = 1e-5 on losses, returns and targets (returns with atol = 1e-5 as there), 1e-5 of a tensor's scale on
gradients (largest element and L2 norm), rtol = 1e-5 with atol = 0.02 * lr on parameters after an update, 1e-5 / 2e-5 of the
vector's largest magnitude on the Adam moments m / v.

alpha_loss and batch.weight have precedents in DiscreteSAC on MLP trunks (tests/test_gpu_dsac.py): rtol = 1e-5 with
atol = 1e-7 on alpha_loss, rtol = 1e-5 with atol = 1e-5 on batch.weight = (td1 + td2) / 2.  The scalar log alpha's two Adam
moments take the moment bars, 1e-5 / 2e-5 relative.

One kind of quantity has no precedent: parameters after THREE chained Adam steps per update on the shared trunk.  It was
measured as the float32 CPU oracle's deviation from a float64 run of the same oracle on the fixture inputs
(test_oracle_dsac_cnn.py::test_float32_oracle_vs_float64 measures it, and every other quantity named here, again and fails if
one exceeds what is recorded below), and the bar is TWICE the measurement wherever that exceeds the precedent.  Why two: the
fixture's numbers and the numbers under test are two float32 evaluations in different summation orders; each lies within
the measured deviation of the exact result, so they lie within twice that of each other.

* PARAM_DEV, per update: the largest deviation beyond rtol * |p|, in units of the larger learning rate.  The first Adam step
  of a tensor moves every element by lr * g / (|g| + eps), so an element whose gradient is of the order of eps = 1e-8 or
  changes sign between two roundings moves by up to lr in either run, and critic 2's and the actor's passes then start from
  that trunk.  Measured: at most 4.2e-5 lr ("fixed") and 7.8e-4 lr ("auto") over ALL parameters of all updates; twice that is
  far below the precedent's 0.02 lr, so the precedent stands for the live and the lagged vector.
* Every other measurement is below half of its precedent too, so no bar is widened: the moments at most 4.5e-6 of a vector's
  scale (against 1e-5 / 2e-5), the four losses and alpha at most 3.8e-6 relative (1e-5), alpha_loss nothing
  beyond rtol = 1e-5 (the atol is 1e-7), log alpha 2.4e-8 (1e-7), log alpha's moments 4.6e-7 / 8.8e-7 relative (1e-5 / 2e-5).

The one-update check on synthetic inputs (test_gpu_dsac_cnn.py::test_three_gradients_and_one_update_vs_oracle) starts from
zero moments, where test_gpu_bcq.py has a bar of its own (check_first_step); the fixtures' bars above are not widened by it.
"""
import os

import numpy as np

from oracle import oracle as O
from tests import oracle_dsac_cnn as OS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAGS = ("fixed", "auto")
STRIDE = 61
RTOL = 1e-5
ATOL_LR = 0.02
FACTOR = 2.0
# float32 oracle vs float64 oracle, per update: largest |diff| beyond RTOL * |p| over ALL live parameters, in units of the larger lr
PARAM_DEV = {"fixed": [3.6e-8, 2.8e-5, 4.2e-5], "auto": [6.3e-4, 7.7e-4, 7.8e-4, 7.8e-4]}
# ... and of the lagged vector (tau times the live deviation, accumulated)
LAGGED_DEV = {"fixed": [0.0, 6.6e-8, 4.4e-7], "auto": [0.0, 1.5e-7, 1.9e-8, 3.0e-7]}
# ... of the three optimizers' moments after the last update, relative to each vector's largest magnitude: {set: (m, v)}
MOMENT_DEV = {"fixed": {"critic1": (1.6e-6, 1.1e-6), "critic2": (9.7e-7, 9.4e-7), "actor": (3.5e-6, 4.5e-6)},
              "auto": {"critic1": (8.7e-7, 1.2e-6), "critic2": (7.9e-7, 1.3e-6), "actor": (1.2e-6, 2.3e-6)}}
# ... of the four losses and alpha (relative), of alpha_loss (absolute, beyond RTOL * |alpha_loss|), of log alpha (absolute) and of
# log alpha's two Adam moments after the last update (relative: (m, v))
STAT_DEV = {"fixed": 3.4e-6, "auto": 3.8e-6}
ALPHA_LOSS_DEV = {"fixed": 0.0, "auto": 0.0}
LOG_ALPHA_DEV = {"fixed": 0.0, "auto": 2.4e-8}
ALPHA_MOMENT_DEV = {"fixed": (0.0, 0.0), "auto": (4.6e-7, 8.8e-7)}
ALPHA_LOSS_ATOL = 1e-7
WEIGHT_ATOL = 1e-5


def load(tag: str):
    g = np.load(os.path.join(GOLDEN, f"dsac_cnn_{tag}.npz"))
    E, slots, steps, c, h, w, n_act, hidden, batch, n_updates, seed, prioritized = (int(x) for x in g["dims"])
    cd = dict(zip(g["cfg_keys"].tolist(), g["cfg_vals"].tolist()))
    cfg = OS.DSACConfig(gamma=cd["gamma"], tau=cd["tau"], n_step=int(cd["n_step"]), alpha=cd["alpha"], auto_alpha=bool(cd["auto_alpha"]),
                        target_entropy=cd["target_entropy"], log_alpha0=cd["log_alpha0"], actor_lr=cd["actor_lr"],
                        critic_lr=cd["critic_lr"], alpha_lr=cd["alpha_lr"])
    dims = dict(E=E, slots=slots, steps=steps, c=c, h=h, w=w, n_act=n_act, hidden=hidden, batch=batch, n_updates=n_updates, seed=seed,
                prioritized=bool(prioritized))
    bstate = O.BufferState(g["buf_offset"], g["buf_last_index"], g["buf_lengths"], g["buf_insertion"],
                           g["rew"], g["terminated"], g["truncated"])
    return g, dims, cfg, bstate


def is_weight(g, d, u: int):
    """The importance weights of update u (float32 [B]) or None for the plain buffer."""
    return g[f"u{u}_is_weight"].astype(np.float32) if d["prioritized"] else None


def lr_of(cfg) -> float:
    return max(cfg.actor_lr, cfg.critic_lr)


def check_stats(got5, g, u: int, cfg, n_act: int) -> None:
    """{actor_loss, critic1_loss, critic2_loss, alpha, alpha_loss} of update u against the fixture."""
    ref = g[f"u{u}_stats"]
    print(f"  u{u} stats", [float(x) for x in got5], ref.tolist())
    for i, name in enumerate(OS.STAT_NAMES[:4]):
        np.testing.assert_allclose(float(got5[i]), ref[i], rtol=RTOL, err_msg=name)
    np.testing.assert_allclose(float(got5[4]), ref[4], rtol=RTOL, atol=ALPHA_LOSS_ATOL, err_msg="alpha_loss")


def check_weight(got, g, u: int) -> None:
    ref = g[f"u{u}_weight_out"]
    np.testing.assert_allclose(np.asarray(got, np.float64), ref, rtol=RTOL, atol=WEIGHT_ATOL, err_msg="batch.weight")


def check_params(got, ref, dev: float, lr: float, what: str) -> None:
    """Sampled parameters against the fixture: rtol = 1e-5 with atol = 0.02 lr, widened only where the float32 oracle's own
    deviation from float64 (`dev`, in units of lr) exceeds it, to FACTOR times that deviation."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = np.abs(got - ref) - RTOL * np.abs(ref)
    print(f"  {what}: largest deviation beyond rtol {max(diff.max(), 0.0) / lr:.3g} lr (bar {max(FACTOR * dev, ATOL_LR):.3g} lr)")
    assert diff.max() <= max(FACTOR * dev, ATOL_LR) * lr, (what, diff.max() / lr)


def check_first_step(got, ref, lr: float, what: str) -> None:
    """Parameters after the FIRST Adam step from zero moments on synthetic inputs: test_gpu_bcq.py's bar for exactly that --
    fewer than 1e-4 of the elements beyond rtol = 1e-5 with atol = 0.02 lr, none beyond 2 lr.  The first step moves an element
    by lr * g / (|g| + eps): where |g| is of the order of eps = 1e-8 the step is anywhere in [-lr, lr] in either evaluation."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = np.abs(got - ref)
    bad = diff > RTOL * np.abs(ref) + ATOL_LR * lr
    print(f"  {what}: {bad.mean():.3g} of the elements beyond the bar, largest deviation {diff.max() / lr:.3g} lr")
    assert bad.mean() < 1e-4 and diff.max() <= 2 * lr, (what, bad.mean(), diff.max() / lr)


def moment_bars(tag: str, which: str) -> tuple[float, float]:
    """-> the bars on (m, v) relative to each vector's largest magnitude: 1e-5 / 2e-5, or FACTOR * MOMENT_DEV if larger."""
    m, v = MOMENT_DEV[tag][which]
    return max(1e-5, FACTOR * m), max(2e-5, FACTOR * v)


def check_moments(m, v, g, tag: str, which: str) -> None:
    m_ref, v_ref = g[f"adam_{which}_m_strided"], g[f"adam_{which}_v_strided"]
    bm, bv = moment_bars(tag, which)
    em, ev = np.abs(m - m_ref).max() / np.abs(m_ref).max(), np.abs(v - v_ref).max() / np.abs(v_ref).max()
    print(f"  {tag} {which} moments: m {em:.3g} (bar {bm:.3g}), v {ev:.3g} (bar {bv:.3g})")
    assert em <= bm and ev <= bv, (which, em, ev)


def check_alpha_moments(m: float, v: float, g) -> None:
    """log alpha's two Adam moments against the fixture: the moment bars, relative (a scalar is its own scale)."""
    m_ref, v_ref = float(g["alpha_adam"][0]), float(g["alpha_adam"][1])
    print(f"  log alpha moments: m {abs(m - m_ref) / abs(m_ref):.3g}, v {abs(v - v_ref) / abs(v_ref):.3g}")
    assert abs(m - m_ref) <= 1e-5 * abs(m_ref) and abs(v - v_ref) <= 2e-5 * abs(v_ref), (m, m_ref, v, v_ref)
