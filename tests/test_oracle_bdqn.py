"""CPU: tests/oracle_bdqn.py against the reference's recorded BDQN runs (tests/golden/bdqn_double.npz: double Q-learning with a
lagged network synchronised inside the run, Adam, one hidden layer in value and branches; tests/golden/bdqn_per.npz: no target
network, prioritized buffer, RMSprop, tanh, heads directly on the trunk), in float32 and in float64.

Measured here (float32 oracle against the float64 oracle, largest over both fixtures and all three updates; the tolerance the
GPU tests use in brackets -- every distance is below half of it):
    returns   |diff| <= 0.013 (rtol 1e-5 |ref| + atol 2e-6)      loss   rel 1.1e-7  [1e-5]      priorities  4.0e-8 max|td| D  [1e-5 max|td| D]
    parameters: largest |diff| / (atol 0.02 lr + rtol 1e-5 |ref|) = 0.003      moments rel 7.0e-6 (entries above 1e-3 of the largest)  [1e-3]
`test_float32_oracle_distance` asserts the halves.
"""
import numpy as np
import pytest
import torch

from tests import bdqn_common as BC
from tests import oracle_bdqn as OB


@pytest.fixture(scope="module", params=BC.TAGS)
def runs(request):
    g = BC.load(request.param)
    return g, BC.oracle_run(g, torch.float32), BC.oracle_run(g, torch.float64)


def test_fixture_layout(runs):
    g = runs[0]
    dims = BC.dims_of(g)
    assert list(OB.shapes(dims)) == OB.state_keys(dims)
    for k, shp in OB.shapes(dims).items():
        assert g["init_" + k].shape == shp
    for u in range(BC.n_updates(g)):
        assert g[f"u{u}_end"].any() and not g[f"u{u}_end"].all()
        assert g[f"u{u}_returns"].shape == g[f"u{u}_indices"].shape == g[f"u{u}_weight_out"].shape
    end = g["done"].copy()
    end[g["unfinished"]] = True
    assert np.array_equal(end[g["u0_indices"]], g["u0_end"]) and len(g["unfinished"]) > 0
    assert (g["truncated"] & ~g["terminated"]).any() and g["terminated"].any()


@pytest.mark.parametrize("which", [1, 2], ids=["float32", "float64"])
def test_oracle_reproduces_the_recorded_run(runs, which):
    g = runs[0]
    agent, steps = runs[which]
    lr = BC.cfg_of(g)["lr"]
    for u, s in enumerate(steps):
        np.testing.assert_allclose(s["ret"], g[f"u{u}_returns"], rtol=BC.RTOL, atol=BC.Q_ATOL)
        np.testing.assert_allclose(s["loss"], g[f"u{u}_loss"], rtol=BC.RTOL)
        np.testing.assert_allclose(s["prio"], g[f"u{u}_weight_out"], rtol=BC.RTOL, atol=BC.prio_atol(g, u))
        np.testing.assert_allclose(s["params"][::BC.STRIDE], g[f"u{u}_params_strided"], rtol=BC.REC_RTOL, atol=0.02 * lr)
        if s["old"] is not None:
            np.testing.assert_allclose(s["old"][::BC.STRIDE], g[f"u{u}_old_strided"], rtol=BC.REC_RTOL, atol=0.02 * lr)
        if f"u{u}_tree_after" in g:
            np.testing.assert_allclose(BC.expected_tree(g, u, s["prio"]), g[f"u{u}_tree_after"], rtol=1e-5, atol=1e-9)
    m, v = (x.numpy() for x in agent.moments())
    ref_v = g["moment_v_strided"]
    np.testing.assert_allclose(v[::BC.STRIDE], ref_v, rtol=BC.MOM_RTOL, atol=1e-6 * float(ref_v.max()))
    if "moment_m_strided" in g:
        ref_m = g["moment_m_strided"]
        np.testing.assert_allclose(m[::BC.STRIDE], ref_m, rtol=BC.MOM_RTOL, atol=1e-6 * float(np.abs(ref_m).max()))
    assert agent.iter == int(g["iter"]) == BC.n_updates(g)


def test_lagged_sync_falls_inside_the_double_run():
    """target_update_freq = 2: synchronised at the start of updates 0 and 2 -- after update 1 the lagged network still holds the
    INITIAL parameters, after update 2 the parameters update 1 left."""
    g = BC.load("double")
    init = torch.cat([torch.as_tensor(g["init_" + k]).reshape(-1) for k in OB.state_keys(BC.dims_of(g))]).numpy()[::BC.STRIDE]
    assert np.array_equal(g["u0_old_strided"], init) and np.array_equal(g["u1_old_strided"], init)
    assert np.array_equal(g["u2_old_strided"], g["u1_params_strided"]) and not np.array_equal(g["u2_old_strided"], init)


def test_float32_oracle_distance(runs):
    """The float32 oracle stays within HALF of every tolerance of the float64 one (figures in the module docstring)."""
    g, (a32, s32), (a64, s64) = runs
    lr = BC.cfg_of(g)["lr"]
    for u, (x, y) in enumerate(zip(s32, s64)):
        np.testing.assert_allclose(x["ret"], y["ret"], rtol=BC.RTOL / 2, atol=BC.Q_ATOL / 2)
        np.testing.assert_allclose(x["loss"], y["loss"], rtol=BC.RTOL / 2)
        np.testing.assert_allclose(x["prio"], y["prio"], rtol=BC.RTOL / 2, atol=BC.prio_atol(g, u) / 2)
        np.testing.assert_allclose(x["params"], y["params"], rtol=BC.PAR_RTOL / 2, atol=0.01 * lr)
    for x, y in zip(a32.moments(), a64.moments()):
        x, y = x.numpy(), y.numpy()
        np.testing.assert_allclose(x, y, rtol=BC.MOM_RTOL / 2, atol=1e-6 * float(np.abs(y).max()) / 2 + 1e-30)
