"""CPU: the inputs of tests/test_gpu_bc_edges.py are what they claim to be and the float32 torch formulas stay inside the bars
of tests/bc_edge_cases.py on every case, so the GPU test cannot hide behind them.  No GPU, no kernel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bc_edge_cases as BE
from tianshou_amd import _lib
from tianshou_amd import bc as BC


def test_grids_cover_the_engine_limits():
    assert max(BE.CE_A_GRID) == BC.MAX_ACT and max(BE.MSE_A_GRID) == BC.MAX_ACT_DIM == BE.HEAD_PITCH
    assert {1, 5, 37, 257} == set(BE.CE_B_GRID) and {1, 5, 37, 1025} == set(BE.MSE_B_GRID)
    assert len(BE.all_ce_cases()) == 7 + 24 and len(BE.all_mse_cases()) == 2 * (3 + 20)


@pytest.mark.parametrize("name", list(BE.all_ce_cases()))
def test_float32_cross_entropy_stays_within_the_floor(name):
    """err32 <= 4 eps32 scale on every case: the floor of the bars is of the size of the float32 formula's own error."""
    units = BE.err32_units("ce", BE.reference("ce", BE.all_ce_cases()[name]))
    print(name, {k: round(v, 3) for k, v in units.items()})
    assert max(units.values()) <= 4.0, units


@pytest.mark.parametrize("name", list(BE.all_mse_cases()))
def test_float32_mse_stays_within_the_bar(name):
    """The float32 torch formula is inside the bar 4 err32 + 4 eps32 scale on every element, and its own error is of the floor's
    size: the loss within 4 eps32 scale; dhead within 16 eps32 scale, float32's worst case written down from the formula
    2 (a - a*) / (B A) * max_action * (1 - t^2): |a - a*| <= 2 max(|a|, |a*|), so the value is at most 4 scale (1 - t^2); 1 - t^2
    carries an absolute error of up to 2 |t| ulp(t) + eps32 / 4 <= 1.25 eps32 from a tanh good to one ulp and the rounding of
    t^2, the five multiplications and the subtraction a - a* another 3 eps32 relative: 4 (1.25 + 3) eps32 scale at the outside.
    Elements beyond the floor are carried by the bar's err32 term on the GPU side."""
    ref = BE.reference("mse", BE.all_mse_cases()[name])
    units = BE.err32_units("mse", ref)
    print(name, {k: round(v, 3) for k, v in units.items()})
    for k in BE.quantities("mse"):
        assert bool((ref[k + "_err32"] <= ref[k + "_bar"]).all()), k
    assert units["loss"] <= 4.0 and units["dhead"] <= 16.0, units


def test_one_action_terms_vanish():
    for b in BE.CE_B_GRID:
        case = BE.ce_grid_case(1, b)
        r64, r32 = BE.ce64(case), BE.ce32(case)
        assert not r64["nll"].any() and not r64["dlogits"].any()
        assert float(r32["loss"]) == 0.0 and not r32["dlogits"].any()


def test_offsets_are_exact_and_shift_invariant():
    plain = BE.ce_offset_case(0.0)
    z0 = plain["logits"] - plain["logits"].max(1, keepdim=True).values
    for off in (80.0, -80.0, 1.0e4):
        c = BE.ce_offset_case(off)
        assert torch.equal(c["logits"] - c["logits"].max(1, keepdim=True).values, z0)         # the offset-free integers, exactly
        assert torch.equal(c["logits"].double() - off, plain["logits"].double())
        a, b = BE.ce32(c), BE.ce32(plain)
        assert torch.equal(a["dlogits"], b["dlogits"]) and float(a["loss"]) == float(b["loss"])
        assert torch.isfinite(a["dlogits"]).all() and np.isfinite(float(a["loss"]))
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.exp(np.float32(1.0e4)))                                    # without the max: overflow
    assert float(np.exp(np.float32(-80.0) - np.float32(3.0) - np.float32(80.0))) < 1e-30


def test_spread_rows_underflow_in_float32_only():
    case = BE.ce_spread_case()
    z = case["logits"] - case["logits"].max(1, keepdim=True).values
    losing = z < 0
    assert float(z[losing].max()) < -104.0 and int((~losing).sum()) == case["B"]
    assert not torch.exp(z)[losing].any() and bool((torch.exp(z.double())[losing] > 0).all())
    r32 = BE.ce32(case)
    b = case["B"]
    hot = torch.nn.functional.one_hot(case["act"], case["A"]).bool()
    taken = r32["dlogits"][hot]
    assert not r32["dlogits"][losing & ~hot].any()                                           # the losers' gradient: exactly 0
    assert taken.tolist() == [0.0, 0.0, -1.0 / b, -1.0 / b]                                  # (p - 1) / B with p = 1 and p = 0
    assert BE.ce64(case)["nll"].tolist()[:2] == pytest.approx([0.0, 0.0], abs=1e-40)


def test_ties_are_exact():
    case = BE.ce_tie_case()
    assert torch.equal(BE.ce64(case)["p"], torch.full((8, 4), 0.25, dtype=torch.float64))
    want = (torch.full((8, 4), 0.25) - torch.nn.functional.one_hot(case["act"], 4)) / 8.0
    assert torch.equal(BE.ce32(case)["dlogits"], want)
    p = BE.ce64(BE.ce_partial_tie_case())["p"]
    assert torch.equal(p[:, 0], p[:, 1].clone()) or float((p[:3, 0] - p[:3, 1]).abs().max()) == 0.0


def test_extreme_targets_are_the_largest_and_the_smallest_logit():
    case = BE.ce_extreme_target_case()
    lg, act = case["logits"], case["act"]
    for k in range(case["B"]):
        assert int(act[k]) == int(lg[k].argmax() if k % 2 == 0 else lg[k].argmin())


def test_tanh_saturates_and_on_target_rows_are_exact():
    assert float(torch.tanh(torch.tensor(20.0))) == 1.0 and float(torch.tanh(torch.tensor(-20.0))) == -1.0
    assert np.tanh(20.0) < 1.0 or np.tanh(np.float64(20.0)) == 1.0          # (float64 keeps 1 - 2 exp(-40) apart from 1 or not: no claim)
    for m in BE.MAX_ACTIONS:
        sat = BE.mse32(BE.mse_saturated_case(m))
        assert not sat["dhead"].any() and np.isfinite(float(sat["loss"])) and float(sat["loss"]) > 0.0
        on = BE.mse_on_target_case(m)
        assert set(on["act_data"].unique().tolist()) == {0.0, m, -m}
        r = BE.mse32(on)
        assert float(r["loss"]) == 0.0 and not r["dhead"].any()
        r64 = BE.mse64(BE.mse_zero_head_case(m))
        case = BE.mse_zero_head_case(m)
        want = -2.0 * case["act_data"].double() * m / (case["B"] * case["A"])
        assert torch.equal(r64["dhead"], want)


def test_padding_columns_of_the_head_block_hold_draws():
    case = BE.mse_grid_case(6, 5, 2.5)
    assert tuple(case["block"].shape) == (5, 32) and torch.equal(case["block"][:, :6], case["head"])
    assert bool((case["block"][:, 6:].abs() > 0).all())
    assert float(case["act_data"].abs().max()) > 1.0


def test_argument_validation_without_gpu():
    """Refusals come before any HIP call: the dummy pointers are never dereferenced."""
    lib = C.CDLL(_lib.LIB_PATH)
    i64, f64, p = C.c_int64, C.c_double, C.c_void_p(4096)

    def ce(lg=p, ld=8, act=p, B=4, A=8, loss=p, dl=p):
        return lib.ts_bc_ce_loss(lg, i64(ld), act, i64(B), i64(A), loss, dl, None)

    def mse(h=p, a=p, B=4, A=6, m=1.0, loss=p, dh=p):
        return lib.ts_bc_mse_loss(h, a, i64(B), i64(A), f64(m), loss, dh, None)

    bad = _lib.TS_ERR_INVALID_ARG
    for kw in (dict(A=0), dict(A=65), dict(B=0), dict(ld=7), dict(lg=None), dict(act=None), dict(loss=None), dict(dl=None)):
        assert ce(**kw) == bad, kw
    for kw in (dict(A=0), dict(B=0), dict(h=None), dict(a=None), dict(loss=None), dict(dh=None)):
        assert mse(**kw) == bad, kw
    assert mse(A=33) == _lib.TS_ERR_UNSUPPORTED
    ws = C.c_void_p()
    assert lib.ts_workspace_create(C.byref(ws), 0, C.c_size_t(0)) == 0
    try:
        from tianshou_amd import dqn, sac

        hp = dqn.DQNHParams(1e-3, 0.9, 0.999, 1e-8, -1.0, 0.0)

        def dq(ws_=ws, B=4, A=6, step=1, h=84, act=p):
            return lib.ts_bc_dqnet_update(ws_, p, p, p, i64(step), i64(4), i64(h), i64(84), i64(A), p, 1, act, i64(B), C.byref(hp),
                                          p, None, None)

        def mlp(ws_=ws, mode=0, n_out=6, B=4, hidden=64, act=p):
            trunk = sac.MLPTrunk(hidden, 2, "relu", 0.0)
            return lib.ts_bc_mlp_update(ws_, p, p, p, i64(1), p, act, i64(B), i64(8), i64(n_out), C.byref(trunk), C.c_int(mode),
                                        f64(1.0), f64(1e-3), f64(0.9), f64(0.999), f64(1e-8), f64(0.0), p, None, None)

        assert dq(ws_=None) == mlp(ws_=None) == _lib.TS_ERR_WORKSPACE
        for kw in (dict(B=0), dict(A=0), dict(A=65), dict(step=0), dict(h=20), dict(act=None)):
            assert dq(**kw) == bad, kw
        for kw in (dict(mode=2), dict(mode=0, n_out=1), dict(mode=0, n_out=65), dict(mode=1, n_out=0), dict(B=0), dict(hidden=100),
                   dict(act=None)):
            assert mlp(**kw) == bad, kw
        assert mlp(mode=1, n_out=33) == _lib.TS_ERR_UNSUPPORTED
    finally:
        lib.ts_workspace_destroy(ws)
