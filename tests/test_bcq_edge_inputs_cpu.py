"""CPU: the preconditions of tests/test_gpu_bcq_edges.py, checked in float64 without a GPU -- the equality row really is exact,
the +-1 Huber rows really are exact, the float32 formula of the oracle stays within the floor of the bars on every case (the
floor is of the size of a float32 evaluation's error, not a loophole) -- and the argument validation of the new entry points
on a library that never touches a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bcq_edge_cases as BE
from tests import oracle_bcq as OB


def test_the_threshold_rows_are_exact():
    lt = np.float32(np.log(0.3))
    assert BE.LT == float(lt) and float(lt) < np.log(0.3)            # below the double value: a double comparison would mask it
    q, lg, tau, want = BE.ARGMAX_CASES["ratio_equal_to_log_tau_is_not_masked"]
    ratio = np.float32(lg[0][1]) - np.float32(lg[0][0])
    assert ratio == lt and float(ratio) == float(lt) and not ratio < np.float32(tau)
    assert np.float64(ratio) < np.log(0.3)                            # ... and here it is: the same ratio IS below log 0.3 in double
    q, lg, tau, want = BE.ARGMAX_CASES["one_ulp_below_is_masked"]
    below = np.float32(lg[0][1])
    assert below < lt and np.nextafter(below, np.float32(0)) == lt and below - np.float32(0.0) < np.float32(tau)
    assert not np.float32(-200.0) < np.float32(-np.inf)               # a threshold of 0 masks nothing


@pytest.mark.parametrize("name", list(BE.ARGMAX_CASES))
def test_hand_made_actions_agree_with_the_float32_rule_and_the_oracle(name):
    q, lg, tau, want = BE.ARGMAX_CASES[name]
    assert BE.masked_argmax32(q, lg, tau).tolist() == want
    assert OB.masked_argmax(BE.f32(q), BE.f32(lg), tau).tolist() == want


def test_masked_3e38_is_not_minus_flt_max():
    v = np.float32(3e38) - BE.FLT_MAX
    assert v > -BE.FLT_MAX and v < np.float32(-4e37) and np.float32(1.0) - BE.FLT_MAX == -BE.FLT_MAX


@pytest.mark.parametrize("a", BE.A_GRID)
def test_grid_ratios_are_exact_and_clear_of_the_threshold(a):
    for b in BE.B_GRID:
        q, lg, _ = BE.grid_pair(a, b)
        r32 = (lg - lg.max(1, keepdim=True).values).double()
        r64 = lg.double() - lg.double().max(1, keepdim=True).values
        assert torch.equal(r32, r64) and float((r64 - np.log(0.3)).abs().min()) >= 0.04
        act = BE.masked_argmax32(q, lg, BE.LT)
        assert np.array_equal(act, OB.masked_argmax(q, lg, BE.LT).numpy())
        top = torch.where(r64 < BE.LT, torch.full_like(q, -np.inf), q).double().sort(1, descending=True).values
        assert a == 1 or float((top[:, 0] - top[:, 1]).min()) > 1e-4                # no near-tie decides an action


def test_the_delta_rows_are_exact():
    case = BE.delta_case()
    rows = torch.arange(case["B"])
    d32 = case["q"][rows, case["act"]] - case["ret"]
    assert torch.equal(d32.double(), torch.tensor(BE.DELTAS, dtype=torch.float64))       # delta is the listed float32, exactly
    assert BE.ONE_UP > 1.0 > BE.ONE_DOWN and BE.ONE_UP - 1.0 == 2.0 ** -23 and 1.0 - BE.ONE_DOWN == 2.0 ** -24
    ref = BE.loss64(case)
    assert ref["huber"][:3].tolist() == [0.0, 0.5, 0.5] and ref["dq"].abs().sum(1)[:3].tolist() == [0.0, 1 / 9, 1 / 9]
    assert set(case["act"].tolist()) == {0, case["A"] - 1}                                # the first and the last action


def test_offset_and_uniform_cases_are_exact():
    for off in (1.0e4, -1.0e4):
        c, c0 = BE.offset_case(off), BE.offset_case(0.0)
        z = c["logits"] - c["logits"].max(1, keepdim=True).values
        assert torch.equal(z, c0["logits"] - c0["logits"].max(1, keepdim=True).values)
    c = BE.uniform_case(0.0)
    ref = BE.loss64(c)
    assert torch.equal(ref["p"], torch.full_like(ref["p"], 0.25))
    assert float(np.float32(np.exp(np.float32(-200.0)))) == 0.0 and np.exp(-200.0) > 0.0


@pytest.mark.parametrize("name", list(BE.all_loss_cases()))
def test_float32_formula_stays_within_the_floor(name):
    """err32 <= 4 eps32 scale on every case and quantity: the floor of the bars is of the size of the float32 formula's error."""
    units = BE.err32_units(BE.reference(BE.all_loss_cases()[name]))
    print(name, {k: round(v, 3) for k, v in units.items()})
    assert max(units.values()) <= 4.0, units


def test_one_action_terms_vanish_in_float64():
    ref = BE.loss64(BE.grid_loss_case(1, 5, theta=0.0))
    assert not ref["nll"].any() and not ref["dlogits"].any()


@pytest.fixture(scope="module")
def lib():
    from tianshou_amd import _lib
    from tianshou_amd.build import build_library

    build_library()
    lib = C.CDLL(_lib.LIB_PATH)
    lib.ts_last_error.restype = C.c_char_p
    return lib


def test_raw_entry_points_validate_before_any_hip_call(lib):
    """ts_bcq_head / ts_bcq_target / ts_bcq_loss: NULLs, B, n_act, log_tau > 0 or NaN, a negative or non-finite penalty fail as
    TS_ERR_INVALID_ARG before a device is touched (the dummy pointers are never dereferenced)."""
    from tianshou_amd import _lib

    d, i64, f64 = C.c_void_p(4096), C.c_int64, C.c_double
    bad = _lib.TS_ERR_INVALID_ARG
    head = lambda q=d, lg=d, B=5, A=3, lt=-1.0, act=d: lib.ts_bcq_head(q, lg, i64(B), i64(A), f64(lt), act, None)      # noqa: E731
    target = lambda q=d, lg=d, qo=d, B=5, A=3, lt=-1.0, out=d: lib.ts_bcq_target(q, lg, qo, i64(B), i64(A), f64(lt), out, None, None)      # noqa: E731
    loss = lambda q=d, lg=d, act=d, ret=d, B=5, A=3, th=0.01, dq=d, dl=d, t=d, l4=d: lib.ts_bcq_loss(      # noqa: E731
        q, lg, act, ret, i64(B), i64(A), f64(th), dq, dl, t, l4, None)
    for kw in (dict(q=None), dict(lg=None), dict(act=None), dict(B=-1), dict(A=0), dict(A=65), dict(lt=1e-9), dict(lt=float("nan")),
               dict(lt=float("inf"))):
        assert head(**kw) == bad, kw
    assert head(B=0, q=None) == 0 and head(B=0, lt=-float("inf")) == 0            # an empty batch is no error; -inf is a threshold of 0
    for kw in (dict(q=None), dict(lg=None), dict(qo=None), dict(out=None), dict(B=-1), dict(A=0), dict(A=65), dict(lt=0.5),
               dict(lt=float("nan"))):
        assert target(**kw) == bad, kw
    for kw in (dict(q=None), dict(lg=None), dict(act=None), dict(ret=None), dict(dq=None), dict(dl=None), dict(t=None), dict(l4=None),
               dict(B=0), dict(B=-2), dict(B=1 << 24), dict(A=0), dict(A=65)):
        assert loss(**kw) == bad, kw
    for th in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        assert loss(th=th) == bad, th
        assert b"imitation_logits_penalty" in lib.ts_last_error()


def test_network_entry_points_validate_before_any_hip_call(lib):
    """ts_bcq_forward / ts_bcq_target_q / ts_bcq_update on a workspace that has never touched a device (ts_workspace_create only
    allocates host memory), and a NULL workspace as TS_ERR_WORKSPACE; ts_bcq_param_count / ts_bcq_layout on the host."""
    from tianshou_amd import _lib
    from tianshou_amd.dqn import DQNHParams

    d, i64, f64 = C.c_void_p(4096), C.c_int64, C.c_double
    bad = _lib.TS_ERR_INVALID_ARG
    ws = C.c_void_p()
    assert lib.ts_workspace_create(C.byref(ws), 0, C.c_size_t(0)) == 0
    hp = DQNHParams(1e-3, 0.9, 0.999, 1e-8, 1.0, 0.0)
    hp_grad = DQNHParams(-1.0, 0.9, 0.999, 1e-8, 1.0, 0.0)

    def fwd(ws=ws, params=d, obs=d, B=5, A=3, lt=-1.0, h=44):
        return lib.ts_bcq_forward(ws, params, i64(2), i64(h), i64(36), i64(A), obs, 1, i64(B), f64(lt), d, d, d, None)

    def tq(ws=ws, params=d, old=d, obs=d, B=5, A=3, lt=-1.0, out=d):
        return lib.ts_bcq_target_q(ws, params, old, i64(2), i64(44), i64(36), i64(A), obs, 1, i64(B), f64(lt), out, None, None)

    def upd(ws=ws, params=d, m=d, v=d, step=1, obs=d, act=d, ret=d, B=5, A=3, hp_=C.byref(hp), th=0.01, l4=d, grad=None):
        return lib.ts_bcq_update(ws, params, m, v, i64(step), i64(2), i64(44), i64(36), i64(A), obs, 1, act, ret, i64(B), hp_,
                                 f64(th), l4, grad, None)

    try:
        assert fwd(ws=None) == tq(ws=None) == upd(ws=None) == _lib.TS_ERR_WORKSPACE
        for kw in (dict(params=None), dict(obs=None), dict(B=-1), dict(A=0), dict(A=65), dict(lt=0.1), dict(lt=float("nan")),
                   dict(h=20)):
            assert fwd(**kw) == bad, kw
        assert fwd(B=0) == 0
        for kw in (dict(params=None), dict(old=None), dict(obs=None), dict(out=None), dict(B=-1), dict(A=65), dict(lt=2.0)):
            assert tq(**kw) == bad, kw
        for kw in (dict(params=None), dict(m=None), dict(v=None), dict(obs=None), dict(act=None), dict(ret=None), dict(hp_=None),
                   dict(l4=None), dict(B=0), dict(step=0), dict(A=0), dict(A=65), dict(hp_=C.byref(hp_grad))):
            assert upd(**kw) == bad, kw
        for th in (-1.0, float("nan"), float("inf")):
            assert upd(th=th) == bad and b"imitation_logits_penalty" in lib.ts_last_error()
    finally:
        lib.ts_workspace_destroy(ws)
    lib.ts_bcq_param_count.restype = C.c_int64
    lib.ts_bcq_param_count.argtypes = [C.c_int64] * 4
    f = 64 * 7 * 7
    assert lib.ts_bcq_param_count(4, 84, 84, 6) == (8 * 8 * 4 + 1) * 32 + 513 * 64 + 577 * 64 + 2 * ((f + 1) * 512 + 513 * 32)
    assert lib.ts_bcq_param_count(4, 84, 84, 65) == -1 and lib.ts_bcq_param_count(4, 20, 84, 6) == -1
    out = (C.c_int64 * 10)()
    assert lib.ts_bcq_layout(i64(4), i64(84), i64(84), i64(33), out) == 0
    assert (out[0], out[1]) == (f, 64) and out[9] - out[8] == (f + 1) * 512 and out[2] - out[9] == 513 * 64
    assert lib.ts_bcq_layout(i64(4), i64(84), i64(84), i64(6), None) == bad
