"""bc_ce_kernel and bc_mse_kernel of ts_sac.hip on raw arrays (ts_bc_ce_loss, ts_bc_mse_loss), where tests/test_gpu_bc.py never
goes: A = 1 .. 64 with and without padding columns, B = 1 .. 257 / 1025 (no multiple of a workgroup's rows, more than one pass of
the loss workgroup); one action; a common offset of +-80 and 1e4; a spread above 104; exact ties; the target on the largest and
on the smallest logit; head = +-20 and 0; a* = a; max_action 1 and 2.5; padding columns, a sentinel in every output, a guard
region behind every output, an out-of-range action, bit-identical reruns.

Bars: exact claims are asserted exactly; the rest is per element against float64, |got - ref64| <= 4 err32 + 4 eps32 scale, err32
being the float32 torch formula's own error on the same input (tests/bc_edge_cases.py states the construction, the scales and the
reasoning; tests/test_bc_edge_inputs_cpu.py checks the preconditions without a GPU)."""
import numpy as np
import pytest
import torch

from tests import bc_edge_cases as BE
from tests.distq_edge_gpu_common import within

pytestmark = pytest.mark.gpu


def _guarded(n: int):
    """A sentinel-filled device buffer of n floats followed by a guard region -> (whole buffer, view of the n floats)."""
    buf = torch.full((n + BE.GUARD,), BE.SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[:n]


def run_ce(case, pad: bool = True):
    """-> (loss float32[], dlogits [B, ld]) on the host; ld = A rounded up to 32 (`pad`) or A itself.  The outputs start as
    sentinels and end in a guard region that must come back untouched."""
    from tianshou_amd import bc as BC

    a, b = case["A"], case["B"]
    ld = BE.ld_of(a) if pad else a
    lg = torch.full((b, ld), 3.0e4, dtype=torch.float32)          # padding columns: a value that would own the softmax
    lg[:, :a] = case["logits"]
    loss_buf, loss = _guarded(1)
    d_buf, d = _guarded(b * ld)
    BC.ce_loss_into(lg.cuda(), case["act"].cuda(), a, loss, d.view(b, ld))
    torch.cuda.synchronize()
    for buf, n in ((loss_buf, 1), (d_buf, b * ld)):
        assert bool((buf[n:] == BE.SENTINEL).all()), "guard region written"
    return loss.cpu()[0], d.view(b, ld).cpu()


def check_ce(case, pad: bool = True):
    a = case["A"]
    loss, d = run_ce(case, pad)
    ref = BE.reference("ce", case)
    print(f"  A={a} B={case['B']} pad={pad}")
    within(loss, ref["loss"], ref["loss_bar"], "loss")
    within(d[:, :a], ref["dlogits"], ref["dlogits_bar"], "dlogits")
    assert not d[:, a:].any()                                                        # padding columns: exact zeros
    assert torch.isfinite(d).all() and not (d[:, :a] == BE.SENTINEL).any() and float(loss) != BE.SENTINEL
    return loss, d, ref


@pytest.mark.parametrize("a", BE.CE_A_GRID)
@pytest.mark.parametrize("b", BE.CE_B_GRID)
def test_cross_entropy_on_the_shape_grid(a, b):
    check_ce(BE.ce_grid_case(a, b))
    if a % 32:
        check_ce(BE.ce_grid_case(a, b), pad=False)                                   # row pitch = A: no padding columns at all


def test_one_action_is_exactly_zero():
    for b in BE.CE_B_GRID:
        loss, d, _ = check_ce(BE.ce_grid_case(1, b))
        assert float(loss) == 0.0 and not d.any()


@pytest.mark.parametrize("offset", [80.0, -80.0, 1.0e4])
def test_common_logit_offset(offset):
    """The max-subtracted softmax sees the offset-free integers: loss and gradient are those of the case without the offset,
    bit for bit, and nothing overflows."""
    loss, d, _ = check_ce(BE.ce_offset_case(offset))
    loss0, d0 = run_ce(BE.ce_offset_case(0.0))
    assert float(loss) == float(loss0) and torch.equal(d, d0)


def test_spread_above_104():
    case = BE.ce_spread_case()
    loss, d, _ = check_ce(case)
    b, a = case["B"], case["A"]
    z = case["logits"] - case["logits"].max(1, keepdim=True).values
    hot = torch.nn.functional.one_hot(case["act"], a).bool()
    assert not d[:, :a][(z < 0) & ~hot].any()                                        # the losers: exactly 0
    assert d[:, :a][hot].tolist() == [0.0, 0.0, -1.0 / b, -1.0 / b]                  # (p - 1) / B with p = 1 and p = 0
    assert float(loss) == float(np.float32(np.float32(105.0) + np.float32(203.0)) / np.float32(b))


def test_exact_ties():
    case = BE.ce_tie_case()
    loss, d, _ = check_ce(case)
    want = (torch.full((8, 4), 0.25) - torch.nn.functional.one_hot(case["act"], 4)) / 8.0
    assert torch.equal(d[:, :4], want)
    _, d, _ = check_ce(BE.ce_partial_tie_case())
    assert float(d[2, 0]) == float(d[2, 1]) and float(d[0, 0]) == float(d[1, 1]) and float(d[0, 1]) == float(d[1, 0])


def test_target_on_the_largest_and_the_smallest_logit():
    check_ce(BE.ce_extreme_target_case())


def test_act_out_of_range_gives_nan_in_its_row_and_touches_nothing_else():
    """Rows 1 (act = -4) and 3 (act = A) are NaN, the loss is NaN, every other row is the in-range case's bit for bit; the guard
    regions are checked by run_ce.  No fault is provoked: the action is compared and range-checked, never used as an index."""
    case = BE.ce_grid_case(5, 6)
    act = case["act"].clone()
    act[1], act[3] = -4, 5
    loss, d = run_ce(dict(case, act=act))
    _, d0 = run_ce(case)
    assert np.isnan(float(loss))
    for r in range(6):
        if r in (1, 3):
            assert torch.isnan(d[r, :5]).all() and not d[r, 5:].any()
        else:
            assert torch.equal(d[r], d0[r])


def test_cross_entropy_reruns_are_bit_identical():
    case = BE.ce_grid_case(33, 257)
    (l1, d1), (l2, d2) = run_ce(case), run_ce(case)
    assert float(l1) == float(l2) and torch.equal(d1, d2)


def run_mse(case):
    from tianshou_amd import bc as BC

    b = case["B"]
    loss_buf, loss = _guarded(1)
    d_buf, d = _guarded(b * BE.HEAD_PITCH)
    BC.mse_loss_into(case["block"].cuda(), case["act_data"].cuda(), case["max_action"], loss, d.view(b, BE.HEAD_PITCH))
    torch.cuda.synchronize()
    for buf, n in ((loss_buf, 1), (d_buf, b * BE.HEAD_PITCH)):
        assert bool((buf[n:] == BE.SENTINEL).all()), "guard region written"
    return loss.cpu()[0], d.view(b, BE.HEAD_PITCH).cpu()


def check_mse(case):
    a = case["A"]
    loss, d = run_mse(case)
    ref = BE.reference("mse", case)
    print(f"  A={a} B={case['B']} max_action={case['max_action']}")
    within(loss, ref["loss"], ref["loss_bar"], "loss")
    within(d[:, :a], ref["dhead"], ref["dhead_bar"], "dhead")
    assert not d[:, a:].any()                                                        # padding columns: exact zeros
    assert torch.isfinite(d).all() and not (d[:, :a] == BE.SENTINEL).any() and float(loss) != BE.SENTINEL
    return loss, d


@pytest.mark.parametrize("m", BE.MAX_ACTIONS)
@pytest.mark.parametrize("a", BE.MSE_A_GRID)
@pytest.mark.parametrize("b", BE.MSE_B_GRID)
def test_mse_on_the_shape_grid(a, b, m):
    check_mse(BE.mse_grid_case(a, b, m))


@pytest.mark.parametrize("m", BE.MAX_ACTIONS)
def test_mse_saturated_zero_and_on_target_heads(m):
    loss, d = check_mse(BE.mse_saturated_case(m))
    assert not d.any() and np.isfinite(float(loss)) and float(loss) > 0.0            # tanh(+-20) = +-1: no gradient at all
    case = BE.mse_zero_head_case(m)
    loss, d = check_mse(case)
    assert float(d[0, 3]) == 0.0 and float(d[0, 2]) < 0.0
    loss, d = check_mse(BE.mse_on_target_case(m))
    assert float(loss) == 0.0 and not d.any()                                         # a* = a as the kernel rounds it


def test_mse_reruns_are_bit_identical():
    case = BE.mse_grid_case(17, 1025, 2.5)
    (l1, d1), (l2, d2) = run_mse(case), run_mse(case)
    assert float(l1) == float(l2) and torch.equal(d1, d2)


def test_head_width_beyond_the_limit_is_refused():
    from tianshou_amd import _lib
    from tianshou_amd import bc as BC

    head = torch.zeros(2, 32, device="cuda")
    with pytest.raises(_lib.EngineError) as e:
        BC.mse_loss(head, torch.zeros(2, 33, device="cuda"))
    assert e.value.code == _lib.TS_ERR_UNSUPPORTED
    with pytest.raises(_lib.EngineError):
        BC.ce_loss(torch.zeros(2, 96, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), 65)
