"""bcq_head_kernel, bcq_target_kernel, bcq_loss_kernel and bcq_mean_kernel of ts_bcq.hip on raw arrays (ts_bcq_head,
ts_bcq_target, ts_bcq_loss), where tests/test_gpu_bcq.py never goes: a ratio exactly at the threshold and one ulp to either
side, a threshold of 0, masked best actions, ties, a masked Q of 3e38; A = 1 .. 64 with and without padding columns, B no
multiple of a workgroup's samples; delta = 0, +-1, +-(1 +- 1 ulp), +-1e6; the first and the last action; logits under a common
offset of +-1e4; a dominated row; theta = 0; one action.

Bars: exact claims are asserted exactly; the rest is per element against float64, |got - ref64| <= 4 err32 + tiny, err32 being
the float32 oracle formula's own error on the same input (tests/bcq_edge_cases.py states the construction, the scales and the
reasoning; tests/test_bcq_edge_inputs_cpu.py checks the preconditions without a GPU)."""
import numpy as np
import pytest
import torch

from tests import bcq_edge_cases as BE
from tests.distq_edge_gpu_common import within

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(BE.ARGMAX_CASES))
def test_hand_made_actions(name):
    from tianshou_amd import bcq as BQ

    q, lg, tau, want = BE.ARGMAX_CASES[name]
    assert BQ.masked_argmax(q, lg, tau).cpu().tolist() == want
    q_old = [[10.0 + a for a in range(len(q[0]))]]
    out, act = BQ.target_select(q, lg, q_old, tau)
    assert act.cpu().tolist() == want and out.cpu().tolist() == [10.0 + want[0]]


@pytest.mark.parametrize("a", BE.A_GRID)
@pytest.mark.parametrize("b", BE.B_GRID)
def test_argmax_and_target_on_the_shape_grid(a, b):
    """Every action equals the float32 rule's, with a threshold and without; the target value is q_old at that action, bit for
    bit; the padding lanes of A = 1, 31, 33 never win."""
    from tianshou_amd import bcq as BQ

    q, lg, q_old = BE.grid_pair(a, b)
    for tau in (BE.LT, -np.inf):
        want = BE.masked_argmax32(q, lg, tau)
        assert np.array_equal(BQ.masked_argmax(q, lg, tau).cpu().numpy(), want)
        out, act = BQ.target_select(q, lg, q_old, tau)
        assert np.array_equal(act.cpu().numpy(), want)
        assert torch.equal(out.cpu(), q_old[torch.arange(b), torch.as_tensor(want)])
    if a > 1:                       # the mask decides somewhere, or the grid would say nothing about it
        assert (BE.masked_argmax32(q, lg, BE.LT) != q.numpy().argmax(1)).any() or b == 1
    # every Q below 0: a zero in a padding lane would win
    neg = -torch.rand(b, a, generator=torch.Generator().manual_seed(3)) - 1.0
    assert np.array_equal(BQ.masked_argmax(neg, lg, -np.inf).cpu().numpy(), neg.numpy().argmax(1))


def run_loss(case):
    from tianshou_amd import bcq as BQ

    out = BQ.loss_terms(case["q"], case["logits"], case["act"], case["ret"], case["theta"], fill=BE.SENTINEL)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check_loss(case, out=None):
    """Per-sample terms, the four losses and both head gradients against float64 within the bars; the padding columns exactly
    0.0; the sentinel gone from every element."""
    a, b = case["A"], case["B"]
    out = run_loss(case) if out is None else out
    ref = BE.reference(case)
    print(f"  A={a} B={b} theta={case['theta']}")
    assert tuple(out["dq"].shape) == tuple(out["dlogits"].shape) == (b, BE.ld_of(a)) and tuple(out["terms"].shape) == (4, b)
    for k, name in enumerate(("delta", "huber", "nll", "sumsq")):
        within(out["terms"][k], ref[name], ref[name + "_bar"], name)
    for k, name in enumerate(("loss", "q_loss", "i_loss", "reg_loss")):
        within(out["losses"][k], ref[name], ref[name + "_bar"], name)
    within(out["dq"][:, :a], ref["dq"], ref["dq_bar"], "dq")
    within(out["dlogits"][:, :a], ref["dlogits"], ref["dlogits_bar"], "dlogits")
    for name in ("dq", "dlogits"):
        assert not out[name][:, a:].any(), name                                       # padding columns: exact zeros
    for v in out.values():
        assert torch.isfinite(v).all() and not (v == BE.SENTINEL).any()
    rows = torch.arange(b)
    other = torch.ones(b, a, dtype=torch.bool)
    other[rows, case["act"]] = False
    assert not out["dq"][:, :a][other].any()                                          # dQ lives in the taken column alone
    return out, ref


@pytest.mark.parametrize("a", BE.A_GRID)
@pytest.mark.parametrize("b", BE.B_GRID)
def test_loss_on_the_shape_grid(a, b):
    check_loss(BE.grid_loss_case(a, b))


def test_huber_at_zero_one_and_beyond():
    """delta = 0: no loss, no gradient; +-1 exactly: 0.5 and +-1 / B exactly; one ulp inside / outside and +-1e6 within the bars,
    the gradient saturated at exactly +-1 / B from 1 on."""
    case = BE.delta_case()
    out, _ = check_loss(case)
    b = case["B"]
    assert torch.equal(out["terms"][0], BE.f32(BE.DELTAS))                           # delta itself: exact
    g = out["dq"][torch.arange(b), case["act"]]
    inv_b = np.float32(1.0) / np.float32(b)
    assert out["terms"][1][:3].tolist() == [0.0, 0.5, 0.5] and g[:3].tolist() == [0.0, float(inv_b), -float(inv_b)]
    for k, d in enumerate(BE.DELTAS):
        if abs(d) >= 1.0:
            assert float(g[k]) == float(np.sign(d) * inv_b), d
        else:
            assert float(g[k]) == float(np.float32(d) / np.float32(b)), d


@pytest.mark.parametrize("offset", [1.0e4, -1.0e4])
def test_common_logit_offset(offset):
    """The max-subtracted log-softmax sees the offset-free integers: nll and the softmax part of the gradient are those of the
    case without the offset, bit for bit (theta = 0 leaves nothing else in the gradient)."""
    out, _ = check_loss(BE.offset_case(offset))
    with0, plain = run_loss(BE.offset_case(offset, theta=0.0)), run_loss(BE.offset_case(0.0, theta=0.0))
    assert torch.equal(with0["terms"][2], plain["terms"][2]) and torch.equal(with0["dlogits"], plain["dlogits"])
    assert float(with0["losses"][2]) == float(plain["losses"][2])


def test_dominated_row():
    out, _ = check_loss(BE.dominated_case())
    assert out["terms"][2].tolist() == [0.0, 200.0]                                   # exp(-200) is 0 in float32
    hot = run_loss(BE.dominated_case(theta=0.0))["dlogits"][:, :2]
    assert hot[0].tolist() == [0.0, 0.0] and hot[1].tolist() == [0.5, -0.5]


def test_theta_zero_leaves_no_regulariser():
    """Equal logits of 1000, A = 4, B = 8: without the regulariser every gradient element is (1/4 - 1{a = act}) / 8 to the bit
    and loss == q_loss + i_loss; reg_loss is still reported; with theta = 0.5 the gradient moves."""
    case = BE.uniform_case(0.0)
    out, _ = check_loss(case)
    a, b = case["A"], case["B"]
    want = (torch.full((b, a), 0.25) - torch.nn.functional.one_hot(case["act"], a)) / 8.0
    assert torch.equal(out["dlogits"][:, :a], want)
    l4 = out["losses"].numpy()
    assert l4[0] == np.float32(l4[1] + l4[2]) and l4[3] == np.float32(1.0e6)
    moved, _ = check_loss(BE.uniform_case(0.5))
    assert not torch.equal(moved["dlogits"], out["dlogits"]) and float(moved["losses"][0]) > float(l4[0])
    check_loss(BE.grid_loss_case(5, 5, theta=0.0))


def test_one_action():
    """A = 1: i_loss is exactly 0.0 and the softmax gradient exactly 0.0; with theta > 0 only the regulariser is left."""
    case = BE.grid_loss_case(1, 5, theta=0.0)
    out, _ = check_loss(case)
    assert not out["terms"][2].any() and float(out["losses"][2]) == 0.0 and not out["dlogits"].any()
    check_loss(BE.grid_loss_case(1, 5, theta=0.5))


def test_act_out_of_range_is_clamped_and_nothing_leaves_the_row():
    case = BE.grid_loss_case(3, 5)
    lo, hi = dict(case, act=torch.full((5,), -4)), dict(case, act=torch.full((5,), 99))
    for c, a in ((lo, 0), (hi, 2)):
        got, want = run_loss(c), run_loss(dict(case, act=torch.full((5,), a)))
        assert all(torch.equal(got[k], want[k]) for k in got)


def test_reruns_are_bit_identical():
    case = BE.grid_loss_case(33, 37)
    a, b = run_loss(case), run_loss(case)
    assert all(torch.equal(a[k], b[k]) for k in a)
