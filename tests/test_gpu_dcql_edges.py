"""cql_loss_kernel and cql_mean_kernel of ts_distq.hip where tests/test_gpu_dcql.py never goes: exact quantiles (zeroed head
weights, tests/distq_edge_cases.py), one action, tied actions, a dominated row, a common offset of +-1e6, the first and the last
action, and the shape limits N = 2 .. 256, A = 1 .. 64, B = 1.  `update_with_batch(apply=False, grad_out=)` returns the gradient:
with zero head weights its bias row is the column sum of the kernel's d_head and everything below the head is exactly zero.

Bars: exact claims are asserted exactly; the rest is per element against float64, |got - ref64| <= 4 err32 + tiny, err32 being
the float32 oracle formula's own error on the same input (tests/dcql_edge_cases.py states the construction, the scales and the
reasoning; tests/test_dcql_edge_inputs_cpu.py checks the preconditions without a GPU)."""
import math

import pytest
import torch

from oracle import oracle_dqn as OD
from tests import dcql_edge_cases as CE
from tests import distq_edge_cases as E
from tests.distq_edge_gpu_common import SENTINEL, dev_obs, within

pytestmark = pytest.mark.gpu


def _flat(case):
    from tianshou_amd import distq as Q

    p = E.edge_params(case["A"], case["N"], case["rows"])
    return Q.flat_from_torch([p[k] for k in OD.PARAM_ORDER], E.C, E.H, E.W, case["A"], case["N"])


def run_update(case, weight="case", mqw=None, qrdqn=False):
    """One gradient-only update on the case's edge network -> dict(losses [3], prio [B], head [513, ld], below); `qrdqn`: the
    QRDQN engine on the same inputs (losses = [loss])."""
    from tianshou_amd import dcql as CQ
    from tianshou_amd import distq as Q

    A, N = case["A"], case["N"]
    if qrdqn:
        eng = Q.DistQEngine(E.C, E.H, E.W, A, _flat(case), Q.DistQConfig(kind="qr", n_atoms=N))
    else:
        cfg = CQ.DiscreteCQLConfig(n_atoms=N, min_q_weight=case["mqw"] if mqw is None else mqw)
        eng = CQ.DiscreteCQLEngine(E.C, E.H, E.W, A, _flat(case), cfg)
    w = case["weight"] if isinstance(weight, str) else weight
    grad = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
    losses, prio = eng.update_with_batch(dev_obs(case["obs"]), case["act"], case["ret"], w, grad_out=grad, apply=False)
    torch.cuda.synchronize()
    ld = E.head_width(A, N)
    g = grad.cpu()
    return dict(losses=losses.cpu(), prio=prio.cpu(), head=g[-513 * ld:].reshape(513, ld), below=g[:-513 * ld])


def check_update(case, out=None, weight="case"):
    """prio / qr_loss / cql_loss / loss / the bias-row gradient of EVERY action against float64 within the bars; the padding
    columns and every gradient below the head exactly 0.0; the sentinel is gone from every element."""
    A, N = case["A"], case["N"]
    if not isinstance(weight, str):
        case = dict(case, weight=weight)
    out = run_update(case) if out is None else out
    ref = CE.reference(case)
    print(f"  A={A} N={N} B={case['B']}")
    within(out["prio"], ref["prio"], ref["prio_bar"], "prio")
    within(out["losses"][1], ref["qr_loss"], ref["qr_loss_bar"], "qr_loss")
    within(out["losses"][2], ref["cql_loss"], ref["cql_loss_bar"], "cql_loss")
    within(out["losses"][0], ref["loss"], ref["loss_bar"], "loss")
    within(out["head"][512, :A * N], ref["gbias"], ref["gbias_bar"], "bias gradient")
    assert torch.isfinite(out["head"]).all() and not out["below"].any()                # zero head weights pass nothing down
    assert not out["head"][:, A * N:].any()                                           # padding columns
    assert not (out["head"] == SENTINEL).any()
    return out, ref


def test_one_action_has_no_cql_term_and_qrdqns_gradient():
    """A = 1: logsumexp(q) - q is exactly 0.0, softmax - 1 is exactly 0.0, so the head gradient is QRDQN's bit for bit."""
    for N in (2, 65, 256):
        case = CE.grid_case(1, N, 5)
        out, _ = check_update(case)
        qr = run_update(case, qrdqn=True)
        assert float(out["losses"][2]) == 0.0 and float(out["losses"][0]) == float(out["losses"][1]) == float(qr["losses"][0])
        assert torch.equal(out["head"], qr["head"]) and torch.equal(out["prio"], qr["prio"])


@pytest.mark.parametrize("mixed", [False, True])
def test_tied_actions_share_the_softmax_evenly(mixed):
    """Every q_a is the same float32: p_a = 1 / A, cql_b = log A.  With act = 0 everywhere the columns of all other actions
    carry min_q_weight / (N A) in the bias row (B samples of min_q_weight / (B N A) each)."""
    case = CE.tied_case(act=torch.tensor([0, 4, 2, 4, 0, 1])) if mixed else CE.tied_case()
    A, N = case["A"], case["N"]
    out, ref = check_update(case)
    assert abs(float(ref["cql_loss"]) - math.log(A)) <= 1e-14
    if not mixed:
        want = torch.full((A - 1, N), case["mqw"] / (N * A), dtype=torch.float64)
        assert float((ref["gbias"][1:] - want).abs().max()) <= 1e-14
        within(out["head"][512, N:A * N], want, ref["gbias_bar"][1:].expand(A - 1, N), "untaken columns")


@pytest.mark.parametrize("act_hot", [True, False])
def test_dominated_row(act_hot):
    """One q is 1e4 above the rest: every other exponential underflows.  The dataset action is the dominating one: cql_b is
    exactly 0.0 and the CQL gradient vanishes exactly (softmax = one-hot = the indicator) -- the gradient is QRDQN's; another
    action: cql_b ~ 1e4.  Everything stays finite."""
    case = CE.dominated_case(act_hot)
    out, ref = check_update(case)
    for k in ("losses", "prio", "head"):
        assert torch.isfinite(out[k]).all(), k
    if act_hot:
        qr = run_update(case, qrdqn=True)
        assert float(out["losses"][2]) == 0.0 and torch.equal(out["head"], qr["head"])
    else:
        assert abs(float(out["losses"][2]) - 1.0e4) <= 8.0


@pytest.mark.parametrize("offset", [1.0e6, -1.0e6])
def test_large_common_offset(offset):
    """Quantiles and returns moved by +-1e6 (all exact in float32, tests/test_dcql_edge_inputs_cpu.py): per element against float64
    within the bar -- and, because T - theta, the means and q - max(q) are then all exact, the priorities, qr_loss and the whole
    head gradient are bit-identical to the offset-free run (the softmax is built from the exponentials of q - max(q), never
    from the logsumexp, which is rounded to an ulp of 1e6)."""
    out, ref = check_update(CE.offset_case(offset))
    base, ref0 = check_update(CE.offset_case(0.0))
    assert torch.equal(out["prio"], base["prio"]) and float(out["losses"][1]) == float(base["losses"][1])
    assert torch.equal(out["head"], base["head"])
    within(out["losses"][2], ref0["cql_loss"], ref["cql_loss_bar"], "cql_loss against the offset-free float64 value")


@pytest.mark.parametrize("last", [False, True])
def test_first_and_last_action(last):
    """act = 0 in every row / act = A - 1 in every row, (A, N) = (3, 255) (three padding columns) and (5, 65)."""
    for A, N in ((3, 255), (5, 65)):
        case = CE.grid_case(A, N, 5)
        case["act"] = torch.full((5,), A - 1 if last else 0, dtype=torch.int64)
        out, ref = check_update(case)
        assert bool((out["head"][512, :A * N] != 0).all())          # the CQL term reaches every live column


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", CE.N_GRID)
@pytest.mark.parametrize("A", CE.A_GRID)
def test_shape_limits(A, N, B):
    """N = 2, 63, 64, 65, 256 (one lane-strided pass, its edges, the limit), A = 1, 2, 64 (one lane per action: 64 is the limit;
    with four waves per sample A = 1, 2 leave waves without an action), B = 1 and 5."""
    check_update(CE.grid_case(A, N, B))


def test_zero_and_absent_weights():
    """weight=None is bit-identical to all ones.  All-zero weights: qr_loss is exactly 0.0, the priorities and cql_loss are
    untouched (the PER weight does not enter the CQL term) and the gradient is the CQL term alone."""
    case = CE.grid_case(3, 21, 5)
    B = case["B"]
    none = run_update(case, weight=None)
    ones = run_update(case, weight=torch.ones(B))
    for k in ("losses", "prio", "head"):
        assert torch.equal(none[k], ones[k]), k
    check_update(case, out=none, weight=None)
    zero = run_update(case, weight=torch.zeros(B))
    out, ref = check_update(case, out=zero, weight=torch.zeros(B))
    assert float(zero["losses"][1]) == 0.0 and float(zero["losses"][2]) == float(none["losses"][2])
    assert torch.equal(zero["prio"], none["prio"])
    assert float(ref["gbias_qr"].abs().max()) == 0.0
    # ... and min_q_weight = 0 with weights leaves QRDQN's gradient alone
    qr, off = run_update(case, qrdqn=True), run_update(case, mqw=0.0)
    assert torch.equal(qr["head"], off["head"]) and float(off["losses"][0]) == float(off["losses"][1]) == float(qr["losses"][0])
    assert float(off["losses"][2]) == float(none["losses"][2])
