"""The per-sample kernels of ts_iqn.hip (iqn_head_kernel, iqn_select_kernel, iqn_loss_kernel, iqn_mean_kernel) where
tests/test_gpu_iqn.py never goes: exact quantile values (zeroed head weights, tests/iqn_edge_cases.py), Q ties across the halves
of the wave shuffle, all-negative Q next to padding columns, A = 1 .. 64, N and N' at 2 and 64 and unequal, fractions 0 and one
ulp below 1, |T - theta| == 1 and its neighbours, returns far in the linear region, weight 0, B = 1 and B > 1024.
`update_with_batch(apply=False, grad_out=)` returns the gradient: with zero head weights its bias row is the column sum of the
kernel's d_out and everything below the head is exactly zero.

Bars: exact claims are asserted exactly; the rest is per element against float64, |got - ref64| <= 4 err32 + 4 eps32 scale, err32
being the float32 oracle formula's own error on the same input (tests/iqn_edge_cases.py states the construction and the measured
figures; tests/test_iqn_edge_inputs_cpu.py checks the preconditions without a GPU)."""
import pytest
import torch

from tests import iqn_edge_cases as E
from tests import oracle_iqn as OI
from tests.distq_edge_gpu_common import SENTINEL, dev_obs, within

pytestmark = pytest.mark.gpu


def flat(p, A):
    from tianshou_amd import iqn as I

    return I.flat_from_torch([p[k] for k in OI.PARAM_ORDER], E.C, E.H, E.W, A)


def make_engine(A, b2, **kw):
    from tianshou_amd import iqn as I

    return I.IQNEngine(E.C, E.H, E.W, A, flat(E.edge_params(A, b2), A), I.IQNConfig(**kw))


def run_update(case, eng=None):
    """One gradient-only update on the case's edge network -> dict(loss, prio [B], head [513, ld], below)."""
    A = case["A"]
    eng = make_engine(A, case["b2"]) if eng is None else eng
    grad = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
    loss, prio = eng.update_with_batch(dev_obs(case["obs"]), case["act"], case["ret"], case["weight"], tau=case["tau"].cuda(),
                                       grad_out=grad, apply=False)
    torch.cuda.synchronize()
    ld = E.head_ld(A)
    g = grad.cpu()
    return dict(loss=loss.cpu(), prio=prio.cpu(), head=g[-513 * ld:].reshape(513, ld), below=g[:-513 * ld])


def check_update(case):
    """prio / loss / bias-row gradient against float64 within the measured bars; the columns of the actions not taken, the padding
    columns and every gradient below the head exactly 0.0; a second run bit-identical."""
    A = case["A"]
    eng = make_engine(A, case["b2"])
    out, again = run_update(case, eng), run_update(case, eng)
    for k in ("loss", "prio", "head", "below"):
        assert torch.equal(out[k], again[k]), k                                       # bit-identical reruns
    ref = E.reference(case)
    print(f"  A={A} N={case['N']} N'={case['Np']} B={case['B']}")
    within(out["prio"], ref["prio"], ref["prio_bar"], "prio")
    within(out["loss"], ref["loss"], ref["loss_bar"], "loss")
    within(out["head"][512, :A], ref["gbias"], ref["gbias_bar"], "bias gradient")
    assert torch.isfinite(out["head"]).all() and not out["below"].any()                # zero head weights pass nothing down
    assert not out["head"][:, A:].any()                                               # padding columns
    taken = set(case["act"].tolist())
    for a in range(A):
        if a not in taken:
            assert not out["head"][:, a].any(), a                                     # ... and the actions not taken
    return out, ref


# ---- head, forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", E.HEAD_A)
def test_head_logits_are_the_bias_and_q_its_mean(A):
    """A = 1, 2, 32, 33, 64 x N = 2, 7, 64 x B = 1, 5 (B = 5 ends in a partly filled last workgroup of 4 waves), biases around 0
    and around -20: logits bit for bit in every (b, n), Q within its bar, the greedy action float64's.  With every Q negative
    (A = 33: 31 padding columns holding 0.0) the action is never a padding column."""
    for N in E.HEAD_N:
        for shift in (0.0, -20.0):
            b2 = E.head_bias(A, N, 3 + A + N, shift)
            eng = make_engine(A, b2)
            h = E.head64(b2)
            qbar = E.bar((E.head32(b2, N).double() - h["q"]).abs(), h["q_scale"])
            for B in E.HEAD_B:
                tau = E.edge_fractions(B, N, torch.Generator().manual_seed(B))
                lg, q, act = (t.cpu() for t in eng.forward(dev_obs(E.obs_batch(B, 3)), tau=tau.cuda()))
                assert torch.equal(lg, b2.view(1, A, 1).expand(B, A, N)), (N, B, shift)
                print(f"  A={A} N={N} B={B} shift={shift}")
                within(q, h["q"].expand(B, A), qbar.expand(B, A), "q")
                assert E.greedy_gap(h) > E.GREEDY_GAP_ULPS                          # (also asserted without a GPU)
                assert bool((act == h["act"]).all()) and int(act.max()) < A, (N, B, shift, act)
                assert torch.equal(act, q.argmax(dim=1))


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("A,tied", E.TIES)
def test_q_ties_take_the_first_index(A, tied, negative):
    """Bit-identical maximal Q in lanes (0, 63), (31, 32), (5, 37), in three lanes, in every lane (act = 0), and a strict maximum on
    the last action; `negative`: every Q below zero."""
    b2 = E.tie_bias(A, tied, negative)
    eng = make_engine(A, b2)
    for N in E.HEAD_N:
        for B in E.HEAD_B:
            tau = torch.rand(B, N, generator=torch.Generator().manual_seed(N + B))
            lg, q, act = (t.cpu() for t in eng.forward(dev_obs(E.obs_batch(B, 4)), tau=tau.cuda()))
            assert torch.equal(lg, b2.view(1, A, 1).expand(B, A, N))
            assert torch.equal(q, b2.view(1, A).expand(B, A)), (N, B)                 # dyadic biases: the mean is exact
            assert bool((act == tied[0]).all()), (N, B, act)


# ---- next_dist ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lagged", [True, False])
@pytest.mark.parametrize("N,Np", [(2, 64), (64, 2), (5, 7)])
def test_next_dist_selects_the_first_tied_action(lagged, N, Np):
    """The online net's Q ties; the lagged net's bias is distinct per action: out[b, j] == b2_old[first tied action] exactly for
    all j ([B, N'] with a lagged net, [B, N] of the online bias without)."""
    for A, tied in ((64, (5, 37)), (33, (31, 32)), (2, (0, 1)), (33, (32,))):
        b2 = E.tie_bias(A, tied, negative=True)
        b2_old = E.head_bias(A, 2, 70 + A)
        assert len(set(b2_old.tolist())) == A
        eng = make_engine(A, b2, target_update_freq=3 if lagged else 0, online_sample_size=N, target_sample_size=Np)
        if lagged:
            eng.params_old = flat(E.edge_params(A, b2_old, seed=2), A)
        for B in (1, 5):
            g = torch.Generator().manual_seed(B)
            out = eng.next_dist(dev_obs(E.obs_batch(B, 5)), torch.rand(B, N, generator=g).cuda(),
                                torch.rand(B, Np, generator=g).cuda() if lagged else None).cpu()
            want = (b2_old if lagged else b2)[tied[0]]
            assert tuple(out.shape) == (B, Np if lagged else N)
            assert bool((out == want).all()), (A, tied, B, out, want)


# ---- loss --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("N,Np", E.LINEAR_SHAPES)
def test_loss_linear_region_closed_form(N, Np, sign):
    """Every T_j >= theta + 1 (sign +) / <= theta - 1 (sign -), two samples at returns ~1e4, tau = 0 and tau one ulp below 1 in
    every row: the bias gradient is the closed form sum over the rows of -w_b N' tau_i / (B N) (+w_b N' (1 - tau_i) / (B N)),
    bar 4 N' eps32 of its absolute sum; the sample whose fractions are all 0 gets exactly nothing for an under-estimate."""
    case = E.linear_case(sign, N, Np)
    out, _ = check_update(case)
    want, size = E.linear_closed_form(case, sign)
    within(out["head"][512, :case["A"]], want, 4 * Np * E.EPS32 * size, "bias gradient against the closed form")
    if sign > 0:
        assert float(out["head"][512, 4]) == 0.0                                      # sample 3: every tau = 0
    else:
        assert float(out["head"][512, 4]) > 0.0


def test_loss_unit_distance_and_its_neighbours():
    """theta == 0, T_j in {-1, +1} and one float32 on either side of each, so d = T_j - theta takes exactly those six values
    (tests/test_iqn_edge_inputs_cpu.py checks it): per element against float64."""
    check_update(E.unit_case())


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("A,N,Np", E.MIXED_SHAPES)
def test_loss_mixed_case(A, N, Np, weighted):
    """T_j on both sides of theta, |d| below and above 1, (A, N, N') = (1, 2, 2), (64, 64, 64), (33, 5, 64), (3, 64, 2).  With
    `weight`, rows 0 and 3 have weight 0: they do not count in the loss (float64 leaves them out), and an action only they take
    has a gradient column that is exactly 0."""
    case = E.mixed_case(A, N, Np, weighted)
    out, ref = check_update(case)
    if weighted and A >= 3:
        assert float(ref["gbias"][0]) == 0.0 and not out["head"][:, 0].any()          # action 0: the zero-weight row 0 alone
        assert out["head"][512, A - 1] != 0.0
    if not weighted:                                                                  # weight=None is all ones, bit for bit
        ones = run_update(dict(case, weight=torch.ones(case["B"])))
        for k in ("loss", "prio", "head"):
            assert torch.equal(out[k], ones[k]), k


@pytest.mark.parametrize("B", [1, 1030])
def test_mean_kernel_batch_sizes(B):
    """B = 1 and B = 1030 (six threads of iqn_mean_kernel take a second trip through the 1024-stride loop), N = N' = 2: the loss
    against float64, scale the sum of |lw| / B."""
    check_update(E.mean_case(B))
