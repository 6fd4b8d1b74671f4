"""The per-sample head kernels of ts_distq.hip (distq_head_kernel, distq_select_kernel, qr_loss_kernel, c51_loss_kernel,
mean_kernel) where tests/test_gpu_distq.py never goes: exact logits (zeroed head weights, tests/distq_edge_cases.py), returns on
and between the atoms and on / beyond the clamp, dominated softmax rows, |T - theta| == 1, Q-value ties, and the shape limits
N = 2 .. 256, A = 1 .. 64, B = 1.  `update_with_batch(apply=False, grad_out=)` returns the gradient: with zero head weights its
bias row is the column sum of the kernel's d_head and everything below the head is exactly zero.

Bars: exact claims are asserted exactly; the rest is per element against float64, |got - ref64| <= 4 err32 + tiny, err32 being
the float32 oracle formula's own error on the same input (tests/distq_edge_cases.py states the construction and the measured
figures; tests/test_distq_edge_inputs_cpu.py checks the preconditions without a GPU)."""
import numpy as np
import pytest
import torch

from oracle import oracle_dqn as OD
from tests import distq_edge_cases as E
from tests.distq_edge_gpu_common import SENTINEL, dev_obs, within

pytestmark = pytest.mark.gpu


def make_engine(kind, A, N, rows, v_min=-10.0, v_max=10.0, **kw):
    from tianshou_amd import distq as Q

    p = E.edge_params(A, N, rows)
    cfg = Q.DistQConfig(kind=kind, n_atoms=N, v_min=v_min, v_max=v_max, **kw)
    return Q.DistQEngine(E.C, E.H, E.W, A, flat(p, A, N), cfg)


def flat(p, A, N):
    from tianshou_amd import distq as Q

    return Q.flat_from_torch([p[k] for k in OD.PARAM_ORDER], E.C, E.H, E.W, A, N)


def run_update(case, weight="case", rows=None):
    """One gradient-only update on the case's edge network -> dict(loss, prio [B], target [B, N] or None, head [513, ld], below)."""
    A, N = case["A"], case["N"]
    eng = make_engine(case["kind"], A, N, case["rows"], case.get("v_min", -10.0), case.get("v_max", 10.0))
    sel = slice(None) if rows is None else rows
    if case["kind"] == E.C51:
        nd = case["nd"][sel].cuda().contiguous()
        eng.next_dist = lambda obs: nd                                     # exact control of the next-state distribution
    w = case["weight"] if isinstance(weight, str) else weight
    if w is not None:
        w = w[sel]
    x = dev_obs(case["obs"][sel])
    grad = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
    out = eng.update_with_batch(x, case["act"][sel], case["ret"][sel], w, obs_next_nhwc=x, grad_out=grad, apply=False,
                                want_target=True)
    torch.cuda.synchronize()
    ld = E.head_width(A, N)
    g = grad.cpu()
    return dict(loss=out[0].cpu(), prio=out[1].cpu(), target=None if out[2] is None else out[2].cpu(),
                head=g[-513 * ld:].reshape(513, ld), below=g[:-513 * ld])


def check_update(case, out=None, weight="case"):
    """target / prio / loss / bias-row gradient against float64 within the measured bars; the columns of the actions not taken,
    the padding columns and every gradient below the head exactly 0.0."""
    A, N = case["A"], case["N"]
    if not isinstance(weight, str):
        case = dict(case, weight=weight)
    out = run_update(case) if out is None else out
    ref = E.reference(case)
    print(f"  {case['kind']} A={A} N={N} B={case['B']}")
    if case["kind"] == E.C51:
        within(out["target"], ref["target"], ref["target_bar"], "target")
    within(out["prio"], ref["prio"], ref["prio_bar"], "prio")
    within(out["loss"], ref["loss"], ref["loss_bar"], "loss")
    within(out["head"][512, :A * N], ref["gbias"], ref["gbias_bar"], "bias gradient")
    assert torch.isfinite(out["head"]).all() and not out["below"].any()                # zero head weights pass nothing down
    assert not out["head"][:, A * N:].any()                                           # padding columns
    for a in range(A):
        if a not in set(case["act"].tolist()):
            assert not out["head"][:, a * N:(a + 1) * N].any(), a                      # ... and the actions not taken
    return out, ref


def check_forward(kind, A, N, B, rows, v_min=-5.0, v_max=5.0):
    eng = make_engine(kind, A, N, rows, v_min, v_max)
    dist, q, act = (t.cpu() for t in eng.forward(dev_obs(E.obs_batch(B, 3))))
    z = E.support32(v_min, v_max, N)
    h = E.head64(kind, rows, z)
    d32, q32 = E.head32(kind, rows, z)
    assert bool((dist == dist[0]).all()) and bool((q == q[0]).all())                   # the head is the same in every row
    if kind == E.QR:
        assert torch.equal(dist[0], rows.float())                                     # the quantiles ARE the bias
    within(dist[0], h["dist"], E.bar((d32.double() - h["dist"]).abs(), h["dist_scale"]), "dist")
    within(q[0], h["q"], E.bar((q32.double() - h["q"]).abs(), h["q_scale"]), "q")
    # the greedy action is the float64 one: the gap to the runner-up is beyond anything float32 can blur (the same assertion
    # runs without a GPU in tests/test_distq_edge_inputs_cpu.py, so no shape can slip out of this check unnoticed)
    assert E.greedy_gap(h) > E.GREEDY_GAP_ULPS
    assert bool((act == h["act"]).all())
    assert torch.equal(act, q.argmax(dim=1))
    return dist, q, act


# ---- C51 ---------------------------------------------------------------------------------------------------------------------
def test_c51_on_atom_returns_project_bit_exactly():
    """v_min, v_max, N = -4, 4, 9: dz == 1.0f and the atoms are the integers.  T_j = z_pi(j): every weight is 0 or 1, the
    projected target is nd permuted, bit for bit; one atom up with the top atom clamped onto itself: the shifted row."""
    A, N, B = 3, 9, 5
    z = E.support32(-4, 4, N)
    g = torch.Generator().manual_seed(1)
    perm = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    nd = E.random_dist(B, N, 2, zeros=True)
    case = E.c51_case(A, N, B, -4, 4, E.random_rows(A, N, 3), z[perm], nd, seed=1)
    out, _ = check_update(case)
    assert torch.equal(out["target"], torch.zeros(B, N).scatter_(1, perm, nd))
    up = dict(case, ret=z[perm] + 1.0)
    out, _ = check_update(up)
    assert torch.equal(out["target"], torch.zeros(B, N).scatter_add_(1, (perm + 1).clamp(max=N - 1), nd))


def test_c51_half_way_returns_split_evenly():
    """T_j = z_j + 0.5: m_i = 0.5 nd_i + 0.5 nd_(i-1) (the top atom takes its own whole mass through the clamp).  Bit-equality is
    not asserted: the kernel adds the N products of one atom one after the other, the oracle in torch's blocked order."""
    case = E.halfway_case()
    out, ref = check_update(case)
    nd = case["nd"].double()
    want = 0.5 * nd
    want[:, 1:] += 0.5 * nd[:, :-1]
    want[:, -1] += 0.5 * nd[:, -1]
    torch.testing.assert_close(ref["target"], want, rtol=0, atol=1e-15)


def test_c51_clamp_boundaries_and_infinite_returns():
    """Returns at v_min / v_max, one float32 inward and outward of both, +-1e6 and +-inf: finite everywhere, and rows whose
    returns all lie beyond one end put their whole mass into that end atom, exactly."""
    case = E.clamp_case()
    out, ref = check_update(case)
    for k in ("target", "prio", "loss", "head"):
        assert torch.isfinite(out[k]).all(), k
    assert not out["target"][2, 1:].any() and not out["target"][3, :-1].any()
    # returns 0, 2 (inward: weight 1 - 2^-22 -> the neighbour gets 2^-22 nd), 4, 6 of row 0 land on atom 0; nothing else does
    assert float(out["target"][0, 0]) > 0 and float(out["target"][0, -1]) > 0


def test_c51_projection_conserves_mass_on_an_inexact_grid():
    """v_min, v_max, N = -10, 10, 51: dz = 0.4 is no float32.  Per row |sum_i m_i - sum_j nd_j| stays within what float64 loses
    to the float32 atoms plus 4 x the float32 oracle's own mass error plus the floor; every m_i lies in [0, 1]."""
    case = E.mass_case()
    out, ref = check_update(case)
    m = out["target"].double()
    assert bool((m >= 0).all()) and bool((m <= 1).all())
    mass, mass64, mass32 = m.sum(-1), ref["target"].sum(-1), ref["target32"].double().sum(-1)
    nd_sum = case["nd"].double().sum(-1)
    mbar = (mass64 - nd_sum).abs() + E.bar((mass32 - mass64).abs(), nd_sum)
    print(f"    mass: |sum m - sum nd| {float((mass - nd_sum).abs().max()):.2e}, bar {float(mbar.min()):.2e}, "
          f"float64 {float((mass64 - nd_sum).abs().max()):.2e}, float32 oracle {float((mass32 - nd_sum).abs().max()):.2e}")
    assert bool(((mass - nd_sum).abs() <= mbar).all())


@pytest.mark.parametrize("graded", [False, True])
def test_c51_dominated_softmax_row(graded):
    """The taken action's row is +60 / -60 (every other p underflows to 0.0f) or graded 0 .. -25 (p straddles the 1e-8 of
    log(p + 1e-8)); the target has mass on those atoms.  prio, loss and every entry of d logits per element against float64."""
    check_update(E.dominated_case(graded))
    if not graded:       # mass m on an atom whose probability is exactly 0, the rest on the hot atom (log(1 + 1e-8f) == 0):
        N = 9            # ce = -m * logf(0 + 1e-8f), for m = 1, a dyadic and a rounded fraction
        z = E.support32(-4, 4, N)
        rows = torch.stack([E.dominated_row(N, 2 * i + 1) for i in range(3)])
        log_eps = np.log(np.float32(1e-8), dtype=np.float32)
        for m in (1.0, 0.25, 0.3):
            nd = torch.zeros(1, N)
            nd[0, 4], nd[0, 1] = m, 1.0 - m                                # action 0 is hot on atom 1
            out, _ = check_update(E.c51_case(3, N, 1, -4, 4, rows, z[None, :], nd, act=[0]))
            want = -(np.float32(m) * log_eps)
            assert abs(float(out["prio"][0]) - float(want)) <= 2 * float(np.spacing(want)), (m, float(out["prio"][0]), float(want))
            assert torch.equal(out["target"], nd)


@pytest.mark.parametrize("kind", [E.C51, E.QR])
def test_zero_and_absent_weights(kind):
    """weight=None is bit-identical to all ones; weight = B e_r (every other row 0) leaves the priorities untouched and the
    gradient bit-identical to a B = 1 update on row r alone: the zero-weight rows contribute exactly nothing."""
    case = E.grid_case(kind, 2, 51, 5)
    B = case["B"]
    none = run_update(case, weight=None)
    ones = run_update(case, weight=torch.ones(B))
    for k in ("loss", "prio", "head") + (("target",) if kind == E.C51 else ()):
        assert torch.equal(none[k], ones[k]), k
    check_update(case, out=none, weight=None)
    mixed = E.f32([0.0, 1.0, 0.5, 0.0, 2.0])
    check_update(case, weight=mixed)
    for r in (0, B - 1):
        w = torch.zeros(B)
        w[r] = float(B)
        hot = run_update(case, weight=w)
        alone = run_update(case, weight=None, rows=slice(r, r + 1))
        assert torch.equal(hot["prio"], none["prio"]) and hot["prio"][r] == alone["prio"][0]
        assert torch.equal(hot["head"][512], alone["head"][512]), r
        assert hot["head"][512].any() and not hot["below"].any()


@pytest.mark.parametrize("kind", [E.C51, E.QR])
@pytest.mark.parametrize("last", [False, True])
def test_columns_of_other_actions_and_padding_stay_zero(kind, last):
    """act = 0 in every row / act = A - 1 in every row, (A, N) = (3, 255) (three padding columns) and (5, 65): the gradient is
    exactly 0.0 in every column of every action not taken and in the padding (check_update asserts it on all 513 rows)."""
    for A, N in ((3, 255), (5, 65)):
        case = E.grid_case(kind, A, N, 5)
        case["act"] = torch.full((5,), A - 1 if last else 0, dtype=torch.int64)
        out, _ = check_update(case)
        a = A - 1 if last else 0
        assert out["head"][512, a * N:(a + 1) * N].any()


@pytest.mark.parametrize("kind", [E.C51, E.QR])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("A,N", E.GRID)
def test_shape_limits(kind, A, N, B):
    """N = 2, 64, 65, 255, 256 (one thread per atom in c51_loss_kernel: 256 is the limit), A = 1 and 64, heads without padding
    columns, B = 1 and B = 5 (the second workgroup of distq_head_kernel has one live wave)."""
    case = E.grid_case(kind, A, N, B)
    check_forward(kind, A, N, B, case["rows"])
    check_update(case)


# ---- QRDQN -------------------------------------------------------------------------------------------------------------------
def test_qr_returns_equal_to_theta_give_exact_zeros():
    A, N, B = 3, 33, 5
    rows = torch.stack([torch.full((N,), 1.25 * (i + 1)) for i in range(A)])
    act = torch.tensor([0, 1, 2, 1, 0])
    case = E.qr_case(A, N, B, rows, rows[act], act=act, weight=E.f32([1.0, 0.5, 2.0, 0.25, 1.5]))
    out = run_update(case)
    assert float(out["loss"]) == 0.0 and not out["prio"].any() and not out["head"].any() and not out["below"].any()


def test_qr_unit_distance_and_its_neighbours():
    """theta == 0, T_j in {-1, +1} and one float32 on either side of each, so d = T_j - theta_i takes exactly those six values
    (tests/test_distq_edge_inputs_cpu.py checks it): per element against float64."""
    check_update(E.qr_unit_case())


@pytest.mark.parametrize("N", [7, 200, 256])
def test_qr_linear_region_closed_forms(N):
    """All T >= all theta + 2: d theta_i = -w_b tau_i / B; all T <= all theta - 2: +w_b (1 - tau_i) / B.  Bar 4 N eps32 of the
    closed form: the kernel adds N equal terms one after the other."""
    A, B = 3, 5
    rows = E.random_rows(A, N, 1, 0.3)
    g = torch.Generator().manual_seed(2)
    act = torch.tensor([0, 2, 2, 1, 0])
    w = E.f32([1.0, 0.5, 2.0, 0.25, 1.5])
    tau = E.OQ.tau_hat(N).double()
    for sign in (1.0, -1.0):
        ret = sign * (float(rows.abs().max()) + 2.0 + torch.rand(B, N, generator=g) * 3.0)
        out = run_update(E.qr_case(A, N, B, rows, ret, act=act, weight=w))
        per_row = (-(w.double() / B)[:, None] * tau[None, :]) if sign > 0 else ((w.double() / B)[:, None] * (1.0 - tau)[None, :])
        want, size = E.scatter_rows(per_row, act, A), E.scatter_rows(per_row.abs(), act, A)
        got = out["head"][512, :A * N].double().reshape(A, N)
        assert bool(((got - want).abs() <= 4 * N * E.EPS32 * size).all()), float(((got - want).abs() / size.clamp_min(1e-300)).max())


def test_qr_large_returns():
    """Returns ~1e4 (every |d| far in the linear region, l ~ 1e4): per element against float64."""
    check_update(E.qr_large_case())


# ---- argmax ties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,negative", [(E.QR, False), (E.QR, True), (E.C51, False), (E.C51, True)])
@pytest.mark.parametrize("A,tied", [(4, (0, 2)), (5, (3, 4)), (6, (1, 3, 4)), (5, (4,))])
def test_argmax_ties_take_the_lowest_index(kind, negative, A, tied):
    """Two or three actions with bit-identical rows hold the maximal Q ((5, (4,)): a strict maximum at the last action).
    `forward` returns the lowest tied index, and `next_dist` the lagged net's row of that index, bit-equal to
    forward(params_old)'s.  `negative`: every Q is below zero (the running maximum must start from the first action's Q, not 0)."""
    from tianshou_amd import distq as Q

    N, B = 9, 5
    v_min, v_max = (-12.0, -4.0) if negative else (-4.0, 4.0)
    rows = E.tie_rows_qr(A, N, tied) - (20.0 if negative else 0.0) if kind == E.QR else E.tie_rows_c51(A, N, tied)
    eng = make_engine(kind, A, N, rows, v_min, v_max, target_update_freq=3)
    old_rows = E.random_rows(A, N, 21)
    eng.params_old = flat(E.edge_params(A, N, old_rows, seed=2), A, N)
    x = dev_obs(E.obs_batch(B, 4))
    dist, q, act = (t.cpu() for t in eng.forward(x))
    d32, q32 = E.head32(kind, rows, E.support32(v_min, v_max, N))
    assert int(q32.argmax()) == tied[0] and bool((q32[list(tied)] == q32[tied[0]]).all())        # the oracle, on the same values
    assert not negative or bool((q32 < 0).all())
    assert bool((act == tied[0]).all()), act
    assert bool((q[:, list(tied)] == q[:, tied[:1]]).all()) and bool((q.max(dim=1).values == q[:, tied[0]]).all())
    nd = eng.next_dist(x).cpu()
    d_old = eng.forward(x, params=eng.params_old)[0].cpu()
    assert torch.equal(nd, d_old[:, tied[0]])
    others = [a for a in range(A) if a != tied[0]]
    assert all(not torch.equal(d_old[:, a], d_old[:, tied[0]]) for a in others)                  # the lagged rows do differ
