"""Rainbow's own kernels in ts_distq.hip (noisy_eff_kernel, noisy_grad_kernel, dueling_kernel, dueling_bwd_kernel) and the C51
head / loss kernels on the ts_rainbow_* call path, on edge networks whose Q.2 / V.2 outputs are exactly their effective biases
(zero weight mu and sigma; tests/distq_edge_cases.py): A = 1 and A = 64, N = 2, chosen noise, dominated rows, on-atom and clamped
returns, Q-value ties.  Bars as in tests/test_gpu_distq_edges.py: exact where the arithmetic is exact, otherwise per element
against float64 with 4 x the float32 oracle's own error plus 4 ulp of the row's scale."""
import pytest
import torch

from oracle import oracle_rainbow as ORB
from tests import distq_edge_cases as E
from tests.distq_edge_gpu_common import SENTINEL, dev_obs, within

pytestmark = pytest.mark.gpu
NOISE_ORDER = [f"{L}.{t}" for L in ORB.NOISY for t in ("eps_p", "eps_q")]
NAMES = dict(bq_mu="Q2.mu_b", bq_sigma="Q2.sigma_b", bv_mu="V2.mu_b", bv_sigma="V2.sigma_b")


def flats(p, noise, A, N):
    from tianshou_amd import rainbow as RB

    dims = (E.C, E.H, E.W, A, N)
    return RB.flat_from_torch([p[k] for k in ORB.PARAM_ORDER], *dims), RB.noise_from_torch([noise[k] for k in NOISE_ORDER], *dims)


def make_engine(case, **kw):
    from tianshou_amd import distq as Q
    from tianshou_amd import rainbow as RB

    A, N = case["A"], case["N"]
    params, noise = flats(*E.rainbow_params(case), A, N)
    eng = RB.RainbowEngine(E.C, E.H, E.W, A, params, noise, Q.DistQConfig(kind="c51", n_atoms=N, v_min=case["v_min"], v_max=case["v_max"], **kw))
    nd = case["nd"].cuda().contiguous()
    if not kw:
        eng.next_dist = lambda obs: nd
    return eng


def run(case):
    """forward and one gradient-only update -> dict(dist [A, N], q [A], act, loss, prio, target, grads by ORB.PARAM_ORDER, raw)."""
    from tianshou_amd import rainbow as RB

    A, N = case["A"], case["N"]
    eng = make_engine(case)
    x = dev_obs(case["obs"])
    dist, q, act = (t.cpu() for t in eng.forward(x))
    assert bool((dist == dist[0]).all()) and bool((q == q[0]).all()) and torch.equal(act, q.argmax(dim=1))
    grad = torch.full((eng.P,), SENTINEL, dtype=torch.float32, device="cuda")
    loss, prio, tgt = eng.update_with_batch(x, case["act"], case["ret"], x, case["weight"], grad_out=grad, apply=False, want_target=True)
    torch.cuda.synchronize()
    grads = dict(zip(ORB.PARAM_ORDER, (t.cpu() for t in RB.flat_to_torch(grad, E.C, E.H, E.W, A, N))))
    return dict(dist=dist[0], q=q[0], act=act, loss=loss.cpu(), prio=prio.cpu(), target=tgt.cpu(), grads=grads, raw=grad.cpu(), eng=eng)


def check(case):
    A, N = case["A"], case["N"]
    out, r = run(case), E.rainbow64(case)
    print(f"  rainbow A={A} N={N} B={case['B']}")
    within(out["dist"], r["dist"], r["dist_bar"], "dist")
    within(out["q"], r["q"], r["q_bar"], "q")
    within(out["target"], r["target"], r["target_bar"], "target")
    within(out["prio"], r["ce"], r["ce_bar"], "prio")
    within(out["loss"], r["loss"], r["loss_bar"], "loss")
    for k, key in NAMES.items():
        within(out["grads"][key], r["grads"][k], r["grad_bars"][k], key)
    # sigma gradient = mu gradient x eps_q: one float32 product per element
    assert torch.equal(out["grads"]["Q2.sigma_b"], out["grads"]["Q2.mu_b"] * case["eps_q"].reshape(-1))
    assert torch.equal(out["grads"]["V2.sigma_b"], out["grads"]["V2.mu_b"] * case["eps_v"])
    # nothing flows below zero Q.2 / V.2 weights; the padding columns of both layers (mu and sigma blocks, all 513 rows) are zero
    for k in ORB.PARAM_ORDER:
        assert torch.isfinite(out["grads"][k]).all(), k
        if not k.startswith(("Q2", "V2")):
            assert not out["grads"][k].any(), k
    lay = out["eng"].lay
    for off, ld, used in ((lay["lin"][1], lay["ldq"], A * N), (lay["lin"][3], lay["ldv"], N)):
        for blk in range(2):
            m = out["raw"][off + blk * 513 * ld: off + (blk + 1) * 513 * ld].reshape(513, ld)
            assert not m[:, used:].any(), (off, blk)
    return out, r


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("A,N", E.RAINBOW_GRID)
def test_dueling_and_noisy_bias_against_float64(A, N, B):
    """logits = bq_eff[a, j] - mean_a bq_eff[., j] + bv_eff[j], b_eff = mu + sigma eps_q: probabilities, Q, loss, priorities and the
    four bias gradients (V.2 mu: sum_a dl; Q.2 mu: dl - mean_a dl; sigma: x eps_q) per element."""
    out, r = check(E.rainbow_case(A, N, B))
    if A == 1:
        assert not out["grads"]["Q2.mu_b"].any() and not out["grads"]["Q2.sigma_b"].any()          # dl - dl / 1 == 0 exactly


@pytest.mark.parametrize("N", [51, 2])
def test_single_action_logits_are_the_value_row(N):
    """A = 1: q - mean_a q cancels exactly (as in the oracle, tests/test_distq_edge_inputs_cpu.py), so the distribution is
    bit-identical to that of a network whose advantage bias is zero."""
    case = E.rainbow_case(1, N, 5)
    bare = dict(case, bq_mu=torch.zeros(1, N), bq_sigma=torch.zeros(1, N))
    x = dev_obs(case["obs"])
    d1, q1, _ = make_engine(case).forward(x)
    d0, q0, _ = make_engine(bare).forward(x)
    assert torch.equal(d1, d0) and torch.equal(q1, q0)


@pytest.mark.parametrize("A,N", [(6, 51), (3, 33)])
def test_zero_noise_is_eval_mode_and_gives_no_sigma_gradient(A, N):
    from tianshou_amd import rainbow as RB

    case = E.rainbow_case(A, N, 5, zero_noise=True)
    eng = make_engine(case)
    eng.noise.zero_()                                                     # all-zero noise in every layer
    x = dev_obs(case["obs"])
    a, b = eng.forward(x, training=True), eng.forward(x, training=False)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    out, _ = check(case)                                                  # eps_q of Q.2 / V.2 zero, the rest drawn
    lay = out["eng"].lay
    for i, ld in ((1, lay["ldq"]), (3, lay["ldv"])):
        sigma = out["raw"][lay["lin"][i] + 513 * ld: lay["lin"][i] + 2 * 513 * ld]
        assert not sigma.any(), i                                         # weights (eps_q[o] * eps_p[k]) and bias (eps_q[o]) alike


@pytest.mark.parametrize("pattern", ["dominated", "on_atom", "clamp"])
def test_c51_edges_through_the_rainbow_update(pattern):
    case = E.rainbow_case(3, 9, 4, pattern)
    out, r = check(case)
    if pattern == "on_atom":
        z = case["support"]
        perm = (case["ret"] - z[0]).long()                                # T_j = z_perm(j)
        assert torch.equal(out["target"], torch.zeros(4, 9).scatter_(1, perm, case["nd"]))
    if pattern == "clamp":
        assert torch.isfinite(out["target"]).all() and torch.isfinite(out["prio"]).all() and torch.isfinite(out["raw"]).all()
    if pattern == "dominated":
        p = r["o32"]["dist"]
        assert int((p == 0.0).sum()) == 3 * 8                            # every row: one 1.0f, eight exact zeros (the oracle)
        assert int((out["dist"] == 0.0).sum()) == 3 * 8


@pytest.mark.parametrize("A,tied", [(4, (0, 2)), (5, (3, 4)), (5, (4,))])
def test_argmax_ties_take_the_lowest_index(A, tied):
    """Tied actions share one advantage row, so their logits, probabilities and Q are bit-identical; `forward` and the greedy
    action inside `next_dist` take the lowest index, and next_dist returns the lagged net's row of it."""
    N, B = 9, 5
    case = E.rainbow_case(A, N, B, seed=1)
    case["bq_mu"] = case["bq_mu"] * 0.2
    for i in tied:                                                        # the tied row leans on the top atoms: the largest Q
        case["bq_mu"][i] = torch.linspace(-2, 2, N)
        case["bq_sigma"][i], case["eps_q"][i] = case["bq_sigma"][tied[0]], case["eps_q"][tied[0]]
    o32 = E.rainbow32(case)
    assert int(o32["q"].argmax()) == tied[0] and bool((o32["q"][list(tied)] == o32["q"][tied[0]]).all())     # the oracle
    assert all(float(o32["q"][a]) < float(o32["q"][tied[0]]) for a in range(A) if a not in tied)
    eng = make_engine(case, target_update_freq=3)
    old = E.rainbow_case(A, N, B, seed=2)
    eng.params_old, eng.noise_old = flats(*E.rainbow_params(old), A, N)
    x = dev_obs(case["obs"])
    dist, q, act = (t.cpu() for t in eng.forward(x))
    assert bool((act == tied[0]).all()), act
    assert bool((q[:, list(tied)] == q[:, tied[:1]]).all()) and bool((q.max(dim=1).values == q[:, tied[0]]).all())
    nd = eng.next_dist(x).cpu()
    d_old = make_engine(old).forward(x)[0].cpu()
    assert torch.equal(nd, d_old[:, tied[0]])
    assert all(not torch.equal(d_old[:, a], d_old[:, tied[0]]) for a in range(A) if a != tied[0])
