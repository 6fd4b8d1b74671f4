"""CPU checks of tests/distq_edge_cases.py: the float64 references agree with the float32 oracles (oracle_distq / oracle_rainbow
`update_with_batch`, already pinned to the unmodified reference) on the edge networks, the preconditions of the exact GPU
assertions hold, and the float32 oracle's own error against float64 (err32, what the GPU bars are built from) is measured:
`pytest -s` prints the figures quoted in tests/distq_edge_cases.py."""
import numpy as np
import pytest
import torch

from oracle import oracle_distq as OQ
from oracle import oracle_dqn as OD
from oracle import oracle_rainbow as ORB
from tests import distq_edge_cases as E


def _c51_cases():
    yield "halfway", E.halfway_case()
    yield "mass", E.mass_case()
    yield "dominated", E.dominated_case(False)
    yield "graded", E.dominated_case(True)
    yield "clamp", E.clamp_case()
    for a, n in E.GRID:
        for b in (1, 5):
            yield f"grid A{a} N{n} B{b}", E.grid_case(E.C51, a, n, b)


def _qr_cases():
    yield "unit", E.qr_unit_case()
    yield "large", E.qr_large_case()
    for a, n in E.GRID:
        for b in (1, 5):
            yield f"grid A{a} N{n} B{b}", E.grid_case(E.QR, a, n, b)


def _oracle_update(case, monkeypatch):
    """oracle_distq.update_with_batch on the case's edge network (C51: next_dist substituted, as the GPU tests do on the
    engine) -> (loss, prio, collect)."""
    kind, a, n = case["kind"], case["A"], case["N"]
    cfg = OQ.DistQConfig(kind=kind, n_atoms=n, v_min=case.get("v_min", -10.0), v_max=case.get("v_max", 10.0))
    st = OD.DQNState.create(E.edge_params(a, n, case["rows"]), cfg.dqn())
    if kind == E.C51:
        monkeypatch.setattr(OQ, "next_dist", lambda *args, **kw: case["nd"].clone())
    col: dict = {}
    w = None if case["weight"] is None else case["weight"].numpy()
    loss, prio = OQ.update_with_batch(st, cfg, case["obs"], case["act"].numpy(), case["ret"].numpy(), a, weight=w, obs_next=case["obs"],
                                      collect=col)
    return loss, prio, col


@pytest.mark.parametrize("kind", [E.C51, E.QR])
def test_float64_references_agree_with_the_oracle_on_the_edge_networks(kind, monkeypatch):
    worst: dict = {}
    for name, case in (_c51_cases() if kind == E.C51 else _qr_cases()):
        a, n = case["A"], case["N"]
        ref = E.reference(case)
        loss, prio, col = _oracle_update(case, monkeypatch)
        # the head is the bias, exactly, and nothing flows below zero head weights
        head = OD.forward(E.edge_params(a, n, case["rows"]), case["obs"])
        assert torch.equal(head, case["rows"].reshape(1, -1).expand(case["B"], -1)), name
        for k in OD.PARAM_ORDER[:8]:
            assert not col["grads"][k].any(), (name, k)
        # the logits-level float32 formula IS the oracle's (same torch expressions on the same values)
        if kind == E.C51:
            assert torch.equal(col["target_dist"], ref["target32"]), name
        got = dict(prio=prio.double(), loss=torch.tensor(loss, dtype=torch.float64), gbias=col["grads"]["fc2.b"].double().reshape(a, n))
        if kind == E.C51:
            got["target"] = col["target_dist"].double()
        for k, v in got.items():
            assert torch.isfinite(v).all(), (name, k)
            # the oracle against float64, within the bar built from the logits-level formula's error (the two differ by the order
            # in which autograd adds rows of one action: 2 ulp of the scale on top)
            excess = (v - ref[k]).abs() - ref[k + "_bar"] - 2 * E.EPS32 * torch.as_tensor(ref[k + "_scale"])
            assert bool((excess <= 0).all()), (name, k, float(excess.max()))
        units = E.err32_units(ref)
        print(f"{kind} {name}: err32 / (eps32 * scale) = " + ", ".join(f"{k} {v:.2f}" for k, v in units.items()))
        for k, v in units.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 4.0, (name, k, v)                  # the float32 oracle itself stays inside the smallest floor
    print(f"{kind}: worst over all cases: {worst}")


def test_forward_references_and_their_err32():
    worst = {}
    for kind in (E.QR, E.C51):
        for a, n in E.GRID:
            rows = E.random_rows(a, n, 11 + a + n)
            z = E.support32(-5, 5, n)
            h = E.head64(kind, rows, z)
            d32, q32 = E.head32(kind, rows, z)
            cfg = OQ.DistQConfig(kind=kind, n_atoms=n, v_min=-5.0, v_max=5.0)
            d_o = OQ.dist(E.edge_params(a, n, rows), cfg, E.obs_batch(2), a)
            assert torch.equal(d_o[0], d32) and torch.equal(d_o[1], d32) and torch.equal(OQ.q_values(d_o, cfg)[0], q32)
            ud = float(((d32.double() - h["dist"]).abs() / (E.EPS32 * h["dist_scale"])).max())
            uq = float(((q32.double() - h["q"]).abs() / (E.EPS32 * h["q_scale"])).max())
            worst[kind] = (max(worst.get(kind, (0, 0))[0], ud), max(worst.get(kind, (0, 0))[1], uq))
            assert ud <= 4.0 and uq <= 4.0
            assert int(q32.argmax()) == h["act"]
            # the GPU tests compare the greedy action with float64's at every one of these shapes: the gap must allow it
            assert E.greedy_gap(h) > E.GREEDY_GAP_ULPS, (kind, a, n, E.greedy_gap(h))
    print(f"forward err32 / (eps32 * scale), (dist, q): {worst}")


def test_integer_support_and_unit_delta_z():
    z = torch.linspace(-4, 4, 9)
    assert torch.equal(z, torch.arange(-4, 5, dtype=torch.float32))
    assert (4.0 - -4.0) / (9 - 1) == 1.0 and np.float32((4.0 - -4.0) / (9 - 1)) == np.float32(1.0)
    # ... and the awkward one is inexact: dz = 0.4 is no float32, nor are most of its atoms
    assert float(np.float32(0.4)) != 0.4 and not torch.equal(torch.linspace(-10, 10, 51).double(), -10 + 0.4 * torch.arange(51).double())


def test_on_atom_projection_is_a_permutation_in_the_oracle():
    n, b = 9, 5
    z = E.support32(-4, 4, n)
    g = torch.Generator().manual_seed(1)
    nd = E.random_dist(b, n, 2, zeros=True)
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(b)])
    t32 = E.c51_loss32(torch.zeros(b, n), z[perm], nd, torch.ones(b), z, -4.0, 4.0)[0]
    want = torch.zeros(b, n).scatter_(1, perm, nd)                            # m[pi(j)] = nd[j]
    assert torch.equal(t32, want) and torch.equal(E.c51_target64(z[perm], nd, z, -4.0, 4.0), want.double())
    shifted = (z[perm] + 1.0)                                                 # one atom up, the top atom clamped onto itself
    want = torch.zeros(b, n).scatter_add_(1, (perm + 1).clamp(max=n - 1), nd)
    got = E.c51_target64(shifted, nd, z, -4.0, 4.0)
    # (two rows of nd meet in the top atom: one float32 add, the same in either order)
    assert torch.equal(got.float(), want) and torch.equal(E.c51_loss32(torch.zeros(b, n), shifted, nd, torch.ones(b), z, -4.0, 4.0)[0], want)


def test_dominated_row_underflows_and_graded_row_straddles_1e_8():
    p = E.dominated_row(9, 3).softmax(dim=-1)
    assert float(p[3]) == 1.0 and int((p == 0.0).sum()) == 8
    assert float(np.exp(np.float32(-120.0))) == 0.0
    assert 0.0 < float(E.softmax64(E.dominated_row(9, 3))[0]) < 1e-50        # ... while float64 keeps it
    p = E.graded_row(9).softmax(dim=-1)
    assert int((p > 1e-8).sum()) >= 4 and int(((p < 1e-8) & (p > 0)).sum()) >= 2
    c = E.dominated_case(False)
    m = E.c51_target64(c["ret"], c["nd"], c["support"], -4.0, 4.0)
    p_taken = c["rows"][c["act"]].softmax(dim=-1)
    assert bool(((m > 0.01) & (p_taken == 0.0)).any(dim=-1).all())             # every row's target sits on p == 0 atoms too


def test_clamp_case_puts_the_mass_on_the_end_atoms():
    c = E.clamp_case()
    ref = E.reference(c)
    r = c["ret"][0]
    assert r[0] == -4 and r[1] == 4 and -4 < r[2] < -3.999 and 3.999 < r[3] < 4 and r[4] < -4 and r[5] > 4 and torch.isinf(r[8])
    m, nd = ref["target"], c["nd"].double()
    assert torch.isfinite(m).all() and torch.isfinite(ref["gbias"]).all() and torch.isfinite(ref["prio"]).all()
    assert float(m[2, 0]) == pytest.approx(float(nd[2].sum()), abs=1e-15) and not m[2, 1:].any()
    assert float(m[3, -1]) == pytest.approx(float(nd[3].sum()), abs=1e-15) and not m[3, :-1].any()
    # float32 oracle: no NaN either, and the +-inf / +-1e6 returns land exactly on the end atoms
    assert torch.isfinite(ref["target32"]).all() and not ref["target32"][3, :-1].any() and not ref["target32"][2, 1:].any()


@pytest.mark.parametrize("kind", [E.QR, E.C51])
@pytest.mark.parametrize("a,tied", [(4, (0, 2)), (5, (3, 4)), (6, (1, 3, 4))])
def test_tie_rows_are_bit_equal_q_values_and_argmax_takes_the_first(kind, a, tied):
    n = 9
    rows = E.tie_rows_qr(a, n, tied) if kind == E.QR else E.tie_rows_c51(a, n, tied)
    z = E.support32(-4, 4, n)
    d, q = E.head32(kind, rows, z)
    terms = (d if kind == E.QR else d * z).numpy()
    seq = np.zeros(a, np.float32)
    for j in range(n):                                                     # one after the other
        seq = (seq + terms[:, j]).astype(np.float32)
    rev = np.zeros(a, np.float32)
    for j in reversed(range(n)):
        rev = (rev + terms[:, j]).astype(np.float32)
    pair = torch.as_tensor(terms).sum(-1).numpy()                          # torch's blocked / pairwise order
    if kind == E.QR:
        seq, rev, pair = seq / np.float32(n), rev / np.float32(n), q.numpy()
    assert np.array_equal(seq, rev) and np.array_equal(seq, pair)
    assert all(seq[i] == seq[tied[0]] for i in tied) and all(seq[i] < seq[tied[0]] for i in range(a) if i not in tied)
    assert int(q.argmax()) == tied[0] == E.head64(kind, rows, z)["act"]
    cfg = OQ.DistQConfig(kind=kind, n_atoms=n, v_min=-4.0, v_max=4.0)
    d_o = OQ.dist(E.edge_params(a, n, rows), cfg, E.obs_batch(3), a)
    assert torch.equal(OQ.q_values(d_o, cfg).argmax(dim=1), torch.full((3,), tied[0]))


def test_unit_distance_case_feeds_exactly_plus_minus_one_and_their_neighbours():
    c = E.qr_unit_case()
    theta = c["rows"][c["act"]].numpy()
    d = np.unique((c["ret"].numpy()[:, None, :] - theta[:, :, None]).astype(np.float32))        # what the kernel computes
    one = np.float32(1.0)
    want = np.array([-np.nextafter(one, np.float32(2)), -one, -np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(0)),
                     one, np.nextafter(one, np.float32(2))], dtype=np.float32)
    assert len(want) == len(np.unique(want)) == 6 and np.array_equal(d, want)
    for r in range(c["B"]):
        assert len(np.unique(c["ret"][r].numpy())) == 6                                          # every row sees all six


def test_qr_closed_forms():
    n, b = 7, 3
    tau = OQ.tau_hat(n)
    theta = E.random_rows(b, n, 1, 0.3)
    w = E.f32([1.0, 0.5, 2.0])
    up = E.qr_loss64(theta, theta.max() + 2.0 + torch.rand(b, n), tau, w)
    dn = E.qr_loss64(theta, theta.min() - 2.0 - torch.rand(b, n), tau, w)
    torch.testing.assert_close(up["dtheta"], -(w.double() / b)[:, None] * tau.double()[None, :].expand(b, -1), rtol=1e-14, atol=0)
    torch.testing.assert_close(dn["dtheta"], (w.double() / b)[:, None] * (1 - tau.double())[None, :].expand(b, -1), rtol=1e-14, atol=0)
    const = torch.full((b, n), 1.25)
    zero = E.qr_loss64(const, const, tau, w)
    assert not zero["dtheta"].any() and not zero["prio"].any() and float(zero["loss"]) == 0.0
    p32, l32, g32 = E.qr_loss32(const, const, tau, w)
    assert not p32.any() and float(l32) == 0.0 and not g32.any()


@pytest.mark.parametrize("a,n", E.RAINBOW_GRID)
def test_rainbow_references_agree_with_the_oracle(a, n, monkeypatch):
    for pattern, b in (("random", 5), ("random", 1), ("dominated", 5), ("on_atom", 3), ("clamp", 4)):
        case = E.rainbow_case(a, n, b, pattern)
        n_ = case["N"]
        r64 = E.rainbow64(case)
        p, noise = E.rainbow_params(case)
        cfg = OQ.DistQConfig(kind="c51", n_atoms=n_, v_min=case["v_min"], v_max=case["v_max"])
        d = ORB.dist(p, noise, case["obs"], a, n_)
        assert bool(((d[0].double() - r64["dist"]).abs() <= r64["dist_bar"] + 2 * E.EPS32 * r64["dist"].max()).all()), pattern
        assert torch.equal(d[0], d[-1])
        monkeypatch.setattr(ORB, "next_dist", lambda *args, **kw: case["nd"].clone())
        st = ORB.RainbowState(p, noise, cfg)
        col: dict = {}
        w = None if case["weight"] is None else case["weight"].numpy()
        loss, ce = ORB.update_with_batch(st, cfg, case["obs"], case["act"].numpy(), case["ret"].numpy(), case["obs"], a, noise, None,
                                         weight=w, collect=col)
        assert bool(((ce.double() - r64["ce"]).abs() <= r64["ce_bar"] + 2 * E.EPS32 * r64["ce"].abs()).all()), pattern
        assert abs(loss - float(r64["loss"])) <= float(r64["loss_bar"]) + 2 * E.EPS32 * abs(float(r64["loss"]))
        assert bool(((col["target_dist"].double() - r64["target"]).abs() <= r64["target_bar"]).all())
        names = dict(bq_mu="Q2.mu_b", bq_sigma="Q2.sigma_b", bv_mu="V2.mu_b", bv_sigma="V2.sigma_b")
        for k, key in names.items():
            g = col["grads"][key].double().reshape(r64["grads"][k].shape)
            slack = 4 * E.EPS32 * r64["grads"][k].abs().max()           # the oracle's F.linear / mean backward adds in another order
            assert bool(((g - r64["grads"][k]).abs() <= r64["grad_bars"][k] + slack).all()), (pattern, k)
        for k in ("conv1.w", "Q0.mu_W", "V0.mu_W", "Q0.sigma_b"):
            assert not col["grads"][k].any(), k
        if a == 1:                                                      # q - mean_a q is exactly 0: the logits ARE the value row
            o32 = r64["o32"]
            bv = case["bv_mu"] + case["bv_sigma"] * case["eps_v"]
            assert torch.equal(o32["logits"][0], bv) and not o32["grads"]["bq_mu"].any() and not o32["grads"]["bq_sigma"].any()
            assert not col["grads"]["Q2.mu_b"].any() and not col["grads"]["Q2.sigma_b"].any()
    z = E.rainbow_case(a, n, 3, zero_noise=True)
    assert torch.equal(E.rainbow32(z, True)["dist"], E.rainbow32(z, False)["dist"])
    assert not E.rainbow32(z)["grads"]["bq_sigma"].any() and not E.rainbow32(z)["grads"]["bv_sigma"].any()
