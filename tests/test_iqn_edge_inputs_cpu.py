"""CPU checks of tests/iqn_edge_cases.py: the float64 closed forms agree with float64 autograd and with the float32 oracle
(oracle_iqn.update_with_batch, already pinned to the unmodified reference) on the edge networks, the preconditions of the exact
GPU assertions hold (exact logits, ties that tie in float32, greedy gaps, both Huber branches, the tile and share counts of the
embedding shapes, the <= 1 % cap of the large forward), and the float32 oracle's own error against float64 (err32 / e_ref, what
the GPU bars are built from) is measured: `pytest -s` prints the figures quoted in tests/iqn_edge_cases.py."""
import numpy as np
import pytest
import torch

from oracle import oracle_dqn as OD
from tests import iqn_edge_cases as E
from tests import oracle_iqn as OI


def _update_cases():
    for n, np_ in E.LINEAR_SHAPES:
        for sign in (1.0, -1.0):
            yield "linear", f"linear {'+' if sign > 0 else '-'} N{n} N'{np_}", E.linear_case(sign, n, np_)
    yield "unit", "unit", E.unit_case()
    for a, n, np_ in E.MIXED_SHAPES:
        for weighted in (True, False):
            yield "mixed", f"mixed A{a} N{n} N'{np_} {'weighted' if weighted else 'unweighted'}", E.mixed_case(a, n, np_, weighted)
    for b in (1, 1030):
        yield "mean", f"mean B{b}", E.mean_case(b)


def test_float64_references_agree_with_the_oracle_on_the_edge_networks():
    worst: dict = {}
    for group, name, case in _update_cases():
        a, b, n = case["A"], case["B"], case["N"]
        ref = E.reference(case)
        p = E.edge_params(a, case["b2"])
        # the head is the bias, exactly, in every row and for every fraction
        assert torch.equal(OI.logits(p, case["obs"], case["tau"]), case["b2"].view(1, a, 1).expand(b, a, n)), name
        ocfg = OI.IQNConfig()
        col: dict = {}
        w = None if case["weight"] is None else case["weight"].numpy()
        loss, prio = OI.update_with_batch(OD.DQNState.create(p, ocfg.dqn()), ocfg, case["obs"], case["act"].numpy(), case["ret"].numpy(),
                                          case["tau"], weight=w, collect=col)
        for k in OI.PARAM_ORDER:                                            # nothing flows below zero head weights
            if not k.startswith("fc2"):
                assert not col["grads"][k].any(), (name, k)
        # the logits-level float32 formula IS the oracle's (same torch expressions on the same values)
        wt = torch.ones(b) if case["weight"] is None else case["weight"]
        prio32, l32, g32 = E.loss32(case["b2"], case["act"], case["ret"], case["tau"], wt)
        assert torch.equal(prio, prio32) and loss == float(l32), name
        got = dict(prio=prio.double(), loss=torch.tensor(loss, dtype=torch.float64), gbias=col["grads"]["fc2.b"].double())
        for k, v in got.items():
            assert torch.isfinite(v).all(), (name, k)
            # (the oracle's bias gradient adds the rows of one action in F.linear's order: 2 ulp of the scale on top)
            excess = (v - ref[k]).abs() - ref[k + "_bar"] - 2 * E.EPS32 * torch.as_tensor(ref[k + "_scale"])
            assert bool((excess <= 0).all()), (name, k, float(excess.max()))
        taken = set(case["act"].tolist())
        assert all(float(ref["gbias"][i]) == 0.0 and not g32[:, i].any() for i in range(a) if i not in taken)
        units = E.err32_units(ref)
        print(f"{name}: err32 / (eps32 * scale) = " + ", ".join(f"{k} {v:.2f}" for k, v in units.items()))
        for k, v in units.items():
            worst.setdefault(group, {})[k] = max(worst.get(group, {}).get(k, 0.0), v)
            assert v <= 4.0, (name, k, v)                  # the float32 oracle itself stays inside the floor
    for group, u in worst.items():
        print(f"worst of {group}: " + ", ".join(f"{k} {v:.2f}" for k, v in u.items()))


def test_closed_forms_agree_with_float64_autograd():
    for _, name, case in _update_cases():
        b, n = case["B"], case["N"]
        w = torch.ones(b) if case["weight"] is None else case["weight"]
        r = E.iqn_loss64(case["b2"][case["act"]], case["ret"], case["tau"], w)
        theta = case["b2"][case["act"]].double()[:, None].expand(b, n).clone().requires_grad_(True)
        curr, tgt = theta.unsqueeze(2), case["ret"].double().unsqueeze(1)
        diff = torch.nn.functional.smooth_l1_loss(tgt.expand(-1, n, -1), curr.expand(-1, -1, case["Np"]), reduction="none")
        huber = (diff * (case["tau"].double().unsqueeze(2) - (tgt - curr).detach().le(0.0).double()).abs()).sum(-1).mean(1)
        loss = (huber * w.double()).mean()
        loss.backward()
        torch.testing.assert_close(r["huber"], huber.detach(), rtol=1e-13, atol=0)
        torch.testing.assert_close(r["prio"], diff.detach().abs().sum(-1).mean(1), rtol=1e-13, atol=0)
        torch.testing.assert_close(r["loss"], loss.detach(), rtol=1e-13, atol=0)
        assert bool(((r["dtheta"] - theta.grad).abs() <= 1e-13 * r["dtheta_scale"]).all()), name      # (mixed signs cancel)


def test_linear_region_cases_and_their_closed_form():
    for n, np_ in E.LINEAR_SHAPES:
        assert n <= 7 * np_ - 3                                             # the worst case of the roundings fits the bar
        for sign in (1.0, -1.0):
            case = E.linear_case(sign, n, np_)
            ref = E.reference(case)
            d32 = case["ret"] - case["b2"][case["act"]][:, None]            # what the kernel computes, float32
            assert bool((sign * d32 >= 1.0).all()) and bool((sign * ref["d"] >= 1.0).all())
            assert float(case["ret"][1:3].abs().min()) > 9e3                # returns far in the linear region
            assert len(set(case["act"].tolist())) == case["B"]              # one sample per action
            assert float(case["tau"][0, 0]) == 0.0 and float(case["tau"][0, -1]) == E.BELOW_ONE < 1.0 and not case["tau"][3].any()
            want, size = E.linear_closed_form(case, sign)
            torch.testing.assert_close(ref["gbias"], want, rtol=1e-13, atol=1e-300)
            if sign > 0:                                                    # tau = 0 rows: exactly nothing for an under-estimate
                assert float(want[4]) == 0.0 and not ref["dtheta"][3].any() and not ref["dtheta"][:, 0].any()
                assert not ref["grad32"][3].any() and not ref["grad32"][:, :, 0].any()
            else:
                assert bool((want[[0, 1, 2, 4]] > 0).all())
            assert float(want[3]) == 0.0 and float(size[3]) == 0.0          # action 3 is never taken


def test_unit_case_feeds_exactly_plus_minus_one_and_their_neighbours():
    c = E.unit_case()
    theta = c["b2"][c["act"]].numpy()
    assert float(c["b2"][0]) == 0.0 == float(np.round(c["b2"][0]))          # theta is an integer
    d = np.unique((c["ret"].numpy() - theta[:, None]).astype(np.float32))   # what the kernel computes
    one = np.float32(1.0)
    want = np.array([-np.nextafter(one, np.float32(2)), -one, -np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(0)),
                     one, np.nextafter(one, np.float32(2))], dtype=np.float32)
    assert len(np.unique(want)) == 6 and np.array_equal(d, want)
    for r in range(c["B"]):
        row = c["ret"][r].numpy()
        assert len(np.unique(row)) == 6                                     # every row sees all six:
        assert (np.abs(row) < 1).any() and (np.abs(row) >= 1).any() and (row > 0).any() and (row < 0).any()      # both branches, both signs
    assert float(c["tau"][0, 0]) == 0.0 and float(c["tau"][0, -1]) == E.BELOW_ONE


@pytest.mark.parametrize("a,n,np_", E.MIXED_SHAPES)
def test_mixed_cases_cover_both_sides_and_both_branches(a, n, np_):
    c = E.mixed_case(a, n, np_, True)
    d = E.reference(c)["d"]
    assert bool((d > 0).any()) and bool((d < 0).any()) and bool((d.abs() < 1).any()) and bool((d.abs() > 1).any())
    assert [float(x) for x in c["weight"]] == list(E.MIXED_WEIGHT) and E.MIXED_WEIGHT[0] == E.MIXED_WEIGHT[3] == 0.0
    ref = E.reference(c)
    assert not ref["dtheta"][0].any() and not ref["dtheta"][3].any() and not ref["grad32"][0].any() and not ref["grad32"][3].any()
    if a >= 3:                                                              # action 0 belongs to the zero-weight row 0 alone
        assert c["act"].tolist().count(0) == 1 and float(ref["gbias"][0]) == 0.0
    unweighted = E.reference(E.mixed_case(a, n, np_, False))
    assert bool(unweighted["dtheta"][0].any()) and float(unweighted["loss"]) != float(ref["loss"])


def test_head_biases_exact_logits_gaps_and_q_err32():
    worst = 0.0
    for a in E.HEAD_A:
        for n in E.HEAD_N:
            for shift in (0.0, -20.0):
                b2 = E.head_bias(a, n, 3 + a + n, shift)
                h = E.head64(b2)
                q32 = E.head32(b2, n)
                u = float(((q32.double() - h["q"]).abs() / (E.EPS32 * h["q_scale"]).clamp_min(1e-300)).max())
                worst = max(worst, u)
                assert u <= 4.0, (a, n, u)
                # the GPU test compares the greedy action with float64's at every one of these shapes: the gap must allow it
                assert E.greedy_gap(h) > E.GREEDY_GAP_ULPS, (a, n, shift, E.greedy_gap(h))
                assert int(q32.argmax()) == h["act"]
                if shift < 0:
                    assert bool((b2 < 0).all())                             # every Q negative: a padding column (0.0) would win
                if n > 7:                                                   # multiples of 2^-10 below 2^5: N = 64 sums are exact
                    assert torch.equal(b2 * 1024.0, torch.round(b2 * 1024.0)) and float(b2.abs().max()) < 32.0
                    seq = np.float32(0.0)
                    for _ in range(n):
                        seq = np.float32(seq + b2.numpy()[0])
                    assert seq / np.float32(n) == b2.numpy()[0]
    b2 = E.head_bias(33, 7, 5, -20.0)
    lg, q, act = OI.policy_forward(E.edge_params(33, b2), E.obs_batch(5, 3), torch.rand(5, 7))
    assert torch.equal(lg, b2.view(1, 33, 1).expand(5, 33, 7)) and bool((act == E.head64(b2)["act"]).all())
    print(f"forward Q: worst err32 / (eps32 * scale) = {worst:.2f}")


@pytest.mark.parametrize("a,tied", E.TIES)
def test_tie_biases_tie_in_float32_and_argmax_takes_the_first(a, tied):
    for negative in (False, True):
        b2 = E.tie_bias(a, tied, negative)
        assert E.head64(b2)["act"] == tied[0]
        for n in E.HEAD_N:
            q = E.head32(b2, n)
            seq = np.zeros(a, np.float32)
            for _ in range(n):                                              # one after the other, as the kernel adds them
                seq = (seq + b2.numpy()).astype(np.float32)
            assert np.array_equal((seq / np.float32(n)).astype(np.float32), b2.numpy()) and torch.equal(q, b2)    # exact in any order
            assert all(q[i] == q[tied[0]] for i in tied) and all(q[i] < q[tied[0]] for i in range(a) if i not in tied)
            assert int(q.argmax()) == tied[0] and (not negative or bool((q < 0).all()))
        lg, q, act = OI.policy_forward(E.edge_params(a, b2), E.obs_batch(3, 4), torch.rand(3, 7))
        assert bool((act == tied[0]).all())


def test_embedding_shapes_walk_their_row_tile_loops_more_than_once():
    """Recomputed from BM = 64, FWD_SHARES = 16 and BWD_SLABS = 8: a later change of those constants cannot silently turn the
    route tests back into single-tile ones."""
    assert (E.BM, E.FWD_SHARES, E.BWD_SLABS, E.FUSED_FROM_ROWS) == (64, 16, 8, 16384)
    for b, n, f in E.FWD_SHAPES + [E.BOUNDARY_FUSED, E.BOUNDARY_UNFUSED]:
        tiles, shares = E.fwd_tiles(b, n)
        assert tiles > shares and f % 64 == 0, (b, n, f)                    # some share walks two tiles or more
    assert E.fwd_tiles(157, 7) == (18, 16) and 157 * 7 == 17 * 64 + 11      # 18 tiles over 16 shares, a partial last tile
    assert any(f % 128 == 64 for _, _, f in E.FWD_SHAPES) and {64, 192} <= {f for _, _, f in E.FWD_SHAPES}
    assert any((b * n) % E.BM for b, n, _ in E.FWD_SHAPES)
    for b, n, f in E.BWD_SHAPES + [E.BOUNDARY_FUSED, E.BOUNDARY_UNFUSED]:
        tiles, shares, sb = E.bwd_tiles(b, n)
        assert tiles > shares and f in (64, 128), (b, n, f)
    assert E.bwd_tiles(157, 7) == (18, 8, 9) and 157 - 17 * 9 == 4          # ... a last tile of 4 samples
    assert E.bwd_tiles(19, 33) == (19, 8, 1) and 33 < E.BM                  # one half-empty tile per sample
    assert E.BOUNDARY_FUSED[0] * E.BOUNDARY_FUSED[1] == E.FUSED_FROM_ROWS == E.BOUNDARY_UNFUSED[0] * E.BOUNDARY_UNFUSED[1] + 1
    u, fw = E.ENGINE_UPDATE, E.ENGINE_FORWARD
    assert u["B"] * u["N"] == 16448 >= E.FUSED_FROM_ROWS and fw["B"] * fw["N"] == E.FUSED_FROM_ROWS
    assert E.fwd_tiles(u["B"], u["N"])[0] > E.FWD_SHARES and E.bwd_tiles(u["B"], u["N"])[0] > E.BWD_SLABS


def test_embedding_references_and_their_e_ref():
    for b, n, f in E.FWD_SHAPES + [E.BOUNDARY_FUSED, E.BOUNDARY_UNFUSED]:
        d, ref = E.embed_inputs(b, n, f, False), E.embed_reference(b, n, f, False)
        flat = d["tau"].reshape(-1)
        last = flat[(b * n - 1) // E.BM * E.BM:]                            # the fractions of the last row tile
        assert bool((last == 0.0).any()) and bool((last == E.BELOW_ONE).any()) and float(flat.max()) < 1.0
        pre = E.cos64(d["tau"]) @ d["we"].double().t() + d["be"].double()
        assert bool((pre < 0).any()) and bool((pre > 0).any())              # the ReLU mask matters
        print(f"embed forward {(b, n, f)}: float32 e_ref {ref['e_x']:.2e}, bar {E.rel_bar(ref['e_x']):.2e}")
        assert ref["e_x"] < 1e-5
    for b, n, f in E.BWD_SHAPES + [E.BOUNDARY_FUSED, E.BOUNDARY_UNFUSED]:
        d, ref = E.embed_inputs(b, n, f, True), E.embed_reference(b, n, f, True)
        pre = E.cos64(d["tau"]) @ d["we"].double().t() + d["be"].double()
        assert float(pre.abs().min()) >= 2e-6                               # off the kink: the gradient has a reference
        # the closed forms against float64 autograd
        f_, w_, b_ = (t.double().clone().requires_grad_(True) for t in (d["feat"], d["we"], d["be"]))
        (f_.repeat_interleave(n, dim=0) * torch.relu(E.cos64(d["tau"]) @ w_.t() + b_)).backward(d["dx"].double())
        torch.testing.assert_close(ref["dfeat"], f_.grad * (d["feat"] > 0), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ref["dwe"], w_.grad.t(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ref["dbe"], b_.grad, rtol=1e-12, atol=1e-12)
        print(f"embed backward {(b, n, f)}: float32 e_ref " + ", ".join(f"{k} {ref['e_' + k]:.2e}" for k in ("dfeat", "dwe", "dbe")))
        assert all(np.isfinite(ref["e_" + k]) and ref["e_" + k] < 1e-4 for k in ("dfeat", "dwe", "dbe"))


def test_engine_update_case_on_the_fused_route():
    c = E.engine_update_case()
    s = E.ENGINE_UPDATE
    assert tuple(c["tau"].shape) == (s["B"], s["N"]) and tuple(c["ret"].shape) == (s["B"], s["Np"])
    assert bool((c["d"].abs() < 1).any()) and bool((c["d"].abs() > 1).any())                # both Huber branches
    assert list(c["parts"]) == ["conv1", "conv2", "conv3", "We", "be", "W1", "b1", "W2", "b2"] and c["parts"]["b2"][1] == c["grad"].numel()
    print("engine update, float32 oracle e_ref: " + ", ".join(f"{k} {v:.2e}" for k, v in c["e_ref"].items()))
    for k, v in c["e_ref"].items():
        assert np.isfinite(v) and v < 1e-4, (k, v)                          # the widened bar stays a tight one
    for k, (lo, hi) in c["parts"].items():
        assert float(c["grad"][lo:hi].abs().max()) > 0, k


def test_engine_forward_case_leaves_out_at_most_one_percent():
    c = E.engine_forward_case()
    left_out = 1.0 - float(c["clear"].double().mean())
    print(f"engine forward, float32 oracle e_ref: logits {c['e_ref']['logits']:.2e}, q {c['e_ref']['q']:.2e}; "
          f"rows left out for a too-small gap: {100 * left_out:.2f} %")
    assert left_out <= 0.01
    assert c["e_ref"]["logits"] < 1e-5 and c["e_ref"]["q"] < 1e-5
    assert torch.equal(c["act32"][c["clear"]], c["act"][c["clear"]])        # the float32 reference alone meets the condition
    assert len(set(c["act"].tolist())) > 1                                  # ... and the greedy action does vary
