"""CPU checks of tests/redq_edge_cases.py: every shape of tests/test_gpu_redq_edges.py takes the route and the chunking it means
to take, and its inputs can tell a wrong kernel from a right one -- every subset member decides the min target somewhere,
the other reductions and the live critics give another target, members (and therefore chunks) have different gradients and
TD rows, the PER weights move the loss -- each by more than 100 times the bar.  The float32 oracle's own error against float64
(e_ref, what the GPU bars are built from) stays below 1e-3 everywhere; `pytest -s` prints the figures."""
import numpy as np
import pytest
import torch

from tests import redq_edge_cases as R

MARGIN = 100.0
VARIANTS = list(R.update_variants())


def test_route_constants_and_helpers():
    assert R.lds4_bytes(480) == 64 * 480 + 50944 <= R.LDS4_MAX < R.lds4_bytes(512) and R.LDS4_LAST_K1 == 480
    assert R.forward_kernel(5, 480) == "four-wave" and R.forward_kernel(5, 512) == "eight-wave"
    assert R.forward_kernel(1, 32) == "eight-wave" and R.forward_kernel(8, 32) == "four-wave"
    for E, chunks in ((6, [5, 1]), (7, [5, 2]), (10, [5, 5]), (11, [5, 5, 1]), (64, [5] * 12 + [4]), (1, [1]), (5, [5]), (4, [4])):
        assert R.update_chunks(E, 256, 32) == ("fused", chunks)
    assert R.update_chunks(7, 64, 32) == ("per-layer", [1] * 7)
    assert R.update_chunks(7, 256, 32, depth=3)[0] == R.update_chunks(7, 256, 32, depth=1)[0] == "per-layer"
    assert R.update_chunks(6, 256, 1024)[0] == "fused" and R.update_chunks(6, 256, 1056)[0] == "per-layer"
    assert R.target_route(8, 256, 32) == ("multi", "four-wave") and R.target_route(9, 256, 32) == ("two-stream", "eight-wave")
    assert R.target_route(1, 256, 32) == ("single", "eight-wave") and R.target_route(2, 64, 32) == ("two-stream", "per-layer")
    assert R.target_route(8, 256, 1024) == ("multi", "eight-wave")


def test_every_gpu_shape_takes_the_path_it_names():
    seen_chunks, seen_e, seen_b, seen_kc = set(), set(), set(), set()
    for tag, shp, route, chunks in R.UPDATE_SHAPES + [R.COPIED_SHAPE]:
        obs_dim, act_dim, B, E, hidden, _, depth = shp
        kc = R.kc_of(obs_dim, act_dim)
        got = R.update_chunks(E, hidden, kc, depth)
        print(f"  update {tag}: obs {obs_dim} act {act_dim} (kc {kc}) B {B} E {E} hidden {hidden} depth {depth} -> {got[0]}, chunks {got[1]}"
              + (f", {R.forward_kernel(max(got[1]), kc)} forward" if got[0] == "fused" else ""))
        assert got == (route, chunks) and sum(chunks) == E <= R.MAX_ENSEMBLE, tag
        seen_e.add(E), seen_b.add(B), seen_kc.add(kc)
        if route == "fused":
            seen_chunks.add(tuple(chunks))
    # the coverage the issue asks for: two or more chunks, a remainder of 1 and of 2, E = 1, E = 64, B = 1 / 1025, kc = 1024 / 1056
    assert any(len(c) >= 3 for c in seen_chunks) and any(c[-1] == 1 and len(c) > 1 for c in seen_chunks)
    assert any(c[-1] == 2 for c in seen_chunks) and (5, 5) in seen_chunks
    assert {1, 64, R.COPIED_E} <= seen_e and {1, 1023, 1025, 2049} <= seen_b and {32, 64, 1024, 1056} <= seen_kc
    assert R.BATCH_SIZES == (1, R.LOSS_STRIDE - 1, R.LOSS_STRIDE + 1, 2 * R.LOSS_STRIDE + 1)
    # the wide fused case: a chunk of 5 on the eight-wave multi-network forward; every kc = 32 / 64 chunk on the four-wave one
    assert R.forward_kernel(5, R.kc_of(*R.WIDE_FUSED[1][:2])) == "eight-wave" and R.kc_of(*R.WIDE_FUSED[1][:2]) == R.K1_MAX
    assert R.forward_kernel(5, 32) == R.forward_kernel(5, 64) == "four-wave"
    # the action columns of the actor phase
    for (_, shp, _, _), (lo, hi) in zip(R.ACTION_SHAPES, ((30, 33), (15, 47))):
        assert (shp[0], shp[0] + shp[1]) == (lo, hi) and R.kc_of(shp[0], shp[1]) == 64
    seen = set()
    for shp, S, mode, max_action in R.TARGET_CASES:
        obs_dim, act_dim, B, E, hidden, _, depth = shp
        got = R.target_route(S, hidden, R.kc_of(obs_dim, act_dim), depth)
        if (S, hidden, B) not in seen:
            print(f"  target E {E} S {S} B {B} hidden {hidden} -> {got[0]}, {got[1]}")
        seen.add((S, hidden, B))
        assert got == R.TARGET_ROUTES_MEANT[(S, hidden)], (shp, S)
    assert {(8, 256, 1), (8, 256, 300), (9, 256, 1), (9, 256, 300), (10, 64, 300), (1, 256, 300), (1, 64, 300)} <= seen
    assert any(m > 0 for _, _, _, m in R.TARGET_CASES)


def test_subsets_are_unsorted_and_hold_both_ends():
    for E, S in [(10, 2), (10, 8), (10, 9), (10, 10), (64, 5), (2, 2)]:
        s = R.subset(E, S, seed=E + S)
        assert len(set(s.tolist())) == S and 0 in s and E - 1 in s and s.min() >= 0 and s.max() < E
        assert not np.array_equal(s, np.sort(s))
    assert R.subset(10, 1).tolist() == [9] and R.subset(1, 1).tolist() == [0]


def test_case_inputs():
    c = R.case(*R.CHUNK_SHAPES[0][1])
    w = c["weight"]
    assert float(w.min()) > 0.0 and float(w.max()) <= 1.0 and float(w.std()) > 0.1
    for k, v in c["critic"].items():                    # the lagged critics differ by about the spread between members
        spread = float((v[0] - v[1]).std()) if v[0].numel() > 1 else float((v - v.mean()).abs().mean())
        moved = float((c["critic_old"][k] - v).abs().mean())
        assert 0.2 * spread < moved < 5.0 * spread, (k, spread, moved)
    cc = R.copied_case()
    for k, v in cc["critic"].items():
        assert v.shape[0] == R.COPIED_E and torch.equal(v[5:10], v[0:5]) and torch.equal(v[10], v[0])
        assert all(not torch.equal(v[i], v[j]) for i in range(5) for j in range(i))


def _update_case(i):
    if i == len(VARIANTS):
        return R.COPIED_SHAPE[0], R.copied_case(), R.copied_reference(True), True
    tag, shp, weighted, auto = VARIANTS[i]
    return tag, R.case(*shp), R.update_reference(shp, weighted, auto), weighted


@pytest.mark.parametrize("i", range(len(VARIANTS) + 1), ids=[v[0] for v in VARIANTS] + [R.COPIED_SHAPE[0]])
def test_update_inputs_discriminate_and_the_oracle_meets_its_bar(i):
    tag, c, ref, weighted = _update_case(i)
    E, e = c["E"], ref["e_ref"]
    worst = {k if isinstance(k, str) else "/".join(k): float(np.max(v)) for k, v in e.items()}
    print(f"  {tag}: e_ref " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(np.isfinite(v) and v < 1e-3 for v in worst.values()), worst
    assert not R.near_kink_rows(c["actor"], c["critic"], c["obs"], c["act"], c["noise"]).any()       # gradients have a reference
    # PER weights matter
    if weighted:
        d = abs(ref["critic_loss"] - ref["unweighted_loss"]) / abs(ref["critic_loss"])
        assert d > MARGIN * R.rel_bar(e["critic_loss"]), (tag, d)
    # members are distinguishable: the TD rows and every gradient tensor of every pair differ by more than 100 bars of their scale
    # (bq's gradient is ONE number per member, 2 / (E B) sum_b w_b td_b: among up to 2016 pairs two such numbers come close by
    # chance; it is a weighted sum of the TD row checked here and is compared with float64 per member on the GPU.  B = 1 leaves one
    # number per member in the TD row and b2's gradient as well: those are required to differ, at the margin, for E = 6)
    copies = tag == R.COPIED_SHAPE[0]
    same = (lambda i, j: i % R.CHUNK == j % R.CHUNK) if copies else (lambda i, j: False)
    tensors = [("td", ref["td"], max(R.rel_bar(e["weight"]), 1e-5))] + \
              [(k, g.detach().reshape(E, -1), R.rel_bar(float(np.max(e[("critic", k)])))) for k, g in ref["critic_grads"].items() if k != "bq"]
    for name, t, bar in tensors:
        scale = float(t.abs().max())
        for a in range(E):
            dist = (t - t[a]).abs().amax(dim=1) / scale
            for b in range(a):
                if same(a, b):
                    assert float(dist[b]) == 0.0, (tag, name, a, b)
                else:
                    assert float(dist[b]) > MARGIN * bar, (tag, name, a, b, float(dist[b]))


TCASES = R.TARGET_CASES


@pytest.mark.parametrize("i", range(len(TCASES)), ids=[f"E{c[0][3]}-S{c[1]}-{c[2]}-B{c[0][2]}-h{c[0][4]}-max{c[3]}" for c in TCASES])
def test_target_inputs_discriminate_and_the_oracle_meets_its_bar(i):
    shp, S, mode, max_action = TCASES[i]
    c, t = R.case(*shp), R.target_reference(shp, S, mode, max_action)
    E, B, bar = c["E"], c["B"], R.rel_bar(R.target_reference(shp, S, mode, max_action)["e_ref"])
    print(f"  target E {E} S {S} {mode} B {B} hidden {c['hidden']} max_action {max_action}: subset {t['subset'].tolist()}, e_ref {t['e_ref']:.1e}")
    assert t["e_ref"] < 1e-3
    far = lambda other: R.rel_err(other, t["tq"]) > MARGIN * bar  # noqa: E731
    assert far(t["tq_live"]), "critic_old must not be mistaken for critic"
    if S > 1:
        assert far(t["tq_mean"] if mode == "min" else t["tq_min"]), "min and mean targets too close"
        for drop in range(S if B >= 300 else 0):       # a kernel that skips subset position `drop` gives another target
            keep = [k for k in range(S) if k != drop]
            q = t["q_sub"][keep]
            other = (q.min(dim=0)[0] if mode == "min" else q.sum(dim=0) / S) - (t["q_sub"].mean(dim=0) - t["tq_mean"])
            assert far(other), ("position", drop)
    if S < E and (B >= 300 or mode == "mean"):
        assert far(t["tq_all"]), "the subset must not be mistaken for the whole ensemble"
    if mode == "min" and S > 1 and B >= 300:           # every subset member is the arg-min on at least one row
        winners = set(t["q_sub"].argmin(dim=0).tolist())
        assert winners == set(range(S)), (sorted(winners), S)
