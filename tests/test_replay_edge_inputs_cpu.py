"""CPU: the inputs of tests/replay_edge_cases.py have the properties tests/test_gpu_replay_edges.py relies on, shown from the
references alone -- the Philox reference reproduces the Random123 known answers, dyadic priorities give exact cumulative sums and
the tie queries equal them, the cdf-tie draws equal entries of the oracle's cdf, every "extreme at position p" case has its unique
extreme at p, every sampler layout has the empty and non-empty sub-buffers it claims, the gather cases take all three routes, and
the Box-Muller float32 deviation behind the GPU bar is the recorded one.  No case is skipped or filtered."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import replay_edge_cases as R


def test_philox_known_answers():
    for ctr, key, out in R.PHILOX_KAT:
        got = R.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert [hex(int(x)) for x in got] == [hex(x) for x in out]
    # vectorised over a batch, and the engine's counter / key layout
    batch = R.philox4x32_10(np.array([k[0] for k in R.PHILOX_KAT], np.uint64), np.array([k[1] for k in R.PHILOX_KAT], np.uint64))
    assert np.array_equal(batch, np.array([k[2] for k in R.PHILOX_KAT], np.uint32))
    ctr, key, out = R.PHILOX_KAT[2]
    b = R.engine_blocks(key[0] | key[1] << 32, ctr[2] | ctr[3] << 32, np.array([ctr[0] | ctr[1] << 32], np.uint64))
    assert np.array_equal(b[0], np.array(out, np.uint32))


def test_uniform_recipes_are_exact():
    w = np.array([0, 1, 31, 32, 0xFFFFFFFF], np.uint32)
    for w0 in w:
        for w1 in w:
            exact = Fraction((int(w0) >> 5) * (1 << 26) + (int(w1) >> 6), 1 << 53)
            assert Fraction(float(R.uniform53(w0, w1))) == exact and exact < 1
    f = R.uniform_f32_ref(257, R.FILL_SEED, R.FILL_COUNTER)
    assert f.dtype == np.float32 and f.min() >= 0.0 and f.max() < 1.0 and np.array_equal(f * 2.0 ** 24, np.round(f * 2.0 ** 24))
    d = R.uniform_f64_ref(257, R.FILL_SEED, R.FILL_COUNTER)
    assert d.min() >= 0.0 and d.max() < 1.0 and len(np.unique(d)) == 257
    assert R.FILL_N_OVER_GRID > 4096 * 256 and R.NORMAL_N_OVER_GRID > 4 * 4096 * 256
    assert R.FILL_SEED >> 32 and R.FILL_COUNTER >> 32 and R.normal_offset(1) >> 32 and R.NORMAL_SEED >> 32     # high words in use


def test_box_muller_deviation_is_the_recorded_one():
    dev = R.normal_f32_deviation()
    print(f"float32 Box-Muller deviation over {sum(R.NORMAL_NS)} draws: {dev!r}; recorded {R.NORMAL_F32_DEV!r}; bar {R.NORMAL_BAR!r}")
    assert R.NORMAL_F32_DEV / 2 <= dev <= R.NORMAL_F32_DEV * 2
    assert R.NORMAL_BAR == 4.0 * R.NORMAL_F32_DEV
    z = np.concatenate([R.normal_ref64(n, R.NORMAL_SEED, R.normal_offset(n)) for n in R.NORMAL_NS])
    assert z.size == sum(R.NORMAL_NS) and np.isfinite(z).all() and 0.8 < z.std() < 1.2 and z.min() < -2 and z.max() > 2
    # the prefix property of the reference itself
    assert np.array_equal(R.normal_ref64(5, 1, 2), R.normal_ref64(1025, 1, 2)[:5])


# ---- sum tree -------------------------------------------------------------------------------------------------------
def test_setitem_updates_hold_the_patterns():
    assert set(R.SETITEM_KS) >= {1, 1023, 1024, 1025, 8192, 8193} and [R.bound_of(s) for s in R.TREE_SIZES] == [1, 2, 4, 64, 4096]
    for size in R.TREE_SIZES:
        for K in R.SETITEM_KS:
            for f32 in (False, True):
                (n0, dup, v0), (n1, single, v1), (n2, ends, v2) = R.setitem_updates(size, K, f32)
                assert (n0, n1, n2) == ("dup", "single", "ends")
                assert v0.dtype == (np.float32 if f32 else np.float64) and v0.size == dup.size == K
                assert all(0 <= i.min() and i.max() < size for i in (dup, single, ends))
                if K > 1:
                    assert len(np.unique(dup)) < K and np.array_equal(dup[K - K // 2:], dup[: K // 2])
                    assert len(np.unique(v1)) == v1.size and len(np.unique(v2)) == K        # a wrong winner shows
                assert len(np.unique(single)) == 1 and single[0] == dup[-1] and single.size == max(1, K // 2)
                assert set(ends) <= {0, size - 1} and size - 1 in ends and (K == 1 or 0 in ends)
    i1, v1, i2, v2 = R.route_agreement_inputs()
    assert i1.size == 8192 and i2.size == 8193 and i2[-1] == i1[-1] and v2[-1] == v1[-1] and np.array_equal(i2[:-1], i1)
    a, b = np.zeros(8192), np.zeros(8192)
    O._setitem(a, i1 + 4096, v1)
    O._setitem(b, i2 + 4096, v2)
    assert np.array_equal(a, b) and a[1] > 0


def test_reduce_ranges_are_all_of_them():
    r = R.reduce_ranges()
    assert len(r) == 13 * 14 // 2 and (0, 13) in r and (12, 13) in r and all(0 <= s < e <= 13 for s, e in r)
    tree, bound = R.reduce_tree()
    assert bound == 16 and O._reduce(tree, bound - 1, 13 + bound) == tree[1]


@pytest.mark.parametrize("size", R.PREFIX_SIZES)
def test_dyadic_priorities_give_exact_sums_and_real_ties(size):
    p = R.dyadic_priorities(size)
    units = [Fraction(float(x)) * 1024 for x in p]
    assert all(u.denominator == 1 and 0 <= u < (1 << 20) for u in units)
    cum = np.cumsum(p)
    exact, run = [], Fraction(0)
    for x in p:
        run += Fraction(float(x))
        exact.append(run)
    assert all(Fraction(float(c)) == e for c, e in zip(cum, exact))                    # every cumulative sum is exact
    tree, bound = R.prefix_tree(size)
    assert bound == R.bound_of(size) and Fraction(float(tree[1])) == exact[-1]
    # parents are exact too, so a query equal to a cumulative sum is an exact tie at some node of its path
    assert np.array_equal(R.rebuild_parents(tree, bound), tree)
    q = R.prefix_queries(size)
    assert np.isin(cum, q).all() and np.isin(np.nextafter(cum, np.inf), q).all() and np.isin(np.nextafter(cum, -np.inf), q).all()
    assert 0.0 in q and cum[-1] in q and np.nextafter(cum[-1], np.inf) in q
    if size >= 64:
        assert (p[:5] == 0).all() and (p[-7:] == 0).all() and p[5] > 0 and p[-8] > 0 and (p[5:-7] == 0).sum() > 10
    if size == 2:
        assert p[0] == 0 and p[1] > 0
    # the tie goes left: a query equal to the cumulative sum up to and including leaf i lands on a leaf <= i
    idx = O._get_prefix_sum_idx(cum.copy(), bound, tree)
    nz = np.flatnonzero(p)
    assert (idx <= np.arange(size)).all() and np.array_equal(idx[nz], nz)
    over = O._get_prefix_sum_idx(np.nextafter(cum[nz[:-1]], np.inf).copy(), bound, tree)
    assert (over > nz[:-1]).all() and (p[over] > 0).all()
    for K in R.PREFIX_KS + (R.PREFIX_K_STRIDE,):
        b = R.prefix_query_batch(size, K)
        assert b.size == K and np.isin(b, q).all()
        if K >= 127:
            assert np.isin(q[:9], b).all() and np.isin(b, cum).sum() >= 9              # named edges and real ties in every batch
    assert R.prefix_query_batch(size, 1)[0] in cum
    assert R.PREFIX_K_STRIDE > 2048 * 128


# ---- PER ------------------------------------------------------------------------------------------------------------
def test_per_sample_cases_put_the_smallest_priority_where_they_say():
    tree, bound, prio = R.per_tree()
    assert prio.argmin() == R.PER_MIN_LEAF and (prio == prio.min()).sum() == 1 and bound == 512
    seen = set()
    for K in R.PER_SAMPLE_KS:
        pos = R.per_sample_positions(K)
        assert pos == sorted({p for p in (0, 63, 64, 1023, 1024, K - 1) if p < K})
        for p in pos:
            u = R.per_sample_u(K, p)
            assert u.shape == (K,) and u.min() >= 0.0 and u.max() < 1.0
            for beta in R.PER_BETAS:
                idx, w = R.per_sample_reference(u, beta, False)
                sampled = prio[idx]
                assert idx[p] == R.PER_MIN_LEAF and (sampled == sampled.min()).sum() == 1 and sampled.argmin() == p
                if beta > 0:
                    assert w.argmax() == p and (w == w.max()).sum() == 1 and w[p] == 1.0
                else:
                    assert (w == 1.0).all()
                wn = R.per_sample_reference(u, beta, True)[1]
                assert wn.max() == 1.0 and np.array_equal(wn, w / w.max())
            if K >= 3:
                assert (u == 0.0).sum() == 1 and (u == np.nextafter(1.0, 0.0)).sum() == 1
                assert idx[u == 0.0][0] == 0 and idx[u.argmax()] == R.PER_SIZE - 1
            seen.add(p)
    assert seen >= {0, 63, 64, 1023, 1024, 2048}


def test_per_update_cases_put_the_extremes_where_they_say():
    eps = np.float32(np.finfo(np.float32).eps)
    seen_max, seen_min, zero_min = set(), set(), 0
    for K in R.PER_UPDATE_KS:
        cases = R.per_update_cases(K)
        for name, idx, td, pmax, pmin in cases:
            assert td.dtype == np.float32 and td.size == idx.size == K and 0 <= idx.min() and idx.max() < R.PER_SIZE
            w = np.abs(td) + eps
            assert w.argmax() == pmax and (w == w.max()).sum() == 1, name
            if K > 1:
                assert w.argmin() == pmin and (w == w.min()).sum() == 1, name
                assert td[pmax] < 0 and (td < 0).sum() > 1 and idx[-1] == idx[0] and td[-1] != td[0], name
            zero_min += int(td[pmin] == 0.0 and w[pmin] == eps)
            seen_max.add(pmax)
            seen_min.add(pmin)
            tree, mm = R.per_update_reference(idx, td)
            assert mm[0] == max(1.0, float(w.max())) and mm[1] == min(1.0, float(w.min())), name
            assert tree[idx[-1] + 512] == float(np.float32(w[-1]) ** np.float32(R.PER_ALPHA)) or K == 1, name     # the last wins
            assert np.array_equal(R.rebuild_parents(tree, 512), tree)
            # a state that already exceeds every new weight does not move
            _, kept = R.per_update_reference(idx, td, (100.0, 1e-9))
            assert np.array_equal(kept, [100.0, 1e-9])
    assert seen_max >= {0, 63, 64, 1023, 1024} and seen_min >= {0, 63, 64, 1023, 1024} and zero_min >= 5


# ---- samplers -------------------------------------------------------------------------------------------------------
def test_sampler_pairs_span_the_sizes():
    assert {e for e, _ in R.SAMPLER_PAIRS} == {1, 2, 64, 65, 512, 513, 1024, 1025, 4096}
    assert {b for _, b in R.SAMPLER_PAIRS} == {1, 1023, 1024, 1025, 4096, 4097, 8193}
    pairs = set(R.SAMPLER_PAIRS)
    # the switch neighbours, each side with a batch on each side of the 4,096-draw round
    assert {(64, 1024), (65, 1025), (64, 4097), (65, 4096), (512, 4096), (513, 4097), (512, 8193), (513, 1024)} <= pairs


@pytest.mark.parametrize("E,bs", R.SAMPLER_PAIRS)
def test_sampler_case_has_the_layout_ties_and_edges_it_claims(E, bs):
    c = R.sampler_case(E, bs)
    off, L, u = c["offset"], c["lengths"], c["u"]
    assert off.size == E + 1 and off[0] == 0 and (np.diff(off) >= np.maximum(L, 1)).all()
    if E == 1:
        assert L[0] > 0
    elif E == 2:
        assert L[0] == 0 and L[1] > 0
    else:
        assert L[0] == 0 and L[-1] == 0 and L[1] > 0 and L[-2] > 0                      # empty first and last, not their neighbours
        z = (L == 0).astype(int)
        runs = np.flatnonzero(np.convolve(z, [1, 1, 1], "valid") == 3)
        assert runs.size >= 2 and (L > 0).sum() > E // 2                                # two runs of three empties
        assert L.max() == R.SAMPLER_LONG and np.sort(L)[-2] <= 8                        # one far longer than the rest
    cdf = R.oracle_cdf(L)
    assert cdf[-1] == 1.0 and u.size == bs and u.min() >= 0.0 and u.max() < 1.0
    ties = np.isin(u, cdf)
    specials = np.concatenate([R.cdf_ties(L), [0.0, np.nextafter(1.0, 0.0)]])
    assert np.isin(specials[:min(bs, specials.size)], u).all()
    if E >= 2:
        assert ties.sum() >= min(bs, R.cdf_ties(L).size) >= 1
        # a tie really takes side="right": the draw lands beyond the sub-buffer whose cdf entry it equals
        t = u[ties][0]
        e = np.flatnonzero(cdf == t)[-1]
        assert cdf.searchsorted(t, side="right") == e + 1 and L[e + 1:][np.flatnonzero(L[e + 1:])[0]] > 0
    sub = R.sub_buffer_of_outputs(L, u)
    assert (L[sub] > 0).all() and sub.max() < E
    assert (c["within_i"] >= 0).all() and (c["within_i"] < L[sub]).all()
    wu = c["within_u"]
    assert (wu == 1.0).sum() == 1 and (wu <= 1.0).all() and (bs < 3 or (0.0 in wu and np.nextafter(1.0, 0.0) in wu))
    ref_w = R.within_from_uniform(L, u, wu)
    assert (ref_w >= 0).all() and (ref_w < L[sub]).all() and ref_w[wu == 1.0][0] == L[sub][wu == 1.0][0] - 1     # the clamp
    # no draw below 1 reaches the clamp, for any length in use (module docstring)
    lens = np.unique(L[L > 0]).astype(np.float64)
    assert (np.floor(np.nextafter(1.0, 0.0) * lens) == lens - 1).all()
    for ref in (c["ref_i"], c["ref_u"]):
        assert ref.shape == (bs,) and (np.diff(np.searchsorted(off, ref, side="right")) >= 0).all()
        s = np.searchsorted(off, ref, side="right") - 1
        assert np.array_equal(s, sub) and (ref - off[s] < L[s]).all()


def test_seeded_reference_uses_both_word_paths():
    assert set(R.SEEDED_ES) == {1, 65, 513} and set(R.SEEDED_BS) == {1, 1024, 4096, 4097, 8193}
    assert R.SEEDED_KEY >> 32 and R.SEEDED_COUNTER >> 32
    for E in R.SEEDED_ES:
        off, L, long_ref = R.seeded_reference(E, 8193)
        sub = np.searchsorted(off, long_ref, side="right") - 1
        assert (np.diff(sub) >= 0).all() and (long_ref - off[sub] < L[sub]).all() and (L[sub] > 0).all()
        if E > 1:
            assert len(np.unique(sub)) > 20 and (L == 0).sum() >= 8
        # swapping the two word pairs, or taking the within draw from the draw's own block order, changes the result
        b = R.engine_blocks(R.SEEDED_KEY, R.SEEDED_COUNTER, np.arange(8193))
        u, wu = R.uniform53(b[:, 0], b[:, 1]), R.uniform53(b[:, 2], b[:, 3])
        swapped = O.sample_indices_random(off, L, wu, R.within_from_uniform(L, wu, u))
        assert not np.array_equal(swapped, long_ref)
        assert not np.array_equal(long_ref[4096:], O.sample_indices_random(off, L, u, R.within_from_uniform(L, u, u))[4096:])
        other = R.seeded_reference(E, 8193, R.SEEDED_KEY, R.SEEDED_COUNTER + 1)[2]
        assert not np.array_equal(other, long_ref)


@pytest.mark.parametrize("E", R.SAMPLE_ALL_ES)
def test_sample_all_cases_mix_wrapped_and_empty(E):
    for empty_ends in (False, True):
        off, L, ins = R.sample_all_case(E, empty_ends)
        assert set(L) <= {0, 1, 4} and (np.diff(off) == 4).all() and off.size == E + 1
        assert ((ins == L) | ((L == 4) & (ins < 4))).all() and (ins >= 0).all()
        if empty_ends:
            assert L[0] == 0 and L[-1] == 0
        wrapped = (L == 4) & (ins > 0)
        if E >= 3:
            assert wrapped.any() and ((L == 4) & (ins == 0)).any() and (L == 1).any() and (empty_ends or E < 63 or (L == 0).any())
        elif not empty_ends:
            assert wrapped.all()
        ref = O.sample_indices_all(off, L, ins)
        assert ref.size == L.sum() and len(np.unique(ref)) == ref.size


def test_small_buffers_are_the_ones_described():
    bufs = R.small_buffers()
    w, p = bufs["wrapped"], bufs["partial"]
    for b in (w, p):
        assert list(np.diff(b["offset"])) == [1, 2, 5] and b["lengths"][0] == 1 and b["lengths"][1] == 0
        q = R.small_queries(b)
        assert set(q % 8) == set(range(8)) and q.min() == -8 and q.max() == 15
    assert w["lengths"][2] == 5 and w["insertion"][2] == 2
    assert w["done"][3 + w["insertion"][2] - 1] and w["done"][3 + 4] and w["done"].sum() == 2
    assert w["last_index"][2] == 3 + w["insertion"][2] - 1
    st = R.small_state(w)
    assert list(st.unfinished_index()) == [0]
    assert list(R.small_state(p).unfinished_index()) == [0, 6]
    assert R.STACKS == (1, 2, 8) and max(R.STACKS) > 5                                  # longer than any episode
    s8 = R.stack_reference(st, np.arange(8), 8)
    assert s8.shape == (8, 8) and np.array_equal(s8[:, -1], np.arange(8)) and np.array_equal(s8[:, -2], st.prev(np.arange(8)))
    assert (s8[:, 0] == s8[:, 1]).all()                                                 # every walk has hit its episode's start
    for stack in (2, 8):
        a = O.sample_indices_stack(st, w["insertion"], stack)
        assert a.size < 6 and (stack == 2) == (a.size > 0)


def test_gather_cases_take_all_three_routes():
    routes = {(o, rb): R.gather_route(o, rb) for o in R.GATHER_BASE_OFFSETS for rb in R.GATHER_ROW_BYTES}
    assert set(R.GATHER_ROW_BYTES) == {1, 3, 4, 12, 16, 20, 48} and set(R.GATHER_BASE_OFFSETS) == {0, 4, 1}
    assert {k for k, v in routes.items() if v == 16} == {(0, 16), (0, 48)}
    assert {k for k, v in routes.items() if v == 4} == {(0, 4), (0, 12), (0, 20), (4, 4), (4, 12), (4, 16), (4, 20), (4, 48)}
    assert all(v == 1 for (o, rb), v in routes.items() if o == 1 or rb in (1, 3))
    for I in R.GATHER_IS:
        idx = R.gather_index(I)
        assert idx.size == I and (I == 0 or (idx.min() >= -R.GATHER_N and idx.max() < R.GATHER_N))
    assert {-R.GATHER_N, -1, 0, R.GATHER_N - 1} <= set(R.gather_index(257))
    assert {R.gather_route(o, rb) for o, rb, _ in R.gather_stride_cases()} == {16, 4, 1}
    for o, rb, I in R.gather_stride_cases():
        assert I * (rb // R.gather_route(o, rb)) > R.GATHER_GRID
        src = R.gather_source(o, rb)
        assert src.size == o + R.GATHER_N * rb and len(np.unique(src[o:].reshape(R.GATHER_N, rb), axis=0)) > R.GATHER_N // 2


def test_permutation_sizes():
    ns = R.permutation_ns()
    assert set(range(1, 71)) <= set(ns) and {15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097} <= set(ns)
