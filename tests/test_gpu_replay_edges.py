"""GPU: the replay data path -- sum tree and PER kernels (ts_segtree.hip), samplers, index math, gathers, the Feistel
permutation and the Philox fills (ts_index.hip) -- at the sizes where the kernels switch behaviour and on exact ties, against the
references of tests/replay_edge_cases.py (its docstring lists the switch points and the cases on either side of each;
tests/test_replay_edge_inputs_cpu.py shows that the inputs are what they claim to be).

Everything is compared exactly (array_equal / torch.equal) except: PER importance weights at rtol 1e-12 and PER leaves at
rtol 5e-7 (the bars of test_per_weights_against_reference_vectors: device pow / powf against the host's), and ts_normal_fill at
NORMAL_BAR = four times the float32 Box-Muller deviation of the reference itself.

Measured on an MI355X: the 179 tests of this file take 2.2 s of wall time (tests/test_gpu_index_segtree.py: 30 tests, 3.1 s).
ts_normal_fill against the float64 Box-Muller, largest |engine - float64| per n (bar 3.845e-06): n = 1: 1.4e-08, 3: 1.5e-07,
4: 2.2e-08, 5: 1.1e-07, 1023: 8.5e-07, 1025: 9.6e-07; n = 2^22 + 5: 1.8e-06 against that stream's own bar of 7.3e-06.

What these tests found.  No index, tie, wave-position or route error in the sum tree, PER, sampler, index-math, gather or
permutation kernels.  Three faults at the edges of the fills and of the wrapper:
  * uniform_fill_f64_kernel and normal_fill_kernel were launched on a grid capped at 4,096 workgroups but had no stride loop, so
    ts_uniform_fill_f64 left every output past 2^20 and ts_normal_fill every output past 2^22 unwritten, without an error
    (test_uniform_fills_match_the_philox_reference[1048579], test_normal_fill_past_the_grid_cap; both fail against the earlier
    kernels).  Both kernels loop now, like uniform_fill_f32_kernel.
  * DeviceReplayBuffer.sample_indices(batch_size > 0) returned an empty tensor on a buffer whose sub-buffers are all empty; the
    reference's RandomState.choice raises there (p = lengths / 0).  It raises ValueError now
    (test_supplied_draw_sampler_refusals).
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import replay_edge_cases as R

pytestmark = pytest.mark.gpu


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def make_buffer(offset, lengths, insertion=None, last_index=None, done=None):
    from tianshou_amd.buffer import DeviceReplayBuffer

    E, B = len(lengths), int(offset[-1])
    return DeviceReplayBuffer(offset=offset, last_index=offset[:-1] if last_index is None else last_index, lengths=lengths,
                              insertion=np.zeros(E, np.int64) if insertion is None else insertion, rew=np.zeros(B),
                              terminated=np.zeros(B, bool) if done is None else done, truncated=np.zeros(B, bool))


# ---- sum tree -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("K", R.SETITEM_KS)
@pytest.mark.parametrize("size", R.TREE_SIZES)
def test_setitem_three_updates_bit_exact(size, K, f32):
    from tianshou_amd import segtree as S

    t = S.SegmentTree(size)
    assert t._bound == R.bound_of(size)
    ref = np.zeros(2 * t._bound)
    for name, idx, val in R.setitem_updates(size, K, f32):
        t[dev(idx)] = dev(val)
        O._setitem(ref, idx + t._bound, val)
        assert np.array_equal(host(t._value), ref), name


def test_setitem_routes_agree_bit_for_bit():
    from tianshou_amd import segtree as S

    i1, v1, i2, v2 = R.route_agreement_inputs()
    a, b = S.SegmentTree(3000), S.SegmentTree(3000)
    a[dev(i1)] = dev(v1)                    # 8,192 entries: one workgroup
    b[dev(i2)] = dev(v2)                    # 8,193 entries: chip-wide leaf phase + one launch per level
    assert torch.equal(a._value, b._value)
    ref = np.zeros(2 * a._bound)
    O._setitem(ref, i1 + a._bound, v1)
    assert np.array_equal(host(a._value), ref)


def test_setitem_workspace_reuse_across_bounds():
    from tianshou_amd import segtree as S

    small, big = S.SegmentTree(64), S.SegmentTree(3000)
    refs = {id(small): np.zeros(128), id(big): np.zeros(8192)}
    rng = np.random.default_rng(5)
    for t, K in ((small, 500), (big, 9000), (small, 40), (big, 700), (small, 9000)):
        idx = rng.integers(0, len(t), size=K)
        val = rng.random(K)
        t[dev(idx)] = dev(val)
        O._setitem(refs[id(t)], idx + t._bound, val)
        assert np.array_equal(host(t._value), refs[id(t)]), (len(t), K)


def test_reduce_every_range_of_a_13_leaf_tree():
    from tianshou_amd import segtree as S

    ref, bound = R.reduce_tree()
    t = S.SegmentTree(R.REDUCE_SIZE)
    t._value.copy_(dev(ref))
    got = torch.stack([t.reduce(s, e) for s, e in R.reduce_ranges()])
    want = np.array([O._reduce(ref, s + bound - 1, e + bound) for s, e in R.reduce_ranges()])
    assert np.array_equal(host(got), want)
    assert float(t.reduce()) == ref[1] == O._reduce(ref, bound - 1, R.REDUCE_SIZE + bound)
    assert float(t.reduce(3)) == O._reduce(ref, 3 + bound - 1, R.REDUCE_SIZE + bound)
    assert float(t.reduce(2, -1)) == O._reduce(ref, 2 + bound - 1, R.REDUCE_SIZE - 1 + bound)


@pytest.mark.parametrize("K", R.PREFIX_KS + ("all", R.PREFIX_K_STRIDE))
@pytest.mark.parametrize("size", R.PREFIX_SIZES)
def test_prefix_search_on_exact_ties(size, K):
    from tianshou_amd import segtree as S

    ref, bound = R.prefix_tree(size)
    q = R.prefix_queries(size) if K == "all" else R.prefix_query_batch(size, K)
    want_v = q.copy()
    want_i = O._get_prefix_sum_idx(want_v, bound, ref)
    v = dev(q)
    got = S._get_prefix_sum_idx(v, bound, dev(ref))
    assert np.array_equal(host(got), want_i)
    assert np.array_equal(host(v), want_v, equal_nan=False)            # the query array is mutated like the reference's
    t = S.SegmentTree(size)                                                # and through the class, which leaves its input alone
    t._value.copy_(dev(ref))
    v2 = dev(q)
    assert np.array_equal(host(t.get_prefix_sum_idx(v2)), want_i) and np.array_equal(host(v2), q)


# ---- PER ------------------------------------------------------------------------------------------------------------
def _per(weight_norm=True, beta=0.4):
    from tianshou_amd import segtree as S

    tree, bound, prio = R.per_tree()
    per = S.PrioritizedWeights(R.PER_SIZE, R.PER_ALPHA, beta, weight_norm)
    per.weight._value.copy_(dev(tree))
    per.prio_minmax.copy_(dev(np.array([prio.max(), prio.min()])))
    return per


@pytest.mark.parametrize("K", R.PER_SAMPLE_KS)
def test_per_sample_with_the_largest_weight_at_every_wave_position(K):
    for weight_norm in (True, False):
        for beta in R.PER_BETAS:
            per = _per(weight_norm, beta)
            for p in R.per_sample_positions(K):
                u = R.per_sample_u(K, p)
                want_i, want_w = R.per_sample_reference(u, beta, weight_norm)
                idx, w = per.sample(u)
                tag = (K, p, beta, weight_norm)
                assert idx.dtype == torch.int64 and np.array_equal(host(idx), want_i), tag
                np.testing.assert_allclose(host(w), want_w, rtol=1e-12, atol=0.0, err_msg=str(tag))
                if weight_norm:
                    assert float(w.max()) == 1.0, tag
                    assert beta == 0.0 or (int(w.argmax()) == p and int((w == 1.0).sum()) == 1), tag


@pytest.mark.parametrize("K", R.PER_UPDATE_KS)
def test_per_update_weight_with_the_extremes_at_every_wave_position(K):
    for name, idx, td, pmax, pmin in R.per_update_cases(K):
        for state in ((1.0, 1.0), (100.0, 1e-9)):
            per = _per()
            per.prio_minmax.copy_(dev(np.array(state)))
            per.update_weight(dev(idx), dev(td))
            want_tree, want_mm = R.per_update_reference(idx, td, state)
            got = host(per.weight._value)
            assert np.array_equal(host(per.prio_minmax), want_mm), (name, state)       # float32 arithmetic widened: exact
            if state[0] == 100.0:
                assert np.array_equal(host(per.prio_minmax), np.array(state)), name     # nothing new exceeds it: it does not move
            bound = per.weight._bound
            np.testing.assert_allclose(got[bound:], want_tree[bound:], rtol=5e-7, atol=0.0, err_msg=name)   # device powf vs host
            touched = np.zeros(bound, bool)
            touched[idx] = True
            assert np.array_equal(got[bound:][~touched], want_tree[bound:][~touched]), name
            # the parents, exactly: the device's own leaves under left + right sums
            assert np.array_equal(got, R.rebuild_parents(got, bound)), name


# ---- samplers -------------------------------------------------------------------------------------------------------
def _sample_raw(buf, u, within_i=None, within_u=None):
    """ts_sample_indices_random through the C ABI (the wrapper offers no within_u with supplied sub-buffer draws)."""
    from tianshou_amd import _lib

    bs = u.numel()
    out = torch.full((bs,), -7, dtype=torch.int64, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.load().ts_sample_indices_random(
        _lib.ptr(buf.offset), _lib.i64(buf.buffer_num), _lib.ptr(buf.lengths), _lib.ptr(u), _lib.ptr(within_i), _lib.ptr(within_u),
        _lib.i64(bs), _lib.ptr(out), _lib.ptr(err), _lib.current_stream(buf.device)))
    return out, int(err.item())


@pytest.mark.parametrize("E,bs", R.SAMPLER_PAIRS)
def test_supplied_draw_sampler(E, bs):
    c = R.sampler_case(E, bs)
    buf = make_buffer(c["offset"], c["lengths"])
    out = buf.sample_indices(bs, u_buffer=c["u"], within=c["within_i"])
    assert out.dtype == torch.int64 and np.array_equal(host(out), c["ref_i"])
    out_u, err = _sample_raw(buf, dev(c["u"]), within_u=dev(c["within_u"]))
    assert err == 0 and np.array_equal(host(out_u), c["ref_u"])
    out_i, err = _sample_raw(buf, dev(c["u"]), within_i=dev(c["within_i"]))
    assert err == 0 and np.array_equal(host(out_i), c["ref_i"])


def test_supplied_draw_sampler_refusals():
    from tianshou_amd import _lib

    off = np.arange(4098, dtype=np.int64)
    with pytest.raises(_lib.EngineError) as e:
        make_buffer(off, np.ones(4097, np.int64)).sample_indices(4, u_buffer=np.full(4, 0.5), within=np.zeros(4, np.int64))
    assert e.value.code == _lib.TS_ERR_UNSUPPORTED
    with pytest.raises(_lib.EngineError) as e:
        make_buffer(off, np.ones(4097, np.int64)).sample_indices(4, seed=(1, 2))
    assert e.value.code == _lib.TS_ERR_UNSUPPORTED
    # manager.py:220-224: lengths / lengths.sum() is 0 / 0, RandomState.choice refuses the probabilities
    empty = make_buffer(np.array([0, 3, 6], np.int64), np.zeros(2, np.int64))
    with pytest.raises(ValueError):
        empty.sample_indices(4, u_buffer=np.full(4, 0.5), within=np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        empty.sample_indices(4, seed=(1, 2))
    assert empty.sample_indices(0).numel() == 0 and empty.sample_indices(-1).numel() == 0
    c = R.sampler_case(65, 1025)
    buf = make_buffer(c["offset"], c["lengths"])
    sub = R.sub_buffer_of_outputs(c["lengths"], c["u"])
    for j in (0, 1024):
        bad = c["within_i"].copy()
        bad[j] = c["lengths"][sub[j]]                          # one past the last slot of its sub-buffer
        with pytest.raises(ValueError):
            buf.sample_indices(1025, u_buffer=c["u"], within=bad)
    bad = c["within_i"].copy()
    bad[512] = -1
    with pytest.raises(ValueError):
        buf.sample_indices(1025, u_buffer=c["u"], within=bad)


@pytest.mark.parametrize("bs", R.SEEDED_BS)
@pytest.mark.parametrize("E", R.SEEDED_ES)
def test_seeded_sampler_matches_the_philox_reference(E, bs):
    off, L, want = R.seeded_reference(E, bs)
    buf = make_buffer(off, L)
    got = buf.sample_indices(bs, seed=(R.SEEDED_KEY, R.SEEDED_COUNTER))
    assert got.dtype == torch.int64 and np.array_equal(host(got), want)
    assert int(buf._err.item()) == 0


@pytest.mark.parametrize("n", R.FILL_NS + (R.FILL_N_OVER_GRID,))
def test_uniform_fills_match_the_philox_reference(n):
    from tianshou_amd.dqn import uniform_draws
    from tianshou_amd.iqn import uniform_fractions

    f = uniform_fractions(n, R.FILL_SEED, R.FILL_COUNTER)
    assert f.dtype == torch.float32 and np.array_equal(host(f), R.uniform_f32_ref(n, R.FILL_SEED, R.FILL_COUNTER))
    d = uniform_draws(n, (R.FILL_SEED, R.FILL_COUNTER))
    assert d.dtype == torch.float64 and np.array_equal(host(d), R.uniform_f64_ref(n, R.FILL_SEED, R.FILL_COUNTER))


@pytest.mark.parametrize("n", R.NORMAL_NS)
def test_normal_fill_against_float64_box_muller(n):
    from tianshou_amd.buffer import normal_noise

    z = normal_noise((n,), R.NORMAL_SEED, R.normal_offset(n))
    want = R.normal_ref64(n, R.NORMAL_SEED, R.normal_offset(n))
    err = float(np.abs(host(z).astype(np.float64) - want).max())
    print(f"normal fill n={n}: max |engine - float64| = {err:.3e}, bar {R.NORMAL_BAR:.3e}")
    assert z.dtype == torch.float32 and err <= R.NORMAL_BAR
    longer = normal_noise((1025,), R.NORMAL_SEED, R.normal_offset(n))         # same seed and offset, another n: the same prefix
    assert torch.equal(longer[:n], z)


def test_normal_fill_past_the_grid_cap():
    from tianshou_amd.buffer import normal_noise

    n = R.NORMAL_N_OVER_GRID
    z = host(normal_noise((n,), R.NORMAL_SEED, 9)).astype(np.float64)
    want = R.normal_ref64(n, R.NORMAL_SEED, 9)
    # the bar of this stream, derived like NORMAL_BAR: four times the float32 deviation of the reference over these draws
    bar = 4.0 * float(np.abs(R.normal_ref32(n, R.NORMAL_SEED, 9).astype(np.float64) - want).max())
    err, tail = float(np.abs(z - want).max()), float(np.abs(z - want)[1 << 22:].max())
    print(f"normal fill n={n}: max |engine - float64| = {err:.3e} (past 2^22: {tail:.3e}), bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("empty_ends", [False, True], ids=["mixed", "empty_ends"])
@pytest.mark.parametrize("E", R.SAMPLE_ALL_ES)
def test_sample_all_indices(E, empty_ends):
    off, L, ins = R.sample_all_case(E, empty_ends)
    buf = make_buffer(off, L, insertion=ins, last_index=off[:-1] + (ins - 1) % np.maximum(L, 1))
    got = buf.sample_indices(0)
    assert got.dtype == torch.int64 and np.array_equal(host(got), O.sample_indices_all(off, L, ins))


@pytest.mark.parametrize("which", ["wrapped", "partial"])
def test_prev_next_stack_unfinished_on_a_tiny_buffer(which):
    from tianshou_amd.dqn import stack_indices

    b = R.small_buffers()[which]
    st = R.small_state(b)
    buf = make_buffer(b["offset"], b["lengths"], b["insertion"], b["last_index"], b["done"])
    q = R.small_queries(b)
    args = (b["offset"], b["done"], b["last_index"], b["lengths"])
    assert np.array_equal(host(buf.prev(dev(q))), O._prev_index(q, *args))
    assert np.array_equal(host(buf.next(dev(q))), O._next_index(q, *args))
    assert np.array_equal(host(buf.unfinished_index()), O.unfinished_index(*args))
    assert np.array_equal(host(buf.sample_indices(0)), st.sample_indices_all())
    for stack in R.STACKS:
        assert np.array_equal(host(stack_indices(buf, dev(q), stack)), R.stack_reference(st, q, stack)), stack
        if stack >= 2:
            assert np.array_equal(host(buf.sample_indices_stacked(0, stack)), O.sample_indices_stack(st, b["insertion"], stack)), stack


# ---- gathers, permutation ---------------------------------------------------------------------------------------------
def _gather(base_offset, row_bytes, index):
    from tianshou_amd.buffer import gather_rows

    raw = R.gather_source(base_offset, row_bytes)
    d = dev(raw)
    src = d[base_offset:].view(R.GATHER_N, row_bytes)
    assert src.is_contiguous() and src.data_ptr() % 16 == base_offset           # the base the case claims
    out = gather_rows(src, dev(index))
    assert out.dtype == torch.uint8 and out.shape == (index.size, row_bytes) and out.data_ptr() % 16 == 0
    return host(out), raw[base_offset:].reshape(R.GATHER_N, row_bytes)[index]


@pytest.mark.parametrize("base_offset", R.GATHER_BASE_OFFSETS)
@pytest.mark.parametrize("row_bytes", R.GATHER_ROW_BYTES)
def test_gather_rows_on_every_route(row_bytes, base_offset):
    for I in R.GATHER_IS:
        got, want = _gather(base_offset, row_bytes, R.gather_index(I))
        assert np.array_equal(got, want), I


@pytest.mark.parametrize("base_offset,row_bytes,I", R.gather_stride_cases())
def test_gather_rows_past_the_grid_cap(base_offset, row_bytes, I):
    got, want = _gather(base_offset, row_bytes, R.gather_index(I))
    assert np.array_equal(got, want)


def test_random_permutation_is_a_bijection_at_every_small_size():
    from tianshou_amd.buffer import random_permutation

    for n in R.permutation_ns():
        p, again, other = random_permutation(n, seed=77), random_permutation(n, seed=77), random_permutation(n, seed=78)
        assert p.dtype == torch.int64 and torch.equal(torch.sort(p).values, torch.arange(n, device="cuda")), n
        assert torch.equal(torch.sort(other).values, torch.arange(n, device="cuda")), n
        assert torch.equal(p, again), n
        assert n < 8 or not torch.equal(p, other), n
