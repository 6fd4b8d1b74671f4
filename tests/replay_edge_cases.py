"""Inputs and plain references for the replay data path at its switch points: the sum tree and the PER kernels
(tianshou_amd/csrc/ts_segtree.hip), the samplers, index math, gathers, the Feistel permutation and the Philox fills
(tianshou_amd/csrc/ts_index.hip).  tests/test_replay_edge_inputs_cpu.py shows on the CPU that the inputs have the properties
claimed here; tests/test_gpu_replay_edges.py runs the kernels against the references.

References: oracle/oracle.py wherever it covers the operation (`_setitem`, `_reduce`, `_get_prefix_sum_idx`, `per_get_weight`,
`per_update_weight`, `sample_indices_all`, `sample_indices_random`, `sample_indices_stack`, `_prev_index`, `_next_index`,
`unfinished_index`), NumPy fancy indexing for the gathers, and -- for the engine's own random streams -- the Philox-4x32-10 below,
written from the round definition of Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11, sec. 3.3 /
the Random123 `philox4x32` bijection) and pinned to the Random123 known-answer vectors by the CPU file:

    one round, counter (c0, c1, c2, c3), key (k0, k1), M0 = 0xD2511F53, M1 = 0xCD9E8D57:
        (hi0, lo0) = M0 * c0,  (hi1, lo1) = M1 * c2   (32 x 32 -> 64 bit)
        counter' = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)
    ten rounds; between rounds the key is bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85).

How the engine keys it (read from buffer.py / ts_index.hip / ts_common.h, restated in `engine_blocks`): counter = (index low, index
high, stream low, stream high), key = (seed low, seed high).  `sample_indices(bs, seed=(key, counter))` passes seed = key and
stream = counter; output position k of the seeded sampler takes its sub-buffer draw from words 0-1 and its within-buffer draw from
words 2-3 of block k (`uniform53`: 27 + 26 bits -> a double in [0, 1)).

Switch points and the cases that sit on either side of them
-----------------------------------------------------------

    switch                                   below / at                          above
    sampler histogram, E <= 64 ballots       sampler_case(64, 1024), (64, 4097)   sampler_case(65, 1025), (65, 4096)
                                             seeded_case(1, *)                    seeded_case(65, *)
    sampler LDS staging, E <= 512            sampler_case(512, 4096), (512, 8193) sampler_case(513, 4097), (513, 1024)
                                             seeded_case(65, *)                   seeded_case(513, *)
    kept Philox words, first 4,096 outputs   seeded_case(E, 4096), (E, 1024)      seeded_case(E, 4097), (E, 8193)
    supplied draws, 4,096 per round          sampler_case(65, 4096), (512, 4096)  sampler_case(64, 4097), (513, 4097)
    sub-buffer limit, E <= 4096              sampler_case(4096, 8193), (4096, 1)  E = 4097 (refused)
    set-item stride, K <= 1024               setitem K = 1023, 1024               setitem K = 1025
    set-item bulk path, K <= 8192            setitem K = 8192                     setitem K = 8193; route agreement
    tree bound                               tree size 1 (bound 1), 2 (bound 2)   tree sizes 3, 64, 3000 (bounds 4, 64, 4096)
    prefix grid stride, 2048 x 128 queries   prefix K = 1, 127, 128, 129          prefix K = 2048 * 128 + 1
    PER wave / stride, 64 lanes, 1024        per K = 1, 63, 64 / 1024             per K = 65 / 1025, 2049
    lengths prefix, 1024 per round           sample_all E = 1023, 1024            sample_all E = 1025, 2049
    gather route                             rows 16, 48 at offset 0 (16-byte); rows 4, 12, 20 at offset 0 and 4, 12, 16, 20, 48 at
                                             offset 4 (4-byte); rows 1, 3 anywhere and every row at offset 1 (1-byte)
    fill grid cap, 4096 x 256                fill n = 1, 255, 256, 257            fill n = 4096 * 256 + 3 (f32 and f64);
                                                                                  normal fill n = 4 * 4096 * 256 + 5

The within_u clamp.  `slot = floor(u * len); if slot >= len: slot = len - 1`.  For a double u < 1 the product never rounds up to
len: u <= 1 - 2^-53, so u * len <= len - len * 2^-53, and for len in (2^k, 2^(k+1)) the spacing of doubles below len is 2^(k-52),
of which len * 2^-53 is more than half (a power of two len makes the product exact).  `nextafter(1, 0)` is in every within_u
case and the CPU file checks that it stays below len for every length used; the clamp itself is reached with u = 1.0 exactly, the
closed end a host-supplied draw can carry, and that value is in every within_u case as well.

Box-Muller bar.  `normal_ref64` evaluates ts::normal4's formula in float64 on the Philox words, `normal_ref32` the same formula in
NumPy float32 (float32 2 pi, float32 log / sqrt / sin / cos).  Over the 2,061 draws of NORMAL_NS (one stream offset per n) the
largest absolute float32 deviation from float64 is NORMAL_F32_DEV = 9.613206114478245e-07 as measured on the development
machine; the GPU bar is NORMAL_BAR = 4 * NORMAL_F32_DEV = 3.845282445791298e-06.  (NumPy's float32 transcendental functions
differ by an ulp between SIMD targets, so the CPU file checks that the deviation it computes lies within a factor of two of the
recorded one; the bar itself is the constant.)
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O

# ---------------------------------------------------------------------------------------------------------------------
# Philox-4x32-10
# ---------------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)

# Random123 known answers: (counter, key, output)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(counter, key) -> np.ndarray:
    """counter uint32[..., 4], key uint32[..., 2] (broadcast against each other) -> uint32[..., 4]."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2                     # 32 x 32 -> 64 bit: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _M32, (p0 >> _S32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + PHILOX_W0) & _M32, (k1 + PHILOX_W1) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def engine_blocks(seed: int, stream: int, index) -> np.ndarray:
    """The engine's block for every element of `index`: counter (index, stream) as two 64-bit halves, key = seed."""
    index = np.asarray(index, dtype=np.uint64)
    ctr = np.stack([index & _M32, index >> _S32, np.full_like(index, stream & 0xFFFFFFFF), np.full_like(index, stream >> 32)], -1)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def uniform53(w0, w1) -> np.ndarray:
    """NumPy's random_sample recipe: 27 + 26 bits -> a double in [0, 1); every step is exact in float64."""
    a, b = (np.asarray(w0, np.uint32) >> np.uint32(5)).astype(np.float64), (np.asarray(w1, np.uint32) >> np.uint32(6)).astype(np.float64)
    return (a * 67108864.0 + b) * (1.0 / 9007199254740992.0)


def uniform_f64_ref(n: int, seed: int, counter: int) -> np.ndarray:
    b = engine_blocks(seed, counter, np.arange(n))
    return uniform53(b[:, 0], b[:, 1])


def uniform_f32_ref(n: int, seed: int, counter: int) -> np.ndarray:
    """24 bits of word 0 -> k * 2^-24 (exact in float32)."""
    b = engine_blocks(seed, counter, np.arange(n))
    return ((b[:, 0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


FILL_NS = (1, 255, 256, 257)
FILL_N_OVER_GRID = 4096 * 256 + 3
FILL_SEED, FILL_COUNTER = 0x0123456789ABCDEF, 0xFEDCBA9876543211


def _normal(n: int, seed: int, offset: int, ft):
    q = np.arange((n + 3) // 4)
    b = engine_blocks(seed, offset, q)
    z = np.zeros((q.size, 4), ft)
    two_pi = ft(6.28318530717958647692)
    for p in range(2):
        # u1 in (0, 1], u2 in [0, 1): 24 bits each, exact in float32 and float64
        u1 = ((b[:, 2 * p] >> np.uint32(8)).astype(ft) + ft(1.0)) * ft(2.0 ** -24)
        u2 = (b[:, 2 * p + 1] >> np.uint32(8)).astype(ft) * ft(2.0 ** -24)
        rad = np.sqrt(ft(-2.0) * np.log(u1))
        z[:, 2 * p] = rad * np.cos(two_pi * u2)
        z[:, 2 * p + 1] = rad * np.sin(two_pi * u2)
    assert z.dtype == ft
    return z.reshape(-1)[:n]


def normal_ref64(n: int, seed: int, offset: int) -> np.ndarray:
    return _normal(n, seed, offset, np.float64)


def normal_ref32(n: int, seed: int, offset: int) -> np.ndarray:
    return _normal(n, seed, offset, np.float32)


NORMAL_NS = (1, 3, 4, 5, 1023, 1025)
NORMAL_SEED = 0x5EED0000DEADBEEF
NORMAL_N_OVER_GRID = 4 * 4096 * 256 + 5
NORMAL_F32_DEV = 9.613206114478245e-07
NORMAL_BAR = 4.0 * NORMAL_F32_DEV


def normal_offset(n: int) -> int:
    return (1 << 33) + n          # one stream per n; bit 33 reaches the counter's high word


def normal_f32_deviation() -> float:
    return max(float(np.abs(normal_ref32(n, NORMAL_SEED, normal_offset(n)).astype(np.float64)
                            - normal_ref64(n, NORMAL_SEED, normal_offset(n))).max()) for n in NORMAL_NS)


# ---------------------------------------------------------------------------------------------------------------------
# sum tree
# ---------------------------------------------------------------------------------------------------------------------
def bound_of(size: int) -> int:
    b = 1
    while b < size:
        b *= 2
    return b


SETITEM_KS = (1, 1023, 1024, 1025, 8192, 8193)
TREE_SIZES = (1, 2, 3, 64, 3000)


def setitem_updates(size: int, K: int, f32: bool, seed: int = 0):
    """Three successive (name, index int64[k], value) updates of one tree.
    'dup': K random leaves, the last K // 2 repeating the first K // 2 (later entries win);
    'single': max(1, K // 2) entries, all on the leaf of the LAST entry of 'dup' -- a winner table left dirty by 'dup' holds K - 1
              there, more than any position of this update, so every one of its writes would be dropped;
    'ends': K entries on leaf 0 and leaf size - 1 only."""
    rng = np.random.default_rng([size, K, int(f32), seed])
    vt = np.float32 if f32 else np.float64

    def values(k):                      # distinct, so that a wrong winner among duplicates shows
        if f32:
            return ((rng.permutation(k) + 1) * 3).astype(np.float32) * np.float32(2.0 ** -12)
        return rng.random(k) * 4.0 + 2.0 ** -20

    dup = rng.integers(0, size, size=K)
    dup[K - K // 2:] = dup[: K // 2]
    k2 = max(1, K // 2)
    single = np.full(k2, dup[-1], np.int64)
    ends = np.where(rng.random(K) < 0.5, 0, size - 1).astype(np.int64)
    ends[0], ends[-1] = 0, size - 1
    if K == 1:
        ends[0] = size - 1
    return [("dup", dup.astype(np.int64), values(K)), ("single", single, values(k2)), ("ends", ends, values(K))]


def route_agreement_inputs(size: int = 3000):
    """8,192 entries (one-workgroup path) and the same plus a repeat of the last (8,193: bulk path)."""
    rng = np.random.default_rng(77)
    idx = rng.integers(0, size, size=8192)
    idx[4096:] = idx[:4096]
    val = rng.random(8192)
    return idx, val, np.concatenate([idx, idx[-1:]]), np.concatenate([val, val[-1:]])


REDUCE_SIZE = 13


def reduce_tree():
    rng = np.random.default_rng(13)
    bound = bound_of(REDUCE_SIZE)
    tree = np.zeros(2 * bound)
    O._setitem(tree, np.arange(REDUCE_SIZE) + bound, rng.random(REDUCE_SIZE) * 3.0)
    return tree, bound


def reduce_ranges():
    return [(s, e) for s in range(REDUCE_SIZE) for e in range(s + 1, REDUCE_SIZE + 1)]


PREFIX_SIZES = (1, 2, 3000)            # bounds 1, 2, 4096
PREFIX_KS = (1, 127, 128, 129)
PREFIX_K_STRIDE = 2048 * 128 + 1


def dyadic_priorities(size: int) -> np.ndarray:
    """Integer multiples of 2^-10 below 2^10: every partial sum is an integer below 2^32 in units of 2^-10, exact in float64 in
    any order.  Zero leaves: a run at the start, a run just before the padding, and scattered ones (size 3000)."""
    rng = np.random.default_rng(size)
    p = rng.integers(1, 1 << 20, size=size).astype(np.float64) * 2.0 ** -10
    if size == 2:
        p[0] = 0.0
    if size >= 64:
        p[:5] = 0.0
        p[-7:] = 0.0
        p[rng.integers(5, size - 7, size=size // 10)] = 0.0
    return p


def prefix_tree(size: int):
    bound = bound_of(size)
    tree = np.zeros(2 * bound)
    O._setitem(tree, np.arange(size) + bound, dyadic_priorities(size))
    return tree, bound


def prefix_queries(size: int) -> np.ndarray:
    """Every cumulative sum, each +- one ulp, 0.0, the total, one ulp over the total; the named edges first, the rest shuffled, so
    that the first K of them hold the edges for every K >= 9."""
    p = dyadic_priorities(size)
    cum = np.cumsum(p)
    total = cum[-1]
    nz = np.flatnonzero(p)
    head = [0.0, total, np.nextafter(total, np.inf), cum[0], cum[nz[0]], np.nextafter(cum[nz[0]], -np.inf),
            np.nextafter(cum[nz[0]], np.inf), cum[nz[-1]], np.nextafter(cum[nz[-1]], -np.inf)]
    rest = np.concatenate([cum, np.nextafter(cum, -np.inf), np.nextafter(cum, np.inf)])
    np.random.default_rng(size + 1).shuffle(rest)
    q = np.concatenate([np.array(head), rest])
    if size == 1:                       # K = 1 on the one-leaf tree: the tie itself
        q = np.concatenate([cum, q])
    return q


def prefix_query_batch(size: int, K: int) -> np.ndarray:
    q = prefix_queries(size)
    return np.resize(q, K).copy()


# ---------------------------------------------------------------------------------------------------------------------
# PER
# ---------------------------------------------------------------------------------------------------------------------
PER_SIZE, PER_MIN_LEAF = 300, 137
PER_ALPHA = 0.6
PER_SAMPLE_KS = (1, 63, 64, 65, 1024, 1025, 2049)
PER_BETAS = (0.0, 0.4, 1.0)
PER_UPDATE_KS = (1, 63, 65, 1024, 1025)
PER_POSITIONS = (0, 63, 64, 1023, 1024)


@functools.lru_cache(maxsize=None)
def _per_tree():
    rng = np.random.default_rng(11)
    prio = rng.integers(64, 1024, size=PER_SIZE).astype(np.float64) / 64.0     # >= 1, dyadic
    prio[PER_MIN_LEAF] = 2.0 ** -4                                               # the unique smallest priority
    bound = bound_of(PER_SIZE)
    tree = np.zeros(2 * bound)
    O._setitem(tree, np.arange(PER_SIZE) + bound, prio)
    return tree, bound, prio


def per_tree():
    tree, bound, prio = _per_tree()
    return tree.copy(), bound, prio.copy()


def per_sample_positions(K: int):
    return sorted({p for p in PER_POSITIONS + (K - 1,) if p < K})


def per_sample_u(K: int, p: int) -> np.ndarray:
    """K draws: position p lands on PER_MIN_LEAF (the smallest priority = the largest weight), every other position on another
    leaf; for K >= 3 one other position is u = 0.0 and one is nextafter(1, 0)."""
    _, _, prio = _per_tree()
    rng = np.random.default_rng([K, p])
    cum = np.cumsum(prio)
    others = np.delete(np.arange(PER_SIZE), PER_MIN_LEAF)
    leaf = rng.choice(others, size=K)
    leaf[p] = PER_MIN_LEAF
    u = (cum[leaf] - prio[leaf] * rng.uniform(0.1, 0.9, size=K)) / cum[-1]
    if K >= 3:
        free = [k for k in (0, 1, 2, K - 2) if k != p]
        u[free[0]], u[free[1]] = 0.0, np.nextafter(1.0, 0.0)
    return u


def per_sample_reference(u, beta: float, weight_norm: bool):
    """prio.py:63-67 (u * total, prefix search), :69-79 (weight), :104-106 (normalisation) on the oracle's leaves."""
    tree, bound, prio = _per_tree()
    v = np.ascontiguousarray(np.asarray(u, np.float64) * tree[1])
    idx = O._get_prefix_sum_idx(v, bound, tree)
    return idx, O.per_get_weight(tree, bound, idx, float(prio.min()), beta, weight_norm)


def per_update_cases(K: int):
    """(name, index, td float32, pmax, pmin): the running max at pmax (a negative TD error), the running min at pmin (an exact
    0.0 in every other case, so that eps alone is the priority); entry K - 1 repeats the leaf of entry 0 with another value."""
    pos = sorted({p for p in PER_POSITIONS + (K - 1,) if p < K})
    out = []
    if K == 1:
        for name, v in (("K1 max", -7.5), ("K1 zero", 0.0)):
            out.append((name, np.array([5], np.int64), np.array([v], np.float32), 0, 0))
        return out
    for n, p in enumerate(pos):
        other = (p + K // 2) % K
        for which in ("max", "min"):
            pmax, pmin = (p, other) if which == "max" else (other, p)
            rng = np.random.default_rng([K, p, int(which == "max")])
            td = ((rng.random(K) * 0.9 + 0.1) * rng.choice([-1.0, 1.0], size=K)).astype(np.float32)
            td[pmax] = -7.5
            td[pmin] = 0.0 if (n + (which == "max")) % 2 == 0 else -(2.0 ** -6)
            idx = rng.integers(0, PER_SIZE, size=K)
            idx[K - 1] = idx[0]
            out.append((f"K{K} {which} at {p}", idx.astype(np.int64), td, pmax, pmin))
    return out


def per_update_reference(index, td, state=(1.0, 1.0)):
    tree, bound, _ = per_tree()
    mx, mn = O.per_update_weight(tree, bound, index, np.asarray(td, np.float32), PER_ALPHA, state[0], state[1])
    return tree, np.array([mx, mn])


def rebuild_parents(tree: np.ndarray, bound: int) -> np.ndarray:
    """The tree's own leaves under parents summed left + right, level by level (segtree.py:98-101)."""
    t = tree.copy()
    n = bound
    while n > 1:
        n //= 2
        t[n:2 * n] = t[2 * n:4 * n:2] + t[2 * n + 1:4 * n:2]
    return t


# ---------------------------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------------------------
SAMPLER_PAIRS = ((1, 1), (1, 8193), (2, 1023), (64, 1024), (65, 1025), (64, 4097), (65, 4096), (512, 4096), (513, 4097),
                 (512, 8193), (513, 1024), (1024, 1025), (1025, 1023), (4096, 8193), (4096, 1))
SAMPLER_LONG = 5000


def sampler_layout(E: int):
    """-> (offset int64[E + 1], lengths int64[E]).  E >= 64: empty sub-buffers first, last and in two runs, one sub-buffer far
    longer than the rest.  E = 2: the first one empty.  E = 1: nothing can be empty."""
    rng = np.random.default_rng(1000 + E)
    if E == 1:
        L = np.array([7], np.int64)
    elif E == 2:
        L = np.array([0, 5], np.int64)
    else:
        L = rng.integers(1, 9, size=E).astype(np.int64)
        L[0] = L[-1] = 0
        L[E // 3:E // 3 + 3] = 0
        L[-6:-3] = 0
        L[E // 2] = SAMPLER_LONG
    cap = np.maximum(L, 1) + rng.integers(0, 3, size=E)
    return np.concatenate([[0], np.cumsum(cap)]).astype(np.int64), L


def oracle_cdf(lengths) -> np.ndarray:
    """The cdf of O.sample_indices_random (NumPy's legacy choice), operation for operation."""
    lengths = np.asarray(lengths, np.int64)
    p = lengths / lengths.sum()
    cdf = p.cumsum()
    cdf /= cdf[-1]
    return cdf


def cdf_ties(lengths) -> np.ndarray:
    """Up to six distinct cdf entries below 1 (first two, two in the middle, last two): u equal to one of them takes side='right'."""
    t = np.unique(oracle_cdf(lengths))
    t = t[t < 1.0]
    if t.size > 6:
        t = t[[0, 1, t.size // 2, t.size // 2 + 1, t.size - 2, t.size - 1]]
    return t


def sampler_u(E: int, bs: int) -> np.ndarray:
    _, L = sampler_layout(E)
    rng = np.random.default_rng([E, bs, 1])
    special = np.concatenate([cdf_ties(L), [0.0, np.nextafter(1.0, 0.0)]])
    u = rng.random(bs)
    m = min(bs, special.size)
    u[rng.choice(bs, size=m, replace=False)] = special[:m]
    return u


def sub_buffer_of_outputs(lengths, u) -> np.ndarray:
    """The sub-buffer every OUTPUT position belongs to: the draws' sub-buffers, sorted (the output is grouped by sub-buffer)."""
    return np.sort(oracle_cdf(lengths).searchsorted(np.asarray(u, np.float64), side="right"))


def within_from_uniform(lengths, u, wu) -> np.ndarray:
    """floor(wu * len) of the output position's sub-buffer, clamped to len - 1 (only wu = 1.0 reaches the clamp)."""
    L = np.asarray(lengths, np.int64)[sub_buffer_of_outputs(lengths, u)]
    return np.minimum(np.floor(np.asarray(wu, np.float64) * L.astype(np.float64)).astype(np.int64), L - 1)


def sampler_case(E: int, bs: int) -> dict:
    """u_buffer plus both kinds of within draws, and the oracle's result for each."""
    offset, L = sampler_layout(E)
    u = sampler_u(E, bs)
    rng = np.random.default_rng([E, bs, 2])
    Lj = L[sub_buffer_of_outputs(L, u)]
    within_i = np.floor(rng.random(bs) * Lj).astype(np.int64)
    wu = rng.random(bs)
    edge = rng.choice(bs, size=min(bs, 3), replace=False)
    for j, (wi_v, wu_v) in zip(edge, ((Lj[edge[0]] - 1, 1.0), (0, 0.0), (None, np.nextafter(1.0, 0.0)))):
        if wi_v is not None:
            within_i[j] = min(wi_v, Lj[j] - 1)
        wu[j] = wu_v
    return dict(E=E, bs=bs, offset=offset, lengths=L, u=u, within_i=within_i, within_u=wu,
                ref_i=O.sample_indices_random(offset, L, u, within_i),
                ref_u=O.sample_indices_random(offset, L, u, within_from_uniform(L, u, wu)))


SEEDED_ES = (1, 65, 513)
SEEDED_BS = (1, 1024, 4096, 4097, 8193)
SEEDED_KEY, SEEDED_COUNTER = 0x1234567890ABCDEF, 0xFEDCBA9800000007


def seeded_reference(E: int, bs: int, key: int = SEEDED_KEY, counter: int = SEEDED_COUNTER):
    """sample_indices(bs, seed=(key, counter)): block k = Philox(counter = (k, counter), key = key); words 0-1 choose draw k's
    sub-buffer, words 2-3 are the within-buffer draw of OUTPUT position k."""
    offset, L = sampler_layout(E)
    b = engine_blocks(key, counter, np.arange(bs))
    u, wu = uniform53(b[:, 0], b[:, 1]), uniform53(b[:, 2], b[:, 3])
    return offset, L, O.sample_indices_random(offset, L, u, within_from_uniform(L, u, wu))


SAMPLE_ALL_ES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
SAMPLE_ALL_CAP = 4


def sample_all_case(E: int, empty_ends: bool):
    """Capacity-4 sub-buffers with lengths from {0, 1, 4}; a full one is wrapped (insertion 1..3 < len) or not (insertion 0), a
    partly filled one has insertion == len."""
    rng = np.random.default_rng([E, int(empty_ends)])
    L = rng.choice([0, 1, 4], size=E).astype(np.int64)
    if E >= 3:
        L[1], L[E // 2] = 4, 1
    if empty_ends:
        L[0] = L[-1] = 0
    elif E == 1:
        L[0] = 4
    ins = np.where(L == 4, rng.integers(0, 4, size=E), L).astype(np.int64)
    if E >= 3 and not empty_ends:
        L[0], ins[0], ins[1] = 4, 3, 0                     # a wrapped one first, an unwrapped full one next
    elif E == 1 and not empty_ends:
        ins[0] = 2
    offset = np.arange(E + 1, dtype=np.int64) * SAMPLE_ALL_CAP
    return offset, L, ins


# ---------------------------------------------------------------------------------------------------------------------
# prev / next / stack / unfinished
# ---------------------------------------------------------------------------------------------------------------------
STACKS = (1, 2, 8)


def small_buffers():
    """E = 3, capacities 1, 2, 5.  Sub-buffer 0 has length 1, sub-buffer 1 is empty.
    'wrapped': sub-buffer 2 is full with insertion 2: done on the slot before the insertion point (= its last index) and on its
    last slot.  'partial': sub-buffer 2 holds 4 of 5 slots, done in the middle only, so its newest episode is unfinished."""
    offset = np.array([0, 1, 3, 8], np.int64)
    done_w = np.zeros(8, bool)
    done_w[[3 + 1, 3 + 4]] = True
    done_p = np.zeros(8, bool)
    done_p[3 + 1] = True
    return {
        "wrapped": dict(offset=offset, lengths=np.array([1, 0, 5], np.int64), insertion=np.array([0, 0, 2], np.int64),
                        last_index=np.array([0, 1, 3 + 1], np.int64), done=done_w),
        "partial": dict(offset=offset, lengths=np.array([1, 0, 4], np.int64), insertion=np.array([0, 0, 4], np.int64),
                        last_index=np.array([0, 1, 3 + 3], np.int64), done=done_p),
    }


def small_state(b: dict) -> O.BufferState:
    B = int(b["offset"][-1])
    return O.BufferState(b["offset"], b["last_index"], b["lengths"], b["insertion"], np.zeros(B), b["done"], np.zeros(B, bool))


def small_queries(b: dict) -> np.ndarray:
    B = int(b["offset"][-1])
    return np.arange(-B, 2 * B, dtype=np.int64)          # every slot three times over: negative, plain, wrapped past the end


def stack_reference(st: O.BufferState, index, stack: int) -> np.ndarray:
    """buffer_base.py:586-596: column stack - 1 - j = prev^j(index), the last column the index as passed."""
    cols, idx = [np.asarray(index, np.int64)], np.asarray(index, np.int64)
    for _ in range(stack - 1):
        idx = st.prev(idx)
        cols.insert(0, idx)
    return np.stack(cols, axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# gathers, permutation
# ---------------------------------------------------------------------------------------------------------------------
GATHER_ROW_BYTES = (1, 3, 4, 12, 16, 20, 48)
GATHER_BASE_OFFSETS = (0, 4, 1)
GATHER_IS = (0, 1, 257)
GATHER_N = 37
GATHER_GRID = 4096 * 256


def gather_route(base_offset: int, row_bytes: int) -> int:
    """Bytes per element of the route ts_gather_rows takes for a source `base_offset` bytes past a 16-byte boundary (the output
    is a fresh allocation, 16-byte aligned)."""
    a = base_offset | row_bytes
    return 16 if a % 16 == 0 else 4 if a % 4 == 0 else 1


def gather_source(base_offset: int, row_bytes: int) -> np.ndarray:
    """uint8[base_offset + GATHER_N * row_bytes]: the rows start at byte base_offset."""
    return np.random.default_rng([base_offset, row_bytes]).integers(0, 256, size=base_offset + GATHER_N * row_bytes, dtype=np.uint8)


def gather_index(I: int) -> np.ndarray:
    idx = np.random.default_rng(I).integers(-GATHER_N, GATHER_N, size=I)
    edge = [-GATHER_N, -1, 0, GATHER_N - 1]
    idx[:min(I, 4)] = edge[:min(I, 4)]
    return idx.astype(np.int64)


def gather_stride_cases():
    """(base_offset, row_bytes, I) with I * row_vecs above the grid cap, one per route."""
    return [(0, 48, GATHER_GRID // 3 + 7), (4, 4, GATHER_GRID + 3), (1, 1, GATHER_GRID + 3)]


def permutation_ns():
    return sorted(set(range(1, 71)) | {4 ** k + d for k in range(2, 7) for d in (-1, 0, 1)})
