// ts_atom_head.h -- what the MLP kernels with N atoms per action share (ts_qrdqn_mlp.hip: quantiles, ts_c51_mlp.hip: the logits of a
// softmax) on the 32-row tile of ts_mlp_tile.h: the network description, the trunk, the A N wide head walked ACTION BY ACTION (action
// a's N columns are ceil(N / 32) MFMA column blocks whose weight loads are masked past column N, so the LDS footprint does not depend
// on A and N needs no alignment), its masked weight and input gradients, the eight-lane row sum and the launch helpers.  Moved here
// from ts_qrdqn_mlp.hip as they were; softmax_row from ts_c51_mlp.hip, for ts_rainbow_mlp.hip as well.  Flat parameter vector: per layer [K + 1, N] (row K = bias), trunk layers then the head
// [top + 1, A N], column a N + j.  Include behind `#pragma clang fp contract(off)`.
#pragma once

#include <algorithm>
#include <cstring>

#include "ts_mlp_tile.h"

namespace {

constexpr int MAX_TRUNK = 4, MAX_ATOMS = 256, MAX_ACT = 32;
constexpr int RPT = 8;                      // threads per row in the row-wise passes (THREADS / TILE)
static_assert(RPT * TILE == THREADS, "thread (row, t) = (tid >> 3, tid & 7)");

struct QNet {
    int obs_dim, n_act, n_atoms, nt;
    Lay t[MAX_TRUNK], head;                 // head: K = top width, N = n_act * n_atoms
    int x_at, t_at[MAX_TRUNK];              // LDS float offsets of obs and of every hidden activation
    int ta_at, tb_at, row_at, pitch;        // two [32][pitch] tables (pitch = n_atoms | 1), per-row scalars [4][32]
    int P, lds_floats;
};

// the trunk on the tile whose observations are in LDS -> the top activation (LDS) and its pitch.  Ends behind a barrier.
__device__ const float* trunk_forward(const QNet& net, const float* __restrict__ p, float* sm, int* ptop) {
    const float* x = sm + net.x_at;
    int px = net.obs_dim + 1;
    for (int l = 0; l < net.nt; ++l) {
        float* y = sm + net.t_at[l];
        dense_relu(p + net.t[l].off, net.t[l].K, net.t[l].N, x, px, y, net.t[l].N + 1);
        __syncthreads();
        x = y; px = net.t[l].N + 1;
    }
    *ptop = px;
    return x;
}

// out[m][c] = top[m][:] W[:, aN + c] + b[aN + c], c < N.  ROWSEL: only the rows with sel[m] == a are stored.
template <bool ROWSEL>
__device__ void head_action(const QNet& net, const float* __restrict__ p, int a, const float* top, int ptop, float* out, const int* sel) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int K = net.head.K, N = net.n_atoms, ld = net.head.N, pt = net.pitch;
    const float* w = p + net.head.off + a * N;
    for (int cb = wave; cb < (N + 31) / 32; cb += 4) {
        const int c = cb * 32 + i;
        const bool live = c < N;
        const float* wp = w + (live ? c : 0);               // past column N: the action's first column is read, 0 is used
        const float* xp = top + i * ptop + h;
        f32x16 acc = {};
#pragma unroll 8
        for (int k = 0; k < K; k += 2) {                    // (K is a hidden width: even)
            const float b = wp[(size_t)(k + h) * ld];
            acc = mfma32(xp[k], live ? b : 0.f, acc);
        }
        const float bias = wp[(size_t)K * ld];
        if (live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = featF(r, h);
                if (!ROWSEL || sel[m] == a) out[m * pt + c] = acc[r] + bias;
            }
        }
    }
}

// the eight partial sums of a row (lanes 8 row .. 8 row + 7 of a wave) in a fixed butterfly: all eight threads hold the same bits
__device__ __forceinline__ float row_sum8(float s) {
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    return s;
}

// softmax of a row of N logits in place, thread t of the row's eight on the atoms i = t (mod 8) -> the expected value sum_i p_i z_i
__device__ __forceinline__ float softmax_row(float* mine, int N, int t, const float* __restrict__ z) {
    float mx = -INFINITY;
    for (int i = t; i < N; i += RPT) mx = fmaxf(mx, mine[i]);
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    mx = fmaxf(mx, __shfl_xor(mx, 4));
    float s = 0.f;
    for (int i = t; i < N; i += RPT) {
        const float e = expf(mine[i] - mx);
        mine[i] = e;                                     // only this thread reads atom i
        s += e;
    }
    s = row_sum8(s);
    float q = 0.f;
    for (int i = t; i < N; i += RPT) {
        const float p = mine[i] / s;
        mine[i] = p;
        q += p * z[i];
    }
    return row_sum8(q);
}

// the head's part of the slab: for action a the columns [aN, aN + N) of rows 0 .. K (row K = bias) = sum over the rows m with
// sel[m] == a of top[m][k] dth[m][c]; an absent action's columns are zeros
__device__ void head_wgrad(const QNet& net, float* __restrict__ slab, const float* top, int ptop, const float* dth, const int* sel, unsigned present) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int K = net.head.K, N = net.n_atoms, ld = net.head.N, pt = net.pitch;
    const int cbs = (N + 31) / 32, kbs = K / 32;
    for (int a = 0; a < net.n_act; ++a) {
        float* sa = slab + a * N;
        if (!((present >> a) & 1)) {                                           // workgroup-uniform
            for (int idx = threadIdx.x; idx < (K + 1) * N; idx += THREADS) {
                const int k = idx / N, c = idx - k * N;
                sa[(size_t)k * ld + c] = 0.f;
            }
            continue;
        }
        for (int blk = wave; blk < kbs * cbs; blk += 4) {
            const int kb = blk / cbs, cb = blk - kb * cbs;
            const int kc = kb * 32 + i, c = cb * 32 + i;
            const bool live = c < N;
            const float* zp = dth + (live ? c : 0);
            f32x16 acc = {};
#pragma unroll
            for (int m = 0; m < TILE; m += 2) {
                const float z = zp[(m + h) * pt];
                acc = mfma32(top[(m + h) * ptop + kc], live && sel[m + h] == a ? z : 0.f, acc);
            }
            if (live) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sa[(size_t)(kb * 32 + featF(r, h)) * ld + c] = acc[r];
            }
        }
        for (int c = threadIdx.x; c < N; c += THREADS) {
            float s = 0.f;
            for (int m = 0; m < TILE; ++m) s += sel[m] == a ? dth[m * pt + c] : 0.f;
            sa[(size_t)K * ld + c] = s;
        }
    }
}

// top[32][K] <- (sum over the present actions a of (dth masked by sel == a) W[:, aN .. aN + N)^T) * (top > 0), in place.  Block k on
// wave k mod 4; A(i, c) = dth[i][c] from LDS, B(c, i) = W[k0 + i][aN + c] along c (N and aN need no alignment: 4-byte loads)
__device__ void head_dgrad(const QNet& net, const float* __restrict__ p, float* top, int ptop, const float* dth, const int* sel, unsigned present) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int K = net.head.K, N = net.n_atoms, ld = net.head.N, pt = net.pitch;
    const int mysel = sel[i];
    const float* zp = dth + i * pt;
    for (int kb = wave; kb < K / 32; kb += 4) {
        const int kc = kb * 32 + i;
        const float* wrow = p + net.head.off + (size_t)kc * ld;
        f32x16 acc = {};
        for (int a = 0; a < net.n_act; ++a) {
            if (!((present >> a) & 1)) continue;                               // workgroup-uniform
            const bool mine = mysel == a;
            const float* wa = wrow + a * N;
#pragma unroll 4
            for (int c = 0; c < N; c += 2) {
                const bool in = c + h < N;                                     // odd N: the last pair is half empty
                const int cc = in ? c + h : 0;
                const float z = zp[cc], w = wa[cc];
                acc = mfma32(in && mine ? z : 0.f, in ? w : 0.f, acc);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float* q = top + featF(r, h) * ptop + kc;
            *q = *q > 0.f ? acc[r] : 0.f;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------

inline int64_t tiles_of(int64_t B) { return ts::ceil_div(B, TILE); }
inline size_t ws_bytes(const QNet& n, int64_t B) { return update_scratch(nullptr, tiles_of(B), n.P).bytes; }

// The QNet of a plain Net whose last Linear has n_act * N outputs, from ts_dqn_mlp's 14 desc entries and N in entry 14, with the LDS
// carve of one tile: obs | hidden activations | n_tables (2 or 3) [32][N | 1] tables in the order ta, tb, [the third one, its offset
// in *third_table_at] | 4 x 32 per-row scalars.  `noun`: what the N outputs of an action are ("quantiles", "atoms").
int make_qnet(const int64_t* d, const char* who, const char* noun, int n_tables, QNet* out, int* third_table_at) {
    TS_REQUIRE(d != nullptr, TS_ERR_INVALID_ARG, "%s: NULL network description", who);
    QNet n{};
    const int64_t obs_dim = d[0], n_act = d[1], nt = d[3], n_atoms = d[14];
    TS_REQUIRE(obs_dim >= 1 && obs_dim <= 256, TS_ERR_UNSUPPORTED, "%s: obs_dim %lld outside [1, 256]", who, (long long)obs_dim);
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_UNSUPPORTED, "%s: %lld actions outside [1, 32]", who, (long long)n_act);
    TS_REQUIRE(n_atoms >= 2 && n_atoms <= MAX_ATOMS, TS_ERR_UNSUPPORTED, "%s: %lld %s outside [2, 256]", who, (long long)n_atoms, noun);
    TS_REQUIRE(nt >= 1 && nt <= MAX_TRUNK, TS_ERR_UNSUPPORTED, "%s: %lld trunk hidden layers outside [1, 4]", who, (long long)nt);
    TS_REQUIRE(d[2] == 0 && d[4] == 0 && d[5] == 0, TS_ERR_UNSUPPORTED, "%s: a dueling head with %s is not supported", who, noun);
    n.obs_dim = (int)obs_dim; n.n_act = (int)n_act; n.n_atoms = (int)n_atoms; n.nt = (int)nt;
    int off = 0, at = 0;
    auto add = [&](Lay* l, int K, int N) { l->K = K; l->N = N; l->off = off; off += (K + 1) * N; };
    auto carve = [&](int floats) { const int o = at; at += floats; return o; };
    n.x_at = carve(TILE * (n.obs_dim + 1));
    int k = n.obs_dim;
    for (int i = 0; i < n.nt; ++i) {
        const int64_t w = d[6 + i];
        TS_REQUIRE(w >= 32 && w <= 256 && w % 32 == 0, TS_ERR_UNSUPPORTED, "%s: hidden width %lld is no multiple of 32 in [32, 256]", who, (long long)w);
        add(&n.t[i], k, (int)w);
        n.t_at[i] = carve(TILE * (n.t[i].N + 1));
        k = n.t[i].N;
    }
    add(&n.head, k, n.n_act * n.n_atoms);
    n.pitch = n.n_atoms | 1;
    n.ta_at = carve(TILE * n.pitch);
    n.tb_at = carve(TILE * n.pitch);
    if (n_tables > 2) *third_table_at = carve(TILE * n.pitch);
    n.row_at = carve(4 * TILE);
    n.P = off;
    n.lds_floats = at;
    TS_REQUIRE((size_t)at * 4 + 256 <= (size_t)LDS_LIMIT, TS_ERR_UNSUPPORTED,       // ("quantile tables": the noun without its s)
               "%s: the activations and %.*s tables of one 32-row tile need %zu bytes of LDS, the workgroup limit is %d", who,
               (int)strlen(noun) - 1, noun, (size_t)at * 4 + 256, LDS_LIMIT);
    *out = n;
    return TS_OK;
}

template <typename Kern>
int allow_lds(ts::DynLds& slot, Kern kern, const QNet& n) {
    return slot.allow(reinterpret_cast<const void*>(kern), (size_t)n.lds_floats * 4);
}

int check_batch(int64_t B, const char* who) {
    TS_REQUIRE(B >= 1 && B <= 4096, B < 1 ? TS_ERR_INVALID_ARG : TS_ERR_UNSUPPORTED, "%s: B = %lld outside [1, 4096]", who, (long long)B);
    return TS_OK;
}

}  // namespace
