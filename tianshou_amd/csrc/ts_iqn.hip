// ts_iqn.hip -- Implicit Quantile Networks (IQN, arXiv:1806.06923) on the Atari trunk for gfx950.
//
// Replaces, on device-resident NHWC observations:
//   CosineEmbeddingNetwork.forward            tianshou/utils/net/discrete.py:144-160
//   ImplicitQuantileNetwork.forward           discrete.py:200-216 (preprocess_net = DQNet(features_only=True), hidden [512])
//   IQNPolicy.forward                         tianshou/algorithm/modelfree/iqn.py:72-100 (Q = mean over the sampled fractions)
//   QRDQN._target_q with IQNPolicy.forward    modelfree/qrdqn.py:94-106
//   IQN._update_with_batch                    iqn.py:156-183 (quantile Huber loss with the SAMPLED fractions, new priorities)
//   Optimizer.step                            algorithm_base.py:484-500 (clip_grad_norm_ + Adam)
// The fractions tau are an INPUT of every entry point (the reference draws them with torch.rand inside the model).
//
//   feat[b, :]  = relu(conv3(relu(conv2(relu(conv1(obs[b]))))))         F = 64 * OH3 * OW3 features in (h, w, c) order
//   phi[r, :]   = relu(cosv[r, :] @ We + be),  cosv[r, i] = cos(tau[r] * ipi[i]),  ipi[i] = fl32(fl32(pi) * (i + 1)),  r = b N + n
//   x[r, :]     = feat[b(r), :] * phi[r, :]
//   out[r, :]   = relu(x[r, :] @ W1 + b1) @ W2 + b2
// The trunk runs on B rows and fc1 / fc2 on R = B N rows through the fp32-MFMA implicit-GEMM kernels of ts_conv.hip; this
// file adds the cosine-embedding kernels (forward: cosines -> MFMA -> bias, ReLU, multiply in one launch, phi never stored;
// backward: phi recomputed, d feat / d We / d be in one launch), the per-sample loss / head kernels and the orchestration.
// Flat parameter layout: conv1 | conv2 | conv3 | [We; be] [65, F] | [W1; b1] [F + 1, 512] | [W2; b2] [513, ld], ld = n_act
// rounded up to a multiple of 32 (GEMM tile width; the padding columns are and stay exactly zero).
#include <algorithm>

#include "ts_common.h"
#include "ts_conv.h"

#pragma clang fp contract(off)

namespace ts {
int adam_step(hipStream_t s, float* params, float* m, float* v, const float* grad, int64_t n, int64_t step,
              double lr, double beta1, double beta2, double eps, double max_grad_norm, float* norm_scratch);
}

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int HIDDEN = 512;
constexpr int MAX_ACT = 64;
constexpr int MAX_N = 64;       // sampled fractions per state
constexpr int KC = 64;          // num_cosines: the reduction depth of the embedding GEMM
constexpr int BM = 64;          // rows of one embedding tile
constexpr int LDC = KC + 1;     // odd LDS pitch of the cosine tile
constexpr int BWD_SLABS = 8;    // row-tile shares of the embedding weight gradient (fixed: part of the summation order)
constexpr int FWD_SHARES = 16;

__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

struct INet {
    ts::ConvGeom l[5];          // conv1, conv2, conv3 (B rows), fc1, fc2 (R = B N rows)
    int64_t off[7];             // conv1, conv2, conv3, embedding, fc1, fc2, total
    int F, n_act, ld;
    int64_t B, R;
    int N;
};

int make_inet(int64_t B, int64_t N, int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t n_cos, INet* n) {
    TS_REQUIRE(c >= 1 && h >= 1 && w >= 1 && c < (1 << 16) && h < (1 << 16) && w < (1 << 16), TS_ERR_INVALID_ARG,
               "iqn: bad observation dimensions");
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_INVALID_ARG, "iqn: 1 <= n_act <= 64");
    TS_REQUIRE(N >= 2 && N <= MAX_N, TS_ERR_INVALID_ARG, "iqn: 2 <= sample size (N, N') <= 64");
    TS_REQUIRE(n_cos == KC, TS_ERR_INVALID_ARG, "iqn: num_cosines must be 64 (hidden layer: 512)");
    TS_REQUIRE(B >= 1 && B * N < (1 << 24), TS_ERR_INVALID_ARG, "iqn: batch too large (B * N < 2^24)");
    static const int oc[3] = {32, 64, 64}, ks[3] = {8, 4, 3}, st[3] = {4, 2, 1};
    int ic = (int)c, ih = (int)h, iw = (int)w;
    for (int i = 0; i < 3; ++i) {
        TS_REQUIRE(ih >= ks[i] && iw >= ks[i], TS_ERR_INVALID_ARG, "iqn: observation too small for DQNet");
        n->l[i] = ts::ConvGeom{(int)B, ih, iw, ic, ks[i], ks[i], st[i], (ih - ks[i]) / st[i] + 1, (iw - ks[i]) / st[i] + 1, oc[i]};
        ic = oc[i]; ih = n->l[i].OH; iw = n->l[i].OW;
    }
    n->B = B; n->N = (int)N; n->R = B * N;
    n->F = ic * ih * iw;
    TS_REQUIRE((int64_t)n->R * std::max(n->F, HIDDEN) < (int64_t(1) << 31), TS_ERR_INVALID_ARG,
               "iqn: batch too large (B * N * features < 2^31)");
    n->n_act = (int)n_act;
    n->ld = ((int)n_act + 31) / 32 * 32;
    n->l[3] = ts::ConvGeom{(int)n->R, 1, 1, n->F, 1, 1, 1, 1, 1, HIDDEN};
    n->l[4] = ts::ConvGeom{(int)n->R, 1, 1, HIDDEN, 1, 1, 1, 1, 1, n->ld};
    int64_t o = 0;
    for (int i = 0; i < 3; ++i) { n->off[i] = o; o += n->l[i].param_elems(); }
    n->off[3] = o; o += (int64_t)(KC + 1) * n->F;
    n->off[4] = o; o += n->l[3].param_elems();
    n->off[5] = o; o += n->l[4].param_elems();
    n->off[6] = o;
    return TS_OK;
}

size_t al(size_t x) { return (x + 255) & ~size_t(255); }

struct IActs { float* c[3]; float* x; float* h1; float* out; float* split; float* cosv; };

size_t split_floats(const INet& n) {
    size_t s = 4;
    for (int i = 0; i < 5; ++i) {
        const int ns = ts::conv_fwd_splits(n.l[i]);
        if (ns > 1) s = std::max(s, (size_t)ns * n.l[i].out_elems());
    }
    return s;
}

size_t acts_bytes(const INet& n) {
    size_t s = al(4 * split_floats(n)) + al(4 * (size_t)n.R * n.F) + al(4 * (size_t)n.R * KC);
    for (int i = 0; i < 5; ++i) s += al(4 * (size_t)n.l[i].out_elems());
    return s;
}

char* carve_acts(const INet& n, char* p, IActs* a) {
    auto take = [&](size_t floats) { float* r = reinterpret_cast<float*>(p); p += al(4 * floats); return r; };
    for (int i = 0; i < 3; ++i) a->c[i] = take((size_t)n.l[i].out_elems());
    a->x = take((size_t)n.R * n.F);
    a->h1 = take((size_t)n.l[3].out_elems());
    a->out = take((size_t)n.l[4].out_elems());
    a->split = take(split_floats(n));
    a->cosv = take((size_t)n.R * KC);
    return p;
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

__device__ __forceinline__ float block_sum_256(float v, float* red) {      // all threads get the sum (fixed order)
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- cosine embedding ------------------------------------------------------------------------------------------------
// cs[i, k] = cos(tau[row0 + i] * ipi[k]) for the `rows` valid rows of a tile (the others: tau = 0).  The argument is formed
// as torch forms it (discrete.py:148-155): ipi = fl32(pi) * fl32(k + 1) rounded to float32, then tau * ipi rounded to
// float32 (no contraction in this file), then an accurate cosf.  One cosine per (row, k) per workgroup.
__device__ __forceinline__ void cos_tile(const float* __restrict__ tau, int64_t row0, int rows, float* cs) {
    for (int e = threadIdx.x; e < BM * KC; e += 256) {
        const int i = e >> 6, k = e & 63;
        const float t = i < rows ? tau[row0 + i] : 0.f;
        const float ipi = 3.14159274101257324f * (float)(k + 1);
        cs[i * LDC + k] = cosf(t * ipi);
    }
}

// We[:, n0 : n0 + BN] -> LDS (columns at or beyond F: zeros).  F is a multiple of 64, so a float4 is inside or outside.
template <int BN>
__device__ __forceinline__ void load_we_tile(const float* __restrict__ We, int F, int n0, float* wsm) {
    for (int e = threadIdx.x; e < KC * BN / 4; e += 256) {
        const int k = e / (BN / 4), n4 = e % (BN / 4), col = n0 + 4 * n4;
        f32x4 v{0.f, 0.f, 0.f, 0.f};
        if (col < F) v = *reinterpret_cast<const f32x4*>(We + (int64_t)k * F + col);
        *reinterpret_cast<f32x4*>(&wsm[k * BN + 4 * n4]) = v;
    }
}

// acc[tn] = cs[wm 32 .. +32, :] @ wsm[:, (wn TN + tn) 32 .. +32]   (k sequential: one fixed summation order)
template <int TN>
__device__ __forceinline__ void phi_tile(const float* cs, const float* wsm, int wm, int wn, int r, int h, f32x16 (&acc)[TN]) {
    constexpr int BN = 64 * TN;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int x = 0; x < 16; ++x) acc[tn][x] = 0.f;
#pragma unroll 8
    for (int kk2 = 0; kk2 < KC / 2; ++kk2) {
        const float av = cs[(wm * 32 + r) * LDC + 2 * kk2 + h];
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const float bv = wsm[(2 * kk2 + h) * BN + (wn * TN + tn) * 32 + r];
            acc[tn] = mfma32(av, bv, acc[tn]);
        }
    }
}

// x[r, :] = feat[r / N, :] * relu(cosv[r, :] @ We + be).  Grid: (column tiles of BN = 64 TN, row-tile shares).  A workgroup
// keeps its We column tile in LDS and walks over its row tiles; four waves as 2 x 2 tiles of 32 x (32 TN).
template <int TN>
__global__ __launch_bounds__(256) void iqn_embed_fwd_kernel(const float* __restrict__ tau, const float* __restrict__ feat,
                                                            const float* __restrict__ We, int64_t R, int N, int F,
                                                            float* __restrict__ xo) {
    constexpr int BN = 64 * TN;
    __shared__ float cs[BM * LDC];
    __shared__ __attribute__((aligned(16))) float wsm[KC * BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * BN;
    load_we_tile<BN>(We, F, n0, wsm);
    const float* be = We + (int64_t)KC * F;
    const int tiles = (int)((R + BM - 1) / BM);
    for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
        const int64_t row0 = (int64_t)t * BM;
        const int rows = (int)min((int64_t)BM, R - row0);
        __syncthreads();                                  // the previous tile's cosines are consumed
        cos_tile(tau, row0, rows, cs);
        __syncthreads();
        f32x16 acc[TN];
        phi_tile<TN>(cs, wsm, wm, wn, r, h, acc);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) {
            const int col = n0 + (wn * TN + tn) * 32 + r;
            if (col >= F) continue;
            const float bias = be[col];
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int i = wm * 32 + (x & 3) + 8 * (x >> 2) + 4 * h;
                if (i < rows) {
                    const int64_t row = row0 + i;
                    const float phi = fmaxf(acc[tn][x] + bias, 0.f);
                    xo[row * F + col] = feat[(row / N) * F + col] * phi;
                }
            }
        }
    }
}

// Backward of the above from dx = d loss / d x.  Row tiles hold WHOLE samples (SB = 64 / N samples, SB N rows):
//   phi recomputed;  dphi = dx * feat[b] * 1{phi > 0};
//   dfeat[b, :] = 1{feat > 0} * sum_n dx[b N + n, :] * phi[b N + n, :]     (n ascending; masked: the gradient conv3's
//                                                                          backward pass takes for its ReLU output)
//   slab[y][k, :]  = sum over the row tiles of share y (ascending), rows ascending: cosv[r, k] * dphi[r, :]    (MFMA)
//   slab[y][64, :] = the same sum of dphi[r, :]                                                                (d be)
// Grid: (F / 64 column tiles, BWD_SLABS shares); ts::slab_sum finishes [d We; d be].
__global__ __launch_bounds__(256) void iqn_embed_bwd_kernel(const float* __restrict__ tau, const float* __restrict__ feat,
                                                            const float* __restrict__ We, const float* __restrict__ dx,
                                                            int64_t B, int N, int F, float* __restrict__ dfeat,
                                                            float* __restrict__ slabs) {
    constexpr int BN = 64;
    __shared__ float cs[BM * LDC];
    __shared__ __attribute__((aligned(16))) float wsm[KC * BN];
    __shared__ float dp[BM * BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * BN;                       // F is a multiple of 64: every column of the tile exists
    load_we_tile<BN>(We, F, n0, wsm);
    const int col = n0 + wn * 32 + r;
    const float bias = We[(int64_t)KC * F + col];
    const int SB = BM / N;
    const int tiles = (int)((B + SB - 1) / SB);
    f32x16 dacc;
#pragma unroll
    for (int x = 0; x < 16; ++x) dacc[x] = 0.f;
    float dbe = 0.f;
    for (int t = blockIdx.y; t < tiles; t += gridDim.y) {
        const int64_t b0 = (int64_t)t * SB;
        const int nb = (int)min((int64_t)SB, B - b0), rows = nb * N;
        const int64_t row0 = b0 * N;
        __syncthreads();                                  // the previous tile's cs / dp are consumed
        cos_tile(tau, row0, rows, cs);
        __syncthreads();
        f32x16 acc[1];
        phi_tile<1>(cs, wsm, wm, wn, r, h, acc);
        float dphi[16];
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int i = wm * 32 + (x & 3) + 8 * (x >> 2) + 4 * h;
            float c = 0.f;
            dphi[x] = 0.f;
            if (i < rows) {
                const float phi = fmaxf(acc[0][x] + bias, 0.f);
                const float d = dx[(row0 + i) * F + col];
                const float f = feat[(b0 + i / N) * F + col];
                c = d * phi;
                dphi[x] = phi > 0.f ? d * f : 0.f;
            }
            dp[i * BN + wn * 32 + r] = c;
        }
        __syncthreads();
        for (int e = tid; e < nb * BN; e += 256) {
            const int bl = e >> 6, cc = e & 63;
            float s = 0.f;
            for (int n = 0; n < N; ++n) s += dp[(bl * N + n) * BN + cc];
            const int64_t o = (b0 + bl) * F + n0 + cc;
            dfeat[o] = feat[o] > 0.f ? s : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int x = 0; x < 16; ++x) dp[(wm * 32 + (x & 3) + 8 * (x >> 2) + 4 * h) * BN + wn * 32 + r] = dphi[x];
        __syncthreads();
        if (tid < BN)
            for (int i = 0; i < BM; ++i) dbe += dp[i * BN + tid];
#pragma unroll 8
        for (int rr2 = 0; rr2 < BM / 2; ++rr2) {          // dWe[k, col] += cosv[rr, k] dphi[rr, col]: rows k = wm 32 + r
            const float av = cs[(2 * rr2 + h) * LDC + wm * 32 + r];
            const float bv = dp[(2 * rr2 + h) * BN + wn * 32 + r];
            dacc = mfma32(av, bv, dacc);
        }
    }
    float* slab = slabs + (int64_t)blockIdx.y * (KC + 1) * F;
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        const int k = wm * 32 + (x & 3) + 8 * (x >> 2) + 4 * h;
        slab[(int64_t)k * F + col] = dacc[x];
    }
    if (tid < BN) slab[(int64_t)KC * F + n0 + tid] = dbe;
}

// ---- the unfused routes through kernels that already exist (the yardstick the fused kernels are measured against, and the
// shipped path wherever it is the faster one: DESIGN.md 4.5b).  Forward: cosv[R, 64] -> ts::conv_forward (bias + ReLU) -> multiply
// in place.  Backward: cosv, phi by the same forward, one elementwise pass (d feat; d phi stored over phi), ts::conv_wgrad.
__global__ __launch_bounds__(256) void iqn_cos_kernel(const float* __restrict__ tau, int64_t R, float* __restrict__ cosv) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * KC) return;
    const float ipi = 3.14159274101257324f * (float)((int)(i & 63) + 1);
    cosv[i] = cosf(tau[i >> 6] * ipi);
}

// x[r, :] *= feat[r / N, :]   (float4 per thread; F is a multiple of 64)
__global__ __launch_bounds__(256) void iqn_mul_kernel(float* __restrict__ x, const float* __restrict__ feat, int64_t R, int N,
                                                      int F) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int f4 = F >> 2;
    if (i >= R * f4) return;
    const int64_t row = i / f4;
    const int c4 = (int)(i - row * f4);
    f32x4 v = reinterpret_cast<f32x4*>(x)[i];
    const f32x4 f = reinterpret_cast<const f32x4*>(feat)[(row / N) * f4 + c4];
    v[0] *= f[0]; v[1] *= f[1]; v[2] *= f[2]; v[3] *= f[3];
    reinterpret_cast<f32x4*>(x)[i] = v;
}

// one thread per (b, column): dfeat = 1{feat > 0} sum_n dx * phi (n ascending), phi <- d phi = dx * feat * 1{phi > 0}
__global__ __launch_bounds__(256) void iqn_dphi_kernel(float* __restrict__ phi, const float* __restrict__ dx,
                                                       const float* __restrict__ feat, int64_t B, int N, int F,
                                                       float* __restrict__ dfeat) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * F) return;
    const int64_t b = i / F;
    const int c = (int)(i - b * F);
    const float f = feat[i];
    float sum = 0.f;
    for (int n = 0; n < N; ++n) {
        const int64_t o = (b * N + n) * F + c;
        const float ph = phi[o], d = dx[o];
        sum += d * ph;
        phi[o] = ph > 0.f ? d * f : 0.f;
    }
    dfeat[i] = f > 0.f ? sum : 0.f;
}

// Routes of the two embedding passes.  The unfused routes are taken below 2^14 rows only: there the GEMMs run on the first-
// generation kernels of ts_conv.hip, whose bounds hold for a 64-deep reduction (rows and k are clamped on load, guarded on store).
enum { ROUTE_DEFAULT = 0, ROUTE_FUSED = 1, ROUTE_UNFUSED = 2 };
constexpr int64_t UNFUSED_MAX_ROWS = 1 << 14;
// the shipped routes, decided by measurement at the C3 shape (profiles/iqn_bench.json)
constexpr bool FWD_DEFAULT_UNFUSED = true;
constexpr bool BWD_DEFAULT_UNFUSED = true;

bool route_unfused(int route, int64_t R, bool fwd) {
    if (R >= UNFUSED_MAX_ROWS || route == ROUTE_FUSED) return false;
    if (route == ROUTE_UNFUSED) return true;
    return fwd ? FWD_DEFAULT_UNFUSED : BWD_DEFAULT_UNFUSED;
}

ts::ConvGeom embed_geom(int64_t R, int F) { return ts::ConvGeom{(int)R, 1, 1, KC, 1, 1, 1, 1, 1, F}; }

int embed_bwd_shares(int64_t B, int N) {
    const int64_t tiles = ts::ceil_div(B, BM / N);
    return (int)std::min<int64_t>(tiles, BWD_SLABS);
}

// slabs of [d We; d be] the backward pass leaves for ts::slab_sum
int embed_bwd_slabs(bool unfused, int64_t B, int N, int F) {
    return unfused ? ts::conv_wgrad_splits(embed_geom(B * N, F)) : embed_bwd_shares(B, N);
}

// cosv: R * 64 floats of scratch (unfused route only)
int embed_forward(hipStream_t s, ts_workspace* ws, bool unfused, const float* tau, const float* feat, const float* We, int64_t R,
                  int N, int F, float* x, float* cosv) {
    if (unfused) {
        hipLaunchKernelGGL(iqn_cos_kernel, dim3((unsigned)ts::ceil_div(R * KC, 256)), dim3(256), 0, s, tau, R, cosv);
        TS_LAUNCH_CHECK();
        if (int rc = ts::conv_forward(s, embed_geom(R, F), cosv, We, x, true, nullptr, ws)) return rc;     // 2 chunks: never split
        hipLaunchKernelGGL(iqn_mul_kernel, dim3((unsigned)ts::ceil_div(R * (F / 4), 256)), dim3(256), 0, s, x, feat, R, N, F);
        TS_LAUNCH_CHECK();
        return TS_OK;
    }
    const int64_t tiles = ts::ceil_div(R, BM);
    const unsigned gy = (unsigned)std::min<int64_t>(tiles, FWD_SHARES);
    hipLaunchKernelGGL(iqn_embed_fwd_kernel<2>, dim3((unsigned)ts::ceil_div(F, 128), gy), dim3(256), 0, s, tau, feat, We, R, N,
                       F, x);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

// slabs: embed_bwd_slabs(...) * 65 F floats; unfused route: cosv R * 64 and phi R * F floats of scratch
int embed_backward(hipStream_t s, ts_workspace* ws, bool unfused, const float* tau, const float* feat, const float* We,
                   const float* dx, int64_t B, int N, int F, float* dfeat, float* slabs, float* cosv, float* phi) {
    if (unfused) {
        const int64_t R = B * N;
        const ts::ConvGeom g = embed_geom(R, F);
        hipLaunchKernelGGL(iqn_cos_kernel, dim3((unsigned)ts::ceil_div(R * KC, 256)), dim3(256), 0, s, tau, R, cosv);
        TS_LAUNCH_CHECK();
        if (int rc = ts::conv_forward(s, g, cosv, We, phi, true, nullptr, ws)) return rc;
        hipLaunchKernelGGL(iqn_dphi_kernel, dim3((unsigned)ts::ceil_div(B * F, 256)), dim3(256), 0, s, phi, dx, feat, B, N, F, dfeat);
        TS_LAUNCH_CHECK();
        return ts::conv_wgrad(s, g, cosv, phi, slabs, ws);
    }
    hipLaunchKernelGGL(iqn_embed_bwd_kernel, dim3((unsigned)(F / 64), (unsigned)embed_bwd_shares(B, N)), dim3(256), 0, s, tau,
                       feat, We, dx, B, N, F, dfeat, slabs);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

// ---- head: one wave per sample, lane a sums the N rows of column a in order.  Q[b, a] = mean_n out[b N + n, a]
// (qrdqn.py:19-21), act = the first maximum (iqn.py:98), logits[b, a, n] = out[b N + n, a] (discrete.py:215).
__global__ __launch_bounds__(256) void iqn_head_kernel(const float* __restrict__ out, int64_t B, int A, int N, int ld,
                                                       float* __restrict__ logits, float* __restrict__ q_out,
                                                       int64_t* __restrict__ act_out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float q = -INFINITY;
    if (lane < A) {
        float s = 0.f;
        for (int n = 0; n < N; ++n) {
            const float v = out[(b * N + n) * ld + lane];
            s += v;
            if (logits) logits[(b * A + lane) * N + n] = v;
        }
        q = s / (float)N;
        if (q_out) q_out[b * A + lane] = q;
    }
    int best = lane < A ? lane : A;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float oq = __shfl_xor(q, off, 64);
        const int ob = __shfl_xor(best, off, 64);
        if (oq > q || (oq == q && ob < best)) { q = oq; best = ob; }
    }
    if (act_out && lane == 0) act_out[b] = best < A ? best : 0;
}

// dst[b, j] = out[b N + j, act[b]]
__global__ __launch_bounds__(256) void iqn_select_kernel(const float* __restrict__ out, const int64_t* __restrict__ act,
                                                         int64_t B, int N, int ld, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * N) return;
    dst[i] = out[i * ld + act[i / N]];          // act: iqn_head_kernel's own output, in [0, A)
}

// ---- IQN loss (iqn.py:162-180), one workgroup per sample; N online fractions, Np target quantiles:
//   theta_i = out[b N + i, act_b], T_j = returns[b, j], d_ij = T_j - theta_i, l_ij = smooth_l1(d_ij)
//   w_ij = |tau[b, i] - 1{d_ij <= 0}|
//   huber_b = (1/N) sum_i sum_j l_ij w_ij,   prio_b = (1/N) sum_i sum_j l_ij,   loss = mean_b(huber_b weight_b)
//   d loss / d theta_i = -(weight_b / (B N)) sum_j w_ij clamp(d_ij, -1, 1);  every other head output of the sample's N rows
//   (padding columns included) gets an exact zero.
__global__ __launch_bounds__(256) void iqn_loss_kernel(const float* __restrict__ out, const int64_t* __restrict__ act,
                                                       const float* __restrict__ ret, const float* __restrict__ weight,
                                                       const float* __restrict__ tau, int64_t B, int A, int N, int Np,
                                                       int ld, float* __restrict__ d_out, float* __restrict__ prio,
                                                       float* __restrict__ lw) {
    __shared__ float T[MAX_N], red[4];
    const int64_t b = blockIdx.x;
    // an action index outside [0, A) is clamped: nothing is written outside the sample's rows or into the padding columns
    const int a = (int)min((int64_t)(A - 1), max((int64_t)0, act[b]));
    if ((int)threadIdx.x < Np) T[threadIdx.x] = ret[b * Np + threadIdx.x];
    __syncthreads();
    const float wb = weight ? weight[b] : 1.f;
    const float scale = wb / ((float)B * (float)N);
    float* drows = d_out + b * N * ld;
    for (int e = threadIdx.x; e < N * ld; e += 256)
        if (e % ld != a) drows[e] = 0.f;
    float li = 0.f, ai = 0.f;
    const int i = threadIdx.x;
    if (i < N) {
        const float theta = out[(b * N + i) * ld + a], tq = tau[b * N + i];
        float g = 0.f;
        for (int j = 0; j < Np; ++j) {
            const float d = T[j] - theta, ad = fabsf(d);
            const bool quad = ad < 1.f;
            const float l = quad ? 0.5f * d * d : ad - 0.5f;
            const float w = fabsf(tq - (d <= 0.f ? 1.f : 0.f));
            li += l * w;
            ai += l;
            g += w * (quad ? d : (d > 0.f ? 1.f : -1.f));
        }
        drows[i * ld + a] = -g * scale;
    }
    const float wl = block_sum_256(li, red);
    const float sl = block_sum_256(ai, red);
    if (threadIdx.x == 0) {
        prio[b] = sl / (float)N;
        lw[b] = (wl / (float)N) * wb;
    }
}

// loss = mean_b lw[b] (fixed order)
__global__ __launch_bounds__(1024) void iqn_mean_kernel(const float* __restrict__ v, int64_t B, float* __restrict__ out) {
    __shared__ float red[1024];
    float s = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += 1024) s += v[b];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0] / (float)B;
}

// One pass of ImplicitQuantileNetwork.forward: a.out[R, ld]
int net_forward(hipStream_t s, ts_workspace* ws, const INet& n, const float* params, const void* obs, bool obs_u8,
                const float* tau, const IActs& a) {
    const float* x = static_cast<const float*>(obs);
    for (int i = 0; i < 3; ++i) {
        if (int rc = ts::conv_forward(s, n.l[i], x, params + n.off[i], a.c[i], true, a.split, ws, i == 0 && obs_u8)) return rc;
        x = a.c[i];
    }
    if (int rc = embed_forward(s, ws, route_unfused(ROUTE_DEFAULT, n.R, true), tau, a.c[2], params + n.off[3], n.R, n.N, n.F, a.x,
                               a.cosv)) return rc;
    if (int rc = ts::conv_forward(s, n.l[3], a.x, params + n.off[4], a.h1, true, a.split, ws)) return rc;
    return ts::conv_forward(s, n.l[4], a.h1, params + n.off[5], a.out, false, a.split, ws);
}

}  // namespace

extern "C" {

int64_t ts_iqn_param_count(int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t n_cos) {
    INet n;
    if (make_inet(1, 2, c, h, w, n_act, n_cos, &n) != TS_OK) return -1;
    return n.off[6];
}

int ts_iqn_layout(int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t n_cos, int64_t* h_out9) {
    INet n;
    if (int rc = make_inet(1, 2, c, h, w, n_act, n_cos, &n)) return rc;
    TS_REQUIRE(h_out9, TS_ERR_INVALID_ARG, "ts_iqn_layout: NULL output");
    h_out9[0] = n.F; h_out9[1] = n.ld; h_out9[2] = n.off[6];
    for (int i = 0; i < 6; ++i) h_out9[3 + i] = n.off[i];
    return TS_OK;
}

int ts_iqn_embed_mul(ts_workspace* ws, const float* tau, const float* feat, const float* we_be, int64_t B, int64_t N,
                     int64_t F, int64_t n_cos, int route, float* x_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_iqn_embed_mul: workspace is NULL");
    TS_REQUIRE(B >= 1 && N >= 1 && N <= MAX_N && B * N < (1 << 24) && F >= 64 && F % 64 == 0 && F < (1 << 24) && n_cos == KC,
               TS_ERR_INVALID_ARG, "ts_iqn_embed_mul: need 1 <= N <= 64, F a multiple of 64, num_cosines = 64");
    TS_REQUIRE(tau && feat && we_be && x_out, TS_ERR_INVALID_ARG, "ts_iqn_embed_mul: NULL argument");
    TS_REQUIRE(route >= ROUTE_DEFAULT && route <= ROUTE_UNFUSED && (route != ROUTE_UNFUSED || B * N < UNFUSED_MAX_ROWS),
               TS_ERR_INVALID_ARG, "ts_iqn_embed_mul: route is TS_IQN_ROUTE_*; the unfused route takes fewer than 16384 rows");
    const bool unfused = route_unfused(route, B * N, true);
    if (int rc = ts::ws_reserve(ws, al(4 * (size_t)B * N * KC))) return rc;
    return embed_forward(ts::as_stream(stream), ws, unfused, tau, feat, we_be, B * N, (int)N, (int)F, x_out,
                         static_cast<float*>(ws->base));
}

int ts_iqn_embed_mul_backward(ts_workspace* ws, const float* tau, const float* feat, const float* we_be, const float* dx,
                              int64_t B, int64_t N, int64_t F, int64_t n_cos, int route, float* dfeat_out, float* dwe_be_out,
                              ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_iqn_embed_mul_backward: workspace is NULL");
    TS_REQUIRE(B >= 1 && N >= 1 && N <= MAX_N && B * N < (1 << 24) && F >= 64 && F % 64 == 0 && F < (1 << 24) && n_cos == KC,
               TS_ERR_INVALID_ARG, "ts_iqn_embed_mul_backward: need 1 <= N <= 64, F a multiple of 64, num_cosines = 64");
    TS_REQUIRE(tau && feat && we_be && dx && dfeat_out && dwe_be_out, TS_ERR_INVALID_ARG,
               "ts_iqn_embed_mul_backward: NULL argument");
    TS_REQUIRE(route >= ROUTE_DEFAULT && route <= ROUTE_UNFUSED && (route != ROUTE_UNFUSED || B * N < UNFUSED_MAX_ROWS),
               TS_ERR_INVALID_ARG, "ts_iqn_embed_mul_backward: route is TS_IQN_ROUTE_*; the unfused route takes fewer than 16384 rows");
    const bool unfused = route_unfused(route, B * N, false);
    const int ns = embed_bwd_slabs(unfused, B, (int)N, (int)F);
    const int64_t pe = (KC + 1) * F;
    const size_t b_slabs = al(4 * (size_t)ns * pe), b_cos = al(4 * (size_t)B * N * KC), b_phi = unfused ? al(4 * (size_t)B * N * F) : 0;
    if (int rc = ts::ws_reserve(ws, b_slabs + b_cos + b_phi)) return rc;
    char* p = static_cast<char*>(ws->base);
    float* slabs = reinterpret_cast<float*>(p);
    float* cosv = reinterpret_cast<float*>(p + b_slabs);
    float* phi = reinterpret_cast<float*>(p + b_slabs + b_cos);
    hipStream_t s = ts::as_stream(stream);
    if (int rc = embed_backward(s, ws, unfused, tau, feat, we_be, dx, B, (int)N, (int)F, dfeat_out, slabs, cosv, phi)) return rc;
    return ts::slab_sum(s, slabs, ns, pe, dwe_be_out);
}

int ts_iqn_forward(ts_workspace* ws, const float* params, int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t n_cos,
                   const void* obs_nhwc, int obs_u8, int64_t B, const float* tau, int64_t N, float* logits_out,
                   float* q_out, int64_t* act_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_iqn_forward: workspace is NULL");
    TS_REQUIRE(B >= 0, TS_ERR_INVALID_ARG, "ts_iqn_forward: negative batch");
    INet n;
    if (int rc = make_inet(std::max<int64_t>(B, 1), N, c, h, w, n_act, n_cos, &n)) return rc;
    if (B == 0) return TS_OK;
    TS_REQUIRE(params && obs_nhwc && tau, TS_ERR_INVALID_ARG, "ts_iqn_forward: NULL argument");
    if (int rc = ts::ws_reserve(ws, acts_bytes(n))) return rc;
    IActs a;
    carve_acts(n, static_cast<char*>(ws->base), &a);
    hipStream_t s = ts::as_stream(stream);
    if (int rc = net_forward(s, ws, n, params, obs_nhwc, obs_u8 != 0, tau, a)) return rc;
    hipLaunchKernelGGL(iqn_head_kernel, dim3((unsigned)ts::ceil_div(B, 4)), dim3(256), 0, s, a.out, B, n.n_act, n.N, n.ld,
                       logits_out, q_out, act_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_iqn_next_dist(ts_workspace* ws, const float* params, const float* params_old, int64_t c, int64_t h, int64_t w,
                     int64_t n_act, int64_t n_cos, const void* obs_next_nhwc, int obs_u8, int64_t B,
                     const float* tau_online, int64_t N, const float* tau_target, int64_t N_target, float* out,
                     ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_iqn_next_dist: workspace is NULL");
    TS_REQUIRE(B >= 0, TS_ERR_INVALID_ARG, "ts_iqn_next_dist: negative batch");
    const bool two = params_old != nullptr;
    INet no, nt;
    if (int rc = make_inet(std::max<int64_t>(B, 1), N, c, h, w, n_act, n_cos, &no)) return rc;
    if (int rc = make_inet(std::max<int64_t>(B, 1), two ? N_target : N, c, h, w, n_act, n_cos, &nt)) return rc;
    if (B == 0) return TS_OK;
    TS_REQUIRE(params && obs_next_nhwc && tau_online && out && (!two || tau_target), TS_ERR_INVALID_ARG,
               "ts_iqn_next_dist: NULL argument");
    const size_t bytes_o = acts_bytes(no), bytes_t = two ? acts_bytes(nt) : 0;
    if (int rc = ts::ws_reserve(ws, bytes_o + bytes_t + al(8 * (size_t)B))) return rc;
    IActs ao, at;
    char* p = carve_acts(no, static_cast<char*>(ws->base), &ao);
    if (two) p = carve_acts(nt, p, &at);
    int64_t* act = reinterpret_cast<int64_t*>(p);
    hipStream_t s = ts::as_stream(stream), side;
    if (int rc = ts::side_stream(ws, s, &side)) return rc;
    if (two) {          // the lagged net's pass runs beside the online net's
        if (int rc = ts::stream_wait(ws, s, side, 9)) return rc;
        if (int rc = net_forward(side, ws, nt, params_old, obs_next_nhwc, obs_u8 != 0, tau_target, at)) return rc;
    }
    if (int rc = net_forward(s, ws, no, params, obs_next_nhwc, obs_u8 != 0, tau_online, ao)) return rc;
    hipLaunchKernelGGL(iqn_head_kernel, dim3((unsigned)ts::ceil_div(B, 4)), dim3(256), 0, s, ao.out, B, no.n_act, no.N, no.ld,
                       (float*)nullptr, (float*)nullptr, act);
    TS_LAUNCH_CHECK();
    if (two)
        if (int rc = ts::stream_wait(ws, side, s, 10)) return rc;
    hipLaunchKernelGGL(iqn_select_kernel, dim3((unsigned)ts::ceil_div(B * nt.N, 256)), dim3(256), 0, s, two ? at.out : ao.out,
                       act, B, nt.N, nt.ld, out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_iqn_update(ts_workspace* ws, float* params, float* adam_m, float* adam_v, int64_t adam_step, int64_t c, int64_t h,
                  int64_t w, int64_t n_act, int64_t n_cos, const void* obs_nhwc, int obs_u8, const int64_t* act,
                  const float* returns, int64_t N_target, const float* tau, int64_t N, const float* weight, int64_t B,
                  const ts_distq_hparams* hp, float* prio_out, float* loss_out, float* grad_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_iqn_update: workspace is NULL");
    TS_REQUIRE(B >= 1 && adam_step >= 1, TS_ERR_INVALID_ARG, "ts_iqn_update: bad batch size / step");
    TS_REQUIRE(N_target >= 2 && N_target <= MAX_N, TS_ERR_INVALID_ARG, "ts_iqn_update: 2 <= sample size (N, N') <= 64");
    INet n;
    if (int rc = make_inet(B, N, c, h, w, n_act, n_cos, &n)) return rc;
    TS_REQUIRE(params && adam_m && adam_v && obs_nhwc && act && returns && tau && hp && prio_out && loss_out,
               TS_ERR_INVALID_ARG, "ts_iqn_update: NULL argument");
    hipStream_t s = ts::as_stream(stream);
    const int Np = (int)N_target;
    const int64_t emb_elems = (int64_t)(KC + 1) * n.F;
    const bool emb_unfused = route_unfused(ROUTE_DEFAULT, n.R, false);
    const int emb_shares = embed_bwd_slabs(emb_unfused, B, n.N, n.F);

    // workspace: activations | d out, d h1, d x, d conv outputs | wgrad slabs (one set per layer: they run side by side) |
    // flat gradient | per-sample loss terms | norm partials
    size_t slab[5], slab_all = 0;
    for (int i = 0; i < 5; ++i) slab_all += slab[i] = al(4 * (size_t)ts::conv_wgrad_splits(n.l[i]) * n.l[i].param_elems());
    const size_t slab_e = al(4 * (size_t)emb_shares * emb_elems), phi_e = emb_unfused ? al(4 * (size_t)n.R * n.F) : 0;
    size_t bytes = acts_bytes(n) + slab_all + slab_e + phi_e + al(4 * (size_t)n.off[6]) + al(4 * (size_t)B) + 4096;
    for (int i = 0; i < 5; ++i) bytes += al(4 * (size_t)n.l[i].out_elems());
    bytes += al(4 * (size_t)n.R * n.F);
    if (int rc = ts::ws_reserve(ws, bytes)) return rc;
    IActs a;
    char* p = carve_acts(n, static_cast<char*>(ws->base), &a);
    auto take = [&](size_t floats) { float* r = reinterpret_cast<float*>(p); p += al(4 * floats); return r; };
    float* dy[5];
    for (int i = 0; i < 5; ++i) dy[i] = take((size_t)n.l[i].out_elems());
    float* dx = take((size_t)n.R * n.F);
    float* slabs[5];
    for (int i = 0; i < 5; ++i) { slabs[i] = reinterpret_cast<float*>(p); p += slab[i]; }
    float* slabs_e = reinterpret_cast<float*>(p); p += slab_e;
    float* phi_s = reinterpret_cast<float*>(p); p += phi_e;
    float* grad = take((size_t)n.off[6]);
    float* lw = take((size_t)B);
    float* norm_part = reinterpret_cast<float*>(p);
    if (grad_out) grad = grad_out;

    if (int rc = net_forward(s, ws, n, params, obs_nhwc, obs_u8 != 0, tau, a)) return rc;
    hipLaunchKernelGGL(iqn_loss_kernel, dim3((unsigned)B), dim3(256), 0, s, a.out, act, returns, weight, tau, B, n.n_act, n.N, Np, n.ld,
                       dy[4], prio_out, lw);
    hipLaunchKernelGGL(iqn_mean_kernel, dim3(1), dim3(1024), 0, s, lw, B, loss_out);
    TS_LAUNCH_CHECK();
    if (int rc = ts::record_td(ws, s)) return rc;        // prio_out / loss_out are written: ts_dqn_wait_td

    // fc2, fc1, embedding: input gradients down the caller's stream, each weight gradient (+ its slab sum) beside them on a
    // side stream of the workspace; the trunk follows through ts::chain_backward, which joins both side streams at its end.
    hipStream_t sv, sw;
    if (int rc = ts::side_streams(ws, s, &sv, &sw)) return rc;
    auto wgrad = [&](hipStream_t st, int i, const float* xin) -> int {
        if (int rc = ts::conv_wgrad(st, n.l[i], xin, dy[i], slabs[i], ws)) return rc;
        return ts::slab_sum(st, slabs[i], ts::conv_wgrad_splits(n.l[i]), n.l[i].param_elems(), grad + n.off[i + 1]);
    };
    if (int rc = ts::stream_wait(ws, s, sv, 11)) return rc;                                         // d out
    if (int rc = wgrad(sv, 4, a.h1)) return rc;
    if (int rc = ts::conv_dgrad(s, n.l[4], dy[4], params + n.off[5], a.h1, dy[3], ws)) return rc;   // d h1 (ReLU mask: h1)
    if (int rc = ts::stream_wait(ws, s, sw, 12)) return rc;
    if (int rc = wgrad(sw, 3, a.x)) return rc;
    if (int rc = ts::conv_dgrad(s, n.l[3], dy[3], params + n.off[4], nullptr, dx, ws)) return rc;   // d x: no ReLU below fc1
    if (int rc = embed_backward(s, ws, emb_unfused, tau, a.c[2], params + n.off[3], dx, B, n.N, n.F, dy[2], slabs_e, a.cosv, phi_s))
        return rc;
    if (int rc = ts::stream_wait(ws, s, sv, 13)) return rc;
    if (int rc = ts::slab_sum(sv, slabs_e, emb_shares, emb_elems, grad + n.off[3])) return rc;
    {
        const float* x[3]; const float* wb[3]; float* g[3];
        for (int i = 0; i < 3; ++i) {
            x[i] = i == 0 ? static_cast<const float*>(obs_nhwc) : a.c[i - 1];
            wb[i] = params + n.off[i];
            g[i] = grad + n.off[i];
        }
        if (int rc = ts::chain_backward(s, ws, 3, n.l, x, dy, wb, slabs, g, obs_u8 != 0)) return rc;
    }
    if (hp->lr < 0.0) return TS_OK;
    return ts::adam_step(s, params, adam_m, adam_v, grad, n.off[6], adam_step, hp->lr, hp->beta1, hp->beta2, hp->adam_eps,
                         hp->max_grad_norm, norm_part);
}

}  // extern "C"
