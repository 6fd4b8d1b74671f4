// ts_mlp_tile.h -- what the one-tile-per-workgroup MLP kernels share (ts_dqn_mlp.hip, ts_qrdqn_mlp.hip): a 256-thread workgroup
// (four waves) owns 32 batch rows, every hidden activation of the tile stays in an odd-pitch LDS array (width + 1 floats per
// row), the weights are streamed from L2 into v_mfma_f32_32x32x2_f32 operands.  The layer passes below are called by every
// thread of the workgroup; the caller places the barriers.  Flat parameter vector: per layer [K + 1, N], row K the bias.
// Include behind `#pragma clang fp contract(off)`.
#pragma once

#include "ts_common.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TILE = 32;
constexpr int THREADS = 256;
constexpr int LDS_LIMIT = 160 * 1024;       // workgroup limit of gfx950

__device__ __forceinline__ int featF(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

struct Lay { int K, N, off; };              // weights params[off + k N + n], bias params[off + K N + n]

// The description is indexed by run-time layer numbers: staged from the kernel arguments into LDS once, so that those reads are
// LDS reads (indexing the by-value argument itself would spill it to scratch memory).
template <typename NetT>
__device__ const NetT& stage_net(const NetT& arg) {
    __shared__ NetT staged;
    constexpr int WORDS = sizeof(NetT) / 4;
    static_assert(WORDS <= THREADS && sizeof(NetT) % 4 == 0 && sizeof(NetT) <= 256, "one word per thread, within the reserved 256 bytes");
    if (threadIdx.x < WORDS) reinterpret_cast<int*>(&staged)[threadIdx.x] = reinterpret_cast<const int*>(&arg)[threadIdx.x];
    __syncthreads();
    return staged;
}

// Y[32][N] = relu(X[32][K] W + b): block n on wave n mod 4; lane (i, h) supplies A(i, k + h) = X[i][k + h] and B(k + h, i) = W[k + h][n0 + i]
__device__ void dense_relu(const float* __restrict__ w, int K, int N, const float* X, int px, float* Y, int py) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    for (int nb = wave; nb < N / 32; nb += 4) {
        const int n = nb * 32 + i;
        const float* wp = w + n;
        const float* xp = X + i * px + h;
        f32x16 acc = {};
        int k = 0;
#pragma unroll 8
        for (; k + 2 <= K; k += 2) acc = mfma32(xp[k], wp[(size_t)(k + h) * N], acc);
        if (k < K) acc = mfma32(h == 0 ? X[i * px + k] : 0.f, h == 0 ? wp[(size_t)k * N] : 0.f, acc);     // odd K: the last pair is half empty
        const float bias = wp[(size_t)K * N];
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[featF(r, h) * py + n] = fmaxf(acc[r] + bias, 0.f);
    }
}

// the tile's observations -> sm[net.x_at ..], pitch obs_dim + 1.  Ends behind a barrier.
template <typename NetT>
__device__ void load_obs(const NetT& net, const float* __restrict__ obs, int64_t row0, int64_t B, float* sm) {
    const int d = net.obs_dim;
    for (int idx = threadIdx.x; idx < TILE * d; idx += THREADS) {
        const int row = idx / d, c = idx - row * d;
        sm[net.x_at + row * (d + 1) + c] = row0 + row < B ? obs[(row0 + row) * d + c] : 0.f;       // rows beyond B: zeros, never read from memory
    }
    __syncthreads();
}

// slab[k N + n] = sum_m Hin[m][k] dZ[m][n] (32 x 32 blocks round-robin over the waves), slab[K N + n] = sum_m dZ[m][n]
__device__ void wgrad(float* __restrict__ slab, const float* Hin, int pin, int K, const float* dZ, int pz, int N) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int nbs = N / 32, kbs = (K + 31) / 32;
    for (int blk = wave; blk < kbs * nbs; blk += 4) {
        const int kb = blk / nbs, nb = blk - kb * nbs;
        const int kc = kb * 32 + i, n = nb * 32 + i;
        const bool live = kc < K;                                   // (obs_dim is no multiple of 32)
        f32x16 acc = {};
#pragma unroll
        for (int m = 0; m < TILE; m += 2) acc = mfma32(live ? Hin[(m + h) * pin + kc] : 0.f, dZ[(m + h) * pz + n], acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = kb * 32 + featF(r, h);
            if (k < K) slab[(size_t)k * N + n] = acc[r];
        }
    }
    for (int n = threadIdx.x; n < N; n += THREADS) {
        float s = 0.f;
        for (int m = 0; m < TILE; ++m) s += dZ[m * pz + n];
        slab[(size_t)K * N + n] = s;
    }
}

struct MSrc { const float* dz; int pz; const float* w; int N; };    // a hidden layer above: dZ[32][N] (LDS), W[Kt][N]
struct HSrc { const float* dq; int pq; const float* w; int A; };    // a head above: dq[32][A] (LDS), W[Kt][A]

// H[32][Kt] <- (sum over the sources of dZ W^T) * (H > 0), in place.  Block k on wave k mod 4; A(i, n) = dZ[i][n] from LDS,
// B(n, i) = W[k0 + i][n] as 16-byte loads along n (lane half h takes n = 8 j + 4 h + e: the same permutation on both operands).
__device__ void dgrad(float* H, int ph, int Kt, MSrc m0, MSrc m1, HSrc h0, HSrc h1) {      // a source with a NULL array is absent
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    for (int kb = wave; kb < Kt / 32; kb += 4) {
        const int kc = kb * 32 + i;
        f32x16 acc = {};
        for (int s = 0; s < 2; ++s) {
            const MSrc m = s ? m1 : m0;
            if (!m.dz) continue;
            const int N = m.N;
            const float* wrow = m.w + (size_t)kc * N + 4 * h;
            const float* zp = m.dz + i * m.pz + 4 * h;
#pragma unroll 2
            for (int n = 0; n < N; n += 8) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(wrow + n);
                acc = mfma32(zp[n], w4[0], acc);
                acc = mfma32(zp[n + 1], w4[1], acc);
                acc = mfma32(zp[n + 2], w4[2], acc);
                acc = mfma32(zp[n + 3], w4[3], acc);
            }
        }
        for (int s = 0; s < 2; ++s) {
            const HSrc hd = s ? h1 : h0;
            if (!hd.dq) continue;
            const int A = hd.A;
            const float* wrow = hd.w + (size_t)kc * A;
            for (int a = 0; a < A; ++a) {
                const float w = wrow[a];
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] += hd.dq[featF(r, h) * hd.pq + a] * w;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float* p = H + featF(r, h) * ph + kc;
            *p = *p > 0.f ? acc[r] : 0.f;
        }
    }
}

// ---- the last launch of an update: slabs and loss partials in tile order, lagged copy of the pre-step parameters, Adam --------
struct ApplyArgs {
    float* p; float* m; float* v; float* p_old;         // p_old != NULL: this call synchronises the lagged network (dqn.py:283-285)
    const float* slabs; const float* partials; int tiles; int P;
    float* grad_out; float* loss_out;
    int adam;                                           // 0: gradient only
    float lr_step, beta2, bc2_sqrt, eps, omb1, omb2;
};

__global__ __launch_bounds__(THREADS) void dqnm_apply_kernel(ApplyArgs a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i == 0) {
        float s = 0.f;
        for (int t = 0; t < a.tiles; ++t) s += a.partials[t];
        a.loss_out[0] = s;
    }
    if (i >= a.P) return;
    float g = 0.f;
    for (int t = 0; t < a.tiles; ++t) g += a.slabs[(size_t)t * a.P + i];
    if (a.grad_out) a.grad_out[i] = g;
    const float p = a.p[i];
    if (a.p_old) a.p_old[i] = p;
    if (!a.adam) return;
    float m = a.m[i], v = a.v[i];
    m = m + (g - m) * a.omb1;                            // exp_avg.lerp_(grad, 1 - beta1)
    v = v * a.beta2 + a.omb2 * g * g;                    // mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    a.p[i] = p + (-a.lr_step * m) / denom;               // addcdiv_(m, denom, -step_size)
    a.m[i] = m;
    a.v[i] = v;
}

// ---- host: the workspace of an update and its last launch ---------------------------------------------------------------------------

// slabs [tiles][P] | partials [tiles] | grad_ws [P] (the summed gradient on its way to the clip) | norm_part [1024] (optim_step's
// scratch); every region but the first starts on a 64-float boundary.  `bytes` is the reserved and reported size: the carve and
// what is left of the padding the size has always had.
struct UpdateScratch { float *slabs, *partials, *grad_ws, *norm_part; size_t bytes; };

// base == NULL: only `bytes` is filled
inline UpdateScratch update_scratch(void* base, int64_t tiles, int64_t P) {
    auto r64 = [](size_t n) { return (n + 63) / 64 * 64; };
    const size_t partials = (size_t)tiles * (size_t)P, grad_ws = partials + r64((size_t)tiles), norm_part = grad_ws + r64((size_t)P);
    UpdateScratch u{};
    u.bytes = ((size_t)tiles * (size_t)P + (size_t)tiles + (size_t)P) * 4 + 4096 + 1024;
    static_assert(2 * 63 * 4 <= 1024, "the two roundings fit the padding behind norm_part's 4096 bytes");
    if (base) {
        u.slabs = static_cast<float*>(base);
        u.partials = u.slabs + partials;
        u.grad_ws = u.slabs + grad_ws;
        u.norm_part = u.slabs + norm_part;
    }
    return u;
}

// The last launch of ts_{dqn,qrdqn,c51,rainbow,iqn}_mlp_update on the slabs and partials the step kernel left in `u`; `hp` is a
// ts_dqn_hparams or a ts_distq_hparams (lr < 0: gradient only).  params_old != NULL: this call synchronises the lagged network.
template <typename HP>
int apply_tiles(hipStream_t s, const UpdateScratch& u, int tiles, int P, float* params, float* params_old, float* m, float* v,
                int64_t adam_step, const HP* hp, float* grad_out, float* loss_out) {
    const bool step = hp->lr >= 0.0, clip = step && hp->max_grad_norm > 0.0;
    ApplyArgs aa{};
    aa.p = params; aa.m = m; aa.v = v; aa.p_old = params_old;
    aa.slabs = u.slabs; aa.partials = u.partials; aa.tiles = tiles; aa.P = P;
    aa.grad_out = grad_out ? grad_out : (clip ? u.grad_ws : nullptr);
    aa.loss_out = loss_out;
    aa.adam = step && !clip;               // clip_grad_norm_ needs the whole gradient first: the sum here, then ts_adam_step's kernels
    float sc[2];
    ts::adam_step_scalars(adam_step, hp->lr, hp->beta1, hp->beta2, sc);
    aa.lr_step = sc[0]; aa.bc2_sqrt = sc[1];
    aa.beta2 = (float)hp->beta2; aa.eps = (float)hp->adam_eps;
    aa.omb1 = (float)(1.0 - hp->beta1); aa.omb2 = (float)(1.0 - hp->beta2);
    hipLaunchKernelGGL(dqnm_apply_kernel, dim3((unsigned)ts::ceil_div(P, THREADS)), dim3(THREADS), 0, s, aa);
    TS_LAUNCH_CHECK();
    if (!clip) return TS_OK;
    return ts::optim_step(s, ts::OptimDesc{}, params, m, v, aa.grad_out, P, adam_step, hp->lr, hp->beta1, hp->beta2, hp->adam_eps,
                          hp->max_grad_norm, u.norm_part);
}

}  // namespace
