// ts_iqn_mlp.hip -- IQN on vector observations: `ImplicitQuantileNetwork(preprocess_net=Net(...), hidden_sizes=H, num_cosines=C)`
// (utils/net/discrete.py:126-216) under QRDQN._target_q / IQN._update_with_batch (modelfree/qrdqn.py:94-106, iqn.py:156-183).
// An update is two launches (step, apply), a target pass is one.
//
// The tile is ts_dqn_mlp.hip's (ts_mlp_tile.h): one four-wave workgroup per 32 batch rows, activations resident in odd-pitch LDS,
// weights streamed from L2 into v_mfma_f32_32x32x2_f32 operands, one gradient slab per tile summed in tile order by
// dqnm_apply_kernel.  The network is evaluated on B N virtual rows (row b under each of its N sampled fractions); here that is
// THE SAMPLE WALK: the trunk runs once per tile, its features f[32][F] stay in LDS, and the samples j = 0 .. N - 1 are taken one
// after the other, so the LDS footprint depends neither on N nor on A.  Sample j:
//   cs[32][C | 1]  = cos(tau[row][j] * ipi[k]), ipi[k] = fl32(fl32(pi) * (k + 1)), the product rounded to float32 (no contraction
//                    in this file), an accurate cosf: the argument of ts_iqn.hip, which is torch's (discrete.py:148-155)
//   phi[32][F]     = relu(cs We + be)
//   x_j            = f (.) phi is never stored: the layer that reads it multiplies the two LDS operands on the way into the MFMA
//   `last`         = 0 .. 2 ReLU layers, then the final Linear as ONE masked 32-column block (A <= 32) on wave 0 -> ob[32][33]
// Features: the Net's linear output layer (dense<.., RELU = false>, its own LDS array) or, without one, its last ReLU layer.
//   * INFER  (ts_iqn_mlp_forward): logits straight to [B, A, N], q = the mean over the samples in registers of thread (row, t) for
//     the actions a = t (mod 8), the arg-max strictly greater (the first index wins a tie).
//   * TARGET (ts_iqn_mlp_next_dist): the online network is walked over tau_online and leaves q[32][A] -> sel[32]; the evaluating
//     network (the lagged one, or the same network again: a bit-identical recompute that skips the trunk) is walked over its
//     fractions and stores column sel[row] of every sample into kept[32][65]; epilogue float(double(theta' mask) gamma^n + mc).
//   * STEP   (ts_iqn_mlp_update): the forward walk stores theta[32][65] (the taken action's quantile of every sample); the pair
//     loss is ts_qrdqn_mlp.hip's with tau = tau[b][i] and N' targets; the backward walk recomputes sample j's cs, phi and `last`
//     activations with the same code and backpropagates.  d x_j is never stored either: the block that produces it ends in
//     df += dx (.) phi, phi <- dx (.) f (.) (phi > 0) on the element its lane owns for the whole walk.  The slab blocks of We, be
//     and `last` are read-modify-written per sample (written on j = 0): each 32 x 32 block belongs to one wave for the whole walk,
//     so += has no race and a fixed order, j ascending.  Then the trunk backward runs on df (wgrad / dgrad of ts_mlp_tile.h).
//     Rows beyond B: sel = -1, tau = 0, theta = d theta = 0: exactly zero in the loss and in every slab.
// Flat parameter vector, per layer [K + 1, N] (row K = bias): trunk | feature output layer (if any) | [We; be] [C + 1, F] | `last`
// hidden layers | final Linear [top + 1, A].
#pragma clang fp contract(off)
#include <algorithm>

#include "ts_atom_head.h"     // RPT, row_sum8, tiles_of, check_batch (and ts_mlp_tile.h)
#include "ts_qr_terms.h"

namespace {

constexpr int MAX_LAST = 2, MAX_COS = 64, MAX_SAMPLES = 64;
constexpr int TP = MAX_SAMPLES | 1;         // pitch of the per-row sample tables
constexpr int OP = TILE + 1;                // pitch of the head's output block

struct INet {
    int obs_dim, n_act, nt, nh, n_cos, feat_lin, F;
    Lay t[MAX_TRUNK], fo, emb, h[MAX_LAST], head;
    int x_at, t_at[MAX_TRUNK], f_at, cs_at, pc, phi_at, h_at[MAX_LAST], df_at, ob_at, th_at, tg_at, row_at;
    int P, lds_floats;
};

// Y[32][N] = act((X (.) X2) W + b); PROD false: X alone.  The lane mapping of dense_relu; K is a hidden width (even).
template <bool PROD, bool RELU>
__device__ void dense(const float* __restrict__ w, int K, int N, const float* X, const float* X2, int px, float* Y, int py) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    for (int nb = wave; nb < N / 32; nb += 4) {
        const int n = nb * 32 + i;
        const float* wp = w + n;
        const float* xp = X + i * px + h;
        const float* x2p = X2 + i * px + h;
        f32x16 acc = {};
#pragma unroll 8
        for (int k = 0; k < K; k += 2) acc = mfma32(PROD ? xp[k] * x2p[k] : xp[k], wp[(size_t)(k + h) * N], acc);
        const float bias = wp[(size_t)K * N];
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[featF(r, h) * py + n] = RELU ? fmaxf(acc[r] + bias, 0.f) : acc[r] + bias;
    }
}

// the final Linear: ob[32][A] = (X (.) X2) W + b as one 32-column block on wave 0, the weight loads masked past column A
template <bool PROD>
__device__ void head_block(const float* __restrict__ w, int K, int A, const float* X, const float* X2, int px, float* ob) {
    if (threadIdx.x >= 64) return;
    const int i = threadIdx.x & 31, h = threadIdx.x >> 5;
    const bool live = i < A;
    const float* wp = w + (live ? i : 0);                      // past column A: column 0 is read, 0 is used
    const float* xp = X + i * px + h;
    const float* x2p = X2 + i * px + h;
    f32x16 acc = {};
#pragma unroll 8
    for (int k = 0; k < K; k += 2) {
        const float b = wp[(size_t)(k + h) * A];
        acc = mfma32(PROD ? xp[k] * x2p[k] : xp[k], live ? b : 0.f, acc);
    }
    const float bias = wp[(size_t)K * A];
    if (live) {
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[featF(r, h) * OP + i] = acc[r] + bias;
    }
}

// the trunk (and the Net's linear output layer) on the tile whose observations are in LDS -> the features.  Ends behind a barrier.
__device__ const float* features(const INet& net, const float* __restrict__ p, float* sm) {
    const float* x = sm + net.x_at;
    int px = net.obs_dim + 1;
    for (int l = 0; l < net.nt; ++l) {
        float* y = sm + net.t_at[l];
        dense_relu(p + net.t[l].off, net.t[l].K, net.t[l].N, x, px, y, net.t[l].N + 1);
        __syncthreads();
        x = y; px = net.t[l].N + 1;
    }
    if (!net.feat_lin) return x;
    dense<false, false>(p + net.fo.off, net.fo.K, net.F, x, x, px, sm + net.f_at, net.F + 1);
    __syncthreads();
    return sm + net.f_at;
}

// sample j up to the top of `last`'s hidden layers: cs, phi, h[0], h[1].  Ends behind a barrier.
__device__ void sample_hidden(const INet& net, const float* __restrict__ p, const float* fa, float* sm, const float* __restrict__ tau, int N,
                              int j, int64_t row0, int64_t B) {
    float* cs = sm + net.cs_at;
    float* phi = sm + net.phi_at;
    const int C = net.n_cos, pc = net.pc, pf = net.F + 1;
    for (int e = threadIdx.x; e < TILE * C; e += THREADS) {                  // one cosine per (row, k)
        const int i = e / C, k = e - i * C;
        const float t = row0 + i < B ? tau[(row0 + i) * N + j] : 0.f;
        const float ipi = 3.14159274101257324f * (float)(k + 1);
        cs[i * pc + k] = cosf(t * ipi);
    }
    __syncthreads();
    dense_relu(p + net.emb.off, C, net.F, cs, pc, phi, pf);
    __syncthreads();
    if (net.nh >= 1) {
        dense<true, true>(p + net.h[0].off, net.F, net.h[0].N, fa, phi, pf, sm + net.h_at[0], net.h[0].N + 1);
        __syncthreads();
    }
    if (net.nh == 2) {
        dense_relu(p + net.h[1].off, net.h[1].K, net.h[1].N, sm + net.h_at[0], net.h[0].N + 1, sm + net.h_at[1], net.h[1].N + 1);
        __syncthreads();
    }
}

// the final Linear of the sample whose hidden activations are in LDS -> ob.  Ends behind a barrier.
__device__ void sample_head(const INet& net, const float* __restrict__ p, const float* fa, float* sm) {
    float* ob = sm + net.ob_at;
    if (net.nh == 0) head_block<true>(p + net.head.off, net.F, net.n_act, fa, sm + net.phi_at, net.F + 1, ob);
    else head_block<false>(p + net.head.off, net.head.K, net.n_act, sm + net.h_at[net.nh - 1], sm + net.h_at[net.nh - 1], net.head.K + 1, ob);
    __syncthreads();
}

// ---- INFER: ImplicitQuantileNetwork.forward + the mean over the samples + the greedy action; TARGET: QRDQN._target_q -------------
struct WalkArgs {
    INet net;
    const float* params; const float* params_old;      // params_old NULL: no lagged network
    const float* obs; int64_t B;
    const float* tau; int N;                            // the online network's fractions [B, N]
    const float* tau2; int N2;                          // TARGET: the evaluating network's fractions [B, N2]
    float* logits; float* q_out; int64_t* act_out;      // INFER
    float* out;                                         // TARGET: [B, N2], the n-step returns when mask != NULL
    const float* mask; const double* gpow; const double* mc;
};

template <bool INFER>
__global__ __launch_bounds__(THREADS) void iqnm_walk_kernel(WalkArgs a) {
    extern __shared__ float sm[];
    const INet& net = stage_net(a.net);
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7, A = net.n_act;
    const int64_t b = row0 + row;
    load_obs(net, a.obs, row0, a.B, sm);
    const float* fa = features(net, a.params, sm);
    float* ob = sm + net.ob_at;
    int* sel = reinterpret_cast<int*>(sm + net.row_at);
    float qa[4] = {0.f, 0.f, 0.f, 0.f};                 // thread (row, t): the sample sums of the actions t, t + 8, t + 16, t + 24
    for (int j = 0; j < a.N; ++j) {
        sample_hidden(net, a.params, fa, sm, a.tau, a.N, j, row0, a.B);
        sample_head(net, a.params, fa, sm);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int act = t + RPT * u;
            if (act < A) {
                const float v = ob[row * OP + act];
                qa[u] += v;
                if (INFER && a.logits && b < a.B) a.logits[(b * A + act) * a.N + j] = v;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {                       // (each thread overwrites the entries it alone read)
        const int act = t + RPT * u;
        if (act < A) {
            const float q = qa[u] / (float)a.N;
            ob[row * OP + act] = q;
            if (INFER && a.q_out && b < a.B) a.q_out[b * A + act] = q;
        }
    }
    __syncthreads();
    if (t == 0) {
        float best = ob[row * OP];
        int arg = 0;
        for (int act = 1; act < A; ++act) {
            const float q = ob[row * OP + act];
            if (q > best) { best = q; arg = act; }      // strictly greater: the first index wins ties
        }
        sel[row] = arg;
        if (INFER && a.act_out && b < a.B) a.act_out[b] = arg;
    }
    if (INFER) return;
    __syncthreads();
    const bool two = a.params_old != nullptr;
    const float* pe = two ? a.params_old : a.params;
    if (two) fa = features(net, pe, sm);                // (the observations are still in LDS)
    float* kept = sm + net.th_at;
    const int s = sel[row];
    for (int j = 0; j < a.N2; ++j) {
        sample_hidden(net, pe, fa, sm, a.tau2, a.N2, j, row0, a.B);
        sample_head(net, pe, fa, sm);
        if ((s & 7) == t) kept[row * TP + j] = ob[row * OP + s];
    }
    __syncthreads();
    if (b >= a.B) return;
    if (a.mask) {                                       // compute_nstep_return's arithmetic, per quantile
        const float mk = a.mask[b];
        const double gp = a.gpow[b], mc = a.mc[b];
        for (int j = t; j < a.N2; j += RPT) a.out[b * a.N2 + j] = (float)((double)(kept[row * TP + j] * mk) * gp + mc);
    } else {
        for (int j = t; j < a.N2; j += RPT) a.out[b * a.N2 + j] = kept[row * TP + j];
    }
}

// ---- STEP: forward walk, pair loss, backward walk, trunk backward, the tile's slab -------------------------------------------------

// slab[k N + n] (+)= sum_m (Hin (.) Hin2)[m][k] dZ[m][n], slab[K N + n] (+)= sum_m dZ[m][n]: wgrad's blocks (32 x 32, round-robin over
// the waves, so a block has one owner wave and an element one owner lane for the whole walk), K and N of any size (masked loads).
// `first`: the sample that writes instead of adding.
template <bool PROD>
__device__ void wgrad_acc(float* __restrict__ slab, bool first, const float* Hin, const float* Hin2, int pin, int K, const float* dZ, int pz, int N) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int nbs = (N + 31) / 32, kbs = (K + 31) / 32;
    for (int blk = wave; blk < kbs * nbs; blk += 4) {
        const int kb = blk / nbs, nb = blk - kb * nbs;
        const int kc = kb * 32 + i, n = nb * 32 + i;
        const bool klive = kc < K, nlive = n < N;
        const int kk = klive ? kc : 0, nn = nlive ? n : 0;
        f32x16 acc = {};
#pragma unroll
        for (int m = 0; m < TILE; m += 2) {
            float hv = Hin[(m + h) * pin + kk];
            if (PROD) hv *= Hin2[(m + h) * pin + kk];
            const float z = dZ[(m + h) * pz + nn];
            acc = mfma32(klive ? hv : 0.f, nlive ? z : 0.f, acc);
        }
        if (nlive) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = kb * 32 + featF(r, h);
                if (k < K) {
                    float* s = slab + (size_t)k * N + n;
                    *s = first ? acc[r] : *s + acc[r];
                }
            }
        }
    }
    for (int n = threadIdx.x; n < N; n += THREADS) {
        float s = 0.f;
        for (int m = 0; m < TILE; ++m) s += dZ[m * pz + n];
        float* q = slab + (size_t)K * N + n;
        *q = first ? s : *q + s;
    }
}

// dx[32][F] = dZ W^T from one source (a hidden layer above: dgrad's MFMA pass; or the final Linear: dgrad's head pass), not stored:
// the lane that owns element (m, k) adds dx phi to df and replaces phi by d phi = dx f (phi > 0)
__device__ void dgrad_embed(float* phi, float* df, const float* fa, int pf, int F, MSrc ms, HSrc hd) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    for (int kb = wave; kb < F / 32; kb += 4) {
        const int kc = kb * 32 + i;
        f32x16 acc = {};
        if (ms.dz) {
            const int N = ms.N;
            const float* wrow = ms.w + (size_t)kc * N + 4 * h;
            const float* zp = ms.dz + i * ms.pz + 4 * h;
#pragma unroll 2
            for (int n = 0; n < N; n += 8) {
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(wrow + n);
                acc = mfma32(zp[n], w4[0], acc);
                acc = mfma32(zp[n + 1], w4[1], acc);
                acc = mfma32(zp[n + 2], w4[2], acc);
                acc = mfma32(zp[n + 3], w4[3], acc);
            }
        } else {
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
            const int idx = featF(r, h) * pf + kc;
            const float dx = acc[r], ph = phi[idx];
            df[idx] += dx * ph;
            phi[idx] = ph > 0.f ? dx * fa[idx] : 0.f;
        }
    }
}

struct StepArgs {
    INet net;
    const float* params; const float* obs; const int64_t* act;
    const float* tau; int N; const float* returns; int N2; const float* weight;
    int64_t B;
    float* prio_out; float* slabs; float* partials;
};

__global__ __launch_bounds__(THREADS) void iqnm_step_kernel(StepArgs a) {
    extern __shared__ float sm[];
    const INet& net = stage_net(a.net);
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    const float* p = a.params;
    float* slab = a.slabs + (size_t)blockIdx.x * net.P;
    float* th = sm + net.th_at;                              // theta of the taken action per sample, then d loss / d theta
    float* tg = sm + net.tg_at;                              // the targets T
    float* ob = sm + net.ob_at;                              // the head's output block, then its gradient
    float* phi = sm + net.phi_at;
    float* df = sm + net.df_at;
    float* term = sm + net.row_at + TILE;
    int* sel = reinterpret_cast<int*>(sm + net.row_at);
    const int N = a.N, N2 = a.N2, A = net.n_act, F = net.F, pf = F + 1, nh = net.nh;
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7;
    if (threadIdx.x < TILE) {                                // rows beyond B select nothing: exactly zero in the loss and in every slab
        const int64_t b = row0 + threadIdx.x;
        int s = -1;
        if (b < a.B) {
            const int64_t ab = a.act[b];
            s = ab < 0 ? 0 : ab >= A ? A - 1 : (int)ab;
        }
        sel[threadIdx.x] = s;
    }
    for (int idx = threadIdx.x; idx < TILE * TP; idx += THREADS) {
        const int r = idx / TP, j = idx - r * TP;
        th[idx] = 0.f;
        tg[idx] = row0 + r < a.B && j < N2 ? a.returns[(row0 + r) * N2 + j] : 0.f;
    }
    for (int idx = threadIdx.x; idx < TILE * pf; idx += THREADS) df[idx] = 0.f;
    load_obs(net, a.obs, row0, a.B, sm);
    const float* fa = features(net, p, sm);
    const int s = sel[row];
    for (int j = 0; j < N; ++j) {                            // the forward walk
        sample_hidden(net, p, fa, sm, a.tau, N, j, row0, a.B);
        sample_head(net, p, fa, sm);
        if (s >= 0 && (s & 7) == t) th[row * TP + j] = ob[row * OP + s];
    }
    __syncthreads();
    {   // the pair loss of row (tid >> 3): thread t takes theta_i, i = t (mod 8), against the row's N' targets
        const int64_t b = row0 + row;
        const bool live = b < a.B;
        const float wb = live ? (a.weight ? a.weight[b] : 1.f) : 0.f;
        const float scale = wb / ((float)a.B * (float)N);
        float wl = 0.f, sl = 0.f;
        if (live) {
            float* mine = th + row * TP;
            for (int i = t; i < N; i += RPT) {
                float li, ai, g;
                qr_terms(tg + row * TP, N2, mine[i], a.tau[b * N + i], li, ai, g);
                mine[i] = -g * scale;                        // only this thread reads theta_i
                wl += li;
                sl += ai;
            }
        }
        wl = row_sum8(wl);
        sl = row_sum8(sl);
        if (t == 0) {
            const float huber = wl / (float)N;
            if (live) a.prio_out[b] = sl / (float)N;
            term[row] = live ? huber * wb / (float)a.B : 0.f;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        for (int m = 0; m < TILE; ++m) sum += term[m];
        a.partials[blockIdx.x] = sum;
    }
    float* h0 = sm + net.h_at[0];
    float* h1 = sm + net.h_at[1];
    const int p0 = net.h[0].N + 1, p1 = net.h[1].N + 1;
    for (int j = 0; j < N; ++j) {                            // the backward walk: the slab blocks take sample j, j ascending
        const bool first = j == 0;
        sample_hidden(net, p, fa, sm, a.tau, N, j, row0, a.B);
        for (int idx = threadIdx.x; idx < TILE * TILE; idx += THREADS) {
            const int m = idx >> 5, c = idx & 31;
            ob[m * OP + c] = c == sel[m] ? th[m * TP + j] : 0.f;
        }
        __syncthreads();
        const HSrc hs{ob, OP, p + net.head.off, A};
        if (nh == 0) {
            wgrad_acc<true>(slab + net.head.off, first, fa, phi, pf, F, ob, OP, A);
            __syncthreads();
            dgrad_embed(phi, df, fa, pf, F, MSrc{}, hs);
        } else {
            float* top = nh == 2 ? h1 : h0;
            const int ptop = nh == 2 ? p1 : p0;
            wgrad_acc<false>(slab + net.head.off, first, top, top, ptop, net.head.K, ob, OP, A);
            __syncthreads();
            dgrad(top, ptop, net.head.K, MSrc{}, MSrc{}, hs, HSrc{});
            __syncthreads();
            if (nh == 2) {
                wgrad_acc<false>(slab + net.h[1].off, first, h0, h0, p0, net.h[1].K, h1, p1, net.h[1].N);
                __syncthreads();
                dgrad(h0, p0, net.h[0].N, MSrc{h1, p1, p + net.h[1].off, net.h[1].N}, MSrc{}, HSrc{}, HSrc{});
                __syncthreads();
            }
            wgrad_acc<true>(slab + net.h[0].off, first, fa, phi, pf, F, h0, p0, net.h[0].N);
            __syncthreads();
            dgrad_embed(phi, df, fa, pf, F, MSrc{h0, p0, p + net.h[0].off, net.h[0].N}, HSrc{});
        }
        __syncthreads();
        wgrad_acc<false>(slab + net.emb.off, first, sm + net.cs_at, sm + net.cs_at, net.pc, net.n_cos, phi, pf, F);
        __syncthreads();                                     // the next sample overwrites cs and phi
    }
    // the trunk backward on df
    float* top = sm + net.t_at[net.nt - 1];
    const int ptop = net.t[net.nt - 1].N + 1;
    if (net.feat_lin) {
        wgrad(slab + net.fo.off, top, ptop, net.fo.K, df, pf, F);
        __syncthreads();
        dgrad(top, ptop, net.fo.K, MSrc{df, pf, p + net.fo.off, F}, MSrc{}, HSrc{}, HSrc{});
    } else {                                                 // the features are the top ReLU layer itself (pitch pf)
        for (int idx = threadIdx.x; idx < TILE * F; idx += THREADS) {
            const int r = idx / F, o = r * pf + idx - r * F;
            top[o] = top[o] > 0.f ? df[o] : 0.f;
        }
    }
    __syncthreads();
    for (int l = net.nt - 1; l >= 0; --l) {
        const float* in = l > 0 ? sm + net.t_at[l - 1] : sm + net.x_at;
        wgrad(slab + net.t[l].off, in, l > 0 ? net.t[l - 1].N + 1 : net.obs_dim + 1, net.t[l].K, sm + net.t_at[l], net.t[l].N + 1, net.t[l].N);
        if (l == 0) break;
        __syncthreads();
        MSrc ms{sm + net.t_at[l], net.t[l].N + 1, p + net.t[l].off, net.t[l].N};
        dgrad(sm + net.t_at[l - 1], net.t[l - 1].N + 1, net.t[l - 1].N, ms, MSrc{}, HSrc{}, HSrc{});
        __syncthreads();
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------

// desc (host, TS_IQN_MLP_DESC_LEN int64): {obs_dim, n_act, n_trunk, trunk[4], width of the Net's linear output layer (0: none, the
// features are the last ReLU layer), num_cosines, n_last, last_hidden[2]}.  LDS carve of one tile, in floats: obs 32 (obs_dim + 1) +
// trunk layers 32 (width + 1) + [features 32 (F + 1)] + cs 32 (C | 1) + phi 32 (F + 1) + `last` hidden layers 32 (width + 1) +
// df 32 (F + 1) + ob 32 x 33 + two sample tables 32 x 65 + 4 x 32 per-row scalars, and 256 bytes for the staged description.
//   test_iqn.py   obs 4, [64, 64] -> 64, C 64, H (), A 2:      160 + 4,160 + 2,080 + 2,080 + 2,080 + 2,080 + 1,056 + 4,160 + 128
//                                                              = 17,984 floats = 72,192 B
//   LunarLander   obs 8, [128, 128] -> 128, C 64, H (), A 4:   288 + 8,256 + 4,128 + 2,080 + 4,128 + 4,128 + 1,056 + 4,160 + 128
//                                                              = 28,352 floats = 113,664 B
//   (refused)     obs 8, [256, 256] -> 256, C 64, H (256,):    6 x 8,224 floats alone = 197,376 B > 163,840 B
int make_net(const int64_t* d, const char* who, INet* out) {
    TS_REQUIRE(d != nullptr, TS_ERR_INVALID_ARG, "%s: NULL network description", who);
    INet n{};
    const int64_t obs_dim = d[0], n_act = d[1], nt = d[2], fl = d[7], n_cos = d[8], nh = d[9];
    TS_REQUIRE(obs_dim >= 1 && obs_dim <= 256, TS_ERR_UNSUPPORTED, "%s: obs_dim %lld outside [1, 256]", who, (long long)obs_dim);
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_UNSUPPORTED, "%s: %lld actions outside [1, 32]", who, (long long)n_act);
    TS_REQUIRE(nt >= 1 && nt <= MAX_TRUNK, TS_ERR_UNSUPPORTED, "%s: %lld trunk hidden layers outside [1, 4]", who, (long long)nt);
    TS_REQUIRE(nh >= 0 && nh <= MAX_LAST, TS_ERR_UNSUPPORTED, "%s: %lld hidden layers in `last` outside [0, 2]", who, (long long)nh);
    TS_REQUIRE(n_cos >= 1 && n_cos <= MAX_COS, TS_ERR_UNSUPPORTED, "%s: num_cosines %lld outside [1, 64]", who, (long long)n_cos);
    auto width_ok = [](int64_t w) { return w >= 32 && w <= 256 && w % 32 == 0; };
    TS_REQUIRE(fl == 0 || width_ok(fl), TS_ERR_UNSUPPORTED, "%s: feature width %lld is no multiple of 32 in [32, 256]", who, (long long)fl);
    n.obs_dim = (int)obs_dim; n.n_act = (int)n_act; n.nt = (int)nt; n.nh = (int)nh; n.n_cos = (int)n_cos; n.feat_lin = fl != 0;
    int off = 0, at = 0;
    auto add = [&](Lay* l, int K, int N) { l->K = K; l->N = N; l->off = off; off += (K + 1) * N; };
    auto carve = [&](int floats) { const int o = at; at += floats; return o; };
    n.x_at = carve(TILE * (n.obs_dim + 1));
    int k = n.obs_dim;
    for (int i = 0; i < n.nt; ++i) {
        const int64_t w = d[3 + i];
        TS_REQUIRE(width_ok(w), TS_ERR_UNSUPPORTED, "%s: hidden width %lld is no multiple of 32 in [32, 256]", who, (long long)w);
        add(&n.t[i], k, (int)w);
        n.t_at[i] = carve(TILE * (n.t[i].N + 1));
        k = n.t[i].N;
    }
    if (n.feat_lin) {
        add(&n.fo, k, (int)fl);
        n.f_at = carve(TILE * ((int)fl + 1));
        k = (int)fl;
    }
    n.F = k;
    add(&n.emb, n.n_cos, n.F);
    n.pc = n.n_cos | 1;
    n.cs_at = carve(TILE * n.pc);
    n.phi_at = carve(TILE * (n.F + 1));
    for (int i = 0; i < n.nh; ++i) {
        const int64_t w = d[10 + i];
        TS_REQUIRE(width_ok(w), TS_ERR_UNSUPPORTED, "%s: hidden width %lld is no multiple of 32 in [32, 256]", who, (long long)w);
        add(&n.h[i], k, (int)w);
        n.h_at[i] = carve(TILE * (n.h[i].N + 1));
        k = n.h[i].N;
    }
    add(&n.head, k, n.n_act);
    n.df_at = carve(TILE * (n.F + 1));
    n.ob_at = carve(TILE * OP);
    n.th_at = carve(TILE * TP);
    n.tg_at = carve(TILE * TP);
    n.row_at = carve(4 * TILE);
    n.P = off;
    n.lds_floats = at;
    TS_REQUIRE((size_t)at * 4 + 256 <= (size_t)LDS_LIMIT, TS_ERR_UNSUPPORTED,
               "%s: the activations and sample tables of one 32-row tile need %zu bytes of LDS, the workgroup limit is %d", who,
               (size_t)at * 4 + 256, LDS_LIMIT);
    *out = n;
    return TS_OK;
}

int check_samples(int64_t N, const char* what, const char* who) {
    TS_REQUIRE(N >= 2 && N <= MAX_SAMPLES, TS_ERR_UNSUPPORTED, "%s: %s = %lld outside [2, 64]", who, what, (long long)N);
    return TS_OK;
}

inline size_t iqnm_ws_bytes(const INet& n, int64_t B) { return ((size_t)tiles_of(B) * n.P + (size_t)tiles_of(B) + (size_t)n.P) * 4 + 4096 + 1024; }

template <typename Kern>
int allow_lds(ts::DynLds& slot, Kern kern, const INet& n) {
    return slot.allow(reinterpret_cast<const void*>(kern), (size_t)n.lds_floats * 4);
}

}  // namespace

extern "C" {

int ts_iqn_mlp_layout(const int64_t* desc, int64_t B, int64_t* h_out) {
    TS_REQUIRE(h_out != nullptr, TS_ERR_INVALID_ARG, "ts_iqn_mlp_layout: NULL output");
    INet n;
    if (int rc = make_net(desc, "ts_iqn_mlp_layout", &n)) return rc;
    if (int rc = check_batch(B, "ts_iqn_mlp_layout")) return rc;
    h_out[0] = n.P;
    h_out[1] = (int64_t)n.lds_floats * 4 + 256;
    h_out[2] = (int64_t)iqnm_ws_bytes(n, B);
    for (int i = 0; i < MAX_TRUNK; ++i) h_out[3 + i] = i < n.nt ? n.t[i].off : -1;
    h_out[7] = n.feat_lin ? n.fo.off : -1;
    h_out[8] = n.emb.off;
    for (int i = 0; i < MAX_LAST; ++i) h_out[9 + i] = i < n.nh ? n.h[i].off : -1;
    h_out[11] = n.head.off;
    h_out[12] = n.F;
    return TS_OK;
}

int ts_iqn_mlp_forward(const float* params, const int64_t* desc, const float* obs, int64_t B, const float* tau, int64_t N,
                       float* logits_out, float* q_out, int64_t* act_out, ts_stream_t stream) {
    INet n;
    if (int rc = make_net(desc, "ts_iqn_mlp_forward", &n)) return rc;
    if (int rc = check_batch(B, "ts_iqn_mlp_forward")) return rc;
    if (int rc = check_samples(N, "sample_size", "ts_iqn_mlp_forward")) return rc;
    TS_REQUIRE(params && obs && tau && (logits_out || q_out || act_out), TS_ERR_INVALID_ARG, "ts_iqn_mlp_forward: NULL argument");
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, iqnm_walk_kernel<true>, n)) return rc;
    WalkArgs a{n, params, nullptr, obs, B, tau, (int)N, nullptr, 0, logits_out, q_out, act_out, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(iqnm_walk_kernel<true>, dim3((unsigned)tiles_of(B)), dim3(THREADS), (size_t)n.lds_floats * 4, ts::as_stream(stream), a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_iqn_mlp_next_dist(const float* params, const float* params_old, const int64_t* desc, const float* obs_next, int64_t B,
                         const float* tau_online, int64_t N, const float* tau_target, int64_t N2, const float* nstep_mask,
                         const double* nstep_gpow, const double* nstep_mc, float* out, ts_stream_t stream) {
    INet n;
    if (int rc = make_net(desc, "ts_iqn_mlp_next_dist", &n)) return rc;
    if (int rc = check_batch(B, "ts_iqn_mlp_next_dist")) return rc;
    if (int rc = check_samples(N, "the online sample count", "ts_iqn_mlp_next_dist")) return rc;
    const bool two = params_old != nullptr && params_old != params;
    if (two) {
        if (int rc = check_samples(N2, "the target sample count", "ts_iqn_mlp_next_dist")) return rc;
    }
    TS_REQUIRE(params && obs_next && tau_online && out && (!two || tau_target), TS_ERR_INVALID_ARG, "ts_iqn_mlp_next_dist: NULL argument");
    TS_REQUIRE((nstep_mask != nullptr) == (nstep_gpow != nullptr) && (nstep_mask != nullptr) == (nstep_mc != nullptr), TS_ERR_INVALID_ARG,
               "ts_iqn_mlp_next_dist: the three n-step coefficient arrays come together or not at all");
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, iqnm_walk_kernel<false>, n)) return rc;
    // without a lagged network the second walk is the same network on the same fractions
    WalkArgs a{n, params, two ? params_old : nullptr, obs_next, B, tau_online, (int)N, two ? tau_target : tau_online, two ? (int)N2 : (int)N,
               nullptr, nullptr, nullptr, out, nstep_mask, nstep_gpow, nstep_mc};
    hipLaunchKernelGGL(iqnm_walk_kernel<false>, dim3((unsigned)tiles_of(B)), dim3(THREADS), (size_t)n.lds_floats * 4, ts::as_stream(stream), a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_iqn_mlp_update(ts_workspace* ws, float* params, float* params_old, int sync_old, float* adam_m, float* adam_v, int64_t adam_step,
                      const int64_t* desc, const float* obs, const int64_t* act, const float* tau, int64_t N, const float* returns,
                      int64_t N2, const float* weight, int64_t B, const ts_distq_hparams* hp, float* loss_out, float* prio_out,
                      float* grad_out, ts_stream_t stream) {
    INet n;
    if (int rc = make_net(desc, "ts_iqn_mlp_update", &n)) return rc;
    if (int rc = check_batch(B, "ts_iqn_mlp_update")) return rc;
    if (int rc = check_samples(N, "the online sample count", "ts_iqn_mlp_update")) return rc;
    if (int rc = check_samples(N2, "the target sample count", "ts_iqn_mlp_update")) return rc;
    TS_REQUIRE(params && adam_m && adam_v && obs && act && tau && returns && hp && loss_out && prio_out, TS_ERR_INVALID_ARG,
               "ts_iqn_mlp_update: NULL argument");
    TS_REQUIRE(adam_step >= 1, TS_ERR_INVALID_ARG, "ts_iqn_mlp_update: adam_step is 1-based");
    TS_REQUIRE(!sync_old || params_old, TS_ERR_INVALID_ARG, "ts_iqn_mlp_update: sync_old without a lagged network");
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_iqn_mlp_update: workspace is NULL");
    if (int rc = ts::ws_reserve(ws, iqnm_ws_bytes(n, B))) return rc;
    hipStream_t s = ts::as_stream(stream);
    const int tiles = (int)tiles_of(B);
    float* slabs = static_cast<float*>(ws->base);
    float* partials = slabs + (size_t)tiles * n.P;
    float* grad_ws = partials + ((tiles + 63) / 64) * 64;
    float* norm_part = grad_ws + ((n.P + 63) / 64) * 64;            // 1024 floats behind it (iqnm_ws_bytes' tail)
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, iqnm_step_kernel, n)) return rc;
    StepArgs sa{n, params, obs, act, tau, (int)N, returns, (int)N2, weight, B, prio_out, slabs, partials};
    hipLaunchKernelGGL(iqnm_step_kernel, dim3((unsigned)tiles), dim3(THREADS), (size_t)n.lds_floats * 4, s, sa);
    TS_LAUNCH_CHECK();
    const bool step = hp->lr >= 0.0, clip = step && hp->max_grad_norm > 0.0;
    ApplyArgs aa{};
    aa.p = params; aa.m = adam_m; aa.v = adam_v; aa.p_old = sync_old ? params_old : nullptr;
    aa.slabs = slabs; aa.partials = partials; aa.tiles = tiles; aa.P = n.P;
    aa.grad_out = grad_out ? grad_out : (clip ? grad_ws : nullptr);
    aa.loss_out = loss_out;
    aa.adam = step && !clip;               // clip_grad_norm_ needs the whole gradient first: the sum here, then ts_adam_step's kernels
    float sc[2];
    ts::adam_step_scalars(adam_step, hp->lr, hp->beta1, hp->beta2, sc);
    aa.lr_step = sc[0]; aa.bc2_sqrt = sc[1];
    aa.beta2 = (float)hp->beta2; aa.eps = (float)hp->adam_eps;
    aa.omb1 = (float)(1.0 - hp->beta1); aa.omb2 = (float)(1.0 - hp->beta2);
    hipLaunchKernelGGL(dqnm_apply_kernel, dim3((unsigned)ts::ceil_div(n.P, THREADS)), dim3(THREADS), 0, s, aa);
    TS_LAUNCH_CHECK();
    if (!clip) return TS_OK;
    return ts::optim_step(s, ts::OptimDesc{}, params, adam_m, adam_v, aa.grad_out, n.P, adam_step, hp->lr, hp->beta1, hp->beta2,
                          hp->adam_eps, hp->max_grad_norm, norm_part);
}

}  // extern "C"
