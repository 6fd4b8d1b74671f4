// ts_iqn_walk.h -- THE SAMPLE WALK that ts_iqn_mlp.hip and ts_fqf_mlp.hip share, on the 32-row tile of ts_mlp_tile.h: the network
// description and its LDS carve, the trunk up to the features f[32][F], one sample forward (cosines -> phi -> f (.) phi -> `last` ->
// the final Linear as one masked 32-column block) and one sample backward (slab blocks read-modify-written per sample, df += dx (.)
// phi).  Moved here from ts_iqn_mlp.hip as it was, with two openings: `last` has up to MAX_LAST_H hidden layers (each file states
// its own limit to make_inet), and the fraction of sample j is read through a TauSrc, so that the table may lie in global memory
// (IQN: drawn fractions [B, N]) or in LDS (FQF: the fractions the tile proposed for itself).
// Include behind `#pragma clang fp contract(off)`.
#pragma once

#include "ts_atom_head.h"     // RPT, row_sum8, tiles_of, check_batch (and ts_mlp_tile.h)
#include "ts_qr_terms.h"

namespace {

constexpr int MAX_LAST_H = 3, MAX_COS = 64, MAX_SAMPLES = 64;
constexpr int TP = MAX_SAMPLES | 1;         // pitch of the per-row sample tables
constexpr int OP = TILE + 1;                // pitch of the head's output block

struct INet {
    int obs_dim, n_act, nt, nh, n_cos, feat_lin, F;
    Lay t[MAX_TRUNK], fo, emb, h[MAX_LAST_H], head;
    int x_at, t_at[MAX_TRUNK], f_at, cs_at, pc, phi_at, h_at[MAX_LAST_H], df_at, ob_at, th_at, tg_at, row_at;
    int P, lds_floats;
};

// where the fraction of (tile row i, sample j) is: p[(row0 + i) * pitch + j], rows with row0 + i >= rows read nothing and take 0
struct TauSrc { const float* p; int pitch; int64_t row0, rows; };

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

// a Linear onto A <= 32 columns: ob[32][A] = (X (.) X2) W + b as one 32-column block on wave 0, the weight loads masked past column A
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

// sample j up to the top of `last`'s hidden layers: cs, phi, h[0 .. nh - 1].  Ends behind a barrier.
__device__ void sample_hidden(const INet& net, const float* __restrict__ p, const float* fa, float* sm, TauSrc tau, int j) {
    float* cs = sm + net.cs_at;
    float* phi = sm + net.phi_at;
    const int C = net.n_cos, pc = net.pc, pf = net.F + 1;
    for (int e = threadIdx.x; e < TILE * C; e += THREADS) {                  // one cosine per (row, k)
        const int i = e / C, k = e - i * C;
        const float t = tau.row0 + i < tau.rows ? tau.p[(tau.row0 + i) * tau.pitch + j] : 0.f;
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
    for (int l = 1; l < net.nh; ++l) {
        dense_relu(p + net.h[l].off, net.h[l].K, net.h[l].N, sm + net.h_at[l - 1], net.h[l - 1].N + 1, sm + net.h_at[l], net.h[l].N + 1);
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

// Sample j backward, its hidden activations in LDS (sample_hidden) and d loss / d theta_j of the taken action in dth[m * TP + j]: the
// slab blocks of the final Linear, of `last` and of the embedding take the sample (`first`: written, else added), df takes dx (.) phi.
// Ends behind a barrier: the next sample may overwrite cs and phi.
__device__ void sample_backward(const INet& net, const float* __restrict__ p, const float* fa, float* sm, float* __restrict__ slab,
                                const float* dth, const int* sel, int j, bool first) {
    float* ob = sm + net.ob_at;
    float* phi = sm + net.phi_at;
    float* df = sm + net.df_at;
    const int A = net.n_act, F = net.F, pf = F + 1, nh = net.nh;
    for (int idx = threadIdx.x; idx < TILE * TILE; idx += THREADS) {
        const int m = idx >> 5, c = idx & 31;
        ob[m * OP + c] = c == sel[m] ? dth[m * TP + j] : 0.f;
    }
    __syncthreads();
    const HSrc hs{ob, OP, p + net.head.off, A};
    if (nh == 0) {
        wgrad_acc<true>(slab + net.head.off, first, fa, phi, pf, F, ob, OP, A);
        __syncthreads();
        dgrad_embed(phi, df, fa, pf, F, MSrc{}, hs);
    } else {
        float* top = sm + net.h_at[nh - 1];
        const int ptop = net.h[nh - 1].N + 1;
        wgrad_acc<false>(slab + net.head.off, first, top, top, ptop, net.head.K, ob, OP, A);
        __syncthreads();
        dgrad(top, ptop, net.head.K, MSrc{}, MSrc{}, hs, HSrc{});
        __syncthreads();
        for (int l = nh - 1; l >= 1; --l) {
            float* hi = sm + net.h_at[l];
            float* lo = sm + net.h_at[l - 1];
            const int pi = net.h[l].N + 1, pl = net.h[l - 1].N + 1;
            wgrad_acc<false>(slab + net.h[l].off, first, lo, lo, pl, net.h[l].K, hi, pi, net.h[l].N);
            __syncthreads();
            dgrad(lo, pl, net.h[l - 1].N, MSrc{hi, pi, p + net.h[l].off, net.h[l].N}, MSrc{}, HSrc{}, HSrc{});
            __syncthreads();
        }
        float* h0 = sm + net.h_at[0];
        const int p0 = net.h[0].N + 1;
        wgrad_acc<true>(slab + net.h[0].off, first, fa, phi, pf, F, h0, p0, net.h[0].N);
        __syncthreads();
        dgrad_embed(phi, df, fa, pf, F, MSrc{h0, p0, p + net.h[0].off, net.h[0].N}, HSrc{});
    }
    __syncthreads();
    wgrad_acc<false>(slab + net.emb.off, first, sm + net.cs_at, sm + net.cs_at, net.pc, net.n_cos, phi, pf, F);
    __syncthreads();
}

// the trunk backward on df (wgrad / dgrad of ts_mlp_tile.h): the slab blocks of the Net's output layer and of the trunk
__device__ void trunk_backward(const INet& net, const float* __restrict__ p, float* sm, float* __restrict__ slab) {
    float* df = sm + net.df_at;
    const int F = net.F, pf = F + 1;
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

// the quantile-Huber pair loss of row (tid >> 3) (ts_qr_terms.h): thread t takes theta_i, i = t (mod 8), against the row's N2 targets
// tg; tau_i = taus[toff + i], read on a live row only (b < B).  th[row][i] becomes d loss / d theta_i; -> the row's loss term on t == 0 (0 on a row beyond B); prio_out[b].
__device__ float pair_loss_row(float* th, const float* tg, const float* taus, int64_t toff, int N, int N2, const float* weight, int64_t b,
                               int64_t B, float* prio_out) {
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7;
    const bool live = b < B;
    const float wb = live ? (weight ? weight[b] : 1.f) : 0.f;
    const float scale = wb / ((float)B * (float)N);
    float wl = 0.f, sl = 0.f;
    if (live) {
        float* mine = th + row * TP;
        for (int i = t; i < N; i += RPT) {
            float li, ai, g;
            qr_terms(tg + row * TP, N2, mine[i], taus[toff + i], li, ai, g);
            mine[i] = -g * scale;                        // only this thread reads theta_i
            wl += li;
            sl += ai;
        }
    }
    wl = row_sum8(wl);
    sl = row_sum8(sl);
    const float huber = wl / (float)N;
    if (t == 0 && live) prio_out[b] = sl / (float)N;
    return live ? huber * wb / (float)B : 0.f;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------

// desc (host int64): {obs_dim, n_act, n_trunk, trunk[4], width of the Net's linear output layer (0: none, the features are the last
// ReLU layer), num_cosines, n_last, last_hidden[max_last]} -> the layers, the flat offsets and the LDS carve of one tile, in floats:
// obs 32 (obs_dim + 1) + trunk layers 32 (width + 1) + [features 32 (F + 1)] + cs 32 (C | 1) + phi 32 (F + 1) + `last` hidden layers
// 32 (width + 1) + df 32 (F + 1) + ob 32 x 33 + two sample tables 32 x 65 + 4 x 32 per-row scalars.  The caller adds what else it
// keeps in LDS and checks the total against LDS_LIMIT.
int make_inet(const int64_t* d, const char* who, int max_last, INet* out) {
    TS_REQUIRE(d != nullptr, TS_ERR_INVALID_ARG, "%s: NULL network description", who);
    INet n{};
    const int64_t obs_dim = d[0], n_act = d[1], nt = d[2], fl = d[7], n_cos = d[8], nh = d[9];
    TS_REQUIRE(obs_dim >= 1 && obs_dim <= 256, TS_ERR_UNSUPPORTED, "%s: obs_dim %lld outside [1, 256]", who, (long long)obs_dim);
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_UNSUPPORTED, "%s: %lld actions outside [1, 32]", who, (long long)n_act);
    TS_REQUIRE(nt >= 1 && nt <= MAX_TRUNK, TS_ERR_UNSUPPORTED, "%s: %lld trunk hidden layers outside [1, 4]", who, (long long)nt);
    TS_REQUIRE(nh >= 0 && nh <= max_last, TS_ERR_UNSUPPORTED, "%s: %lld hidden layers in `last` outside [0, %d]", who, (long long)nh, max_last);
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
    *out = n;
    return TS_OK;
}

int check_samples(int64_t N, const char* what, const char* who) {
    TS_REQUIRE(N >= 2 && N <= MAX_SAMPLES, TS_ERR_UNSUPPORTED, "%s: %s = %lld outside [2, 64]", who, what, (long long)N);
    return TS_OK;
}

}  // namespace
