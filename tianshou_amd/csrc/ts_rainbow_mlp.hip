// ts_rainbow_mlp.hip -- Rainbow on vector observations: `Net(softmax=True, num_atoms=N, dueling_param=(Q, V))` whose streams are
// NoisyLinear (utils/net/discrete.py:317-374) or plain Linear layers (utils/net/common.py:286-369), under RainbowDQN._update_with_batch
// (modelfree/rainbow.py:93-101 -> c51.py:123-160) as two launches per update: step, apply.
//
// The frame is ts_c51_mlp.hip's: one four-wave workgroup per 32 batch rows, activations resident in odd-pitch LDS, weights streamed
// from L2 into v_mfma_f32_32x32x2_f32 operands, the head walked action by action with loads masked past column N, one gradient slab
// and one loss partial per tile, dqnm_apply_kernel as the last launch.  New here, inside rbm_kernel<MODE, NZ>:
//   * the noisy operand is composed in registers: the lane that loads mu[k][c] loads sigma[k][c] and forms mu + sigma * (eps_q[c] *
//     eps_p[k]) in that order (contraction is off: the reference's float32 weight, bit for bit), the bias is mu_b + sigma_b * eps_q.
//     eps_p of the four stream layers is staged in LDS once per network pass, eps_q[c] is one register per lane per column block;
//     nothing composed is written to memory.  NZ false (eval mode, or plain Linear streams): mu alone is read;
//   * each of Q and V has 0 or 1 hidden layer (a dense_relu on the composed operand, its activation in LDS) and an output layer;
//   * dueling over atoms in two walks of the Q head: walk 1 keeps sum_a Q_a in registers (a lane owns its 16 entries of a column block
//     over all actions, in action order) and leaves sum / A in the table `mean`, V's N columns land in the table `vt`; walk 2 computes
//     Q_a again and forms (Q_a - mean) + V, then C51's softmax_row, the strictly-greater argmax and the kept row.  Four tables
//     [32][N | 1]: current, kept, mean (clamp(returns) while the projection runs: mean is dead by then), V;
//   * target phase and cross-entropy: c51m_kernel's, each network under its own noise;
//   * backward, with g = d loss / d logit of the taken action: dV = g, dQ_a = g ((sel == a) - 1/A).  Head weight gradient: one shared
//     block -(1/A) X^T g per 32 x 32 block, kept in registers, plus X^T (g masked by sel == a) for the actions present in the tile --
//     an absent action's columns carry the shared block.  Head input gradient: sum_a (g ((sel == a) - 1/A)) W_a^T on the composed
//     operand, all A N columns streamed once.  Every noisy accumulator is stored twice: mu <- acc, sigma <- acc * (eps_q[c] * eps_p[k]);
//     the bias row db and db * eps_q.  The trunk's top activation receives both streams' input gradients before its ReLU mask.
#pragma clang fp contract(off)
#include "ts_atom_head.h"

namespace {

enum { L_QH, L_VH, L_QO, L_VO };            // the stream layers: Q hidden, V hidden, Q output [K + 1, A N], V output [K + 1, N]

struct RNet {
    QNet q;                                  // trunk, the tables `current` / `kept`, per-row scalars; q.head = the Q output layer
    Lay qh, vh, vo;                          // N == 0: no hidden layer in that stream
    int noisy;                               // every stream layer is a mu block [K + 1, N] followed by a sigma block [K + 1, N]
    int qh_at, vh_at, tc_at, td_at;          // LDS: the stream activations, the tables `mean` and `vt`
    int ep_at[4], nz[4];                     // per stream layer: its staged eps_p in LDS; its eps_p[K] | eps_q[N] in the noise vector
    int n_noise;
};

// one stream layer as the kernel reads (parameters) or writes (slab) it
struct NL { const float* mu; const float* sg; const float* eq; const float* ep; int K, ld; };   // eq: memory, ep: LDS
struct SL { float* mu; float* sg; const float* eq; const float* ep; int K, ld; };

enum { RB_INFER, RB_TARGET, RB_STEP };

struct RbArgs {
    RNet net;
    const float* params; const float* noise;            // NZ: noise of the online network
    const float* params_old; const float* noise_old;    // params_old NULL: the online network is read for the target as well
    const float* support; float v_min, v_max, delta_z;
    const float* obs; const float* obs_next; const float* returns; const int64_t* act; const float* weight;
    int64_t B;
    float* dist_out; float* q_out; int64_t* act_out;      // INFER
    float* target_out;                                    // TARGET; STEP: optional
    float* prio_out; float* slabs; float* partials;       // STEP
};

__device__ __forceinline__ const Lay& lay_of(const RNet& rn, int w) { return w == L_QH ? rn.qh : w == L_VH ? rn.vh : w == L_QO ? rn.q.head : rn.vo; }

__device__ __forceinline__ NL view(const RNet& rn, int w, const float* p, const float* noise, const float* sm) {
    const Lay& l = lay_of(rn, w);
    return NL{p + l.off, p + l.off + (size_t)(l.K + 1) * l.N, noise + rn.nz[w] + l.K, sm + rn.ep_at[w], l.K, l.N};
}
__device__ __forceinline__ SL slab_view(const RNet& rn, int w, float* slab, const float* noise, const float* sm) {
    const Lay& l = lay_of(rn, w);
    return SL{slab + l.off, slab + l.off + (size_t)(l.K + 1) * l.N, noise + rn.nz[w] + l.K, sm + rn.ep_at[w], l.K, l.N};
}

// eps_p of every stream layer of one network -> LDS.  The caller's next barrier publishes it.
__device__ void stage_eps(const RNet& rn, const float* __restrict__ noise, float* sm) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const Lay& l = lay_of(rn, w);
        if (l.N == 0) continue;
        for (int k = threadIdx.x; k < l.K; k += THREADS) sm[rn.ep_at[w] + k] = noise[rn.nz[w] + k];
    }
}

// Y[32][N] = relu(X[32][K] W + b) on the composed operand (ts_mlp_tile.h's dense_relu otherwise; K is a hidden width: even)
template <bool NZ>
__device__ void stream_dense_relu(const NL& L, const float* X, int px, float* Y, int py) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int K = L.K, N = L.ld;
    for (int nb = wave; nb < N / 32; nb += 4) {
        const int n = nb * 32 + i;
        const float eqc = NZ ? L.eq[n] : 0.f;
        const float* mp = L.mu + n;
        const float* sp = L.sg + n;
        const float* xp = X + i * px + h;
        f32x16 acc = {};
#pragma unroll 8
        for (int k = 0; k < K; k += 2) {
            float w = mp[(size_t)(k + h) * N];
            if (NZ) w = w + sp[(size_t)(k + h) * N] * (eqc * L.ep[k + h]);
            acc = mfma32(xp[k], w, acc);
        }
        float bias = mp[(size_t)K * N];
        if (NZ) bias = bias + sp[(size_t)K * N] * eqc;
#pragma unroll
        for (int r = 0; r < 16; ++r) Y[featF(r, h) * py + n] = fmaxf(acc[r] + bias, 0.f);
    }
}

// one 32 x 32 block of a head: X[32][K] W[:, col] for this lane's column `col` (`live` false: a masked column, 0 is used) and its bias
template <bool NZ>
__device__ __forceinline__ f32x16 head_block(const NL& L, int col, bool live, const float* xp, float* bias) {
    const int h = (threadIdx.x & 63) >> 5, K = L.K, ld = L.ld;
    const float eqc = NZ ? L.eq[col] : 0.f;
    const float* mp = L.mu + col;
    const float* sp = L.sg + col;
    f32x16 acc = {};
#pragma unroll 8
    for (int k = 0; k < K; k += 2) {
        float w = mp[(size_t)(k + h) * ld];
        if (NZ) w = w + sp[(size_t)(k + h) * ld] * (eqc * L.ep[k + h]);
        acc = mfma32(xp[k], live ? w : 0.f, acc);
    }
    float b = mp[(size_t)K * ld];
    if (NZ) b = b + sp[(size_t)K * ld] * eqc;
    *bias = b;
    return acc;
}

// walk 1: mean[m][c] = (sum over the actions, in order, of Q_a[m][c]) / A
template <bool NZ>
__device__ void head_mean(const NL& L, int A, int N, int pt, const float* X, int px, float* mean) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const float* xp = X + i * px + h;
    for (int cb = wave; cb < (N + 31) / 32; cb += 4) {
        const int c = cb * 32 + i;
        const bool live = c < N;
        f32x16 sum = {};
        for (int a = 0; a < A; ++a) {
            float bias;
            const f32x16 acc = head_block<NZ>(L, a * N + (live ? c : 0), live, xp, &bias);
#pragma unroll
            for (int r = 0; r < 16; ++r) sum[r] = sum[r] + (acc[r] + bias);
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) mean[featF(r, h) * pt + c] = sum[r] / (float)A;
        }
    }
}

// the N columns from `col0` of a head -> out[m][c].  DUEL: (Q - mean[m][c]) + vt[m][c] (walk 2).  ROWSEL: only the rows with sel[m] == a.
template <bool NZ, bool DUEL, bool ROWSEL>
__device__ void head_cols(const NL& L, int col0, int N, int pt, const float* X, int px, float* out, const float* mean, const float* vt,
                          const int* sel, int a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const float* xp = X + i * px + h;
    for (int cb = wave; cb < (N + 31) / 32; cb += 4) {
        const int c = cb * 32 + i;
        const bool live = c < N;
        float bias;
        const f32x16 acc = head_block<NZ>(L, col0 + (live ? c : 0), live, xp, &bias);
        if (live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = featF(r, h);
                if (ROWSEL && sel[m] != a) continue;
                const float q = acc[r] + bias;
                out[m * pt + c] = DUEL ? (q - mean[m * pt + c]) + vt[m * pt + c] : q;
            }
        }
    }
}

struct Fwd { const float* xq; int pxq; const float* xv; int pxv; NL qo, vo; };     // the heads' inputs (LDS) and operands

// One network on the tile whose observations are in LDS: trunk, stream hidden layers, walk 1 -> `mean`, V -> `vt`.  Every earlier
// reader of the staged eps_p, of `mean` and of `vt` is behind a barrier when this is called.  Ends behind a barrier.
template <bool NZ>
__device__ Fwd net_forward(const RNet& rn, const float* __restrict__ p, const float* __restrict__ noise, float* sm) {
    if (NZ) stage_eps(rn, noise, sm);
    int ptop;
    const float* top = trunk_forward(rn.q, p, sm, &ptop);                      // (its barriers publish eps_p)
    Fwd f{top, ptop, top, ptop, view(rn, L_QO, p, noise, sm), view(rn, L_VO, p, noise, sm)};
    if (rn.qh.N) {
        f.xq = sm + rn.qh_at; f.pxq = rn.qh.N + 1;
        stream_dense_relu<NZ>(view(rn, L_QH, p, noise, sm), top, ptop, sm + rn.qh_at, f.pxq);
    }
    if (rn.vh.N) {
        f.xv = sm + rn.vh_at; f.pxv = rn.vh.N + 1;
        stream_dense_relu<NZ>(view(rn, L_VH, p, noise, sm), top, ptop, sm + rn.vh_at, f.pxv);
    }
    if (rn.qh.N || rn.vh.N) __syncthreads();
    const int N = rn.q.n_atoms, pt = rn.q.pitch;
    head_mean<NZ>(f.qo, rn.q.n_act, N, pt, f.xq, f.pxq, sm + rn.tc_at);
    head_cols<NZ, false, false>(f.vo, 0, N, pt, f.xv, f.pxv, sm + rn.td_at, nullptr, nullptr, nullptr, 0);
    __syncthreads();
    return f;
}

// Walk 2 over every action: softmax of the dueling logits, the running argmax of the expected value -> returned (thread (row, t): its
// row's).  KEEP: the argmax's normalised row is left in `kept`.  INFER: probabilities and expected values go to memory.  Ends behind a barrier.
template <bool NZ, bool KEEP, bool INFER>
__device__ int head_select(const RNet& rn, const Fwd& f, float* sm, const RbArgs& a, int64_t b) {
    const int N = rn.q.n_atoms, A = rn.q.n_act, pt = rn.q.pitch, row = threadIdx.x >> 3, t = threadIdx.x & 7;
    float* cur = sm + rn.q.ta_at;
    float* kept = sm + rn.q.tb_at;
    float best = 0.f;
    int arg = 0;
    for (int act = 0; act < A; ++act) {
        head_cols<NZ, true, false>(f.qo, act * N, N, pt, f.xq, f.pxq, cur, sm + rn.tc_at, sm + rn.td_at, nullptr, act);
        __syncthreads();
        float* mine = cur + row * pt;
        const float q = softmax_row(mine, N, t, a.support);
        const bool take = act == 0 || q > best;                                // strictly greater: the first index wins ties
        if (take) { best = q; arg = act; }
        if (INFER && b < a.B) {
            if (a.dist_out) for (int j = t; j < N; j += RPT) a.dist_out[(b * A + act) * N + j] = mine[j];
            if (a.q_out && t == 0) a.q_out[b * A + act] = q;
        }
        if (KEEP && take)
            for (int j = t; j < N; j += RPT) kept[row * pt + j] = mine[j];
        __syncthreads();                                                       // the next action overwrites `cur`
    }
    return arg;
}

// walk 2 over the actions some row selected: only the rows with sel[m] == a are stored -> `kept` (disjoint rows: no barrier between actions)
template <bool NZ>
__device__ void head_taken(const RNet& rn, const Fwd& f, float* sm, const int* sel, unsigned present) {
    const int N = rn.q.n_atoms, pt = rn.q.pitch;
    for (int act = 0; act < rn.q.n_act; ++act)
        if ((present >> act) & 1)                                              // workgroup-uniform
            head_cols<NZ, true, true>(f.qo, act * N, N, pt, f.xq, f.pxq, sm + rn.q.tb_at, sm + rn.tc_at, sm + rn.td_at, sel, act);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------

template <bool NZ>
__device__ __forceinline__ void store2(const SL& S, size_t idx, int k, float eqc, float v) {
    S.mu[idx] = v;
    if (NZ) S.sg[idx] = v * (eqc * S.ep[k]);
}

// slab of a layer [K + 1, N] whose output gradient is dZ[32][N] (V output layer: N = atoms, masked past N; stream hidden layers)
template <bool NZ>
__device__ void stream_wgrad(const SL& S, const float* X, int px, const float* dZ, int pz) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int K = S.K, N = S.ld, cbs = (N + 31) / 32, kbs = K / 32;
    for (int blk = wave; blk < kbs * cbs; blk += 4) {
        const int kb = blk / cbs, cb = blk - kb * cbs;
        const int kc = kb * 32 + i, c = cb * 32 + i;
        const bool live = c < N;
        const float* zp = dZ + (live ? c : 0);
        f32x16 acc = {};
#pragma unroll
        for (int m = 0; m < TILE; m += 2) acc = mfma32(X[(m + h) * px + kc], live ? zp[(m + h) * pz] : 0.f, acc);
        if (live) {
            const float eqc = NZ ? S.eq[c] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = kb * 32 + featF(r, h);
                store2<NZ>(S, (size_t)k * N + c, k, eqc, acc[r]);
            }
        }
    }
    for (int c = threadIdx.x; c < N; c += THREADS) {
        float s = 0.f;
        for (int m = 0; m < TILE; ++m) s += dZ[m * pz + c];
        S.mu[(size_t)K * N + c] = s;
        if (NZ) S.sg[(size_t)K * N + c] = s * S.eq[c];
    }
}

// slab of the Q output layer: per 32 x 32 block the shared part -(1/A) X^T g once, then per action the shared part plus, where the
// action is present in the tile, X^T (g masked by sel == a)
template <bool NZ>
__device__ void qhead_wgrad(const SL& S, int A, int N, const float* X, int px, const float* g, int pt, const int* sel, unsigned present) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int K = S.K, ld = S.ld, cbs = (N + 31) / 32, kbs = K / 32;
    const float nia = -(1.f / (float)A);
    for (int blk = wave; blk < kbs * cbs; blk += 4) {
        const int kb = blk / cbs, cb = blk - kb * cbs;
        const int kc = kb * 32 + i, c = cb * 32 + i;
        const bool live = c < N;
        const float* zp = g + (live ? c : 0);
        f32x16 sh = {};
#pragma unroll
        for (int m = 0; m < TILE; m += 2) sh = mfma32(X[(m + h) * px + kc], live ? zp[(m + h) * pt] : 0.f, sh);
#pragma unroll
        for (int r = 0; r < 16; ++r) sh[r] = sh[r] * nia;
        for (int a = 0; a < A; ++a) {
            f32x16 v = sh;
            if ((present >> a) & 1) {                                          // workgroup-uniform
                f32x16 acc = {};
#pragma unroll
                for (int m = 0; m < TILE; m += 2) acc = mfma32(X[(m + h) * px + kc], live && sel[m + h] == a ? zp[(m + h) * pt] : 0.f, acc);
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = acc[r] + sh[r];
            }
            if (live) {
                const float eqc = NZ ? S.eq[a * N + c] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int k = kb * 32 + featF(r, h);
                    store2<NZ>(S, (size_t)k * ld + a * N + c, k, eqc, v[r]);
                }
            }
        }
    }
    for (int c = threadIdx.x; c < N; c += THREADS) {
        float all = 0.f;
        for (int m = 0; m < TILE; ++m) all += g[m * pt + c];
        all = all * nia;
        for (int a = 0; a < A; ++a) {
            float v = all;
            if ((present >> a) & 1) {
                float s = 0.f;
                for (int m = 0; m < TILE; ++m) s += sel[m] == a ? g[m * pt + c] : 0.f;
                v = s + all;
            }
            S.mu[(size_t)K * ld + a * N + c] = v;
            if (NZ) S.sg[(size_t)K * ld + a * N + c] = v * S.eq[a * N + c];
        }
    }
}

// a source of an input gradient: dz[32][ncol] (LDS) against the composed W[Kt][nact ncol]; sel != NULL: the Q head, whose action a
// sees dz ((sel == a) - inv_a)
struct GSrc { const float* dz; int pz; NL w; int ncol, nact; const int* sel; float inv_a; };

// H[32][Kt] <- (sum over the sources and their actions of (dz coef) W[:, a ncol .. a ncol + ncol)^T) * (H > 0), in place.  Block k on
// wave k mod 4; A(i, c) = dz[i][c] coef from LDS, B(c, i) = W[k0 + i][a ncol + c] along c (4-byte loads: no alignment is needed)
template <bool NZ>
__device__ void stream_dgrad(float* H, int ph, int Kt, const GSrc& s0, const GSrc& s1) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    for (int kb = wave; kb < Kt / 32; kb += 4) {
        const int kc = kb * 32 + i;
        f32x16 acc = {};
        for (int s = 0; s < 2; ++s) {
            const GSrc& gs = s ? s1 : s0;
            if (!gs.dz) continue;                                              // workgroup-uniform
            const int ncol = gs.ncol;
            const float* mrow = gs.w.mu + (size_t)kc * gs.w.ld;
            const float* srow = gs.w.sg + (size_t)kc * gs.w.ld;
            const float* eq = gs.w.eq;
            const float epk = NZ ? gs.w.ep[kc] : 0.f;
            const float* zp = gs.dz + i * gs.pz;
            const int mysel = gs.sel ? gs.sel[i] : 0;
            for (int a = 0; a < gs.nact; ++a) {
                const float coef = gs.sel ? (mysel == a ? 1.f : 0.f) - gs.inv_a : 1.f;
                const int base = a * ncol;
#pragma unroll 4
                for (int c = 0; c < ncol; c += 2) {
                    const bool in = c + h < ncol;                              // odd ncol: the last pair is half empty
                    const int cc = base + (in ? c + h : 0);
                    float w = mrow[cc];
                    if (NZ) w = w + srow[cc] * (eq[cc] * epk);
                    acc = mfma32(in ? zp[cc - base] * coef : 0.f, in ? w : 0.f, acc);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float* q = H + featF(r, h) * ph + kc;
            *q = *q > 0.f ? acc[r] : 0.f;
        }
    }
}

template <int MODE, bool NZ>
__global__ __launch_bounds__(THREADS) void rbm_kernel(RbArgs a) {
    extern __shared__ float sm[];
    const RNet& rn = stage_net(a.net);
    const QNet& net = rn.q;
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7;
    const int64_t b = row0 + row;
    const int N = net.n_atoms, A = net.n_act, pt = net.pitch;
    float* cur = sm + net.ta_at;                             // dueling logits / probabilities of one action; then the projected target m
    float* kept = sm + net.tb_at;                            // next_dist; then p and d loss / d logit of the taken action
    float* tsup = sm + rn.tc_at;                             // `mean` during a network pass; clamp(returns, v_min, v_max) for the projection
    float* term = sm + net.row_at;
    int* sel = reinterpret_cast<int*>(sm + net.row_at + TILE);
    unsigned* present = reinterpret_cast<unsigned*>(sm + net.row_at + 2 * TILE);
    if (MODE == RB_INFER) {
        load_obs(net, a.obs, row0, a.B, sm);
        const Fwd f = net_forward<NZ>(rn, a.params, a.noise, sm);
        const int arg = head_select<NZ, false, true>(rn, f, sm, a, b);
        if (a.act_out && t == 0 && b < a.B) a.act_out[b] = arg;
        return;
    }

    // ---- C51._target_dist on obs_next: next_dist -> `kept`, the projected distribution m -> `cur` ------------------------------------
    load_obs(net, a.obs_next, row0, a.B, sm);
    if (a.params_old) {                                                        // workgroup-uniform
        Fwd f = net_forward<NZ>(rn, a.params, a.noise, sm);
        const int arg = head_select<NZ, false, false>(rn, f, sm, a, b);
        if (t == 0) sel[row] = arg;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned m = 0u;
            for (int r = 0; r < TILE; ++r) m |= 1u << sel[r];
            *present = m;
        }
        f = net_forward<NZ>(rn, a.params_old, a.noise_old, sm);                // (its barriers publish `present`)
        head_taken<NZ>(rn, f, sm, sel, *present);
        __syncthreads();
        softmax_row(kept + row * pt, N, t, a.support);
    } else {
        const Fwd f = net_forward<NZ>(rn, a.params, a.noise, sm);
        head_select<NZ, true, false>(rn, f, sm, a, b);
    }
    __syncthreads();                                                           // `mean` is dead
    for (int idx = threadIdx.x; idx < TILE * pt; idx += THREADS) {
        const int r = idx / pt, j = idx - r * pt;
        tsup[idx] = row0 + r < a.B && j < N ? fminf(fmaxf(a.returns[(row0 + r) * N + j], a.v_min), a.v_max) : 0.f;
    }
    __syncthreads();
    {
        const float* nd = kept + row * pt;
        const float* ts_ = tsup + row * pt;
        for (int i = t; i < N; i += RPT) {
            const float z = a.support[i];
            float m = 0.f;
            for (int j = 0; j < N; ++j) m += fminf(fmaxf(1.f - fabsf(ts_[j] - z) / a.delta_z, 0.f), 1.f) * nd[j];
            cur[row * pt + i] = m;
            if (a.target_out && b < a.B) a.target_out[b * N + i] = m;
        }
    }
    if (MODE == RB_TARGET) return;
    __syncthreads();                                                           // `kept`, sel and clamp(returns) are dead

    // ---- forward on obs, cross-entropy against m, backward, the tile's slab ------------------------------------------------------------
    const float* p = a.params;
    float* slab = a.slabs + (size_t)blockIdx.x * net.P;
    if (threadIdx.x < TILE) {                                // rows beyond B select nothing: exactly zero in the loss and in every slab
        const int64_t br = row0 + threadIdx.x;
        int s = -1;
        if (br < a.B) {
            const int64_t ab = a.act[br];
            s = ab < 0 ? 0 : ab >= A ? A - 1 : (int)ab;
        }
        sel[threadIdx.x] = s;
    }
    for (int idx = threadIdx.x; idx < TILE * pt; idx += THREADS) kept[idx] = 0.f;
    load_obs(net, a.obs, row0, a.B, sm);
    if (threadIdx.x == 0) {
        unsigned m = 0u;
        for (int r = 0; r < TILE; ++r) if (sel[r] >= 0) m |= 1u << sel[r];
        *present = m;
    }
    const Fwd f = net_forward<NZ>(rn, p, a.noise, sm);                         // (its barriers publish `present`)
    const unsigned pres = *present;
    head_taken<NZ>(rn, f, sm, sel, pres);
    __syncthreads();
    {
        const bool live = b < a.B;
        const float wb = live ? (a.weight ? a.weight[b] : 1.f) : 0.f;
        const float scale = wb / (float)a.B;
        float* mine = kept + row * pt;
        const float* mrow = cur + row * pt;
        softmax_row(mine, N, t, a.support);
        float ce = 0.f, pg = 0.f;
        for (int i = t; i < N; i += RPT) {
            const float pi = mine[i], m = mrow[i];
            ce += -(m * logf(pi + 1e-8f));
            pg += pi * (-(m / (pi + 1e-8f)) * scale);
        }
        ce = row_sum8(ce);
        pg = row_sum8(pg);
        for (int i = t; i < N; i += RPT) {
            const float pi = mine[i];
            const float g = -(mrow[i] / (pi + 1e-8f)) * scale;
            mine[i] = live ? pi * (g - pg) : 0.f;            // only this thread reads atom i
        }
        if (t == 0) {
            if (live) a.prio_out[b] = ce;
            term[row] = live ? ce * wb / (float)a.B : 0.f;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int m = 0; m < TILE; ++m) s += term[m];
        a.partials[blockIdx.x] = s;
    }
    float* top = sm + net.t_at[net.nt - 1];
    const int ptop = net.t[net.nt - 1].N + 1, ktop = net.t[net.nt - 1].N;
    qhead_wgrad<NZ>(slab_view(rn, L_QO, slab, a.noise, sm), A, N, f.xq, f.pxq, kept, pt, sel, pres);
    stream_wgrad<NZ>(slab_view(rn, L_VO, slab, a.noise, sm), f.xv, f.pxv, kept, pt);
    __syncthreads();
    GSrc tq{kept, pt, f.qo, N, A, sel, 1.f / (float)A}, tv{kept, pt, f.vo, N, 1, nullptr, 0.f};     // what `top` receives from each stream
    const GSrc none{};
    if (rn.qh.N) {
        stream_dgrad<NZ>(sm + rn.qh_at, rn.qh.N + 1, rn.qh.N, tq, none);
        tq = GSrc{sm + rn.qh_at, rn.qh.N + 1, view(rn, L_QH, p, a.noise, sm), rn.qh.N, 1, nullptr, 0.f};
    }
    if (rn.vh.N) {
        stream_dgrad<NZ>(sm + rn.vh_at, rn.vh.N + 1, rn.vh.N, tv, none);
        tv = GSrc{sm + rn.vh_at, rn.vh.N + 1, view(rn, L_VH, p, a.noise, sm), rn.vh.N, 1, nullptr, 0.f};
    }
    if (rn.qh.N || rn.vh.N) {
        __syncthreads();
        if (rn.qh.N) stream_wgrad<NZ>(slab_view(rn, L_QH, slab, a.noise, sm), top, ptop, sm + rn.qh_at, rn.qh.N + 1);
        if (rn.vh.N) stream_wgrad<NZ>(slab_view(rn, L_VH, slab, a.noise, sm), top, ptop, sm + rn.vh_at, rn.vh.N + 1);
        __syncthreads();
    }
    stream_dgrad<NZ>(top, ptop, ktop, tq, tv);               // both streams' input gradients, then the ReLU mask
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

// desc (host, TS_RAINBOW_MLP_DESC_LEN int64): {obs_dim, A, 1, trunk layers, Q hidden layers (0 | 1), V hidden layers (0 | 1), trunk
// widths[4], Q width, 0, V width, 0, N, noisy}: the DQN-MLP route's 14 entries, the atoms, the noisy flag.  LDS carve of one tile, in
// floats: obs 32 (obs_dim + 1) + sum over the trunk and stream hidden layers of 32 (width + 1) + 4 x 32 (N | 1) (the four tables) +
// 4 x 32 (per-row scalars) + the staged eps_p (the sum of the stream layers' input widths, when noisy), and 256 bytes for the staged
// description.  Checked:
//   test_rainbow.py  obs 4, [128] x 4, no stream hidden layer, A = 2, N = 51, noisy:
//                    160 + 4 x 4,128 + 4 x 1,632 + 128 + 2 x 128 = 23,584 floats = 94,336 B
//   (refused) [256] x 4, Q and V hidden 256, N = 256, noisy:
//                    160 + 6 x 8,224 + 4 x 8,224 + 128 + 4 x 256 = 83,552 floats = 334,208 B > 163,840 B
int make_net(const int64_t* d, const char* who, RNet* out) {
    TS_REQUIRE(d != nullptr, TS_ERR_INVALID_ARG, "%s: NULL network description", who);
    RNet rn{};
    QNet& n = rn.q;
    const int64_t obs_dim = d[0], n_act = d[1], nt = d[3], n_atoms = d[14];
    TS_REQUIRE(obs_dim >= 1 && obs_dim <= 256, TS_ERR_UNSUPPORTED, "%s: obs_dim %lld outside [1, 256]", who, (long long)obs_dim);
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_UNSUPPORTED, "%s: %lld actions outside [1, 32]", who, (long long)n_act);
    TS_REQUIRE(n_atoms >= 2 && n_atoms <= MAX_ATOMS, TS_ERR_UNSUPPORTED, "%s: %lld atoms outside [2, 256]", who, (long long)n_atoms);
    TS_REQUIRE(nt >= 1 && nt <= MAX_TRUNK, TS_ERR_UNSUPPORTED, "%s: %lld trunk hidden layers outside [1, 4]", who, (long long)nt);
    TS_REQUIRE(d[2] == 1, TS_ERR_UNSUPPORTED, "%s: a dueling head is needed (C51 on a plain Net is ts_c51_mlp's)", who);
    TS_REQUIRE(d[4] >= 0 && d[4] <= 1 && d[5] >= 0 && d[5] <= 1, TS_ERR_UNSUPPORTED, "%s: Q / V streams with %lld / %lld hidden layers (0 or 1)", who,
               (long long)d[4], (long long)d[5]);
    TS_REQUIRE(d[15] == 0 || d[15] == 1, TS_ERR_INVALID_ARG, "%s: the noisy flag is 0 or 1", who);
    n.obs_dim = (int)obs_dim; n.n_act = (int)n_act; n.n_atoms = (int)n_atoms; n.nt = (int)nt;
    rn.noisy = (int)d[15];
    int off = 0, at = 0, nz = 0;
    auto add = [&](Lay* l, int K, int N, int copies) { l->K = K; l->N = N; l->off = off; off += copies * (K + 1) * N; };
    auto carve = [&](int floats) { const int o = at; at += floats; return o; };
    auto width = [&](int64_t w) {
        TS_REQUIRE(w >= 32 && w <= 256 && w % 32 == 0, TS_ERR_UNSUPPORTED, "%s: hidden width %lld is no multiple of 32 in [32, 256]", who, (long long)w);
        return TS_OK;
    };
    n.x_at = carve(TILE * (n.obs_dim + 1));
    int k = n.obs_dim;
    for (int i = 0; i < n.nt; ++i) {
        if (int rc = width(d[6 + i])) return rc;
        add(&n.t[i], k, (int)d[6 + i], 1);
        n.t_at[i] = carve(TILE * (n.t[i].N + 1));
        k = n.t[i].N;
    }
    // flat order: the Q stream (hidden, output), then the V stream; the noise vector in the same order, eps_p[K] then eps_q[N] per layer
    const int copies = rn.noisy ? 2 : 1;
    auto stream = [&](int hidden, int64_t w, Lay* hid, int* hid_at, int wh, Lay* outl, int wo, int n_out) {
        int kin = k;
        if (hidden) {
            if (int rc = width(w)) return rc;
            add(hid, kin, (int)w, copies);
            *hid_at = carve(TILE * ((int)w + 1));
            rn.nz[wh] = nz; nz += kin + (int)w;
            kin = (int)w;
        }
        add(outl, kin, n_out, copies);
        rn.nz[wo] = nz; nz += kin + n_out;
        return TS_OK;
    };
    if (int rc = stream((int)d[4], d[10], &rn.qh, &rn.qh_at, L_QH, &n.head, L_QO, n.n_act * n.n_atoms)) return rc;
    if (int rc = stream((int)d[5], d[12], &rn.vh, &rn.vh_at, L_VH, &rn.vo, L_VO, n.n_atoms)) return rc;
    n.pitch = n.n_atoms | 1;
    n.ta_at = carve(TILE * n.pitch);
    n.tb_at = carve(TILE * n.pitch);
    rn.tc_at = carve(TILE * n.pitch);
    rn.td_at = carve(TILE * n.pitch);
    n.row_at = carve(4 * TILE);
    if (rn.noisy)
        for (int w = 0; w < 4; ++w) {
            const Lay& l = w == L_QH ? rn.qh : w == L_VH ? rn.vh : w == L_QO ? n.head : rn.vo;
            if (l.N) rn.ep_at[w] = carve(l.K);
        }
    n.P = off;
    n.lds_floats = at;
    rn.n_noise = rn.noisy ? nz : 0;
    TS_REQUIRE((size_t)at * 4 + 256 <= (size_t)LDS_LIMIT, TS_ERR_UNSUPPORTED,
               "%s: the activations, atom tables and staged noise of one 32-row tile need %zu bytes of LDS, the workgroup limit is %d", who,
               (size_t)at * 4 + 256, LDS_LIMIT);
    *out = rn;
    return TS_OK;
}

template <int MODE, bool NZ>
int launch_as(const RNet& rn, const RbArgs& a, hipStream_t s) {
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, rbm_kernel<MODE, NZ>, rn.q)) return rc;
    hipLaunchKernelGGL((rbm_kernel<MODE, NZ>), dim3((unsigned)tiles_of(a.B)), dim3(THREADS), (size_t)rn.q.lds_floats * 4, s, a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

template <int MODE>
int launch(const RNet& rn, const RbArgs& a, hipStream_t s) {
    return a.noise ? launch_as<MODE, true>(rn, a, s) : launch_as<MODE, false>(rn, a, s);
}

int check_support(float v_min, float v_max, float delta_z, const char* who) {
    TS_REQUIRE(v_min < v_max && delta_z > 0.f, TS_ERR_INVALID_ARG, "%s: v_min < v_max and delta_z > 0 are needed", who);
    return TS_OK;
}

// a training pass of a noisy network needs its noise; a plain network has none (the pointers are then not read)
int check_noise(const RNet& rn, const float* noise, const float* params_old, const float* noise_old, const char* who) {
    TS_REQUIRE(!rn.noisy || noise, TS_ERR_INVALID_ARG, "%s: NoisyLinear streams need the noise vector", who);
    TS_REQUIRE(!rn.noisy || !params_old || noise_old, TS_ERR_INVALID_ARG, "%s: the lagged network needs its own noise vector", who);
    return TS_OK;
}

}  // namespace

extern "C" {

int ts_rainbow_mlp_layout(const int64_t* desc, int64_t B, int64_t* h_out) {
    TS_REQUIRE(h_out != nullptr, TS_ERR_INVALID_ARG, "ts_rainbow_mlp_layout: NULL output");
    RNet rn;
    if (int rc = make_net(desc, "ts_rainbow_mlp_layout", &rn)) return rc;
    if (int rc = check_batch(B, "ts_rainbow_mlp_layout")) return rc;
    const QNet& n = rn.q;
    h_out[0] = n.P;
    h_out[1] = (int64_t)n.lds_floats * 4 + 256;
    h_out[2] = (int64_t)ws_bytes(n, B);
    for (int i = 0; i < MAX_TRUNK; ++i) h_out[3 + i] = i < n.nt ? n.t[i].off : -1;
    h_out[7] = rn.qh.N ? rn.qh.off : -1;
    h_out[8] = n.head.off;
    h_out[9] = rn.vh.N ? rn.vh.off : -1;
    h_out[10] = rn.vo.off;
    h_out[11] = rn.n_noise;
    return TS_OK;
}

int ts_rainbow_mlp_forward(const float* params, const float* noise, const int64_t* desc, const float* support, const float* obs, int64_t B,
                           float* dist_out, float* q_out, int64_t* act_out, ts_stream_t stream) {
    RNet rn;
    if (int rc = make_net(desc, "ts_rainbow_mlp_forward", &rn)) return rc;
    if (int rc = check_batch(B, "ts_rainbow_mlp_forward")) return rc;
    TS_REQUIRE(params && support && obs && (dist_out || q_out || act_out), TS_ERR_INVALID_ARG, "ts_rainbow_mlp_forward: NULL argument");
    RbArgs a{};
    a.net = rn; a.params = params; a.noise = rn.noisy ? noise : nullptr; a.support = support; a.obs = obs; a.B = B;
    a.dist_out = dist_out; a.q_out = q_out; a.act_out = act_out;
    return launch<RB_INFER>(rn, a, ts::as_stream(stream));
}

int ts_rainbow_mlp_target_dist(const float* params, const float* noise, const float* params_old, const float* noise_old, const int64_t* desc,
                               const float* support, float v_min, float v_max, float delta_z, const float* obs_next, const float* returns,
                               int64_t B, float* out, ts_stream_t stream) {
    RNet rn;
    if (int rc = make_net(desc, "ts_rainbow_mlp_target_dist", &rn)) return rc;
    if (int rc = check_batch(B, "ts_rainbow_mlp_target_dist")) return rc;
    TS_REQUIRE(params && support && obs_next && returns && out, TS_ERR_INVALID_ARG, "ts_rainbow_mlp_target_dist: NULL argument");
    if (int rc = check_support(v_min, v_max, delta_z, "ts_rainbow_mlp_target_dist")) return rc;
    RbArgs a{};
    a.net = rn; a.params = params; a.params_old = params_old == params ? nullptr : params_old;
    if (int rc = check_noise(rn, noise, a.params_old, noise_old, "ts_rainbow_mlp_target_dist")) return rc;
    a.noise = rn.noisy ? noise : nullptr; a.noise_old = rn.noisy ? noise_old : nullptr;
    a.support = support; a.v_min = v_min; a.v_max = v_max; a.delta_z = delta_z;
    a.obs_next = obs_next; a.returns = returns; a.B = B; a.target_out = out;
    return launch<RB_TARGET>(rn, a, ts::as_stream(stream));
}

int ts_rainbow_mlp_update(ts_workspace* ws, float* params, const float* noise, float* params_old, const float* noise_old, int sync_old,
                          float* adam_m, float* adam_v, int64_t adam_step, const int64_t* desc, const float* support, float v_min,
                          float v_max, float delta_z, const float* obs, const int64_t* act, const float* obs_next, const float* returns,
                          const float* weight, int64_t B, const ts_dqn_hparams* hp, float* loss_out, float* prio_out, float* grad_out,
                          float* target_out, ts_stream_t stream) {
    RNet rn;
    if (int rc = make_net(desc, "ts_rainbow_mlp_update", &rn)) return rc;
    if (int rc = check_batch(B, "ts_rainbow_mlp_update")) return rc;
    const QNet& n = rn.q;
    TS_REQUIRE(params && adam_m && adam_v && support && obs && act && obs_next && returns && hp && loss_out && prio_out, TS_ERR_INVALID_ARG,
               "ts_rainbow_mlp_update: NULL argument");
    if (int rc = check_support(v_min, v_max, delta_z, "ts_rainbow_mlp_update")) return rc;
    TS_REQUIRE(adam_step >= 1, TS_ERR_INVALID_ARG, "ts_rainbow_mlp_update: adam_step is 1-based");
    TS_REQUIRE(!sync_old || params_old, TS_ERR_INVALID_ARG, "ts_rainbow_mlp_update: sync_old without a lagged network");
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_rainbow_mlp_update: workspace is NULL");
    RbArgs a{};
    a.net = rn; a.params = params;
    // the sync comes before the target (c51.py:147-149): on a sync iteration the lagged network IS the online one, noise included
    a.params_old = sync_old || params_old == params ? nullptr : params_old;
    if (int rc = check_noise(rn, noise, a.params_old, noise_old, "ts_rainbow_mlp_update")) return rc;
    a.noise = rn.noisy ? noise : nullptr; a.noise_old = rn.noisy ? noise_old : nullptr;
    if (int rc = ts::ws_reserve(ws, ws_bytes(n, B))) return rc;
    hipStream_t s = ts::as_stream(stream);
    const int tiles = (int)tiles_of(B);
    const UpdateScratch u = update_scratch(ws->base, tiles, n.P);
    a.support = support; a.v_min = v_min; a.v_max = v_max; a.delta_z = delta_z;
    a.obs = obs; a.obs_next = obs_next; a.returns = returns; a.act = act; a.weight = weight; a.B = B;
    a.target_out = target_out; a.prio_out = prio_out; a.slabs = u.slabs; a.partials = u.partials;
    if (int rc = launch<RB_STEP>(rn, a, s)) return rc;
    return apply_tiles(s, u, tiles, n.P, params, sync_old ? params_old : nullptr, adam_m, adam_v, adam_step, hp, grad_out, loss_out);
}

}  // extern "C"
