// ts_fqf_mlp.hip -- FQF on vector observations: `FullQuantileFunction(preprocess_net=Net(...), hidden_sizes=H, num_cosines=C)` with a
// `FractionProposalNetwork(N, F)` (utils/net/discrete.py:219-314) under FQFPolicy.forward, FQF._target_q and FQF._update_with_batch
// (modelfree/fqf.py:66-106, 178-256); the setup of test/discrete/test_fqf.py.  A target pass is one launch, an update three (step,
// apply, the fraction optimizer's step; two more when the model's gradient is clipped).
//
// The tile and the sample walk are ts_iqn_mlp.hip's (ts_mlp_tile.h, ts_iqn_walk.h).  What is new here: the fractions are not drawn,
// the tile computes them from its own features, keeps them in LDS and walks over them twice.
//   PROPOSAL (discrete.py:239-252, on the detached features): z[32][N] = f Wp + bp as ceil(N / 32) masked 32-column MFMA blocks into
//     the table lp; per row, its eight threads on the columns i = t (mod 8): logp = z - max - log(sum exp(z - max)), p = exp(z - max)
//     / sum, the entropy H = -sum p logp (butterfly row sums); then one thread per row the serial ascending cumsum taus[0] = 0,
//     taus[j + 1] = taus[j] + p[j] and tau_hats[j] = (taus[j] + taus[j + 1]) / 2.  Tables per row, pitch 65: taus, tau_hats, p, logp.
//     Rows beyond B: all four tables and H are zeros.
//   WALK: ts_iqn_walk.h's, the fraction of sample j read from the LDS table (tau_hats: N samples; taus + 1: the N - 1 interior ones).
//   * INFER  (ts_fqf_mlp_forward): logits at tau_hats to [B, A, N], q[b][a] = sum_j (taus[j + 1] - taus[j]) logits[b][a][j], j
//     ascending in the registers of thread (row, t), the arg-max strictly greater; optionally the quantiles at taus[1:-1].  With the
//     fractions passed in, the tables are loaded instead of proposed.
//   * TARGET (ts_fqf_mlp_next_dist): the online network proposes, walks and selects; the evaluating network (the lagged one on its own
//     trunk, or the online one again: a bit-identical recompute that skips the trunk) walks over the SAME tau_hats, still in LDS, and
//     column sel[row] of every sample is kept; epilogue float(double(theta' mask) gamma^n + mc).
//   * STEP   (ts_fqf_mlp_update): forward walk over tau_hats -> th (theta-hat of the taken action), forward walk over the interior
//     taus -> qt (theta, no gradient); the fraction loss; the pair loss (ts_iqn_walk.h) with tau = tau_hats against the N targets; the
//     fraction network's slab f^T dz (+ bias row) as one masked wgrad block set; the backward walk over the N tau_hat samples; the
//     trunk backward.  The fraction loss of a row, i = 1 .. N - 1 (fqf.py:222-244):
//         g_i = +-(theta_i - theta-hat_{i-1}) +- (theta_i - theta-hat_i),  L = sum_i g_i taus_i,
//     and with taus_i = sum_{m < i} p_m (p indexed from 0) its derivative is dL / dp_k = S_k = sum_{i = k + 1}^{N - 1} g_i (a suffix
//     sum; S_{N-1} = 0), so through the softmax dL / dz_k = p_k (S_k - sum_m p_m S_m) = p_k (S_k - L) (sum_m p_m S_m = sum_i g_i taus_i);
//     the entropy gives d(-H) / dz_k = p_k (logp_k + H).  dz_k = (p_k (S_k - L) + ent_coef p_k (logp_k + H)) / B overwrites logp_k.
//     (S_k starts at i = k + 1, not at max(k, 1) as a 1-based reading of p would have it: p_k enters taus_i only for i > k.  Do not
//     "fix" it: tests/test_gpu_fqf_mlp.py compares this gradient with autograd's in tests/oracle_fqf_mlp.py.)
//     Rows beyond B: sel = -1, tables 0: exactly zero in the three losses and in every slab.
// One slab per tile holds the model's P floats and behind them the fraction network's P2; fqfm_apply_kernel sums slabs and the three
// loss partials (quantile, fraction, entropy) in tile order, so a repeated update is bit-identical.
// Flat vectors: the model's as ts_iqn_mlp.hip's; the fraction network's [F + 1, N], row F the bias.
#pragma clang fp contract(off)
#include <algorithm>

#include "ts_iqn_walk.h"

namespace {

constexpr int MAX_LAST = 3;                 // test_fqf.py: hidden_sizes = [64, 64, 64] in `last`
constexpr int STAGE_BYTES = 512;            // reserved for the staged description (FNet is larger than stage_net's 256)

struct FNet {
    INet n;
    Lay prop;                               // the fraction network in ITS flat vector: K = F, N = num_fractions, off = 0
    int N, P2;
    int taus_at, tauh_at, pr_at, lp_at, qt_at, ent_at;     // five [32][65] tables and the rows' entropies
    int lds_floats;
};

__device__ const FNet& stage_fnet(const FNet& arg) {
    __shared__ FNet staged;
    constexpr int WORDS = sizeof(FNet) / 4;
    static_assert(WORDS <= THREADS && sizeof(FNet) % 4 == 0 && sizeof(FNet) <= STAGE_BYTES, "one word per thread, within the reserved bytes");
    if (threadIdx.x < WORDS) reinterpret_cast<int*>(&staged)[threadIdx.x] = reinterpret_cast<const int*>(&arg)[threadIdx.x];
    __syncthreads();
    return staged;
}

// ---- the proposal --------------------------------------------------------------------------------------------------------------------
// Z[32][N] = X W + b, N of any size <= 64: column block nb on wave nb, the weight loads masked past column N.  K is a width (even).
__device__ void propose_logits(const float* __restrict__ w, int K, int N, const float* X, int px, float* Z) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    for (int nb = wave; nb < (N + 31) / 32; nb += 4) {
        const int n = nb * 32 + i;
        const bool live = n < N;
        const float* wp = w + (live ? n : 0);                  // past column N: column 0 is read, 0 is used
        const float* xp = X + i * px + h;
        f32x16 acc = {};
#pragma unroll 8
        for (int k = 0; k < K; k += 2) {
            const float b = wp[(size_t)(k + h) * N];
            acc = mfma32(xp[k], live ? b : 0.f, acc);
        }
        const float bias = wp[(size_t)K * N];
        if (live) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Z[featF(r, h) * TP + n] = acc[r] + bias;
        }
    }
}

// the features in LDS -> the four tables and the entropies of the tile.  Ends behind a barrier.
__device__ void propose(const FNet& net, const float* __restrict__ fp, const float* fa, float* sm, int64_t row0, int64_t B) {
    const int N = net.N, row = threadIdx.x >> 3, t = threadIdx.x & 7;
    float* lp = sm + net.lp_at + row * TP;
    float* pr = sm + net.pr_at + row * TP;
    float* taus = sm + net.taus_at + row * TP;
    float* tauh = sm + net.tauh_at + row * TP;
    propose_logits(fp, net.n.F, N, fa, net.n.F + 1, sm + net.lp_at);
    __syncthreads();
    const bool live = row0 + row < B;
    float mx = -INFINITY;
    for (int i = t; i < N; i += RPT) mx = fmaxf(mx, lp[i]);
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    mx = fmaxf(mx, __shfl_xor(mx, 4));
    float s = 0.f;
    for (int i = t; i < N; i += RPT) {
        const float e = expf(lp[i] - mx);
        pr[i] = e;                                       // only this thread reads column i before the barrier
        s += e;
    }
    s = row_sum8(s);
    const float ls = logf(s);
    float hs = 0.f;
    for (int i = t; i < N; i += RPT) {
        const float l = (lp[i] - mx) - ls, p = pr[i] / s;
        lp[i] = live ? l : 0.f;
        pr[i] = live ? p : 0.f;
        hs += p * l;
    }
    hs = row_sum8(hs);
    __syncthreads();
    if (t == 0) {
        sm[net.ent_at + row] = live ? -hs : 0.f;
        float c = 0.f;
        taus[0] = 0.f;
        for (int j = 0; j < N; ++j) {                    // torch.cumsum in float32, ascending; F.pad's zero in front
            const float prev = c;
            c = c + pr[j];
            taus[j + 1] = c;
            tauh[j] = (prev + c) / 2.0f;
        }
    }
    __syncthreads();
}

// ---- INFER: FullQuantileFunction.forward + FQFPolicy.forward's weighted q and arg-max; TARGET: FQF._target_q --------------------------
struct FWalkArgs {
    FNet net;
    const float* params; const float* params_old;      // params_old NULL: no lagged network
    const float* fparams;
    const float* obs; int64_t B;
    const float* taus_in; const float* tauh_in;         // INFER: fractions passed in ([B, N + 1], [B, N]) or both NULL
    float* logits; float* q_out; int64_t* act_out; float* qtau_out; float* ent_out;      // INFER
    float* taus_out; float* tauh_out;                   // the fractions used (nullable)
    float* out;                                         // TARGET: [B, N], the n-step returns when mask != NULL
    const float* mask; const double* gpow; const double* mc;
};

template <bool INFER>
__global__ __launch_bounds__(THREADS) void fqfm_walk_kernel(FWalkArgs a) {
    extern __shared__ float sm[];
    const FNet& fnet = stage_fnet(a.net);
    const INet& net = fnet.n;
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7, A = net.n_act, N = fnet.N;
    const int64_t b = row0 + row;
    float* taus = sm + fnet.taus_at;
    float* tauh = sm + fnet.tauh_at;
    load_obs(net, a.obs, row0, a.B, sm);
    const float* fa = features(net, a.params, sm);
    if (INFER && a.taus_in) {
        for (int idx = threadIdx.x; idx < TILE * TP; idx += THREADS) {
            const int r = idx / TP, j = idx - r * TP;
            const bool live = row0 + r < a.B;
            taus[idx] = live && j <= N ? a.taus_in[(row0 + r) * (N + 1) + j] : 0.f;
            tauh[idx] = live && j < N ? a.tauh_in[(row0 + r) * N + j] : 0.f;
        }
        __syncthreads();
    } else {
        propose(fnet, a.fparams, fa, sm, row0, a.B);
        if (INFER && a.ent_out && t == 0 && b < a.B) a.ent_out[b] = sm[fnet.ent_at + row];
    }
    if (b < a.B) {
        if (a.taus_out) for (int j = t; j <= N; j += RPT) a.taus_out[b * (N + 1) + j] = taus[row * TP + j];
        if (a.tauh_out) for (int j = t; j < N; j += RPT) a.tauh_out[b * N + j] = tauh[row * TP + j];
    }
    const TauSrc hats{tauh, TP, 0, TILE};
    float* ob = sm + net.ob_at;
    int* sel = reinterpret_cast<int*>(sm + net.row_at);
    float qa[4] = {0.f, 0.f, 0.f, 0.f};                 // thread (row, t): the weighted sums of the actions t, t + 8, t + 16, t + 24
    for (int j = 0; j < N; ++j) {
        sample_hidden(net, a.params, fa, sm, hats, j);
        sample_head(net, a.params, fa, sm);
        const float wj = taus[row * TP + j + 1] - taus[row * TP + j];        // fqf.py:94
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int act = t + RPT * u;
            if (act < A) {
                const float v = ob[row * OP + act];
                qa[u] += wj * v;
                if (INFER && a.logits && b < a.B) a.logits[(b * A + act) * N + j] = v;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {                       // (each thread overwrites the entries it alone read)
        const int act = t + RPT * u;
        if (act < A) {
            ob[row * OP + act] = qa[u];
            if (INFER && a.q_out && b < a.B) a.q_out[b * A + act] = qa[u];
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
    if (INFER) {
        if (!a.qtau_out) return;
        __syncthreads();                                // (wave 0 rewrites ob)
        const TauSrc inner{taus + 1, TP, 0, TILE};      // discrete.py:313: taus[:, 1:-1]
        for (int j = 0; j < N - 1; ++j) {
            sample_hidden(net, a.params, fa, sm, inner, j);
            sample_head(net, a.params, fa, sm);
            if (b < a.B) for (int act = t; act < A; act += RPT) a.qtau_out[(b * A + act) * (N - 1) + j] = ob[row * OP + act];
        }
        return;
    }
    __syncthreads();
    const bool two = a.params_old != nullptr;
    const float* pe = two ? a.params_old : a.params;
    if (two) fa = features(net, pe, sm);                // (the observations and the fraction tables are still in LDS)
    float* kept = sm + net.th_at;
    const int s = sel[row];
    for (int j = 0; j < N; ++j) {
        sample_hidden(net, pe, fa, sm, hats, j);
        sample_head(net, pe, fa, sm);
        if ((s & 7) == t) kept[row * TP + j] = ob[row * OP + s];
    }
    __syncthreads();
    if (b >= a.B) return;
    if (a.mask) {                                       // compute_nstep_return's arithmetic, per quantile
        const float mk = a.mask[b];
        const double gp = a.gpow[b], mc = a.mc[b];
        for (int j = t; j < N; j += RPT) a.out[b * N + j] = (float)((double)(kept[row * TP + j] * mk) * gp + mc);
    } else {
        for (int j = t; j < N; j += RPT) a.out[b * N + j] = kept[row * TP + j];
    }
}

// ---- STEP ---------------------------------------------------------------------------------------------------------------------------
struct FStepArgs {
    FNet net;
    const float* params; const float* fparams; const float* obs; const int64_t* act;
    const float* returns; const float* weight;          // returns [B, N]
    int64_t B; float ent_coef;
    float* prio_out; float* slabs; float* partials;     // partials [3][tiles]: quantile, fraction, entropy
    float* taus_out; float* tauh_out;                   // nullable
    int tiles;
};

__global__ __launch_bounds__(THREADS) void fqfm_step_kernel(FStepArgs a) {
    extern __shared__ float sm[];
    const FNet& fnet = stage_fnet(a.net);
    const INet& net = fnet.n;
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    const float* p = a.params;
    float* slab = a.slabs + (size_t)blockIdx.x * (net.P + fnet.P2);
    float* th = sm + net.th_at;                              // theta-hat of the taken action per sample, then d loss / d theta-hat
    float* tg = sm + net.tg_at;                              // the targets T
    float* qt = sm + fnet.qt_at;                             // qt[j] = theta_{j+1} (the interior quantiles), then g_{j+1}
    float* taus = sm + fnet.taus_at;
    float* tauh = sm + fnet.tauh_at;
    float* ob = sm + net.ob_at;
    float* df = sm + net.df_at;
    float* term = sm + net.row_at + TILE;                    // [3][32]: the rows' terms of the three losses
    int* sel = reinterpret_cast<int*>(sm + net.row_at);
    const int N = fnet.N, A = net.n_act, F = net.F, pf = F + 1;
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7;
    const int64_t b = row0 + row;
    const bool live = b < a.B;
    if (threadIdx.x < TILE) {                                // rows beyond B select nothing
        const int64_t br = row0 + threadIdx.x;
        int s = -1;
        if (br < a.B) {
            const int64_t ab = a.act[br];
            s = ab < 0 ? 0 : ab >= A ? A - 1 : (int)ab;
        }
        sel[threadIdx.x] = s;
    }
    for (int idx = threadIdx.x; idx < TILE * TP; idx += THREADS) {
        const int r = idx / TP, j = idx - r * TP;
        th[idx] = 0.f;
        qt[idx] = 0.f;
        tg[idx] = row0 + r < a.B && j < N ? a.returns[(row0 + r) * N + j] : 0.f;
    }
    for (int idx = threadIdx.x; idx < TILE * pf; idx += THREADS) df[idx] = 0.f;
    load_obs(net, a.obs, row0, a.B, sm);
    const float* fa = features(net, p, sm);
    propose(fnet, a.fparams, fa, sm, row0, a.B);
    if (live) {
        if (a.taus_out) for (int j = t; j <= N; j += RPT) a.taus_out[b * (N + 1) + j] = taus[row * TP + j];
        if (a.tauh_out) for (int j = t; j < N; j += RPT) a.tauh_out[b * N + j] = tauh[row * TP + j];
    }
    const TauSrc hats{tauh, TP, 0, TILE}, inner{taus + 1, TP, 0, TILE};
    const int s = sel[row];
    for (int j = 0; j < N; ++j) {                            // the forward walk at tau_hats
        sample_hidden(net, p, fa, sm, hats, j);
        sample_head(net, p, fa, sm);
        if (s >= 0 && (s & 7) == t) th[row * TP + j] = ob[row * OP + s];
    }
    for (int j = 0; j < N - 1; ++j) {                        // the forward walk at the interior taus: no gradient
        sample_hidden(net, p, fa, sm, inner, j);
        sample_head(net, p, fa, sm);
        if (s >= 0 && (s & 7) == t) qt[row * TP + j] = ob[row * OP + s];
    }
    __syncthreads();
    {   // gradient_of_taus (fqf.py:227-243) of row (tid >> 3): thread t takes i = 1 + t (mod 8); g_i replaces theta_i behind a barrier
        const float* hat = th + row * TP;
        float* q = qt + row * TP;
        float gv[MAX_SAMPLES / RPT];
#pragma unroll
        for (int u = 0; u < MAX_SAMPLES / RPT; ++u) {
            const int i = 1 + t + RPT * u;
            gv[u] = 0.f;
            if (i < N) {
                const float th_i = q[i - 1];
                const float v1 = th_i - hat[i - 1], v2 = th_i - hat[i];
                const bool s1 = th_i > (i == 1 ? hat[0] : q[i - 2]);
                const bool s2 = th_i < (i == N - 1 ? hat[N - 1] : q[i]);
                gv[u] = (s1 ? v1 : -v1) + (s2 ? v2 : -v2);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < MAX_SAMPLES / RPT; ++u) {
            const int i = 1 + t + RPT * u;
            if (i < N) q[i - 1] = gv[u];
        }
        __syncthreads();
        if (t == 0) {                                        // the row's fraction loss, its suffix sums and dz (over logp)
            const float* tr = taus + row * TP;
            const float* pr = sm + fnet.pr_at + row * TP;
            float* lp = sm + fnet.lp_at + row * TP;
            const float H = sm[fnet.ent_at + row];
            float L = 0.f;
            for (int i = 1; i < N; ++i) L += q[i - 1] * tr[i];
            float S = 0.f;
            for (int k = N - 1; k >= 0; --k) {
                const float pk = pr[k];
                lp[k] = live ? (pk * (S - L) + a.ent_coef * (pk * (lp[k] + H))) / (float)a.B : 0.f;
                if (k >= 1) S += q[k - 1];
            }
            term[TILE + row] = live ? L / (float)a.B : 0.f;
            term[2 * TILE + row] = live ? H / (float)a.B : 0.f;
        }
    }
    {   // the pair loss of the row: tau = tau_hats, constants of the main model
        const float v = pair_loss_row(th, tg, tauh, row * TP, N, N, a.weight, b, a.B, a.prio_out);
        if (t == 0) term[row] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float sum = 0.f;
        for (int m = 0; m < TILE; ++m) sum += term[threadIdx.x * TILE + m];
        a.partials[threadIdx.x * a.tiles + blockIdx.x] = sum;
    }
    wgrad_acc<false>(slab + net.P, true, fa, fa, pf, F, sm + fnet.lp_at, TP, N);      // the fraction network's slab: f^T dz, bias row
    for (int j = 0; j < N; ++j) {                            // the backward walk over the tau_hat samples, j ascending
        sample_hidden(net, p, fa, sm, hats, j);
        sample_backward(net, p, fa, sm, slab, th, sel, j, j == 0);
    }
    trunk_backward(net, p, sm, slab);
}

// ---- the apply launch: both slabs and the three partials in tile order, the lagged copy, the model's Adam ------------------------------
struct FApplyArgs {
    float* p; float* m; float* v; float* p_old;
    const float* slabs; const float* partials; int tiles; int P; int PT;
    float* grad_out; float* fgrad;                      // grad_out nullable; fgrad: the fraction network's gradient, for its optimizer
    float* loss_out;                                    // [3]
    int adam;
    float lr_step, beta2, bc2_sqrt, eps, omb1, omb2;
};

__global__ __launch_bounds__(THREADS) void fqfm_apply_kernel(FApplyArgs a) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < 3) {
        float s = 0.f;
        for (int t = 0; t < a.tiles; ++t) s += a.partials[i * a.tiles + t];
        a.loss_out[i] = s;
    }
    if (i >= a.PT) return;
    float g = 0.f;
    for (int t = 0; t < a.tiles; ++t) g += a.slabs[(size_t)t * a.PT + i];
    if (i >= a.P) {
        a.fgrad[i - a.P] = g;
        return;
    }
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

// ---- host ---------------------------------------------------------------------------------------------------------------------------

// desc (host, TS_FQF_MLP_DESC_LEN int64): ts_iqn_mlp's {obs_dim, n_act, n_trunk, trunk[4], width of the Net's linear output layer or
// 0, num_cosines, n_last} then last_hidden[3] and num_fractions.  LDS carve of one tile, in floats: ts_iqn_walk.h's (obs, trunk,
// [features], cs, phi, `last`, df, ob, th, tg, 4 x 32 row scalars) + five tables 32 x 65 (taus, tau_hats, p, logp / dz, theta / g) +
// 32 entropies, and 512 bytes for the staged description.
//   test_fqf.py   obs 4, [64, 64] -> 64, C 64, H (64, 64, 64), A 2, N 32:
//                 160 + 4,160 + 2,080 + 2,080 + 2,080 + 6,240 + 2,080 + 1,056 + 4,160 + 128 = 24,224; + 10,400 + 32 = 34,656 floats
//                 = 138,624 B, + 512 = 139,136 B of 163,840
int make_fnet(const int64_t* d, const char* who, FNet* out) {
    FNet n{};
    if (int rc = make_inet(d, who, MAX_LAST, &n.n)) return rc;
    if (int rc = check_samples(d[13], "num_fractions", who)) return rc;
    n.N = (int)d[13];
    n.prop = Lay{n.n.F, n.N, 0};
    n.P2 = (n.n.F + 1) * n.N;
    int at = n.n.lds_floats;
    auto carve = [&](int floats) { const int o = at; at += floats; return o; };
    n.taus_at = carve(TILE * TP);
    n.tauh_at = carve(TILE * TP);
    n.pr_at = carve(TILE * TP);
    n.lp_at = carve(TILE * TP);
    n.qt_at = carve(TILE * TP);
    n.ent_at = carve(TILE);
    n.lds_floats = at;
    TS_REQUIRE((size_t)at * 4 + STAGE_BYTES <= (size_t)LDS_LIMIT, TS_ERR_UNSUPPORTED,
               "%s: the activations and fraction tables of one 32-row tile need %zu bytes of LDS, the workgroup limit is %d", who,
               (size_t)at * 4 + STAGE_BYTES, LDS_LIMIT);
    *out = n;
    return TS_OK;
}

inline size_t r64(size_t n) { return (n + 63) / 64 * 64; }
// slabs [tiles][P + P2] | partials [3][tiles] | the model's gradient | the fraction network's gradient | 1024 norm partials
inline size_t fqfm_ws_bytes(const FNet& n, int64_t B) {
    const size_t tiles = (size_t)tiles_of(B), PT = (size_t)n.n.P + n.P2;
    return (tiles * PT + r64(3 * tiles) + r64(n.n.P) + r64(n.P2) + 1024) * 4 + 4096;
}

template <typename Kern>
int allow_lds(ts::DynLds& slot, Kern kern, const FNet& n) {
    return slot.allow(reinterpret_cast<const void*>(kern), (size_t)n.lds_floats * 4);
}

}  // namespace

extern "C" {

int ts_fqf_mlp_layout(const int64_t* desc, int64_t B, int64_t* h_out) {
    TS_REQUIRE(h_out != nullptr, TS_ERR_INVALID_ARG, "ts_fqf_mlp_layout: NULL output");
    TS_REQUIRE(desc != nullptr, TS_ERR_INVALID_ARG, "ts_fqf_mlp_layout: NULL network description");
    FNet n;
    if (int rc = make_fnet(desc, "ts_fqf_mlp_layout", &n)) return rc;
    if (int rc = check_batch(B, "ts_fqf_mlp_layout")) return rc;
    h_out[0] = n.n.P;
    h_out[1] = n.P2;
    h_out[2] = (int64_t)n.lds_floats * 4 + STAGE_BYTES;
    h_out[3] = (int64_t)fqfm_ws_bytes(n, B);
    h_out[4] = n.n.F;
    return TS_OK;
}

int ts_fqf_mlp_forward(const float* params, const float* fparams, const int64_t* desc, const float* obs, int64_t B, const float* taus_in,
                       const float* tau_hats_in, float* logits_out, float* q_out, int64_t* act_out, float* taus_out, float* tau_hats_out,
                       float* entropies_out, float* quantiles_tau_out, ts_stream_t stream) {
    TS_REQUIRE(desc != nullptr, TS_ERR_INVALID_ARG, "ts_fqf_mlp_forward: NULL network description");
    FNet n;
    if (int rc = make_fnet(desc, "ts_fqf_mlp_forward", &n)) return rc;
    if (int rc = check_batch(B, "ts_fqf_mlp_forward")) return rc;
    TS_REQUIRE(params && obs && (logits_out || q_out || act_out || taus_out), TS_ERR_INVALID_ARG, "ts_fqf_mlp_forward: NULL argument");
    TS_REQUIRE((taus_in != nullptr) == (tau_hats_in != nullptr), TS_ERR_INVALID_ARG,
               "ts_fqf_mlp_forward: taus and tau_hats are passed in together or not at all");
    TS_REQUIRE(taus_in || fparams, TS_ERR_INVALID_ARG, "ts_fqf_mlp_forward: neither fractions nor a fraction network");
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, fqfm_walk_kernel<true>, n)) return rc;
    FWalkArgs a{};
    a.net = n; a.params = params; a.fparams = fparams; a.obs = obs; a.B = B; a.taus_in = taus_in; a.tauh_in = tau_hats_in;
    a.logits = logits_out; a.q_out = q_out; a.act_out = act_out; a.qtau_out = quantiles_tau_out;
    a.ent_out = taus_in ? nullptr : entropies_out; a.taus_out = taus_out; a.tauh_out = tau_hats_out;
    hipLaunchKernelGGL(fqfm_walk_kernel<true>, dim3((unsigned)tiles_of(B)), dim3(THREADS), (size_t)n.lds_floats * 4, ts::as_stream(stream), a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_fqf_mlp_next_dist(const float* params, const float* params_old, const float* fparams, const int64_t* desc, const float* obs_next,
                         int64_t B, const float* nstep_mask, const double* nstep_gpow, const double* nstep_mc, float* out, float* taus_out,
                         float* tau_hats_out, ts_stream_t stream) {
    TS_REQUIRE(desc != nullptr, TS_ERR_INVALID_ARG, "ts_fqf_mlp_next_dist: NULL network description");
    FNet n;
    if (int rc = make_fnet(desc, "ts_fqf_mlp_next_dist", &n)) return rc;
    if (int rc = check_batch(B, "ts_fqf_mlp_next_dist")) return rc;
    TS_REQUIRE(params && fparams && obs_next && out, TS_ERR_INVALID_ARG, "ts_fqf_mlp_next_dist: NULL argument");
    TS_REQUIRE((nstep_mask != nullptr) == (nstep_gpow != nullptr) && (nstep_mask != nullptr) == (nstep_mc != nullptr), TS_ERR_INVALID_ARG,
               "ts_fqf_mlp_next_dist: the three n-step coefficient arrays come together or not at all");
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, fqfm_walk_kernel<false>, n)) return rc;
    FWalkArgs a{};
    a.net = n; a.params = params; a.params_old = params_old != params ? params_old : nullptr; a.fparams = fparams; a.obs = obs_next; a.B = B;
    a.taus_out = taus_out; a.tauh_out = tau_hats_out; a.out = out; a.mask = nstep_mask; a.gpow = nstep_gpow; a.mc = nstep_mc;
    hipLaunchKernelGGL(fqfm_walk_kernel<false>, dim3((unsigned)tiles_of(B)), dim3(THREADS), (size_t)n.lds_floats * 4, ts::as_stream(stream), a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_fqf_mlp_update(ts_workspace* ws, float* params, float* params_old, int sync_old, float* adam_m, float* adam_v, int64_t adam_step,
                      float* fparams, float* f_m, float* f_v, int64_t f_step, const int64_t* desc, const float* obs, const int64_t* act,
                      const float* returns, const float* weight, int64_t B, const ts_distq_hparams* hp, const ts_ppo_hparams* fhp,
                      float* losses_out, float* prio_out, float* grad_out, float* fgrad_out, float* taus_out, float* tau_hats_out, ts_stream_t stream) {
    TS_REQUIRE(desc != nullptr, TS_ERR_INVALID_ARG, "ts_fqf_mlp_update: NULL network description");
    FNet n;
    if (int rc = make_fnet(desc, "ts_fqf_mlp_update", &n)) return rc;
    if (int rc = check_batch(B, "ts_fqf_mlp_update")) return rc;
    TS_REQUIRE(params && adam_m && adam_v && fparams && f_m && f_v && obs && act && returns && hp && fhp && losses_out && prio_out,
               TS_ERR_INVALID_ARG, "ts_fqf_mlp_update: NULL argument");
    TS_REQUIRE(adam_step >= 1 && f_step >= 1, TS_ERR_INVALID_ARG, "ts_fqf_mlp_update: the optimizer steps are 1-based");
    TS_REQUIRE(!sync_old || params_old, TS_ERR_INVALID_ARG, "ts_fqf_mlp_update: sync_old without a lagged network");
    TS_REQUIRE(fhp->optimizer == TS_OPT_ADAM || fhp->optimizer == TS_OPT_RMSPROP, TS_ERR_UNSUPPORTED,
               "ts_fqf_mlp_update: fraction optimizer kind %d", fhp->optimizer);
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_fqf_mlp_update: workspace is NULL");
    if (int rc = ts::ws_reserve(ws, fqfm_ws_bytes(n, B))) return rc;
    hipStream_t s = ts::as_stream(stream);
    const int tiles = (int)tiles_of(B), P = n.n.P, PT = P + n.P2;
    float* slabs = static_cast<float*>(ws->base);
    float* partials = slabs + (size_t)tiles * PT;
    float* grad_ws = partials + r64(3 * (size_t)tiles);
    float* fgrad_ws = grad_ws + r64(P);
    float* norm_part = fgrad_ws + r64(n.P2);                        // 1024 floats behind it
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, fqfm_step_kernel, n)) return rc;
    FStepArgs sa{};
    sa.net = n; sa.params = params; sa.fparams = fparams; sa.obs = obs; sa.act = act; sa.returns = returns; sa.weight = weight; sa.B = B;
    sa.ent_coef = (float)fhp->ent_coef; sa.prio_out = prio_out; sa.slabs = slabs; sa.partials = partials; sa.taus_out = taus_out;
    sa.tauh_out = tau_hats_out; sa.tiles = tiles;
    hipLaunchKernelGGL(fqfm_step_kernel, dim3((unsigned)tiles), dim3(THREADS), (size_t)n.lds_floats * 4, s, sa);
    TS_LAUNCH_CHECK();
    const bool step = hp->lr >= 0.0, clip = step && hp->max_grad_norm > 0.0;
    FApplyArgs aa{};
    aa.p = params; aa.m = adam_m; aa.v = adam_v; aa.p_old = sync_old ? params_old : nullptr;
    aa.slabs = slabs; aa.partials = partials; aa.tiles = tiles; aa.P = P; aa.PT = PT;
    aa.grad_out = grad_out ? grad_out : (clip ? grad_ws : nullptr);
    aa.fgrad = fgrad_out ? fgrad_out : fgrad_ws;
    aa.loss_out = losses_out;
    aa.adam = step && !clip;               // clip_grad_norm_ needs the whole gradient first: the sum here, then ts::optim_step
    float sc[2];
    ts::adam_step_scalars(adam_step, hp->lr, hp->beta1, hp->beta2, sc);
    aa.lr_step = sc[0]; aa.bc2_sqrt = sc[1];
    aa.beta2 = (float)hp->beta2; aa.eps = (float)hp->adam_eps;
    aa.omb1 = (float)(1.0 - hp->beta1); aa.omb2 = (float)(1.0 - hp->beta2);
    hipLaunchKernelGGL(fqfm_apply_kernel, dim3((unsigned)ts::ceil_div(PT, THREADS)), dim3(THREADS), 0, s, aa);
    TS_LAUNCH_CHECK();
    if (!step) return TS_OK;
    if (clip) {
        if (int rc = ts::optim_step(s, ts::OptimDesc{}, params, adam_m, adam_v, aa.grad_out, P, adam_step, hp->lr, hp->beta1, hp->beta2,
                                    hp->adam_eps, hp->max_grad_norm, norm_part)) return rc;
    }
    // the fraction optimizer has no max_grad_norm (fqf.py:170)
    return ts::optim_step(s, ts::optim_from(fhp), fparams, f_m, f_v, aa.fgrad, n.P2, f_step, fhp->lr, fhp->beta1, fhp->beta2, fhp->adam_eps,
                          0.0, norm_part);
}

}  // extern "C"
