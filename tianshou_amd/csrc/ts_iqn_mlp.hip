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

#include "ts_iqn_walk.h"      // the network, the sample walk forward and backward, the pair loss (shared with ts_fqf_mlp.hip)

namespace {

constexpr int MAX_LAST = 2;                 // this file's envelope of `last` (the walk itself takes MAX_LAST_H)

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
        sample_hidden(net, a.params, fa, sm, TauSrc{a.tau, a.N, row0, a.B}, j);
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
        sample_hidden(net, pe, fa, sm, TauSrc{a.tau2, a.N2, row0, a.B}, j);
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
    float* ob = sm + net.ob_at;                              // the head's output block (its gradient in the backward walk)
    float* df = sm + net.df_at;
    float* term = sm + net.row_at + TILE;
    int* sel = reinterpret_cast<int*>(sm + net.row_at);
    const int N = a.N, N2 = a.N2, A = net.n_act, pf = net.F + 1;
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
        sample_hidden(net, p, fa, sm, TauSrc{a.tau, N, row0, a.B}, j);
        sample_head(net, p, fa, sm);
        if (s >= 0 && (s & 7) == t) th[row * TP + j] = ob[row * OP + s];
    }
    __syncthreads();
    {   // the pair loss of row (tid >> 3) against the row's N' targets
        const int64_t b = row0 + row;
        const float v = pair_loss_row(th, tg, a.tau, b * N, N, N2, a.weight, b, a.B, a.prio_out);
        if (t == 0) term[row] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sum = 0.f;
        for (int m = 0; m < TILE; ++m) sum += term[m];
        a.partials[blockIdx.x] = sum;
    }
    for (int j = 0; j < N; ++j) {                            // the backward walk: the slab blocks take sample j, j ascending
        sample_hidden(net, p, fa, sm, TauSrc{a.tau, N, row0, a.B}, j);
        sample_backward(net, p, fa, sm, slab, th, sel, j, j == 0);
    }
    trunk_backward(net, p, sm, slab);
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
    if (int rc = make_inet(d, who, MAX_LAST, out)) return rc;
    TS_REQUIRE((size_t)out->lds_floats * 4 + 256 <= (size_t)LDS_LIMIT, TS_ERR_UNSUPPORTED,
               "%s: the activations and sample tables of one 32-row tile need %zu bytes of LDS, the workgroup limit is %d", who,
               (size_t)out->lds_floats * 4 + 256, LDS_LIMIT);
    return TS_OK;
}

inline size_t iqnm_ws_bytes(const INet& n, int64_t B) { return update_scratch(nullptr, tiles_of(B), n.P).bytes; }

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
    const UpdateScratch u = update_scratch(ws->base, tiles, n.P);
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, iqnm_step_kernel, n)) return rc;
    StepArgs sa{n, params, obs, act, tau, (int)N, returns, (int)N2, weight, B, prio_out, u.slabs, u.partials};
    hipLaunchKernelGGL(iqnm_step_kernel, dim3((unsigned)tiles), dim3(THREADS), (size_t)n.lds_floats * 4, s, sa);
    TS_LAUNCH_CHECK();
    return apply_tiles(s, u, tiles, n.P, params, sync_old ? params_old : nullptr, adam_m, adam_v, adam_step, hp, grad_out, loss_out);
}

}  // extern "C"
