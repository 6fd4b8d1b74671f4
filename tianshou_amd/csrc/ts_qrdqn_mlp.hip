// ts_qrdqn_mlp.hip -- QRDQN on vector observations: the plain MLP `Net(softmax=False, num_atoms=N)` (utils/net/common.py:286-369)
// under QRDQN._target_q / _update_with_batch (modelfree/qrdqn.py:94-131) as three launches per update.
//
// The trunk is ts_dqn_mlp.hip's (ts_mlp_tile.h): one four-wave workgroup per 32-row tile, activations resident in odd-pitch LDS,
// weights streamed from L2 into v_mfma_f32_32x32x2_f32 operands, a hidden layer's gradient overwrites its activation, one
// gradient slab per tile summed in tile order by dqnm_apply_kernel.  New here are the A N wide head and the N^2 pair loss:
//   * the head is walked ACTION BY ACTION, so the LDS footprint does not depend on A: action a's N columns are ceil(N / 32)
//     MFMA column blocks (round-robin over the waves) whose weight loads are masked past column N (the address is clamped
//     into the action's own columns, the value replaced by 0): N need be no multiple of 32, 4 or 2;
//   * step kernel: a block's rows are stored only where act[m] == a, into a compact theta table [32][N | 1]; the n-step targets
//     T sit in a second table of the same shape.  Actions that no row of the tile selected are skipped (a 32-bit presence mask
//     in LDS, a workgroup-uniform branch);
//   * pair loss in the tile: eight threads per row, thread t takes the quantiles i = t (mod 8) against all N targets of the
//     row (qr_terms of ts_qr_terms.h: smooth-L1 with kappa 1, weight |tau_i - 1{d <= 0}|, compensated gradient sum); the eight
//     partial sums of a row meet in a fixed butterfly; d theta overwrites theta;
//   * head weight gradient: per present action an MFMA over the tile rows whose d theta operand is masked by act[m] == a; an
//     absent action's slab columns are written as zeros with no matrix work.  Input gradient of the top hidden layer: the sum
//     over the present actions of masked d theta W[:, aN .. aN + N)^T in one accumulator per 32-column block, ReLU mask in place;
//   * target kernel: a "current" and a "kept" table; per action the quantile mean of every row, a running argmax (strictly
//     greater: the first index wins ties) that copies current -> kept.  With a lagged network and double-Q selection the online
//     pass leaves sel[32] only, the lagged pass keeps row sel (and skips actions nobody selected).  The epilogue writes
//     float(double(theta' mask) gamma^n + mc) per quantile: compute_nstep_return's arithmetic on a [B, N] target.
// Flat parameter vector: per layer [K + 1, N] (row K = bias), trunk layers then the head [top + 1, A N], column a N + j.
#pragma clang fp contract(off)
#include <algorithm>

#include "ts_atom_head.h"     // QNet, trunk_forward, head_action / head_wgrad / head_dgrad, row_sum8, launch helpers (shared with ts_c51_mlp.hip)
#include "ts_qr_terms.h"

namespace {

// ---- launch 1: QRDQN._target_q with the n-step arithmetic (INFER: Net.forward, the quantile means, the greedy action) -----------
struct TargetArgs {
    QNet net;
    const float* params; const float* params_old;     // params_old NULL: no lagged network
    const float* obs; int64_t B; int is_double;
    float* dist_out; float* q_out; int64_t* act_out;    // INFER
    float* out;                                         // target_dist[B, N], or the n-step returns when mask != NULL
    const float* mask; const double* gpow; const double* mc;
};

enum { SCAN_INFER, SCAN_SELECT, SCAN_KEEP, SCAN_GATHER };

// The head, action by action, on the tile whose top activation is in LDS.  SELECT / KEEP / INFER: the running argmax of the
// quantile mean -> returned (thread (row, t): its row's); KEEP also leaves that action's row in `kept`.  GATHER: `kept` = the row
// of action sel[row], actions outside `present` skipped.  Ends behind a barrier.
template <int MODE>
__device__ int head_scan(const QNet& net, const float* __restrict__ p, const float* top, int ptop, float* sm, const int* sel, unsigned present,
                         const TargetArgs& a, int64_t b) {
    float* cur = sm + net.ta_at;
    float* kept = sm + net.tb_at;
    const int N = net.n_atoms, A = net.n_act, pt = net.pitch, row = threadIdx.x >> 3, t = threadIdx.x & 7;
    float best = 0.f;
    int arg = 0;
    for (int act = 0; act < A; ++act) {
        if (MODE == SCAN_GATHER && !((present >> act) & 1)) continue;          // workgroup-uniform
        head_action<false>(net, p, act, top, ptop, cur, nullptr);
        __syncthreads();
        const float* mine = cur + row * pt;
        bool take;
        if (MODE == SCAN_GATHER) {
            take = sel[row] == act;
        } else {
            float s = 0.f;
            for (int j = t; j < N; j += RPT) s += mine[j];
            const float q = row_sum8(s) / (float)N;
            take = act == 0 || q > best;                                       // strictly greater: the first index wins ties
            if (take) { best = q; arg = act; }
            if (MODE == SCAN_INFER && b < a.B) {
                if (a.dist_out) for (int j = t; j < N; j += RPT) a.dist_out[(b * A + act) * N + j] = mine[j];
                if (a.q_out && t == 0) a.q_out[b * A + act] = q;
            }
        }
        if ((MODE == SCAN_KEEP || MODE == SCAN_GATHER) && take)
            for (int j = t; j < N; j += RPT) kept[row * pt + j] = mine[j];
        __syncthreads();                                                       // the next action overwrites `cur`
    }
    return arg;
}

template <bool INFER>
__global__ __launch_bounds__(THREADS) void qrm_target_kernel(TargetArgs a) {
    extern __shared__ float sm[];
    const QNet& net = stage_net(a.net);
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7;
    const int64_t b = row0 + row;
    load_obs(net, a.obs, row0, a.B, sm);
    int* sel = reinterpret_cast<int*>(sm + net.row_at + TILE);
    unsigned* present = reinterpret_cast<unsigned*>(sm + net.row_at + 2 * TILE);
    int ptop;
    if (INFER) {
        const float* top = trunk_forward(net, a.params, sm, &ptop);
        const int arg = head_scan<SCAN_INFER>(net, a.params, top, ptop, sm, nullptr, 0u, a, b);
        if (a.act_out && t == 0 && b < a.B) a.act_out[b] = arg;
        return;
    }
    // the selecting network is needed only for the double-Q gather from a lagged network; otherwise the evaluating one selects
    const bool two = a.params_old != nullptr && a.is_double;
    const float* pe = a.params_old ? a.params_old : a.params;
    if (two) {
        const float* top = trunk_forward(net, a.params, sm, &ptop);
        const int arg = head_scan<SCAN_SELECT>(net, a.params, top, ptop, sm, nullptr, 0u, a, b);
        if (t == 0) sel[row] = arg;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned m = 0u;
            for (int r = 0; r < TILE; ++r) m |= 1u << sel[r];
            *present = m;
        }
        top = trunk_forward(net, pe, sm, &ptop);                               // (its barriers publish `present`)
        head_scan<SCAN_GATHER>(net, pe, top, ptop, sm, sel, *present, a, b);
    } else {
        const float* top = trunk_forward(net, pe, sm, &ptop);
        head_scan<SCAN_KEEP>(net, pe, top, ptop, sm, nullptr, 0u, a, b);
    }
    if (b >= a.B) return;
    const int N = net.n_atoms;
    const float* kept = sm + net.tb_at + row * net.pitch;
    if (a.mask) {                                                              // compute_nstep_return's arithmetic, per quantile
        const float mk = a.mask[b];
        const double gp = a.gpow[b], mc = a.mc[b];
        for (int j = t; j < N; j += RPT) a.out[b * N + j] = (float)((double)(kept[j] * mk) * gp + mc);
    } else {
        for (int j = t; j < N; j += RPT) a.out[b * N + j] = kept[j];
    }
}

// ---- launch 2: forward, pair loss, backward, the tile's slab ---------------------------------------------------------------------

struct StepArgs {
    QNet net;
    const float* params; const float* obs; const int64_t* act; const float* returns; const float* weight; const float* tau_hat;
    int64_t B;
    float* prio_out; float* slabs; float* partials;
};

__global__ __launch_bounds__(THREADS) void qrm_step_kernel(StepArgs a) {
    extern __shared__ float sm[];
    const QNet& net = stage_net(a.net);
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    const float* p = a.params;
    float* slab = a.slabs + (size_t)blockIdx.x * net.P;
    float* th = sm + net.ta_at;                              // theta of the taken action, then d loss / d theta
    float* tg = sm + net.tb_at;                              // the targets T
    float* term = sm + net.row_at;
    int* sel = reinterpret_cast<int*>(sm + net.row_at + TILE);
    unsigned* present = reinterpret_cast<unsigned*>(sm + net.row_at + 2 * TILE);
    const int N = net.n_atoms, A = net.n_act, pt = net.pitch;
    if (threadIdx.x < TILE) {                                // rows beyond B select nothing: exactly zero in the loss and in every slab
        const int64_t b = row0 + threadIdx.x;
        int s = -1;
        if (b < a.B) {
            const int64_t ab = a.act[b];
            s = ab < 0 ? 0 : ab >= A ? A - 1 : (int)ab;
        }
        sel[threadIdx.x] = s;
    }
    for (int idx = threadIdx.x; idx < TILE * pt; idx += THREADS) {
        const int row = idx / pt, j = idx - row * pt;
        th[idx] = 0.f;
        tg[idx] = row0 + row < a.B && j < N ? a.returns[(row0 + row) * N + j] : 0.f;
    }
    load_obs(net, a.obs, row0, a.B, sm);
    if (threadIdx.x == 0) {
        unsigned m = 0u;
        for (int r = 0; r < TILE; ++r) if (sel[r] >= 0) m |= 1u << sel[r];
        *present = m;
    }
    int ptop;
    float* top = const_cast<float*>(trunk_forward(net, p, sm, &ptop));         // (its barriers publish `present`)
    const unsigned pres = *present;
    for (int act = 0; act < A; ++act)
        if ((pres >> act) & 1) head_action<true>(net, p, act, top, ptop, th, sel);     // disjoint rows: no barrier between actions
    __syncthreads();
    {   // the pair loss of row (tid >> 3): thread t takes theta_i, i = t (mod 8), against the row's N targets
        const int row = threadIdx.x >> 3, t = threadIdx.x & 7;
        const int64_t b = row0 + row;
        const bool live = b < a.B;
        const float wb = live ? (a.weight ? a.weight[b] : 1.f) : 0.f;
        const float scale = wb / ((float)a.B * (float)N);
        float wl = 0.f, sl = 0.f;
        if (live) {
            float* mine = th + row * pt;
            for (int i = t; i < N; i += RPT) {
                float li, ai, g;
                qr_terms(tg + row * pt, N, mine[i], a.tau_hat[i], li, ai, g);
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
        float s = 0.f;
        for (int m = 0; m < TILE; ++m) s += term[m];
        a.partials[blockIdx.x] = s;
    }
    head_wgrad(net, slab + net.head.off, top, ptop, th, sel, pres);
    __syncthreads();
    head_dgrad(net, p, top, ptop, th, sel, pres);
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

// desc (host, TS_QRDQN_MLP_DESC_LEN int64): ts_dqn_mlp's 14 entries {obs_dim, n_act, dueling, n_trunk, n_q, n_v, trunk[4], q_hidden[2],
// v_hidden[2]} and the number of quantiles.  LDS carve of one tile, in floats: obs 32 (obs_dim + 1) + sum over the hidden layers of
// 32 (width + 1) + 2 x 32 (N | 1) (the two tables) + 4 x 32 (per-row scalars), and 256 bytes for the staged description.  Checked:
//   test_qrdqn.py   obs 4, [128] x 4, A = 2, N = 200: 160 + 4 x 4,128 + 2 x 6,432 + 128 = 29,664 floats = 118,912 B
//   LunarLander     obs 8, [128] x 4, A = 4, N = 200: 288 + 4 x 4,128 + 2 x 6,432 + 128 = 29,792 floats = 119,424 B
//   (refused) [256] x 4, N = 256: 4 x 8,224 + 2 x 8,224 = 49,344 floats > 163,840 B
int make_net(const int64_t* d, const char* who, QNet* out) { return make_qnet(d, who, "quantiles", 2, out, nullptr); }

}  // namespace

extern "C" {

int ts_qrdqn_mlp_layout(const int64_t* desc, int64_t B, int64_t* h_out) {
    TS_REQUIRE(h_out != nullptr, TS_ERR_INVALID_ARG, "ts_qrdqn_mlp_layout: NULL output");
    QNet n;
    if (int rc = make_net(desc, "ts_qrdqn_mlp_layout", &n)) return rc;
    if (int rc = check_batch(B, "ts_qrdqn_mlp_layout")) return rc;
    h_out[0] = n.P;
    h_out[1] = (int64_t)n.lds_floats * 4 + 256;
    h_out[2] = (int64_t)ws_bytes(n, B);
    for (int i = 0; i < MAX_TRUNK; ++i) h_out[3 + i] = i < n.nt ? n.t[i].off : -1;
    h_out[7] = n.head.off;
    return TS_OK;
}

int ts_qrdqn_mlp_forward(const float* params, const int64_t* desc, const float* obs, int64_t B, float* dist_out, float* q_out,
                         int64_t* act_out, ts_stream_t stream) {
    QNet n;
    if (int rc = make_net(desc, "ts_qrdqn_mlp_forward", &n)) return rc;
    if (int rc = check_batch(B, "ts_qrdqn_mlp_forward")) return rc;
    TS_REQUIRE(params && obs && (dist_out || q_out || act_out), TS_ERR_INVALID_ARG, "ts_qrdqn_mlp_forward: NULL argument");
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, qrm_target_kernel<true>, n)) return rc;
    TargetArgs a{n, params, nullptr, obs, B, 0, dist_out, q_out, act_out, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(qrm_target_kernel<true>, dim3((unsigned)tiles_of(B)), dim3(THREADS), (size_t)n.lds_floats * 4, ts::as_stream(stream), a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_qrdqn_mlp_target_dist(const float* params, const float* params_old, const int64_t* desc, const float* obs_next, int64_t B,
                             int is_double, const float* nstep_mask, const double* nstep_gpow, const double* nstep_mc, float* out,
                             ts_stream_t stream) {
    QNet n;
    if (int rc = make_net(desc, "ts_qrdqn_mlp_target_dist", &n)) return rc;
    if (int rc = check_batch(B, "ts_qrdqn_mlp_target_dist")) return rc;
    TS_REQUIRE(params && obs_next && out, TS_ERR_INVALID_ARG, "ts_qrdqn_mlp_target_dist: NULL argument");
    TS_REQUIRE((nstep_mask != nullptr) == (nstep_gpow != nullptr) && (nstep_mask != nullptr) == (nstep_mc != nullptr), TS_ERR_INVALID_ARG,
               "ts_qrdqn_mlp_target_dist: the three n-step coefficient arrays come together or not at all");
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, qrm_target_kernel<false>, n)) return rc;
    TargetArgs a{n, params, params_old == params ? nullptr : params_old, obs_next, B, is_double, nullptr, nullptr, nullptr, out,
                 nstep_mask, nstep_gpow, nstep_mc};
    hipLaunchKernelGGL(qrm_target_kernel<false>, dim3((unsigned)tiles_of(B)), dim3(THREADS), (size_t)n.lds_floats * 4, ts::as_stream(stream), a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_qrdqn_mlp_update(ts_workspace* ws, float* params, float* params_old, int sync_old, float* adam_m, float* adam_v, int64_t adam_step,
                        const int64_t* desc, const float* obs, const int64_t* act, const float* returns, const float* weight,
                        const float* tau_hat, int64_t B, const ts_dqn_hparams* hp, float* loss_out, float* prio_out, float* grad_out,
                        ts_stream_t stream) {
    QNet n;
    if (int rc = make_net(desc, "ts_qrdqn_mlp_update", &n)) return rc;
    if (int rc = check_batch(B, "ts_qrdqn_mlp_update")) return rc;
    TS_REQUIRE(params && adam_m && adam_v && obs && act && returns && tau_hat && hp && loss_out && prio_out, TS_ERR_INVALID_ARG,
               "ts_qrdqn_mlp_update: NULL argument");
    TS_REQUIRE(adam_step >= 1, TS_ERR_INVALID_ARG, "ts_qrdqn_mlp_update: adam_step is 1-based");
    TS_REQUIRE(!sync_old || params_old, TS_ERR_INVALID_ARG, "ts_qrdqn_mlp_update: sync_old without a lagged network");
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_qrdqn_mlp_update: workspace is NULL");
    if (int rc = ts::ws_reserve(ws, ws_bytes(n, B))) return rc;
    hipStream_t s = ts::as_stream(stream);
    const int tiles = (int)tiles_of(B);
    const UpdateScratch u = update_scratch(ws->base, tiles, n.P);
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, qrm_step_kernel, n)) return rc;
    StepArgs sa{n, params, obs, act, returns, weight, tau_hat, B, prio_out, u.slabs, u.partials};
    hipLaunchKernelGGL(qrm_step_kernel, dim3((unsigned)tiles), dim3(THREADS), (size_t)n.lds_floats * 4, s, sa);
    TS_LAUNCH_CHECK();
    return apply_tiles(s, u, tiles, n.P, params, sync_old ? params_old : nullptr, adam_m, adam_v, adam_step, hp, grad_out, loss_out);
}

}  // extern "C"
