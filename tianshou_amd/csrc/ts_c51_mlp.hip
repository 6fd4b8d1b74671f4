// ts_c51_mlp.hip -- C51 on vector observations: the plain MLP `Net(softmax=True, num_atoms=N)` (utils/net/common.py:286-369) under
// C51._target_dist / _update_with_batch (modelfree/c51.py:123-160) as two launches per update: step, apply.
//
// The tile is ts_dqn_mlp.hip's (ts_mlp_tile.h), the A N wide head is ts_qrdqn_mlp.hip's (ts_atom_head.h): one four-wave workgroup per
// 32 batch rows, activations resident in odd-pitch LDS, weights streamed from L2 into v_mfma_f32_32x32x2_f32 operands, the head walked
// action by action with loads masked past column N.  New here, all inside c51m_kernel<MODE>, on three tables [32][N | 1] in LDS:
//   * softmax head: per action the N logits of the tile land in a table; thread (row, t) = (tid >> 3, tid & 7) takes the atoms
//     i = t (mod 8): row maximum, expf(x - max), the sum and the expected value sum p_i z_i each meet in the fixed butterfly (1, 2, 4),
//     so the eight lanes of a row hold the same bits;
//   * selection: a running argmax over the actions of the expected value (strictly greater: the first index wins ties) that copies
//     the normalised row "current" -> "kept".  With a lagged network the online pass leaves sel[32] only; the lagged pass stores, per
//     action that some row selected (32-bit presence mask, a workgroup-uniform branch), only the rows that selected it straight into
//     "kept" (disjoint rows: no barrier between actions) and normalises "kept" once.  With params_old NULL (no lagged network, or a
//     sync iteration: the lagged network IS the online one) the selecting pass keeps the row and the network runs once;
//   * projection in the tile (c51.py:133-141): the third table holds clamp(returns, v_min, v_max); thread (row, t) sums
//     m_i = sum_j clamp(1 - |ts_j - z_i| / delta_z, 0, 1) next_dist_j for its atoms, j ascending (c51_loss_kernel's arithmetic and
//     order); m overwrites "current", which is dead by then.  TARGET stops here;
//   * STEP: forward on obs, rows stored only where act[m] == a into "kept" (dead after the projection), softmax in place,
//     ce_b = -sum_i m_i logf(p_i + 1e-8f), g_i = -(m_i / (p_i + 1e-8f)) (w_b / B), dlogit_i = p_i (g_i - sum_k p_k g_k) in place;
//     then the masked head gradients of ts_atom_head.h and ts_mlp_tile.h's trunk loop: one gradient slab and one loss partial per tile,
//     summed in tile order by dqnm_apply_kernel (fused Adam, lagged copy of the pre-step parameters on sync iterations).
#pragma clang fp contract(off)
#include "ts_atom_head.h"

namespace {

struct CNet {
    QNet q;
    int tc_at;                               // the third table: clamp(returns)
};

enum { C51_INFER, C51_TARGET, C51_STEP };

struct C51Args {
    CNet net;
    const float* params; const float* params_old;       // params_old NULL: the online network is read for the target as well
    const float* support; float v_min, v_max, delta_z;
    const float* obs; const float* obs_next; const float* returns; const int64_t* act; const float* weight;
    int64_t B;
    float* dist_out; float* q_out; int64_t* act_out;      // INFER
    float* target_out;                                    // TARGET; STEP: optional
    float* prio_out; float* slabs; float* partials;       // STEP
};

// The head, action by action, on the tile whose top activation is in LDS: softmax of every action's row, the running argmax of the
// expected value -> returned (thread (row, t): its row's).  KEEP: the argmax's normalised row is left in `kept`.  INFER: the
// probabilities and expected values of every action go to memory.  Ends behind a barrier.
template <bool KEEP, bool INFER>
__device__ int head_select(const QNet& net, const float* __restrict__ p, const float* top, int ptop, float* cur, float* kept, const C51Args& a, int64_t b) {
    const int N = net.n_atoms, A = net.n_act, pt = net.pitch, row = threadIdx.x >> 3, t = threadIdx.x & 7;
    float best = 0.f;
    int arg = 0;
    for (int act = 0; act < A; ++act) {
        head_action<false>(net, p, act, top, ptop, cur, nullptr);
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

template <int MODE>
__global__ __launch_bounds__(THREADS) void c51m_kernel(C51Args a) {
    extern __shared__ float sm[];
    const CNet& cn = stage_net(a.net);
    const QNet& net = cn.q;
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7;
    const int64_t b = row0 + row;
    const int N = net.n_atoms, A = net.n_act, pt = net.pitch;
    float* cur = sm + net.ta_at;                             // logits / probabilities of one action; then the projected target m
    float* kept = sm + net.tb_at;                            // next_dist; then p and d loss / d logit of the taken action
    float* tsup = sm + cn.tc_at;                             // clamp(returns, v_min, v_max)
    float* term = sm + net.row_at;
    int* sel = reinterpret_cast<int*>(sm + net.row_at + TILE);
    unsigned* present = reinterpret_cast<unsigned*>(sm + net.row_at + 2 * TILE);
    int ptop;
    if (MODE == C51_INFER) {
        load_obs(net, a.obs, row0, a.B, sm);
        const float* top = trunk_forward(net, a.params, sm, &ptop);
        const int arg = head_select<false, true>(net, a.params, top, ptop, cur, kept, a, b);
        if (a.act_out && t == 0 && b < a.B) a.act_out[b] = arg;
        return;
    }

    // ---- C51._target_dist on obs_next: next_dist -> `kept`, the projected distribution m -> `cur` ------------------------------------
    for (int idx = threadIdx.x; idx < TILE * pt; idx += THREADS) {
        const int r = idx / pt, j = idx - r * pt;
        tsup[idx] = row0 + r < a.B && j < N ? fminf(fmaxf(a.returns[(row0 + r) * N + j], a.v_min), a.v_max) : 0.f;
    }
    load_obs(net, a.obs_next, row0, a.B, sm);
    if (a.params_old) {                                                        // workgroup-uniform
        const float* top = trunk_forward(net, a.params, sm, &ptop);
        const int arg = head_select<false, false>(net, a.params, top, ptop, cur, kept, a, b);
        if (t == 0) sel[row] = arg;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned m = 0u;
            for (int r = 0; r < TILE; ++r) m |= 1u << sel[r];
            *present = m;
        }
        top = trunk_forward(net, a.params_old, sm, &ptop);                     // (its barriers publish `present`)
        const unsigned pres = *present;
        for (int act = 0; act < A; ++act)
            if ((pres >> act) & 1) head_action<true>(net, a.params_old, act, top, ptop, kept, sel);    // disjoint rows: no barrier between actions
        __syncthreads();
        softmax_row(kept + row * pt, N, t, a.support);
    } else {
        const float* top = trunk_forward(net, a.params, sm, &ptop);
        head_select<true, false>(net, a.params, top, ptop, cur, kept, a, b);
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
    if (MODE == C51_TARGET) return;
    __syncthreads();                                                           // `kept` and sel are dead

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
    float* top = const_cast<float*>(trunk_forward(net, p, sm, &ptop));         // (its barriers publish `present`)
    const unsigned pres = *present;
    for (int act = 0; act < A; ++act)
        if ((pres >> act) & 1) head_action<true>(net, p, act, top, ptop, kept, sel);       // disjoint rows: no barrier between actions
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
    head_wgrad(net, slab + net.head.off, top, ptop, kept, sel, pres);
    __syncthreads();
    head_dgrad(net, p, top, ptop, kept, sel, pres);
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

// desc (host, TS_C51_MLP_DESC_LEN int64): the QRDQN-MLP route's 15 entries, entry 14 the number of atoms.  LDS carve of one tile, in
// floats: obs 32 (obs_dim + 1) + sum over the hidden layers of 32 (width + 1) + 3 x 32 (N | 1) (the three tables) + 4 x 32 (per-row
// scalars), and 256 bytes for the staged description.  Checked:
//   test_c51.py     obs 4, [128] x 4, A = 2, N = 51: 160 + 4 x 4,128 + 3 x 1,632 + 128 = 21,696 floats = 86,784 B
//   LunarLander     obs 8, [128] x 4, A = 4, N = 51: 288 + 4 x 4,128 + 3 x 1,632 + 128 = 21,824 floats = 87,296 B
//   (refused) [256] x 4, N = 256: 160 + 4 x 8,224 + 3 x 8,224 + 128 = 57,856 floats = 231,424 B > 163,840 B
int make_net(const int64_t* d, const char* who, CNet* out) { return make_qnet(d, who, "atoms", 3, &out->q, &out->tc_at); }

template <int MODE>
int launch(const CNet& cn, const C51Args& a, hipStream_t s) {
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, c51m_kernel<MODE>, cn.q)) return rc;
    hipLaunchKernelGGL(c51m_kernel<MODE>, dim3((unsigned)tiles_of(a.B)), dim3(THREADS), (size_t)cn.q.lds_floats * 4, s, a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int check_support(float v_min, float v_max, float delta_z, const char* who) {
    TS_REQUIRE(v_min < v_max && delta_z > 0.f, TS_ERR_INVALID_ARG, "%s: v_min < v_max and delta_z > 0 are needed", who);
    return TS_OK;
}

}  // namespace

extern "C" {

int ts_c51_mlp_layout(const int64_t* desc, int64_t B, int64_t* h_out) {
    TS_REQUIRE(h_out != nullptr, TS_ERR_INVALID_ARG, "ts_c51_mlp_layout: NULL output");
    CNet cn;
    if (int rc = make_net(desc, "ts_c51_mlp_layout", &cn)) return rc;
    if (int rc = check_batch(B, "ts_c51_mlp_layout")) return rc;
    const QNet& n = cn.q;
    h_out[0] = n.P;
    h_out[1] = (int64_t)n.lds_floats * 4 + 256;
    h_out[2] = (int64_t)ws_bytes(n, B);
    for (int i = 0; i < MAX_TRUNK; ++i) h_out[3 + i] = i < n.nt ? n.t[i].off : -1;
    h_out[7] = n.head.off;
    return TS_OK;
}

int ts_c51_mlp_forward(const float* params, const int64_t* desc, const float* support, const float* obs, int64_t B, float* dist_out,
                       float* q_out, int64_t* act_out, ts_stream_t stream) {
    CNet cn;
    if (int rc = make_net(desc, "ts_c51_mlp_forward", &cn)) return rc;
    if (int rc = check_batch(B, "ts_c51_mlp_forward")) return rc;
    TS_REQUIRE(params && support && obs && (dist_out || q_out || act_out), TS_ERR_INVALID_ARG, "ts_c51_mlp_forward: NULL argument");
    C51Args a{};
    a.net = cn; a.params = params; a.support = support; a.obs = obs; a.B = B;
    a.dist_out = dist_out; a.q_out = q_out; a.act_out = act_out;
    return launch<C51_INFER>(cn, a, ts::as_stream(stream));
}

int ts_c51_mlp_target_dist(const float* params, const float* params_old, const int64_t* desc, const float* support, float v_min,
                           float v_max, float delta_z, const float* obs_next, const float* returns, int64_t B, float* out,
                           ts_stream_t stream) {
    CNet cn;
    if (int rc = make_net(desc, "ts_c51_mlp_target_dist", &cn)) return rc;
    if (int rc = check_batch(B, "ts_c51_mlp_target_dist")) return rc;
    TS_REQUIRE(params && support && obs_next && returns && out, TS_ERR_INVALID_ARG, "ts_c51_mlp_target_dist: NULL argument");
    if (int rc = check_support(v_min, v_max, delta_z, "ts_c51_mlp_target_dist")) return rc;
    C51Args a{};
    a.net = cn; a.params = params; a.params_old = params_old == params ? nullptr : params_old;
    a.support = support; a.v_min = v_min; a.v_max = v_max; a.delta_z = delta_z;
    a.obs_next = obs_next; a.returns = returns; a.B = B; a.target_out = out;
    return launch<C51_TARGET>(cn, a, ts::as_stream(stream));
}

int ts_c51_mlp_update(ts_workspace* ws, float* params, float* params_old, int sync_old, float* adam_m, float* adam_v, int64_t adam_step,
                      const int64_t* desc, const float* support, float v_min, float v_max, float delta_z, const float* obs,
                      const int64_t* act, const float* obs_next, const float* returns, const float* weight, int64_t B,
                      const ts_dqn_hparams* hp, float* loss_out, float* prio_out, float* grad_out, float* target_out,
                      ts_stream_t stream) {
    CNet cn;
    if (int rc = make_net(desc, "ts_c51_mlp_update", &cn)) return rc;
    if (int rc = check_batch(B, "ts_c51_mlp_update")) return rc;
    const QNet& n = cn.q;
    TS_REQUIRE(params && adam_m && adam_v && support && obs && act && obs_next && returns && hp && loss_out && prio_out, TS_ERR_INVALID_ARG,
               "ts_c51_mlp_update: NULL argument");
    if (int rc = check_support(v_min, v_max, delta_z, "ts_c51_mlp_update")) return rc;
    TS_REQUIRE(adam_step >= 1, TS_ERR_INVALID_ARG, "ts_c51_mlp_update: adam_step is 1-based");
    TS_REQUIRE(!sync_old || params_old, TS_ERR_INVALID_ARG, "ts_c51_mlp_update: sync_old without a lagged network");
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_c51_mlp_update: workspace is NULL");
    if (int rc = ts::ws_reserve(ws, ws_bytes(n, B))) return rc;
    hipStream_t s = ts::as_stream(stream);
    const int tiles = (int)tiles_of(B);
    const UpdateScratch u = update_scratch(ws->base, tiles, n.P);
    C51Args a{};
    a.net = cn; a.params = params;
    // the sync comes before the target (c51.py:147-149): on a sync iteration the lagged network IS the online one, read once
    a.params_old = sync_old || params_old == params ? nullptr : params_old;
    a.support = support; a.v_min = v_min; a.v_max = v_max; a.delta_z = delta_z;
    a.obs = obs; a.obs_next = obs_next; a.returns = returns; a.act = act; a.weight = weight; a.B = B;
    a.target_out = target_out; a.prio_out = prio_out; a.slabs = u.slabs; a.partials = u.partials;
    if (int rc = launch<C51_STEP>(cn, a, s)) return rc;
    return apply_tiles(s, u, tiles, n.P, params, sync_old ? params_old : nullptr, adam_m, adam_v, adam_step, hp, grad_out, loss_out);
}

}  // extern "C"
