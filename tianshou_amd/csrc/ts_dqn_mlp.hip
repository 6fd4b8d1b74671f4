// ts_dqn_mlp.hip -- DQN on vector observations: the dueling MLP `Net` (utils/net/common.py:246-370) under
// DQN._target_q / _update_with_batch (modelfree/dqn.py:365-404) as three launches per update.
//
// At B = 64 .. 128 on 128-wide layers a layer-by-layer route is launch latency and nothing else, and the network (84 k floats
// for lunarlander_dqn.py) is twice the LDS, so the CartPole trick (weights in LDS) does not carry over.  Here the ACTIVATIONS
// are resident and the WEIGHTS are streamed:
//   * one 256-thread workgroup (four waves) owns a tile of 32 batch rows and runs the whole chain for it; every hidden
//     activation of the tile stays in an odd-pitch LDS array (width + 1 floats per row: the row walk of the forward pass, the
//     column walk of H^T dZ and the row walk of dZ W^T are all bank-conflict free from the one copy);
//   * a layer is a set of 32-column output blocks, block n on wave n mod 4, each a chain of v_mfma_f32_32x32x2_f32 whose A
//     operand comes from LDS and whose B operand is loaded from L2 straight into the operand register (forward: W[k + h][n],
//     128 contiguous bytes per half wave; input gradient: 16-byte loads along the reduction index of row W[k][.]); no barrier
//     inside a reduction loop, one barrier between layers;
//   * backward, the gradient of a hidden layer OVERWRITES the activation it is masked by (dZ = dH * (H > 0) needs H at the
//     same position only), after the weight gradients that read H are out: no gradient arrays are carved at all;
//   * the A <= 32 head and the one-output V head are VALU dot products (a padded fp32 MFMA tile measured 2.7x the VALU head at
//     6 of 32 rows; here at most A of 32 columns would be live);
//   * every tile writes a full-size gradient "slab"; dqnm_apply_kernel sums slabs and loss partials in tile order (bit-identical
//     from run to run), takes the Adam step with torch's single-tensor formulas and makes the lagged copy of the pre-step
//     parameters in the same pass.
// Flat parameter vector: per layer [K + 1, N] (row K = bias), order trunk | Q hidden | V hidden | Q head [., A] | V head [., 1].
#pragma clang fp contract(off)
#include <algorithm>

#include "ts_mlp_tile.h"     // the tile's layer passes (dense_relu, wgrad, dgrad), stage_net / load_obs, dqnm_apply_kernel

namespace {

constexpr int QP = 33;                      // pitch of the [32][A <= 32] head arrays
constexpr int MAX_TRUNK = 4, MAX_STREAM = 2;

struct Net {
    int obs_dim, n_act, dueling, nt, nq, nv;
    Lay t[MAX_TRUNK], q[MAX_STREAM + 1], v[MAX_STREAM + 1];      // q[nq] / v[nv]: the heads
    int x_at, t_at[MAX_TRUNK], q_at[MAX_STREAM], v_at[MAX_STREAM];   // LDS float offsets of obs and of every hidden activation
    int qa_at, qb_at, va_at, row_at;        // Q tables [32][33] x 2, V column [32], per-row scalars [32]
    int P, lds_floats;
};

// out[32][A] = X[32][K] W + b on the VALU: thread (row, a)
__device__ void head_forward(const float* __restrict__ w, int K, int A, const float* X, int px, float* out, int po) {
    for (int idx = threadIdx.x; idx < TILE * A; idx += THREADS) {
        const int row = idx & 31, a = idx >> 5;
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += X[row * px + k] * w[k * A + a];
        out[row * po + a] = s + w[K * A + a];
    }
}

// Net.forward on the tile whose observations are in LDS: q (combined when dueling) -> qout[32][QP].  Ends behind a barrier.
__device__ void net_forward(const Net& net, const float* __restrict__ p, float* sm, float* qout) {
    const float* x = sm + net.x_at;
    int px = net.obs_dim + 1;
    for (int l = 0; l < net.nt; ++l) {
        float* y = sm + net.t_at[l];
        dense_relu(p + net.t[l].off, net.t[l].K, net.t[l].N, x, px, y, net.t[l].N + 1);
        __syncthreads();
        x = y; px = net.t[l].N + 1;
    }
    const float* top = x;
    const int ptop = px;
    // the two streams are independent: Q then V hidden layers share barriers level by level
    const float* xq = top; int pq = ptop;
    const float* xv = top; int pv = ptop;
    for (int l = 0; l < MAX_STREAM; ++l) {
        if (l >= net.nq && l >= net.nv) break;
        if (l < net.nq) dense_relu(p + net.q[l].off, net.q[l].K, net.q[l].N, xq, pq, sm + net.q_at[l], net.q[l].N + 1);
        if (l < net.nv) dense_relu(p + net.v[l].off, net.v[l].K, net.v[l].N, xv, pv, sm + net.v_at[l], net.v[l].N + 1);
        __syncthreads();
        if (l < net.nq) { xq = sm + net.q_at[l]; pq = net.q[l].N + 1; }
        if (l < net.nv) { xv = sm + net.v_at[l]; pv = net.v[l].N + 1; }
    }
    head_forward(p + net.q[net.nq].off, net.q[net.nq].K, net.n_act, xq, pq, qout, QP);
    if (net.dueling) head_forward(p + net.v[net.nv].off, net.v[net.nv].K, 1, xv, pv, sm + net.va_at, 1);
    __syncthreads();
    if (net.dueling) {                      // logits = q - q.mean(dim=1) + v (common.py:364)
        if (threadIdx.x < TILE) {
            float* q = qout + threadIdx.x * QP;
            float s = 0.f;
            for (int a = 0; a < net.n_act; ++a) s += q[a];
            const float mean = s / (float)net.n_act, v = sm[net.va_at + threadIdx.x];
            for (int a = 0; a < net.n_act; ++a) q[a] = q[a] - mean + v;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int argmax_first(const float* q, int A) {       // torch.max: the first index wins ties
    int best = 0;
    for (int a = 1; a < A; ++a) if (q[a] > q[best]) best = a;
    return best;
}

// ---- launch 1: DQN._target_q (INFER: Net.forward + the greedy action) ---------------------------------------------------------
struct TargetArgs {
    Net net;
    const float* params; const float* params_old;     // params_old NULL: no lagged network
    const float* obs; int64_t B; int is_double;
    float* q_out; int64_t* act_out;                     // INFER
    float* out;                                         // target_q[B], or the n-step returns when mask != NULL
    const float* mask; const double* gpow; const double* mc;
};

template <bool INFER>
__global__ __launch_bounds__(THREADS) void dqnm_target_kernel(TargetArgs a) {
    extern __shared__ float sm[];
    const Net& net = stage_net(a.net);
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    load_obs(net, a.obs, row0, a.B, sm);
    float* qa = sm + net.qa_at;
    float* qb = sm + net.qb_at;
    const int A = net.n_act;
    if (INFER) {
        net_forward(net, a.params, sm, qa);
        const int64_t b = row0 + threadIdx.x;
        if (threadIdx.x < TILE && b < a.B) {
            if (a.q_out) for (int j = 0; j < A; ++j) a.q_out[b * A + j] = qa[threadIdx.x * QP + j];
            if (a.act_out) a.act_out[b] = argmax_first(qa + threadIdx.x * QP, A);
        }
        return;
    }
    // the selecting network is needed only for the double-Q gather from a lagged network; otherwise max of the evaluating one
    const bool two = a.params_old != nullptr && a.is_double;
    if (two) net_forward(net, a.params, sm, qa);
    net_forward(net, a.params_old ? a.params_old : a.params, sm, qb);
    const int64_t b = row0 + threadIdx.x;
    if (threadIdx.x < TILE && b < a.B) {
        const float* qe = qb + threadIdx.x * QP;
        const float tq = qe[argmax_first(two ? qa + threadIdx.x * QP : qe, A)];
        a.out[b] = a.mask ? (float)((double)(tq * a.mask[b]) * a.gpow[b] + a.mc[b]) : tq;     // compute_nstep_return's arithmetic
    }
}

// ---- launch 2: forward, loss, backward, the tile's slab ------------------------------------------------------------------------

__device__ void head_wgrad(float* __restrict__ slab, const float* Hin, int pin, int K, const float* dq, int pq, int A) {
    for (int idx = threadIdx.x; idx < (K + 1) * A; idx += THREADS) {
        const int k = idx / A, a = idx - k * A;
        float s = 0.f;
        for (int m = 0; m < TILE; ++m) s += (k < K ? Hin[m * pin + k] : 1.f) * dq[m * pq + a];
        slab[idx] = s;
    }
}

struct StepArgs {
    Net net;
    const float* params; const float* obs; const int64_t* act; const float* returns; const float* weight;
    int64_t B; float huber_delta;                       // <= 0: (td^2 * weight).mean()
    float* td_out; float* slabs; float* partials;
};

// one stream (Q or V) from its head down to its first layer: slabs of all its layers; afterwards dZ of its first hidden layer
// sits in LDS (n > 0) -- the input gradient into the trunk's top is left to the caller, which adds the two streams
__device__ void stream_backward(const Lay* lay, const int* at, int n, int A, const float* dq, int pq, const float* top, int ptop,
                                const float* __restrict__ p, float* __restrict__ slab, float* sm) {
    const float* hin = n > 0 ? sm + at[n - 1] : top;
    head_wgrad(slab + lay[n].off, hin, n > 0 ? lay[n - 1].N + 1 : ptop, lay[n].K, dq, pq, A);
    if (n == 0) return;
    __syncthreads();
    HSrc hs{dq, pq, p + lay[n].off, A};
    dgrad(sm + at[n - 1], lay[n - 1].N + 1, lay[n - 1].N, MSrc{}, MSrc{}, hs, HSrc{});
    __syncthreads();
    for (int l = n - 1; l >= 0; --l) {
        const float* in = l > 0 ? sm + at[l - 1] : top;
        wgrad(slab + lay[l].off, in, l > 0 ? lay[l - 1].N + 1 : ptop, lay[l].K, sm + at[l], lay[l].N + 1, lay[l].N);
        if (l == 0) break;
        __syncthreads();
        MSrc ms{sm + at[l], lay[l].N + 1, p + lay[l].off, lay[l].N};
        dgrad(sm + at[l - 1], lay[l - 1].N + 1, lay[l - 1].N, ms, MSrc{}, HSrc{}, HSrc{});
        __syncthreads();
    }
}

__global__ __launch_bounds__(THREADS) void dqnm_step_kernel(StepArgs a) {
    extern __shared__ float sm[];
    const Net& net = stage_net(a.net);
    const int64_t row0 = (int64_t)blockIdx.x * TILE;
    const float* p = a.params;
    float* slab = a.slabs + (size_t)blockIdx.x * net.P;
    float* q = sm + net.qa_at;
    float* dq = sm + net.qb_at;
    float* dv = sm + net.va_at;
    float* term = sm + net.row_at;
    const int A = net.n_act;
    load_obs(net, a.obs, row0, a.B, sm);
    net_forward(net, p, sm, q);
    if (threadIdx.x < TILE) {
        const int64_t b = row0 + threadIdx.x;
        float g = 0.f, t = 0.f;                              // rows beyond B: exactly zero in the loss and in every slab
        int sel = 0;
        if (b < a.B) {
            const int64_t ab = a.act[b];
            sel = ab < 0 ? 0 : ab >= A ? A - 1 : (int)ab;
            const float td = a.returns[b] - q[threadIdx.x * QP + sel];
            a.td_out[b] = td;
            const float nb = (float)a.B;
            if (a.huber_delta > 0.f) {                       // F.huber_loss(q, returns, delta, "mean"): the PER weight is not used (dqn.py:392-397)
                const float d = -td, ad = fabsf(d);
                t = (ad < a.huber_delta ? 0.5f * d * d : a.huber_delta * (ad - 0.5f * a.huber_delta)) / nb;
                g = (ad < a.huber_delta ? d : (d > 0.f ? a.huber_delta : -a.huber_delta)) / nb;
            } else {
                const float w = a.weight ? a.weight[b] : 1.f;
                t = td * td * w / nb;
                g = -2.f * td * w / nb;
            }
        }
        term[threadIdx.x] = t;
        const float share = net.dueling ? g / (float)A : 0.f;        // d(q - mean q + v): dq_j = g (delta_ja - 1 / A), dv = g
        for (int j = 0; j < A; ++j) dq[threadIdx.x * QP + j] = (j == sel ? g : 0.f) - share;
        dv[threadIdx.x] = g;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int m = 0; m < TILE; ++m) s += term[m];
        a.partials[blockIdx.x] = s;
    }
    float* top = sm + net.t_at[net.nt - 1];
    const int wtop = net.t[net.nt - 1].N, ptop = wtop + 1;
    stream_backward(net.q, net.q_at, net.nq, A, dq, QP, top, ptop, p, slab, sm);
    if (net.dueling) stream_backward(net.v, net.v_at, net.nv, 1, dv, 1, top, ptop, p, slab, sm);
    __syncthreads();
    {   // the trunk's top: the input gradients of both streams, summed in one accumulator
        MSrc mq{}, mv{};
        HSrc hq{}, hv{};
        if (net.nq > 0) mq = MSrc{sm + net.q_at[0], net.q[0].N + 1, p + net.q[0].off, net.q[0].N};
        else hq = HSrc{dq, QP, p + net.q[0].off, A};
        if (net.dueling && net.nv > 0) mv = MSrc{sm + net.v_at[0], net.v[0].N + 1, p + net.v[0].off, net.v[0].N};
        else if (net.dueling) hv = HSrc{dv, 1, p + net.v[0].off, 1};
        dgrad(top, ptop, wtop, mq, mv, hq, hv);
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

// desc (host, TS_DQN_MLP_DESC_LEN int64): {obs_dim, n_act, dueling, n_trunk, n_q, n_v, trunk[4], q_hidden[2], v_hidden[2]}.
// LDS carve of one tile, in floats: obs 32 (obs_dim + 1) + sum over the hidden layers of 32 (width + 1) + 2 x 32 x 33 (Q tables)
// + 2 x 32 (V column, per-row terms), and 256 bytes for the staged description.  No gradient arrays: a hidden layer's gradient overwrites its activation.  Checked:
//   discrete_dqn.py      obs 4, [128, 128, 128], plain:                 160 + 3 x 4,128 + 2,176 = 14,720 floats =  58,880 B
//   lunarlander_dqn.py   obs 8, [128, 128] + Q [128, 128] + V [128, 128]: 288 + 6 x 4,128 + 2,176 = 27,232 floats = 108,928 B
//   acrobot_dualdqn.py   obs 6, [128] + Q [128, 128] + V [128, 128]:     224 + 5 x 4,128 + 2,176 = 23,040 floats =  92,160 B
//   (refused) 4 + 2 + 2 layers of 256: 8 x 32 x 257 = 65,792 floats = 263,168 B > 163,840 B
int make_net(const int64_t* d, const char* who, Net* out) {
    TS_REQUIRE(d != nullptr, TS_ERR_INVALID_ARG, "%s: NULL network description", who);
    Net n{};
    const int64_t obs_dim = d[0], n_act = d[1], nt = d[3], nq = d[4], nv = d[5];
    TS_REQUIRE(obs_dim >= 1 && obs_dim <= 256, TS_ERR_UNSUPPORTED, "%s: obs_dim %lld outside [1, 256]", who, (long long)obs_dim);
    TS_REQUIRE(n_act >= 1 && n_act <= 32, TS_ERR_UNSUPPORTED, "%s: %lld actions outside [1, 32]", who, (long long)n_act);
    TS_REQUIRE(nt >= 1 && nt <= MAX_TRUNK, TS_ERR_UNSUPPORTED, "%s: %lld trunk hidden layers outside [1, 4]", who, (long long)nt);
    TS_REQUIRE(nq >= 0 && nq <= MAX_STREAM && nv >= 0 && nv <= MAX_STREAM, TS_ERR_UNSUPPORTED, "%s: Q / V streams have 0 .. 2 hidden layers", who);
    TS_REQUIRE(d[2] == 0 || d[2] == 1, TS_ERR_INVALID_ARG, "%s: dueling must be 0 or 1", who);
    TS_REQUIRE(d[2] == 1 || (nq == 0 && nv == 0), TS_ERR_INVALID_ARG, "%s: a plain Net has no Q / V hidden layers", who);
    n.obs_dim = (int)obs_dim; n.n_act = (int)n_act; n.dueling = (int)d[2]; n.nt = (int)nt; n.nq = (int)nq; n.nv = (int)nv;
    int off = 0, at = 0;
    auto width_ok = [](int64_t w) { return w >= 32 && w <= 256 && w % 32 == 0; };
    auto add = [&](Lay* l, int K, int N) { l->K = K; l->N = N; l->off = off; off += (K + 1) * N; };
    auto carve = [&](int floats) { const int o = at; at += floats; return o; };
    n.x_at = carve(TILE * (n.obs_dim + 1));
    int k = n.obs_dim;
    for (int i = 0; i < n.nt; ++i) {
        TS_REQUIRE(width_ok(d[6 + i]), TS_ERR_UNSUPPORTED, "%s: hidden width %lld is no multiple of 32 in [32, 256]", who, (long long)d[6 + i]);
        add(&n.t[i], k, (int)d[6 + i]);
        n.t_at[i] = carve(TILE * (n.t[i].N + 1));
        k = n.t[i].N;
    }
    const int top = k;
    int kq = top, kv = top;
    for (int i = 0; i < n.nq; ++i) {
        TS_REQUIRE(width_ok(d[10 + i]), TS_ERR_UNSUPPORTED, "%s: hidden width %lld is no multiple of 32 in [32, 256]", who, (long long)d[10 + i]);
        add(&n.q[i], kq, (int)d[10 + i]);
        n.q_at[i] = carve(TILE * (n.q[i].N + 1));
        kq = n.q[i].N;
    }
    for (int i = 0; i < n.nv; ++i) {
        TS_REQUIRE(width_ok(d[12 + i]), TS_ERR_UNSUPPORTED, "%s: hidden width %lld is no multiple of 32 in [32, 256]", who, (long long)d[12 + i]);
        add(&n.v[i], kv, (int)d[12 + i]);
        n.v_at[i] = carve(TILE * (n.v[i].N + 1));
        kv = n.v[i].N;
    }
    add(&n.q[n.nq], kq, n.n_act);
    if (n.dueling) add(&n.v[n.nv], kv, 1);
    n.qa_at = carve(TILE * QP);
    n.qb_at = carve(TILE * QP);
    n.va_at = carve(TILE);
    n.row_at = carve(TILE);
    n.P = off;
    n.lds_floats = at;
    TS_REQUIRE((size_t)at * 4 + 256 <= (size_t)LDS_LIMIT, TS_ERR_UNSUPPORTED,
               "%s: the activations of one 32-row tile need %zu bytes of LDS, the workgroup limit is %d", who, (size_t)at * 4 + 256, LDS_LIMIT);
    *out = n;
    return TS_OK;
}

inline int64_t tiles_of(int64_t B) { return ts::ceil_div(B, TILE); }
inline size_t ws_bytes(const Net& n, int64_t B) { return update_scratch(nullptr, tiles_of(B), n.P).bytes; }

template <typename Kern>
int allow_lds(ts::DynLds& slot, Kern kern, const Net& n) {
    return slot.allow(reinterpret_cast<const void*>(kern), (size_t)n.lds_floats * 4);
}

int check_batch(int64_t B, const char* who) {
    TS_REQUIRE(B >= 1 && B <= 4096, B < 1 ? TS_ERR_INVALID_ARG : TS_ERR_UNSUPPORTED, "%s: B = %lld outside [1, 4096]", who, (long long)B);
    return TS_OK;
}

int launch_target(const Net& n, const float* params, const float* params_old, const float* obs_next, int64_t B, int is_double,
                  const float* mask, const double* gpow, const double* mc, float* out, hipStream_t s) {
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, dqnm_target_kernel<false>, n)) return rc;
    TargetArgs a{n, params, params_old == params ? nullptr : params_old, obs_next, B, is_double, nullptr, nullptr, out, mask, gpow, mc};
    hipLaunchKernelGGL(dqnm_target_kernel<false>, dim3((unsigned)tiles_of(B)), dim3(THREADS), (size_t)n.lds_floats * 4, s, a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

}  // namespace

extern "C" {

int ts_dqn_mlp_layout(const int64_t* desc, int64_t B, int64_t* h_out) {
    TS_REQUIRE(h_out != nullptr, TS_ERR_INVALID_ARG, "ts_dqn_mlp_layout: NULL output");
    Net n;
    if (int rc = make_net(desc, "ts_dqn_mlp_layout", &n)) return rc;
    if (int rc = check_batch(B, "ts_dqn_mlp_layout")) return rc;
    h_out[0] = n.P;
    h_out[1] = (int64_t)n.lds_floats * 4;
    h_out[2] = (int64_t)ws_bytes(n, B);
    int o = 3;
    for (int i = 0; i < MAX_TRUNK; ++i) h_out[o++] = i < n.nt ? n.t[i].off : -1;
    for (int i = 0; i < MAX_STREAM; ++i) h_out[o++] = i < n.nq ? n.q[i].off : -1;
    for (int i = 0; i < MAX_STREAM; ++i) h_out[o++] = i < n.nv ? n.v[i].off : -1;
    h_out[o++] = n.q[n.nq].off;
    h_out[o++] = n.dueling ? n.v[n.nv].off : -1;
    return TS_OK;
}

int ts_dqn_mlp_forward(const float* params, const int64_t* desc, const float* obs, int64_t B, float* q_out, int64_t* act_out,
                       ts_stream_t stream) {
    Net n;
    if (int rc = make_net(desc, "ts_dqn_mlp_forward", &n)) return rc;
    if (int rc = check_batch(B, "ts_dqn_mlp_forward")) return rc;
    TS_REQUIRE(params && obs && (q_out || act_out), TS_ERR_INVALID_ARG, "ts_dqn_mlp_forward: NULL argument");
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, dqnm_target_kernel<true>, n)) return rc;
    TargetArgs a{n, params, nullptr, obs, B, 0, q_out, act_out, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(dqnm_target_kernel<true>, dim3((unsigned)tiles_of(B)), dim3(THREADS), (size_t)n.lds_floats * 4, ts::as_stream(stream), a);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_dqn_mlp_target_q(const float* params, const float* params_old, const int64_t* desc, const float* obs_next, int64_t B,
                        int is_double, const float* nstep_mask, const double* nstep_gpow, const double* nstep_mc, float* out,
                        ts_stream_t stream) {
    Net n;
    if (int rc = make_net(desc, "ts_dqn_mlp_target_q", &n)) return rc;
    if (int rc = check_batch(B, "ts_dqn_mlp_target_q")) return rc;
    TS_REQUIRE(params && obs_next && out, TS_ERR_INVALID_ARG, "ts_dqn_mlp_target_q: NULL argument");
    TS_REQUIRE((nstep_mask != nullptr) == (nstep_gpow != nullptr) && (nstep_mask != nullptr) == (nstep_mc != nullptr), TS_ERR_INVALID_ARG,
               "ts_dqn_mlp_target_q: the three n-step coefficient arrays come together or not at all");
    return launch_target(n, params, params_old, obs_next, B, is_double, nstep_mask, nstep_gpow, nstep_mc, out, ts::as_stream(stream));
}

int ts_dqn_mlp_update(ts_workspace* ws, float* params, float* params_old, int sync_old, float* adam_m, float* adam_v, int64_t adam_step,
                      const int64_t* desc, const float* obs, const int64_t* act, const float* returns, const float* weight, int64_t B,
                      const ts_dqn_hparams* hp, float* td_out, float* loss_out, float* grad_out, ts_stream_t stream) {
    Net n;
    if (int rc = make_net(desc, "ts_dqn_mlp_update", &n)) return rc;
    if (int rc = check_batch(B, "ts_dqn_mlp_update")) return rc;
    TS_REQUIRE(params && adam_m && adam_v && obs && act && returns && hp && td_out && loss_out, TS_ERR_INVALID_ARG, "ts_dqn_mlp_update: NULL argument");
    TS_REQUIRE(adam_step >= 1, TS_ERR_INVALID_ARG, "ts_dqn_mlp_update: adam_step is 1-based");
    TS_REQUIRE(!sync_old || params_old, TS_ERR_INVALID_ARG, "ts_dqn_mlp_update: sync_old without a lagged network");
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_dqn_mlp_update: workspace is NULL");
    if (int rc = ts::ws_reserve(ws, ws_bytes(n, B))) return rc;
    hipStream_t s = ts::as_stream(stream);
    const int tiles = (int)tiles_of(B);
    const UpdateScratch u = update_scratch(ws->base, tiles, n.P);
    static ts::DynLds lds;
    if (int rc = allow_lds(lds, dqnm_step_kernel, n)) return rc;
    StepArgs sa{n, params, obs, act, returns, weight, B, (float)hp->huber_delta, td_out, u.slabs, u.partials};
    hipLaunchKernelGGL(dqnm_step_kernel, dim3((unsigned)tiles), dim3(THREADS), (size_t)n.lds_floats * 4, s, sa);
    TS_LAUNCH_CHECK();
    return apply_tiles(s, u, tiles, n.P, params, sync_old ? params_old : nullptr, adam_m, adam_v, adam_step, hp, grad_out, loss_out);
}

}  // extern "C"
