// ts_bcq.hip -- discrete batch-constrained Q-learning (DiscreteBCQ, arXiv:1910.01708) on the Atari trunk for gfx950.
//
// Replaces, on device-resident NHWC observations:
//   DiscreteActor.forward (twice, one trunk)   tianshou/utils/net/discrete.py (preprocess_net = DQNet(features_only=True),
//                                              hidden_sizes = [512], softmax_output = False; examples/offline/atari_bcq.py:100-118)
//   DiscreteBCQPolicy.forward                  tianshou/algorithm/imitation/discrete_bcq.py:104-127 (threshold-masked argmax)
//   DiscreteBCQ._target_q                      discrete_bcq.py:228-234
//   DiscreteBCQ._update_with_batch             discrete_bcq.py:236-261 (Huber + NLL + logit penalty, both heads into one trunk)
//   Optimizer.step                             algorithm_base.py:484-500 (clip_grad_norm_ + ONE Adam over all 14 tensors)
//
//   feat[b, :]   = relu(conv3(relu(conv2(relu(conv1(obs[b]))))))      F = 64 * OH3 * OW3 features in (h, w, c) order
//   Q[b, :]      = relu(feat[b] @ Wq1 + bq1) @ Wq2 + bq2              the Q head
//   logits[b, :] = relu(feat[b] @ Wi1 + bi1) @ Wi2 + bi2              the imitator, on the SAME features
// Every layer runs through the fp32-MFMA implicit-GEMM kernels of ts_conv.hip; this file adds the per-sample kernels (masked
// argmax, target selection, the three-term loss with both head gradients, the sum of the two feature gradients) and the
// orchestration.  Flat parameter layout: conv1 | conv2 | conv3 | [Wq1; bq1] [F + 1, 512] | [Wq2; bq2] [513, ld] |
// [Wi1; bi1] [F + 1, 512] | [Wi2; bi2] [513, ld], ld = n_act rounded up to a multiple of 32 (GEMM tile width; the padding
// columns are and stay exactly zero).  The lagged vector has the same length; its imitator part is never read.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "ts_common.h"
#include "ts_conv.h"

#pragma clang fp contract(off)

#include "ts_twin.h"

namespace ts {
int adam_step(hipStream_t s, float* params, float* m, float* v, const float* grad, int64_t n, int64_t step,
              double lr, double beta1, double beta2, double eps, double max_grad_norm, float* norm_scratch);
}

namespace {

// DiscreteBCQPolicy.forward's action (discrete_bcq.py:116-118) of one sample, one wave: lane a < A holds q = Q[b, a] and
// lg = logits[b, a].  ratio = lg - max_a lg and the comparison with log_tau are float32 operations (log_tau is the caller's
// float32 rounding of log(threshold), -inf for a threshold of 0: nothing is below it); a masked action's value is
// q - FLT_MAX as the reference forms it, an allowed one's is q - FLT_MAX * 0 = q.  The first maximum wins; lanes at or beyond
// A (the padding columns) are never candidates.  Every lane returns the action.
__device__ __forceinline__ int masked_argmax(float q, float lg, int lane, int A, float log_tau) {
    const float mx = wave_max(lane < A ? lg : -INFINITY);
    float v = -INFINITY;
    int best = A;
    if (lane < A) {
        const float ratio = lg - mx;
        v = q - FLT_MAX * (ratio < log_tau ? 1.f : 0.f);
        best = lane;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int ob = __shfl_xor(best, off, 64);
        if (ov > v || (ov == v && ob < best)) { v = ov; best = ob; }
    }
    return best < A ? best : 0;         // (every value NaN: action 0)
}

// ---- head: one wave per sample.  qo / io: the two head outputs, `pitch` floats per row.
__global__ __launch_bounds__(256) void bcq_head_kernel(const float* __restrict__ qo, const float* __restrict__ io, int64_t B, int A,
                                                       int pitch, float log_tau, float* __restrict__ q_out,
                                                       float* __restrict__ logits_out, int64_t* __restrict__ act_out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float q = 0.f, lg = 0.f;
    if (lane < A) {
        q = qo[b * pitch + lane];
        lg = io[b * pitch + lane];
        if (q_out) q_out[b * A + lane] = q;
        if (logits_out) logits_out[b * A + lane] = lg;
    }
    const int act = masked_argmax(q, lg, lane, A, log_tau);
    if (act_out && lane == 0) act_out[b] = act;
}

// ---- target (discrete_bcq.py:228-234): the live pair's masked argmax, then out[b] = q_old[b, act]
__global__ __launch_bounds__(256) void bcq_target_kernel(const float* __restrict__ qo, const float* __restrict__ io,
                                                         const float* __restrict__ q_old, int64_t B, int A, int pitch,
                                                         float log_tau, float* __restrict__ out, int64_t* __restrict__ act_out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float q = 0.f, lg = 0.f;
    if (lane < A) {
        q = qo[b * pitch + lane];
        lg = io[b * pitch + lane];
    }
    const int act = masked_argmax(q, lg, lane, A, log_tau);          // in [0, A)
    if (lane == 0) {
        out[b] = q_old[b * pitch + act];
        if (act_out) act_out[b] = act;
    }
}

// ---- loss (discrete_bcq.py:244-252), one wave per sample.  q / lg: [B, pitch]; per-sample terms ps[4, B]:
//   ps[0] = delta = Q[b, a_b] - returns[b]        ps[1] = smooth_l1(delta) (beta = 1)
//   ps[2] = -log_softmax(logits[b])[a_b]          ps[3] = sum_a logits[b, a]^2
// and the head gradients of  loss = mean_b ps[1] + mean_b ps[2] + theta * sum_b ps[3] / (B A), all ld columns of both rows
// written (the padding columns: exact zeros):
//   dq[b, a] = clamp(delta, -1, 1) / B at a = a_b, else 0
//   dl[b, a] = (softmax[b, a] - 1{a = a_b}) / B + 2 theta logits[b, a] / (B A)        (theta == 0: the first term alone)
// An action index outside [0, A) is clamped into it.
__global__ __launch_bounds__(256) void bcq_loss_kernel(const float* __restrict__ q, const float* __restrict__ lg,
                                                       const int64_t* __restrict__ act, const float* __restrict__ ret, int64_t B,
                                                       int A, int pitch, int ld, float theta, float* __restrict__ dq,
                                                       float* __restrict__ dl, float* __restrict__ ps) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int a = (int)min((int64_t)(A - 1), max((int64_t)0, act[b]));
    const bool live = lane < A;
    const float l = live ? lg[b * pitch + lane] : 0.f;
    const float mx = wave_max(live ? l : -INFINITY);
    const float z = l - mx;
    const float e = live ? expf(z) : 0.f;
    const float se = wave_sum(e);
    const float lse = logf(se);
    const float sq = wave_sum(l * l);
    const float za = __shfl(z, a, 64);
    const float delta = q[b * pitch + a] - ret[b];
    const float ad = fabsf(delta);
    const float fb = (float)B;
    if (lane < ld) {
        float gq = 0.f, gl = 0.f;
        if (live) {
            if (lane == a) gq = fminf(fmaxf(delta, -1.f), 1.f) / fb;
            gl = (e / se - (lane == a ? 1.f : 0.f)) / fb;
            if (theta != 0.f) gl += 2.f * theta * l / (fb * (float)A);
        }
        dq[b * ld + lane] = gq;
        dl[b * ld + lane] = gl;
    }
    if (lane == 0) {
        ps[b] = delta;
        ps[B + b] = ad < 1.f ? 0.5f * delta * delta : ad - 0.5f;
        ps[2 * B + b] = lse - za;
        ps[3 * B + b] = sq;
    }
}

// out4 = [loss, q_loss, i_loss, reg_loss]: q_loss = mean_b ps[1], i_loss = mean_b ps[2], reg_loss = sum_b ps[3] / (B A), each
// in one fixed order; loss = (q_loss + i_loss) + theta * reg_loss in float32, as the reference adds them
__global__ __launch_bounds__(1024) void bcq_mean_kernel(const float* __restrict__ ps, int64_t B, int A, float theta,
                                                        float* __restrict__ out4) {
    __shared__ float red[3][1024];
    float s[3] = {0.f, 0.f, 0.f};
    for (int64_t b = threadIdx.x; b < B; b += 1024)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += ps[(k + 1) * B + b];
#pragma unroll
    for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
#pragma unroll
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float ql = red[0][0] / (float)B, il = red[1][0] / (float)B, rl = red[2][0] / ((float)B * (float)A);
        out4[0] = (ql + il) + theta * rl;
        out4[1] = ql;
        out4[2] = il;
        out4[3] = rl;
    }
}

int check_scalars(const char* who, double log_tau, double penalty) {
    TS_REQUIRE(!std::isnan(log_tau) && log_tau <= 0.0, TS_ERR_INVALID_ARG,
               "%s: log_tau = log(unlikely_action_threshold) must be <= 0 (-inf for a threshold of 0)", who);
    TS_REQUIRE(std::isfinite(penalty) && penalty >= 0.0, TS_ERR_INVALID_ARG,
               "%s: imitation_logits_penalty must be finite and >= 0", who);
    return TS_OK;
}

}  // namespace

extern "C" {

int64_t ts_bcq_param_count(int64_t c, int64_t h, int64_t w, int64_t n_act) {
    BNet n;
    if (make_bnet(1, c, h, w, n_act, &n) != TS_OK) return -1;
    return n.off[7];
}

int ts_bcq_layout(int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t* h_out10) {
    BNet n;
    if (int rc = make_bnet(1, c, h, w, n_act, &n)) return rc;
    TS_REQUIRE(h_out10, TS_ERR_INVALID_ARG, "ts_bcq_layout: NULL output");
    h_out10[0] = n.F; h_out10[1] = n.ld; h_out10[2] = n.off[7];
    for (int i = 0; i < 7; ++i) h_out10[3 + i] = n.off[i];
    return TS_OK;
}

int ts_bcq_head(const float* q, const float* logits, int64_t B, int64_t n_act, double log_tau, int64_t* act_out,
                ts_stream_t stream) {
    TS_REQUIRE(B >= 0 && B < (int64_t(1) << 31), TS_ERR_INVALID_ARG, "ts_bcq_head: bad batch size");
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_INVALID_ARG, "ts_bcq_head: 1 <= n_act <= 64");
    if (int rc = check_scalars("ts_bcq_head", log_tau, 0.0)) return rc;
    if (B == 0) return TS_OK;
    TS_REQUIRE(q && logits && act_out, TS_ERR_INVALID_ARG, "ts_bcq_head: NULL argument");
    hipLaunchKernelGGL(bcq_head_kernel, dim3(wave_blocks(B)), dim3(256), 0, ts::as_stream(stream), q, logits, B, (int)n_act,
                       (int)n_act, (float)log_tau, (float*)nullptr, (float*)nullptr, act_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_bcq_target(const float* q, const float* logits, const float* q_old, int64_t B, int64_t n_act, double log_tau,
                  float* out, int64_t* act_out, ts_stream_t stream) {
    TS_REQUIRE(B >= 0 && B < (int64_t(1) << 31), TS_ERR_INVALID_ARG, "ts_bcq_target: bad batch size");
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_INVALID_ARG, "ts_bcq_target: 1 <= n_act <= 64");
    if (int rc = check_scalars("ts_bcq_target", log_tau, 0.0)) return rc;
    if (B == 0) return TS_OK;
    TS_REQUIRE(q && logits && q_old && out, TS_ERR_INVALID_ARG, "ts_bcq_target: NULL argument");
    hipLaunchKernelGGL(bcq_target_kernel, dim3(wave_blocks(B)), dim3(256), 0, ts::as_stream(stream), q, logits, q_old, B,
                       (int)n_act, (int)n_act, (float)log_tau, out, act_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_bcq_loss(const float* q, const float* logits, const int64_t* act, const float* returns, int64_t B, int64_t n_act,
                double imitation_logits_penalty, float* dq_out, float* dlogits_out, float* terms_out, float* loss4_out,
                ts_stream_t stream) {
    TS_REQUIRE(B >= 1 && B < (1 << 24), TS_ERR_INVALID_ARG, "ts_bcq_loss: batch size must be in [1, 2^24)");
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_INVALID_ARG, "ts_bcq_loss: 1 <= n_act <= 64");
    if (int rc = check_scalars("ts_bcq_loss", 0.0, imitation_logits_penalty)) return rc;
    TS_REQUIRE(q && logits && act && returns && dq_out && dlogits_out && terms_out && loss4_out, TS_ERR_INVALID_ARG,
               "ts_bcq_loss: NULL argument");
    const int A = (int)n_act, ld = (A + 31) / 32 * 32;
    const float theta = (float)imitation_logits_penalty;
    hipStream_t s = ts::as_stream(stream);
    hipLaunchKernelGGL(bcq_loss_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, q, logits, act, returns, B, A, A, ld, theta, dq_out,
                       dlogits_out, terms_out);
    hipLaunchKernelGGL(bcq_mean_kernel, dim3(1), dim3(1024), 0, s, terms_out, B, A, theta, loss4_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_bcq_forward(ts_workspace* ws, const float* params, int64_t c, int64_t h, int64_t w, int64_t n_act, const void* obs_nhwc,
                   int obs_u8, int64_t B, double log_tau, float* q_out, float* logits_out, int64_t* act_out,
                   ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_bcq_forward: workspace is NULL");
    TS_REQUIRE(B >= 0, TS_ERR_INVALID_ARG, "ts_bcq_forward: negative batch");
    BNet n;
    if (int rc = make_bnet(std::max<int64_t>(B, 1), c, h, w, n_act, &n)) return rc;
    if (int rc = check_scalars("ts_bcq_forward", log_tau, 0.0)) return rc;
    if (B == 0) return TS_OK;
    TS_REQUIRE(params && obs_nhwc, TS_ERR_INVALID_ARG, "ts_bcq_forward: NULL argument");
    if (int rc = ts::ws_reserve(ws, acts_bytes(n, true))) return rc;
    BActs a;
    carve_acts(n, true, static_cast<char*>(ws->base), &a);
    hipStream_t s = ts::as_stream(stream), sa, sb;
    if (int rc = ts::side_streams(ws, s, &sa, &sb)) return rc;
    if (int rc = net_forward(s, sb, ws, n, params, obs_nhwc, obs_u8 != 0, true, a, 10)) return rc;
    hipLaunchKernelGGL(bcq_head_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, a.oq, a.oi, B, n.n_act, n.ld, (float)log_tau, q_out,
                       logits_out, act_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_bcq_target_q(ts_workspace* ws, const float* params, const float* params_old, int64_t c, int64_t h, int64_t w,
                    int64_t n_act, const void* obs_next_nhwc, int obs_u8, int64_t B, double log_tau, float* out,
                    int64_t* act_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_bcq_target_q: workspace is NULL");
    TS_REQUIRE(B >= 0, TS_ERR_INVALID_ARG, "ts_bcq_target_q: negative batch");
    BNet n;
    if (int rc = make_bnet(std::max<int64_t>(B, 1), c, h, w, n_act, &n)) return rc;
    if (int rc = check_scalars("ts_bcq_target_q", log_tau, 0.0)) return rc;
    if (B == 0) return TS_OK;
    TS_REQUIRE(params && params_old && obs_next_nhwc && out, TS_ERR_INVALID_ARG, "ts_bcq_target_q: NULL argument");
    const size_t live = acts_bytes(n, true);
    if (int rc = ts::ws_reserve(ws, live + acts_bytes(n, false))) return rc;
    BActs a, o;
    char* p = carve_acts(n, true, static_cast<char*>(ws->base), &a);
    carve_acts(n, false, p, &o);
    hipStream_t s = ts::as_stream(stream), sa, sb;
    if (int rc = ts::side_streams(ws, s, &sa, &sb)) return rc;
    // the lagged trunk + Q head run beside the live pass (the imitator of the lagged vector is never evaluated)
    if (int rc = ts::stream_wait(ws, s, sa, 12)) return rc;
    if (int rc = net_forward(sa, sa, ws, n, params_old, obs_next_nhwc, obs_u8 != 0, false, o, 0)) return rc;
    if (int rc = net_forward(s, sb, ws, n, params, obs_next_nhwc, obs_u8 != 0, true, a, 10)) return rc;
    if (int rc = ts::stream_wait(ws, sa, s, 13)) return rc;
    hipLaunchKernelGGL(bcq_target_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, a.oq, a.oi, o.oq, B, n.n_act, n.ld, (float)log_tau,
                       out, act_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_bcq_update(ts_workspace* ws, float* params, float* adam_m, float* adam_v, int64_t adam_step, int64_t c, int64_t h,
                  int64_t w, int64_t n_act, const void* obs_nhwc, int obs_u8, const int64_t* act, const float* returns,
                  int64_t B, const ts_dqn_hparams* hp, double imitation_logits_penalty, float* loss4_out, float* grad_out,
                  ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_bcq_update: workspace is NULL");
    TS_REQUIRE(B >= 1 && adam_step >= 1, TS_ERR_INVALID_ARG, "ts_bcq_update: bad batch size / step");
    BNet n;
    if (int rc = make_bnet(B, c, h, w, n_act, &n)) return rc;
    if (int rc = check_scalars("ts_bcq_update", 0.0, imitation_logits_penalty)) return rc;
    TS_REQUIRE(params && adam_m && adam_v && obs_nhwc && act && returns && hp && loss4_out, TS_ERR_INVALID_ARG,
               "ts_bcq_update: NULL argument");
    TS_REQUIRE(hp->lr >= 0.0 || grad_out, TS_ERR_INVALID_ARG, "ts_bcq_update: a gradient-only call (lr < 0) needs grad_out");
    hipStream_t s = ts::as_stream(stream);
    const float theta = (float)imitation_logits_penalty;

    // workspace: activations | the backward pass's buffers (ts_twin.h) | per-sample loss terms | norm partials
    if (int rc = ts::ws_reserve(ws, acts_bytes(n, true) + back_bytes(n) + al(4 * 4 * (size_t)B) + 4096)) return rc;
    BActs a;
    BBack k;
    char* p = carve_back(n, carve_acts(n, true, static_cast<char*>(ws->base), &a), &k);
    float* ps = reinterpret_cast<float*>(p);
    float* norm_part = reinterpret_cast<float*>(p + al(4 * 4 * (size_t)B));
    float* const* dy = k.dy;
    float* grad = grad_out ? grad_out : k.grad;

    hipStream_t sv, sw;
    if (int rc = ts::side_streams(ws, s, &sv, &sw)) return rc;
    if (int rc = net_forward(s, sw, ws, n, params, obs_nhwc, obs_u8 != 0, true, a, 10)) return rc;
    hipLaunchKernelGGL(bcq_loss_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, a.oq, a.oi, act, returns, B, n.n_act, n.ld, n.ld, theta,
                       dy[4], dy[6], ps);
    hipLaunchKernelGGL(bcq_mean_kernel, dim3(1), dim3(1024), 0, s, ps, B, n.n_act, theta, loss4_out);
    TS_LAUNCH_CHECK();
    if (int rc = ts::record_td(ws, s)) return rc;        // the four losses are written: ts_dqn_wait_td

    if (int rc = twin_backward(s, sv, sw, ws, n, params, obs_nhwc, obs_u8 != 0, a, k, grad)) return rc;
    if (hp->lr < 0.0) return TS_OK;
    return ts::adam_step(s, params, adam_m, adam_v, grad, n.off[7], adam_step, hp->lr, hp->beta1, hp->beta2, hp->adam_eps,
                         hp->max_grad_norm, norm_part);
}

}  // extern "C"
