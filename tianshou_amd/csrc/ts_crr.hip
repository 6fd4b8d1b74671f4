// ts_crr.hip -- discrete critic-regularized regression (DiscreteCRR, arXiv:2006.15134) on the Atari trunk for gfx950.
//
// Replaces, on device-resident NHWC observations:
//   DiscreteActor.forward / DiscreteCritic.forward   tianshou/utils/net/discrete.py (both on ONE DQNet(features_only=True),
//                                                    hidden_sizes = [512]; examples/offline/atari_crr.py)
//   DiscreteCRR._update_with_batch                   tianshou/algorithm/imitation/discrete_crr.py:125-167 (expected-value
//                                                    target of the lagged pair, advantage-weighted actor loss whose weight
//                                                    is NOT detached, critic loss, CQL term)
//   Optimizer.step                                   algorithm_base.py:484-500 (clip_grad_norm_ + ONE Adam over all 14 tensors)
//
// The network, its flat layout and the backward pass are the twin-head code of ts_twin.h, shared with ts_bcq.hip: the first
// head (BCQ's Q head) is the critic, the second (BCQ's imitator) is the actor; ts_bcq_param_count / ts_bcq_layout serve both.
// This file adds CRR's own mathematics as per-sample kernels (one wave per sample) and the orchestration.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "ts_common.h"
#include "ts_conv.h"

#pragma clang fp contract(off)

#include "ts_twin.h"

namespace ts {
int adam_step(hipStream_t s, float* params, float* m, float* v, const float* grad, int64_t n, int64_t step,
              double lr, double beta1, double beta2, double eps, double max_grad_norm, float* norm_scratch);
}

namespace {

enum { MODE_EXP = 0, MODE_BINARY = 1, MODE_ALL = 2 };

// sum_j softmax(lg)_j * q_j of one sample, one wave: lane j < A holds q and lg (max-subtracted softmax, butterfly sums; every
// lane returns the value).  discrete_crr.py:136-140: Categorical(logits).probs times the critic's values.
__device__ __forceinline__ float expected_q(float q, float lg, bool live) {
    const float mx = wave_max(live ? lg : -INFINITY);
    const float e = live ? expf(lg - mx) : 0.f;
    const float se = wave_sum(e);
    return wave_sum(live ? (e / se) * q : 0.f);
}

// ---- target (discrete_crr.py:135-142): out[b] = rew[b] + gamma * (done[b] > 0 ? 0 : sum_j softmax(l_old[b])_j q_old[b, j])
__global__ __launch_bounds__(256) void crr_target_kernel(const float* __restrict__ q_old, const float* __restrict__ l_old,
                                                         const float* __restrict__ rew, const uint8_t* __restrict__ done,
                                                         int64_t B, int A, int pitch, float gamma, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bool live = lane < A;
    const float q = live ? q_old[b * pitch + lane] : 0.f, lg = live ? l_old[b * pitch + lane] : 0.f;
    float ev = expected_q(q, lg, live);
    if (done[b] > 0) ev = 0.f;
    if (lane == 0) out[b] = rew[b] + gamma * ev;
}

// ---- loss (discrete_crr.py:131-158), one wave per sample, in three launches: the per-sample terms, their batch means, the
// head gradients.  q / lg: [B, pitch], the critic's values and the actor's logits on obs.  With a = act[b] (clamped into
// [0, A)), pi = softmax(lg), nll = logsumexp(lg) - lg[a], qa = q[a], V = sum_j pi_j q_j, adv = qa - V, delta = qa - y:
//   exp:    e = exp(adv / beta), coef = clamp(e, 0, U)          binary: coef = 1{adv > 0}          all: coef = 1
// The reference multiplies -log_prob(act), a [B], by the weight, a [B, 1], and takes the mean of the [B, B] product: its actor
// loss is  mean_i nll_i * mean_j coef_j  (not mean_b nll_b coef_b), and so is this one.  Its CQL mean runs over the same kind
// of broadcast, logsumexp(q) [B] minus qa [B, 1]; that one equals the per-sample mean_b (lse_b - qa_b) computed here, in value
// and gradient up to rounding.
//
// crr_terms_kernel: the target y[b] is read from `target`, or (q_old != nullptr: the update path, one launch less) formed
// here from the lagged pair as crr_target_kernel forms it and written to target_out.  Per-sample terms
// ps[6, B] = {delta, 0.5 delta^2, nll, coef, logsumexp(q) - qa, adv}.
__global__ __launch_bounds__(256) void crr_terms_kernel(const float* __restrict__ q, const float* __restrict__ lg,
                                                        const int64_t* __restrict__ act, const float* __restrict__ target,
                                                        const float* __restrict__ q_old, const float* __restrict__ l_old,
                                                        const float* __restrict__ rew, const uint8_t* __restrict__ done,
                                                        float gamma, float* __restrict__ target_out, int64_t B, int A, int pitch,
                                                        int mode, float beta, float U, float* __restrict__ ps) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int a = (int)min((int64_t)(A - 1), max((int64_t)0, act[b]));
    const bool live = lane < A;
    float y;
    if (q_old) {
        float ev = expected_q(live ? q_old[b * pitch + lane] : 0.f, live ? l_old[b * pitch + lane] : 0.f, live);
        if (done[b] > 0) ev = 0.f;
        y = rew[b] + gamma * ev;
        if (lane == 0) target_out[b] = y;
    } else {
        y = target[b];
    }
    const float l = live ? lg[b * pitch + lane] : 0.f;
    const float qv = live ? q[b * pitch + lane] : 0.f;
    // the actor: pi and nll = -(l[a] - logsumexp(l)), in Categorical's order
    const float mxl = wave_max(live ? l : -INFINITY);
    const float el = live ? expf(l - mxl) : 0.f;
    const float sel = wave_sum(el);
    const float nll = -(__shfl(l, a, 64) - (mxl + logf(sel)));
    // the critic: qa, V, adv and the log-sum-exp of q
    const float qa = __shfl(qv, a, 64);
    const float adv = qa - wave_sum(live ? (el / sel) * qv : 0.f);
    const float mxq = wave_max(live ? qv : -INFINITY);
    const float lseq = mxq + logf(wave_sum(live ? expf(qv - mxq) : 0.f));
    const float delta = qa - y;
    float coef = 1.f;
    if (mode == MODE_EXP) {
        const float e = expf(adv / beta);
        coef = e < 0.f ? 0.f : (e > U ? U : e);                 // (a NaN stays a NaN, as in torch.clamp)
    } else if (mode == MODE_BINARY) {
        coef = adv > 0.f ? 1.f : 0.f;
    }
    if (lane == 0) {
        ps[b] = delta;
        ps[B + b] = 0.5f * delta * delta;
        ps[2 * B + b] = nll;
        ps[3 * B + b] = coef;
        ps[4 * B + b] = lseq - qa;
        ps[5 * B + b] = adv;
    }
}

// out6 = [loss, actor_loss, critic_loss, cql_loss, mean_b nll, mean_b coef]: critic_loss = mean_b ps[1], actor_loss =
// mean_b ps[2] * mean_b ps[3], cql_loss = mean_b ps[4], each mean in one fixed order (that of bcq_mean_kernel);
// loss = (actor_loss + critic_loss) + w * cql_loss in float32, as the reference adds them
__global__ __launch_bounds__(1024) void crr_mean_kernel(const float* __restrict__ ps, int64_t B, float w, float* __restrict__ out6) {
    __shared__ float red[4][1024];
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t b = threadIdx.x; b < B; b += 1024)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += ps[(k + 1) * B + b];
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float fb = (float)B;
        const float cl = red[0][0] / fb, nbar = red[1][0] / fb, cbar = red[2][0] / fb, ql = red[3][0] / fb;
        const float al_ = nbar * cbar;
        out6[0] = (al_ + cl) + w * ql;
        out6[1] = al_;
        out6[2] = cl;
        out6[3] = ql;
        out6[4] = nbar;
        out6[5] = cbar;
    }
}

// crr_grad_kernel: the head gradients of loss = nbar * cbar + mean_b ps[1] + w * mean_b ps[4], with nbar = mean_b nll and
// cbar = mean_b coef read from out6.  In "exp" mode the weight is NOT detached (the reference does not detach it): with
// g = nbar * e / beta * 1{e <= U} (torch's clamp passes the gradient at equality; where e overflows to inf under a finite U,
// g = 0 * inf = NaN as in the reference's autograd), g = 0 in the other modes,
//   dq[b, j] = (delta 1{j=a} + g (1{j=a} - pi_j) + w (softmax(q)_j - 1{j=a})) / B
//   dl[b, j] = (cbar (pi_j - 1{j=a}) - g pi_j (q_j - V)) / B
// all ld columns of both rows written (the padding columns: exact zeros).  delta and adv come from ps, so e is the very
// float32 value the terms kernel clamped.
__global__ __launch_bounds__(256) void crr_grad_kernel(const float* __restrict__ q, const float* __restrict__ lg,
                                                       const int64_t* __restrict__ act, const float* __restrict__ ps,
                                                       const float* __restrict__ out6, int64_t B, int A, int pitch, int ld,
                                                       int mode, float beta, float U, float w, float* __restrict__ dq,
                                                       float* __restrict__ dl) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int a = (int)min((int64_t)(A - 1), max((int64_t)0, act[b]));
    const bool live = lane < A;
    const float l = live ? lg[b * pitch + lane] : 0.f;
    const float qv = live ? q[b * pitch + lane] : 0.f;
    const float mxl = wave_max(live ? l : -INFINITY);
    const float el = live ? expf(l - mxl) : 0.f;
    const float pi = el / wave_sum(el);
    const float V = wave_sum(live ? pi * qv : 0.f);
    const float mxq = wave_max(live ? qv : -INFINITY);
    const float eq = live ? expf(qv - mxq) : 0.f;
    const float seq = wave_sum(eq);
    const float delta = ps[b], adv = ps[5 * B + b];
    const float nbar = out6[4], cbar = out6[5];
    float g = 0.f;
    if (mode == MODE_EXP) {
        const float e = expf(adv / beta);
        g = (e <= U ? nbar : 0.f) * e / beta;
    }
    const float fb = (float)B;
    if (lane < ld) {
        float gq = 0.f, gl = 0.f;
        if (live) {
            const float hot = lane == a ? 1.f : 0.f;
            gq = delta * hot + w * (eq / seq - hot);
            gl = cbar * (pi - hot);
            if (mode == MODE_EXP) {
                gq += g * (hot - pi);
                gl -= g * pi * (qv - V);
            }
            gq /= fb;
            gl /= fb;
        }
        dq[b * ld + lane] = gq;
        dl[b * ld + lane] = gl;
    }
}

int check_scalars(const char* who, int64_t n_act, int64_t mode, double beta, double U, double w, double gamma) {
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_INVALID_ARG, "%s: 1 <= n_act <= 64", who);
    TS_REQUIRE(mode == MODE_EXP || mode == MODE_BINARY || mode == MODE_ALL, TS_ERR_INVALID_ARG,
               "%s: policy_improvement_mode must be 0 (exp), 1 (binary) or 2 (all)", who);
    TS_REQUIRE(std::isfinite(beta) && beta != 0.0, TS_ERR_INVALID_ARG, "%s: beta must be finite and nonzero", who);
    TS_REQUIRE(!std::isnan(U), TS_ERR_INVALID_ARG, "%s: ratio_upper_bound must not be NaN", who);
    TS_REQUIRE(std::isfinite(w) && std::isfinite(gamma), TS_ERR_INVALID_ARG, "%s: min_q_weight and gamma must be finite", who);
    return TS_OK;
}

}  // namespace

extern "C" {

int ts_crr_target(const float* q_old, const float* logits_old, const float* rew, const uint8_t* done, int64_t B, int64_t n_act,
                  double gamma, float* out, ts_stream_t stream) {
    TS_REQUIRE(B >= 0 && B < (int64_t(1) << 31), TS_ERR_INVALID_ARG, "ts_crr_target: bad batch size");
    if (int rc = check_scalars("ts_crr_target", n_act, MODE_ALL, 1.0, 0.0, 0.0, gamma)) return rc;
    TS_REQUIRE(q_old && logits_old && rew && done && out, TS_ERR_INVALID_ARG, "ts_crr_target: NULL argument");
    if (B == 0) return TS_OK;
    hipLaunchKernelGGL(crr_target_kernel, dim3(wave_blocks(B)), dim3(256), 0, ts::as_stream(stream), q_old, logits_old, rew, done,
                       B, (int)n_act, (int)n_act, (float)gamma, out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_crr_loss(const float* q, const float* logits, const int64_t* act, const float* target, int64_t B, int64_t n_act,
                int64_t mode, double beta, double ratio_upper_bound, double min_q_weight, float* dq_out, float* dlogits_out,
                float* terms_out, float* loss6_out, ts_stream_t stream) {
    TS_REQUIRE(B >= 1 && B < (1 << 24), TS_ERR_INVALID_ARG, "ts_crr_loss: batch size must be in [1, 2^24)");
    if (int rc = check_scalars("ts_crr_loss", n_act, mode, beta, ratio_upper_bound, min_q_weight, 0.0)) return rc;
    TS_REQUIRE(q && logits && act && target && dq_out && dlogits_out && terms_out && loss6_out, TS_ERR_INVALID_ARG,
               "ts_crr_loss: NULL argument");
    const int A = (int)n_act, ld = (A + 31) / 32 * 32;
    const float w = (float)min_q_weight;
    hipStream_t s = ts::as_stream(stream);
    const float be = (float)beta, U = (float)ratio_upper_bound;
    hipLaunchKernelGGL(crr_terms_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, q, logits, act, target, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (const uint8_t*)nullptr, 0.f, (float*)nullptr, B, A, A,
                       (int)mode, be, U, terms_out);
    hipLaunchKernelGGL(crr_mean_kernel, dim3(1), dim3(1024), 0, s, terms_out, B, w, loss6_out);
    hipLaunchKernelGGL(crr_grad_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, q, logits, act, terms_out, loss6_out, B, A, A, ld,
                       (int)mode, be, U, w, dq_out, dlogits_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_crr_update(ts_workspace* ws, float* params, const float* params_old, float* adam_m, float* adam_v, int64_t adam_step,
                  int64_t c, int64_t h, int64_t w, int64_t n_act, const void* obs_nhwc, const void* obs_next_nhwc, int obs_u8,
                  const int64_t* act, const float* rew, const uint8_t* done, int64_t B, const ts_dqn_hparams* hp, double gamma,
                  int64_t mode, double beta, double ratio_upper_bound, double min_q_weight, float* loss6_out, float* target_out,
                  float* grad_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_crr_update: workspace is NULL");
    TS_REQUIRE(B >= 1 && adam_step >= 1, TS_ERR_INVALID_ARG, "ts_crr_update: bad batch size / step");
    BNet n;
    if (int rc = make_bnet(B, c, h, w, n_act, &n)) return rc;
    if (int rc = check_scalars("ts_crr_update", n_act, mode, beta, ratio_upper_bound, min_q_weight, gamma)) return rc;
    TS_REQUIRE(params && params_old && adam_m && adam_v && obs_nhwc && obs_next_nhwc && act && rew && done && hp && loss6_out,
               TS_ERR_INVALID_ARG, "ts_crr_update: NULL argument");
    TS_REQUIRE(hp->lr >= 0.0 || grad_out, TS_ERR_INVALID_ARG, "ts_crr_update: a gradient-only call (lr < 0) needs grad_out");
    hipStream_t s = ts::as_stream(stream);

    // workspace: live activations | lagged activations | the backward pass's buffers (ts_twin.h) | per-sample loss terms |
    // targets | norm partials
    const size_t acts = acts_bytes(n, true);
    if (int rc = ts::ws_reserve(ws, 2 * acts + back_bytes(n) + al(4 * 6 * (size_t)B) + al(4 * (size_t)B) + 4096)) return rc;
    BActs a, o;
    BBack k;
    char* p = carve_acts(n, true, static_cast<char*>(ws->base), &a);
    p = carve_back(n, carve_acts(n, true, p, &o), &k);
    float* ps = reinterpret_cast<float*>(p);
    p += al(4 * 6 * (size_t)B);
    float* y = target_out ? target_out : reinterpret_cast<float*>(p);
    float* norm_part = reinterpret_cast<float*>(p + al(4 * (size_t)B));
    float* grad = grad_out ? grad_out : k.grad;

    hipStream_t sv, sw;
    if (int rc = ts::side_streams(ws, s, &sv, &sw)) return rc;
    // the lagged trunk and its two heads (one after the other) on obs_next run on a side stream beside the live pass on obs
    if (int rc = ts::stream_wait(ws, s, sv, 12)) return rc;
    if (int rc = net_forward(sv, sv, ws, n, params_old, obs_next_nhwc, obs_u8 != 0, false, o, 0)) return rc;
    if (int rc = ts::conv_forward(sv, n.l[5], o.c[2], params_old + n.off[5], o.hi, true, o.split, ws)) return rc;
    if (int rc = ts::conv_forward(sv, n.l[6], o.hi, params_old + n.off[6], o.oi, false, o.split, ws)) return rc;
    if (int rc = net_forward(s, sw, ws, n, params, obs_nhwc, obs_u8 != 0, true, a, 10)) return rc;
    if (int rc = ts::stream_wait(ws, sv, s, 13)) return rc;
    const float wq = (float)min_q_weight;
    const float be = (float)beta, U = (float)ratio_upper_bound;
    hipLaunchKernelGGL(crr_terms_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, a.oq, a.oi, act, (const float*)nullptr, o.oq, o.oi,
                       rew, done, (float)gamma, y, B, n.n_act, n.ld, (int)mode, be, U, ps);
    hipLaunchKernelGGL(crr_mean_kernel, dim3(1), dim3(1024), 0, s, ps, B, wq, loss6_out);
    hipLaunchKernelGGL(crr_grad_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, a.oq, a.oi, act, ps, loss6_out, B, n.n_act, n.ld, n.ld,
                       (int)mode, be, U, wq, k.dy[4], k.dy[6]);
    TS_LAUNCH_CHECK();
    if (int rc = ts::record_td(ws, s)) return rc;        // the losses are written: ts_dqn_wait_td

    // the target is complete (the side stream has joined) before anything below writes: params_old == params is legal
    if (int rc = twin_backward(s, sv, sw, ws, n, params, obs_nhwc, obs_u8 != 0, a, k, grad)) return rc;
    if (hp->lr < 0.0) return TS_OK;
    return ts::adam_step(s, params, adam_m, adam_v, grad, n.off[7], adam_step, hp->lr, hp->beta1, hp->beta2, hp->adam_eps,
                         hp->max_grad_norm, norm_part);
}

}  // extern "C"
