// ts_dsac_cnn.hip -- DiscreteSAC (arXiv:1910.07207) on the Atari trunk for gfx950: an actor and two critics on ONE shared
// DQNet(features_only=True, output_dim_added_layer=H), as examples/atari/atari_sac.py builds them.
//
// Replaces, on device-resident NHWC observations:
//   DiscreteActor.forward / DiscreteCritic.forward     tianshou/utils/net/discrete.py (single Linear heads on the shared DQNet)
//   DiscreteSAC._target_q_compute_value                tianshou/algorithm/modelfree/discrete_sac.py:147-155
//   DiscreteSAC._update_with_batch                     discrete_sac.py:157-196: critic 1, critic 2, actor, each with an Adam of
//                                                      its own over trunk + own head -- the shared trunk is stepped THREE times per
//                                                      update, strictly in sequence -- then AutoAlpha.update (sac.py:203-209) and
//                                                      the Polyak step of the lagged critics
//
//   feat[b, :] = relu(fc(relu(conv3(relu(conv2(relu(conv1(obs[b]))))))))      fc: F -> H, F = 64 * OH3 * OW3 in (h, w, c) order
//   logits = feat @ Wa + ba,  q1 = feat @ W1 + b1,  q2 = feat @ W2 + b2         three Linear heads H -> n_act
// Flat parameter layout: conv1 | conv2 | conv3 | fc | actor head | critic-1 head | critic-2 head, each block [K + 1, OC] with
// the bias as last row; the head width ld is n_act rounded up to a multiple of 32 (GEMM tile width; the padding columns are and
// stay exactly zero in parameters, gradients and moments).  Lagged vector: conv1 | conv2 | conv3 | fc | critic-1 head |
// critic-2 head (critic_old and critic2_old each own a trunk copy; both start equal and follow the same live trunk with the
// same tau, so they stay bit-equal and one is kept).  Gradients and Adam moments come in three sets, critic 1, critic 2, actor,
// each trunk | own head.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "ts_common.h"
#include "ts_conv.h"

#pragma clang fp contract(off)

namespace ts {
int adam_step(hipStream_t s, float* params, float* m, float* v, const float* grad, int64_t n, int64_t step,
              double lr, double beta1, double beta2, double eps, double max_grad_norm, float* norm_scratch);
}

namespace {

constexpr int MAX_ACT = 64;

struct DNet {
    ts::ConvGeom l[5];          // conv1, conv2, conv3, fc, one head (the three heads share the geometry)
    int64_t off[8];             // starts of conv1, conv2, conv3, fc, actor head, critic-1 head, critic-2 head and the total
    int64_t T, Hd;              // trunk length (= off[4]) and the length of one head
    int F, H, n_act, ld;
    int64_t B;
};

int make_dnet(const char* who, int64_t B, int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t hidden, DNet* n) {
    TS_REQUIRE(c >= 1 && h >= 1 && w >= 1 && c < (1 << 16) && h < (1 << 16) && w < (1 << 16), TS_ERR_INVALID_ARG,
               "%s: bad observation dimensions", who);
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_INVALID_ARG, "%s: 1 <= n_act <= 64", who);
    TS_REQUIRE(hidden >= 32 && hidden <= 1024 && hidden % 32 == 0, TS_ERR_INVALID_ARG,
               "%s: the added layer's width must be a multiple of 32 in [32, 1024]", who);
    TS_REQUIRE(B >= 1 && B < (1 << 24), TS_ERR_INVALID_ARG, "%s: batch size must be in [1, 2^24)", who);
    static const int oc[3] = {32, 64, 64}, ks[3] = {8, 4, 3}, st[3] = {4, 2, 1};
    int ic = (int)c, ih = (int)h, iw = (int)w;
    for (int i = 0; i < 3; ++i) {
        TS_REQUIRE(ih >= ks[i] && iw >= ks[i], TS_ERR_INVALID_ARG, "%s: observation too small for DQNet", who);
        n->l[i] = ts::ConvGeom{(int)B, ih, iw, ic, ks[i], ks[i], st[i], (ih - ks[i]) / st[i] + 1, (iw - ks[i]) / st[i] + 1, oc[i]};
        ic = oc[i]; ih = n->l[i].OH; iw = n->l[i].OW;
    }
    n->B = B;
    n->F = ic * ih * iw;
    n->H = (int)hidden;
    TS_REQUIRE(B * std::max<int64_t>(n->l[0].OH * n->l[0].OW * 32, std::max(n->F, n->H)) < (int64_t(1) << 31), TS_ERR_INVALID_ARG,
               "%s: batch too large (B * activations of one layer < 2^31)", who);
    n->n_act = (int)n_act;
    n->ld = ((int)n_act + 31) / 32 * 32;
    n->l[3] = ts::ConvGeom{(int)B, 1, 1, n->F, 1, 1, 1, 1, 1, n->H};
    n->l[4] = ts::ConvGeom{(int)B, 1, 1, n->H, 1, 1, 1, 1, 1, n->ld};
    int64_t o = 0;
    for (int i = 0; i < 4; ++i) { n->off[i] = o; o += n->l[i].param_elems(); }
    n->T = o;
    n->Hd = n->l[4].param_elems();
    for (int i = 4; i < 8; ++i) n->off[i] = n->T + (i - 4) * n->Hd;
    return TS_OK;
}

size_t al(size_t x) { return (x + 255) & ~size_t(255); }

size_t split_floats(const DNet& n) {
    size_t s = 4;
    for (int i = 0; i < 5; ++i) {
        const int ns = ts::conv_fwd_splits(n.l[i]);
        if (ns > 1) s = std::max(s, (size_t)ns * n.l[i].out_elems());
    }
    return s;
}

// activations of one trunk pass and up to three head outputs [B, ld]; every head GEMM that may run beside another has its own
// split buffer
struct DActs { float* c[3]; float* feat; float* o[3]; float* split[3]; };

size_t acts_bytes(const DNet& n) {
    size_t s = 3 * al(4 * split_floats(n)) + 3 * al(4 * (size_t)n.l[4].out_elems());
    for (int i = 0; i < 4; ++i) s += al(4 * (size_t)n.l[i].out_elems());
    return s;
}

char* carve_acts(const DNet& n, char* p, DActs* a) {
    auto take = [&](size_t floats) { float* r = reinterpret_cast<float*>(p); p += al(4 * floats); return r; };
    for (int i = 0; i < 3; ++i) a->c[i] = take((size_t)n.l[i].out_elems());
    a->feat = take((size_t)n.l[3].out_elems());
    for (int k = 0; k < 3; ++k) a->o[k] = take((size_t)n.l[4].out_elems());
    for (int k = 0; k < 3; ++k) a->split[k] = take(split_floats(n));
    return p;
}

// what a backward pass needs beside the activations: d (layer outputs) | wgrad slabs, one set per layer (they run side by side)
struct DBack { float* dy[5]; float* slabs[5]; };

size_t back_bytes(const DNet& n) {
    size_t s = 0;
    for (int i = 0; i < 5; ++i)
        s += al(4 * (size_t)n.l[i].out_elems()) + al(4 * (size_t)ts::conv_wgrad_splits(n.l[i]) * n.l[i].param_elems());
    return s;
}

char* carve_back(const DNet& n, char* p, DBack* k) {
    auto take = [&](size_t floats) { float* r = reinterpret_cast<float*>(p); p += al(4 * floats); return r; };
    for (int i = 0; i < 5; ++i) k->dy[i] = take((size_t)n.l[i].out_elems());
    for (int i = 0; i < 5; ++i) k->slabs[i] = take((size_t)ts::conv_wgrad_splits(n.l[i]) * n.l[i].param_elems());
    return p;
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return s;
}

__device__ __forceinline__ float wave_max(float s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = fmaxf(s, __shfl_xor(s, off, 64));
    return s;
}

unsigned wave_blocks(int64_t B) { return (unsigned)ts::ceil_div(B, 4); }

// Categorical(logits = lg) of one sample, one wave: lane j < A holds lg.  lp = lg - logsumexp(lg) (the normalised logits,
// floored at the most negative float as Categorical.entropy floors them), p = softmax (max-subtracted), H = -sum_j p_j lp_j.
struct Cat { float p, lp, H; };

__device__ __forceinline__ Cat categorical(float lg, bool live) {
    const float mx = wave_max(live ? lg : -INFINITY);
    const float e = live ? expf(lg - mx) : 0.f;
    const float se = wave_sum(e);
    Cat c;
    c.p = e / se;
    c.lp = live ? fmaxf(lg - (mx + logf(se)), -FLT_MAX) : 0.f;
    c.H = -wave_sum(live ? c.p * c.lp : 0.f);
    return c;
}

// ---- target (discrete_sac.py:147-155): out[b] = sum_j p_j min(q1_old[b, j], q2_old[b, j]) + alpha H(p).  alpha is read from
// log_alpha on the device when that is given (auto-tuned), else the scalar
__global__ __launch_bounds__(256) void dsacc_target_kernel(const float* __restrict__ lg, const float* __restrict__ q1,
                                                           const float* __restrict__ q2, const float* __restrict__ log_alpha,
                                                           float fixed_alpha, int64_t B, int A, int pitch, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bool live = lane < A;
    const float alpha = log_alpha ? expf(*log_alpha) : fixed_alpha;
    const Cat c = categorical(live ? lg[b * pitch + lane] : 0.f, live);
    const float q = live ? fminf(q1[b * pitch + lane], q2[b * pitch + lane]) : 0.f;
    const float sq = wave_sum(live ? c.p * q : 0.f);
    if (lane == 0) out[b] = sq + alpha * c.H;
}

// ---- critic (discrete_sac.py:163-174): td = q[b, act[b]] - y[b]; term[b] = td^2 w_b (w_b = 1 without weights);
// dq[b, j] = 2 w_b td / B at j = act[b] and zero elsewhere, all ld columns written.  With td_prev (the other critic's td) the
// new batch.weight (td_prev + td) / 2 is written too.
__global__ __launch_bounds__(256) void dsacc_critic_kernel(const float* __restrict__ q, const int64_t* __restrict__ act,
                                                           const float* __restrict__ y, const float* __restrict__ weight,
                                                           const float* __restrict__ td_prev, int64_t B, int A, int pitch, int ld,
                                                           float* __restrict__ dq, float* __restrict__ td_out,
                                                           float* __restrict__ term, float* __restrict__ weight_out) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const int a = (int)min((int64_t)(A - 1), max((int64_t)0, act[b]));
    const float qv = lane < A ? q[b * pitch + lane] : 0.f;
    const float td = __shfl(qv, a, 64) - y[b];
    const float w = weight ? weight[b] : 1.f;
    if (lane < ld) dq[b * ld + lane] = lane == a ? 2.f * w * td / (float)B : 0.f;
    if (lane == 0) {
        td_out[b] = td;
        term[b] = td * td * w;
        if (weight_out) weight_out[b] = (td_prev[b] + td) / 2.f;
    }
}

// ---- actor (discrete_sac.py:177-184): q = min(q1, q2) without gradient, f_b = alpha H_b + sum_j p_j q_j, loss = -mean_b f_b;
//   d f / d logit_k = p_k (q_k - sum_j p_j q_j) - alpha p_k (lp_k + H)
// dl[b, :] = -that / B over all ld columns (the padding: exact zeros), ent[b] = H_b, f[b] = f_b
__global__ __launch_bounds__(256) void dsacc_actor_kernel(const float* __restrict__ lg, const float* __restrict__ q1,
                                                          const float* __restrict__ q2, const float* __restrict__ log_alpha,
                                                          float fixed_alpha, int64_t B, int A, int pitch, int ld,
                                                          float* __restrict__ dl, float* __restrict__ ent, float* __restrict__ f) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bool live = lane < A;
    const float alpha = log_alpha ? expf(*log_alpha) : fixed_alpha;
    const Cat c = categorical(live ? lg[b * pitch + lane] : 0.f, live);
    const float q = live ? fminf(q1[b * pitch + lane], q2[b * pitch + lane]) : 0.f;
    const float sq = wave_sum(live ? c.p * q : 0.f);
    if (lane < ld) dl[b * ld + lane] = live ? -((c.p * (q - sq) - alpha * c.p * (c.lp + c.H)) / (float)B) : 0.f;
    if (lane == 0) {
        ent[b] = c.H;
        f[b] = alpha * c.H + sq;
    }
}

// sum of x[0 .. B) in one fixed order (strided partial sums, then a tree over the 1024 threads): reruns are bit-identical
__device__ __forceinline__ float block_sum_1024(const float* __restrict__ x, int64_t B, float* red) {
    float s = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += 1024) s += x[b];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 512; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    return red[0];
}

// *out = sign * mean_b x[b]
__global__ __launch_bounds__(1024) void dsacc_mean_kernel(const float* __restrict__ x, int64_t B, float sign, float* __restrict__ out) {
    __shared__ float red[1024];
    const float tot = block_sum_1024(x, B, red);
    if (threadIdx.x == 0) *out = sign * (tot / (float)B);
}

// AutoAlpha.update (sac.py:203-209) on the per-sample entropies: alpha_loss = -mean(log_alpha (target_entropy - H)) = -(log_alpha
// mean_def) and one torch.optim.Adam step on the scalar (gradient -mean_def), in the float operations of the SAC engine's alpha
// step.  Without log_alpha (a fixed alpha): alpha_out = the scalar, alpha_loss = 0.  step == false: the two outputs only.
struct AlphaStep { float lr_step, beta2, bc2_sqrt, eps, omb1, omb2; };

__global__ __launch_bounds__(1024) void dsacc_alpha_kernel(const float* __restrict__ ent, int64_t B, float target_entropy,
                                                           float* __restrict__ log_alpha, float* __restrict__ am,
                                                           float* __restrict__ av, AlphaStep a, float fixed_alpha, int step,
                                                           float* __restrict__ alpha_loss, float* __restrict__ alpha_out) {
    __shared__ float red[1024];
    const float tot = block_sum_1024(ent, B, red);
    if (threadIdx.x != 0) return;
    if (!log_alpha) { *alpha_out = fixed_alpha; *alpha_loss = 0.f; return; }
    const float mean_def = target_entropy - tot / (float)B;
    const float la = *log_alpha;
    *alpha_loss = -(la * mean_def);
    if (!step) { *alpha_out = expf(la); return; }
    const float g = -mean_def;
    float m = *am, v = *av;
    m = m + (g - m) * a.omb1;
    v = v * a.beta2 + a.omb2 * g * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    const float nla = la + (-a.lr_step * m) / denom;
    *log_alpha = nla; *am = m; *av = v;
    *alpha_out = expf(nla);
}

// out[b, 0 .. A) = in[b, 0 .. A) of rows ld wide
__global__ __launch_bounds__(256) void dsacc_unpad_kernel(const float* __restrict__ in, int64_t n, int A, int ld, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = in[(i / A) * ld + (i % A)];
}

// the trunk of one pass on `s`: conv1 .. conv3 and the added layer, every one with its ReLU
int trunk_forward(hipStream_t s, ts_workspace* ws, const DNet& n, const float* trunk, const void* obs, bool obs_u8, const DActs& a) {
    const float* x = static_cast<const float*>(obs);
    for (int i = 0; i < 4; ++i) {
        float* y = i < 3 ? a.c[i] : a.feat;
        if (int rc = ts::conv_forward(s, n.l[i], x, trunk + n.off[i], y, true, a.split[0], ws, i == 0 && obs_u8)) return rc;
        x = y;
    }
    return TS_OK;
}

// head k of the activations: o[k] = feat @ head (no activation), with split buffer k
int head_forward(hipStream_t s, ts_workspace* ws, const DNet& n, const float* head, const DActs& a, int k) {
    return ts::conv_forward(s, n.l[4], a.feat, head, a.o[k], false, a.split[k], ws);
}

// The backward pass from k.dy[4] (the gradient at one head's output, [B, ld], written on `s`) through that head and the trunk:
// gtrunk[T] and ghead[Hd].  ts::chain_backward over the five layers; it joins both side streams at its end.
int net_backward(hipStream_t s, ts_workspace* ws, const DNet& n, const float* trunk, const float* head, const void* obs, bool obs_u8,
                 const DActs& a, const DBack& k, float* gtrunk, float* ghead) {
    const float* x[5] = {static_cast<const float*>(obs), a.c[0], a.c[1], a.c[2], a.feat};
    const float* wb[5];
    float* g[5];
    for (int i = 0; i < 4; ++i) { wb[i] = trunk + n.off[i]; g[i] = gtrunk + n.off[i]; }
    wb[4] = head; g[4] = ghead;
    return ts::chain_backward(s, ws, 5, n.l, x, k.dy, wb, k.slabs, g, obs_u8);
}

int check_head_args(const char* who, int64_t B, int64_t n_act, double fixed_alpha) {
    TS_REQUIRE(B >= 1 && B < (1 << 24), TS_ERR_INVALID_ARG, "%s: batch size must be in [1, 2^24)", who);
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_INVALID_ARG, "%s: 1 <= n_act <= 64", who);
    TS_REQUIRE(!std::isnan(fixed_alpha), TS_ERR_INVALID_ARG, "%s: alpha must not be NaN", who);
    return TS_OK;
}

}  // namespace

extern "C" {

int64_t ts_dsac_cnn_param_count(int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t hidden) {
    DNet n;
    if (make_dnet("ts_dsac_cnn_param_count", 1, c, h, w, n_act, hidden, &n)) return -1;
    return n.off[7];
}

int ts_dsac_cnn_layout(int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t hidden, int64_t* out11) {
    TS_REQUIRE(out11 != nullptr, TS_ERR_INVALID_ARG, "ts_dsac_cnn_layout: NULL output");
    DNet n;
    if (int rc = make_dnet("ts_dsac_cnn_layout", 1, c, h, w, n_act, hidden, &n)) return rc;
    out11[0] = n.F; out11[1] = n.ld; out11[2] = n.off[7]; out11[3] = n.T;
    for (int i = 0; i < 7; ++i) out11[4 + i] = n.off[i];
    return TS_OK;
}

int ts_dsac_cnn_target(const float* logits, const float* q1_old, const float* q2_old, const float* log_alpha, double fixed_alpha,
                       int64_t B, int64_t n_act, float* out, ts_stream_t stream) {
    if (int rc = check_head_args("ts_dsac_cnn_target", B, n_act, fixed_alpha)) return rc;
    TS_REQUIRE(logits && q1_old && q2_old && out, TS_ERR_INVALID_ARG, "ts_dsac_cnn_target: NULL argument");
    hipLaunchKernelGGL(dsacc_target_kernel, dim3(wave_blocks(B)), dim3(256), 0, ts::as_stream(stream), logits, q1_old, q2_old,
                       log_alpha, (float)fixed_alpha, B, (int)n_act, (int)n_act, out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_dsac_cnn_critic(const float* q, const int64_t* act, const float* target, const float* weight, int64_t B, int64_t n_act,
                       float* dq_out, float* td_out, float* terms_out, float* loss_out, ts_stream_t stream) {
    if (int rc = check_head_args("ts_dsac_cnn_critic", B, n_act, 0.0)) return rc;
    TS_REQUIRE(q && act && target && dq_out && td_out && terms_out && loss_out, TS_ERR_INVALID_ARG,
               "ts_dsac_cnn_critic: NULL argument");
    const int A = (int)n_act, ld = (A + 31) / 32 * 32;
    hipStream_t s = ts::as_stream(stream);
    hipLaunchKernelGGL(dsacc_critic_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, q, act, target, weight, (const float*)nullptr, B,
                       A, A, ld, dq_out, td_out, terms_out, (float*)nullptr);
    hipLaunchKernelGGL(dsacc_mean_kernel, dim3(1), dim3(1024), 0, s, terms_out, B, 1.f, loss_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_dsac_cnn_actor(const float* logits, const float* q1, const float* q2, const float* log_alpha, double fixed_alpha, int64_t B,
                      int64_t n_act, float* dlogits_out, float* entropy_out, float* terms_out, float* loss_out,
                      ts_stream_t stream) {
    if (int rc = check_head_args("ts_dsac_cnn_actor", B, n_act, fixed_alpha)) return rc;
    TS_REQUIRE(logits && q1 && q2 && dlogits_out && entropy_out && terms_out && loss_out, TS_ERR_INVALID_ARG,
               "ts_dsac_cnn_actor: NULL argument");
    const int A = (int)n_act, ld = (A + 31) / 32 * 32;
    hipStream_t s = ts::as_stream(stream);
    hipLaunchKernelGGL(dsacc_actor_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, logits, q1, q2, log_alpha, (float)fixed_alpha, B, A,
                       A, ld, dlogits_out, entropy_out, terms_out);
    hipLaunchKernelGGL(dsacc_mean_kernel, dim3(1), dim3(1024), 0, s, terms_out, B, -1.f, loss_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_dsac_cnn_forward(ts_workspace* ws, const float* params, int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t hidden,
                        const void* obs_nhwc, int obs_u8, int64_t B, float* logits_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_dsac_cnn_forward: workspace is NULL");
    DNet n;
    if (int rc = make_dnet("ts_dsac_cnn_forward", B, c, h, w, n_act, hidden, &n)) return rc;
    TS_REQUIRE(params && obs_nhwc && logits_out, TS_ERR_INVALID_ARG, "ts_dsac_cnn_forward: NULL argument");
    hipStream_t s = ts::as_stream(stream);
    if (int rc = ts::ws_reserve(ws, acts_bytes(n) + 4096)) return rc;
    DActs a;
    carve_acts(n, static_cast<char*>(ws->base), &a);
    if (int rc = trunk_forward(s, ws, n, params, obs_nhwc, obs_u8 != 0, a)) return rc;
    if (int rc = head_forward(s, ws, n, params + n.off[4], a, 0)) return rc;
    const int64_t tot = B * n.n_act;
    hipLaunchKernelGGL(dsacc_unpad_kernel, dim3((unsigned)ts::ceil_div(tot, 256)), dim3(256), 0, s, a.o[0], tot, n.n_act, n.ld,
                       logits_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_dsac_cnn_target_q(ts_workspace* ws, const float* params, const float* params_old, const float* log_alpha,
                         double fixed_alpha, int64_t c, int64_t h, int64_t w, int64_t n_act, int64_t hidden,
                         const void* obs_next_nhwc, int obs_u8, int64_t B, float* out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_dsac_cnn_target_q: workspace is NULL");
    DNet n;
    if (int rc = make_dnet("ts_dsac_cnn_target_q", B, c, h, w, n_act, hidden, &n)) return rc;
    TS_REQUIRE(!std::isnan(fixed_alpha), TS_ERR_INVALID_ARG, "ts_dsac_cnn_target_q: alpha must not be NaN");
    TS_REQUIRE(params && params_old && obs_next_nhwc && out, TS_ERR_INVALID_ARG, "ts_dsac_cnn_target_q: NULL argument");
    hipStream_t s = ts::as_stream(stream);
    if (int rc = ts::ws_reserve(ws, 2 * acts_bytes(n) + 4096)) return rc;
    DActs a, o;
    carve_acts(n, carve_acts(n, static_cast<char*>(ws->base), &a), &o);
    hipStream_t sv, sw;
    if (int rc = ts::side_streams(ws, s, &sv, &sw)) return rc;
    // the lagged trunk and its two heads (one after the other) on a side stream beside the live trunk and the actor head
    if (int rc = ts::stream_wait(ws, s, sv, 12)) return rc;
    if (int rc = trunk_forward(sv, ws, n, params_old, obs_next_nhwc, obs_u8 != 0, o)) return rc;
    if (int rc = head_forward(sv, ws, n, params_old + n.T, o, 1)) return rc;
    if (int rc = head_forward(sv, ws, n, params_old + n.T + n.Hd, o, 2)) return rc;
    if (int rc = trunk_forward(s, ws, n, params, obs_next_nhwc, obs_u8 != 0, a)) return rc;
    if (int rc = head_forward(s, ws, n, params + n.off[4], a, 0)) return rc;
    if (int rc = ts::stream_wait(ws, sv, s, 13)) return rc;
    hipLaunchKernelGGL(dsacc_target_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, a.o[0], o.o[1], o.o[2], log_alpha,
                       (float)fixed_alpha, B, n.n_act, n.ld, out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_dsac_cnn_update(ts_workspace* ws, float* params, float* params_old, float* adam_m3, float* adam_v3, float* log_alpha,
                       float* log_alpha_m, float* log_alpha_v, int64_t adam_step, int64_t c, int64_t h, int64_t w, int64_t n_act,
                       int64_t hidden, const void* obs_nhwc, int obs_u8, const int64_t* act, const float* returns,
                       const float* weight, int64_t B, const ts_sac_hparams* hp, float* stats_out5, float* weight_out,
                       float* grads_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_dsac_cnn_update: workspace is NULL");
    TS_REQUIRE(adam_step >= 1, TS_ERR_INVALID_ARG, "ts_dsac_cnn_update: bad step");
    DNet n;
    if (int rc = make_dnet("ts_dsac_cnn_update", B, c, h, w, n_act, hidden, &n)) return rc;
    TS_REQUIRE(params && params_old && adam_m3 && adam_v3 && obs_nhwc && act && returns && hp && stats_out5 && weight_out,
               TS_ERR_INVALID_ARG, "ts_dsac_cnn_update: NULL argument");
    TS_REQUIRE(!hp->auto_alpha || (log_alpha && log_alpha_m && log_alpha_v), TS_ERR_INVALID_ARG,
               "ts_dsac_cnn_update: auto alpha needs log_alpha and its Adam moments");
    TS_REQUIRE((hp->actor_lr < 0.0) == (hp->critic_lr < 0.0), TS_ERR_INVALID_ARG,
               "ts_dsac_cnn_update: a gradient-only call takes both learning rates negative");
    const bool apply = hp->actor_lr >= 0.0;
    TS_REQUIRE(apply || grads_out, TS_ERR_INVALID_ARG, "ts_dsac_cnn_update: a gradient-only call (lr < 0) needs grads_out");
    TS_REQUIRE(!std::isnan(hp->alpha) && hp->tau >= 0.0 && hp->tau <= 1.0, TS_ERR_INVALID_ARG,
               "ts_dsac_cnn_update: alpha must not be NaN, tau in [0, 1]");
    hipStream_t s = ts::as_stream(stream);
    const bool u8 = obs_u8 != 0;
    const int64_t G = n.T + n.Hd;                        // one gradient / moment set: trunk | own head

    // workspace: activations | the backward pass's buffers | one gradient set | td1, td2, per-sample terms, entropies | norm partials
    const size_t Bb = al(4 * (size_t)B);
    if (int rc = ts::ws_reserve(ws, acts_bytes(n) + back_bytes(n) + al(4 * (size_t)G) + 4 * Bb + 4096)) return rc;
    DActs a;
    DBack k;
    char* p = carve_back(n, carve_acts(n, static_cast<char*>(ws->base), &a), &k);
    float* gbuf = reinterpret_cast<float*>(p);
    p += al(4 * (size_t)G);
    float* td[2] = {reinterpret_cast<float*>(p), reinterpret_cast<float*>(p + Bb)};
    float* term = reinterpret_cast<float*>(p + 2 * Bb);
    float* ent = reinterpret_cast<float*>(p + 3 * Bb);
    float* norm_part = reinterpret_cast<float*>(p + 4 * Bb);
    const float* la = hp->auto_alpha ? log_alpha : nullptr;

    // one optimizer's step over trunk + own head: two launches, since the head does not follow the trunk in `params`
    auto adam = [&](int set, float* head, const float* g, double lr) -> int {
        float* m = adam_m3 + set * G;
        float* v = adam_v3 + set * G;
        if (int rc = ts::adam_step(s, params, m, v, g, n.T, adam_step, lr, hp->beta1, hp->beta2, hp->adam_eps, 0.0, norm_part))
            return rc;
        return ts::adam_step(s, head, m + n.T, v + n.T, g + n.T, n.Hd, adam_step, lr, hp->beta1, hp->beta2, hp->adam_eps, 0.0,
                             norm_part);
    };

    // 1, 2: the critics, one after the other (discrete_sac.py:162-172): critic 2's pass reads the trunk critic 1's step has
    // just moved.  A gradient-only call changes nothing in between, so one trunk pass serves all three.
    for (int q = 0; q < 2; ++q) {
        float* head = params + n.off[5 + q];
        float* g = grads_out ? grads_out + q * G : gbuf;
        if (q == 0 || apply)
            if (int rc = trunk_forward(s, ws, n, params, obs_nhwc, u8, a)) return rc;
        if (int rc = head_forward(s, ws, n, head, a, 1 + q)) return rc;
        hipLaunchKernelGGL(dsacc_critic_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, a.o[1 + q], act, returns, weight,
                           q == 1 ? td[0] : (const float*)nullptr, B, n.n_act, n.ld, n.ld, k.dy[4], td[q], term,
                           q == 1 ? weight_out : (float*)nullptr);
        hipLaunchKernelGGL(dsacc_mean_kernel, dim3(1), dim3(1024), 0, s, term, B, 1.f, stats_out5 + 1 + q);
        TS_LAUNCH_CHECK();
        if (q == 1)
            if (int rc = ts::record_td(ws, s)) return rc;            // batch.weight is written: ts_dqn_wait_td
        if (int rc = net_backward(s, ws, n, params, head, obs_nhwc, u8, a, k, g, g + n.T)) return rc;
        if (apply)
            if (int rc = adam(q, head, g, hp->critic_lr)) return rc;
    }

    // 3: the actor (discrete_sac.py:176-184): ONE pass of the twice-moved trunk feeds the actor head and both updated critic
    // heads; the two critic GEMMs run on the side streams beside the actor's
    {
        float* g = grads_out ? grads_out + 2 * G : gbuf;
        if (apply)
            if (int rc = trunk_forward(s, ws, n, params, obs_nhwc, u8, a)) return rc;
        hipStream_t sv, sw;
        if (int rc = ts::side_streams(ws, s, &sv, &sw)) return rc;
        if (int rc = ts::stream_wait(ws, s, sv, 12)) return rc;
        if (int rc = ts::stream_wait(ws, s, sw, 13)) return rc;
        if (int rc = head_forward(sv, ws, n, params + n.off[5], a, 1)) return rc;
        if (int rc = head_forward(sw, ws, n, params + n.off[6], a, 2)) return rc;
        if (int rc = head_forward(s, ws, n, params + n.off[4], a, 0)) return rc;
        if (int rc = ts::stream_wait(ws, sv, s, 14)) return rc;
        if (int rc = ts::stream_wait(ws, sw, s, 15)) return rc;
        hipLaunchKernelGGL(dsacc_actor_kernel, dim3(wave_blocks(B)), dim3(256), 0, s, a.o[0], a.o[1], a.o[2], la, (float)hp->alpha, B,
                           n.n_act, n.ld, n.ld, k.dy[4], ent, term);
        hipLaunchKernelGGL(dsacc_mean_kernel, dim3(1), dim3(1024), 0, s, term, B, -1.f, stats_out5);
        TS_LAUNCH_CHECK();
        if (int rc = net_backward(s, ws, n, params, params + n.off[4], obs_nhwc, u8, a, k, g, g + n.T)) return rc;
        if (apply)
            if (int rc = adam(2, params + n.off[4], g, hp->actor_lr)) return rc;
    }

    // 4: alpha (sac.py:203-209 on the entropies of step 3); a gradient-only call reports alpha and its loss and steps nothing
    AlphaStep as{};
    const double bc1 = 1.0 - pow(hp->beta1, (double)adam_step), bc2 = 1.0 - pow(hp->beta2, (double)adam_step);
    as.lr_step = (float)(std::max(hp->alpha_lr, 0.0) / bc1);
    as.beta2 = (float)hp->beta2;
    as.omb1 = (float)(1.0 - hp->beta1); as.omb2 = (float)(1.0 - hp->beta2);
    as.bc2_sqrt = (float)sqrt(bc2); as.eps = (float)hp->adam_eps;
    hipLaunchKernelGGL(dsacc_alpha_kernel, dim3(1), dim3(1024), 0, s, ent, B, (float)hp->target_entropy, hp->auto_alpha ? log_alpha : nullptr,
                       log_alpha_m, log_alpha_v, as, (float)hp->alpha, apply ? 1 : 0, stats_out5 + 4, stats_out5 + 3);
    TS_LAUNCH_CHECK();
    if (!apply || hp->tau <= 0.0) return TS_OK;

    // 5: Polyak of the lagged vector from the live one: the trunk, then the two critic heads (adjacent in both vectors)
    if (int rc = ts_polyak_update(params_old, params, n.T, hp->tau, stream)) return rc;
    return ts_polyak_update(params_old + n.T, params + n.off[5], 2 * n.Hd, hp->tau, stream);
}

}  // extern "C"
