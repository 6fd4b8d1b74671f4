// ts_icm.hip -- the Intrinsic Curiosity Module (arXiv 1705.05363) of a discrete-action rollout for gfx950.
//
// Replaces, on device-resident batches:
//   IntrinsicCuriosityModule.forward        tianshou/utils/net/discrete.py:377-428
//   _ICMMixin._icm_preprocess_batch         tianshou/algorithm/modelbased/icm.py:77-83   rew += mse_loss * reward_scale
//   _ICMMixin._icm_update                   icm.py:90-109: cross entropy + mse, one Optimizer.step on the whole batch
//
// Three Linear chains in one flat vector `feature | forward | inverse` (layout: tsengine.h).  Linear layers run on the fp32-MFMA
// GEMM kernels of ts_conv.hip; this file adds the per-row kernels (stack, pack, loss, reward, gradient merge) and the
// orchestration.  The feature net runs ONCE over the stacked [obs; obs_next] (2B rows), forward and backward; the first layers of
// the forward and the inverse model give their input gradient through conv_dgrad restricted to the feature columns.
#include <algorithm>

#include "ts_common.h"
#include "ts_conv.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXL = TS_NET_MAX_HIDDEN + 1;          // linear layers of one chain incl. the last

int pad32(int64_t v) { return (int)((v + 31) / 32 * 32); }
size_t al(size_t x) { return (x + 255) & ~size_t(255); }

struct Carve {
    char* p;
    float* f(size_t n) { float* r = reinterpret_cast<float*>(p); p += al(4 * n); return r; }
};

// One chain of Linear layers: width[0] = the padded input width, width[L] = the padded output width; hidden layers carry `act`
struct Chain {
    ts::ConvGeom l[MAXL];
    int64_t off[MAXL + 1];        // offsets into the flat vector; off[L] = end of the chain
    int L, act, wmax;
    int width[MAXL + 1];
};

void make_chain(int rows, int64_t in_dim, const int64_t* hidden, int n_hidden, int64_t out_dim, int act, int64_t base, Chain* c) {
    c->L = n_hidden + 1; c->act = act;
    c->width[0] = pad32(in_dim);
    for (int i = 0; i < n_hidden; ++i) c->width[i + 1] = pad32(hidden[i]);
    c->width[c->L] = pad32(out_dim);
    c->wmax = 32;
    int64_t o = base;
    for (int i = 0; i < c->L; ++i) {
        c->l[i] = ts::ConvGeom{rows, 1, 1, c->width[i], 1, 1, 1, 1, 1, c->width[i + 1]};
        c->off[i] = o;
        o += c->l[i].param_elems();
        c->wmax = std::max(c->wmax, c->width[i + 1]);
    }
    c->wmax = std::max(c->wmax, c->width[0]);
    c->off[c->L] = o;
}

struct Icm {
    Chain feat, fwd, inv;         // feat over 2B rows, fwd / inv over B rows
    int od, A, F, k0, Fp, Ap, KF, KI, wmax;
    int64_t P;
};

// Validates the descriptor (no launch has happened yet) and lays the three chains out for B transitions.
int make_icm(const ts_net_desc* fn, const ts_net_desc* mn, int64_t n_act, int64_t B, const char* who, Icm* m) {
    TS_REQUIRE(fn != nullptr && mn != nullptr, TS_ERR_INVALID_ARG, "%s: a network descriptor is NULL", who);
    const int64_t f_dim = mn->obs_dim;              // the models' unit: the feature net's output width
    TS_REQUIRE(fn->obs_dim >= 1 && fn->obs_dim <= 65536 && n_act >= 1 && f_dim >= 1 && f_dim <= 1024 && fn->n_hidden >= 0 &&
                   fn->n_hidden <= TS_NET_MAX_HIDDEN && mn->n_hidden >= 0 && mn->n_hidden <= TS_NET_MAX_HIDDEN, TS_ERR_INVALID_ARG,
               "%s: obs_dim in [1, 65536], n_act >= 1, feature_dim in [1, 1024], 0 .. %d hidden layers per net", who, TS_NET_MAX_HIDDEN);
    TS_REQUIRE(n_act <= TS_ICM_MAX_ACTIONS, TS_ERR_UNSUPPORTED, "%s: at most %d actions (got %lld)", who, TS_ICM_MAX_ACTIONS,
               (long long)n_act);
    TS_REQUIRE(fn->activation == TS_NET_ACT_RELU || fn->activation == TS_NET_ACT_TANH, TS_ERR_UNSUPPORTED,
               "%s: the feature net's activation must be ReLU or tanh", who);
    TS_REQUIRE(mn->activation == TS_NET_ACT_RELU, TS_ERR_UNSUPPORTED, "%s: the forward and the inverse model use ReLU", who);
    TS_REQUIRE(fn->flags == 0 && mn->flags == 0, TS_ERR_UNSUPPORTED, "%s: layer norm / conditioned sigma are not part of an ICM model", who);
    for (int i = 0; i < fn->n_hidden; ++i)
        TS_REQUIRE(fn->hidden[i] >= 1 && fn->hidden[i] <= 1024, TS_ERR_INVALID_ARG, "%s: hidden widths must be in [1, 1024]", who);
    for (int i = 0; i < mn->n_hidden; ++i)
        TS_REQUIRE(mn->hidden[i] >= 1 && mn->hidden[i] <= 1024, TS_ERR_INVALID_ARG, "%s: hidden widths must be in [1, 1024]", who);
    TS_REQUIRE(B >= 1 && B <= (int64_t)1 << 29, TS_ERR_INVALID_ARG, "%s: 1 <= B <= 2^29", who);
    m->od = (int)fn->obs_dim; m->A = (int)n_act; m->F = (int)f_dim;
    make_chain((int)(2 * B), fn->obs_dim, fn->hidden, fn->n_hidden, f_dim, fn->activation, 0, &m->feat);
    make_chain((int)B, f_dim + n_act, mn->hidden, mn->n_hidden, f_dim, TS_NET_ACT_RELU, m->feat.off[m->feat.L], &m->fwd);
    make_chain((int)B, 2 * f_dim, mn->hidden, mn->n_hidden, n_act, TS_NET_ACT_RELU, m->fwd.off[m->fwd.L], &m->inv);
    m->k0 = m->feat.width[0]; m->Fp = m->feat.width[m->feat.L]; m->Ap = m->inv.width[m->inv.L];
    m->KF = m->fwd.width[0]; m->KI = m->inv.width[0];
    m->wmax = std::max(m->feat.wmax, std::max(m->fwd.wmax, m->inv.wmax));
    m->P = m->inv.off[m->inv.L];
    // (the GEMM kernels index with 32 bits: the widest activation matrix must stay below 2^31 elements)
    TS_REQUIRE(2 * B * (int64_t)m->wmax < ((int64_t)1 << 31), TS_ERR_INVALID_ARG,
               "%s: 2 B x the widest layer (%d) must stay below 2^31 elements (split the batch)", who, m->wmax);
    return TS_OK;
}

struct ActC { float* h[MAXL]; };

ActC take_act(Carve& c, const Chain& n, int64_t rows) {
    ActC a{};
    for (int i = 0; i < n.L; ++i) a.h[i] = c.f(rows * n.width[i + 1]);
    return a;
}
size_t act_bytes(const Chain& n, int64_t rows) {
    size_t s = 0;
    for (int i = 0; i < n.L; ++i) s += al(4 * rows * n.width[i + 1]);
    return s;
}
size_t split_floats(const Chain& n) {
    size_t s = 4;
    for (int i = 0; i < n.L; ++i) { const int ns = ts::conv_fwd_splits(n.l[i]); if (ns > 1) s = std::max(s, (size_t)ns * n.l[i].out_elems()); }
    return s;
}
// floats of one scratch buffer for the hidden-layer gradients of a chain over `rows` rows
size_t hidden_grad_floats(const Chain& n, int64_t rows) {
    size_t s = 4;
    for (int i = 1; i < n.L; ++i) s = std::max(s, (size_t)rows * n.width[i]);
    return s;
}
size_t slab_floats(const Chain& n) {
    size_t s = 4;
    for (int i = 0; i < n.L; ++i) s = std::max(s, (size_t)ts::conv_wgrad_splits(n.l[i]) * n.l[i].param_elems());
    return s;
}

// ---- elementwise kernels ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void icm_tanh_kernel(float* __restrict__ h, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) h[i] = tanhf(h[i]);
}
// dh *= 1 - h^2 (tanh) resp. (h > 0) (ReLU; h is the layer's OUTPUT, torch's threshold_backward uses the same sign test)
__global__ __launch_bounds__(256) void icm_act_bwd_kernel(float* __restrict__ dh, const float* __restrict__ h, int64_t n, int act) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = h[i];
    dh[i] = act == TS_NET_ACT_TANH ? dh[i] * (1.f - v * v) : (v > 0.f ? dh[i] : 0.f);
}

// x[r, :] = obs[r] for r < B, obs_next[r - B] behind them, zero-padded to k0 columns
__global__ __launch_bounds__(256) void icm_stack_kernel(const float* __restrict__ obs, const float* __restrict__ obs_next, int64_t B,
                                                        int od, int k0, float* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * B * k0) return;
    const int64_t r = i / k0;
    const int j = (int)(i - r * k0);
    const float* src = r < B ? obs + r * od : obs_next + (r - B) * od;
    x[i] = j < od ? src[j] : 0.f;
}

// Both model inputs in one launch (they are independent): xf[b, :] = [phi1 | one_hot(act) | 0-pad] (KF columns), xi[b, :] =
// [phi1 | phi2 | 0-pad] (KI columns; xi == NULL: the forward model's alone).  phi: [2B, Fp], rows [0, B) = phi1, [B, 2B) = phi2.
// An action outside [0, A) is clamped into it.
__global__ __launch_bounds__(256) void icm_pack_kernel(const float* __restrict__ phi, const int64_t* __restrict__ act, int64_t B, int F,
                                                       int Fp, int A, int KF, int KI, float* __restrict__ xf, float* __restrict__ xi) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nf = B * KF;
    if (i < nf) {
        const int64_t b = i / KF;
        const int j = (int)(i - b * KF);
        float v = 0.f;
        if (j < F) {
            v = phi[b * Fp + j];
        } else if (j < F + A) {
            int64_t a = act[b];
            a = a < 0 ? 0 : (a >= A ? A - 1 : a);
            v = (j - F) == (int)a ? 1.f : 0.f;
        }
        xf[i] = v;
    } else if (xi != nullptr && i < nf + B * KI) {
        const int64_t k = i - nf;
        const int64_t b = k / KI;
        const int j = (int)(k - b * KI);
        xi[k] = j < F ? phi[b * Fp + j] : (j < 2 * F ? phi[(B + b) * Fp + (j - F)] : 0.f);
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

constexpr int LOSS_ROWS = 64;     // rows per workgroup of icm_loss_kernel: 4 wavefronts x 16 rows, one wavefront per row

// One wavefront per row.  e = phi2_hat - phi2 over the F feature columns (row pitches ps / qs); mse[b] = 0.5 sum e^2;
// d_p2h[b, j] = cf e for j < F, 0 for F <= j < dw (row pitch dw).  logits != NULL (A <= 64, row pitch ls): log-softmax with the
// row maximum subtracted, ce = log(sum exp(l - max)) - (l[act] - max), d_logits[b, j] = ci (softmax - one_hot) for j < A, 0 up
// to dlw.  partial[block] = {sum mse, sum ce} of the workgroup's rows, every wavefront adding its rows in order.
__global__ __launch_bounds__(256) void icm_loss_kernel(const float* __restrict__ p2h, int ps, const float* __restrict__ p2, int qs,
                                                       const float* __restrict__ logits, int ls, const int64_t* __restrict__ act,
                                                       int64_t B, int F, int A, float cf, float ci, float* __restrict__ mse,
                                                       float* __restrict__ d_p2h, int dw, float* __restrict__ d_logits, int dlw,
                                                       float* __restrict__ partial) {
    __shared__ float red[2][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc_m = 0.f, acc_c = 0.f;
    for (int k = 0; k < LOSS_ROWS / 4; ++k) {
        const int64_t b = (int64_t)blockIdx.x * LOSS_ROWS + 4 * k + wave;
        if (b >= B) break;                                   // (uniform per wavefront)
        float q = 0.f;
        const int cols = d_p2h ? (dw > F ? dw : F) : F;
        for (int j = lane; j < cols; j += 64) {
            float e = 0.f;
            if (j < F) {
                e = p2h[b * ps + j] - p2[b * qs + j];
                q += e * e;
            }
            if (d_p2h) d_p2h[b * dw + j] = cf * e;
        }
        const float m = 0.5f * wave_sum(q);
        if (lane == 0 && mse) mse[b] = m;
        acc_m += m;
        if (logits) {
            int64_t a = act[b];
            a = a < 0 ? 0 : (a >= A ? A - 1 : a);
            const float l = lane < A ? logits[b * ls + lane] : -INFINITY;
            const float mx = wave_max(l);
            const float z = l - mx;
            const float ex = lane < A ? expf(z) : 0.f;
            const float s = wave_sum(ex);
            const float za = __shfl(z, (int)a, 64);
            acc_c += logf(s) - za;
            if (d_logits && lane < dlw) d_logits[b * dlw + lane] = lane < A ? ci * (ex / s - (lane == (int)a ? 1.f : 0.f)) : 0.f;
        }
    }
    if (lane == 0) { red[0][wave] = acc_m; red[1][wave] = acc_c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        partial[2 * blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

__device__ __forceinline__ float block_sum256(float v, float* red4) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// stats3 = {((1 - w) inverse_loss + w forward_loss) lr_scale, forward_loss = mean mse, inverse_loss = mean ce} (icm.py:95-101);
// thread t adds partials t, t + 256, ... then block_sum256: a fixed order
__global__ __launch_bounds__(256) void icm_loss_finish_kernel(const float* __restrict__ partial, int n_blocks, float n, float w,
                                                              float lr_scale, float* __restrict__ stats3) {
    __shared__ float red4[4];
    float v0 = 0.f, v1 = 0.f;
    for (int i = threadIdx.x; i < n_blocks; i += 256) { v0 += partial[2 * i]; v1 += partial[2 * i + 1]; }
    const float t0 = block_sum256(v0, red4);
    __syncthreads();
    const float t1 = block_sum256(v1, red4);
    if (threadIdx.x == 0) {
        const float fl = t0 / n, il = t1 / n;
        stats3[0] = ((1.f - w) * il + w * fl) * lr_scale;
        stats3[1] = fl;
        stats3[2] = il;
    }
}

// icm.py:83: rew_out = rew + (double)(mse * (float)reward_scale); reward_scale == 0 copies rew
__global__ __launch_bounds__(256) void icm_reward_kernel(const double* __restrict__ rew, const float* __restrict__ mse, int64_t B, float rs,
                                                         double* __restrict__ rew_out) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const double r = rew[b];
    rew_out[b] = rs == 0.f ? r : r + (double)(mse[b] * rs);
}

// The upstream gradient of the stacked feature pass, [2B, Fp]: d_phi1 = the forward model's input gradient + the inverse model's
// (columns [0, F) of dxf / dxi); d_phi2 = the inverse model's (columns [F, 2F) of dxi) + the direct mse term -d_p2h; padding 0.
__global__ __launch_bounds__(256) void icm_merge_kernel(const float* __restrict__ dxf, int KF, const float* __restrict__ dxi, int KI,
                                                        const float* __restrict__ d_p2h, int64_t B, int F, int Fp, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * B * Fp) return;
    const int64_t r = i / Fp;
    const int j = (int)(i - r * Fp);
    float v = 0.f;
    if (j < F) {
        if (r < B) v = dxf[r * KF + j] + dxi[r * KI + j];
        else v = dxi[(r - B) * KI + F + j] - d_p2h[(r - B) * Fp + j];
    }
    out[i] = v;
}

// out[b, j] = in[b, j] for j < A (pitch Ap -> A)
__global__ __launch_bounds__(256) void icm_unpad_kernel(const float* __restrict__ in, int64_t B, int A, int Ap, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * A) return;
    const int64_t b = i / A;
    out[i] = in[b * Ap + (i - b * A)];
}

unsigned blocks_of(int64_t n) { return (unsigned)ts::ceil_div(n, 256); }

int chain_forward(hipStream_t s, ts_workspace* ws, const Chain& n, const float* p, const float* x, const ActC& a, float* split, int64_t rows) {
    const float* in = x;
    for (int i = 0; i < n.L; ++i) {
        const bool hidden = i + 1 < n.L;
        if (int rc = ts::conv_forward(s, n.l[i], in, p + n.off[i], a.h[i], hidden && n.act == TS_NET_ACT_RELU, split, ws)) return rc;
        if (hidden && n.act == TS_NET_ACT_TANH) {
            const int64_t cnt = rows * n.width[i + 1];
            hipLaunchKernelGGL(icm_tanh_kernel, dim3(blocks_of(cnt)), dim3(256), 0, s, a.h[i], cnt);
            TS_LAUNCH_CHECK();
        }
        in = a.h[i];
    }
    return TS_OK;
}

// grad[off[0] .. off[L]) = J^T d_out (d_out: [rows, width[L]], padding columns zero); dha / dhb: two scratch buffers of
// hidden_grad_floats(n, rows) floats (the hidden gradients ping-pong between them).
// dx0 != NULL: columns [0, dx_cols) of the gradient w.r.t. the chain's input go to dx0 ([rows, width[0]]; the other columns of
// the last computed tile aside, the rest is left unwritten).
int chain_backward(hipStream_t s, ts_workspace* ws, const Chain& n, const float* p, const float* x, const ActC& a, const float* d_out,
                   float* grad, float* dha, float* dhb, float* slabs, int64_t rows, float* dx0, int dx_cols) {
    const float* dy = d_out;
    for (int i = n.L - 1; i >= 0; --i) {
        const float* xin = i == 0 ? x : a.h[i - 1];
        if (int rc = ts::conv_wgrad(s, n.l[i], xin, dy, slabs, ws)) return rc;
        if (int rc = ts::slab_sum(s, slabs, ts::conv_wgrad_splits(n.l[i]), n.l[i].param_elems(), grad + n.off[i])) return rc;
        if (i > 0) {
            float* dx = (dy == dha) ? dhb : dha;
            if (int rc = ts::conv_dgrad(s, n.l[i], dy, p + n.off[i], nullptr, dx, ws)) return rc;
            const int64_t cnt = rows * n.width[i];
            hipLaunchKernelGGL(icm_act_bwd_kernel, dim3(blocks_of(cnt)), dim3(256), 0, s, dx, a.h[i - 1], cnt, n.act);
            TS_LAUNCH_CHECK();
            dy = dx;
        } else if (dx0 != nullptr) {
            if (int rc = ts::conv_dgrad(s, n.l[0], dy, p + n.off[0], nullptr, dx0, ws, 0, dx_cols)) return rc;
        }
    }
    return TS_OK;
}

struct Fwd {                      // what the forward pass leaves in the workspace
    float *x0, *xf, *xi, *split;
    ActC af, aw, ai;
    const float *phi, *p2h, *logits;
};

size_t fwd_bytes(const Icm& m, int64_t B, bool inverse) {
    const size_t sp = std::max(split_floats(m.feat), std::max(split_floats(m.fwd), inverse ? split_floats(m.inv) : 4));
    return al(4 * 2 * B * m.k0) + act_bytes(m.feat, 2 * B) + al(4 * B * m.KF) + act_bytes(m.fwd, B) +
           (inverse ? al(4 * B * m.KI) + act_bytes(m.inv, B) : 0) + al(4 * sp);
}

// stack -> feature net over 2B rows -> pack -> forward model (-> inverse model)
int icm_forward_pass(hipStream_t s, ts_workspace* ws, const Icm& m, const float* params, const float* obs, const int64_t* act,
                     const float* obs_next, int64_t B, bool inverse, Carve& c, Fwd* f) {
    f->x0 = c.f(2 * B * m.k0);
    f->af = take_act(c, m.feat, 2 * B);
    f->xf = c.f(B * m.KF);
    f->aw = take_act(c, m.fwd, B);
    f->xi = nullptr;
    if (inverse) { f->xi = c.f(B * m.KI); f->ai = take_act(c, m.inv, B); }
    f->split = c.f(std::max(split_floats(m.feat), std::max(split_floats(m.fwd), inverse ? split_floats(m.inv) : 4)));
    hipLaunchKernelGGL(icm_stack_kernel, dim3(blocks_of(2 * B * m.k0)), dim3(256), 0, s, obs, obs_next, B, m.od, m.k0, f->x0);
    TS_LAUNCH_CHECK();
    if (int rc = chain_forward(s, ws, m.feat, params, f->x0, f->af, f->split, 2 * B)) return rc;
    f->phi = f->af.h[m.feat.L - 1];
    hipLaunchKernelGGL(icm_pack_kernel, dim3(blocks_of(B * (m.KF + (inverse ? m.KI : 0)))), dim3(256), 0, s, f->phi, act, B, m.F, m.Fp,
                       m.A, m.KF, m.KI, f->xf, f->xi);
    TS_LAUNCH_CHECK();
    if (int rc = chain_forward(s, ws, m.fwd, params, f->xf, f->aw, f->split, B)) return rc;
    f->p2h = f->aw.h[m.fwd.L - 1];
    f->logits = nullptr;
    if (inverse) {
        if (int rc = chain_forward(s, ws, m.inv, params, f->xi, f->ai, f->split, B)) return rc;
        f->logits = f->ai.h[m.inv.L - 1];
    }
    return TS_OK;
}

}  // namespace

extern "C" {

int ts_icm_layout(const ts_net_desc* feat_net, const ts_net_desc* model_net, int64_t n_act, int64_t* h_out7) {
    TS_REQUIRE(h_out7 != nullptr, TS_ERR_INVALID_ARG, "ts_icm_layout: output is NULL");
    Icm m;
    if (int rc = make_icm(feat_net, model_net, n_act, 1, "ts_icm_layout", &m)) return rc;
    h_out7[0] = m.P;
    h_out7[1] = m.feat.off[0]; h_out7[2] = m.feat.off[m.feat.L] - m.feat.off[0];
    h_out7[3] = m.fwd.off[0]; h_out7[4] = m.fwd.off[m.fwd.L] - m.fwd.off[0];
    h_out7[5] = m.inv.off[0]; h_out7[6] = m.inv.off[m.inv.L] - m.inv.off[0];
    return TS_OK;
}

int ts_icm_loss(ts_workspace* ws, const float* phi2_hat, const float* phi2, const float* logits, const int64_t* act, int64_t B,
                int64_t F, int64_t A, double forward_loss_weight, double lr_scale, float* mse_out, float* d_phi2_hat_out,
                float* d_logits_out, float* stats_out3, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_icm_loss: workspace is NULL");
    TS_REQUIRE(phi2_hat && phi2 && logits && act && stats_out3, TS_ERR_INVALID_ARG, "ts_icm_loss: NULL argument");
    TS_REQUIRE(B >= 1 && B <= (int64_t)1 << 29 && F >= 1 && F <= 1024 && A >= 1, TS_ERR_INVALID_ARG,
               "ts_icm_loss: 1 <= B <= 2^29, F in [1, 1024], A >= 1");
    TS_REQUIRE(A <= TS_ICM_MAX_ACTIONS, TS_ERR_UNSUPPORTED, "ts_icm_loss: at most %d actions (got %lld)", TS_ICM_MAX_ACTIONS, (long long)A);
    const int n_blocks = (int)ts::ceil_div(B, LOSS_ROWS);
    if (int rc = ts::ws_reserve(ws, al(8 * (size_t)n_blocks) + 4096)) return rc;
    float* partial = static_cast<float*>(ws->base);
    hipStream_t s = ts::as_stream(stream);
    const double w = forward_loss_weight;
    hipLaunchKernelGGL(icm_loss_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, phi2_hat, (int)F, phi2, (int)F, logits, (int)A, act, B,
                       (int)F, (int)A, (float)(w * lr_scale / (double)B), (float)((1.0 - w) * lr_scale / (double)B), mse_out,
                       d_phi2_hat_out, (int)F, d_logits_out, (int)A, partial);
    hipLaunchKernelGGL(icm_loss_finish_kernel, dim3(1), dim3(256), 0, s, partial, n_blocks, (float)B, (float)w, (float)lr_scale, stats_out3);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_icm_forward(ts_workspace* ws, const float* params, const ts_net_desc* feat_net, const ts_net_desc* model_net, int64_t n_act, const float* obs, const int64_t* act,
                   const float* obs_next, int64_t B, float* mse_out, float* act_hat_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_icm_forward: workspace is NULL");
    TS_REQUIRE(params && obs && act && obs_next && mse_out, TS_ERR_INVALID_ARG, "ts_icm_forward: NULL argument");
    Icm m;
    if (int rc = make_icm(feat_net, model_net, n_act, B, "ts_icm_forward", &m)) return rc;
    const bool inverse = act_hat_out != nullptr;
    const int n_blocks = (int)ts::ceil_div(B, LOSS_ROWS);
    if (int rc = ts::ws_reserve(ws, fwd_bytes(m, B, inverse) + al(8 * (size_t)n_blocks) + 8192)) return rc;
    hipStream_t s = ts::as_stream(stream);
    Carve c{static_cast<char*>(ws->base)};
    Fwd f;
    if (int rc = icm_forward_pass(s, ws, m, params, obs, act, obs_next, B, inverse, c, &f)) return rc;
    float* partial = c.f(2 * (size_t)n_blocks);
    hipLaunchKernelGGL(icm_loss_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, f.p2h, m.Fp, f.phi + B * m.Fp, m.Fp, (const float*)nullptr, 0,
                       act, B, m.F, m.A, 0.f, 0.f, mse_out, (float*)nullptr, 0, (float*)nullptr, 0, partial);
    if (inverse) hipLaunchKernelGGL(icm_unpad_kernel, dim3(blocks_of(B * m.A)), dim3(256), 0, s, f.logits, B, m.A, m.Ap, act_hat_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_icm_reward(ts_workspace* ws, const float* params, const ts_net_desc* feat_net, const ts_net_desc* model_net, int64_t n_act, const float* obs, const int64_t* act,
                  const float* obs_next, int64_t B, const double* rew, double reward_scale, double* rew_out, float* mse_out,
                  ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_icm_reward: workspace is NULL");
    TS_REQUIRE(params && obs && act && obs_next && rew && rew_out, TS_ERR_INVALID_ARG, "ts_icm_reward: NULL argument");
    Icm m;
    if (int rc = make_icm(feat_net, model_net, n_act, B, "ts_icm_reward", &m)) return rc;
    const int n_blocks = (int)ts::ceil_div(B, LOSS_ROWS);
    if (int rc = ts::ws_reserve(ws, fwd_bytes(m, B, false) + al(8 * (size_t)n_blocks) + al(4 * B) + 8192)) return rc;
    hipStream_t s = ts::as_stream(stream);
    Carve c{static_cast<char*>(ws->base)};
    Fwd f;
    if (int rc = icm_forward_pass(s, ws, m, params, obs, act, obs_next, B, false, c, &f)) return rc;
    float* partial = c.f(2 * (size_t)n_blocks);
    float* mse = mse_out ? mse_out : c.f(B);
    hipLaunchKernelGGL(icm_loss_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, f.p2h, m.Fp, f.phi + B * m.Fp, m.Fp, (const float*)nullptr, 0,
                       act, B, m.F, m.A, 0.f, 0.f, mse, (float*)nullptr, 0, (float*)nullptr, 0, partial);
    hipLaunchKernelGGL(icm_reward_kernel, dim3(blocks_of(B)), dim3(256), 0, s, rew, mse, B, (float)reward_scale, rew_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_icm_update(ts_workspace* ws, float* params, float* state_m, float* state_v, int64_t optim_step, const ts_net_desc* feat_net, const ts_net_desc* model_net, int64_t n_act,
                  const float* obs, const int64_t* act, const float* obs_next, int64_t B, double forward_loss_weight,
                  double lr_scale, int32_t optim_kind, double lr, double beta1, double beta2, double eps, double weight_decay,
                  double rms_alpha, double rms_momentum, int32_t rms_centered, double max_grad_norm, float* stats_out3,
                  float* grad_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_icm_update: workspace is NULL");
    TS_REQUIRE(params && state_m && state_v && obs && act && obs_next && stats_out3, TS_ERR_INVALID_ARG, "ts_icm_update: NULL argument");
    TS_REQUIRE(optim_step >= 1 && (optim_kind == TS_OPT_ADAM || optim_kind == TS_OPT_RMSPROP), TS_ERR_INVALID_ARG,
               "ts_icm_update: optim_step >= 1, optim_kind Adam or RMSprop");
    Icm m;
    if (int rc = make_icm(feat_net, model_net, n_act, B, "ts_icm_update", &m)) return rc;
    const int n_blocks = (int)ts::ceil_div(B, LOSS_ROWS);
    const size_t sl = std::max(slab_floats(m.feat), std::max(slab_floats(m.fwd), slab_floats(m.inv)));
    const size_t dh = std::max(hidden_grad_floats(m.feat, 2 * B), std::max(hidden_grad_floats(m.fwd, B), hidden_grad_floats(m.inv, B)));
    const size_t bytes = fwd_bytes(m, B, true) + al(8 * (size_t)n_blocks) + al(4 * B * m.Fp) + al(4 * B * m.Ap) + al(4 * B * m.KF) +
                         al(4 * B * m.KI) + al(4 * 2 * B * m.Fp) + 2 * al(4 * dh) + al(4 * sl) + al(4 * m.P) + al(4 * 1024) +
                         16384;
    if (int rc = ts::ws_reserve(ws, bytes)) return rc;
    hipStream_t s = ts::as_stream(stream);
    Carve c{static_cast<char*>(ws->base)};
    Fwd f;
    if (int rc = icm_forward_pass(s, ws, m, params, obs, act, obs_next, B, true, c, &f)) return rc;
    float* partial = c.f(2 * (size_t)n_blocks);
    float* d_p2h = c.f(B * m.Fp);
    float* d_logits = c.f(B * m.Ap);
    float* dxf = c.f(B * m.KF);
    float* dxi = c.f(B * m.KI);
    float* dphi = c.f(2 * B * m.Fp);
    float* dha = c.f(dh);
    float* dhb = c.f(dh);
    float* slabs = c.f(sl);
    float* grad = grad_out ? grad_out : c.f(m.P);
    float* norm_part = c.f(1024);
    const double w = forward_loss_weight;
    hipLaunchKernelGGL(icm_loss_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, f.p2h, m.Fp, f.phi + B * m.Fp, m.Fp, f.logits, m.Ap, act, B,
                       m.F, m.A, (float)(w * lr_scale / (double)B), (float)((1.0 - w) * lr_scale / (double)B), (float*)nullptr, d_p2h, m.Fp,
                       d_logits, m.Ap, partial);
    hipLaunchKernelGGL(icm_loss_finish_kernel, dim3(1), dim3(256), 0, s, partial, n_blocks, (float)B, (float)w, (float)lr_scale, stats_out3);
    TS_LAUNCH_CHECK();
    // the two models, each down to the feature columns of its input
    if (int rc = chain_backward(s, ws, m.fwd, params, f.xf, f.aw, d_p2h, grad, dha, dhb, slabs, B, dxf, m.F)) return rc;
    if (int rc = chain_backward(s, ws, m.inv, params, f.xi, f.ai, d_logits, grad, dha, dhb, slabs, B, dxi, 2 * m.F)) return rc;
    hipLaunchKernelGGL(icm_merge_kernel, dim3(blocks_of(2 * B * m.Fp)), dim3(256), 0, s, dxf, m.KF, dxi, m.KI, d_p2h, B, m.F, m.Fp, dphi);
    TS_LAUNCH_CHECK();
    // the shared feature net, once over the stacked rows
    if (int rc = chain_backward(s, ws, m.feat, params, f.x0, f.af, dphi, grad, dha, dhb, slabs, 2 * B, nullptr, 0)) return rc;
    if (lr < 0.0) return TS_OK;
    ts::OptimDesc o;
    o.kind = optim_kind; o.centered = rms_centered; o.weight_decay = weight_decay; o.alpha = rms_alpha; o.momentum = rms_momentum;
    return ts::optim_step(s, o, params, state_m, state_v, grad, m.P, optim_step, lr, beta1, beta2, eps, max_grad_norm, norm_part);
}

}  // extern "C"

// ---- ICM on the Atari trunk (ts_icm_cnn_*) ------------------------------------------------------------------------------------
// The feature net is DQNet(features_only=True).net (atari_network.py: three convolutions, a ReLU behind EACH, Flatten) on NHWC
// frames; phi = conv3's output [2B, OH3, OW3, 64] read as [2B, F] -- the NHWC flatten, F a multiple of 64, no padding columns.
// The forward / inverse models, the pack / loss / reward kernels and the model chains' reverse pass are the ones above.  New
// here: the frame stack (bytes, no float32 copy), the MASKED merge of the upstream feature gradient (phi carries a ReLU, the MLP
// feature net's output does not) and the chunk accumulation: a rollout is walked in chunks of B rows whose gradients and loss
// sums are added onto the caller's accumulators in chunk order, so one optimizer step sees the whole batch (icm.py:90-109).
namespace {

struct IcmCnn {
    ts::ConvGeom cv[3];           // over 2B rows
    int64_t coff[4];
    Chain fwd, inv;               // over B rows
    int c, h, w, A, F, Ap, KF, KI;
    int64_t P;
};

int make_icm_cnn(int64_t c, int64_t h, int64_t w, const ts_net_desc* mn, int64_t n_act, int64_t B, const char* who, IcmCnn* m) {
    TS_REQUIRE(mn != nullptr, TS_ERR_INVALID_ARG, "%s: the model descriptor is NULL", who);
    TS_REQUIRE(c >= 1 && c <= 4096 && h >= 1 && h <= 16384 && w >= 1 && w <= 16384 && n_act >= 1 && mn->n_hidden >= 0 &&
                   mn->n_hidden <= TS_NET_MAX_HIDDEN, TS_ERR_INVALID_ARG,
               "%s: c in [1, 4096], h and w in [1, 16384], n_act >= 1, 0 .. %d hidden layers", who, TS_NET_MAX_HIDDEN);
    TS_REQUIRE(n_act <= TS_ICM_MAX_ACTIONS, TS_ERR_UNSUPPORTED, "%s: at most %d actions (got %lld)", who, TS_ICM_MAX_ACTIONS,
               (long long)n_act);
    TS_REQUIRE(mn->activation == TS_NET_ACT_RELU, TS_ERR_UNSUPPORTED, "%s: the forward and the inverse model use ReLU", who);
    TS_REQUIRE(mn->flags == 0, TS_ERR_UNSUPPORTED, "%s: layer norm / conditioned sigma are not part of an ICM model", who);
    for (int i = 0; i < mn->n_hidden; ++i)
        TS_REQUIRE(mn->hidden[i] >= 1 && mn->hidden[i] <= 1024, TS_ERR_INVALID_ARG, "%s: hidden widths must be in [1, 1024]", who);
    TS_REQUIRE(B >= 1 && B <= (int64_t)1 << 29, TS_ERR_INVALID_ARG, "%s: 1 <= B <= 2^29", who);
    static const int oc[3] = {32, 64, 64}, ks[3] = {8, 4, 3}, st[3] = {4, 2, 1};
    int ic = (int)c, ih = (int)h, iw = (int)w;
    int64_t o = 0;
    for (int i = 0; i < 3; ++i) {
        TS_REQUIRE(ih >= ks[i] && iw >= ks[i], TS_ERR_INVALID_ARG,
                   "%s: a %lld x %lld frame is too small for the conv stack (layer %d sees %d x %d, kernel %d)", who, (long long)h,
                   (long long)w, i + 1, ih, iw, ks[i]);
        m->cv[i] = ts::ConvGeom{(int)(2 * B), ih, iw, ic, ks[i], ks[i], st[i], (ih - ks[i]) / st[i] + 1, (iw - ks[i]) / st[i] + 1, oc[i]};
        m->coff[i] = o;
        o += m->cv[i].param_elems();
        ic = oc[i]; ih = m->cv[i].OH; iw = m->cv[i].OW;
    }
    m->coff[3] = o;
    // (what ts_conv.hip's geometry check asks of conv1; conv2 / conv3 have 32 / 64 input channels)
    TS_REQUIRE((w * c) % 4 == 0, TS_ERR_INVALID_ARG, "%s: w x c = %lld must be a multiple of 4 (the conv layer's 16-byte runs)", who,
               (long long)(w * c));
    TS_REQUIRE(2 * B * h * w * c < ((int64_t)1 << 31) && 2 * B * m->cv[0].OH * m->cv[0].OW * 32 < ((int64_t)1 << 31), TS_ERR_INVALID_ARG,
               "%s: 2 B x the frame (%lld values) and 2 B x conv1's output (%lld) must stay below 2^31 elements (split the batch)", who,
               (long long)(h * w * c), (long long)m->cv[0].OH * m->cv[0].OW * 32);
    m->c = (int)c; m->h = (int)h; m->w = (int)w; m->A = (int)n_act;
    m->F = 64 * ih * iw;
    make_chain((int)B, m->F + n_act, mn->hidden, mn->n_hidden, m->F, TS_NET_ACT_RELU, o, &m->fwd);
    make_chain((int)B, 2 * (int64_t)m->F, mn->hidden, mn->n_hidden, n_act, TS_NET_ACT_RELU, m->fwd.off[m->fwd.L], &m->inv);
    m->KF = m->fwd.width[0]; m->KI = m->inv.width[0]; m->Ap = m->inv.width[m->inv.L];
    m->P = m->inv.off[m->inv.L];
    return TS_OK;
}

// out = [a; b], n vector elements each (V = 16 or 4 bytes): the two frame blocks as ONE 2B-row operand, bytes as they are
template <typename V>
__global__ __launch_bounds__(256) void icm_cnn_stack_kernel(const V* __restrict__ a, const V* __restrict__ b, int64_t n, V* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i];
    else if (i < 2 * n) out[i] = b[i - n];
}

// The upstream gradient of the stacked feature pass, [2B, F], four columns per thread: d_phi1 = dxf[:, :F] + dxi[:, :F], d_phi2 =
// dxi[:, F:2F] - d_p2h, both times (phi > 0): phi is conv3's output AFTER its ReLU (torch's threshold_backward tests the output).
__global__ __launch_bounds__(256) void icm_cnn_merge_kernel(const float* __restrict__ dxf, int KF, const float* __restrict__ dxi, int KI,
                                                            const float* __restrict__ d_p2h, const float* __restrict__ phi, int64_t B,
                                                            int F, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int q = F / 4;
    if (i >= 2 * B * q) return;
    const int64_t r = i / q;
    const int j = 4 * (int)(i - r * q);
    float4 v;
    if (r < B) {
        const float4 a = *reinterpret_cast<const float4*>(dxf + r * KF + j), b = *reinterpret_cast<const float4*>(dxi + r * KI + j);
        v = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    } else {
        const float4 a = *reinterpret_cast<const float4*>(dxi + (r - B) * KI + F + j);
        const float4 b = *reinterpret_cast<const float4*>(d_p2h + (r - B) * F + j);
        v = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
    }
    const float4 p = *reinterpret_cast<const float4*>(phi + r * F + j);
    v.x = p.x > 0.f ? v.x : 0.f; v.y = p.y > 0.f ? v.y : 0.f; v.z = p.z > 0.f ? v.z : 0.f; v.w = p.w > 0.f ? v.w : 0.f;
    *reinterpret_cast<float4*>(out + r * F + j) = v;
}

// acc += g (n a multiple of 4): one chunk's gradient onto the accumulator; every element is one thread's, chunks arrive in order
__global__ __launch_bounds__(256) void icm_cnn_accum_kernel(float* __restrict__ acc, const float* __restrict__ g, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 a = reinterpret_cast<float4*>(acc)[i];
    const float4 b = reinterpret_cast<const float4*>(g)[i];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    reinterpret_cast<float4*>(acc)[i] = a;
}

// sums2 = {sum mse, sum ce} of this chunk's loss workgroups (the order of icm_loss_finish_kernel), overwriting or added onto it
__global__ __launch_bounds__(256) void icm_cnn_sums_kernel(const float* __restrict__ partial, int n_blocks, int accumulate,
                                                           float* __restrict__ sums2) {
    __shared__ float red4[4];
    float v0 = 0.f, v1 = 0.f;
    for (int i = threadIdx.x; i < n_blocks; i += 256) { v0 += partial[2 * i]; v1 += partial[2 * i + 1]; }
    const float t0 = block_sum256(v0, red4);
    __syncthreads();
    const float t1 = block_sum256(v1, red4);
    if (threadIdx.x == 0) {
        sums2[0] = accumulate ? sums2[0] + t0 : t0;
        sums2[1] = accumulate ? sums2[1] + t1 : t1;
    }
}

struct FwdCnn {
    void* x0;
    float* a[3];
    float *xf, *xi, *split;
    ActC aw, ai;
    const float *phi, *p2h, *logits;
};

size_t cnn_split_floats(const IcmCnn& m, bool inverse) {
    size_t s = std::max(split_floats(m.fwd), inverse ? split_floats(m.inv) : 4);
    for (int i = 0; i < 3; ++i) { const int ns = ts::conv_fwd_splits(m.cv[i]); if (ns > 1) s = std::max(s, (size_t)ns * m.cv[i].out_elems()); }
    return s;
}

size_t cnn_fwd_bytes(const IcmCnn& m, int64_t B, bool inverse) {
    size_t s = al(4 * (size_t)m.cv[0].in_elems());
    for (int i = 0; i < 3; ++i) s += al(4 * (size_t)m.cv[i].out_elems());
    return s + al(4 * B * m.KF) + act_bytes(m.fwd, B) + (inverse ? al(4 * B * m.KI) + act_bytes(m.inv, B) : 0) +
           al(4 * cnn_split_floats(m, inverse));
}

int cnn_check_frames(const void* obs, const void* obs_next, const char* who) {
    TS_REQUIRE(((uintptr_t)obs | (uintptr_t)obs_next) % 4 == 0, TS_ERR_INVALID_ARG, "%s: the frame blocks must be 4-byte aligned", who);
    return TS_OK;
}

// stack -> conv1..3 over 2B rows -> pack -> forward model (-> inverse model)
int icm_cnn_forward_pass(hipStream_t s, ts_workspace* ws, const IcmCnn& m, const float* params, const void* obs, bool obs_u8,
                         const int64_t* act, const void* obs_next, int64_t B, bool inverse, Carve& c, FwdCnn* f) {
    f->x0 = c.f((size_t)m.cv[0].in_elems());
    for (int i = 0; i < 3; ++i) f->a[i] = c.f((size_t)m.cv[i].out_elems());
    f->xf = c.f(B * m.KF);
    f->aw = take_act(c, m.fwd, B);
    f->xi = nullptr;
    if (inverse) { f->xi = c.f(B * m.KI); f->ai = take_act(c, m.inv, B); }
    f->split = c.f(cnn_split_floats(m, inverse));
    const int64_t nb = B * m.h * m.w * m.c * (obs_u8 ? 1 : 4);       // bytes of one block: a multiple of 4 (w c is)
    if ((((uintptr_t)obs | (uintptr_t)obs_next) % 16 == 0) && nb % 16 == 0)
        hipLaunchKernelGGL(icm_cnn_stack_kernel<uint4>, dim3(blocks_of(2 * (nb / 16))), dim3(256), 0, s, static_cast<const uint4*>(obs),
                           static_cast<const uint4*>(obs_next), nb / 16, static_cast<uint4*>(f->x0));
    else
        hipLaunchKernelGGL(icm_cnn_stack_kernel<uint32_t>, dim3(blocks_of(2 * (nb / 4))), dim3(256), 0, s, static_cast<const uint32_t*>(obs),
                           static_cast<const uint32_t*>(obs_next), nb / 4, static_cast<uint32_t*>(f->x0));
    TS_LAUNCH_CHECK();
    const float* x = static_cast<const float*>(f->x0);
    for (int i = 0; i < 3; ++i) {
        if (int rc = ts::conv_forward(s, m.cv[i], x, params + m.coff[i], f->a[i], true, f->split, ws, i == 0 && obs_u8)) return rc;
        x = f->a[i];
    }
    f->phi = f->a[2];
    hipLaunchKernelGGL(icm_pack_kernel, dim3(blocks_of(B * (m.KF + (inverse ? m.KI : 0)))), dim3(256), 0, s, f->phi, act, B, m.F, m.F,
                       m.A, m.KF, m.KI, f->xf, f->xi);
    TS_LAUNCH_CHECK();
    if (int rc = chain_forward(s, ws, m.fwd, params, f->xf, f->aw, f->split, B)) return rc;
    f->p2h = f->aw.h[m.fwd.L - 1];
    f->logits = nullptr;
    if (inverse) {
        if (int rc = chain_forward(s, ws, m.inv, params, f->xi, f->ai, f->split, B)) return rc;
        f->logits = f->ai.h[m.inv.L - 1];
    }
    return TS_OK;
}

}  // namespace

extern "C" {

int ts_icm_cnn_layout(int64_t c, int64_t h, int64_t w, const ts_net_desc* model_net, int64_t n_act, int64_t* h_out12) {
    TS_REQUIRE(h_out12 != nullptr, TS_ERR_INVALID_ARG, "ts_icm_cnn_layout: output is NULL");
    IcmCnn m;
    if (int rc = make_icm_cnn(c, h, w, model_net, n_act, 1, "ts_icm_cnn_layout", &m)) return rc;
    h_out12[0] = m.P; h_out12[1] = m.F;
    for (int i = 0; i < 3; ++i) { h_out12[2 + 2 * i] = m.coff[i]; h_out12[3 + 2 * i] = m.coff[i + 1] - m.coff[i]; }
    h_out12[8] = m.fwd.off[0]; h_out12[9] = m.fwd.off[m.fwd.L] - m.fwd.off[0];
    h_out12[10] = m.inv.off[0]; h_out12[11] = m.inv.off[m.inv.L] - m.inv.off[0];
    return TS_OK;
}

int ts_icm_cnn_forward(ts_workspace* ws, const float* params, int64_t c, int64_t h, int64_t w, const ts_net_desc* model_net, int64_t n_act,
                       const void* obs_nhwc, int obs_u8, const int64_t* act, const void* obs_next_nhwc, int64_t B, float* mse_out,
                       float* act_hat_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_icm_cnn_forward: workspace is NULL");
    TS_REQUIRE(params && obs_nhwc && act && obs_next_nhwc && mse_out, TS_ERR_INVALID_ARG, "ts_icm_cnn_forward: NULL argument");
    IcmCnn m;
    if (int rc = make_icm_cnn(c, h, w, model_net, n_act, B, "ts_icm_cnn_forward", &m)) return rc;
    if (int rc = cnn_check_frames(obs_nhwc, obs_next_nhwc, "ts_icm_cnn_forward")) return rc;
    const bool inverse = act_hat_out != nullptr;
    const int n_blocks = (int)ts::ceil_div(B, LOSS_ROWS);
    if (int rc = ts::ws_reserve(ws, cnn_fwd_bytes(m, B, inverse) + al(8 * (size_t)n_blocks) + 8192)) return rc;
    hipStream_t s = ts::as_stream(stream);
    Carve cv{static_cast<char*>(ws->base)};
    FwdCnn f;
    if (int rc = icm_cnn_forward_pass(s, ws, m, params, obs_nhwc, obs_u8 != 0, act, obs_next_nhwc, B, inverse, cv, &f)) return rc;
    float* partial = cv.f(2 * (size_t)n_blocks);
    hipLaunchKernelGGL(icm_loss_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, f.p2h, m.F, f.phi + B * m.F, m.F, (const float*)nullptr, 0,
                       act, B, m.F, m.A, 0.f, 0.f, mse_out, (float*)nullptr, 0, (float*)nullptr, 0, partial);
    if (inverse) hipLaunchKernelGGL(icm_unpad_kernel, dim3(blocks_of(B * m.A)), dim3(256), 0, s, f.logits, B, m.A, m.Ap, act_hat_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_icm_cnn_reward(ts_workspace* ws, const float* params, int64_t c, int64_t h, int64_t w, const ts_net_desc* model_net, int64_t n_act,
                      const void* obs_nhwc, int obs_u8, const int64_t* act, const void* obs_next_nhwc, int64_t B, const double* rew,
                      double reward_scale, double* rew_out, float* mse_out, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_icm_cnn_reward: workspace is NULL");
    TS_REQUIRE(params && obs_nhwc && act && obs_next_nhwc && rew && rew_out, TS_ERR_INVALID_ARG, "ts_icm_cnn_reward: NULL argument");
    IcmCnn m;
    if (int rc = make_icm_cnn(c, h, w, model_net, n_act, B, "ts_icm_cnn_reward", &m)) return rc;
    if (int rc = cnn_check_frames(obs_nhwc, obs_next_nhwc, "ts_icm_cnn_reward")) return rc;
    const int n_blocks = (int)ts::ceil_div(B, LOSS_ROWS);
    if (int rc = ts::ws_reserve(ws, cnn_fwd_bytes(m, B, false) + al(8 * (size_t)n_blocks) + al(4 * B) + 8192)) return rc;
    hipStream_t s = ts::as_stream(stream);
    Carve cv{static_cast<char*>(ws->base)};
    FwdCnn f;
    if (int rc = icm_cnn_forward_pass(s, ws, m, params, obs_nhwc, obs_u8 != 0, act, obs_next_nhwc, B, false, cv, &f)) return rc;
    float* partial = cv.f(2 * (size_t)n_blocks);
    float* mse = mse_out ? mse_out : cv.f(B);
    hipLaunchKernelGGL(icm_loss_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, f.p2h, m.F, f.phi + B * m.F, m.F, (const float*)nullptr, 0,
                       act, B, m.F, m.A, 0.f, 0.f, mse, (float*)nullptr, 0, (float*)nullptr, 0, partial);
    hipLaunchKernelGGL(icm_reward_kernel, dim3(blocks_of(B)), dim3(256), 0, s, rew, mse, B, (float)reward_scale, rew_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_icm_cnn_grad(ts_workspace* ws, const float* params, int64_t c, int64_t h, int64_t w, const ts_net_desc* model_net, int64_t n_act,
                    const void* obs_nhwc, int obs_u8, const int64_t* act, const void* obs_next_nhwc, int64_t B, int64_t B_total,
                    double forward_loss_weight, double lr_scale, int accumulate, float* grad, float* sums2, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_icm_cnn_grad: workspace is NULL");
    TS_REQUIRE(params && obs_nhwc && act && obs_next_nhwc && grad && sums2, TS_ERR_INVALID_ARG, "ts_icm_cnn_grad: NULL argument");
    TS_REQUIRE(B >= 1 && B <= B_total, TS_ERR_INVALID_ARG, "ts_icm_cnn_grad: 1 <= B <= B_total (got %lld, %lld)", (long long)B,
               (long long)B_total);
    IcmCnn m;
    if (int rc = make_icm_cnn(c, h, w, model_net, n_act, B, "ts_icm_cnn_grad", &m)) return rc;
    if (int rc = cnn_check_frames(obs_nhwc, obs_next_nhwc, "ts_icm_cnn_grad")) return rc;
    const int n_blocks = (int)ts::ceil_div(B, LOSS_ROWS);
    const size_t sl = std::max(slab_floats(m.fwd), slab_floats(m.inv));
    const size_t dh = std::max(hidden_grad_floats(m.fwd, B), hidden_grad_floats(m.inv, B));
    size_t conv_sl[3], bytes = cnn_fwd_bytes(m, B, true) + al(8 * (size_t)n_blocks) + al(4 * B * m.F) + al(4 * B * m.Ap) + al(4 * B * m.KF) +
                               al(4 * B * m.KI) + 2 * al(4 * dh) + al(4 * sl) + (accumulate ? al(4 * m.P) : 0) + 16384;
    for (int i = 0; i < 3; ++i) {
        conv_sl[i] = (size_t)ts::conv_wgrad_splits(m.cv[i]) * m.cv[i].param_elems();
        bytes += al(4 * conv_sl[i]) + al(4 * (size_t)m.cv[i].out_elems());
    }
    if (int rc = ts::ws_reserve(ws, bytes)) return rc;
    hipStream_t s = ts::as_stream(stream);
    Carve cv{static_cast<char*>(ws->base)};
    FwdCnn f;
    if (int rc = icm_cnn_forward_pass(s, ws, m, params, obs_nhwc, obs_u8 != 0, act, obs_next_nhwc, B, true, cv, &f)) return rc;
    float* partial = cv.f(2 * (size_t)n_blocks);
    float* d_p2h = cv.f(B * m.F);
    float* d_logits = cv.f(B * m.Ap);
    float* dxf = cv.f(B * m.KF);
    float* dxi = cv.f(B * m.KI);
    float* dha = cv.f(dh);
    float* dhb = cv.f(dh);
    float* slabs = cv.f(sl);
    float* g = accumulate ? cv.f(m.P) : grad;            // this chunk's gradient
    float *dy[3], *cslab[3];
    for (int i = 0; i < 3; ++i) { dy[i] = cv.f((size_t)m.cv[i].out_elems()); cslab[i] = cv.f(conv_sl[i]); }
    const double wt = forward_loss_weight;
    hipLaunchKernelGGL(icm_loss_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, f.p2h, m.F, f.phi + B * m.F, m.F, f.logits, m.Ap, act, B,
                       m.F, m.A, (float)(wt * lr_scale / (double)B_total), (float)((1.0 - wt) * lr_scale / (double)B_total), (float*)nullptr,
                       d_p2h, m.F, d_logits, m.Ap, partial);
    hipLaunchKernelGGL(icm_cnn_sums_kernel, dim3(1), dim3(256), 0, s, partial, n_blocks, accumulate, sums2);
    TS_LAUNCH_CHECK();
    if (int rc = chain_backward(s, ws, m.fwd, params, f.xf, f.aw, d_p2h, g, dha, dhb, slabs, B, dxf, m.F)) return rc;
    if (int rc = chain_backward(s, ws, m.inv, params, f.xi, f.ai, d_logits, g, dha, dhb, slabs, B, dxi, 2 * m.F)) return rc;
    hipLaunchKernelGGL(icm_cnn_merge_kernel, dim3(blocks_of(2 * B * (m.F / 4))), dim3(256), 0, s, dxf, m.KF, dxi, m.KI, d_p2h, f.phi, B, m.F,
                       dy[2]);
    TS_LAUNCH_CHECK();
    const float* x[3] = {static_cast<const float*>(f.x0), f.a[0], f.a[1]};
    const float* wb[3] = {params + m.coff[0], params + m.coff[1], params + m.coff[2]};
    float* gl[3] = {g + m.coff[0], g + m.coff[1], g + m.coff[2]};
    if (int rc = ts::chain_backward(s, ws, 3, m.cv, x, dy, wb, cslab, gl, obs_u8 != 0)) return rc;
    if (accumulate) {
        hipLaunchKernelGGL(icm_cnn_accum_kernel, dim3(blocks_of(m.P / 4)), dim3(256), 0, s, grad, g, m.P / 4);
        TS_LAUNCH_CHECK();
    }
    return TS_OK;
}

int ts_icm_cnn_apply(ts_workspace* ws, float* params, float* state_m, float* state_v, int64_t optim_step, int64_t c, int64_t h, int64_t w,
                     const ts_net_desc* model_net, int64_t n_act, const float* grad, const float* sums2, int64_t B_total,
                     double forward_loss_weight, double lr_scale, int32_t optim_kind, double lr, double beta1, double beta2, double eps,
                     double weight_decay, double rms_alpha, double rms_momentum, int32_t rms_centered, double max_grad_norm,
                     float* stats_out3, ts_stream_t stream) {
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_icm_cnn_apply: workspace is NULL");
    TS_REQUIRE(params && state_m && state_v && grad && sums2 && stats_out3, TS_ERR_INVALID_ARG, "ts_icm_cnn_apply: NULL argument");
    TS_REQUIRE(B_total >= 1 && optim_step >= 1 && (optim_kind == TS_OPT_ADAM || optim_kind == TS_OPT_RMSPROP), TS_ERR_INVALID_ARG,
               "ts_icm_cnn_apply: B_total >= 1, optim_step >= 1, optim_kind Adam or RMSprop");
    IcmCnn m;
    if (int rc = make_icm_cnn(c, h, w, model_net, n_act, 1, "ts_icm_cnn_apply", &m)) return rc;
    if (int rc = ts::ws_reserve(ws, al(4 * 1024) + 4096)) return rc;
    hipStream_t s = ts::as_stream(stream);
    hipLaunchKernelGGL(icm_loss_finish_kernel, dim3(1), dim3(256), 0, s, sums2, 1, (float)B_total, (float)forward_loss_weight, (float)lr_scale,
                       stats_out3);
    TS_LAUNCH_CHECK();
    if (lr < 0.0) return TS_OK;
    ts::OptimDesc o;
    o.kind = optim_kind; o.centered = rms_centered; o.weight_decay = weight_decay; o.alpha = rms_alpha; o.momentum = rms_momentum;
    return ts::optim_step(s, o, params, state_m, state_v, grad, m.P, optim_step, lr, beta1, beta2, eps, max_grad_norm,
                          static_cast<float*>(ws->base));
}

}  // extern "C"
