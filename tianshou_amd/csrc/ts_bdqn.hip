// ts_bdqn.hip -- Branching Dueling Q-Network (arXiv 1711.08946) for gfx950.
//
// Replaces, on device-resident batches:
//   BranchingNet.forward                     tianshou/utils/net/common.py:658-674    q = v + adv - mean_a adv
//   BDQN._target_q / _compute_return         tianshou/algorithm/modelfree/bdqn.py:155-195   1-step, mean over the branches
//   BDQN._update_with_batch                  bdqn.py:206-224                          one Optimizer.step
//
// Route: the common chain runs layer by layer on the fp32-MFMA GEMM kernels of ts_conv.hip.  The first layers of `value` and of
// all D branches read the same input, so where they exist they are ONE "fan" GEMM of pad32(Hv) + D pad32(Ha) columns (forward,
// input gradient and weight gradient once each).  The D + 1 last Linears -- the heads -- are the kernels of this file: one
// wavefront per sample, head d reading a column segment of its input matrix (the fan's output, or the common output where a
// net has no hidden layer).  Head weight gradients go to slabs that ts::slab_sum adds in a fixed order: no atomics anywhere.
#include <algorithm>

#include "ts_common.h"
#include "ts_conv.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXL = TS_NET_MAX_HIDDEN;              // linear layers of the common chain
constexpr int ROWS = 4;                              // samples per workgroup of the head kernels: one wavefront each
constexpr int WG_ROWS = 32;                          // samples per slab of the head weight gradient

int pad32(int64_t v) { return (int)((v + 31) / 32 * 32); }
size_t al(size_t x) { return (x + 255) & ~size_t(255); }
unsigned blocks_of(int64_t n) { return (unsigned)ts::ceil_div(n, 256); }

struct Carve {
    char* p;
    float* f(size_t n) { float* r = reinterpret_cast<float*>(p); p += al(4 * n); return r; }
};

// What the head kernels need to know; value and branches may read different matrices (one of them the fan's output, the other
// the common output).  Gradient buffers w.r.t. those inputs mirror their pitches and offsets.
struct Heads {
    int D, A, Np;                 // Np = pad32(A): columns of a branch head block
    int Kv, Kvp, pv;              // value head: input width, padded, row pitch of its input matrix (segment at column 0)
    int Ka, Kap, pa, a_off, a_stride;   // branch d reads columns [a_off + d a_stride, .. + Ka)
    int64_t blk;                  // floats of one branch head block: (Kap + 1) Np
    int shared;                   // both read the common output (no hidden layer in either net)
    int act;                      // activation that produced the inputs (the mask of the input gradient)
};

struct Model {
    ts::ConvGeom l[MAXL], fan;
    int64_t off[MAXL + 1];        // common layers; off[L] = the fan block (if any)
    int64_t fan_off, vhead_off, ahead_off, P, head_total;
    int L, act, od, k0, Hc, Hcp, Hv, Hvp, Ha, Hap, Nf, wmax;
    int width[MAXL + 1];
    Heads h;
};

int make_model(const ts_net_desc* net, int64_t value_hidden, int64_t action_hidden, int64_t D, int64_t A, int64_t B, const char* who,
               Model* m) {
    TS_REQUIRE(net != nullptr, TS_ERR_INVALID_ARG, "%s: the network descriptor is NULL", who);
    TS_REQUIRE(B >= 1 && B <= (int64_t)1 << 29, TS_ERR_INVALID_ARG, "%s: 1 <= B <= 2^29", who);
    TS_REQUIRE(net->obs_dim >= 1 && net->obs_dim <= 65536 && D >= 1 && A >= 1 && value_hidden >= 0 && action_hidden >= 0,
               TS_ERR_INVALID_ARG, "%s: obs_dim in [1, 65536], num_branches >= 1, action_per_branch >= 1, hidden widths >= 0", who);
    TS_REQUIRE(net->n_hidden >= 1 && net->n_hidden <= TS_NET_MAX_HIDDEN, TS_ERR_UNSUPPORTED,
               "%s: the common net has 1 .. %d hidden layers (got %d)", who, TS_NET_MAX_HIDDEN, (int)net->n_hidden);
    TS_REQUIRE(D <= TS_BDQN_MAX_BRANCHES && A <= TS_BDQN_MAX_ACTIONS, TS_ERR_UNSUPPORTED,
               "%s: at most %d branches of at most %d actions (got %lld x %lld)", who, TS_BDQN_MAX_BRANCHES, TS_BDQN_MAX_ACTIONS,
               (long long)D, (long long)A);
    TS_REQUIRE(net->activation == TS_NET_ACT_RELU || net->activation == TS_NET_ACT_TANH, TS_ERR_UNSUPPORTED,
               "%s: the activation must be ReLU or tanh", who);
    TS_REQUIRE(net->flags == 0, TS_ERR_UNSUPPORTED, "%s: layer norm / conditioned sigma are not part of a BranchingNet here", who);
    TS_REQUIRE(value_hidden <= 1024 && action_hidden <= 1024, TS_ERR_UNSUPPORTED,
               "%s: value / action hidden widths up to 1024 (0 = no hidden layer)", who);
    for (int i = 0; i < net->n_hidden; ++i)
        TS_REQUIRE(net->hidden[i] >= 1 && net->hidden[i] <= 1024, TS_ERR_UNSUPPORTED, "%s: hidden widths must be in [1, 1024]", who);
    m->L = net->n_hidden; m->act = net->activation; m->od = (int)net->obs_dim;
    m->width[0] = m->k0 = pad32(net->obs_dim);
    m->wmax = m->k0;
    int64_t o = 0;
    for (int i = 0; i < m->L; ++i) {
        m->width[i + 1] = pad32(net->hidden[i]);
        m->l[i] = ts::ConvGeom{(int)B, 1, 1, m->width[i], 1, 1, 1, 1, 1, m->width[i + 1]};
        m->off[i] = o;
        o += m->l[i].param_elems();
        m->wmax = std::max(m->wmax, m->width[i + 1]);
    }
    m->off[m->L] = o;
    m->Hc = (int)net->hidden[m->L - 1]; m->Hcp = m->width[m->L];
    m->Hv = (int)value_hidden; m->Hvp = pad32(value_hidden);
    m->Ha = (int)action_hidden; m->Hap = pad32(action_hidden);
    m->Nf = m->Hvp + (int)D * m->Hap;
    m->fan_off = o;
    if (m->Nf > 0) {
        m->fan = ts::ConvGeom{(int)B, 1, 1, m->Hcp, 1, 1, 1, 1, 1, m->Nf};
        o += m->fan.param_elems();
        m->wmax = std::max(m->wmax, m->Nf);
    }
    Heads& h = m->h;
    h.D = (int)D; h.A = (int)A; h.Np = pad32(A); h.act = m->act;
    h.Kv = m->Hv ? m->Hv : m->Hc; h.Kvp = pad32(h.Kv); h.pv = m->Hv ? m->Nf : m->Hcp;
    h.Ka = m->Ha ? m->Ha : m->Hc; h.Kap = pad32(h.Ka); h.pa = m->Ha ? m->Nf : m->Hcp;
    h.a_off = m->Ha ? m->Hvp : 0; h.a_stride = m->Hap;
    h.blk = (int64_t)(h.Kap + 1) * h.Np;
    h.shared = !m->Hv && !m->Ha;
    m->vhead_off = o;
    m->ahead_off = o + (int64_t)(h.Kvp + 1) * 32;
    m->head_total = (int64_t)(h.Kvp + 1) * 32 + D * h.blk;
    m->P = m->vhead_off + m->head_total;
    // (the GEMM kernels index with 32 bits: the widest activation matrix must stay below 2^31 elements)
    TS_REQUIRE(B * (int64_t)m->wmax < ((int64_t)1 << 31), TS_ERR_INVALID_ARG,
               "%s: B x the widest layer (%d) must stay below 2^31 elements (split the batch)", who, m->wmax);
    return TS_OK;
}

// ---- elementwise kernels ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bdqn_tanh_kernel(float* __restrict__ h, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) h[i] = tanhf(h[i]);
}
__device__ __forceinline__ float act_mask(float s, float h, int act) { return act == TS_NET_ACT_TANH ? s * (1.f - h * h) : (h > 0.f ? s : 0.f); }
// dh = dh * act'(h) + add (h is the layer's OUTPUT; add nullable: a part of the gradient that is already masked)
__global__ __launch_bounds__(256) void bdqn_act_bwd_kernel(float* __restrict__ dh, const float* __restrict__ h, const float* __restrict__ add,
                                                            int64_t n, int act) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = act_mask(dh[i], h[i], act);
    dh[i] = add ? v + add[i] : v;
}
// x[b, :] = obs[b] zero-padded to k0 columns
__global__ __launch_bounds__(256) void bdqn_pad_kernel(const float* __restrict__ obs, int64_t B, int od, int k0, float* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B * k0) return;
    const int64_t r = i / k0;
    const int j = (int)(i - r * k0);
    x[i] = j < od ? obs[r * od + j] : 0.f;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- the heads ----------------------------------------------------------------------------------------------------------------
// One wavefront per sample, ROWS samples per workgroup.  v = xv[b, :Kv] . wv + bias; adv[d, a] = xa[b, seg_d] . W_d[:, a] + bias
// (lane o = d A + a, o += 64: lanes of one branch read one weight row coalesced, the input value is a broadcast); then per
// branch (lane d) the mean over a in index order, q = v + (adv - mean) (the reference's order of operations) and the argmax
// over q with a strict comparison: ties take the lowest index.  q_out / act_out nullable.
__global__ __launch_bounds__(256) void bdqn_head_forward_kernel(Heads h, const float* __restrict__ xv, const float* __restrict__ xa,
                                                                const float* __restrict__ wv, const float* __restrict__ wa, int64_t B,
                                                                float* __restrict__ q_out, int64_t* __restrict__ act_out) {
    __shared__ float adv[ROWS][TS_BDQN_MAX_BRANCHES * TS_BDQN_MAX_ACTIONS];
    __shared__ float mean[ROWS][TS_BDQN_MAX_BRANCHES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * ROWS + wave;
    const bool on = b < B;                                   // (uniform per wavefront; every wavefront reaches the barriers)
    const int DA = h.D * h.A;
    float v = 0.f;
    if (on) {
        float p = 0.f;
        const float* x = xv + b * h.pv;
        for (int k = lane; k < h.Kv; k += 64) p += x[k] * wv[(int64_t)k * 32];
        v = wave_sum(p) + wv[(int64_t)h.Kvp * 32];
        for (int o = lane; o < DA; o += 64) {
            const int d = o / h.A, a = o - d * h.A;
            const float* xs = xa + b * h.pa + h.a_off + d * h.a_stride;
            const float* w = wa + d * h.blk + a;
            float acc = 0.f;
#pragma unroll 4
            for (int k = 0; k < h.Ka; ++k) acc += xs[k] * w[(int64_t)k * h.Np];
            adv[wave][o] = acc + w[(int64_t)h.Kap * h.Np];
        }
    }
    __syncthreads();
    if (on && lane < h.D) {
        const float* r = adv[wave] + lane * h.A;
        float s = 0.f;
        for (int a = 0; a < h.A; ++a) s += r[a];
        const float mu = s / (float)h.A;
        mean[wave][lane] = mu;
        if (act_out) {
            int best = 0;
            float qb = v + (r[0] - mu);
            for (int a = 1; a < h.A; ++a) {
                const float qa = v + (r[a] - mu);
                if (qa > qb) { qb = qa; best = a; }
            }
            act_out[b * h.D + lane] = best;
        }
    }
    __syncthreads();
    if (on && q_out)
        for (int o = lane; o < DA; o += 64) q_out[b * DA + o] = v + (adv[wave][o] - mean[wave][o / h.A]);
}

// One wavefront per sample: lane d < D takes branch d.  a* = act[b, d] clamped into [0, A); td = ret - q[b, d, a*];
// prio[b] = sum_d td (signed); loss partial of the workgroup = sum over its rows of w mean_d td^2 (rows in order);
// g[b, d] = dL/dq[b, d, a*] = -2 w td / (B D); dV[b] = sum_d g; dq_out (nullable, dense [B, D, A]) = g at a*, 0 elsewhere.
// With head weights (wv != NULL) the gradient w.r.t. the heads' inputs, masked by the activation that produced them:
//   dAdv[d, a] = g[d] ((a == a*) - 1/A);  branch input: sum_a dAdv[d, a] W_d[k, a];  value input: dV wv[k];
// written to dxv / dxa with the pitches and offsets of xv / xa, padding columns of every segment zero.  h.shared: both read
// the common output, the sum of both goes to dxa.
__global__ __launch_bounds__(256) void bdqn_head_backward_kernel(Heads h, const float* __restrict__ q, const float* __restrict__ ret,
                                                                 const int64_t* __restrict__ act, const float* __restrict__ wgt, int64_t B,
                                                                 float coef, const float* __restrict__ xv, const float* __restrict__ xa,
                                                                 const float* __restrict__ wv, const float* __restrict__ wa,
                                                                 float* __restrict__ prio, float* __restrict__ partial,
                                                                 float* __restrict__ dq_out, float* __restrict__ g_out,
                                                                 int* __restrict__ a_out, float* __restrict__ dv_out,
                                                                 float* __restrict__ dxv, float* __restrict__ dxa) {
    __shared__ float gs[ROWS][TS_BDQN_MAX_BRANCHES];
    __shared__ int as[ROWS][TS_BDQN_MAX_BRANCHES];
    __shared__ float red[ROWS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * ROWS + wave;
    const bool on = b < B;
    const int DA = h.D * h.A;
    float dV = 0.f, lb = 0.f;
    if (on) {
        float td = 0.f, g = 0.f;
        const float w = wgt ? wgt[b] : 1.f;
        if (lane < h.D) {
            int64_t a = act[b * h.D + lane];
            a = a < 0 ? 0 : (a >= h.A ? h.A - 1 : a);
            td = ret[b] - q[b * DA + lane * h.A + a];
            g = -(coef * w) * td;
            gs[wave][lane] = g;
            as[wave][lane] = (int)a;
            if (g_out) { g_out[b * h.D + lane] = g; a_out[b * h.D + lane] = (int)a; }
        }
        const float p = wave_sum(td);
        lb = w * (wave_sum(td * td) / (float)h.D);
        dV = wave_sum(g);
        if (lane == 0) {
            prio[b] = p;
            if (dv_out) dv_out[b] = dV;
        }
    }
    if (lane == 0) red[wave] = on ? lb : 0.f;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    if (!on) return;
    if (dq_out)
        for (int o = lane; o < DA; o += 64) {
            const int d = o / h.A;
            dq_out[b * DA + o] = (o - d * h.A) == as[wave][d] ? gs[wave][d] : 0.f;
        }
    if (!wv) return;
    const float inv_a = 1.f / (float)h.A;
    if (h.a_stride > 0) {                                    // every branch has its own segment of the fan's output
        for (int d = 0; d < h.D; ++d) {
            const float g = gs[wave][d];
            const int sel = as[wave][d];
            const int64_t base = b * h.pa + h.a_off + d * h.a_stride;
            const float* w = wa + d * h.blk;
            for (int k = lane; k < h.Kap; k += 64) {
                float s = 0.f;
                if (k < h.Ka) {
                    const float* wr = w + (int64_t)k * h.Np;
                    for (int a = 0; a < h.A; ++a) s += (g * ((a == sel ? 1.f : 0.f) - inv_a)) * wr[a];
                    s = act_mask(s, xa[base + k], h.act);
                }
                dxa[base + k] = s;
            }
        }
    } else {                                                 // all branches read the common output: one sum over d and a
        const int64_t base = b * h.pa;
        for (int k = lane; k < h.Kap; k += 64) {
            float s = 0.f;
            if (k < h.Ka) {
                for (int d = 0; d < h.D; ++d) {
                    const float g = gs[wave][d];
                    const int sel = as[wave][d];
                    const float* wr = wa + d * h.blk + (int64_t)k * h.Np;
                    for (int a = 0; a < h.A; ++a) s += (g * ((a == sel ? 1.f : 0.f) - inv_a)) * wr[a];
                }
                if (h.shared) s += dV * wv[(int64_t)k * 32];
                s = act_mask(s, xa[base + k], h.act);
            }
            dxa[base + k] = s;
        }
    }
    if (!h.shared) {
        const int64_t base = b * h.pv;
        for (int k = lane; k < h.Kvp; k += 64) dxv[base + k] = k < h.Kv ? act_mask(dV * wv[(int64_t)k * 32], xv[base + k], h.act) : 0.f;
    }
}

// loss = (sum of the workgroups' partials) / B: thread t adds partials t, t + 256, ... then a fixed-order block sum
__global__ __launch_bounds__(256) void bdqn_loss_finish_kernel(const float* __restrict__ partial, int n_blocks, float n, float* __restrict__ loss) {
    __shared__ float red4[4];
    float v = 0.f;
    for (int i = threadIdx.x; i < n_blocks; i += 256) v += partial[i];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = ((red4[0] + red4[1]) + (red4[2] + red4[3])) / n;
}

// Slab s (blockIdx.y) of the head gradients over samples [s WG_ROWS', ...): element e of the head region (value head block
// [Kvp + 1, 32], column 0 in use; then D branch blocks [Kap + 1, Np]) = sum_b x[b, k] dOut[b, .] with x = 1 in the bias row;
// padding rows and columns are written as zero.  One thread per element, samples in index order.
__global__ __launch_bounds__(256) void bdqn_head_wgrad_kernel(Heads h, const float* __restrict__ xv, const float* __restrict__ xa,
                                                              const float* __restrict__ g, const int* __restrict__ asel,
                                                              const float* __restrict__ dv, int64_t B, int64_t rows, int64_t total,
                                                              float* __restrict__ slabs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t b0 = (int64_t)blockIdx.y * rows, b1 = b0 + rows < B ? b0 + rows : B;
    const int64_t nv = (int64_t)(h.Kvp + 1) * 32;
    float acc = 0.f;
    if (e < nv) {
        const int k = (int)(e / 32), c = (int)(e % 32);
        if (c == 0 && (k < h.Kv || k == h.Kvp))
            for (int64_t b = b0; b < b1; ++b) acc += (k < h.Kv ? xv[b * h.pv + k] : 1.f) * dv[b];
    } else {
        const int64_t r = e - nv;
        const int d = (int)(r / h.blk);
        const int64_t t = r - d * h.blk;
        const int k = (int)(t / h.Np), a = (int)(t % h.Np);
        if (a < h.A && (k < h.Ka || k == h.Kap)) {
            const float inv_a = 1.f / (float)h.A;
            const int64_t col = h.a_off + d * h.a_stride + k;
            for (int64_t b = b0; b < b1; ++b) {
                const float gd = g[b * h.D + d];
                acc += (k < h.Ka ? xa[b * h.pa + col] : 1.f) * (gd * ((asel[b * h.D + d] == a ? 1.f : 0.f) - inv_a));
            }
        }
    }
    slabs[(int64_t)blockIdx.y * total + e] = acc;
}

// BDQN._target_q + _compute_return: a*[b, d] = act_sel[b, d] or, with act_sel NULL, the lowest-index argmax of q_sel[b, d, :];
// ret[b] = rew[b] + gamma mean_d q_eval[b, d, a*] (1 - end[b]) (the mean in branch order)
__global__ __launch_bounds__(256) void bdqn_target_kernel(const float* __restrict__ q_sel, const int64_t* __restrict__ act_sel,
                                                          const float* __restrict__ q_eval, const float* __restrict__ rew,
                                                          const uint8_t* __restrict__ end, int64_t B, int D, int A, float gamma,
                                                          float* __restrict__ ret) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float s = 0.f;
    for (int d = 0; d < D; ++d) {
        const int64_t row = (b * D + d) * A;
        int best = 0;
        if (act_sel) {
            const int64_t a = act_sel[b * D + d];
            best = (int)(a < 0 ? 0 : (a >= A ? A - 1 : a));
        } else {
            float qb = q_sel[row];
            for (int a = 1; a < A; ++a) {
                const float v = q_sel[row + a];
                if (v > qb) { qb = v; best = a; }
            }
        }
        s += q_eval[row + best];
    }
    const float m = s / (float)D;
    ret[b] = end[b] ? rew[b] : rew[b] + gamma * m;
}

// ---- orchestration ------------------------------------------------------------------------------------------------------------
struct Fwd {
    float *x0, *hc[MAXL], *fan, *split;
    const float *xv, *xa;
};

size_t split_floats(const Model& m) {
    size_t s = 4;
    for (int i = 0; i < m.L; ++i) { const int ns = ts::conv_fwd_splits(m.l[i]); if (ns > 1) s = std::max(s, (size_t)ns * m.l[i].out_elems()); }
    if (m.Nf > 0) { const int ns = ts::conv_fwd_splits(m.fan); if (ns > 1) s = std::max(s, (size_t)ns * m.fan.out_elems()); }
    return s;
}
size_t fwd_bytes(const Model& m, int64_t B) {
    size_t s = al(4 * B * m.k0) + al(4 * split_floats(m));
    for (int i = 0; i < m.L; ++i) s += al(4 * B * m.width[i + 1]);
    return s + (m.Nf > 0 ? al(4 * B * m.Nf) : 0);
}
void take_fwd(Carve& c, const Model& m, int64_t B, Fwd* f) {
    f->x0 = c.f(B * m.k0);
    for (int i = 0; i < m.L; ++i) f->hc[i] = c.f(B * m.width[i + 1]);
    f->fan = m.Nf > 0 ? c.f(B * m.Nf) : nullptr;
    f->split = c.f(split_floats(m));
    f->xv = m.Hv ? f->fan : f->hc[m.L - 1];
    f->xa = m.Ha ? f->fan : f->hc[m.L - 1];
}

int layer_forward(hipStream_t s, ts_workspace* ws, const ts::ConvGeom& g, int act, const float* x, const float* wb, float* y, float* split,
                  int64_t B) {
    if (int rc = ts::conv_forward(s, g, x, wb, y, act == TS_NET_ACT_RELU, split, ws)) return rc;
    if (act == TS_NET_ACT_TANH) {
        const int64_t cnt = B * g.OC;
        hipLaunchKernelGGL(bdqn_tanh_kernel, dim3(blocks_of(cnt)), dim3(256), 0, s, y, cnt);
        TS_LAUNCH_CHECK();
    }
    return TS_OK;
}

// f->x0 (the padded observations) -> common chain -> fan -> heads; q_out / act_out nullable
int net_forward(hipStream_t s, ts_workspace* ws, const Model& m, const float* params, int64_t B, const Fwd& f, float* q_out, int64_t* act_out) {
    const float* in = f.x0;
    for (int i = 0; i < m.L; ++i) {
        if (int rc = layer_forward(s, ws, m.l[i], m.act, in, params + m.off[i], f.hc[i], f.split, B)) return rc;
        in = f.hc[i];
    }
    if (m.Nf > 0)
        if (int rc = layer_forward(s, ws, m.fan, m.act, in, params + m.fan_off, f.fan, f.split, B)) return rc;
    hipLaunchKernelGGL(bdqn_head_forward_kernel, dim3((unsigned)ts::ceil_div(B, ROWS)), dim3(256), 0, s, m.h, f.xv, f.xa, params + m.vhead_off,
                       params + m.ahead_off, B, q_out, act_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int pad_obs(hipStream_t s, const Model& m, const float* obs, int64_t B, float* x0) {
    hipLaunchKernelGGL(bdqn_pad_kernel, dim3(blocks_of(B * m.k0)), dim3(256), 0, s, obs, B, m.od, m.k0, x0);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int check_da(int64_t B, int64_t D, int64_t A, const char* who) {
    TS_REQUIRE(B >= 1 && B <= (int64_t)1 << 29 && D >= 1 && A >= 1, TS_ERR_INVALID_ARG, "%s: 1 <= B <= 2^29, D >= 1, A >= 1", who);
    TS_REQUIRE(D <= TS_BDQN_MAX_BRANCHES && A <= TS_BDQN_MAX_ACTIONS, TS_ERR_UNSUPPORTED,
               "%s: at most %d branches of at most %d actions (got %lld x %lld)", who, TS_BDQN_MAX_BRANCHES, TS_BDQN_MAX_ACTIONS,
               (long long)D, (long long)A);
    return TS_OK;
}

}  // namespace

extern "C" {

int ts_bdqn_layout(const ts_net_desc* common_net, int64_t value_hidden, int64_t action_hidden, int64_t num_branches,
                   int64_t action_per_branch, int64_t* h_out8) {
    TS_REQUIRE(h_out8 != nullptr, TS_ERR_INVALID_ARG, "ts_bdqn_layout: output is NULL");
    Model m;
    if (int rc = make_model(common_net, value_hidden, action_hidden, num_branches, action_per_branch, 1, "ts_bdqn_layout", &m)) return rc;
    h_out8[0] = m.P;
    h_out8[1] = m.fan_off; h_out8[2] = m.Nf;
    h_out8[3] = m.Hvp; h_out8[4] = m.Hap;
    h_out8[5] = m.vhead_off; h_out8[6] = m.ahead_off; h_out8[7] = m.h.blk;
    return TS_OK;
}

int ts_bdqn_forward(ts_workspace* ws, const float* params, const ts_net_desc* common_net, int64_t value_hidden, int64_t action_hidden,
                    int64_t num_branches, int64_t action_per_branch, const float* obs, int64_t B, float* q_out, int64_t* act_out,
                    ts_stream_t stream) {
    TS_REQUIRE(params && obs && (q_out || act_out), TS_ERR_INVALID_ARG, "ts_bdqn_forward: NULL argument");
    Model m;
    if (int rc = make_model(common_net, value_hidden, action_hidden, num_branches, action_per_branch, B, "ts_bdqn_forward", &m)) return rc;
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_bdqn_forward: workspace is NULL");
    if (int rc = ts::ws_reserve(ws, fwd_bytes(m, B) + 4096)) return rc;
    hipStream_t s = ts::as_stream(stream);
    Carve c{static_cast<char*>(ws->base)};
    Fwd f;
    take_fwd(c, m, B, &f);
    if (int rc = pad_obs(s, m, obs, B, f.x0)) return rc;
    return net_forward(s, ws, m, params, B, f, q_out, act_out);
}

int ts_bdqn_target(const float* q_sel, const float* q_eval, const float* rew, const uint8_t* end, int64_t B, int64_t D, int64_t A,
                   double gamma, float* ret_out, ts_stream_t stream) {
    TS_REQUIRE(q_sel && q_eval && rew && end && ret_out, TS_ERR_INVALID_ARG, "ts_bdqn_target: NULL argument");
    if (int rc = check_da(B, D, A, "ts_bdqn_target")) return rc;
    hipLaunchKernelGGL(bdqn_target_kernel, dim3(blocks_of(B)), dim3(256), 0, ts::as_stream(stream), q_sel, (const int64_t*)nullptr, q_eval,
                       rew, end, B, (int)D, (int)A, (float)gamma, ret_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_bdqn_loss(ts_workspace* ws, const float* q, const int64_t* act, const float* ret, const float* weight, int64_t B, int64_t D,
                 int64_t A, float* loss_out, float* prio_out, float* dq_out, ts_stream_t stream) {
    TS_REQUIRE(q && act && ret && loss_out && prio_out, TS_ERR_INVALID_ARG, "ts_bdqn_loss: NULL argument");
    if (int rc = check_da(B, D, A, "ts_bdqn_loss")) return rc;
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_bdqn_loss: workspace is NULL");
    const int n_blocks = (int)ts::ceil_div(B, ROWS);
    if (int rc = ts::ws_reserve(ws, al(4 * (size_t)n_blocks) + 4096)) return rc;
    float* partial = static_cast<float*>(ws->base);
    hipStream_t s = ts::as_stream(stream);
    Heads h{};
    h.D = (int)D; h.A = (int)A;
    const float* nf = nullptr;
    hipLaunchKernelGGL(bdqn_head_backward_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, h, q, ret, act, weight, B,
                       (float)(2.0 / ((double)B * (double)D)), nf, nf, nf, nf, prio_out, partial, dq_out, (float*)nullptr, (int*)nullptr,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(bdqn_loss_finish_kernel, dim3(1), dim3(256), 0, s, partial, n_blocks, (float)B, loss_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_bdqn_target_q(ts_workspace* ws, const float* params, const float* params_old, const ts_net_desc* common_net, int64_t value_hidden,
                     int64_t action_hidden, int64_t num_branches, int64_t action_per_branch, const float* obs_next, const float* rew,
                     const uint8_t* end, int64_t B, double gamma, int32_t is_double, float* ret_out, ts_stream_t stream) {
    TS_REQUIRE(params && obs_next && rew && end && ret_out, TS_ERR_INVALID_ARG, "ts_bdqn_target_q: NULL argument");
    Model m;
    if (int rc = make_model(common_net, value_hidden, action_hidden, num_branches, action_per_branch, B, "ts_bdqn_target_q", &m)) return rc;
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_bdqn_target_q: workspace is NULL");
    const int64_t DA = (int64_t)m.h.D * m.h.A;
    if (int rc = ts::ws_reserve(ws, fwd_bytes(m, B) + al(4 * B * DA) + al(8 * B * m.h.D) + 4096)) return rc;
    hipStream_t s = ts::as_stream(stream);
    Carve c{static_cast<char*>(ws->base)};
    Fwd f;
    take_fwd(c, m, B, &f);
    float* q_eval = c.f(B * DA);
    int64_t* a_sel = reinterpret_cast<int64_t*>(c.f(2 * B * m.h.D));
    if (int rc = pad_obs(s, m, obs_next, B, f.x0)) return rc;
    // the selecting network: the online one under double Q-learning, otherwise the evaluating one (bdqn.py:160-170)
    if (params_old != nullptr && is_double) {
        if (int rc = net_forward(s, ws, m, params, B, f, nullptr, a_sel)) return rc;
        if (int rc = net_forward(s, ws, m, params_old, B, f, q_eval, nullptr)) return rc;
    } else {
        if (int rc = net_forward(s, ws, m, params_old ? params_old : params, B, f, q_eval, a_sel)) return rc;
    }
    hipLaunchKernelGGL(bdqn_target_kernel, dim3(blocks_of(B)), dim3(256), 0, s, (const float*)nullptr, a_sel, q_eval, rew, end, B, m.h.D,
                       m.h.A, (float)gamma, ret_out);
    TS_LAUNCH_CHECK();
    return TS_OK;
}

int ts_bdqn_update(ts_workspace* ws, float* params, float* state_m, float* state_v, int64_t optim_step, const ts_net_desc* common_net,
                   int64_t value_hidden, int64_t action_hidden, int64_t num_branches, int64_t action_per_branch, const float* obs,
                   const int64_t* act, const float* ret, const float* weight, int64_t B, int32_t optim_kind, double lr, double beta1,
                   double beta2, double eps, double weight_decay, double rms_alpha, double rms_momentum, int32_t rms_centered,
                   double max_grad_norm, float* loss_out, float* prio_out, float* grad_out, ts_stream_t stream) {
    TS_REQUIRE(params && state_m && state_v && obs && act && ret && loss_out && prio_out, TS_ERR_INVALID_ARG,
               "ts_bdqn_update: NULL argument");
    TS_REQUIRE(optim_step >= 1 && (optim_kind == TS_OPT_ADAM || optim_kind == TS_OPT_RMSPROP), TS_ERR_INVALID_ARG,
               "ts_bdqn_update: optim_step >= 1, optim_kind Adam or RMSprop");
    Model m;
    if (int rc = make_model(common_net, value_hidden, action_hidden, num_branches, action_per_branch, B, "ts_bdqn_update", &m)) return rc;
    TS_REQUIRE(ws != nullptr, TS_ERR_WORKSPACE, "ts_bdqn_update: workspace is NULL");
    const Heads& h = m.h;
    const int64_t DA = (int64_t)h.D * h.A;
    const int n_blocks = (int)ts::ceil_div(B, ROWS);
    const int n_slab = (int)std::min<int64_t>(ts::ceil_div(B, WG_ROWS), 64);
    const int64_t slab_rows = ts::ceil_div(B, n_slab);
    size_t sl = (size_t)n_slab * m.head_total, dh = 4;
    for (int i = 0; i < m.L; ++i) {
        sl = std::max(sl, (size_t)ts::conv_wgrad_splits(m.l[i]) * m.l[i].param_elems());
        dh = std::max(dh, (size_t)B * m.width[i + 1]);
    }
    if (m.Nf > 0) sl = std::max(sl, (size_t)ts::conv_wgrad_splits(m.fan) * m.fan.param_elems());
    const size_t bytes = fwd_bytes(m, B) + al(4 * B * DA) + 2 * al(4 * B * h.D) + al(4 * B) + al(4 * (size_t)n_blocks) +
                         (m.Nf > 0 ? al(4 * B * m.Nf) : 0) + 3 * al(4 * dh) + al(4 * sl) + al(4 * m.P) + al(4 * 1024) + 16384;
    if (int rc = ts::ws_reserve(ws, bytes)) return rc;
    hipStream_t s = ts::as_stream(stream);
    Carve c{static_cast<char*>(ws->base)};
    Fwd f;
    take_fwd(c, m, B, &f);
    float* q = c.f(B * DA);
    float* g = c.f(B * h.D);
    int* asel = reinterpret_cast<int*>(c.f(B * h.D));
    float* dv = c.f(B);
    float* partial = c.f((size_t)n_blocks);
    float* dfan = m.Nf > 0 ? c.f(B * m.Nf) : nullptr;
    float* direct = c.f(dh);                                 // the part of d(common output) that does not pass through the fan
    float* dha = c.f(dh);
    float* dhb = c.f(dh);
    float* slabs = c.f(sl);
    float* grad = grad_out ? grad_out : c.f(m.P);
    float* norm_part = c.f(1024);
    if (int rc = pad_obs(s, m, obs, B, f.x0)) return rc;
    if (int rc = net_forward(s, ws, m, params, B, f, q, nullptr)) return rc;
    const float* wv = params + m.vhead_off;
    const float* wa = params + m.ahead_off;
    hipLaunchKernelGGL(bdqn_head_backward_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, h, q, ret, act, weight, B,
                       (float)(2.0 / ((double)B * (double)h.D)), f.xv, f.xa, wv, wa, prio_out, partial, (float*)nullptr, g, asel, dv,
                       m.Hv ? dfan : direct, m.Ha ? dfan : direct);
    hipLaunchKernelGGL(bdqn_loss_finish_kernel, dim3(1), dim3(256), 0, s, partial, n_blocks, (float)B, loss_out);
    hipLaunchKernelGGL(bdqn_head_wgrad_kernel, dim3(blocks_of(m.head_total), (unsigned)n_slab), dim3(256), 0, s, h, f.xv, f.xa, g, asel, dv, B,
                       slab_rows, m.head_total, slabs);
    TS_LAUNCH_CHECK();
    if (int rc = ts::slab_sum(s, slabs, n_slab, m.head_total, grad + m.vhead_off)) return rc;
    // d(common output), masked: through the fan (+ the direct part of a net without hidden layer), or the direct part alone
    const float* hc_out = f.hc[m.L - 1];
    const bool relu = m.act == TS_NET_ACT_RELU;
    float* dy = direct;
    if (m.Nf > 0) {
        if (int rc = ts::conv_wgrad(s, m.fan, hc_out, dfan, slabs, ws)) return rc;
        if (int rc = ts::slab_sum(s, slabs, ts::conv_wgrad_splits(m.fan), m.fan.param_elems(), grad + m.fan_off)) return rc;
        // (ReLU: conv_dgrad applies (h > 0) itself; the extra launch is left to tanh and to the direct part that has to be added)
        const bool mixed = !m.Hv || !m.Ha;
        const bool fused = relu && !mixed;
        if (int rc = ts::conv_dgrad(s, m.fan, dfan, params + m.fan_off, fused ? hc_out : nullptr, dha, ws)) return rc;
        if (!fused) {
            const int64_t cnt = B * m.Hcp;
            hipLaunchKernelGGL(bdqn_act_bwd_kernel, dim3(blocks_of(cnt)), dim3(256), 0, s, dha, hc_out, mixed ? direct : (const float*)nullptr,
                               cnt, m.act);
            TS_LAUNCH_CHECK();
        }
        dy = dha;
    }
    for (int i = m.L - 1; i >= 0; --i) {
        const float* xin = i == 0 ? f.x0 : f.hc[i - 1];
        if (int rc = ts::conv_wgrad(s, m.l[i], xin, dy, slabs, ws)) return rc;
        if (int rc = ts::slab_sum(s, slabs, ts::conv_wgrad_splits(m.l[i]), m.l[i].param_elems(), grad + m.off[i])) return rc;
        if (i > 0) {
            float* dx = (dy == dha) ? dhb : dha;
            if (int rc = ts::conv_dgrad(s, m.l[i], dy, params + m.off[i], relu ? f.hc[i - 1] : nullptr, dx, ws)) return rc;
            if (!relu) {
                const int64_t cnt = B * m.width[i];
                hipLaunchKernelGGL(bdqn_act_bwd_kernel, dim3(blocks_of(cnt)), dim3(256), 0, s, dx, f.hc[i - 1], (const float*)nullptr, cnt, m.act);
                TS_LAUNCH_CHECK();
            }
            dy = dx;
        }
    }
    if (lr < 0.0) return TS_OK;
    ts::OptimDesc o;
    o.kind = optim_kind; o.centered = rms_centered; o.weight_decay = weight_decay; o.alpha = rms_alpha; o.momentum = rms_momentum;
    return ts::optim_step(s, o, params, state_m, state_v, grad, m.P, optim_step, lr, beta1, beta2, eps, max_grad_norm, norm_part);
}

}  // extern "C"
