// ts_twin.h -- internal: the twin-head Atari network shared by ts_bcq.hip (DiscreteBCQ) and ts_crr.hip (DiscreteCRR).
//
// Two heads, each F -> 512 -> n_act, on ONE DQNet(features_only=True) trunk:
//   feat[b, :] = relu(conv3(relu(conv2(relu(conv1(obs[b]))))))        F = 64 * OH3 * OW3 features in (h, w, c) order
//   oq[b, :]   = relu(feat[b] @ Wq1 + bq1) @ Wq2 + bq2                the first head  (BCQ: Q;        CRR: the critic)
//   oi[b, :]   = relu(feat[b] @ Wi1 + bi1) @ Wi2 + bi2                the second head (BCQ: imitator; CRR: the actor)
// Flat parameter layout: conv1 | conv2 | conv3 | [Wq1; bq1] [F + 1, 512] | [Wq2; bq2] [513, ld] | [Wi1; bi1] [F + 1, 512] |
// [Wi2; bi2] [513, ld], ld = n_act rounded up to a multiple of 32 (GEMM tile width; the padding columns are and stay
// exactly zero).  This header holds the geometry, the activation / gradient carving of the workspace, the forward pass and
// the backward pass from the two head-output gradients to the flat gradient.  Everything here has internal linkage: include
// it inside no namespace, once per translation unit.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "ts_common.h"
#include "ts_conv.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int HIDDEN = 512;
constexpr int MAX_ACT = 64;

struct BNet {
    ts::ConvGeom l[7];          // conv1, conv2, conv3, Q fc1, Q fc2, I fc1, I fc2
    int64_t off[8];             // their starts and the total
    int F, n_act, ld;
    int64_t B;
};

int make_bnet(int64_t B, int64_t c, int64_t h, int64_t w, int64_t n_act, BNet* n) {
    TS_REQUIRE(c >= 1 && h >= 1 && w >= 1 && c < (1 << 16) && h < (1 << 16) && w < (1 << 16), TS_ERR_INVALID_ARG,
               "bcq: bad observation dimensions");
    TS_REQUIRE(n_act >= 1 && n_act <= MAX_ACT, TS_ERR_INVALID_ARG, "bcq: 1 <= n_act <= 64");
    TS_REQUIRE(B >= 1 && B < (1 << 24), TS_ERR_INVALID_ARG, "bcq: batch size must be in [1, 2^24)");
    static const int oc[3] = {32, 64, 64}, ks[3] = {8, 4, 3}, st[3] = {4, 2, 1};
    int ic = (int)c, ih = (int)h, iw = (int)w;
    for (int i = 0; i < 3; ++i) {
        TS_REQUIRE(ih >= ks[i] && iw >= ks[i], TS_ERR_INVALID_ARG, "bcq: observation too small for DQNet");
        n->l[i] = ts::ConvGeom{(int)B, ih, iw, ic, ks[i], ks[i], st[i], (ih - ks[i]) / st[i] + 1, (iw - ks[i]) / st[i] + 1, oc[i]};
        ic = oc[i]; ih = n->l[i].OH; iw = n->l[i].OW;
    }
    n->B = B;
    n->F = ic * ih * iw;
    TS_REQUIRE(B * std::max(n->F, HIDDEN) < (int64_t(1) << 31), TS_ERR_INVALID_ARG, "bcq: batch too large (B * features < 2^31)");
    n->n_act = (int)n_act;
    n->ld = ((int)n_act + 31) / 32 * 32;
    n->l[3] = n->l[5] = ts::ConvGeom{(int)B, 1, 1, n->F, 1, 1, 1, 1, 1, HIDDEN};
    n->l[4] = n->l[6] = ts::ConvGeom{(int)B, 1, 1, HIDDEN, 1, 1, 1, 1, 1, n->ld};
    int64_t o = 0;
    for (int i = 0; i < 7; ++i) { n->off[i] = o; o += n->l[i].param_elems(); }
    n->off[7] = o;
    return TS_OK;
}

size_t al(size_t x) { return (x + 255) & ~size_t(255); }

// activations of one pass: the trunk, the Q branch (hq, oq) and, where asked for, the imitator branch (hi, oi).  The two
// branches run side by side, so each has its own split buffer.
struct BActs { float* c[3]; float* hq; float* oq; float* hi; float* oi; float* split; float* split_i; };

size_t split_floats(const BNet& n) {
    size_t s = 4;
    for (int i = 0; i < 5; ++i) {
        const int ns = ts::conv_fwd_splits(n.l[i]);
        if (ns > 1) s = std::max(s, (size_t)ns * n.l[i].out_elems());
    }
    return s;
}

size_t acts_bytes(const BNet& n, bool imitator) {
    size_t s = al(4 * split_floats(n));
    for (int i = 0; i < 5; ++i) s += al(4 * (size_t)n.l[i].out_elems());
    if (imitator) s += al(4 * split_floats(n)) + al(4 * (size_t)n.l[5].out_elems()) + al(4 * (size_t)n.l[6].out_elems());
    return s;
}

char* carve_acts(const BNet& n, bool imitator, char* p, BActs* a) {
    auto take = [&](size_t floats) { float* r = reinterpret_cast<float*>(p); p += al(4 * floats); return r; };
    for (int i = 0; i < 3; ++i) a->c[i] = take((size_t)n.l[i].out_elems());
    a->hq = take((size_t)n.l[3].out_elems());
    a->oq = take((size_t)n.l[4].out_elems());
    a->split = take(split_floats(n));
    a->hi = a->oi = a->split_i = nullptr;
    if (imitator) {
        a->hi = take((size_t)n.l[5].out_elems());
        a->oi = take((size_t)n.l[6].out_elems());
        a->split_i = take(split_floats(n));
    }
    return p;
}

// what the backward pass needs beside the activations: d (layer outputs) | the two fc1 input gradients | wgrad slabs (one
// set per layer: they run side by side) | flat gradient
struct BBack { float* dy[7]; float* dxq; float* dxi; float* slabs[7]; float* grad; };

size_t back_bytes(const BNet& n) {
    size_t s = al(4 * (size_t)n.off[7]) + 2 * al(4 * (size_t)n.B * n.F);
    for (int i = 0; i < 7; ++i)
        s += al(4 * (size_t)n.l[i].out_elems()) + al(4 * (size_t)ts::conv_wgrad_splits(n.l[i]) * n.l[i].param_elems());
    return s;
}

char* carve_back(const BNet& n, char* p, BBack* k) {
    auto take = [&](size_t floats) { float* r = reinterpret_cast<float*>(p); p += al(4 * floats); return r; };
    for (int i = 0; i < 7; ++i) k->dy[i] = take((size_t)n.l[i].out_elems());
    k->dxq = take((size_t)n.B * n.F);
    k->dxi = take((size_t)n.B * n.F);
    for (int i = 0; i < 7; ++i) k->slabs[i] = take((size_t)ts::conv_wgrad_splits(n.l[i]) * n.l[i].param_elems());
    k->grad = take((size_t)n.off[7]);
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

// dfeat = (dx_q + dx_i) * 1{feat > 0}: the two fc1 input gradients meet at the shared features (float4 per thread)
__global__ __launch_bounds__(256) void bcq_dfeat_kernel(const float* __restrict__ dxq, const float* __restrict__ dxi,
                                                        const float* __restrict__ feat, int64_t n4, float* __restrict__ dfeat) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4 a = reinterpret_cast<const f32x4*>(dxq)[i], c = reinterpret_cast<const f32x4*>(dxi)[i];
    const f32x4 f = reinterpret_cast<const f32x4*>(feat)[i];
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = f[k] > 0.f ? a[k] + c[k] : 0.f;
    reinterpret_cast<f32x4*>(dfeat)[i] = o;
}

unsigned wave_blocks(int64_t B) { return (unsigned)ts::ceil_div(B, 4); }

// One pass: the trunk, the Q branch on `s` and (imitator) the imitator branch beside it on `si`; `s` has joined `si` on return.
int net_forward(hipStream_t s, hipStream_t si, ts_workspace* ws, const BNet& n, const float* params, const void* obs, bool obs_u8,
                bool imitator, const BActs& a, int slot) {
    const float* x = static_cast<const float*>(obs);
    for (int i = 0; i < 3; ++i) {
        if (int rc = ts::conv_forward(s, n.l[i], x, params + n.off[i], a.c[i], true, a.split, ws, i == 0 && obs_u8)) return rc;
        x = a.c[i];
    }
    if (imitator) {
        if (int rc = ts::stream_wait(ws, s, si, slot)) return rc;
        if (int rc = ts::conv_forward(si, n.l[5], a.c[2], params + n.off[5], a.hi, true, a.split_i, ws)) return rc;
        if (int rc = ts::conv_forward(si, n.l[6], a.hi, params + n.off[6], a.oi, false, a.split_i, ws)) return rc;
    }
    if (int rc = ts::conv_forward(s, n.l[3], a.c[2], params + n.off[3], a.hq, true, a.split, ws)) return rc;
    if (int rc = ts::conv_forward(s, n.l[4], a.hq, params + n.off[4], a.oq, false, a.split, ws)) return rc;
    if (imitator) return ts::stream_wait(ws, si, s, slot + 1);
    return TS_OK;
}

// The backward pass from k.dy[4] (d oq) and k.dy[6] (d oi), both [B, ld] and written on `s`, to the flat gradient `grad`.
// The input gradients of the two branches run down the caller's stream; the weight gradients of the two fc2 layers (one
// launch) and of the two fc1 layers (one launch) run beside them on the side streams sv / sw, each followed by its slab
// sums.  The trunk follows through ts::chain_backward, which joins both side streams at its end.
int twin_backward(hipStream_t s, hipStream_t sv, hipStream_t sw, ts_workspace* ws, const BNet& n, const float* params,
                  const void* obs_nhwc, bool obs_u8, const BActs& a, const BBack& k, float* grad) {
    float* const* dy = k.dy;
    float* const* slabs = k.slabs;
    auto wgrad_pair = [&](hipStream_t st, int iq, int ii, const float* xq, const float* xi) -> int {
        const ts::ConvGeom g[2] = {n.l[iq], n.l[ii]};
        const float* X[2] = {xq, xi};
        const float* dY[2] = {dy[iq], dy[ii]};
        float* sl[2] = {slabs[iq], slabs[ii]};
        if (int rc = ts::conv_wgrad_group(st, 2, g, X, dY, sl, ws)) return rc;
        const ts::SlabSeg segs[2] = {{slabs[iq], ts::conv_wgrad_splits(n.l[iq]), n.l[iq].param_elems(), grad + n.off[iq]},
                                     {slabs[ii], ts::conv_wgrad_splits(n.l[ii]), n.l[ii].param_elems(), grad + n.off[ii]}};
        return ts::slab_sum_multi(st, segs, 2);
    };
    if (int rc = ts::stream_wait(ws, s, sv, 12)) return rc;                                          // d Q, d logits
    if (int rc = wgrad_pair(sv, 4, 6, a.hq, a.hi)) return rc;
    if (int rc = ts::conv_dgrad(s, n.l[4], dy[4], params + n.off[4], a.hq, dy[3], ws)) return rc;    // ReLU masks: hq, hi
    if (int rc = ts::conv_dgrad(s, n.l[6], dy[6], params + n.off[6], a.hi, dy[5], ws)) return rc;
    if (int rc = ts::stream_wait(ws, s, sw, 13)) return rc;
    if (int rc = wgrad_pair(sw, 3, 5, a.c[2], a.c[2])) return rc;
    if (int rc = ts::conv_dgrad(s, n.l[3], dy[3], params + n.off[3], nullptr, k.dxq, ws)) return rc;   // no mask: summed first
    if (int rc = ts::conv_dgrad(s, n.l[5], dy[5], params + n.off[5], nullptr, k.dxi, ws)) return rc;
    const int64_t n4 = n.B * n.F / 4;                                                                // F is a multiple of 64
    hipLaunchKernelGGL(bcq_dfeat_kernel, dim3((unsigned)ts::ceil_div(n4, 256)), dim3(256), 0, s, k.dxq, k.dxi, a.c[2], n4, dy[2]);
    TS_LAUNCH_CHECK();
    const float* x[3]; const float* wb[3]; float* g[3];
    for (int i = 0; i < 3; ++i) {
        x[i] = i == 0 ? static_cast<const float*>(obs_nhwc) : a.c[i - 1];
        wb[i] = params + n.off[i];
        g[i] = grad + n.off[i];
    }
    return ts::chain_backward(s, ws, 3, n.l, x, dy, wb, slabs, g, obs_u8);
}

}  // namespace
