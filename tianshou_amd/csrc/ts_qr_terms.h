// ts_qr_terms.h -- the inner sums of the quantile-Huber loss (qrdqn.py:111-128), shared by qr_loss_kernel / cql_loss_kernel
// (ts_distq.hip) and the in-tile pair loss of ts_qrdqn_mlp.hip.  Include behind `#pragma clang fp contract(off)`.
#pragma once

#include <hip/hip_runtime.h>

namespace {

// The quantile-Huber terms of one theta_i against the N targets T_j, d_ij = T_j - theta_i, l_ij = smooth_l1(d_ij),
// w_ij = |tau_i - 1{d_ij <= 0}|:  li = sum_j l_ij w_ij,  ai = sum_j l_ij,  g = sum_j w_ij clamp(d_ij, -1, 1)
__device__ __forceinline__ void qr_terms(const float* T, int N, float theta, float tau, float& li, float& ai, float& g) {
    float gc = 0.f;                                        // gc: compensation of g (Kahan)
    li = 0.f; ai = 0.f; g = 0.f;
    for (int j = 0; j < N; ++j) {
        const float d = T[j] - theta, ad = fabsf(d);
        const bool quad = ad < 1.f;
        const float l = quad ? 0.5f * d * d : ad - 0.5f;
        const float w = fabsf(tau - (d <= 0.f ? 1.f : 0.f));
        li += l * w;
        ai += l;
        // in the linear region the N terms are all +-w: added one after the other they round the same way every time
        // and the error grows with N (27 ulp of the sum at N = 255), so the gradient sum is compensated
        const float y = w * (quad ? d : (d > 0.f ? 1.f : -1.f)) - gc, t = g + y;
        gc = (t - g) - y;
        g = t;
    }
}

}  // namespace
