// ts_bc.h -- device helpers of the behaviour-cloning cross-entropy (imitation/imitation_base.py:119-122), shared by the DQNet
// route (ts_dqn.hip: fused with the dense head backward) and the raw-array / MLP route (ts_sac.hip).
//
// A row's softmax is kept as two numbers, its maximum m and s = sum_c exp(x_c - m), which ONE thread takes serially in the order
// c = 0 .. A - 1 (bc_row_stats): no cross-lane traffic, and every kernel that needs the row gets the same bits.  (A wavefront
// per row with butterfly reductions was measured first: thirteen dependent cross-lane operations per row made the fused head
// kernel 128 us at B = 512, twenty times DQN's.)  Everything else is per element and independent from row to row.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ts {

constexpr int BC_MAX_ACT = 64;

struct BcRow { float m, s; };

__device__ __forceinline__ BcRow bc_row_stats(const float* __restrict__ row, int A) {
    float m = row[0];
#pragma unroll 8
    for (int c = 1; c < A; ++c) m = fmaxf(m, row[c]);          // (unrolled: the loads of a row go out together)
    float s = 0.f;
#pragma unroll 8
    for (int c = 0; c < A; ++c) s += expf(row[c] - m);
    return BcRow{m, s};
}

// nll = log s - (x_act - m)  (F.nll_loss(F.log_softmax(.))).  `act` is range-checked before it is used as an index: outside
// [0, A) nothing is read and the result is NaN (torch raises there).
__device__ __forceinline__ float bc_row_nll(const float* __restrict__ row, int A, int64_t act, BcRow r) {
    if (act < 0 || act >= (int64_t)A) return __builtin_nanf("");
    return logf(r.s) - (row[act] - r.m);
}

// softmax_a - 1{a = act} for the element x = row[a]; NaN for an `act` outside [0, A) (compared, never an index)
__device__ __forceinline__ float bc_elem_grad(float x, int a, int A, int64_t act, BcRow r) {
    if (act < 0 || act >= (int64_t)A) return __builtin_nanf("");
    return expf(x - r.m) / r.s - ((int64_t)a == act ? 1.f : 0.f);
}

// mean over B of the rows' nll by one workgroup of 256 threads: thread t adds rows t, t + 256, ... in order, a shuffle tree per
// wavefront, then the four wave sums in order.  `red`: four floats of LDS.  Thread 0 returns the mean.
__device__ __forceinline__ float bc_block_mean_nll(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ act,
                                                   int64_t B, int A, float* red) {
    float acc = 0.f;
    for (int64_t b = threadIdx.x; b < B; b += 256) {
        const float* row = logits + b * ld;
        acc += bc_row_nll(row, A, act[b], bc_row_stats(row, A));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((red[0] + red[1]) + (red[2] + red[3])) / (float)B;
}

}  // namespace ts
