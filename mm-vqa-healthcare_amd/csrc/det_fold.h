// Deterministic mode: the ordered fold of per-workgroup partial rows (misc.hip: column sum and loss scalars; norm.hip:
// dgamma / dbeta).  Every workgroup of an ordered kernel stores its partial into a workspace row of its own instead of adding
// it with an atomic; this kernel then sums the rows in an order that depends on the row count alone.  One writer per output
// element.
#pragma once
#include "common.h"

namespace {

// out[i] (+)= scale * sum_b part[b * ld + i], i < n (out1 != nullptr: columns >= n0 go to out1[i - n0]; a caller without a
// second output folds the first n < ld columns of every row only).  CL column lanes x (256 / CL) row lanes per workgroup: row
// lane r adds rows r, r + RL, r + 2 RL, ... in ascending order, lane 0 adds the RL lane sums in ascending order.
template <int CL>
__global__ __launch_bounds__(256) void det_fold_kernel(const float* __restrict__ part, float* __restrict__ out0,
                                                       float* __restrict__ out1, int64_t count, int64_t n, int64_t ld,
                                                       int64_t n0, float scale, int accumulate) {
    constexpr int RL = 256 / CL;
    __shared__ float red[RL][CL + 1];
    const int cl = threadIdx.x % CL, rl = threadIdx.x / CL;
    const int64_t i = (int64_t)blockIdx.x * CL + cl;
    float s = 0.f;
    if (i < n)
        for (int64_t b = rl; b < count; b += RL) s += part[b * ld + i];
    red[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < RL; ++r) t += red[r][cl];
        float* o = (out1 && i >= n0) ? out1 + (i - n0) : out0 + i;
        *o = accumulate ? *o + t * scale : t * scale;
    }
}
inline void det_fold(const float* part, float* out0, float* out1, int64_t count, int64_t n, int64_t ld, int64_t n0, float scale,
                     int accumulate, hipStream_t s) {
    if (n <= 2) hipLaunchKernelGGL(det_fold_kernel<2>, dim3(1), dim3(256), 0, s, part, out0, out1, count, n, ld, n0, scale, accumulate);
    else hipLaunchKernelGGL(det_fold_kernel<32>, dim3((unsigned)cdiv(n, 32)), dim3(256), 0, s, part, out0, out1, count, n, ld, n0, scale, accumulate);
}

}  // namespace
