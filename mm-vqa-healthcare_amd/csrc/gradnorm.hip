// Global gradient norm for clipping and the non-finite step guard: per-segment sums of squares of the flat fp32 gradient buffer
// in double, and the one-workgroup kernel that turns them into {norm, clip coefficient, skip flag, counters} on the device.
//
// No atomics anywhere: the result is a function of (x, piece table) alone.
//   * sumsq_piece_kernel, one workgroup per piece [begin, end): every lane owns fixed positions of the piece (scalar head and tail
//     around a 16-byte-aligned interior), squares in double (exact: 48 bits of product fit 53) and adds in double from the first
//     add; lanes, then waves, combine in a fixed tree.  One double per piece goes to the caller's workspace.
//   * sumsq_fold_kernel, one wave per segment: the segment's pieces (adjacent rows of the workspace, CSR) are added in ascending
//     order -- 64 coalesced loads, then one serial chain over v_readlane.
//   * clip_finalize_kernel, one workgroup: wave 0 adds the segments in ascending index the same way.
// Only the adds round, so |got - exact| <= (len - 1) * 2^-53 * exact whatever the order, and no finite gradient overflows or
// underflows on the way to its norm (fp32 accumulation would read 3e19 as inf and 1e-25 as 0).
#include "common.h"
#include <math.h>

namespace {

constexpr int SQ_BLOCK = 256;

DEVINL double shfl_xor_f64(double v, int o) { return __shfl_xor(v, o, 64); }
DEVINL double sq(float v) { const double d = (double)v; return d * d; }

DEVINL double readlane_f64(double v, int k) {   // k wave-uniform: two v_readlane_b32
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, k), hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), k);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// ascending serial sum of v over lanes 0 .. cnt - 1 of the wave (cnt wave-uniform), continuing `acc`
DEVINL double wave_chain(double acc, double v, int cnt) {
    for (int k = 0; k < cnt; ++k) acc += readlane_f64(v, k);
    return acc;
}

__global__ __launch_bounds__(SQ_BLOCK) void sumsq_piece_kernel(const float* __restrict__ x, int64_t n,
                                                               const int64_t* __restrict__ pieces, double* __restrict__ ws) {
    __shared__ double red[SQ_BLOCK / 64];
    int64_t b = pieces[2 * (int64_t)blockIdx.x], e = pieces[2 * (int64_t)blockIdx.x + 1];
    if (b < 0) b = 0;            // a table that lies about the buffer is clamped, never followed
    if (e > n) e = n;
    if (e < b) e = b;
    // x is 16-byte aligned (checked on the host): element indices that are multiples of 4 are the aligned ones
    int64_t a0 = (b + 3) & ~(int64_t)3, a1 = e & ~(int64_t)3;
    if (a0 > e) a0 = e;
    if (a1 < a0) a1 = a0;
    const int t = threadIdx.x;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    if (b + t < a0) acc0 = sq(x[b + t]);                  // head: at most 3 elements, lanes 0..2
    if (a1 + t < e) acc1 = sq(x[a1 + t]);                 // tail: at most 3 elements (a1 == a0 == e when the head took everything)
    const f32x4* xv = (const f32x4*)x;
    const int64_t v0 = a0 >> 2, v1 = a1 >> 2;
    int64_t i = v0 + t;
    for (; i + 3 * SQ_BLOCK < v1; i += 4 * SQ_BLOCK) {    // four 16-byte loads in flight per lane
        const f32x4 p = xv[i], q = xv[i + SQ_BLOCK], r = xv[i + 2 * SQ_BLOCK], s = xv[i + 3 * SQ_BLOCK];
        acc0 += sq(p[0]); acc1 += sq(p[1]); acc2 += sq(p[2]); acc3 += sq(p[3]);
        acc0 += sq(q[0]); acc1 += sq(q[1]); acc2 += sq(q[2]); acc3 += sq(q[3]);
        acc0 += sq(r[0]); acc1 += sq(r[1]); acc2 += sq(r[2]); acc3 += sq(r[3]);
        acc0 += sq(s[0]); acc1 += sq(s[1]); acc2 += sq(s[2]); acc3 += sq(s[3]);
    }
    for (; i < v1; i += SQ_BLOCK) {
        const f32x4 p = xv[i];
        acc0 += sq(p[0]); acc1 += sq(p[1]); acc2 += sq(p[2]); acc3 += sq(p[3]);
    }
    double acc = (acc0 + acc1) + (acc2 + acc3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += shfl_xor_f64(acc, o);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) ws[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(SQ_BLOCK) void sumsq_fold_kernel(const double* __restrict__ ws, const int64_t* __restrict__ seg_ptr,
                                                              int64_t nseg, int64_t npieces, double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * (SQ_BLOCK / 64) + (threadIdx.x >> 6);
    if (s >= nseg) return;       // whole waves leave: no barrier below
    const int lane = threadIdx.x & 63;
    int64_t p0 = seg_ptr[s], p1 = seg_ptr[s + 1];
    if (p0 < 0) p0 = 0;          // as for the piece table: clamped to the workspace, never followed out of it
    if (p1 > npieces) p1 = npieces;
    double acc = 0.0;
    for (int64_t p = p0; p < p1; p += 64) {
        const int cnt = (int)(p1 - p < 64 ? p1 - p : 64);
        const double v = lane < cnt ? ws[p + lane] : 0.0;
        acc = wave_chain(acc, v, cnt);
    }
    if (lane == 0) out[s] = acc;
}

__global__ __launch_bounds__(64) void clip_finalize_kernel(const double* __restrict__ seg, int64_t nseg, float grad_scale,
                                                           float max_norm, float* __restrict__ rec) {
    const int lane = threadIdx.x;
    double total = 0.0;
    for (int64_t p = 0; p < nseg; p += 64) {
        const int cnt = (int)(nseg - p < 64 ? nseg - p : 64);
        const double v = lane < cnt ? seg[p + lane] : 0.0;
        total = wave_chain(total, v, cnt);
    }
    if (lane != 0) return;
    uint32_t* cnt = (uint32_t*)rec;
    const bool bad = !(total <= 1.7976931348623157e308);    // inf or nan (a sum of squares is never negative)
    const double norm = sqrt(total) * fabs((double)grad_scale);
    double c = (double)max_norm / (norm + 1e-6);             // torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6), clamped to 1
    if (c > 1.0) c = 1.0;
    const float coef = bad ? 0.0f : (float)c;
    rec[M3AE_CLIP_NORM] = (float)norm;
    rec[M3AE_CLIP_COEF] = coef;
    cnt[M3AE_CLIP_SKIP] = bad ? 1u : 0u;
    cnt[M3AE_CLIP_STEPS] += 1u;
    if (bad) cnt[M3AE_CLIP_SKIPPED_STEPS] += 1u;
    else if (coef < 1.0f) cnt[M3AE_CLIP_CLIPPED_STEPS] += 1u;
}

}  // namespace

extern "C" int64_t m3ae_sumsq_workspace_bytes(int64_t npieces) {
    if (npieces < 0) return M3AE_ERR_ARG;
    return 8 * (npieces > 0 ? npieces : 1);
}

extern "C" int m3ae_sumsq_segments(const float* x, int64_t n, const int64_t* pieces_dev, int64_t npieces, const int64_t* seg_ptr_dev,
                                   int64_t nseg, double* out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!x || n < 0 || !pieces_dev || npieces < 0 || !seg_ptr_dev || nseg <= 0 || !out) return M3AE_ERR_ARG;
    if (npieces > 0x7fffffffLL || nseg > 0x7fffffffLL) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)x & 15) || ((uintptr_t)out & 7) || ((uintptr_t)pieces_dev & 7) || ((uintptr_t)seg_ptr_dev & 7)) return M3AE_ERR_ALIGN;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < m3ae_sumsq_workspace_bytes(npieces)) return M3AE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (npieces > 0)
        hipLaunchKernelGGL(sumsq_piece_kernel, dim3((unsigned)npieces), dim3(SQ_BLOCK), 0, s, x, n, pieces_dev, (double*)workspace);
    hipLaunchKernelGGL(sumsq_fold_kernel, dim3((unsigned)cdiv(nseg, SQ_BLOCK / 64)), dim3(SQ_BLOCK), 0, s, (const double*)workspace,
                       seg_ptr_dev, nseg, npieces, out);
    return hip_launch_status();
}

extern "C" int m3ae_clip_finalize(const double* seg_sumsq, int64_t nseg, float grad_scale, float max_norm, float* record,
                                  void* stream) {
    if (!seg_sumsq || nseg <= 0 || !record) return M3AE_ERR_ARG;
    if (!(max_norm > 0.0f) || !isfinite(grad_scale)) return M3AE_ERR_ARG;   // max_norm: (0, +inf]; nan fails the comparison
    if (((uintptr_t)seg_sumsq & 7) || ((uintptr_t)record & 3)) return M3AE_ERR_ALIGN;
    hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, seg_sumsq, nseg, grad_scale, max_norm,
                       record);
    return hip_launch_status();
}
