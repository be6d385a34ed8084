// Sample expansion of a de-duplicated image batch and its backward (M3AETransformerSS.infer with batch["image_index"]): the image
// tower runs once per DISTINCT image, m3ae_expand_samples copies every sample's [L, D] token block out of its image's block
// before the fusion layers, m3ae_segment_sum_rows adds the samples' gradients back per image.
//
// Both are HBM-streaming kernels over whole rows of R = L * D elements (886 KB at 577 x 768 bf16): grid.y walks the rows, grid.x
// the 16-byte units of a row, so no lane divides by the row length and every wave-instruction moves 1 KiB of one row.  Row bases
// are 64-bit element offsets (ViT-L at 1025 tokens and 256 samples is past 2^31 bytes).  When R * sizeof(T) is no multiple of 16
// or a base pointer is not 16-byte aligned the same kernels run with one element per lane.
// The segment sum gives every output element to ONE lane, which adds the group's members in the order the member list holds them
// (ascending sample index) in an fp32 register and rounds once on the store: no atomics, so the result is the same bits on every
// run and deterministic mode needs no second form.  The first member initialises the sum, so a group of one is a plain copy.
#include "common.h"

namespace {

constexpr int SAMPLES_BLOCK = 256;
constexpr int SAMPLES_UNROLL = 4;   // row units (expand) / group members (segment sum) in flight per lane

// one 16-byte unit of T as fp32 values, or one element (VEC = false)
template <typename T, bool VEC> struct RowUnit;
template <> struct RowUnit<float, true> {
    static constexpr int N = 4;
    static DEVINL void ld(const float* p, float* x) { const f32x4 v = *(const f32x4*)p; x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3]; }
    static DEVINL void st(float* p, const float* x) { *(f32x4*)p = (f32x4){x[0], x[1], x[2], x[3]}; }
};
template <> struct RowUnit<bf16_t, true> {
    static constexpr int N = 8;
    static DEVINL void ld(const bf16_t* p, float* x) {
        const u32x4 v = *(const u32x4*)p;
#pragma unroll
        for (int t = 0; t < 4; ++t) { x[2 * t] = __uint_as_float(v[t] << 16); x[2 * t + 1] = __uint_as_float(v[t] & 0xffff0000u); }
    }
    static DEVINL void st(bf16_t* p, const float* x) {   // round-to-nearest-even, once
        *(u32x4*)p = (u32x4){pack2bf(x[0], x[1]), pack2bf(x[2], x[3]), pack2bf(x[4], x[5]), pack2bf(x[6], x[7])};
    }
};
template <typename T> struct RowUnit<T, false> {
    static constexpr int N = 1;
    static DEVINL void ld(const T* p, float* x) { x[0] = Elem<T>::ld(p); }
    static DEVINL void st(T* p, const float* x) { Elem<T>::st(p, x[0]); }
};

// out[b] = in[src[b]]; U = u32x4 (C 16-byte units per row) or the element type (C elements per row).  A source index outside
// [0, n_in) is never turned into an address: that output row is left as it was (the host wrappers validate the tables).
template <typename U>
__global__ __launch_bounds__(SAMPLES_BLOCK) void expand_samples_kernel(const U* __restrict__ in, const int64_t* __restrict__ src,
                                                                        U* __restrict__ out, int64_t n_out, int64_t n_in, int64_t C) {
    constexpr int64_t STEP = (int64_t)SAMPLES_BLOCK * SAMPLES_UNROLL;
    for (int64_t b = blockIdx.y; b < n_out; b += gridDim.y) {
        const int64_t s = src[b];
        if ((uint64_t)s >= (uint64_t)n_in) continue;
        const U* p = in + s * C;
        U* q = out + b * C;
        for (int64_t c = (int64_t)blockIdx.x * STEP + threadIdx.x; c < C; c += (int64_t)gridDim.x * STEP) {
            U v[SAMPLES_UNROLL];
#pragma unroll
            for (int k = 0; k < SAMPLES_UNROLL; ++k)
                if (c + k * SAMPLES_BLOCK < C) v[k] = p[c + k * SAMPLES_BLOCK];
#pragma unroll
            for (int k = 0; k < SAMPLES_UNROLL; ++k)
                if (c + k * SAMPLES_BLOCK < C) q[c + k * SAMPLES_BLOCK] = v[k];
        }
    }
}

// d_in[u] = sum of d_out[members[j]], j in [offsets[u], offsets[u + 1]), added in list order.  C = units per row.  Offsets are
// clamped to [0, n_out] and a member outside [0, n_out) adds nothing; an empty group stores zeros.
template <typename T, bool VEC>
__global__ __launch_bounds__(SAMPLES_BLOCK) void segment_sum_rows_kernel(const T* __restrict__ d_out, const int64_t* __restrict__ offsets,
                                                                          const int64_t* __restrict__ members, T* __restrict__ d_in,
                                                                          int64_t n_in, int64_t n_out, int64_t C) {
    using Unit = RowUnit<T, VEC>;
    constexpr int N = Unit::N;
    for (int64_t u = blockIdx.y; u < n_in; u += gridDim.y) {
        int64_t beg = offsets[u], end = offsets[u + 1];
        if (beg < 0) beg = 0;
        if (end > n_out) end = n_out;
        for (int64_t c = (int64_t)blockIdx.x * SAMPLES_BLOCK + threadIdx.x; c < C; c += (int64_t)gridDim.x * SAMPLES_BLOCK) {
            float acc[N];
#pragma unroll
            for (int t = 0; t < N; ++t) acc[t] = 0.f;
            int64_t j = beg;
            if (j < end) {   // the first member IS the sum so far (a group of one: a copy, the sign of a zero included)
                const int64_t m = members[j];
                if ((uint64_t)m < (uint64_t)n_out) Unit::ld(d_out + (m * C + c) * N, acc);
                ++j;
            }
            for (; j < end; j += SAMPLES_UNROLL) {   // loads of up to four members in flight, adds in list order
                float v[SAMPLES_UNROLL][N];
#pragma unroll
                for (int k = 0; k < SAMPLES_UNROLL; ++k) {
#pragma unroll
                    for (int t = 0; t < N; ++t) v[k][t] = 0.f;
                    if (j + k < end) {
                        const int64_t m = members[j + k];
                        if ((uint64_t)m < (uint64_t)n_out) Unit::ld(d_out + (m * C + c) * N, v[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < SAMPLES_UNROLL; ++k)
                    if (j + k < end) {
#pragma unroll
                        for (int t = 0; t < N; ++t) acc[t] += v[k][t];
                    }
            }
            Unit::st(d_in + (u * C + c) * N, acc);
        }
    }
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
inline dim3 samples_grid(int64_t rows, int64_t units_per_block, int64_t C) {
    int64_t gx = cdiv(C, units_per_block), gy = rows;
    if (gx > 1024) gx = 1024;
    if (gy > 65535) gy = 65535;
    return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

extern "C" int m3ae_expand_samples(const void* in, const int64_t* src, void* out, int64_t n_out, int64_t n_in, int64_t R,
                                   int dtype, void* stream) {
    if (!in || !src || !out || n_out <= 0 || n_in <= 0 || R <= 0) return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int64_t esize = dtype == M3AE_F32 ? 4 : 2, row_bytes = R * esize;
    constexpr int64_t per_block = (int64_t)SAMPLES_BLOCK * SAMPLES_UNROLL;
    if (row_bytes % 16 == 0 && aligned16(in) && aligned16(out)) {
        const int64_t C = row_bytes / 16;
        hipLaunchKernelGGL(expand_samples_kernel<u32x4>, samples_grid(n_out, per_block, C), dim3(SAMPLES_BLOCK), 0, s,
                           (const u32x4*)in, src, (u32x4*)out, n_out, n_in, C);
    } else if (dtype == M3AE_F32) {
        hipLaunchKernelGGL(expand_samples_kernel<float>, samples_grid(n_out, per_block, R), dim3(SAMPLES_BLOCK), 0, s,
                           (const float*)in, src, (float*)out, n_out, n_in, R);
    } else {
        hipLaunchKernelGGL(expand_samples_kernel<bf16_t>, samples_grid(n_out, per_block, R), dim3(SAMPLES_BLOCK), 0, s,
                           (const bf16_t*)in, src, (bf16_t*)out, n_out, n_in, R);
    }
    return hip_launch_status();
}

template <typename T>
static int launch_segment_sum(const void* d_out, const int64_t* offsets, const int64_t* members, void* d_in, int64_t n_in,
                              int64_t n_out, int64_t R, hipStream_t s) {
    constexpr int64_t N = 16 / (int64_t)sizeof(T);
    if (R % N == 0 && aligned16(d_out) && aligned16(d_in)) {
        const int64_t C = R / N;
        hipLaunchKernelGGL((segment_sum_rows_kernel<T, true>), samples_grid(n_in, SAMPLES_BLOCK, C), dim3(SAMPLES_BLOCK), 0, s,
                           (const T*)d_out, offsets, members, (T*)d_in, n_in, n_out, C);
    } else {
        hipLaunchKernelGGL((segment_sum_rows_kernel<T, false>), samples_grid(n_in, SAMPLES_BLOCK, R), dim3(SAMPLES_BLOCK), 0, s,
                           (const T*)d_out, offsets, members, (T*)d_in, n_in, n_out, R);
    }
    return hip_launch_status();
}

extern "C" int m3ae_segment_sum_rows(const void* d_out, const int64_t* offsets, const int64_t* members, void* d_in, int64_t n_in,
                                     int64_t n_out, int64_t R, int dtype, void* stream) {
    if (!d_out || !offsets || !members || !d_in || n_in <= 0 || n_out <= 0 || R <= 0) return M3AE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == M3AE_F32) return launch_segment_sum<float>(d_out, offsets, members, d_in, n_in, n_out, R, s);
    if (dtype == M3AE_BF16) return launch_segment_sum<bf16_t>(d_out, offsets, members, d_in, n_in, n_out, R, s);
    return M3AE_ERR_UNSUPPORTED;
}
