// Tree attention for exhaustive answer-list scoring (m3ae_amd/modules/m3ae_decoder.py::Decoder.answer_scores_async): the decoder rows
// of ALL internal nodes of the answer trie (m3ae_amd/answer_trie.py::score_tables) run in one pass, and a row's self-attention keys
// are the rows of its trie ancestors, itself included -- what the causal mask leaves to the last row of a full-prefix pass.
// Forward only, no dropout.
//
// m3ae_tree_attn.  q, k, v [G][Ni][H * Dh] with row strides (the thirds of a packed qkv buffer, or the halves of k|v), fp32 or
//   bf16; anc int32 [Ni][Dmax], Dmax <= 32: for row i the rows from the root (first) to i itself (last), then -1; rel_bias optional
//   fp32 [H][Dmax], added to a score by depth(query) - depth(key) (T5's relative-position term).  Out [G][Ni][H * Dh] in the input
//   dtype.  One wave per (group, row, head), four waves a workgroup; keys and values are read straight from the [G][Ni] buffers
//   through anc, no gathered copy is formed.
//
// Order of operations (all fp32; tests/trie_score_model.py restates it):
//   n = the count of leading entries >= 0 of the row's anc; key j (0 <= j < n) is row anc[j] of the same group.
//   dot_j: lane l holds p = q[l] k_j[l], and for l + 64 < Dh p = fmaf(q[l + 64], k_j[l + 64], p); lanes with l >= Dh hold 0; the 64
//     partial sums are added by a butterfly of 6 stages (xor 32, 16, .. 1), after which every lane holds the same bits.
//   s_j = fmaf(dot_j, scale, bias) with bias = rel_bias[h][n - 1 - j], or dot_j * scale without a bias table.
//   m = max_j s_j; e_j = expf(s_j - m); den = the butterfly sum of e over the 64 lanes (lane j holds e_j, lanes >= n hold 0).
//   acc[c] = fmaf(e_j, v_j[c], acc[c]) for j ascending from acc = 0; out[c] = acc[c] / den, rounded once to the output dtype.
//   One key: e_0 = 1, den = 1, out = v_0 exactly.
// Every anc value is range-checked before it becomes an address: a row with no leading entry, or an entry >= Ni, sets err[0] = 1
// and its output is written as zeros.  No atomics: two runs on the same inputs give the same bits.
#include "common.h"

namespace {

constexpr int TA_T = 256;          // threads of a workgroup: four waves, one (group, row, head) each
constexpr int TA_MAX_DEPTH = 32;

template <typename T, int DH>
__global__ __launch_bounds__(TA_T) void tree_attn_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t ldk,
                                                         const T* __restrict__ v, int64_t ldv, T* __restrict__ out, int64_t ldo,
                                                         const int32_t* __restrict__ anc, int64_t Dmax,
                                                         const float* __restrict__ rel_bias, float scale, int64_t G, int64_t Ni,
                                                         int64_t H, int64_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t unit = (int64_t)blockIdx.x * (TA_T / 64) + (threadIdx.x >> 6);     // wave-uniform
    if (unit >= G * Ni * H) return;
    const int64_t h = unit % H, row = unit / H, i = row % Ni, g = row / Ni;
    constexpr bool TWO = DH > 64;
    const bool has2 = TWO && lane + 64 < DH;

    const int a = lane < Dmax ? anc[i * Dmax + lane] : -1;
    const unsigned long long neg = __ballot(a < 0);
    const int n = neg ? __ffsll((long long)neg) - 1 : 64;          // leading entries >= 0; n <= Dmax <= 32
    const bool bad = n < 1 || __ballot(lane < n && (int64_t)a >= Ni) != 0;
    T* o = out + (g * Ni + i) * ldo + h * DH;
    if (bad) {
        if (lane == 0) err[0] = 1;
        if (lane < DH) Elem<T>::st(o + lane, 0.0f);
        if (has2) Elem<T>::st(o + lane + 64, 0.0f);
        return;
    }
    const T* qr = q + (g * Ni + i) * ldq + h * DH;
    const float q0 = lane < DH ? Elem<T>::ld(qr + lane) : 0.0f;
    const float q1 = has2 ? Elem<T>::ld(qr + lane + 64) : 0.0f;

    float s = -INFINITY;                                           // lane j holds s_j
    for (int j = 0; j < n; ++j) {
        const int64_t kr = g * Ni + __shfl(a, j, 64);
        const T* kp = k + kr * ldk + h * DH;
        float p = lane < DH ? q0 * Elem<T>::ld(kp + lane) : 0.0f;
        if (has2) p = fmaf(q1, Elem<T>::ld(kp + lane + 64), p);
        p = wave_sum(p);
        const float sj = rel_bias ? fmaf(p, scale, rel_bias[h * Dmax + (n - 1 - j)]) : p * scale;
        if (lane == j) s = sj;
    }
    const float m = wave_max(s);
    const float e = lane < n ? expf(s - m) : 0.0f;
    const float den = wave_sum(e);
    float acc0 = 0.0f, acc1 = 0.0f;
    for (int j = 0; j < n; ++j) {
        const int64_t vr = g * Ni + __shfl(a, j, 64);
        const float ej = __shfl(e, j, 64);
        const T* vp = v + vr * ldv + h * DH;
        if (lane < DH) acc0 = fmaf(ej, Elem<T>::ld(vp + lane), acc0);
        if (has2) acc1 = fmaf(ej, Elem<T>::ld(vp + lane + 64), acc1);
    }
    if (lane < DH) Elem<T>::st(o + lane, acc0 / den);
    if (has2) Elem<T>::st(o + lane + 64, acc1 / den);
}

}  // namespace

extern "C" int m3ae_tree_attn(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out, int64_t ldo,
                              const int32_t* anc, int64_t Dmax, const float* rel_bias, float scale, int64_t G, int64_t Ni, int64_t H,
                              int64_t Dh, int dtype, int64_t* err, void* stream) {
    if (!q || !k || !v || !out || !anc || !err || G < 1 || Ni < 1 || H < 1 || Dh < 1 || Dmax < 1) return M3AE_ERR_ARG;
    if (ldq < H * Dh || ldk < H * Dh || ldv < H * Dh || ldo < H * Dh) return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if ((Dh != 64 && Dh != 96) || Dmax > TA_MAX_DEPTH || Ni > (int64_t)INT32_MAX || G > (int64_t)INT32_MAX || H > 65536 ||
        G * Ni > (int64_t)INT32_MAX || G * Ni * H > (int64_t)INT32_MAX * (TA_T / 64))
        return M3AE_ERR_UNSUPPORTED;
    const uintptr_t em = dtype == M3AE_F32 ? 3 : 1;
    if (((uintptr_t)q & em) || ((uintptr_t)k & em) || ((uintptr_t)v & em) || ((uintptr_t)out & em) || ((uintptr_t)anc & 3) ||
        ((uintptr_t)rel_bias & 3) || ((uintptr_t)err & 7))
        return M3AE_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(G * Ni * H, TA_T / 64));
#define TA_LAUNCH(T, DH)                                                                                                              \
    hipLaunchKernelGGL((tree_attn_kernel<T, DH>), grid, dim3(TA_T), 0, s, (const T*)q, ldq, (const T*)k, ldk, (const T*)v, ldv, (T*)out, \
                       ldo, anc, Dmax, rel_bias, scale, G, Ni, H, err)
    if (dtype == M3AE_F32) {
        if (Dh == 64) TA_LAUNCH(float, 64);
        else TA_LAUNCH(float, 96);
    } else {
        if (Dh == 64) TA_LAUNCH(bf16_t, 64);
        else TA_LAUNCH(bf16_t, 96);
    }
#undef TA_LAUNCH
    return hip_launch_status();
}
