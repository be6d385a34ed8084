// What the decode and evaluation kernels (csrc/greedy.hip, answer_trie.hip, trie_beam.hip, token_eval.hip, vqa_eval.hip) share:
// how a row of logits is read (walk_row, MsAcc), how a workgroup of 256 threads folds what its threads gathered (block_*), the
// trie table's child_range, and on the host side chunk_shape_ok with the chunk bounds and the by_dtype launcher.
//
// walk_row.  n elements at x are read ONCE: a scalar head up to the first 16-byte boundary, 16-byte loads, a scalar tail; whatever
//   the row stride, no load touches an element at or past x + n.  f(u, cnt, j0) gets the fp32 bit patterns of cnt consecutive
//   elements starting at element j0 of x: cnt == 1 for a head or tail element, cnt == W = 16 / sizeof(T) for one load.  A thread
//   sees its head element, then its loads in ascending order, then its tail element; this grouping is part of the contract
//   ((m, s) is not associative, and MsAcc::take forms one maximum per group).
// MsAcc.  The (m, s) = (maximum, sum exp(x - m)) pair of csrc/lse_pair.h over a thread's groups.
// block_*.  Six butterfly stages per wave, lane 0 of each wave leaves its value in LDS, one barrier, then thread 0 (EVERY: every
//   thread, with the same bits in each) folds the four waves in ascending order.  `red` is LDS of the caller, one array per fold:
//   a fold does not end with a barrier, so an array is not reused without one.  Each fold is *_put, __syncthreads(), *_get; a
//   kernel with several folds calls the halves itself and shares the one barrier (csrc/token_eval.hip).
//   The (m, s) outputs are promised bit for bit, and ms_merge's s1 e1 + s2 e2 is contracted to one multiply and one fused
//   multiply-add by the compiler, which nothing in the source pins.  In the thread-0 form thread 0 must go on from the pair in its
//   registers: reloading wave 0's pair from LDS made the compiler form both products first, and s moved by 1-2 ulp.  The host models
//   are bounds and do not notice; after any edit here compare the raw workspaces of m3ae_trie_scan and the nll of
//   m3ae_token_eval with the previous build on the same inputs.
// child_range.  The one place a trie node becomes a range of the CSR table of csrc/answer_trie.hip.
// Host side: the chunk bounds of the chunked entry points and the fp32 / bf16 dispatch.
#pragma once
#include "common.h"
#include "lse_pair.h"
#include "order_key.h"

namespace {

constexpr int SCAN_T = 256;              // threads of a workgroup that uses these helpers
constexpr int64_t SCAN_MIN_CHUNK = 64, SCAN_MAX_CHUNK = 65536;

template <typename T, class F>
DEVINL void walk_row(const T* __restrict__ x, int64_t n, int tid, F&& f) {
    constexpr int W = 16 / (int)sizeof(T);   // elements of one 16-byte load
    // x is element-aligned (host check): `mis` elements past a 16-byte boundary
    const int64_t mis = (int64_t)(((uintptr_t)x & 15) / sizeof(T));
    int64_t head = mis ? W - mis : 0;
    head = head < n ? head : n;
    const int64_t nvec = (n - head) / W;
    const int64_t tail0 = head + nvec * W;
    if (tid < head) {
        const uint32_t u = bits_of(x[tid]);
        f(&u, 1, (uint32_t)tid);
    }
    const u32x4* xv = (const u32x4*)(x + head);
    for (int64_t i = tid; i < nvec; i += SCAN_T) {
        const u32x4 q = xv[i];
        uint32_t u[W];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (sizeof(T) == 4) {
                u[e] = q[e];
            } else {   // two bf16 per dword, the lower column in the low half
                u[(2 * e) % W] = q[e] << 16;
                u[(2 * e + 1) % W] = q[e] & 0xffff0000u;
            }
        }
        f(u, W, (uint32_t)(head + i * W));
    }
    if (tail0 + tid < n) {   // < W <= SCAN_T columns
        const uint32_t u = bits_of(x[tail0 + tid]);
        f(&u, 1, (uint32_t)(tail0 + tid));
    }
}

struct MsAcc {
    float m = -INFINITY, s = 0.0f;
    // n <= 8 values (fp32 bits)
    DEVINL void take(const uint32_t* u, int n) {
        float vm = __uint_as_float(u[0]);
        for (int e = 1; e < n; ++e) vm = fmaxf(vm, __uint_as_float(u[e]));
        const float mn = fmaxf(m, vm);       // a NaN is skipped here and caught by expf below
        if (mn != m) { s *= exp_diff(m, mn); m = mn; }
        for (int e = 0; e < n; ++e) s += exp_diff(__uint_as_float(u[e]), m);
    }
};

DEVINL void max_put(uint64_t v, uint64_t* red, int tid) {
    v = wave_max_u64(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
}
template <bool EVERY = false>
DEVINL uint64_t max_get(const uint64_t* red, int tid) {
    uint64_t v = 0;
    if (EVERY || tid == 0) {
        v = red[0];
        for (int w = 1; w < SCAN_T / 64; ++w) v = max_u64(v, red[w]);
    }
    return v;
}
DEVINL uint64_t block_max_u64(uint64_t v, uint64_t* red, int tid) {
    max_put(v, red, tid);
    __syncthreads();
    return max_get(red, tid);
}

DEVINL void sum_put(int v, int* red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
}
template <bool EVERY = false>
DEVINL int sum_get(const int* red, int tid) {
    return (EVERY || tid == 0) ? red[0] + red[1] + red[2] + red[3] : 0;
}
DEVINL int block_sum_int(int v, int* red, int tid) {
    sum_put(v, red, tid);
    __syncthreads();
    return sum_get(red, tid);
}

DEVINL void ms_put(float& m, float& s, float* redm, float* reds, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        ms_merge(m, s, m2, s2);
    }
    if ((tid & 63) == 0) {
        redm[tid >> 6] = m;
        reds[tid >> 6] = s;
    }
}
template <bool EVERY = false>
DEVINL void ms_get(float& m, float& s, const float* redm, const float* reds, int tid) {
    if (EVERY) {   // thread 0 goes on from wave 0's pair in its registers: see the note on bits above
        m = redm[0];
        s = reds[0];
    }
    if (EVERY || tid == 0) {
        for (int w = 1; w < SCAN_T / 64; ++w) ms_merge(m, s, redm[w], reds[w]);
    }
}
DEVINL void block_ms_merge(float& m, float& s, float* redm, float* reds, int tid) {
    ms_put(m, s, redm, reds, tid);
    __syncthreads();
    ms_get(m, s, redm, reds, tid);
}

// rec[i] += the workgroup's sum of acc[i], i < N, as (w0 + w1) + (w2 + w3) of the wave sums; rec[N] += 1 counts the call.
// The order depends on nothing but what each thread holds; no atomics.
template <int N>
DEVINL void block_add_record(double* acc, double (*red)[N], double* __restrict__ rec, int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[i] += __shfl_xor(acc[i], o, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) red[tid >> 6][i] = acc[i];
    }
    __syncthreads();
    if (tid < N) rec[tid] += (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    if (tid == N) rec[N] += 1.0;
}

// The child range of node n, or false when the table does not hold one (never an address then).
DEVINL bool child_range(const int32_t* __restrict__ child_off, int64_t n, int64_t N, int64_t E, int64_t& lo, int64_t& hi) {
    if (n < 0 || n >= N) return false;
    lo = child_off[n];
    hi = child_off[n + 1];
    return lo >= 0 && hi <= E && lo < hi;
}

// R rows of V columns in chunks of `chunk`, plus `extra` work items a row, make a grid.
inline bool chunk_shape_ok(int64_t R, int64_t V, int64_t chunk, int64_t extra) {
    return R >= 1 && V >= 1 && V <= (int64_t)INT32_MAX && chunk >= SCAN_MIN_CHUNK && chunk <= SCAN_MAX_CHUNK && R <= (int64_t)INT32_MAX &&
           R * (cdiv(V, chunk) + extra) <= (int64_t)INT32_MAX;
}

// f(T()) with T the element type behind dtype, which the caller has checked to be M3AE_F32 or M3AE_BF16
template <class F>
void by_dtype(int dtype, F&& f) {
    if (dtype == M3AE_F32) f(float());
    else f(bf16_t());
}

}  // namespace
