// Answer-list decoding for the generator heads (m3ae_amd/modules/m3ae_decoder.py::Decoder.answer_path_async,
// m3ae_amd/modules/t5.py::T5.constrained_greedy_async): greedy search constrained to a prefix trie of the candidate answers
// (m3ae_amd/answer_trie.py), with the log-probability of the chosen path, and no host involvement.
//
// The trie is a CSR table in device memory: child_off int32 [N + 1], child_tok / child_node int32 [E] (tokens ascending within a
// node), leaf_label int32 [N] (the label behind an end token, -1 elsewhere); node 0 is the root.  The host checks the table
// (AnswerTrie.to_device); the kernels still turn no table value into an address without a range check.
//
// m3ae_trie_scan, one launch, grid (work item, row) with chunks + 1 work items per row.  Every workgroup of a row whose `finished`
//   word is set returns before its first load.
//   items 0 .. chunks - 1: csrc/greedy.hip's geometry.  The workgroup reads its chunk of the row ONCE (scalar head up to the first
//     16-byte boundary, 16-byte loads, scalar tail: no load touches a column at or past V) and writes the chunk's
//     (m, s) = (maximum, sum exp(x - m)) in fp32 to a workspace slot of its own: csrc/lse_pair.h, in csrc/token_eval.hip's order of
//     operations (per thread, 6 butterfly stages per wave, the four waves in sequence).
//   item chunks: reads the row's node and gathers the logits at that node's child tokens, any number of them (a loop of 256 per
//     pass).  Child i of the node gives the order key of csrc/order_key.h with greedy.hip's NaN / -0 handling,
//     (monotone image of the value) << 32 | (2^32 - 1 - i); children are ascending in token, so the greatest key is torch.argmax's
//     choice restricted to the allowed columns.  Keys of distinct children are distinct: the maximum depends on no order.
// m3ae_trie_step, one workgroup, a thread per row (csrc/greedy.hip's greedy_step_kernel): folds the row's (m, s) pairs in ascending
//   chunk order, lse = m + logf(s); decodes the child position from the key, takes token and next node from the table, adds
//   x[tok] - lse (fp32) onto the row's score in double and applies one step of the search to the device state.
// No atomics, every reduction in a fixed order: two runs on the same inputs give the same bits, the score included.
#include "common.h"
#include "lse_pair.h"
#include "order_key.h"
#include "topk_keep.h"

namespace {

constexpr int AT = 256;                   // threads of both kernels
constexpr int64_t A_DEF_CHUNK = 8192;     // csrc/token_eval.hip's: the chunk work is its (m, s) pass
constexpr int64_t A_MIN_CHUNK = 64, A_MAX_CHUNK = 65536;

// What a thread has gathered from its columns of the chunk: token_eval.hip's Acc, the (m, s) part.
struct MsAcc {
    float m, s;
    // n <= 8 values (fp32 bits)
    DEVINL void take(const uint32_t* u, int n) {
        float vm = __uint_as_float(u[0]);
        for (int e = 1; e < n; ++e) vm = fmaxf(vm, __uint_as_float(u[e]));
        const float mn = fmaxf(m, vm);       // a NaN is skipped here and caught by expf below
        if (mn != m) { s *= exp_diff(m, mn); m = mn; }
        for (int e = 0; e < n; ++e) s += exp_diff(__uint_as_float(u[e]), m);
    }
};

// The child range of node n, or false when the table does not hold one (never an address then).
DEVINL bool child_range(const int32_t* __restrict__ child_off, int64_t n, int64_t N, int64_t E, int64_t& lo, int64_t& hi) {
    if (n < 0 || n >= N) return false;
    lo = child_off[n];
    hi = child_off[n + 1];
    return lo >= 0 && hi <= E && lo < hi;
}

template <typename T>
__global__ __launch_bounds__(AT) void trie_scan_kernel(const T* __restrict__ logits, int64_t ld, int64_t V, int64_t chunk, int64_t nch,
                                                       const int32_t* __restrict__ child_off, const int32_t* __restrict__ child_tok,
                                                       int64_t N, int64_t E, const int32_t* __restrict__ node,
                                                       const int32_t* __restrict__ finished, uint64_t* __restrict__ ckey,
                                                       float* __restrict__ ms) {
    constexpr int W = 16 / (int)sizeof(T);   // elements of one 16-byte load
    __shared__ uint64_t redk[AT / 64];
    __shared__ float redm[AT / 64], reds[AT / 64];
    const int64_t r = blockIdx.x / (nch + 1), c = blockIdx.x % (nch + 1);
    if (finished[r]) return;                  // the whole workgroup: nothing of the row is read
    const int tid = threadIdx.x;
    const T* row = logits + r * ld;

    if (c == nch) {   // the children of the row's node
        int64_t lo = 0, hi = 0;
        uint64_t best = 0;                    // stays 0 without a child range: the step reports it
        if (child_range(child_off, node[r], N, E, lo, hi)) {
            for (int64_t i = lo + tid; i < hi; i += AT) {
                const int64_t tok = child_tok[i];
                if (tok >= 0 && tok < V) {
                    const uint64_t key = eval_key(bits_of(row[tok]), (uint32_t)(i - lo));
                    best = key > best ? key : best;
                }
            }
        }
        best = wave_max_u64(best);
        if ((tid & 63) == 0) redk[tid >> 6] = best;
        __syncthreads();
        if (tid == 0) {
            const uint64_t a = redk[0] > redk[1] ? redk[0] : redk[1], b = redk[2] > redk[3] ? redk[2] : redk[3];
            ckey[r] = a > b ? a : b;
        }
        return;
    }

    const int64_t v0 = c * chunk;
    const int64_t n = (V - v0) < chunk ? (V - v0) : chunk;
    const T* x = row + v0;
    MsAcc acc;
    acc.m = -INFINITY;
    acc.s = 0.0f;
    // x is element-aligned (host check): `mis` elements past a 16-byte boundary
    const int64_t mis = (int64_t)(((uintptr_t)x & 15) / sizeof(T));
    int64_t head = mis ? W - mis : 0;
    head = head < n ? head : n;
    const int64_t nvec = (n - head) / W;
    const int64_t tail0 = head + nvec * W;
    if (tid < head) {
        const uint32_t u = bits_of(x[tid]);
        acc.take(&u, 1);
    }
    const u32x4* xv = (const u32x4*)(x + head);
    for (int64_t i = tid; i < nvec; i += AT) {
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
        acc.take(u, W);
    }
    if (tail0 + tid < n) {   // < W <= AT columns
        const uint32_t u = bits_of(x[tail0 + tid]);
        acc.take(&u, 1);
    }

    float m = acc.m, s = acc.s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        ms_merge(m, s, m2, s2);
    }
    if ((tid & 63) == 0) {
        redm[tid >> 6] = m;
        reds[tid >> 6] = s;
    }
    __syncthreads();
    if (tid == 0) {   // lane 0 of wave 0 folds the four waves in order
        for (int w = 1; w < AT / 64; ++w) ms_merge(m, s, redm[w], reds[w]);
        const int64_t slot = r * nch + c;
        ms[2 * slot] = m;
        ms[2 * slot + 1] = s;
    }
}

template <typename T>
__global__ __launch_bounds__(AT) void trie_step_kernel(const T* __restrict__ logits, int64_t ld, const uint64_t* __restrict__ ckey,
                                                       const float* __restrict__ ms, int64_t nch, const int32_t* __restrict__ child_off,
                                                       const int32_t* __restrict__ child_tok, const int32_t* __restrict__ child_node,
                                                       const int32_t* __restrict__ leaf_label, int64_t N, int64_t E,
                                                       int64_t* __restrict__ seq, int64_t* __restrict__ len, int64_t* __restrict__ label,
                                                       double* __restrict__ score, int64_t* __restrict__ last_tok,
                                                       int32_t* __restrict__ node, int32_t* __restrict__ finished,
                                                       int32_t* __restrict__ open_count, int64_t* __restrict__ err, int64_t B, int64_t V,
                                                       int64_t max_len, int64_t pos, int64_t pad) {
    __shared__ int red[AT / 64];
    const int tid = threadIdx.x;
    int open = 0;
    for (int64_t r = tid; r < B; r += AT) {
        if (finished[r]) {                    // node, score, label and last_tok stay; the scan wrote nothing for this row
            seq[r * max_len + pos] = pad;
            continue;
        }
        int64_t lo = 0, hi = 0, tok = -1, nn = -1;
        if (child_range(child_off, node[r], N, E, lo, hi)) {
            const uint64_t g = ckey[r];
            const int64_t p = (int64_t)(0xffffffffu - (uint32_t)g);
            if (g != 0 && p < hi - lo) {      // a position outside the node's range is never an address
                tok = child_tok[lo + p];
                nn = child_node[lo + p];
            }
        }
        if (tok < 0 || tok >= V || nn < 0 || nn >= N) {
            err[0] = 1;
            last_tok[r] = 0;                  // the next step gathers an embedding row by it: keep it a row of the table
            seq[r * max_len + pos] = 0;
            open += 1;                        // node and score stay; the row stays open
            continue;
        }
        float m = -INFINITY, s = 0.0f;
        const float* p2 = ms + 2 * r * nch;
        for (int64_t i = 0; i < nch; ++i) ms_merge(m, s, p2[2 * i], p2[2 * i + 1]);
        const float lse = m + logf(s);
        const float term = Elem<T>::ld(logits + r * ld + tok) - lse;
        score[r] += (double)term;
        last_tok[r] = tok;
        seq[r * max_len + pos] = tok;
        node[r] = (int32_t)nn;
        const int32_t lab = leaf_label[nn];
        if (lab >= 0) {
            label[r] = lab;
            len[r] = pos + 1;
            finished[r] = 1;
        } else {
            open += 1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) open += __shfl_xor(open, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = open;
    __syncthreads();
    if (tid == 0) open_count[pos] = red[0] + red[1] + red[2] + red[3];
}

inline bool trie_shape_ok(int64_t R, int64_t V, int64_t chunk) {
    return R >= 1 && V >= 1 && V <= (int64_t)INT32_MAX && chunk >= A_MIN_CHUNK && chunk <= A_MAX_CHUNK && R <= (int64_t)INT32_MAX &&
           R * (cdiv(V, chunk) + 1) <= (int64_t)INT32_MAX;
}
// workspace: child key u64 [R] | (m, s) fp32 [R][chunks][2]
inline int64_t trie_ws_bytes(int64_t R, int64_t nch) { return R * 8 + R * nch * 8; }

}  // namespace

extern "C" int64_t m3ae_trie_workspace_bytes(int64_t R, int64_t V, int64_t chunk) {
    if (chunk == 0) chunk = A_DEF_CHUNK;
    if (!trie_shape_ok(R, V, chunk)) return 0;
    return trie_ws_bytes(R, cdiv(V, chunk));
}

extern "C" int m3ae_trie_scan(const void* logits, int64_t ld, int64_t R, int64_t V, int64_t chunk, int dtype, const int32_t* child_off,
                              const int32_t* child_tok, int64_t N, int64_t E, const int32_t* node, const int32_t* finished,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    if (!logits || R < 1 || V < 1 || ld < V || chunk < 0 || !child_off || !child_tok || !node || !finished || N < 1 || E < 1) return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (chunk == 0) chunk = A_DEF_CHUNK;
    if (!trie_shape_ok(R, V, chunk) || N > (int64_t)INT32_MAX || E > (int64_t)INT32_MAX) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) || ((uintptr_t)child_off & 3) || ((uintptr_t)child_tok & 3) || ((uintptr_t)node & 3) ||
        ((uintptr_t)finished & 3))
        return M3AE_ERR_ALIGN;
    const int64_t nch = cdiv(V, chunk);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < trie_ws_bytes(R, nch)) return M3AE_ERR_WORKSPACE;
    uint64_t* ckey = (uint64_t*)workspace;
    float* ms = (float*)(ckey + R);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(R * (nch + 1)));
    if (dtype == M3AE_F32)
        hipLaunchKernelGGL(trie_scan_kernel<float>, grid, dim3(AT), 0, s, (const float*)logits, ld, V, chunk, nch, child_off, child_tok, N, E, node,
                           finished, ckey, ms);
    else
        hipLaunchKernelGGL(trie_scan_kernel<bf16_t>, grid, dim3(AT), 0, s, (const bf16_t*)logits, ld, V, chunk, nch, child_off, child_tok, N, E,
                           node, finished, ckey, ms);
    return hip_launch_status();
}

extern "C" int m3ae_trie_step(const void* logits, int64_t ld, int dtype, const void* workspace, int64_t workspace_bytes, int64_t nch,
                              const int32_t* child_off, const int32_t* child_tok, const int32_t* child_node, const int32_t* leaf_label,
                              int64_t N, int64_t E, int64_t* seq, int64_t* len, int64_t* label, double* score, int64_t* last_tok,
                              int32_t* node, int32_t* finished, int32_t* open_count, int64_t* err, int64_t B, int64_t V, int64_t max_len,
                              int64_t pos, int64_t pad, void* stream) {
    if (!logits || !child_off || !child_tok || !child_node || !leaf_label || !seq || !len || !label || !score || !last_tok || !node ||
        !finished || !open_count || !err || B < 1 || B > (int64_t)INT32_MAX || V < 1 || V > (int64_t)INT32_MAX || ld < V || max_len < 1 ||
        max_len > (int64_t)INT32_MAX || pos < 0 || pos >= max_len || nch < 1 || nch > (int64_t)INT32_MAX || N < 1 || N > (int64_t)INT32_MAX ||
        E < 1 || E > (int64_t)INT32_MAX)
        return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) || ((uintptr_t)child_off & 3) || ((uintptr_t)child_tok & 3) ||
        ((uintptr_t)child_node & 3) || ((uintptr_t)leaf_label & 3) || ((uintptr_t)seq & 7) || ((uintptr_t)len & 7) || ((uintptr_t)label & 7) ||
        ((uintptr_t)score & 7) || ((uintptr_t)last_tok & 7) || ((uintptr_t)node & 3) || ((uintptr_t)finished & 3) || ((uintptr_t)open_count & 3) ||
        ((uintptr_t)err & 7))
        return M3AE_ERR_ALIGN;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < trie_ws_bytes(B, nch)) return M3AE_ERR_WORKSPACE;
    const uint64_t* ckey = (const uint64_t*)workspace;
    const float* ms = (const float*)(ckey + B);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == M3AE_F32)
        hipLaunchKernelGGL(trie_step_kernel<float>, dim3(1), dim3(AT), 0, s, (const float*)logits, ld, ckey, ms, nch, child_off, child_tok,
                           child_node, leaf_label, N, E, seq, len, label, score, last_tok, node, finished, open_count, err, B, V, max_len, pos, pad);
    else
        hipLaunchKernelGGL(trie_step_kernel<bf16_t>, dim3(1), dim3(AT), 0, s, (const bf16_t*)logits, ld, ckey, ms, nch, child_off, child_tok,
                           child_node, leaf_label, N, E, seq, len, label, score, last_tok, node, finished, open_count, err, B, V, max_len, pos, pad);
    return hip_launch_status();
}
