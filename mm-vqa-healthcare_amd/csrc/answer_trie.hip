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
//   items 0 .. chunks - 1: the workgroup reads its chunk of the row ONCE (csrc/row_scan.h's walk_row: no load touches a column at
//     or past V) and writes the chunk's (m, s) = (maximum, sum exp(x - m)) in fp32 to a workspace slot of its own: csrc/lse_pair.h,
//     in the order of operations of csrc/row_scan.h (MsAcc per thread, then block_ms_merge: 6 butterfly stages per wave, the four
//     waves in sequence), which csrc/token_eval.hip shares.
//   item chunks: reads the row's node and gathers the logits at that node's child tokens, any number of them (a loop of 256 per
//     pass).  Child i of the node gives the order key of csrc/order_key.h (eval_key),
//     (monotone image of the value) << 32 | (2^32 - 1 - i); children are ascending in token, so the greatest key is torch.argmax's
//     choice restricted to the allowed columns.  Keys of distinct children are distinct: the maximum depends on no order.
// m3ae_trie_step, one workgroup, a thread per row (as csrc/greedy.hip's greedy_step_kernel): folds the row's (m, s) pairs in ascending
//   chunk order, lse = m + logf(s); decodes the child position from the key, takes token and next node from the table, adds
//   x[tok] - lse (fp32) onto the row's score in double and applies one step of the search to the device state.
// No atomics, every reduction in a fixed order: two runs on the same inputs give the same bits, the score included.
#include "common.h"
#include "row_scan.h"

namespace {

constexpr int AT = SCAN_T;                // threads of both kernels
constexpr int64_t A_DEF_CHUNK = 8192;     // csrc/token_eval.hip's: the chunk work is its (m, s) pass

template <typename T>
__global__ __launch_bounds__(AT) void trie_scan_kernel(const T* __restrict__ logits, int64_t ld, int64_t V, int64_t chunk, int64_t nch,
                                                       const int32_t* __restrict__ child_off, const int32_t* __restrict__ child_tok,
                                                       int64_t N, int64_t E, const int32_t* __restrict__ node,
                                                       const int32_t* __restrict__ finished, uint64_t* __restrict__ ckey,
                                                       float* __restrict__ ms) {
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
                if (tok >= 0 && tok < V) best = max_u64(best, eval_key(bits_of(row[tok]), (uint32_t)(i - lo)));
            }
        }
        best = block_max_u64(best, redk, tid);
        if (tid == 0) ckey[r] = best;
        return;
    }

    const int64_t v0 = c * chunk;
    const int64_t n = (V - v0) < chunk ? (V - v0) : chunk;
    MsAcc acc;
    walk_row(row + v0, n, tid, [&](const uint32_t* u, int cnt, uint32_t) { acc.take(u, cnt); });
    block_ms_merge(acc.m, acc.s, redm, reds, tid);
    if (tid == 0) {
        const int64_t slot = r * nch + c;
        ms[2 * slot] = acc.m;
        ms[2 * slot + 1] = acc.s;
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
            const int64_t p = key_index_in(ckey[r], hi - lo);
            if (p >= 0) {                     // a position outside the node's range is never an address
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
    open = block_sum_int(open, red, tid);
    if (tid == 0) open_count[pos] = open;
}

// workspace: child key u64 [R] | (m, s) fp32 [R][chunks][2]
inline int64_t trie_ws_bytes(int64_t R, int64_t nch) { return R * 8 + R * nch * 8; }

}  // namespace

extern "C" int64_t m3ae_trie_workspace_bytes(int64_t R, int64_t V, int64_t chunk) {
    if (chunk == 0) chunk = A_DEF_CHUNK;
    if (!chunk_shape_ok(R, V, chunk, 1)) return 0;
    return trie_ws_bytes(R, cdiv(V, chunk));
}

extern "C" int m3ae_trie_scan(const void* logits, int64_t ld, int64_t R, int64_t V, int64_t chunk, int dtype, const int32_t* child_off,
                              const int32_t* child_tok, int64_t N, int64_t E, const int32_t* node, const int32_t* finished,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    if (!logits || R < 1 || V < 1 || ld < V || chunk < 0 || !child_off || !child_tok || !node || !finished || N < 1 || E < 1) return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (chunk == 0) chunk = A_DEF_CHUNK;
    if (!chunk_shape_ok(R, V, chunk, 1) || N > (int64_t)INT32_MAX || E > (int64_t)INT32_MAX) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) || ((uintptr_t)child_off & 3) || ((uintptr_t)child_tok & 3) || ((uintptr_t)node & 3) ||
        ((uintptr_t)finished & 3))
        return M3AE_ERR_ALIGN;
    const int64_t nch = cdiv(V, chunk);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < trie_ws_bytes(R, nch)) return M3AE_ERR_WORKSPACE;
    uint64_t* ckey = (uint64_t*)workspace;
    float* ms = (float*)(ckey + R);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(R * (nch + 1)));
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(trie_scan_kernel<T>, grid, dim3(AT), 0, s, (const T*)logits, ld, V, chunk, nch, child_off, child_tok, N, E, node,
                           finished, ckey, ms);
    });
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
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(trie_step_kernel<T>, dim3(1), dim3(AT), 0, s, (const T*)logits, ld, ckey, ms, nch, child_off, child_tok, child_node,
                           leaf_label, N, E, seq, len, label, score, last_tok, node, finished, open_count, err, B, V, max_len, pos, pad);
    });
    return hip_launch_status();
}
