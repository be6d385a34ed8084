// Exhaustive answer-list scoring for the generator heads (m3ae_amd/modules/m3ae_decoder.py::Decoder.answer_scores_async): the
// log-probability of EVERY entry of the answer list from one decoder pass over the internal nodes of the answer trie, the list's
// arg-max, its k best entries with probabilities over the list, and the mass the head puts on the list.  No host involvement.
//
// Tables (m3ae_amd/answer_trie.py::score_tables, int32, device memory; the CSR arrays are csrc/answer_trie.hip's): internal [Ni] the
// nodes with children, parent / depth [N], level_off [Dmax + 2], leaf_node [A].  Nodes are numbered breadth-first in the order their
// edges are made: the edge into node n is entry n - 1 of child_tok, and a parent precedes its children.  The host checks the tables
// (AnswerTrie.score_to_device); the kernels still turn no table value into an address without a range check.
// Logits [R][V], R = G * Ni: row g * Ni + i is the next-token row of sample g at node internal[i].
//
// m3ae_listscore_lse, grid (chunk, row): the chunk work of m3ae_trie_scan and nothing else -- a workgroup reads its chunk of the row
//   once (walk_row) and writes (m, s) in fp32, in the order of operations of csrc/row_scan.h (MsAcc, block_ms_merge).
// m3ae_listscore_edges, one workgroup per row: every thread folds the row's pairs in ascending chunk order, lse = m + logf(s) (as
//   m3ae_trie_step), then edge_lp[g][e] = x[tok_e] - lse in fp32 for every child edge e of the row's node, 256 per pass.  A node
//   outside [0, N) or without a child range sets err and writes nothing; a token outside [0, V) sets err, is never an address, and its
//   edge is written as NaN.
// m3ae_listscore_fold, one workgroup per sample.
//   1. node_lp[0] = 0; level by level over level_off, node_lp[n] = node_lp[parent[n]] + (double)edge_lp[n - 1]: fp32 terms added in
//      double in path order, the rule of m3ae_trie_step -- on the same logits an entry's log-probability has the bits that search
//      would accumulate along the path.  node_lp lives in LDS for N <= LS_LDS_NODES, else in the caller's workspace.  A parent
//      that does not lie in an earlier level sets err and gives NaN.
//   2. all_logprob[b][i] = node_lp[leaf_node[i]]; len_i = depth[leaf_node[i]]; score_i = logprob_i / pen[len_i], pen a double table
//      [Dmax + 1] of len ** length_penalty from the caller.  A leaf outside [1, N) or a depth outside [1, Dmax] sets err and gives NaN.
//   3. log_mass = M + log(sum_i exp(logprob_i - M)), M = the greatest finite logprob: the terms are formed in parallel and added by one
//      thread in label order, in double.
//   4. The k <= 16 best entries by (score descending, label ascending): rank j is the greatest entry below rank j - 1, the selection
//      of csrc/topk_keep.h.  A double score and a label do not fit one 64-bit key, so a key is the pair (monotone image of the score,
//      label); a thread keeps the keys of its own entries in registers (the first 4; it forms further ones again each pass)
//      instead of a candidate table in LDS.  For rank j: labels, scores,
//      logprob, probs = exp(logprob - log_mass); ranks >= A hold label -1 and zeros.  best = labels[0], len = its token count.
//   Non-finite values.  An entry whose logprob is not finite (-inf, NaN) has probability 0 and adds nothing to the mass; if no entry
//   is finite, log_mass = -inf and every probability is 0.  A NaN score ranks after every number (-inf included), label ascending
//   among NaNs; -0 == +0.  None of this sets err: err is for tables.
// No atomics, every reduction in a fixed order: two runs on the same inputs give the same bits.
#include "common.h"
#include "row_scan.h"

namespace {

constexpr int LS_T = SCAN_T;
constexpr int64_t LS_DEF_CHUNK = 8192;       // m3ae_trie_scan's
constexpr int LS_LDS_NODES = 4096;           // 32 KiB of doubles
constexpr int LS_MAX_K = 16, LS_MAX_DEPTH = 32;
constexpr int LS_OWN = 4;                    // entries whose ranking key a thread keeps in registers (A <= 1024 in full)

template <typename T>
__global__ __launch_bounds__(LS_T) void listscore_lse_kernel(const T* __restrict__ logits, int64_t ld, int64_t V, int64_t chunk, int64_t nch,
                                                             float* __restrict__ ms) {
    __shared__ float redm[LS_T / 64], reds[LS_T / 64];
    const int64_t r = blockIdx.x / nch, c = blockIdx.x % nch;
    const int tid = threadIdx.x;
    const T* row = logits + r * ld;
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
__global__ __launch_bounds__(LS_T) void listscore_edges_kernel(const T* __restrict__ logits, int64_t ld, int64_t V, const float* __restrict__ ms,
                                                               int64_t nch, const int32_t* __restrict__ internal, int64_t Ni,
                                                               const int32_t* __restrict__ child_off, const int32_t* __restrict__ child_tok,
                                                               int64_t N, int64_t E, float* __restrict__ edge_lp, int64_t* __restrict__ err) {
    const int64_t r = blockIdx.x, g = r / Ni;
    const int tid = threadIdx.x;
    int64_t lo = 0, hi = 0;
    if (!child_range(child_off, internal[r % Ni], N, E, lo, hi)) {
        if (tid == 0) err[0] = 1;
        return;
    }
    float m = -INFINITY, s = 0.0f;
    const float* p2 = ms + 2 * r * nch;
    for (int64_t i = 0; i < nch; ++i) ms_merge(m, s, p2[2 * i], p2[2 * i + 1]);
    const float lse = m + logf(s);
    const T* row = logits + r * ld;
    for (int64_t e = lo + tid; e < hi; e += LS_T) {
        const int64_t tok = child_tok[e];
        float term = __uint_as_float(0x7fc00000u);
        if (tok >= 0 && tok < V) term = Elem<T>::ld(row + tok) - lse;
        else err[0] = 1;
        edge_lp[g * E + e] = term;
    }
}

// the monotone image of a double: greater score, greater key; NaN -> 1 (below every number), -0 -> +0; no key is 0
DEVINL uint64_t ord64(double d) {
    if (d != d) return 1;
    if (d == 0.0) d = 0.0;
    const uint64_t u = (uint64_t)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
// (ka, la) ranks before (kb, lb)
DEVINL bool before(uint64_t ka, int64_t la, uint64_t kb, int64_t lb) { return ka > kb || (ka == kb && la < lb); }

DEVINL uint64_t shfl_xor_u64(uint64_t v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(LS_T) void listscore_fold_kernel(const float* __restrict__ edge_lp, const int32_t* __restrict__ parent,
                                                              const int32_t* __restrict__ depth, const int32_t* __restrict__ level_off,
                                                              const int32_t* __restrict__ leaf_node, const double* __restrict__ pen,
                                                              int64_t N, int64_t A, int64_t Dmax, int64_t k, double* __restrict__ node_ws,
                                                              double* __restrict__ all_logprob, int64_t* __restrict__ labels,
                                                              double* __restrict__ scores, double* __restrict__ logprob,
                                                              double* __restrict__ probs, double* __restrict__ log_mass,
                                                              int64_t* __restrict__ n_hyp, int64_t* __restrict__ best, int64_t* __restrict__ len,
                                                              int64_t* __restrict__ err) {
    __shared__ double node_lds[LS_LDS_NODES];
    __shared__ double redd[LS_T / 64];
    __shared__ uint64_t redk[2][LS_T / 64];
    __shared__ int64_t redl[2][LS_T / 64];
    __shared__ double mass_sh;
    const int64_t b = blockIdx.x, E = N - 1;
    const int tid = threadIdx.x;
    double* node_lp = N <= LS_LDS_NODES ? node_lds : node_ws + b * N;
    const float* el = edge_lp + b * E;
    double* alp = all_logprob + b * A;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    // 1. the levels
    if (tid == 0) node_lp[0] = 0.0;
    __syncthreads();
    for (int64_t d = 1; d <= Dmax; ++d) {
        int64_t n0 = level_off[d], n1 = level_off[d + 1];
        if (n0 < 1 || n1 > N || n0 > n1) {      // wave-uniform: the level is skipped as a whole
            if (tid == 0) err[0] = 1;
            n0 = n1 = 0;
        }
        for (int64_t n = n0 + tid; n < n1; n += LS_T) {
            const int64_t p = parent[n];
            if (p < 0 || p >= n0) {              // a parent lies in an earlier level: nothing of this level's pass is read
                err[0] = 1;
                node_lp[n] = nan;
            } else {
                node_lp[n] = node_lp[p] + (double)el[n - 1];
            }
        }
        __syncthreads();
    }

    // 2. the entries; M = the greatest finite logprob
    double mx = -INFINITY;
    for (int64_t i = tid; i < A; i += LS_T) {
        const int64_t n = leaf_node[i];
        double lp = nan;
        if (n >= 1 && n < N) lp = node_lp[n];
        else err[0] = 1;
        alp[i] = lp;
        if (lp - lp == 0.0 && lp > mx) mx = lp;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double w = __longlong_as_double((long long)shfl_xor_u64((uint64_t)__double_as_longlong(mx), o));
        mx = w > mx ? w : mx;
    }
    if ((tid & 63) == 0) redd[tid >> 6] = mx;
    __syncthreads();                              // also: every thread is through with node_lp
    mx = redd[0];
    for (int w = 1; w < LS_T / 64; ++w) mx = redd[w] > mx ? redd[w] : mx;

    // 3. the mass: terms in parallel (into node_lp, which has N > A slots), their sum in label order
    for (int64_t i = tid; i < A; i += LS_T) {
        const double lp = alp[i];                 // this thread's own store
        node_lp[i] = (lp - lp == 0.0) ? exp(lp - mx) : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int64_t i = 0; i < A; ++i) sum += node_lp[i];
        const double lm = mx == -INFINITY ? -INFINITY : mx + log(sum);
        mass_sh = lm;
        log_mass[b] = lm;
        n_hyp[b] = k < A ? k : A;
    }
    __syncthreads();
    const double lm = mass_sh;

    // 4. the k best.  The key of an entry is formed once: a thread keeps the keys of its first LS_OWN entries (all of them up to
    // A = LS_OWN * 256) in registers and forms the others again in every pass.
    auto key_at = [&](int64_t i) -> uint64_t {
        const int64_t n = leaf_node[i];
        const int64_t dl = (n >= 1 && n < N) ? depth[n] : 0;
        return ord64((dl >= 1 && dl <= Dmax) ? alp[i] / pen[dl] : nan);
    };
    uint64_t own[LS_OWN];
#pragma unroll
    for (int s = 0; s < LS_OWN; ++s) {
        const int64_t i = tid + (int64_t)s * LS_T;
        own[s] = i < A ? key_at(i) : 0;          // 0: no entry
    }
    uint64_t pk = 0;
    int64_t pl = -1;
    for (int64_t j = 0; j < k; ++j) {
        uint64_t bk = 0;
        int64_t bl = -1;
        if (j < A) {
            auto take = [&](uint64_t key, int64_t i) {
                if ((j == 0 || before(pk, pl, key, i)) && (bk == 0 || before(key, i, bk, bl))) { bk = key; bl = i; }
            };
#pragma unroll
            for (int s = 0; s < LS_OWN; ++s) {
                if (own[s] != 0) take(own[s], tid + (int64_t)s * LS_T);
            }
            for (int64_t i = tid + (int64_t)LS_OWN * LS_T; i < A; i += LS_T) take(key_at(i), i);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint64_t wk = shfl_xor_u64(bk, o);
                const int64_t wl = (int64_t)shfl_xor_u64((uint64_t)bl, o);
                if (wk != 0 && (bk == 0 || before(wk, wl, bk, bl))) { bk = wk; bl = wl; }
            }
            if ((tid & 63) == 0) { redk[j & 1][tid >> 6] = bk; redl[j & 1][tid >> 6] = bl; }
            __syncthreads();      // one barrier a pass: pass j + 2 reuses the slot only after every thread has passed the barrier of j + 1
            bk = redk[j & 1][0];
            bl = redl[j & 1][0];
            for (int w = 1; w < LS_T / 64; ++w) {
                const uint64_t wk = redk[j & 1][w];
                const int64_t wl = redl[j & 1][w];
                if (wk != 0 && (bk == 0 || before(wk, wl, bk, bl))) { bk = wk; bl = wl; }
            }
            pk = bk;
            pl = bl;
        }
        if (tid == 0) {
            const int64_t slot = b * k + j;
            if (j < A && bl >= 0 && bl < A) {
                const int64_t n = leaf_node[bl];
                const int64_t dl = (n >= 1 && n < N) ? depth[n] : 0;
                const bool ok = dl >= 1 && dl <= Dmax;
                const double lp = alp[bl];
                if (!ok) err[0] = 1;
                labels[slot] = bl;
                scores[slot] = ok ? lp / pen[dl] : nan;
                logprob[slot] = lp;
                probs[slot] = (lp - lp == 0.0 && lm != -INFINITY) ? exp(lp - lm) : 0.0;
                if (j == 0) { best[b] = bl; len[b] = ok ? dl : 0; }
            } else {
                labels[slot] = -1;
                scores[slot] = 0.0;
                logprob[slot] = 0.0;
                probs[slot] = 0.0;
            }
        }
    }
}

inline bool ls_chunk_ok(int64_t R, int64_t V, int64_t chunk) { return chunk_shape_ok(R, V, chunk, 0); }

}  // namespace

extern "C" int64_t m3ae_listscore_workspace_bytes(int64_t R, int64_t V, int64_t chunk) {
    if (chunk == 0) chunk = LS_DEF_CHUNK;
    if (!ls_chunk_ok(R, V, chunk)) return 0;
    return R * cdiv(V, chunk) * 8;
}

extern "C" int m3ae_listscore_lse(const void* logits, int64_t ld, int64_t R, int64_t V, int64_t chunk, int dtype, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    if (!logits || R < 1 || V < 1 || ld < V || chunk < 0) return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (chunk == 0) chunk = LS_DEF_CHUNK;
    if (!ls_chunk_ok(R, V, chunk)) return M3AE_ERR_UNSUPPORTED;
    if ((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) return M3AE_ERR_ALIGN;
    const int64_t nch = cdiv(V, chunk);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < R * nch * 8) return M3AE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(listscore_lse_kernel<T>, dim3((unsigned)(R * nch)), dim3(LS_T), 0, s, (const T*)logits, ld, V, chunk, nch,
                           (float*)workspace);
    });
    return hip_launch_status();
}

extern "C" int m3ae_listscore_edges(const void* logits, int64_t ld, int64_t G, int64_t Ni, int64_t V, int dtype, const void* workspace,
                                    int64_t workspace_bytes, int64_t nch, const int32_t* internal, const int32_t* child_off,
                                    const int32_t* child_tok, int64_t N, int64_t E, float* edge_lp, int64_t* err, void* stream) {
    if (!logits || !internal || !child_off || !child_tok || !edge_lp || !err || G < 1 || Ni < 1 || V < 1 || ld < V || nch < 1 || N < 1 || E < 1)
        return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (V > (int64_t)INT32_MAX || N > (int64_t)INT32_MAX || E > (int64_t)INT32_MAX || Ni > N || G > (int64_t)INT32_MAX ||
        G * Ni > (int64_t)INT32_MAX || nch > (int64_t)INT32_MAX)
        return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) || ((uintptr_t)internal & 3) || ((uintptr_t)child_off & 3) ||
        ((uintptr_t)child_tok & 3) || ((uintptr_t)edge_lp & 3) || ((uintptr_t)err & 7))
        return M3AE_ERR_ALIGN;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < G * Ni * nch * 8) return M3AE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(listscore_edges_kernel<T>, dim3((unsigned)(G * Ni)), dim3(LS_T), 0, s, (const T*)logits, ld, V,
                           (const float*)workspace, nch, internal, Ni, child_off, child_tok, N, E, edge_lp, err);
    });
    return hip_launch_status();
}

extern "C" int64_t m3ae_listscore_fold_workspace_bytes(int64_t B, int64_t N) {
    if (B < 1 || N < 2 || N > (int64_t)INT32_MAX || B > (int64_t)INT32_MAX) return -1;
    return N <= LS_LDS_NODES ? 0 : B * N * 8;
}

extern "C" int m3ae_listscore_fold(const float* edge_lp, const int32_t* parent, const int32_t* depth, const int32_t* level_off,
                                   const int32_t* leaf_node, const double* pen, int64_t B, int64_t N, int64_t A, int64_t Dmax, int64_t k,
                                   void* workspace, int64_t workspace_bytes, double* all_logprob, int64_t* labels, double* scores,
                                   double* logprob, double* probs, double* log_mass, int64_t* n_hyp, int64_t* best, int64_t* len,
                                   int64_t* err, void* stream) {
    if (!edge_lp || !parent || !depth || !level_off || !leaf_node || !pen || !all_logprob || !labels || !scores || !logprob || !probs ||
        !log_mass || !n_hyp || !best || !len || !err || B < 1 || N < 2 || A < 1 || Dmax < 1 || k < 1)
        return M3AE_ERR_ARG;
    if (k > LS_MAX_K || Dmax > LS_MAX_DEPTH || A >= N || N > (int64_t)INT32_MAX || B > (int64_t)INT32_MAX) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)edge_lp & 3) || ((uintptr_t)parent & 3) || ((uintptr_t)depth & 3) || ((uintptr_t)level_off & 3) ||
        ((uintptr_t)leaf_node & 3) || ((uintptr_t)pen & 7) || ((uintptr_t)all_logprob & 7) || ((uintptr_t)labels & 7) ||
        ((uintptr_t)scores & 7) || ((uintptr_t)logprob & 7) || ((uintptr_t)probs & 7) || ((uintptr_t)log_mass & 7) ||
        ((uintptr_t)n_hyp & 7) || ((uintptr_t)best & 7) || ((uintptr_t)len & 7) || ((uintptr_t)err & 7))
        return M3AE_ERR_ALIGN;
    const int64_t need = N <= LS_LDS_NODES ? 0 : B * N * 8;
    if (need && (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need)) return M3AE_ERR_WORKSPACE;
    hipLaunchKernelGGL(listscore_fold_kernel, dim3((unsigned)B), dim3(LS_T), 0, (hipStream_t)stream, edge_lp, parent, depth, level_off,
                       leaf_node, pen, N, A, Dmax, k, (double*)workspace, all_logprob, labels, scores, logprob, probs, log_mass, n_hyp, best,
                       len, err);
    return hip_launch_status();
}
