// Constrained beam search on the answer list (Decoder.answer_beam_async, T5.constrained_beam_async): the transformers-4.6.0
// `beam_search` + `BeamSearchScorer` of csrc/beam.hip with the prefix trie of csrc/answer_trie.hip as the constraint, and an n-best
// list of answers with scores as the result.  Log-probabilities come from the UNCONSTRAINED softmax; a token the trie does not
// allow is simply not a candidate.
//
// State of the R = B * nb beam rows, 1 <= nb <= 8: node int32 (-1 = a DEAD slot), beam_score fp32, last_tok int64.  At the start
// slot 0 of every sample is at the root with score 0 and the others are dead: a dead slot contributes no candidate (there is no
// -1e9 trick).  m3ae_trie_scan runs unchanged over the R rows with the dead flags as its `finished` argument; of its workspace the
// (m, s) pairs are used here.
//
// m3ae_triebeam_select, one workgroup of 256 threads per sample: thread k < nb folds the (m, s) pairs of live beam k in ascending
//   chunk order, lse = m + logf(s) (csrc/answer_trie.hip's step).  The workgroup then walks the children of every live beam's node
//   in passes of 256; child entry e (an index into child_tok / child_node, ascending in token within a node) of beam k gives
//   score = fl(fl(x[tok] - lse) + beam_score) and the order key (monotone image of the score) << 32 | (2^32 - 1 - (k * E + e))
//   with eval_key's NaN / -0 handling.  Every thread keeps its best 2 nb keys in LDS and the ranks are read off as in
//   csrc/vqa_eval.hip: the best min(2 nb, candidates) by (rounded score descending, (beam, token) ascending), a NaN first.
// m3ae_triebeam_step, one workgroup, a thread per sample (csrc/answer_trie.hip's step): walks the ranks, pushes leaves at rank < nb
//   into the sample's hypothesis list (csrc/hyp_list.h), fills the next beam slots, writes the gather order of the caches and the
//   dead flags, and counts the samples not done.
//   Its per-thread arrays of MAX_BEAMS entries (the old nodes and the next slots' node / score / token / source) are indexed at run
//   time and may live in scratch (up to 224 bytes a thread): accepted for one thread per sample on a kernel of a few microseconds
//   (the no-scratch rule of m3ae_amd/build.py covers the kernels with inline-asm epilogue loads, which this file has none of).
// No atomics; keys of distinct (beam, entry) pairs are distinct: two runs on the same inputs give the same bits.
#include "common.h"
#include "hyp_list.h"
#include "row_scan.h"
#include "topk_keep.h"

extern "C" int64_t m3ae_trie_workspace_bytes(int64_t R, int64_t V, int64_t chunk);   // csrc/answer_trie.hip: its default chunk

namespace {

constexpr int TB = KEEP_T;       // threads of both kernels (256: the scheme of csrc/topk_keep.h)
static_assert(KEEP_T == SCAN_T, "walk_row and the folds stride by SCAN_T, the candidate scheme by KEEP_T");
constexpr int TB_MAX_BEAMS = 8;
constexpr int TB_MAX_K = 2 * TB_MAX_BEAMS;

template <typename T>
__global__ __launch_bounds__(TB) void trie_beam_select_kernel(const T* __restrict__ logits, int64_t ld, int64_t V, const float* __restrict__ ms,
                                                              int64_t nch, const int32_t* __restrict__ child_off,
                                                              const int32_t* __restrict__ child_tok, int64_t N, int64_t E,
                                                              const int32_t* __restrict__ node, const float* __restrict__ beam_score, int nb,
                                                              float* __restrict__ top_s, int32_t* __restrict__ top_beam,
                                                              int32_t* __restrict__ top_edge, int32_t* __restrict__ n_cand,
                                                              int64_t* __restrict__ err) {
    __shared__ uint64_t cand[TB_MAX_K * TB];
    __shared__ uint64_t red[2][TB / 64];
    __shared__ uint64_t sel[TB_MAX_K];
    __shared__ float s_lse[TB_MAX_BEAMS], s_bs[TB_MAX_BEAMS];
    __shared__ int64_t s_lo[TB_MAX_BEAMS], s_hi[TB_MAX_BEAMS];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int kk = 2 * nb;
    for (int s = 0; s < kk; ++s) cand[s * TB + tid] = 0;   // a thread reads and writes its own column of cand only
    Keep keep{cand + tid, kk, 0, 0};

    if (tid < nb) {
        const int64_t r = b * nb + tid;
        const int64_t nd = node[r];
        int64_t lo = 0, hi = 0;          // lo == hi: the beam has no candidate
        float lse = 0.0f, bs = 0.0f;
        if (nd >= 0) {                   // a dead slot: nothing of its row is read, the (m, s) pairs included
            if (child_range(child_off, nd, N, E, lo, hi)) {
                float m = -INFINITY, s = 0.0f;
                const float* p = ms + 2 * r * nch;
                for (int64_t i = 0; i < nch; ++i) ms_merge(m, s, p[2 * i], p[2 * i + 1]);
                lse = m + logf(s);
                bs = beam_score[r];
            } else {
                lo = hi = 0;
                err[0] = 1;
            }
        }
        s_lse[tid] = lse; s_bs[tid] = bs; s_lo[tid] = lo; s_hi[tid] = hi;
    }
    __syncthreads();

    for (int k = 0; k < nb; ++k) {
        const int64_t lo = s_lo[k], hi = s_hi[k];
        const float lse = s_lse[k], bs = s_bs[k];
        const T* row = logits + (b * nb + k) * ld;
        for (int64_t e = lo + tid; e < hi; e += TB) {
            const int64_t tok = child_tok[e];
            if (tok < 0 || tok >= V) { err[0] = 1; continue; }   // never an address
            const float lp = Elem<T>::ld(row + tok) - lse;
            const float sc = lp + bs;
            keep.put(eval_key(__float_as_uint(sc), (uint32_t)(k * E + e)));
        }
    }

    keep_select(cand, kk, red, sel, tid);   // rank j = the greatest candidate below rank j - 1 (rank 0: the greatest)

    if (tid < kk) {
        const int64_t flat = key_index_in(sel[tid], (int64_t)nb * E);
        const bool ok = flat >= 0;
        top_s[b * kk + tid] = ok ? key_value(sel[tid]) : 0.0f;
        top_beam[b * kk + tid] = ok ? (int32_t)(flat / E) : -1;
        top_edge[b * kk + tid] = ok ? (int32_t)(flat % E) : -1;
    }
    if (tid == 0) {
        int n = 0;
        for (int j = 0; j < kk; ++j) n += sel[j] != 0 ? 1 : 0;
        n_cand[b] = n;
    }
}

__global__ __launch_bounds__(TB) void trie_beam_step_kernel(const float* __restrict__ top_s, const int32_t* __restrict__ top_beam,
                                                            const int32_t* __restrict__ top_edge, const int32_t* __restrict__ child_off,
                                                            const int32_t* __restrict__ child_tok, const int32_t* __restrict__ child_node,
                                                            const int32_t* __restrict__ leaf_label, int64_t N, int64_t E,
                                                            int32_t* __restrict__ node, float* __restrict__ beam_score,
                                                            int64_t* __restrict__ last_tok, int64_t* __restrict__ order,
                                                            int32_t* __restrict__ dead, int32_t* __restrict__ done, int64_t* __restrict__ n_hyp,
                                                            int64_t* __restrict__ labels, double* __restrict__ scores,
                                                            double* __restrict__ logprob, int64_t* __restrict__ hyp_len,
                                                            int64_t* __restrict__ best, int64_t* __restrict__ len,
                                                            int32_t* __restrict__ open_count, int64_t* __restrict__ err, int64_t B, int nb,
                                                            int64_t V, int64_t A, int64_t pos, int64_t pad, double div) {
    __shared__ int red[TB / 64];
    const int tid = threadIdx.x;
    const int kk = 2 * nb;
    int open = 0;
    for (int64_t b = tid; b < B; b += TB) {
        int32_t old_node[TB_MAX_BEAMS], new_node[TB_MAX_BEAMS];
        float new_score[TB_MAX_BEAMS];
        int64_t new_tok[TB_MAX_BEAMS], new_src[TB_MAX_BEAMS];
        int k = 0;
        bool is_done = done[b] != 0;
        if (!is_done) {
            for (int j = 0; j < nb; ++j) old_node[j] = node[b * nb + j];
            int n = (int)n_hyp[b];
            n = n < 0 ? 0 : (n > nb ? nb : n);
            double* hs = scores + b * nb;
            double* hr = logprob + b * nb;
            int64_t* hl = labels + b * nb;
            int64_t* hn = hyp_len + b * nb;
            for (int rank = 0; rank < kk && k < nb; ++rank) {
                const int64_t e = top_edge[b * kk + rank], bm = top_beam[b * kk + rank];
                if (e == -1 && bm == -1) continue;             // an unused slot
                if (bm < 0 || bm >= nb || e < 0 || e >= E) { err[0] = 1; continue; }   // never an address
                int64_t lo = 0, hi = 0;
                if (!child_range(child_off, old_node[bm], N, E, lo, hi) || e < lo || e >= hi) { err[0] = 1; continue; }
                const int64_t tok = child_tok[e], nn = child_node[e];
                if (tok < 0 || tok >= V || nn < 0 || nn >= N) { err[0] = 1; continue; }
                const float s = top_s[b * kk + rank];
                const int32_t lab = leaf_label[nn];
                if (lab >= A) { err[0] = 1; continue; }       // best[] indexes the answers table by it
                if (lab >= 0) {
                    if (rank >= nb) continue;
                    const double sc = (double)s / div;
                    int last = 0;
                    const int p = hyp_insert_pos(sc, nb, n, hs, last);
                    if (p < 0) continue;
                    for (int q = last; q > p; --q) { hs[q] = hs[q - 1]; hr[q] = hr[q - 1]; hl[q] = hl[q - 1]; hn[q] = hn[q - 1]; }
                    hs[p] = sc; hr[p] = (double)s; hl[p] = lab; hn[p] = pos + 1;
                    n = hyp_count(n, nb);
                } else {
                    new_score[k] = s; new_tok[k] = tok; new_src[k] = b * nb + bm; new_node[k] = (int32_t)nn;
                    ++k;
                }
            }
            n_hyp[b] = n;
            if (n > 0) {
                best[b] = hl[0] < 0 ? 0 : hl[0];   // a row of the answers table whatever happened: the gather of seq reads it
                len[b] = hn[0];
            }
            is_done = n >= nb || k == 0;
            if (is_done) { done[b] = 1; k = 0; }
        }
        for (int j = 0; j < nb; ++j) {
            const int64_t r = b * nb + j;
            const bool live = j < k;
            node[r] = live ? new_node[j] : -1;
            beam_score[r] = live ? new_score[j] : 0.0f;
            last_tok[r] = live ? new_tok[j] : pad;
            order[r] = live ? new_src[j] : b * nb;
            dead[r] = live ? 0 : 1;
        }
        open += is_done ? 0 : 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) open += __shfl_xor(open, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = open;
    __syncthreads();
    if (tid == 0) open_count[pos] = red[0] + red[1] + red[2] + red[3];
}

}  // namespace

extern "C" int m3ae_triebeam_select(const void* logits, int64_t ld, int64_t B, int64_t nb, int64_t V, int64_t chunk, int dtype,
                                     const int32_t* child_off, const int32_t* child_tok, int64_t N, int64_t E, const int32_t* node,
                                     const float* beam_score, const void* workspace, int64_t workspace_bytes, float* top_s,
                                     int32_t* top_beam, int32_t* top_edge, int32_t* n_cand, int64_t* err, void* stream) {
    if (!logits || !child_off || !child_tok || !node || !beam_score || !top_s || !top_beam || !top_edge || !n_cand || !err || B < 1 || V < 1 ||
        ld < V || chunk < 0 || N < 1 || E < 1)
        return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (nb < 1 || nb > TB_MAX_BEAMS || B > (int64_t)INT32_MAX / nb || N > (int64_t)INT32_MAX || E > (int64_t)INT32_MAX ||
        nb * E > (int64_t)INT32_MAX)
        return M3AE_ERR_UNSUPPORTED;
    const int64_t R = B * nb;
    const int64_t need = m3ae_trie_workspace_bytes(R, V, chunk);   // 0: not a shape m3ae_trie_scan takes
    if (need <= 0) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) || ((uintptr_t)child_off & 3) || ((uintptr_t)child_tok & 3) || ((uintptr_t)node & 3) ||
        ((uintptr_t)beam_score & 3) || ((uintptr_t)top_s & 3) || ((uintptr_t)top_beam & 3) || ((uintptr_t)top_edge & 3) || ((uintptr_t)n_cand & 3) ||
        ((uintptr_t)err & 7))
        return M3AE_ERR_ALIGN;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need) return M3AE_ERR_WORKSPACE;
    const int64_t nch = need / (8 * R) - 1;                         // workspace: child key u64 [R] | (m, s) fp32 [R][chunks][2]
    const float* ms = (const float*)((const uint64_t*)workspace + R);
    hipStream_t s = (hipStream_t)stream;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(trie_beam_select_kernel<T>, dim3((unsigned)B), dim3(TB), 0, s, (const T*)logits, ld, V, ms, nch, child_off, child_tok,
                           N, E, node, beam_score, (int)nb, top_s, top_beam, top_edge, n_cand, err);
    });
    return hip_launch_status();
}

extern "C" int m3ae_triebeam_step(const float* top_s, const int32_t* top_beam, const int32_t* top_edge, const int32_t* child_off,
                                   const int32_t* child_tok, const int32_t* child_node, const int32_t* leaf_label, int64_t N, int64_t E,
                                   int32_t* node, float* beam_score, int64_t* last_tok, int64_t* order, int32_t* dead, int32_t* done,
                                   int64_t* n_hyp, int64_t* labels, double* scores, double* logprob, int64_t* hyp_len, int64_t* best,
                                   int64_t* len, int32_t* open_count, int64_t* err, int64_t B, int64_t nb, int64_t V, int64_t A, int64_t max_len,
                                   int64_t pos, int64_t pad, double div, void* stream) {
    if (!top_s || !top_beam || !top_edge || !child_off || !child_tok || !child_node || !leaf_label || !node || !beam_score || !last_tok ||
        !order || !dead || !done || !n_hyp || !labels || !scores || !logprob || !hyp_len || !best || !len || !open_count || !err || B < 1 ||
        V < 1 || V > (int64_t)INT32_MAX || A < 1 || N < 1 || E < 1 || max_len < 1 || max_len > (int64_t)INT32_MAX || pos < 0 || pos >= max_len ||
        !(div > 0.0))
        return M3AE_ERR_ARG;
    if (nb < 1 || nb > TB_MAX_BEAMS || B > (int64_t)INT32_MAX / nb || N > (int64_t)INT32_MAX || E > (int64_t)INT32_MAX ||
        nb * E > (int64_t)INT32_MAX)
        return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)top_s & 3) || ((uintptr_t)top_beam & 3) || ((uintptr_t)top_edge & 3) || ((uintptr_t)child_off & 3) ||
        ((uintptr_t)child_tok & 3) || ((uintptr_t)child_node & 3) || ((uintptr_t)leaf_label & 3) || ((uintptr_t)node & 3) ||
        ((uintptr_t)beam_score & 3) || ((uintptr_t)last_tok & 7) || ((uintptr_t)order & 7) || ((uintptr_t)dead & 3) || ((uintptr_t)done & 3) ||
        ((uintptr_t)n_hyp & 7) || ((uintptr_t)labels & 7) || ((uintptr_t)scores & 7) || ((uintptr_t)logprob & 7) || ((uintptr_t)hyp_len & 7) ||
        ((uintptr_t)best & 7) || ((uintptr_t)len & 7) || ((uintptr_t)open_count & 3) || ((uintptr_t)err & 7))
        return M3AE_ERR_ALIGN;
    hipLaunchKernelGGL(trie_beam_step_kernel, dim3(1), dim3(TB), 0, (hipStream_t)stream, top_s, top_beam, top_edge, child_off, child_tok,
                       child_node, leaf_label, N, E, node, beam_score, last_tok, order, dead, done, n_hyp, labels, scores, logprob, hyp_len,
                       best, len, open_count, err, B, (int)nb, V, A, pos, pad, div);
    return hip_launch_status();
}
