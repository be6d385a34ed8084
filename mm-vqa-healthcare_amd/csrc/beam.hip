// Device-resident beam search for T5 generate (m3ae_amd/modules/t5.py::generate_async): the log-softmax + top-2*beams candidate
// selection over the vocabulary, the BeamSearchScorer step and the final hypothesis pick, with no host involvement.
//
// m3ae_beam_topk, three launches:
//   1 stats   grid (vocabulary chunk, row): chunk maximum and sum of exp(x - chunk maximum); fixed order (strided per-thread sums,
//             xor butterfly, four wave partials added by one thread).
//   2 select  grid (vocabulary chunk, row): every workgroup folds the row's chunk statistics in ascending chunk order into
//             m = max x and lse = log sum exp(x - m) (all workgroups of a row compute the same bits), forms
//             score = fl(fl(fl(x - m) - lse) + beam_score) for its chunk and keeps the chunk's best 2*beams by the key below.
//   3 merge   grid (sample): best 2*beams of the sample's beams * chunks * 2*beams survivors, same key.
// The order key is one 64-bit integer, (monotone image of the fp32 score) << 32 | (2^32 - 1 - flat index): its maximum is the
// highest ROUNDED score, the lowest flat index beam * V + token among equals.  Selecting on the rounded score (a second pass over
// the row, out of L2) is what makes distinct logits that round to one score come out in index order.  Keys are unique (the index
// is part of them) and a taken key is cleared, so the indices of a result are distinct and in range whatever the logits hold.
// No atomics: every output bit depends on the inputs and the shapes alone.
//
// m3ae_beam_step / m3ae_beam_finalize: one wave per sample; lane 0 walks the candidates (hypothesis lists in double, as the
// host's Python floats), the wave copies the token rows.
#include "common.h"
#include "order_key.h"   // ord32 / unord32 / make_key / wave_max_u64, shared with csrc/greedy.hip
#include "hyp_list.h"

namespace {

constexpr int BT = 256;          // threads of the top-k kernels
constexpr int MAX_CHUNK = 4096;  // keys of one chunk live in LDS (32 KB)
constexpr int DEF_CHUNK = 2048;
constexpr int MAX_BEAMS = 8;

// The K largest keys of keys[0..n) (0 = empty slot) in descending order into out[0..K); thread t owns keys[t], keys[t + BT], ...
// (reads and clears only those), so the one barrier per round is the exchange of the wave maxima (double-buffered).
DEVINL void block_topk(uint64_t* keys, int64_t n, int K, uint64_t* out, uint64_t (*wbest)[BT / 64]) {
    const int tid = threadIdx.x;
    uint64_t mine = 0;
    for (int64_t j = tid; j < n; j += BT) { const uint64_t k = keys[j]; mine = k > mine ? k : mine; }
    for (int r = 0; r < K; ++r) {
        const uint64_t w = wave_max_u64(mine);
        if ((tid & 63) == 0) wbest[r & 1][tid >> 6] = w;
        __syncthreads();
        uint64_t g = wbest[r & 1][0];
#pragma unroll
        for (int i = 1; i < BT / 64; ++i) g = wbest[r & 1][i] > g ? wbest[r & 1][i] : g;
        if (tid == 0) out[r] = g;
        if (g != 0 && g == mine) {
            mine = 0;
            for (int64_t j = tid; j < n; j += BT) {
                uint64_t k = keys[j];
                if (k == g) { keys[j] = 0; k = 0; }
                mine = k > mine ? k : mine;
            }
        }
    }
}

__global__ __launch_bounds__(BT) void beam_stats_kernel(const float* __restrict__ logits, int64_t ld, int64_t V, int64_t chunk,
                                                        int64_t nch, float* __restrict__ part) {
    __shared__ float red[BT / 64];
    const int64_t r = blockIdx.x / nch, c = blockIdx.x % nch;
    const int64_t v0 = c * chunk;
    const int64_t n = (V - v0) < chunk ? (V - v0) : chunk;
    const float* x = logits + r * ld + v0;
    const int tid = threadIdx.x;
    float m = -INFINITY;
    for (int64_t j = tid; j < n; j += BT) m = fmaxf(m, x[j]);
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
    for (int64_t j = tid; j < n; j += BT) s += expf(x[j] - m);
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        s = ((red[0] + red[1]) + red[2]) + red[3];
        part[2 * blockIdx.x] = m;
        part[2 * blockIdx.x + 1] = m == -INFINITY ? 0.f : s;   // a chunk of -inf alone adds nothing to the row's sum
    }
}

__global__ __launch_bounds__(BT) void beam_select_kernel(const float* __restrict__ logits, int64_t ld, const float* __restrict__ beam_scores,
                                                         int64_t nb, int64_t V, int64_t chunk, int64_t nch, int K,
                                                         const float* __restrict__ part, uint64_t* __restrict__ cand) {
    __shared__ uint64_t keys[MAX_CHUNK];
    __shared__ uint64_t wbest[2][BT / 64];
    const int64_t r = blockIdx.x / nch, c = blockIdx.x % nch;
    const float* pr = part + 2 * r * nch;
    float m = pr[0];
    for (int64_t i = 1; i < nch; ++i) m = fmaxf(m, pr[2 * i]);
    float s = 0.f;
    for (int64_t i = 0; i < nch; ++i) s += pr[2 * i + 1] * expf(pr[2 * i] - m);
    const float lse = logf(s);
    const float bs = beam_scores[r];
    const int64_t v0 = c * chunk;
    const int64_t n = (V - v0) < chunk ? (V - v0) : chunk;
    const float* x = logits + r * ld + v0;
    const uint32_t flat0 = (uint32_t)((r % nb) * V + v0);
    for (int64_t j = threadIdx.x; j < n; j += BT) {
        const float d = x[j] - m;
        const float lp = d - lse;
        const float sc = (lp + bs) + 0.0f;   // -0 -> +0: one key per value
        keys[j] = make_key(sc, flat0 + (uint32_t)j);
    }
    __syncthreads();
    block_topk(keys, n, K, cand + (int64_t)blockIdx.x * K, wbest);
}

__global__ __launch_bounds__(BT) void beam_merge_kernel(uint64_t* __restrict__ cand, int64_t per_sample, int K, float* __restrict__ top_s,
                                                        int32_t* __restrict__ top_i) {
    __shared__ uint64_t best[2 * MAX_BEAMS];
    __shared__ uint64_t wbest[2][BT / 64];
    const int64_t b = blockIdx.x;
    block_topk(cand + b * per_sample, per_sample, K, best, wbest);
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const uint64_t g = best[threadIdx.x];
        top_s[b * K + threadIdx.x] = unord32((uint32_t)(g >> 32));
        top_i[b * K + threadIdx.x] = (int32_t)key_index(g);
    }
}

// ---- BeamSearchScorer ------------------------------------------------------------------------------------------------------------
// Hypothesis list of one sample: scores descending, a new entry goes AFTER entries of equal score (Python's stable sorted() on the
// appended list), then the list is cut to nb.
DEVINL void hyp_push(double score, const int64_t* row, int len, int nb, int max_length, int32_t& n, double* hs, int32_t* hl,
                     int64_t* ht) {
    int last = 0;
    const int p = hyp_insert_pos(score, nb, n, hs, last);   // csrc/hyp_list.h, shared with csrc/trie_beam.hip
    if (p < 0) return;
    for (int q = last; q > p; --q) {
        hs[q] = hs[q - 1];
        hl[q] = hl[q - 1];
        for (int j = 0; j < max_length; ++j) ht[(int64_t)q * max_length + j] = ht[(int64_t)(q - 1) * max_length + j];
    }
    hs[p] = score;
    hl[p] = len;
    for (int j = 0; j < max_length; ++j) ht[(int64_t)p * max_length + j] = j < len ? row[j] : 0;
    n = hyp_count(n, nb);
}

__global__ __launch_bounds__(64) void beam_step_kernel(const float* __restrict__ top_s, const int32_t* __restrict__ top_i,
                                                       const int64_t* __restrict__ ids_in, int64_t* __restrict__ ids_out,
                                                       int64_t* __restrict__ last_tok, float* __restrict__ beam_scores,
                                                       int64_t* __restrict__ order, int32_t* __restrict__ done, int32_t* __restrict__ n_hyp,
                                                       double* __restrict__ hyp_score, int32_t* __restrict__ hyp_len,
                                                       int64_t* __restrict__ hyp_tok, int64_t* __restrict__ err, int nb, int64_t V,
                                                       int max_length, int cur_len, int64_t eos, int64_t pad, double div) {
    __shared__ int64_t s_src[MAX_BEAMS], s_tok[MAX_BEAMS];
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    if (lane == 0) {
        float sc[MAX_BEAMS];
        for (int k = 0; k < nb; ++k) { s_src[k] = b * nb; s_tok[k] = pad; sc[k] = 0.f; }
        if (!done[b]) {
            int32_t n = n_hyp[b];
            double* hs = hyp_score + b * nb;
            int32_t* hl = hyp_len + b * nb;
            int64_t* ht = hyp_tok + b * nb * max_length;
            int k = 0;
            for (int rank = 0; rank < 2 * nb && k < nb; ++rank) {
                const int64_t i = top_i[b * 2 * nb + rank];
                if (i < 0 || i >= (int64_t)nb * V) { err[0] = 1; continue; }   // never an address
                const int64_t src = b * nb + i / V, tok = i % V;
                const float s = top_s[b * 2 * nb + rank];
                if (tok == eos) {
                    if (rank >= nb) continue;
                    hyp_push((double)s / div, ids_in + src * max_length, cur_len, nb, max_length, n, hs, hl, ht);
                } else {
                    sc[k] = s; s_tok[k] = tok; s_src[k] = src;
                    ++k;
                }
            }
            n_hyp[b] = n;
            if (n >= nb) done[b] = 1;
        }
        for (int k = 0; k < nb; ++k) {
            beam_scores[b * nb + k] = sc[k];
            order[b * nb + k] = s_src[k];
            last_tok[b * nb + k] = s_tok[k];
        }
    }
    __syncthreads();
    for (int k = 0; k < nb; ++k) {
        const int64_t* src = ids_in + s_src[k] * max_length;
        int64_t* dst = ids_out + (b * nb + k) * max_length;
        for (int j = lane; j < cur_len; j += 64) dst[j] = src[j];
        if (lane == 0) dst[cur_len] = s_tok[k];
    }
}

__global__ __launch_bounds__(BT) void beam_open_count_kernel(const int32_t* __restrict__ done, int64_t B, int32_t* __restrict__ out) {
    __shared__ int red[BT / 64];
    int c = 0;
    for (int64_t i = threadIdx.x; i < B; i += BT) c += done[i] ? 0 : 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(64) void beam_finalize_kernel(const int64_t* __restrict__ ids, const float* __restrict__ beam_scores,
                                                           const int32_t* __restrict__ done, int32_t* __restrict__ n_hyp,
                                                           double* __restrict__ hyp_score, int32_t* __restrict__ hyp_len,
                                                           int64_t* __restrict__ hyp_tok, int64_t* __restrict__ seq, int64_t* __restrict__ len,
                                                           int nb, int max_length, int cur_len, int64_t eos, int64_t pad, double div) {
    __shared__ int s_len;
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    int64_t* ht = hyp_tok + b * nb * max_length;
    if (lane == 0) {
        int32_t n = n_hyp[b];
        if (!done[b]) {
            for (int j = 0; j < nb; ++j)
                hyp_push((double)beam_scores[b * nb + j] / div, ids + (b * nb + j) * max_length, cur_len, nb, max_length, n,
                         hyp_score + b * nb, hyp_len + b * nb, ht);
            n_hyp[b] = n;
        }
        int l = n > 0 ? hyp_len[b * nb] : 0;
        l = l < 0 ? 0 : (l > max_length ? max_length : l);
        s_len = l;
        len[b] = l;
    }
    __syncthreads();
    const int l = s_len;
    for (int j = lane; j < max_length; j += 64) seq[b * max_length + j] = j < l ? ht[j] : (j == l ? eos : pad);
}

inline bool topk_shape_ok(int64_t B, int64_t nb, int64_t V, int64_t chunk) {
    return B >= 1 && nb >= 1 && nb <= MAX_BEAMS && V >= 2 * nb + 1 && nb * V <= (int64_t)INT32_MAX && chunk >= 1 && chunk <= MAX_CHUNK &&
           B * nb * cdiv(V, chunk) <= (int64_t)INT32_MAX;
}

}  // namespace

extern "C" int64_t m3ae_beam_topk_workspace_bytes(int64_t B, int64_t nb, int64_t V, int64_t chunk) {
    if (chunk <= 0) chunk = DEF_CHUNK;
    if (!topk_shape_ok(B, nb, V, chunk)) return 0;
    const int64_t blocks = B * nb * cdiv(V, chunk);
    return blocks * (2 * nb) * (int64_t)sizeof(uint64_t) + blocks * 2 * (int64_t)sizeof(float);
}

extern "C" int m3ae_beam_topk(const float* logits, int64_t ld, const float* beam_scores, int64_t B, int64_t nb, int64_t V,
                              int64_t chunk, void* workspace, int64_t workspace_bytes, float* top_s, int32_t* top_i, void* stream) {
    if (!logits || !beam_scores || !top_s || !top_i || B < 1 || ld < V || chunk < 0) return M3AE_ERR_ARG;
    if (chunk == 0) chunk = DEF_CHUNK;
    if (!topk_shape_ok(B, nb, V, chunk)) return M3AE_ERR_UNSUPPORTED;
    const int64_t need = m3ae_beam_topk_workspace_bytes(B, nb, V, chunk);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need) return M3AE_ERR_WORKSPACE;
    const int64_t nch = cdiv(V, chunk), blocks = B * nb * nch;
    const int K = (int)(2 * nb);
    uint64_t* cand = (uint64_t*)workspace;
    float* part = (float*)(cand + blocks * K);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(beam_stats_kernel, dim3((unsigned)blocks), dim3(BT), 0, s, logits, ld, V, chunk, nch, part);
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)blocks), dim3(BT), 0, s, logits, ld, beam_scores, nb, V, chunk, nch, K,
                       (const float*)part, cand);
    hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)B), dim3(BT), 0, s, cand, nb * nch * K, K, top_s, top_i);
    return hip_launch_status();
}

extern "C" int m3ae_beam_step(const float* top_s, const int32_t* top_i, const int64_t* ids_in, int64_t* ids_out, int64_t* last_tok,
                              float* beam_scores, int64_t* order, int32_t* done, int32_t* n_hyp, double* hyp_score, int32_t* hyp_len,
                              int64_t* hyp_tok, int32_t* open_count, int64_t* err, int64_t B, int64_t nb, int64_t V, int64_t max_length,
                              int64_t cur_len, int64_t eos, int64_t pad, double div, void* stream) {
    if (!top_s || !top_i || !ids_in || !ids_out || ids_in == ids_out || !last_tok || !beam_scores || !order || !done || !n_hyp ||
        !hyp_score || !hyp_len || !hyp_tok || !open_count || !err || B < 1 || B > INT32_MAX || max_length < 2 ||
        max_length > INT32_MAX || cur_len < 1 || cur_len >= max_length || !(div > 0.0))
        return M3AE_ERR_ARG;
    if (nb < 1 || nb > MAX_BEAMS || V < 1 || nb * V > (int64_t)INT32_MAX) return M3AE_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)B), dim3(64), 0, s, top_s, top_i, ids_in, ids_out, last_tok, beam_scores, order,
                       done, n_hyp, hyp_score, hyp_len, hyp_tok, err, (int)nb, V, (int)max_length, (int)cur_len, eos, pad, div);
    hipLaunchKernelGGL(beam_open_count_kernel, dim3(1), dim3(BT), 0, s, (const int32_t*)done, B, open_count);
    return hip_launch_status();
}

extern "C" int m3ae_beam_finalize(const int64_t* ids, const float* beam_scores, const int32_t* done, int32_t* n_hyp, double* hyp_score,
                                  int32_t* hyp_len, int64_t* hyp_tok, int64_t* seq, int64_t* len, int64_t B, int64_t nb,
                                  int64_t max_length, int64_t cur_len, int64_t eos, int64_t pad, double div, void* stream) {
    if (!ids || !beam_scores || !done || !n_hyp || !hyp_score || !hyp_len || !hyp_tok || !seq || !len || B < 1 || B > INT32_MAX ||
        max_length < 2 || max_length > INT32_MAX || cur_len < 1 || cur_len > max_length || !(div > 0.0))
        return M3AE_ERR_ARG;
    if (nb < 1 || nb > MAX_BEAMS) return M3AE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(beam_finalize_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, ids, beam_scores, done, n_hyp, hyp_score,
                       hyp_len, hyp_tok, seq, len, (int)nb, (int)max_length, (int)cur_len, eos, pad, div);
    return hip_launch_status();
}
