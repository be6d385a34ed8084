// Device-side token evaluation for rows of vocabulary width (m3ae_amd/metrics.py: TokenAccuracy, M3AETransformerSS.fill_mask): the
// argmax, the rank of the label, the negative log-likelihood and the top-k tokens with their softmax probabilities of the rows
// that carry a label (or are selected), and the running record {n, hit1, hitk, sum_nll, calls}, with no host involvement.
//
// m3ae_token_eval, three launches (the third only with a record):
//   token_chunk_kernel, grid (chunk, row): a workgroup of a row that is not evaluated returns before it reads a logit.  Otherwise
//   it reads its chunk ONCE (walk_row's geometry of csrc/row_scan.h, in a copy of its own: no load touches a column at or past V;
//   see the note at Acc) and leaves four things in workspace slots of its own: the greatest order key (csrc/order_key.h's
//   eval_key: torch.argmax's rule), the number of keys strictly greater than the label's key, the chunk's
//   (m, s) = (maximum, sum exp(x - m)) in fp32, and, for k > 0, its k greatest keys (csrc/topk_keep.h).
//   token_row_kernel, one workgroup per row: the maximum of the chunk keys, the sum of the counts, the merge of the (m, s) pairs
//   (the folds of csrc/row_scan.h, in their every-thread form), lse = m + logf(s), the top-k of the chunks' candidates; writes
//   pred / rank / nll / topk_idx / topk_prob.
//   token_fold_kernel, one workgroup: thread t adds rows t, t + 256, ... in double, lanes then waves combine in a fixed tree
//   (csrc/row_scan.h's block_add_record), thread 0 .. 3 add the four sums onto the record, thread 4 counts the call.  The order
//   depends on R alone; no atomics.
// (m, s) arithmetic.  A term is e(x, m) = x == m ? 1 : expf(x - m), which is expf(x - m) for finite values and keeps inf - inf out
// of the sum: a row of -inf alone has lse = -inf + logf(count) = -inf, a row with a +inf has lse = +inf, a NaN anywhere gives a NaN
// (fmaxf skips it, expf does not) -- the values torch.logsumexp returns.  Two pairs merge as m' = fmaxf(m1, m2),
// s' = s1 e(m1, m') + s2 e(m2, m'); every s is a sum of terms in [0, 1], so there is no inf * 0.
// m3ae_record_add: rec[0] += value[0], rec[1] += 1 in double (metrics.LossMean).
#include "common.h"
#include "row_scan.h"
#include "topk_keep.h"
#include <math.h>

namespace {

constexpr int TT = KEEP_T;       // threads of every kernel here
static_assert(KEEP_T == SCAN_T, "walk_row and the folds stride by SCAN_T, the candidate scheme by KEEP_T");
constexpr int64_t T_DEF_CHUNK = 8192;                       // measured: tools/token_eval_bench.py --chunks
constexpr int T_MAX_K = M3AE_TOKEN_MAX_K;
constexpr int64_t T_IGNORE = M3AE_TOKEN_IGNORE;
enum { ROW_SKIPPED = 0, ROW_UNLABELLED = 1, ROW_LABELLED = 2 };
constexpr int32_t RANK_SKIPPED = -2, RANK_NONE = -1;        // the per-row word the fold reads: a rank >= 0 otherwise

// What happens to row r.  bad: the label is neither T_IGNORE nor a column (the row is skipped and err is set).
DEVINL int row_state(const int64_t* __restrict__ labels, const uint8_t* __restrict__ select, int64_t r, int64_t V, int64_t& label,
                     bool& bad) {
    label = labels ? labels[r] : T_IGNORE;
    const bool ev = select ? select[r] != 0 : (labels ? label != T_IGNORE : true);
    bad = ev && label != T_IGNORE && (label < 0 || label >= V);
    if (!ev || bad) return ROW_SKIPPED;
    return label == T_IGNORE ? ROW_UNLABELLED : ROW_LABELLED;
}

// token_chunk_kernel keeps its own body -- its accumulator with the (m, s) part inline, its own copy of the row geometry of
// csrc/row_scan.h's walk_row and its own fold: on the shared pieces it measured 1 - 1.5 % slower (k = 5) on the MI355X
// (profiles/r26_row_scan.log), and a kernel that cannot be held level stays as it was.  A change to walk_row must be made here too.
// What a thread has gathered from its columns of the chunk.
template <bool TOPK>
struct Acc {
    uint64_t best, lkey;
    int cnt;
    float m, s;
    Keep keep;
    // n <= 8 values (fp32 bits) of columns j0, j0 + 1, ...
    DEVINL void take(const uint32_t* u, int n, uint32_t j0) {
        float vm = __uint_as_float(u[0]);
        for (int e = 1; e < n; ++e) vm = fmaxf(vm, __uint_as_float(u[e]));
        const float mn = fmaxf(m, vm);       // a NaN is skipped here and caught by expf below
        if (mn != m) { s *= exp_diff(m, mn); m = mn; }
        for (int e = 0; e < n; ++e) {
            s += exp_diff(__uint_as_float(u[e]), m);
            const uint64_t key = eval_key(u[e], j0 + e);
            best = max_u64(best, key);
            cnt += key > lkey ? 1 : 0;
            if (TOPK) keep.put(key);
        }
    }
};

template <typename T, bool TOPK>
__global__ __launch_bounds__(TT) void token_chunk_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                         const uint8_t* __restrict__ select, int64_t V, int64_t chunk, int64_t nch, int k,
                                                         uint64_t* __restrict__ keys, int32_t* __restrict__ cnts, float* __restrict__ ms,
                                                         uint64_t* __restrict__ tops) {
    constexpr int W = 16 / (int)sizeof(T);   // elements of one 16-byte load
    __shared__ uint64_t cand[TOPK ? T_MAX_K * TT : 1];
    __shared__ uint64_t red[2][TT / 64];
    __shared__ uint64_t sel[T_MAX_K];
    __shared__ uint64_t redk[TT / 64];
    __shared__ int redc[TT / 64];
    __shared__ float redm[TT / 64], reds[TT / 64];
    const int64_t r = blockIdx.x / nch, c = blockIdx.x % nch;
    int64_t label;
    bool bad;
    const int st = row_state(labels, select, r, V, label, bad);
    if (st == ROW_SKIPPED) return;            // the whole workgroup: nothing of the row is read
    const int tid = threadIdx.x;
    const int64_t v0 = c * chunk;
    const int64_t n = (V - v0) < chunk ? (V - v0) : chunk;
    const T* row = logits + r * ld;
    const T* x = row + v0;
    if (TOPK)
        for (int s = 0; s < k; ++s) cand[s * TT + tid] = 0;   // a thread reads and writes its own column of cand only
    Acc<TOPK> acc;
    acc.best = 0;
    // without a label nothing is greater than the key: the count stays 0.  0 <= label < V here: the one address a label makes.
    acc.lkey = st == ROW_LABELLED ? eval_key(bits_of(row[label]), (uint32_t)label) : ~(uint64_t)0;
    acc.cnt = 0;
    acc.m = -INFINITY;
    acc.s = 0.0f;
    acc.keep = Keep{cand + tid, k, 0, 0};

    // x is element-aligned (host check): `mis` elements past a 16-byte boundary
    const int64_t mis = (int64_t)(((uintptr_t)x & 15) / sizeof(T));
    int64_t head = mis ? W - mis : 0;
    head = head < n ? head : n;
    const int64_t nvec = (n - head) / W;
    const int64_t tail0 = head + nvec * W;
    if (tid < head) {
        const uint32_t u = bits_of(x[tid]);
        acc.take(&u, 1, (uint32_t)(v0 + tid));
    }
    const u32x4* xv = (const u32x4*)(x + head);
    for (int64_t i = tid; i < nvec; i += TT) {
        const u32x4 q = xv[i];
        const uint32_t j0 = (uint32_t)(v0 + head + i * W);
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
        acc.take(u, W, j0);
    }
    if (tail0 + tid < n) {   // < W <= TT columns
        const uint32_t u = bits_of(x[tail0 + tid]);
        acc.take(&u, 1, (uint32_t)(v0 + tail0 + tid));
    }

    uint64_t best = wave_max_u64(acc.best);
    int cnt = acc.cnt;
    float m = acc.m, s = acc.s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        ms_merge(m, s, m2, s2);
    }
    if ((tid & 63) == 0) {
        redk[tid >> 6] = best;
        redc[tid >> 6] = cnt;
        redm[tid >> 6] = m;
        reds[tid >> 6] = s;
    }
    __syncthreads();
    if (tid == 0) {   // lane 0 of wave 0 folds the four waves in order
        for (int w = 1; w < TT / 64; ++w) {
            best = max_u64(best, redk[w]);
            cnt += redc[w];
            ms_merge(m, s, redm[w], reds[w]);
        }
        keys[blockIdx.x] = best;
        cnts[blockIdx.x] = cnt;
        ms[2 * (int64_t)blockIdx.x] = m;
        ms[2 * (int64_t)blockIdx.x + 1] = s;
    }
    if (TOPK) {
        keep_select(cand, k, red, sel, tid);
        if (tid < k) tops[(int64_t)blockIdx.x * k + tid] = sel[tid];   // 0 where the chunk has fewer than k columns
    }
}

template <typename T>
__global__ __launch_bounds__(TT) void token_row_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                       const uint8_t* __restrict__ select, int64_t V, int64_t nch, int k,
                                                       const uint64_t* __restrict__ keys, const int32_t* __restrict__ cnts,
                                                       const float* __restrict__ ms, const uint64_t* __restrict__ tops,
                                                       int64_t* __restrict__ pred, int32_t* __restrict__ rank, float* __restrict__ nll,
                                                       int32_t* __restrict__ topk_idx, float* __restrict__ topk_prob,
                                                       int64_t* __restrict__ err, int32_t* __restrict__ row_rank,
                                                       float* __restrict__ row_nll) {
    __shared__ uint64_t cand[T_MAX_K * TT];
    __shared__ uint64_t red[2][TT / 64];
    __shared__ uint64_t sel[T_MAX_K];
    __shared__ uint64_t redk[TT / 64];
    __shared__ int redc[TT / 64];
    __shared__ float redm[TT / 64], reds[TT / 64];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    int64_t label;
    bool bad;
    const int st = row_state(labels, select, r, V, label, bad);
    if (st == ROW_SKIPPED) {
        if (tid < k) {
            if (topk_idx) topk_idx[r * k + tid] = -1;
            if (topk_prob) topk_prob[r * k + tid] = 0.0f;
        }
        if (tid == 0) {
            if (bad && err) err[0] = 1;
            if (pred) pred[r] = -1;
            if (rank) rank[r] = RANK_NONE;
            if (nll) nll[r] = 0.0f;
            row_rank[r] = RANK_SKIPPED;
            row_nll[r] = 0.0f;
        }
        return;
    }
    const int64_t s0 = r * nch;
    uint64_t best = 0;
    int cnt = 0;
    float m = -INFINITY, s = 0.0f;
    for (int64_t i = tid; i < nch; i += TT) {
        best = max_u64(best, keys[s0 + i]);
        cnt += cnts[s0 + i];
        ms_merge(m, s, ms[2 * (s0 + i)], ms[2 * (s0 + i) + 1]);
    }
    // every thread folds the four waves in the same order: the same bits in every thread
    max_put(best, redk, tid);
    sum_put(cnt, redc, tid);
    ms_put(m, s, redm, reds, tid);
    __syncthreads();
    best = max_get<true>(redk, tid);
    cnt = sum_get<true>(redc, tid);
    ms_get<true>(m, s, redm, reds, tid);
    const float lse = m + logf(s);

    if (k > 0) {
        for (int j = 0; j < k; ++j) cand[j * TT + tid] = 0;
        Keep keep{cand + tid, k, 0, 0};
        const int64_t nc = nch * k;
        for (int64_t i = tid; i < nc; i += TT) keep.put(tops[s0 * k + i]);    // an empty slot is 0 and is never kept
        keep_select(cand, k, red, sel, tid);
        if (tid < k) {   // a key of 0 (the host refuses k > V) or a column outside [0, V) is never an address
            const int64_t col = key_index_in(sel[tid], V);
            if (topk_idx) topk_idx[r * k + tid] = (int32_t)col;
            if (topk_prob) topk_prob[r * k + tid] = col >= 0 ? expf(key_value(sel[tid]) - lse) : 0.0f;
        }
    }
    if (tid == 0) {
        if (pred) pred[r] = key_index_in(best, V);
        const bool lab = st == ROW_LABELLED;
        const float xl = lab ? Elem<T>::ld(logits + r * ld + label) : 0.0f;   // 0 <= label < V
        const float v = lab ? lse - xl : lse;
        if (rank) rank[r] = lab ? cnt : RANK_NONE;
        if (nll) nll[r] = v;
        row_rank[r] = lab ? cnt : RANK_NONE;
        row_nll[r] = v;
    }
}

// row_rank int32 [R] (>= 0: the rank of a labelled row), row_nll fp32 [R]; rec double [5] += {n, hit1, hitk, sum_nll}, rec[4] += 1
__global__ __launch_bounds__(TT) void token_fold_kernel(const int32_t* __restrict__ row_rank, const float* __restrict__ row_nll, int64_t R,
                                                        int k, double* __restrict__ rec) {
    __shared__ double red[TT / 64][4];
    const int tid = threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = tid; r < R; r += TT) {
        const int32_t rk = row_rank[r];
        if (rk >= 0) {
            acc[0] += 1.0;
            acc[1] += rk == 0 ? 1.0 : 0.0;
            acc[2] += rk < k ? 1.0 : 0.0;
            acc[3] += (double)row_nll[r];
        }
    }
    block_add_record<4>(acc, red, rec, tid);
}

__global__ void record_add_kernel(const float* __restrict__ value, double* __restrict__ rec) {
    if (threadIdx.x == 0) {
        rec[0] += (double)value[0];
        rec[1] += 1.0;
    }
}

inline int64_t pad8(int64_t b) { return (b + 7) & ~(int64_t)7; }

inline bool token_shape_ok(int64_t R, int64_t V, int64_t chunk, int64_t k) {
    return chunk_shape_ok(R, V, chunk, 0) && k >= 0 && k <= T_MAX_K && k <= V;
}

// workspace: keys u64 [S] | tops u64 [S][k] | ms fp32 [S][2] | cnts i32 [S] | row_rank i32 [R] | row_nll fp32 [R], S = R * chunks
struct TokenWs {
    int64_t keys, tops, ms, cnts, row_rank, row_nll, bytes;
};
inline TokenWs token_ws(int64_t R, int64_t nch, int64_t k) {
    const int64_t S = R * nch;
    TokenWs w;
    w.keys = 0;
    w.tops = w.keys + S * 8;
    w.ms = w.tops + S * k * 8;
    w.cnts = w.ms + S * 8;
    w.row_rank = w.cnts + pad8(S * 4);
    w.row_nll = w.row_rank + pad8(R * 4);
    w.bytes = w.row_nll + pad8(R * 4);
    return w;
}

template <typename T>
void launch_token(const void* logits, int64_t ld, const int64_t* labels, const uint8_t* select, int64_t R, int64_t V, int64_t chunk,
                  int64_t nch, int k, int64_t* pred, int32_t* rank, float* nll, int32_t* topk_idx, float* topk_prob, int64_t* err,
                  char* ws, const TokenWs& w, hipStream_t s) {
    uint64_t* keys = (uint64_t*)(ws + w.keys);
    uint64_t* tops = (uint64_t*)(ws + w.tops);
    float* ms = (float*)(ws + w.ms);
    int32_t* cnts = (int32_t*)(ws + w.cnts);
    if (k > 0)
        hipLaunchKernelGGL((token_chunk_kernel<T, true>), dim3((unsigned)(R * nch)), dim3(TT), 0, s, (const T*)logits, ld, labels, select, V,
                           chunk, nch, k, keys, cnts, ms, tops);
    else
        hipLaunchKernelGGL((token_chunk_kernel<T, false>), dim3((unsigned)(R * nch)), dim3(TT), 0, s, (const T*)logits, ld, labels, select, V,
                           chunk, nch, k, keys, cnts, ms, tops);
    hipLaunchKernelGGL(token_row_kernel<T>, dim3((unsigned)R), dim3(TT), 0, s, (const T*)logits, ld, labels, select, V, nch, k,
                       (const uint64_t*)keys, (const int32_t*)cnts, (const float*)ms, (const uint64_t*)tops, pred, rank, nll, topk_idx,
                       topk_prob, err, (int32_t*)(ws + w.row_rank), (float*)(ws + w.row_nll));
}

}  // namespace

extern "C" int64_t m3ae_token_eval_workspace_bytes(int64_t R, int64_t V, int64_t chunk, int64_t k) {
    if (chunk == 0) chunk = T_DEF_CHUNK;
    if (!token_shape_ok(R, V, chunk, k)) return 0;
    return token_ws(R, cdiv(V, chunk), k).bytes;
}

extern "C" int m3ae_token_eval(const void* logits, int64_t ld, const int64_t* labels, const uint8_t* select, int64_t R, int64_t V,
                               int64_t chunk, int64_t k, int dtype, int64_t* pred, int32_t* rank, float* nll, int32_t* topk_idx,
                               float* topk_prob, double* rec, int64_t* err, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!logits || R < 1 || V < 1 || ld < V || chunk < 0 || k < 0 || (labels && !err) || !workspace) return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (chunk == 0) chunk = T_DEF_CHUNK;
    if (!token_shape_ok(R, V, chunk, k)) return M3AE_ERR_UNSUPPORTED;
    const int64_t nch = cdiv(V, chunk);
    const TokenWs w = token_ws(R, nch, k);
    if (workspace_bytes < w.bytes) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) || ((uintptr_t)labels & 7) || ((uintptr_t)pred & 7) || ((uintptr_t)rank & 3) ||
        ((uintptr_t)nll & 3) || ((uintptr_t)topk_idx & 3) || ((uintptr_t)topk_prob & 3) || ((uintptr_t)rec & 7) || ((uintptr_t)err & 7) ||
        ((uintptr_t)workspace & 7))
        return M3AE_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    by_dtype(dtype, [&](auto t) {
        launch_token<decltype(t)>(logits, ld, labels, select, R, V, chunk, nch, (int)k, pred, rank, nll, topk_idx, topk_prob, err,
                                  (char*)workspace, w, s);
    });
    if (rec)
        hipLaunchKernelGGL(token_fold_kernel, dim3(1), dim3(TT), 0, s, (const int32_t*)((char*)workspace + w.row_rank),
                           (const float*)((char*)workspace + w.row_nll), R, (int)k, rec);
    return hip_launch_status();
}

extern "C" int m3ae_record_add(const float* value, double* rec, void* stream) {
    if (!value || !rec) return M3AE_ERR_ARG;
    if (((uintptr_t)value & 3) || ((uintptr_t)rec & 7)) return M3AE_ERR_ALIGN;
    hipLaunchKernelGGL(record_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, value, rec);
    return hip_launch_status();
}
