// Device-side VQA evaluation (m3ae_amd/metrics.py, M3AETransformerSS.predict): the prediction of the reference's VQARADScore
// (my_metrics.py:68, torch.max(logits, 1)[1]), the top-k answers with their probabilities, the per-row hits against the soft
// targets and the running record {n, sum_top1, sum_topk} x {all, closed, open}, with no host involvement.
//
// m3ae_vqa_eval, one launch (+ the fold when there are targets and a record):
//   vqa_eval_kernel, one workgroup per row.  The row is read ONCE (csrc/row_scan.h's walk_row: no load touches a column at or past
//   C).  Every value becomes the order key of csrc/order_key.h (eval_key); a thread keeps the kk = max(k, 1) greatest keys of ITS
//   columns in LDS (cand[slot][thread]; 0 = empty, no key is 0; csrc/topk_keep.h, shared with csrc/token_eval.hip).  The row's
//   top-k is a subset of the union of the threads' top-k, so rank j is
//   "the greatest candidate below rank j - 1": k passes over LDS, each a wave maximum and a four-way fold.  Keys of distinct
//   columns are distinct integers: the result does not depend on any order.  The value of a chosen column is decoded from its
//   key (exact but for -0 -> +0 and the NaN payload, neither of which the sigmoid sees).
//   vqa_fold_kernel, one workgroup: thread t adds rows t, t + 256, ... in double, lanes then waves combine in a fixed tree
//   (csrc/row_scan.h's block_add_record), threads 0 .. 8 add the nine sums onto the record, thread 9 counts the call.  The order
//   depends on B alone; no atomics.
// m3ae_seq_match: one thread per row walks gen[r] and ref[r] with the skip ids dropped; then the same fold.
// m3ae_vqa_label_eval: one thread per row reads targets[r][labels[r]] (answer-list decoding, csrc/answer_trie.hip: the prediction
//   is a label already); then the same fold.
#include "common.h"
#include "row_scan.h"
#include "topk_keep.h"
#include <math.h>

namespace {

constexpr int VT = KEEP_T;       // threads of every kernel here (256: the scheme of csrc/topk_keep.h)
static_assert(KEEP_T == SCAN_T, "walk_row and the folds stride by SCAN_T, the candidate scheme by KEEP_T");
constexpr int V_MAX_K = M3AE_VQA_MAX_K;
constexpr int V_MAX_SKIP = M3AE_SEQ_MAX_SKIP;

template <typename T>
__global__ __launch_bounds__(VT) void vqa_eval_kernel(const T* __restrict__ logits, int64_t ld, const float* __restrict__ targets,
                                                      int64_t ldt, int64_t C, int k, int64_t* __restrict__ pred,
                                                      int32_t* __restrict__ topk_idx, float* __restrict__ topk_prob,
                                                      float* __restrict__ hit1_out, float* __restrict__ rows) {
    __shared__ uint64_t cand[V_MAX_K * VT];
    __shared__ uint64_t red[2][VT / 64];
    __shared__ uint64_t sel[V_MAX_K];
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const int kk = k > 0 ? k : 1;
    for (int s = 0; s < kk; ++s) cand[s * VT + tid] = 0;   // a thread reads and writes its own column of cand only
    Keep keep{cand + tid, kk, 0, 0};

    walk_row(logits + r * ld, C, tid, [&](const uint32_t* u, int cnt, uint32_t j0) {
        for (int e = 0; e < cnt; ++e) keep.put(eval_key(u[e], j0 + e));
    });

    keep_select(cand, kk, red, sel, tid);   // rank j = the greatest candidate below rank j - 1 (rank 0: the greatest)

    // a key of 0 (fewer than kk columns: the host refuses k > C) or a column outside [0, C) is never an address
    if (tid < k) {
        const int64_t col = key_index_in(sel[tid], C);
        if (topk_idx) topk_idx[r * k + tid] = (int32_t)col;
        if (topk_prob) topk_prob[r * k + tid] = col >= 0 ? 1.0f / (1.0f + expf(-key_value(sel[tid]))) : 0.0f;
    }
    if (tid == 0) {
        const int64_t top = key_index_in(sel[0], C);
        const bool ok0 = top >= 0;
        if (pred) pred[r] = top;
        if (targets) {
            const float* t = targets + r * ldt;
            const float h1 = ok0 ? t[top] : 0.0f;
            float hk = k > 0 ? h1 : 0.0f;      // k = 0: the maximum over no column
            for (int j = 1; j < k; ++j) {
                const int64_t col = key_index_in(sel[j], C);
                if (col >= 0) {
                    const float v = t[col];
                    hk = v > hk ? v : hk;
                }
            }
            if (hit1_out) hit1_out[r] = h1;
            if (rows) { rows[2 * r] = h1; rows[2 * r + 1] = hk; }
        }
    }
}

// rows fp32 [B][2] = {hit1, hitk}; rec double [10] += {n, sum_top1, sum_topk} of (all, closed, open), rec[9] += 1
__global__ __launch_bounds__(VT) void vqa_fold_kernel(const float* __restrict__ rows, const int32_t* __restrict__ types, int64_t B,
                                                      double* __restrict__ rec) {
    __shared__ double red[VT / 64][9];
    const int tid = threadIdx.x;
    double acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.0;
    for (int64_t r = tid; r < B; r += VT) {
        const double h1 = (double)rows[2 * r], hk = (double)rows[2 * r + 1];
        const int ty = types ? types[r] : -1;
        acc[0] += 1.0; acc[1] += h1; acc[2] += hk;
        if (ty == M3AE_ANS_CLOSED) { acc[3] += 1.0; acc[4] += h1; acc[5] += hk; }
        if (ty == M3AE_ANS_OPEN) { acc[6] += 1.0; acc[7] += h1; acc[8] += hk; }
    }
    block_add_record<9>(acc, red, rec, tid);
}

struct SkipIds { int64_t id[V_MAX_SKIP]; };

__global__ __launch_bounds__(VT) void seq_match_kernel(const int64_t* __restrict__ gen, int64_t ldg, int64_t Lg,
                                                       const int64_t* __restrict__ ref, int64_t ldr, int64_t Lr,
                                                       const int64_t* __restrict__ skip, int ns, int64_t B,
                                                       int32_t* __restrict__ match, float* __restrict__ rows) {
    const int64_t r = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (r >= B) return;
    SkipIds sk;
#pragma unroll
    for (int i = 0; i < V_MAX_SKIP; ++i) sk.id[i] = i < ns ? skip[i] : 0;
    auto skipped = [&](int64_t t) {
        bool s = false;
#pragma unroll
        for (int i = 0; i < V_MAX_SKIP; ++i) s = s || (i < ns && t == sk.id[i]);
        return s;
    };
    const int64_t* g = gen + r * ldg;
    const int64_t* f = ref + r * ldr;
    int64_t i = 0, j = 0;
    bool same = true;
    while (same) {
        while (i < Lg && skipped(g[i])) ++i;
        while (j < Lr && skipped(f[j])) ++j;
        if (i >= Lg || j >= Lr) {
            same = i >= Lg && j >= Lr;     // both subsequences end together
            break;
        }
        same = g[i] == f[j];
        ++i;
        ++j;
    }
    if (match) match[r] = same ? 1 : 0;
    rows[2 * r] = rows[2 * r + 1] = same ? 1.0f : 0.0f;
}

// rows[r] = {t, t} with t = targets[r][labels[r]]; a label outside [0, C) scores 0, sets err and is never an address
__global__ __launch_bounds__(VT) void label_rows_kernel(const int64_t* __restrict__ labels, const float* __restrict__ targets, int64_t ldt,
                                                        int64_t B, int64_t C, float* __restrict__ hit1_out, float* __restrict__ rows,
                                                        int64_t* __restrict__ err) {
    const int64_t r = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (r >= B) return;
    const int64_t l = labels[r];
    const bool ok = l >= 0 && l < C;
    const float t = ok ? targets[r * ldt + l] : 0.0f;
    if (!ok) err[0] = 1;
    if (hit1_out) hit1_out[r] = t;
    rows[2 * r] = rows[2 * r + 1] = t;
}

// the n-best form: rows[r] = {targets[r][labels[r][0]], max over the row's entries l >= 0 of targets[r][l]}.  -1 in columns 1.. is
// an empty slot; any other value outside [0, C), or an empty column 0, scores 0 and sets err (never an address)
__global__ __launch_bounds__(VT) void labels_rows_kernel(const int64_t* __restrict__ labels, int64_t ldl, int k,
                                                         const float* __restrict__ targets, int64_t ldt, int64_t B, int64_t C,
                                                         float* __restrict__ hit1_out, float* __restrict__ rows, int64_t* __restrict__ err) {
    const int64_t r = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (r >= B) return;
    const int64_t* lr = labels + r * ldl;
    const float* t = targets + r * ldt;
    const int64_t l0 = lr[0];
    const bool ok0 = l0 >= 0 && l0 < C;
    if (!ok0) err[0] = 1;
    const float h1 = ok0 ? t[l0] : 0.0f;
    float hk = h1;
    for (int j = 1; j < k; ++j) {
        const int64_t l = lr[j];
        if (l == -1) continue;
        if (l < 0 || l >= C) { err[0] = 1; continue; }
        const float v = t[l];
        hk = v > hk ? v : hk;
    }
    if (hit1_out) hit1_out[r] = h1;
    rows[2 * r] = h1;
    rows[2 * r + 1] = hk;
}

inline int64_t rows_bytes(int64_t B) { return B * 2 * (int64_t)sizeof(float); }

}  // namespace

extern "C" int64_t m3ae_vqa_eval_workspace_bytes(int64_t B, int64_t k) {
    if (B < 1 || B > (int64_t)INT32_MAX || k < 0 || k > V_MAX_K) return 0;
    return rows_bytes(B);
}

extern "C" int m3ae_vqa_eval(const void* logits, int64_t ld, const float* targets, int64_t ldt, const int32_t* types, int64_t B,
                             int64_t C, int64_t k, int dtype, int64_t* pred, int32_t* topk_idx, float* topk_prob, float* hit1,
                             double* rec, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!logits || B < 1 || C < 1 || k < 0) return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (k > V_MAX_K || k > C || C > (int64_t)INT32_MAX || B > (int64_t)INT32_MAX || ld < C || (targets && ldt < C)) return M3AE_ERR_UNSUPPORTED;
    const bool fold = targets && rec;
    if (fold && (!workspace || workspace_bytes < rows_bytes(B))) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) || ((uintptr_t)targets & 3) || ((uintptr_t)types & 3) || ((uintptr_t)pred & 7) ||
        ((uintptr_t)topk_idx & 3) || ((uintptr_t)topk_prob & 3) || ((uintptr_t)hit1 & 3) || ((uintptr_t)rec & 7) ||
        (fold && ((uintptr_t)workspace & 7)))
        return M3AE_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    float* rows = fold ? (float*)workspace : nullptr;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(vqa_eval_kernel<T>, dim3((unsigned)B), dim3(VT), 0, s, (const T*)logits, ld, targets, ldt, C, (int)k, pred, topk_idx,
                           topk_prob, hit1, rows);
    });
    if (fold) hipLaunchKernelGGL(vqa_fold_kernel, dim3(1), dim3(VT), 0, s, (const float*)rows, types, B, rec);
    return hip_launch_status();
}

extern "C" int m3ae_seq_match(const int64_t* gen, int64_t ldg, int64_t Lg, const int64_t* ref, int64_t ldr, int64_t Lr,
                              const int64_t* skip, int64_t ns, const int32_t* types, int64_t B, int32_t* match, double* rec,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    if (!gen || !ref || !rec || B < 1 || Lg < 0 || Lr < 0 || ns < 0 || (ns > 0 && !skip)) return M3AE_ERR_ARG;
    if (ns > V_MAX_SKIP || B > (int64_t)INT32_MAX || ldg < Lg || ldr < Lr) return M3AE_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < rows_bytes(B)) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)gen & 7) || ((uintptr_t)ref & 7) || ((uintptr_t)skip & 7) || ((uintptr_t)types & 3) || ((uintptr_t)match & 3) ||
        ((uintptr_t)rec & 7) || ((uintptr_t)workspace & 7))
        return M3AE_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(seq_match_kernel, dim3((unsigned)cdiv(B, VT)), dim3(VT), 0, s, gen, ldg, Lg, ref, ldr, Lr, skip, (int)ns, B, match,
                       (float*)workspace);
    hipLaunchKernelGGL(vqa_fold_kernel, dim3(1), dim3(VT), 0, s, (const float*)workspace, types, B, rec);
    return hip_launch_status();
}

extern "C" int m3ae_vqa_label_eval(const int64_t* labels, const float* targets, int64_t ldt, const int32_t* types, int64_t B, int64_t C,
                                   float* hit1, double* rec, int64_t* err, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!labels || !targets || !rec || !err || B < 1 || C < 1) return M3AE_ERR_ARG;
    if (C > (int64_t)INT32_MAX || B > (int64_t)INT32_MAX || ldt < C) return M3AE_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < rows_bytes(B)) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)labels & 7) || ((uintptr_t)targets & 3) || ((uintptr_t)types & 3) || ((uintptr_t)hit1 & 3) || ((uintptr_t)rec & 7) ||
        ((uintptr_t)err & 7) || ((uintptr_t)workspace & 7))
        return M3AE_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(label_rows_kernel, dim3((unsigned)cdiv(B, VT)), dim3(VT), 0, s, labels, targets, ldt, B, C, hit1, (float*)workspace, err);
    hipLaunchKernelGGL(vqa_fold_kernel, dim3(1), dim3(VT), 0, s, (const float*)workspace, types, B, rec);
    return hip_launch_status();
}

extern "C" int m3ae_vqa_labels_eval(const int64_t* labels, int64_t ldl, int64_t k, const float* targets, int64_t ldt, const int32_t* types,
                                    int64_t B, int64_t C, float* hit1, double* rec, int64_t* err, void* workspace, int64_t workspace_bytes,
                                    void* stream) {
    if (!labels || !targets || !rec || !err || B < 1 || C < 1 || k < 1) return M3AE_ERR_ARG;
    if (k > V_MAX_K || C > (int64_t)INT32_MAX || B > (int64_t)INT32_MAX || ldt < C || ldl < k) return M3AE_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < rows_bytes(B)) return M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)labels & 7) || ((uintptr_t)targets & 3) || ((uintptr_t)types & 3) || ((uintptr_t)hit1 & 3) || ((uintptr_t)rec & 7) ||
        ((uintptr_t)err & 7) || ((uintptr_t)workspace & 7))
        return M3AE_ERR_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(labels_rows_kernel, dim3((unsigned)cdiv(B, VT)), dim3(VT), 0, s, labels, ldl, (int)k, targets, ldt, B, C, hit1,
                       (float*)workspace, err);
    hipLaunchKernelGGL(vqa_fold_kernel, dim3(1), dim3(VT), 0, s, (const float*)workspace, types, B, rec);
    return hip_launch_status();
}
