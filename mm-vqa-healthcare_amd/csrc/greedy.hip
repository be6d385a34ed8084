// Device-resident greedy search for the decoder head (m3ae_amd/modules/m3ae_decoder.py::Decoder.search_path_async): the argmax over
// the vocabulary and the per-step bookkeeping of `search_path`, with no host involvement.
//
// m3ae_greedy_argmax, one launch (+ one small one when the caller asks for tokens):
//   grid (vocabulary chunk, row): a workgroup reduces its chunk of one row to the maximum of the order key of csrc/order_key.h,
//   (monotone image of the fp32 value) << 32 | (2^32 - 1 - column), and writes it to keys[row][chunk].  The rule is eval_key's,
//   which is torch.argmax's: greatest value, lowest column among equals, a NaN above every number and the first NaN first.  The
//   chunk is read by csrc/row_scan.h's walk_row: whatever the row stride, no load touches a column at or past V.
// m3ae_greedy_step, one workgroup: a thread per row folds the row's chunk keys (distinct integers: the fold is order-free), decodes
//   the token and applies one step of the search to the device state; the workgroup counts the rows still open.
// No atomics, no float arithmetic at all: every output bit depends on the inputs and the shapes alone.
#include "common.h"
#include "row_scan.h"

namespace {

constexpr int GT = SCAN_T;               // threads of both kernels
constexpr int64_t G_DEF_CHUNK = 2048;

template <typename T>
__global__ __launch_bounds__(GT) void greedy_argmax_kernel(const T* __restrict__ logits, int64_t ld, int64_t V, int64_t chunk, int64_t nch,
                                                           uint64_t* __restrict__ keys) {
    __shared__ uint64_t red[GT / 64];
    const int64_t r = blockIdx.x / nch, c = blockIdx.x % nch;
    const int64_t v0 = c * chunk;
    const int64_t n = (V - v0) < chunk ? (V - v0) : chunk;
    const int tid = threadIdx.x;
    uint64_t best = 0;
    walk_row(logits + r * ld + v0, n, tid, [&](const uint32_t* u, int cnt, uint32_t j0) {
        for (int e = 0; e < cnt; ++e) best = max_u64(best, eval_key(u[e], (uint32_t)v0 + j0 + e));
    });
    best = block_max_u64(best, red, tid);
    if (tid == 0) keys[blockIdx.x] = best;
}

// The token of a row from its chunk keys; -1 when the decoded column is outside [0, V) (never an address).
DEVINL int64_t fold_token(const uint64_t* __restrict__ k, int64_t nch, int64_t V) {
    uint64_t g = 0;
    for (int64_t i = 0; i < nch; ++i) g = max_u64(g, k[i]);
    return key_index_in(g, V);
}

__global__ __launch_bounds__(GT) void greedy_tokens_kernel(const uint64_t* __restrict__ keys, int64_t nch, int64_t R, int64_t V,
                                                           int64_t* __restrict__ tokens) {
    const int64_t r = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (r < R) tokens[r] = fold_token(keys + r * nch, nch, V);
}

__global__ __launch_bounds__(GT) void greedy_step_kernel(const uint64_t* __restrict__ keys, int64_t nch, int64_t* __restrict__ seq,
                                                         int64_t* __restrict__ len, int64_t* __restrict__ last_tok,
                                                         int32_t* __restrict__ finished, int32_t* __restrict__ open_count,
                                                         int64_t* __restrict__ err, int64_t B, int64_t V, int64_t max_len, int64_t pos,
                                                         int64_t sep, int64_t eos, int64_t pad) {
    __shared__ int red[GT / 64];
    const int tid = threadIdx.x;
    int open = 0;
    for (int64_t r = tid; r < B; r += GT) {
        int64_t tok = fold_token(keys + r * nch, nch, V);
        if (tok < 0) { err[0] = 1; tok = 0; }   // the next step gathers an embedding row by it: keep it a row of the table
        last_tok[r] = tok;                      // fed back whether the row has finished or not, as the host loop does
        int fin = finished[r];
        if (fin) {
            seq[r * max_len + pos] = pad;
        } else {
            seq[r * max_len + pos] = tok;
            if (tok == sep || (eos >= 0 && tok == eos)) {
                fin = 1;
                finished[r] = 1;
                len[r] = pos + 1;
            }
        }
        open += fin ? 0 : 1;
    }
    open = block_sum_int(open, red, tid);
    if (tid == 0) open_count[pos] = open;
}

}  // namespace

extern "C" int64_t m3ae_greedy_workspace_bytes(int64_t R, int64_t V, int64_t chunk) {
    if (chunk == 0) chunk = G_DEF_CHUNK;
    if (!chunk_shape_ok(R, V, chunk, 0)) return 0;
    return R * cdiv(V, chunk) * (int64_t)sizeof(uint64_t);
}

extern "C" int m3ae_greedy_argmax(const void* logits, int64_t ld, int64_t R, int64_t V, int64_t chunk, int dtype, void* workspace,
                                  int64_t workspace_bytes, int64_t* tokens, void* stream) {
    if (!logits || R < 1 || V < 1 || ld < V || chunk < 0) return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (chunk == 0) chunk = G_DEF_CHUNK;
    if (!chunk_shape_ok(R, V, chunk, 0)) return M3AE_ERR_UNSUPPORTED;
    if ((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) return M3AE_ERR_ALIGN;
    const int64_t nch = cdiv(V, chunk);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < R * nch * (int64_t)sizeof(uint64_t)) return M3AE_ERR_WORKSPACE;
    uint64_t* keys = (uint64_t*)workspace;
    hipStream_t s = (hipStream_t)stream;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(greedy_argmax_kernel<T>, dim3((unsigned)(R * nch)), dim3(GT), 0, s, (const T*)logits, ld, V, chunk, nch, keys);
    });
    if (tokens)
        hipLaunchKernelGGL(greedy_tokens_kernel, dim3((unsigned)cdiv(R, GT)), dim3(GT), 0, s, (const uint64_t*)keys, nch, R, V, tokens);
    return hip_launch_status();
}

extern "C" int m3ae_greedy_step(const void* keys, int64_t nch, int64_t* seq, int64_t* len, int64_t* last_tok, int32_t* finished,
                                int32_t* open_count, int64_t* err, int64_t B, int64_t V, int64_t max_len, int64_t pos, int64_t sep,
                                int64_t eos, int64_t pad, void* stream) {
    if (!keys || ((uintptr_t)keys & 7) || !seq || !len || !last_tok || !finished || !open_count || !err || B < 1 || B > (int64_t)INT32_MAX ||
        V < 1 || V > (int64_t)INT32_MAX || max_len < 1 || max_len > (int64_t)INT32_MAX || pos < 0 || pos >= max_len || nch < 1 ||
        nch > (int64_t)INT32_MAX)
        return M3AE_ERR_ARG;
    hipLaunchKernelGGL(greedy_step_kernel, dim3(1), dim3(GT), 0, (hipStream_t)stream, (const uint64_t*)keys, nch, seq, len, last_tok, finished,
                       open_count, err, B, V, max_len, pos, sep, eos, pad);
    return hip_launch_status();
}
