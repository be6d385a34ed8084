// Device-resident greedy search for the decoder head (m3ae_amd/modules/m3ae_decoder.py::Decoder.search_path_async): the argmax over
// the vocabulary and the per-step bookkeeping of `search_path`, with no host involvement.
//
// m3ae_greedy_argmax, one launch (+ one small one when the caller asks for tokens):
//   grid (vocabulary chunk, row): a workgroup reduces its chunk of one row to the maximum of the order key of csrc/order_key.h,
//   (monotone image of the fp32 value) << 32 | (2^32 - 1 - column), and writes it to keys[row][chunk].  The rule is torch.argmax's:
//   greatest value, lowest column among equals (-0 is folded onto +0 first), and every NaN of either sign takes the top image
//   2^32 - 1, so a NaN beats every number and the first NaN wins.  bf16 widens to fp32 exactly (16 zero bits), so the compare is the
//   same compare.  A chunk is read as a scalar head up to the first 16-byte boundary of its row, 16-byte loads, and a scalar tail:
//   whatever the row stride, no load touches a column at or past V.
// m3ae_greedy_step, one workgroup: a thread per row folds the row's chunk keys (distinct integers: the fold is order-free), decodes
//   the token and applies one step of the search to the device state; the workgroup counts the rows still open.
// No atomics, no float arithmetic at all: every output bit depends on the inputs and the shapes alone.
#include "common.h"
#include "order_key.h"

namespace {

constexpr int GT = 256;                  // threads of both kernels
constexpr int64_t G_DEF_CHUNK = 2048;
constexpr int64_t G_MIN_CHUNK = 64, G_MAX_CHUNK = 65536;

// u = the bits of an fp32 value
DEVINL uint64_t greedy_key(uint32_t u, uint32_t col) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return ((uint64_t)0xffffffffu << 32) | (uint64_t)(0xffffffffu - col);   // NaN: above +inf
    return make_key(__uint_as_float(u == 0x80000000u ? 0u : u), col);                                           // -0 -> +0
}
DEVINL uint32_t f32_bits(float v) { return __float_as_uint(v); }
DEVINL uint32_t f32_bits(bf16_t v) { return (uint32_t)v << 16; }
DEVINL uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }

template <typename T>
__global__ __launch_bounds__(GT) void greedy_argmax_kernel(const T* __restrict__ logits, int64_t ld, int64_t V, int64_t chunk, int64_t nch,
                                                           uint64_t* __restrict__ keys) {
    constexpr int W = 16 / (int)sizeof(T);   // elements of one 16-byte load
    __shared__ uint64_t red[GT / 64];
    const int64_t r = blockIdx.x / nch, c = blockIdx.x % nch;
    const int64_t v0 = c * chunk;
    const int64_t n = (V - v0) < chunk ? (V - v0) : chunk;
    const T* x = logits + r * ld + v0;
    const int tid = threadIdx.x;
    // x is element-aligned (host check): `mis` elements past a 16-byte boundary
    const int64_t mis = (int64_t)(((uintptr_t)x & 15) / sizeof(T));
    int64_t head = mis ? W - mis : 0;
    head = head < n ? head : n;
    const int64_t nvec = (n - head) / W;
    const int64_t tail0 = head + nvec * W;
    uint64_t best = 0;
    if (tid < head) best = greedy_key(f32_bits(x[tid]), (uint32_t)(v0 + tid));
    const u32x4* xv = (const u32x4*)(x + head);
    for (int64_t i = tid; i < nvec; i += GT) {
        const u32x4 q = xv[i];
        const uint32_t j0 = (uint32_t)(v0 + head + i * W);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (sizeof(T) == 4) {
                best = max_u64(best, greedy_key(q[e], j0 + e));
            } else {   // two bf16 per dword, the lower column in the low half
                best = max_u64(best, greedy_key(q[e] << 16, j0 + 2 * e));
                best = max_u64(best, greedy_key(q[e] & 0xffff0000u, j0 + 2 * e + 1));
            }
        }
    }
    if (tail0 + tid < n) best = max_u64(best, greedy_key(f32_bits(x[tail0 + tid]), (uint32_t)(v0 + tail0 + tid)));   // < W <= GT columns
    best = wave_max_u64(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) keys[blockIdx.x] = max_u64(max_u64(red[0], red[1]), max_u64(red[2], red[3]));
}

// The token of a row from its chunk keys; -1 when the decoded column is outside [0, V) (never an address).
DEVINL int64_t fold_token(const uint64_t* __restrict__ k, int64_t nch, int64_t V) {
    uint64_t g = 0;
    for (int64_t i = 0; i < nch; ++i) g = max_u64(g, k[i]);
    const int64_t tok = (int64_t)(0xffffffffu - (uint32_t)g);
    return (g == 0 || tok >= V) ? -1 : tok;
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
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) open += __shfl_xor(open, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = open;
    __syncthreads();
    if (tid == 0) open_count[pos] = red[0] + red[1] + red[2] + red[3];
}

inline bool argmax_shape_ok(int64_t R, int64_t V, int64_t chunk) {
    return R >= 1 && V >= 1 && V <= (int64_t)INT32_MAX && chunk >= G_MIN_CHUNK && chunk <= G_MAX_CHUNK && R <= (int64_t)INT32_MAX &&
           R * cdiv(V, chunk) <= (int64_t)INT32_MAX;
}

}  // namespace

extern "C" int64_t m3ae_greedy_workspace_bytes(int64_t R, int64_t V, int64_t chunk) {
    if (chunk == 0) chunk = G_DEF_CHUNK;
    if (!argmax_shape_ok(R, V, chunk)) return 0;
    return R * cdiv(V, chunk) * (int64_t)sizeof(uint64_t);
}

extern "C" int m3ae_greedy_argmax(const void* logits, int64_t ld, int64_t R, int64_t V, int64_t chunk, int dtype, void* workspace,
                                  int64_t workspace_bytes, int64_t* tokens, void* stream) {
    if (!logits || R < 1 || V < 1 || ld < V || chunk < 0) return M3AE_ERR_ARG;
    if (dtype != M3AE_F32 && dtype != M3AE_BF16) return M3AE_ERR_UNSUPPORTED;
    if (chunk == 0) chunk = G_DEF_CHUNK;
    if (!argmax_shape_ok(R, V, chunk)) return M3AE_ERR_UNSUPPORTED;
    if ((uintptr_t)logits & (dtype == M3AE_F32 ? 3 : 1)) return M3AE_ERR_ALIGN;
    const int64_t nch = cdiv(V, chunk);
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < R * nch * (int64_t)sizeof(uint64_t)) return M3AE_ERR_WORKSPACE;
    uint64_t* keys = (uint64_t*)workspace;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == M3AE_F32)
        hipLaunchKernelGGL(greedy_argmax_kernel<float>, dim3((unsigned)(R * nch)), dim3(GT), 0, s, (const float*)logits, ld, V, chunk, nch, keys);
    else
        hipLaunchKernelGGL(greedy_argmax_kernel<bf16_t>, dim3((unsigned)(R * nch)), dim3(GT), 0, s, (const bf16_t*)logits, ld, V, chunk, nch,
                           keys);
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
