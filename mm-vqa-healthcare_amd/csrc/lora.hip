// LoRA on the flat buffers, merged form: the effective weight W = W0 + s B A lives in the ordinary master / shadow buffers, so no
// GEMM changes; the adapter gradients come from the full weight gradient the step already computes (y = x W^T, so by the chain
// rule dA = s B^T dW and dB = s dW A^T).  Two grouped launches per optimizer step over a device table of targets
//     {elem_offset, N, K, a_off, b_off, base_off}        (int64 x 6, include/m3ae_hip.h)
// with one rank r in 1..64 for the whole table.  Fp32 FMA streaming kernels, no MFMA, no atomics: every output is a function of
// the inputs alone, so deterministic mode takes the same kernels.
//
// Work distribution.  The table is on the device, so the host does not know the tile count: both launches use a fixed grid of
// LORA_GRID workgroups -- more than a full-size model has row panels, so the hardware dispatcher balances panels of different
// length; each workgroup builds the running tile count per target in LDS (ntargets <= LORA_MAX_TARGETS), walks tiles blockIdx.x,
// blockIdx.x + gridDim.x, ... and finds a tile's target by bisection (made wave-uniform with readfirstlane, so the record is read
// with scalar loads).
//
// m3ae_lora_merge, tile = MG_ROWS x MG_COLS = 64 x 128 of one W.  Lane t owns 4 adjacent columns (one 16-byte load of W0, one
// 16-byte store of W, one 8-byte store of the shadow) of rows t / 32 + 8 i, i = 0..7; the 8 loads of W0 are issued before the
// arithmetic.  Per output, in this order:
//     acc = 0;  for j = 0 .. r-1:  acc = fmaf(B[n][j], A[j][k], acc);     W = fmaf(s, acc, W0)
// and the shadow is the RNE bf16 of that W.  (B = 0: acc = +0 and W = W0 bit for bit, but a W0 of -0 comes out +0.)
// LDS layout, chosen for the reads of the inner loop and sized by the rank class RP (r rounded up to 4, 8, 16, 32, 64: a small rank
// does not pay the occupancy of the largest): sA[j][128] -- lanes read their 4 columns as one ds_read_b128, lane-contiguous
// (conflict-free; both half-waves read the same addresses); sB[row][RP] -- every lane of a half-wave reads the same word
// (broadcast).  mode 1 stages nothing, reads no A / B and never multiplies by s: W = W0.
//
// m3ae_lora_grad, panel = GR_ROWS = 64 rows x all K columns of one dW, walked in chunks of GR_COLS = 64 columns; dW is read once.
// Wave w of the workgroup owns the JQ ranks j = w JQ + jj (RP = 4 JQ >= r).  The chunk goes to LDS as sW[64][65] (odd stride: the
// dB phase reads one column of 64 rows per wave, the dA phase one row piece of 64 columns; both conflict-free).  A and B are NOT in
// LDS: lane n holds B[n][j] of the panel's row n, lane k holds A[j][k] of the chunk's column k, and the loops fetch the value of
// the wave-uniform row / column with v_readlane -- the first form kept both in LDS, where the broadcast reads made the kernel
// LDS-issue bound (3 LDS reads per 2 FMAs at r = 8).
//   * dA phase, lane owns column k:
//         acc = 0;  for n ascending over the panel's rows:  acc = fmaf(B[n][j], dW[n][k], acc)      -> plane[panel][j][k]
//   * dB phase, lane owns row n; one chain over the WHOLE row:
//         acc = 0;  for k = 0 .. K-1:  acc = fmaf(dW[n][k], A[j][k], acc);                          dB[n][j] = s * acc
//   * lora_fold_kernel: dA[j][k] = s * (((plane[0] + plane[1]) + plane[2]) + ...), ascending panel order, fp32 adds.
// Outputs are overwritten.
#include "common.h"
#include <math.h>

namespace {

constexpr int LORA_BLOCK = 256;
constexpr int LORA_GRID = 8192;
constexpr int LORA_MAX_TARGETS = M3AE_LORA_MAX_TARGETS;
constexpr int LORA_MAX_RANK = M3AE_LORA_MAX_RANK;
constexpr int MG_ROWS = 64, MG_COLS = 128;
constexpr int GR_ROWS = M3AE_LORA_PANEL_ROWS, GR_COLS = 64, GR_LD = GR_COLS + 1;
constexpr int FOLD_CHUNK = LORA_BLOCK;

struct Target { int64_t off, N, K, a_off, b_off, base_off; };

DEVINL int64_t cdiv_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }

DEVINL Target load_target(const int64_t* __restrict__ table, int t) {
    const int64_t* p = table + 6 * (int64_t)t;
    Target g = {p[0], p[1], p[2], p[3], p[4], p[5]};
    if (g.N < 0) g.N = 0;      // a table that lies about its shapes owns no tile
    if (g.K < 0) g.K = 0;
    return g;
}

DEVINL int64_t merge_tiles(const Target& g) { return cdiv_dev(g.N, MG_ROWS) * cdiv_dev(g.K, MG_COLS); }
DEVINL int64_t grad_panels(const Target& g) { return g.K > 0 ? cdiv_dev(g.N, GR_ROWS) : 0; }

// first[t] = tiles of targets 0 .. t-1 (first[nt] = all), by every workgroup for itself: the counts in parallel, the running sum
// by one lane.  COUNT: 0 merge tiles, 1 grad panels, 2 fold chunks.  `extra`, where given, is the running sum of the workspace
// elements (panels * r * K) in the same pass.
template <int COUNT>
DEVINL void build_first(const int64_t* __restrict__ table, int nt, int r, int* first, int64_t* extra) {
    for (int t = threadIdx.x; t < nt; t += LORA_BLOCK) {
        const Target g = load_target(table, t);
        first[t + 1] = (int)(COUNT == 0 ? merge_tiles(g) : COUNT == 1 ? grad_panels(g) : cdiv_dev((int64_t)r * g.K, FOLD_CHUNK) * (g.N > 0));
        if (extra) extra[t + 1] = grad_panels(g) * r * g.K;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        first[0] = 0;
        if (extra) extra[0] = 0;
        for (int t = 0; t < nt; ++t) {
            first[t + 1] += first[t];
            if (extra) extra[t + 1] += extra[t];
        }
    }
    __syncthreads();
}

DEVINL int find_target(const int* first, int nt, int tile) {   // the t with first[t] <= tile < first[t + 1], wave-uniform
    int lo = 0, hi = nt;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= tile) lo = mid; else hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

DEVINL float readlane_f32(float v, int lane) {   // lane wave-uniform
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

template <int RP>
__global__ __launch_bounds__(LORA_BLOCK) void lora_merge_kernel(const int64_t* __restrict__ table, int nt, int r, float s,
                                                                const float* __restrict__ base, const float* __restrict__ lora,
                                                                float* __restrict__ flat, bf16_t* __restrict__ shadow, int mode) {
    __shared__ int first[LORA_MAX_TARGETS + 1];
    __shared__ __attribute__((aligned(16))) float sA[RP * MG_COLS];
    __shared__ float sB[MG_ROWS * RP];
    build_first<0>(table, nt, r, first, nullptr);
    const int t = threadIdx.x, cg = t & 31, rs = t >> 5;
    constexpr int RPT = MG_ROWS / 8;      // rows per lane
    for (int tile = blockIdx.x; tile < first[nt]; tile += gridDim.x) {
        const int ti = find_target(first, nt, tile);
        const Target g = load_target(table, ti);
        const int64_t ktiles = cdiv_dev(g.K, MG_COLS), local = tile - first[ti];
        const int64_t n0 = local / ktiles * MG_ROWS, k0 = local % ktiles * MG_COLS;
        const int64_t k = k0 + 4 * cg;
        const bool vec = (g.K & 3) == 0;     // rows 16-byte aligned (offsets are multiples of 4 elements): k + 3 < K whenever k < K
        const int cnt = k >= g.K ? 0 : g.K - k < 4 ? (int)(g.K - k) : 4;
        float w[RPT][4];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {      // all loads of W0 in flight before the staging and the arithmetic
            const int64_t n = n0 + rs + 8 * i;
            w[i][0] = w[i][1] = w[i][2] = w[i][3] = 0.f;
            if (n >= g.N || cnt == 0) continue;
            const float* src = base + g.base_off + n * g.K + k;
            if (vec) {
                const f32x4 v = *(const f32x4*)src;
                w[i][0] = v[0]; w[i][1] = v[1]; w[i][2] = v[2]; w[i][3] = v[3];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < cnt) w[i][e] = src[e];
            }
        }
        if (mode == 0) {
            __syncthreads();      // the previous tile's reads of sA / sB are done
            for (int i = t; i < r * MG_COLS; i += LORA_BLOCK) {
                const int j = i / MG_COLS, kk = i % MG_COLS;
                sA[i] = k0 + kk < g.K ? lora[g.a_off + (int64_t)j * g.K + k0 + kk] : 0.f;
            }
            for (int i = t; i < MG_ROWS * r; i += LORA_BLOCK) {
                const int n = i / r, j = i % r;
                sB[n * RP + j] = n0 + n < g.N ? lora[g.b_off + (n0 + n) * r + j] : 0.f;
            }
            __syncthreads();
            float acc[RPT][4];
#pragma unroll
            for (int i = 0; i < RPT; ++i) acc[i][0] = acc[i][1] = acc[i][2] = acc[i][3] = 0.f;
            for (int j = 0; j < r; ++j) {
                const f32x4 a = *(const f32x4*)&sA[j * MG_COLS + 4 * cg];
#pragma unroll
                for (int i = 0; i < RPT; ++i) {
                    const float b = sB[(rs + 8 * i) * RP + j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][e] = fmaf(b, a[e], acc[i][e]);
                }
            }
#pragma unroll
            for (int i = 0; i < RPT; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) w[i][e] = fmaf(s, acc[i][e], w[i][e]);
        }
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int64_t n = n0 + rs + 8 * i;
            if (n >= g.N || cnt == 0) continue;
            const int64_t at = g.off + n * g.K + k;
            if (vec) {
                *(f32x4*)(flat + at) = (f32x4){w[i][0], w[i][1], w[i][2], w[i][3]};
                if (shadow) *(u32x2*)(shadow + at) = (u32x2){pack2bf(w[i][0], w[i][1]), pack2bf(w[i][2], w[i][3])};
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < cnt) {
                        flat[at + e] = w[i][e];
                        if (shadow) shadow[at + e] = f2bf(w[i][e]);
                    }
            }
        }
    }
}

template <int JQ>
__global__ __launch_bounds__(LORA_BLOCK) void lora_grad_kernel(const int64_t* __restrict__ table, int nt, int r, float s,
                                                               const float* __restrict__ lora, const float* __restrict__ grad,
                                                               float* __restrict__ lora_grad, float* __restrict__ ws) {
    __shared__ int first[LORA_MAX_TARGETS + 1];
    __shared__ int64_t ws_first[LORA_MAX_TARGETS + 1];
    __shared__ float sW[GR_ROWS * GR_LD];
    build_first<1>(table, nt, r, first, ws_first);
    const int t = threadIdx.x, lane = t & 63, j0 = __builtin_amdgcn_readfirstlane((t >> 6) * JQ);
    for (int tile = blockIdx.x; tile < first[nt]; tile += gridDim.x) {
        const int ti = find_target(first, nt, tile);
        const Target g = load_target(table, ti);
        const int64_t panel = tile - first[ti], n0 = panel * GR_ROWS;
        const int rows = g.N - n0 < GR_ROWS ? (int)(g.N - n0) : GR_ROWS;
        float* plane = ws + ws_first[ti] + panel * r * g.K;
        const bool vec = (g.K & 3) == 0;
        float breg[JQ], accB[JQ];       // lane n: B[n0 + n][j0 + jj] (0 outside the panel and the rank)
#pragma unroll
        for (int jj = 0; jj < JQ; ++jj) {
            breg[jj] = lane < rows && j0 + jj < r ? lora[g.b_off + (n0 + lane) * r + j0 + jj] : 0.f;
            accB[jj] = 0.f;
        }
        // chunk k0 as this lane holds it between its loads and the LDS image: 4 pieces of 4 columns, and A[j0 + jj][k0 + lane]
        // (0 outside the panel, the chunk and the rank).  The loads of chunk k0 + 64 are issued before the arithmetic on chunk k0.
        float cur[GR_ROWS * GR_COLS / 4 / LORA_BLOCK][4], anext[JQ];
        auto load_chunk = [&](int64_t k0) {
            const int kcnt = g.K - k0 < GR_COLS ? (int)(g.K - k0) : GR_COLS;
#pragma unroll
            for (int i = 0; i < GR_ROWS * GR_COLS / 4 / LORA_BLOCK; ++i) {
                const int idx = t + LORA_BLOCK * i, row = idx / (GR_COLS / 4), c = 4 * (idx % (GR_COLS / 4));
                cur[i][0] = cur[i][1] = cur[i][2] = cur[i][3] = 0.f;
                if (row < rows && c < kcnt) {
                    const float* src = grad + g.off + (n0 + row) * g.K + k0 + c;
                    if (vec) {
                        const f32x4 q = *(const f32x4*)src;
                        cur[i][0] = q[0]; cur[i][1] = q[1]; cur[i][2] = q[2]; cur[i][3] = q[3];
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (c + e < kcnt) cur[i][e] = src[e];
                    }
                }
            }
#pragma unroll
            for (int jj = 0; jj < JQ; ++jj)
                anext[jj] = lane < kcnt && j0 + jj < r ? lora[g.a_off + (int64_t)(j0 + jj) * g.K + k0 + lane] : 0.f;
        };
        load_chunk(0);
        for (int64_t k0 = 0; k0 < g.K; k0 += GR_COLS) {
            const int kcnt = g.K - k0 < GR_COLS ? (int)(g.K - k0) : GR_COLS;
            __syncthreads();      // the previous chunk's reads of sW are done
#pragma unroll
            for (int i = 0; i < GR_ROWS * GR_COLS / 4 / LORA_BLOCK; ++i) {
                const int idx = t + LORA_BLOCK * i, row = idx / (GR_COLS / 4), c = 4 * (idx % (GR_COLS / 4));
#pragma unroll
                for (int e = 0; e < 4; ++e) sW[row * GR_LD + c + e] = cur[i][e];
            }
            float areg[JQ];
#pragma unroll
            for (int jj = 0; jj < JQ; ++jj) areg[jj] = anext[jj];
            __syncthreads();
            if (k0 + GR_COLS < g.K) load_chunk(k0 + GR_COLS);
            {   // dA of this panel, columns k0 .. k0 + kcnt - 1: complete after the panel's rows
                float acc[JQ];
#pragma unroll
                for (int jj = 0; jj < JQ; ++jj) acc[jj] = 0.f;
#pragma unroll 8
                for (int n = 0; n < rows; ++n) {
                    const float x = sW[n * GR_LD + lane];
#pragma unroll
                    for (int jj = 0; jj < JQ; ++jj) acc[jj] = fmaf(readlane_f32(breg[jj], n), x, acc[jj]);
                }
                if (lane < kcnt) {
#pragma unroll
                    for (int jj = 0; jj < JQ; ++jj)
                        if (j0 + jj < r) plane[(int64_t)(j0 + jj) * g.K + k0 + lane] = acc[jj];
                }
            }
            // dB of row `lane`: the chain goes on over the chunks
#pragma unroll 8
            for (int kk = 0; kk < kcnt; ++kk) {
                const float x = sW[lane * GR_LD + kk];
#pragma unroll
                for (int jj = 0; jj < JQ; ++jj) accB[jj] = fmaf(x, readlane_f32(areg[jj], kk), accB[jj]);
            }
        }
        if (lane < rows) {
#pragma unroll
            for (int jj = 0; jj < JQ; ++jj)
                if (j0 + jj < r) lora_grad[g.b_off + (n0 + lane) * r + j0 + jj] = s * accB[jj];
        }
    }
}

__global__ __launch_bounds__(LORA_BLOCK) void lora_fold_kernel(const int64_t* __restrict__ table, int nt, int r, float s,
                                                               const float* __restrict__ ws, float* __restrict__ lora_grad) {
    __shared__ int first[LORA_MAX_TARGETS + 1];
    __shared__ int64_t ws_first[LORA_MAX_TARGETS + 1];
    build_first<2>(table, nt, r, first, ws_first);
    for (int tile = blockIdx.x; tile < first[nt]; tile += gridDim.x) {
        const int ti = find_target(first, nt, tile);
        const Target g = load_target(table, ti);
        const int64_t rk = (int64_t)r * g.K, e = (tile - first[ti]) * FOLD_CHUNK + threadIdx.x, panels = grad_panels(g);
        if (e >= rk) continue;
        const float* p = ws + ws_first[ti] + e;
        float acc = p[0];
        for (int64_t q = 1; q < panels; ++q) acc += p[q * rk];
        lora_grad[g.a_off + e] = s * acc;
    }
}

bool rank_ok(int64_t ntargets, int64_t r) { return ntargets >= 1 && ntargets <= LORA_MAX_TARGETS && r >= 1 && r <= LORA_MAX_RANK; }

}  // namespace

extern "C" int m3ae_lora_merge(const int64_t* table_dev, int64_t ntargets, int64_t r, float s, const float* base, const float* lora,
                               float* flat, void* shadow_bf16, int mode, void* stream) {
    if (!table_dev || !base || !flat || (mode != 0 && mode != 1) || (mode == 0 && (!lora || !isfinite(s)))) return M3AE_ERR_ARG;
    if (!rank_ok(ntargets, r)) return ntargets < 1 || r < 1 ? M3AE_ERR_ARG : M3AE_ERR_UNSUPPORTED;
    if (((uintptr_t)table_dev & 7) || (((uintptr_t)base | (uintptr_t)lora | (uintptr_t)flat) & 15) || ((uintptr_t)shadow_bf16 & 7))
        return M3AE_ERR_ALIGN;
#define LORA_MERGE(RP) hipLaunchKernelGGL(lora_merge_kernel<RP>, dim3(LORA_GRID), dim3(LORA_BLOCK), 0, (hipStream_t)stream, table_dev, \
                                          (int)ntargets, (int)r, s, base, lora, flat, (bf16_t*)shadow_bf16, mode)
    if (r <= 4) LORA_MERGE(4);
    else if (r <= 8) LORA_MERGE(8);
    else if (r <= 16) LORA_MERGE(16);
    else if (r <= 32) LORA_MERGE(32);
    else LORA_MERGE(64);
#undef LORA_MERGE
    return hip_launch_status();
}

extern "C" int64_t m3ae_lora_grad_workspace_bytes(const int64_t* table_host, int64_t ntargets, int64_t r) {
    if (!table_host || ntargets < 1 || r < 1) return M3AE_ERR_ARG;
    if (!rank_ok(ntargets, r)) return M3AE_ERR_UNSUPPORTED;
    int64_t elems = 0;
    for (int64_t t = 0; t < ntargets; ++t) {
        const int64_t N = table_host[6 * t + 1], K = table_host[6 * t + 2];
        if (N < 1 || K < 1) return M3AE_ERR_ARG;
        elems += cdiv(N, GR_ROWS) * r * K;
    }
    return 4 * elems;
}

extern "C" int m3ae_lora_grad(const int64_t* table_dev, int64_t ntargets, int64_t r, float s, const float* lora, const float* grad_flat,
                              float* lora_grad, void* workspace, void* stream) {
    if (!table_dev || !lora || !grad_flat || !lora_grad || !isfinite(s)) return M3AE_ERR_ARG;
    if (!rank_ok(ntargets, r)) return ntargets < 1 || r < 1 ? M3AE_ERR_ARG : M3AE_ERR_UNSUPPORTED;
    if (!workspace) return M3AE_ERR_WORKSPACE;
    if (((uintptr_t)table_dev & 7) || (((uintptr_t)lora | (uintptr_t)grad_flat | (uintptr_t)lora_grad) & 15) || ((uintptr_t)workspace & 3))
        return M3AE_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(LORA_GRID), block(LORA_BLOCK);
    const int nt = (int)ntargets, ri = (int)r;
    float* ws = (float*)workspace;
#define LORA_GRAD(JQ) hipLaunchKernelGGL(lora_grad_kernel<JQ>, grid, block, 0, st, table_dev, nt, ri, s, lora, grad_flat, lora_grad, ws)
    if (r <= 4) LORA_GRAD(1);
    else if (r <= 8) LORA_GRAD(2);
    else if (r <= 16) LORA_GRAD(4);
    else if (r <= 32) LORA_GRAD(8);
    else LORA_GRAD(16);
#undef LORA_GRAD
    hipLaunchKernelGGL(lora_fold_kernel, grid, block, 0, st, table_dev, nt, ri, s, (const float*)ws, lora_grad);
    return hip_launch_status();
}
