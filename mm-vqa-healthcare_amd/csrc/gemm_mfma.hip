// bf16 MFMA GEMM kernels for gfx950 (CDNA4): the 93 % of the hot path's FLOPs.
//
//   NT : C[M,N] = epi(alpha * A[M,K] . B[N,K]^T)  -- forward Linear (x . W^T) and dgrad (dY . (W^T)^T with the
//        transposed bf16 weight shadow), both operands K-contiguous.
//   TN : C[N1,N2] += alpha * A[Mr,N1]^T . B[Mr,N2] -- wgrad (dY^T . X): the reduction runs over the ROWS of both
//        operands, so MFMA fragments are fetched with the hardware transposing LDS read ds_read_b64_tr_b16;
//        split over the reduction with fp32 atomics into the (fp32) gradient buffer, or (deterministic mode, m3ae_gemm_det)
//        with partial tiles in a workspace that a streaming kernel folds in ascending split order.
//
// Structure (both): 128x128 output tile per 256-thread workgroup (4 waves as 2x2, 64x64 per wave = 4x4 MFMA
// 16x16x32 tiles, 64 fp32 accumulators/lane), 64-deep reduction step, operands staged global->LDS with
// global_load_lds_dwordx4 (no VGPR round trip) into a 2-stage ring (64 KiB -> 2 workgroups/CU), one barrier per
// step with the next stage's DMA in flight under the MFMAs.  LDS images are XOR-swizzled on the SOURCE address
// (the LDS-DMA destination is lane-linear) with the same involution on the read, so ds_read_b128 / tr reads are
// bank-conflict free.  Workgroup ids are remapped so that each XCD (own L2) walks a contiguous range of tiles.
#include "gemm_nt_common.h"
#include "pp_ring.h"
#include "launch.h"
#include <stdlib.h>

namespace {

constexpr int BM = 128, BN = 128, BK = 64;         // TN kernel tile
constexpr int STAGE_BYTES = (BM + BN) * BK * 2;    // 32 KiB
constexpr int LDS_BYTES = 2 * STAGE_BYTES;         // 64 KiB

using namespace m3g;

// BM_ x BN_ output tile, one WM x 64 sub-tile per wave ((BM_/WM) x (BN_/64) waves), BKT-deep reduction steps, NST-stage
// LDS ring with the DMA of stage t + NST - 1 issued before the MFMAs of stage t and retired by a COUNTED s_waitcnt
// (loads stay in flight across the raw s_barrier).
template <int BM_, int BN_, int BKT, int NST, int WM, int EPI>
__global__ __launch_bounds__((BM_ / WM) * (BN_ / 64) * 64, 2) void gemm_nt_bf16_kernel(MfmaArgs a) {
    if (a.has_drop) drop_resolve(a.drop);
    constexpr int WAVES_N = BN_ / 64, NWAVES = (BM_ / WM) * WAVES_N, MI = WM / 16;
    constexpr int A_BYTES = BM_ * BKT * 2, ST_BYTES = (BM_ + BN_) * BKT * 2;
    constexpr int A_SEGS = A_BYTES / 1024 / NWAVES, B_SEGS = BN_ * BKT * 2 / 1024 / NWAVES;  // DMA pieces per wave
    constexpr int G = A_SEGS + B_SEGS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;

    const unsigned tiles_n = (unsigned)((a.N + BN_ - 1) / BN_);
    unsigned tm, tn;
    nt_tile_coords(xcd_remap(blockIdx.x, gridDim.x), gridDim.x / tiles_n, tiles_n, tm, tn);
    const int64_t m0 = (int64_t)tm * BM_;
    const int64_t n0 = (int64_t)tn * BN_;

    f32x4 acc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nt = (int)(a.K / BKT);
#pragma unroll
    for (int s = 0; s < NST - 1; ++s) {
        if (s < nt) {
            nt_stage<BKT, A_SEGS, NWAVES>(a.A, a.lda, m0, a.M, (int64_t)s * BKT, smem + s * ST_BYTES, wave, lane);
            if (a.b_tiled) nt_stage_tiled<BKT, B_SEGS, NWAVES>(a.B, a.K, n0, (int64_t)s * BKT, smem + s * ST_BYTES + A_BYTES, wave, lane);
            else nt_stage<BKT, B_SEGS, NWAVES>(a.B, a.ldb, n0, a.N, (int64_t)s * BKT, smem + s * ST_BYTES + A_BYTES, wave, lane);
        }
    }

    const int frow = lane & 15, fchunk = lane >> 4;
    int cur_s = 0, nxt_s = NST - 1;
    for (int t = 0; t < nt; ++t) {
        // stage t has landed once at most the NST - 2 younger stages of this wave are still in flight
        if (t + NST - 2 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * G) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // every wave's pieces of stage t landed; everyone left stage t - 1's buffer
        asm volatile("" ::: "memory");
        if (t + NST - 1 < nt) {
            char* nxt = smem + nxt_s * ST_BYTES;
            nt_stage<BKT, A_SEGS, NWAVES>(a.A, a.lda, m0, a.M, (int64_t)(t + NST - 1) * BKT, nxt, wave, lane);
            if (a.b_tiled) nt_stage_tiled<BKT, B_SEGS, NWAVES>(a.B, a.K, n0, (int64_t)(t + NST - 1) * BKT, nxt + A_BYTES, wave, lane);
            else nt_stage<BKT, B_SEGS, NWAVES>(a.B, a.ldb, n0, a.N, (int64_t)(t + NST - 1) * BKT, nxt + A_BYTES, wave, lane);
        }
        const char* At = smem + cur_s * ST_BYTES;
        const char* Bt = At + A_BYTES;
#pragma unroll
        for (int kk = 0; kk < BKT / 32; ++kk) {
            s16x8 af[MI], bfr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = nt_frag<BKT>(Bt, wc * 64 + j * 16 + frow, kk * 4 + fchunk);
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = nt_frag<BKT>(At, wr * WM + i * 16 + frow, kk * 4 + fchunk);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    // D'[n][m] = sum_k B[n][k] * A[m][k]: each lane ends with 4 consecutive n of one m
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        __builtin_bit_cast(bf16x8_t, bfr[j]), __builtin_bit_cast(bf16x8_t, af[i]), acc[i][j], 0, 0, 0);
        }
        asm volatile("" ::: "memory");
        cur_s = cur_s + 1 == NST ? 0 : cur_s + 1;
        nxt_s = nxt_s + 1 == NST ? 0 : nxt_s + 1;
    }

    if (a.rows_epi) {
        __builtin_amdgcn_s_barrier();  // every wave has consumed its last stage: the ring is free for the C slabs
        asm volatile("" ::: "memory");
        if (a.c_f32) epilogue_rows<float, EPI, MI>(a, smem, wave, lane, m0 + wr * WM, n0 + wc * 64, acc);
        else epilogue_rows<bf16_t, EPI, MI>(a, smem, wave, lane, m0 + wr * WM, n0 + wc * 64, acc);
        return;
    }
    // direct epilogue (N % 8 != 0): lane holds C[m = .. + (lane & 15)][n = .. + 4 * (lane >> 4) + 0..3]
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int64_t m = m0 + wr * WM + i * 16 + (lane & 15);
        if (m >= a.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t n = n0 + wc * 64 + j * 16 + 4 * (lane >> 4);
            if (n >= a.N) continue;  // N % 4 == 0 is a precondition, so n < N implies n + 3 < N
            if (a.c_f32) epilogue4<float, EPI>(a, m, n, acc[i][j]);
            else epilogue4<bf16_t, EPI>(a, m, n, acc[i][j]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// TN kernel (wgrad)
// ---------------------------------------------------------------------------------------------------------
// C[n1][n2] (+)= alpha * sum_r A[r][n1] * B[r][n2];  a.M = N1, a.N = N2, a.K = reduction rows.
// BM_ x BN_ output tile, one WM x 64 sub-tile per wave, 64 reduction rows per step, 2-stage ring.
// DET (deterministic mode, M3AE_GEMM_DETERMINISTIC): the workgroup of (tile, split) stores its raw fp32 accumulators -- and its
// partial a_rowsum rows -- into the caller's workspace instead of adding them into C with atomics: a.C / a.a_rowsum then point
// at the partial planes, laid out in accumulator order ([split][tile][wave][i][j][lane] f32x4: every store instruction of a
// wave writes 1 KiB of consecutive bytes), and tn_det_fold_kernel sums the planes in ascending split order.  The main loop is
// the same code, so the order of accumulation inside a split is the atomic form's.
template <int BM_, int BN_, int WM, int BKR, int NST, bool DET = false>
__global__ __launch_bounds__((BM_ / WM) * (BN_ / 64) * 64, 2) void gemm_tn_bf16_kernel(MfmaArgs a) {
    constexpr int WAVES_N = BN_ / 64, NWAVES = (BM_ / WM) * WAVES_N, MI = WM / 16;
    constexpr int A_BYTES = BM_ * BKR * 2, ST_BYTES = (BM_ + BN_) * BKR * 2;
    constexpr int A_SEGS = A_BYTES / 1024 / NWAVES, B_SEGS = BN_ * BKR * 2 / 1024 / NWAVES;
    constexpr int G = A_SEGS + B_SEGS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WAVES_N, wc = wave % WAVES_N;

    const unsigned tiles_n = (unsigned)(a.N / BN_);
    const unsigned tiles = (unsigned)(a.M / BM_) * tiles_n;
    const unsigned wg = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned tile_id = wg % tiles, split = wg / tiles;
    const int64_t m0 = (int64_t)(tile_id / tiles_n) * BM_;
    const int64_t n0 = (int64_t)(tile_id % tiles_n) * BN_;
    const int64_t r_begin = (int64_t)split * a.k_chunk;
    int64_t r_end = r_begin + a.k_chunk;
    if (r_end > a.K) r_end = a.K;
    if (r_begin >= r_end) return;  // whole workgroup: uniform
    const int nt = (int)((r_end - r_begin + BKR - 1) / BKR);

    f32x4 acc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // bias gradient rides along: the waves of the first output-column tile also multiply their A^T fragments by a
    // ones fragment (every column of that product is the row sum of A^T = the column sum of dY)
    const bool do_rowsum = a.a_rowsum != nullptr && n0 == 0 && wc == 0;
    f32x4 rsum[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) rsum[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const s16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

#pragma unroll
    for (int s = 0; s < NST - 1; ++s) {
        if (s < nt) {
            const int64_t r0 = r_begin + (int64_t)s * BKR;
            tn_stage<BM_, A_SEGS, NWAVES>(a.A, a.lda, r0, r_end, m0, smem + s * ST_BYTES, wave, lane);
            tn_stage<BN_, B_SEGS, NWAVES>(a.B, a.ldb, r0, r_end, n0, smem + s * ST_BYTES + A_BYTES, wave, lane);
        }
    }
    int cur_s = 0, nxt_s = NST - 1;
    for (int t = 0; t < nt; ++t) {
        if (t + NST - 2 < nt) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NST - 2) * G) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + NST - 1 < nt) {
            char* nxt = smem + nxt_s * ST_BYTES;
            const int64_t r0 = r_begin + (int64_t)(t + NST - 1) * BKR;
            tn_stage<BM_, A_SEGS, NWAVES>(a.A, a.lda, r0, r_end, m0, nxt, wave, lane);
            tn_stage<BN_, B_SEGS, NWAVES>(a.B, a.ldb, r0, r_end, n0, nxt + A_BYTES, wave, lane);
        }
        const char* At = smem + cur_s * ST_BYTES;
        const char* Bt = At + A_BYTES;
#pragma unroll
        for (int kk = 0; kk < BKR / 32; ++kk) {
            s16x8 af[MI], bfr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = tn_frag<BN_>(Bt, kk * 32, wc * 64 + j * 16, lane);
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = tn_frag<BM_>(At, kk * 32, wr * WM + i * 16, lane);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    // D[n1][n2] = sum_r A^T[n1][r] * B[r][n2]
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        __builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, bfr[j]), acc[i][j], 0, 0, 0);
            if (do_rowsum) {
#pragma unroll
                for (int i = 0; i < MI; ++i)
                    rsum[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        __builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, ones), rsum[i], 0, 0, 0);
            }
        }
        asm volatile("" ::: "memory");
        cur_s = cur_s + 1 == NST ? 0 : cur_s + 1;
        nxt_s = nxt_s + 1 == NST ? 0 : nxt_s + 1;
    }
    if constexpr (DET) {
        if (do_rowsum && (lane & 15) == 0) {
            float* rs = a.a_rowsum + (int64_t)split * a.M + m0 + wr * WM + 4 * (lane >> 4);
#pragma unroll
            for (int i = 0; i < MI; ++i) *(f32x4*)(rs + i * 16) = rsum[i];
        }
        float* P = (float*)a.C + ((int64_t)split * tiles + tile_id) * (BM_ * BN_) + ((int64_t)wave * MI * 4 * 64 + lane) * 4;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) *(f32x4*)(P + (i * 4 + j) * 256) = acc[i][j];
        return;
    }
    if (do_rowsum && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) atomicAdd(a.a_rowsum + m0 + wr * WM + i * 16 + 4 * (lane >> 4) + r, rsum[i][r]);
    }

    // lane holds D[n1 = .. + 4 * (lane >> 4) + reg][n2 = .. + (lane & 15)]
    float* C = (float*)a.C;
    const bool atomic = a.splits > 1;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t n1 = m0 + wr * WM + i * 16 + 4 * (lane >> 4) + r;
                const int64_t n2 = n0 + wc * 64 + j * 16 + (lane & 15);
                float* p = C + n1 * a.ldc + n2;
                const float x = acc[i][j][r] * a.alpha;
                if (atomic) atomicAdd(p, x);
                else if (a.accumulate) *p += x;
                else *p = x;
            }
}

}  // namespace

static thread_local const char* g_last_path = "none";
const char* m3ae_last_gemm_path(void) { return g_last_path; }

int m3ae_gemm_generic(const m3ae_gemm_desc& d, hipStream_t s, DropRows rows = DropRows{0, 1});
int m3ae_gemm_f32x3(const m3ae_gemm_desc& d, hipStream_t s, DropRows rows = DropRows{0, 1});

static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// Kernel selection is by shape (nt_kernel_choice / tn_kernel_choice below).  A caller may pin a variant PER CALL through the selector
// fields of m3ae_gemm_desc.launch_flags (M3AE_GEMM_NT_VARIANT / _TN_VARIANT / _COL_GROUP: tests compare the variants bit for bit, tools
// time them against each other); the library keeps no tuning state and reads no environment variable.
// The persistent launch of the second-generation ping-pong kernel (gemm_nt_pp2.hip: static tile lists, one workgroup per CU) is never
// taken under M3AE_GEMM_NO_PERSISTENT (data-parallel runs): when RCCL's kernels hold some CUs the persistent workgroups that found no
// CU only start after others have walked their whole tile list (the kernel's time doubles); the one-tile-per-workgroup launch just
// runs on the CUs that are free.

template <int BM_, int BN_, int BKT, int NST, int WM, int EPI>
static int launch_nt_t(const MfmaArgs& a, hipStream_t s) {
    constexpr int nwaves = (BM_ / WM) * (BN_ / 64);
    constexpr int ring = NST * (BM_ + BN_) * BKT * 2, slabs = nwaves * 32 * 68 * 4;
    constexpr int lds = ring > slabs ? ring : slabs;
    constexpr int threads = nwaves * 64;
    const int64_t tiles = cdiv(a.M, BM_) * cdiv(a.N, BN_);
    return launch_dyn<gemm_nt_bf16_kernel<BM_, BN_, BKT, NST, WM, EPI>>(dim3((unsigned)tiles), dim3(threads), lds, s, a);
}


// ---------------------------------------------------------------------------------------------------------
// NT "ping-pong" kernel: 256 x 256 tile, 8 waves (2 x 4, 128 x 64 each), 32-deep reduction chunks in a 4-slot LDS
// ring (128 KiB): the two-phase schedule of pp_ring.h (ring safety and the counted-wait rule there) -- rows 0-63 / 64-127 of the
// wave's sub-tile, 16 MFMAs per phase, the two wave rows (wr = 0 / 1: one wave of each per SIMD) staggered by one barrier, 2 + 2
// LDS-DMA pieces per wave and chunk.  The loop is written out in each of the three kernels that run this schedule (this one,
// gemm_tn_pp_kernel, xg_kernel with NLOAD == 0).  ONE template over staging / fragment / MFMA callables was built and measured
// (profiles/r17_pp_ring_ab.log): hipcc no longer shared the row clamps and row products of the three prologue chunks (+120..200
// instructions per tile) and K = 192 here and the 3072 x 768 wgrad ran 1-2 % slower.  Those builds also carried the slower form of
// the in-flight rule (pp_ring.h, pp_inflight_next), which alone costs the wgrad kernel 2 %: the template was not measured again
// without it.
// The B operand of a chunk comes from the tiled copy of the weight under M3AE_GEMM_B_TILED (one lane-linear 1-KiB block per piece).
// ---------------------------------------------------------------------------------------------------------
template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_nt_pp_kernel(MfmaArgs a) {
    if (a.has_drop) drop_resolve(a.drop);
    constexpr int CK = 32, NW = 8, A_BYTES = 256 * CK * 2, SLOT = 2 * A_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    const unsigned tiles_n = (unsigned)((a.N + 255) / 256);
    unsigned tm, tn;
    nt_tile_coords(xcd_remap(blockIdx.x, gridDim.x), gridDim.x / tiles_n, tiles_n, tm, tn, (unsigned)a.col_group);
    const int64_t m0 = (int64_t)tm * 256;
    const int64_t n0 = (int64_t)tn * 256;

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    constexpr int DEPTH = 3, G = 4;   // chunks requested ahead; LDS-DMA pieces per wave and chunk (pp_ring.h)
    const int nc = (int)(a.K / CK);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c < nc) {
            if (a.b_tiled) nt_stage_tiled32<2, NW>(a.B, a.K, n0, (int64_t)c * CK, smem + c * SLOT + A_BYTES, wave, lane);
            else nt_stage<CK, 2, NW>(a.B, a.ldb, n0, a.N, (int64_t)c * CK, smem + c * SLOT + A_BYTES, wave, lane);
            nt_stage<CK, 2, NW>(a.A, a.lda, m0, a.M, (int64_t)c * CK, smem + c * SLOT, wave, lane);
        }
    }
    wait_vm_chunks<G, DEPTH - 1>(pp_inflight_prologue<DEPTH>(nc));
    PP_FENCE();
    __builtin_amdgcn_s_barrier();  // chunk 0 is in LDS for every wave
    PP_FENCE();
    if (wr == 1) { __builtin_amdgcn_s_barrier(); PP_FENCE(); }  // stagger the second wave row by one barrier

    const int frow = lane & 15, fchunk = lane >> 4;
    for (int c = 0; c < nc; ++c) {
        const char* At = smem + (c & 3) * SLOT;
        const char* Bt = At + A_BYTES;
        char* nxt = smem + ((c + 3) & 3) * SLOT;
        const bool more = c + 3 < nc;
        s16x8 bfr[4], af[4];
        // ---------------- phase 2c: rows 0..63 of the wave's sub-tile
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = nt_frag<CK>(Bt, wc * 64 + j * 16 + frow, fchunk);
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = nt_frag<CK>(At, wr * 128 + i * 16 + frow, fchunk);
        if (more) {
            if (a.b_tiled) nt_stage_tiled32<2, NW>(a.B, a.K, n0, (int64_t)(c + 3) * CK, nxt + A_BYTES, wave, lane);
            else nt_stage<CK, 2, NW>(a.B, a.ldb, n0, a.N, (int64_t)(c + 3) * CK, nxt + A_BYTES, wave, lane);
        }
        PP_FENCE();
        __builtin_amdgcn_s_barrier();
        PP_FENCE();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(bf16x8_t, bfr[j]), __builtin_bit_cast(bf16x8_t, af[i]), acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        PP_FENCE();
        __builtin_amdgcn_s_barrier();
        PP_FENCE();
        // ---------------- phase 2c + 1: rows 64..127 (the B fragments stay in registers)
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = nt_frag<CK>(At, wr * 128 + 64 + i * 16 + frow, fchunk);
        if (more) nt_stage<CK, 2, NW>(a.A, a.lda, m0, a.M, (int64_t)(c + 3) * CK, nxt, wave, lane);
        wait_vm_chunks<G, DEPTH - 1>(pp_inflight_next<DEPTH>(nc, c));   // chunk c + 1 must have landed before the next phase
        PP_FENCE();
        __builtin_amdgcn_s_barrier();
        PP_FENCE();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(bf16x8_t, bfr[j]), __builtin_bit_cast(bf16x8_t, af[i]), acc[4 + i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        PP_FENCE();
        __builtin_amdgcn_s_barrier();
        PP_FENCE();
    }
    if (wr == 0) { __builtin_amdgcn_s_barrier(); PP_FENCE(); }  // re-align: every wave has executed 4 nc + 2 barriers
    // all fragment reads are retired and no DMA is outstanding: the ring is free (pp_ring.h)

    if (a.rows_epi) {
        if (a.c_f32) epilogue_rows<float, EPI, 8>(a, smem, wave, lane, m0 + wr * 128, n0 + wc * 64, acc);
        else epilogue_rows<bf16_t, EPI, 8>(a, smem, wave, lane, m0 + wr * 128, n0 + wc * 64, acc);
        return;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t m = m0 + wr * 128 + i * 16 + (lane & 15);
        if (m >= a.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t n = n0 + wc * 64 + j * 16 + 4 * (lane >> 4);
            if (n >= a.N) continue;
            if (a.c_f32) epilogue4<float, EPI>(a, m, n, acc[i][j]);
            else epilogue4<bf16_t, EPI>(a, m, n, acc[i][j]);
        }
    }
}

template <int EPI>
static int launch_nt_pp(const MfmaArgs& a, hipStream_t s) {
    constexpr int lds = 4 * (256 + 256) * 32 * 2;  // 128 KiB ring; the epilogue slabs (8 x 8704 B) reuse it
    const int64_t tiles = cdiv(a.M, 256) * cdiv(a.N, 256);
    return launch_dyn<gemm_nt_pp_kernel<EPI>>(dim3((unsigned)tiles), dim3(512), lds, s, a);
}

// NT kernels (launch_flags: M3AE_GEMM_NT_VARIANT(v) pins one; every other value of v runs the 128 x 128 kernel):
//   NT_T128 (v = 0): 128x128 tile, BK 64, 2 stages, 4 waves x (64x64)  -- 64 KiB LDS, 2 workgroups / CU (small / few-tile shapes)
//   NT_T256 (v = 4): 256x256 tile, BK 64, 2 stages, 8 waves x (128x64) -- 128 KiB LDS, 1 workgroup / CU (the ping-pong kernels'
//      bit-exact reference in tools/gemm_race.py)
//   NT_PP (v = 7): 256x256 tile, 32-deep chunks in a 4-slot ring, 8 waves in two staggered rows (ping-pong, gemm_nt_pp_kernel): the
//      256 tile of the shapes the second generation does not take (K < 256, or an output that is not row-epilogue capable)
//   NT_PP2 / NT_PP2_PERSISTENT (v = 9 / 10): the second-generation ping-pong kernel (gemm_nt_pp2.hip), one workgroup per tile /
//      persistent (grid = CUs)
//   v = 8 was the persistent form of gemm_nt_pp_kernel (static tile lists, one workgroup per CU; >= 512 tiles); retired: the class
//      it still served by shape (K in {128, 192}, >= 512 tiles, row-epilogue capable) is one no model configuration produces
//      (DESIGN.md 6).  Last present in commit 8532550.
// Tilings tried and dropped (measured slower on every shape of the path, r01 logs): a 128x256 "dual" kernel (4 waves, two
// workgroups per CU so that one's main loop runs under the other's epilogue; bit-identical, 3-9 % slower, removed in r02);
// 256x128 with BK 64 / 3 stages,
// 256x128 with BK 32 / 2 and 3 stages, 256x256 with BK 32 / 4 stages (single barrier), 128x128 with BK 32;
// 256x256 with FOUR waves of 128x128 (256 accumulators pinned to AGPRs through asm constraints, one wave per SIMD, fragments
// software-pipelined in registers, 33 % fewer LDS fragment bytes per MFMA): bit-identical, 1143 vs 1281 TF/s at 8192^3
// and 12-25 % slower on the path's shapes (profiles/r01_nt_w4_probe.log) -- one wave per SIMD does not keep the MFMA
// pipe as busy as the two staggered wave rows do.
enum NtKernel { NT_T128, NT_T256, NT_PP, NT_PP2, NT_PP2_PERSISTENT };

static NtKernel nt_kernel_choice(const MfmaArgs& a) {
    const bool both = a.M > 128 && a.N > 128;               // a 256 x 256 tile needs more than 128 rows and columns to fill
    const bool pp2_ok = both && a.rows_epi && a.K >= 256;   // gemm_nt_pp2.hip
    if (a.nt_variant >= 0) {                                // pinned
        switch (a.nt_variant) {
        case 9: return pp2_ok ? NT_PP2 : NT_T128;
        case 10: return pp2_ok ? NT_PP2_PERSISTENT : NT_T128;
        case 7: return both ? NT_PP : NT_T128;
        case 4: return both ? NT_T256 : NT_T128;
        default: return NT_T128;
        }
    }
    // by shape (default): measured on MI355X, profiles/r01_gemm_shapes.log
    // 256 x 256 ping-pong kernel (one workgroup per CU, 256 slots) or 128 x 128 kernel (two per CU, 512 slots)?  What
    // decides is how full the last round of tiles is: efficiency = tiles / (rounds * slots).  The ping-pong kernel is
    // ~12 % faster per FLOP on full rounds, so it is taken when eff256 >= 0.88 eff128.  Fits every measured pair
    // (MI355X, K = 768 / 3072): 8192 x 3072 (0.75 vs 1.00: 66 vs 47 us -> 128), 8192 x 768 (0.38 vs 0.75 -> 128),
    // 36928 x 768 (0.85 vs 0.85: 54 vs 57 us, 164 vs 181 us -> 256), 3072 x 3072 (0.56 vs 0.56: 25.7 vs 26.0 us),
    // 2048 x 3072 (0.38 vs 0.75: 23.5 vs 17.1 us -> 128); profiles/r01_gemm_shapes.log, r01_nt_tile_rule.log.
    const int64_t t256 = cdiv(a.M, 256) * cdiv(a.N, 256), t128 = cdiv(a.M, 128) * cdiv(a.N, 128);
    const double eff256 = (double)t256 / (double)(cdiv(t256, 256) * 256);
    const double eff128 = (double)t128 / (double)(cdiv(t128, 512) * 512);
    // (round 4, pp2 against the 128 x 128 kernel at 18464 rows: N = 3072 (0.855 vs 0.971) is 5-13 % faster on the 128 x 128 kernel,
    // N = 768 / 2304 (0.855 vs 0.85) 4-19 % faster on pp2: the threshold moved from 0.88 to 0.93, profiles/r04_nt_kernel_choice_small_batch.log)
    if (!both || eff256 < 0.93 * eff128) return NT_T128;
    if (!pp2_ok) return NT_PP;
    // second-generation ping-pong kernel (gemm_nt_pp2.hip): -2.2 % against the persistent first-generation kernel (retired, see above)
    // over the step's eleven shape / epilogue classes at per-GPU batch 256, -3.6 % against the one-tile-per-workgroup form
    // data-parallel runs take (profiles/r04_nt_pp2_second_ab.log).  Its persistent launch (grid = CUs) is 0.9 % faster than one
    // workgroup per tile on the kernels alone and 0.8 % on the whole step (1303 vs 1293 pairs/s,
    // profiles/r04_nt_pp2_stagger_and_persistent_ab.log), from two full rounds of tiles on; data-parallel runs
    // (M3AE_GEMM_NO_PERSISTENT) take the per-tile launch: static tile lists start late beside RCCL's kernels.
    return t256 >= 512 && !a.no_persist ? NT_PP2_PERSISTENT : NT_PP2;
}

template <int EPI>
static int launch_nt_v(const MfmaArgs& a, hipStream_t s) {
    const NtKernel k = nt_kernel_choice(a);
    g_last_path = k == NT_PP ? "mfma_nt_pp" : (k == NT_PP2 || k == NT_PP2_PERSISTENT) ? "mfma_nt_pp2" : "mfma_nt";
    switch (k) {
    case NT_PP2: return launch_nt_pp2(a, EPI, false, s);
    case NT_PP2_PERSISTENT: return launch_nt_pp2(a, EPI, true, s);
    case NT_PP: return launch_nt_pp<EPI>(a, s);
    case NT_T256: return launch_nt_t<256, 256, 64, 2, 128, EPI>(a, s);
    default: return launch_nt_t<128, 128, 64, 2, 64, EPI>(a, s);
    }
}


static int launch_nt(const m3ae_gemm_desc& d, hipStream_t s, DropRows rows) {
    MfmaArgs a{};
    a.A = (const bf16_t*)d.A; a.lda = d.a_sm;
    a.B = (const bf16_t*)d.B; a.ldb = d.b_sn;
    a.C = d.C; a.ldc = d.c_sm;
    a.M = d.M; a.N = d.N; a.K = d.K;
    a.c_f32 = d.dtype_c == M3AE_F32;
    a.alpha = d.alpha; a.accumulate = d.accumulate; a.bias = d.bias; a.act = d.act; a.preact = d.preact;
    a.preact_grad = d.preact_grad;
    a.residual = d.residual; a.dact_aux = d.dact_aux; a.dact = d.dact;
    a.rows_epi = (d.N % 8 == 0 && d.c_sm % 8 == 0) ? 1 : 0;
    {   // column tiles per group of the ping-pong kernels' tile order: all of them up to 9 (N <= 2304: B <= 3.4 MiB at
        // K = 768), else 6 -- measured against 3 / 4 / 12 on the path's shapes (profiles/r01_nt_col_group.log: -3..5 %)
        const int tiles_n = (int)((d.N + 255) / 256);
        const int g_nt_col_group = (d.launch_flags >> 16) & 0xf;
        a.col_group = g_nt_col_group > 0 ? g_nt_col_group : (tiles_n <= 9 ? tiles_n : 6);
    }
    a.has_drop = d.dropout_p > 0.f;
    a.drop = make_drop(d.dropout_p, d.dropout_seed, d.dropout_salt, rows);
    a.no_persist = (d.launch_flags & M3AE_GEMM_NO_PERSISTENT) ? 1 : 0;
    a.nt_variant = ((d.launch_flags >> 8) & 0xf) - 1;
    a.b_tiled = (d.launch_flags & M3AE_GEMM_B_TILED) ? 1 : 0;
    a.st_policy = (d.launch_flags >> 20) & 0x3;
    // by shape: outputs of 32 MB and more (the image-side GEMMs: 113-900 MB at per-GPU batch 256) are written -- and their residual /
    // derivative operands read -- with the streaming policy: with the default one they evict the weight panel and the activation rows
    // the XCD's other tiles are about to read (-5.2 % over the step's shapes, profiles/r04_nt_store_cache_policy_ab.log); small
    // outputs (the text stream) keep the default: the next kernel finds them in L2 / Infinity Cache
    if (a.st_policy == 0) a.st_policy = (d.M * d.N >= (int64_t)16 << 20) ? 3 : 1;
    const bool has_act = d.act != M3AE_ACT_NONE, has_dact = d.dact_aux != nullptr;
    if (!has_act && !has_dact && !d.preact) return launch_nt_v<EPI_PLAIN>(a, s);
    if (!has_dact && d.act == M3AE_ACT_RELU) return launch_nt_v<EPI_RELU>(a, s);                       // dropout allowed
    // (the derivative classes store no preact: a descriptor that asks for one takes EPI_ANY)
    if (!has_act && has_dact && !d.preact && d.dact == M3AE_ACT_MULAUX) return launch_nt_v<EPI_DMUL>(a, s);   // dropout allowed
    if (a.has_drop) return launch_nt_v<EPI_ANY>(a, s);
    if (!has_dact && d.act == M3AE_ACT_GELU) return launch_nt_v<EPI_GELU>(a, s);
    if (!has_dact && d.act == M3AE_ACT_QUICKGELU) return launch_nt_v<EPI_QGELU>(a, s);
    if (!has_act && !d.preact && d.dact == M3AE_ACT_GELU) return launch_nt_v<EPI_DGELU>(a, s);
    if (!has_act && !d.preact && d.dact == M3AE_ACT_QUICKGELU) return launch_nt_v<EPI_DQGELU>(a, s);
    return launch_nt_v<EPI_ANY>(a, s);
}


// ---------------------------------------------------------------------------------------------------------
// TN "ping-pong" kernel (wgrad): the structure of gemm_nt_pp_kernel with transposing fragment reads -- the two-phase schedule of
// pp_ring.h (ring safety and the counted-wait rule there), written out.  256 x 256 output tile, 8 waves (2 x 4, 128 x 64 each),
// 32 reduction rows per chunk ([32][256] bf16 image of each operand, 16 KiB) in a 4-slot ring; two phases per chunk (output rows
// 0-63 / 64-127 of the wave), the two wave rows staggered by one barrier.  Split over the reduction
// with fp32 atomics; the bias gradient rides on a ones-fragment MFMA in the first column tile's waves.
// Ring depth: a 5-slot ring (160 KiB, three chunks in flight behind the one awaited) measured the same as 4 slots on every
// wgrad shape of the step (r02, profiles/r02_tn_ring_depth.log): the kernel is not waiting on load latency.  An L2 prefetch
// of chunk c + 4 / 8 / 16 (one 4-byte LDS-DMA per 64-B segment, one instruction per wave and chunk) made every shape 9 %
// SLOWER (profiles/r02_tn_l2_prefetch.log): one more LDS-DMA instruction per wave and chunk (5 instead of 4) costs ~240
// clocks of the chunk -- what bounds the loop is the issue of the DMA instructions themselves (in-loop stamps,
// tools/tn_trace.py: a wave row's "fragment reads + 2 DMA issues" phase takes 650-1000 clocks against 420 for the other
// row's 16 MFMAs).  Moving the two DMA issues of a phase INTO the wave's own MFMA cluster (after its first 4 MFMAs) is 10 %
// slower again (profiles/r02_tn_dma_in_mfma.log): a 1-KiB piece costs its wave ~250 clocks wherever it is issued while
// eight waves stage 32 KiB per chunk -- ~30 B / clk / CU of LDS-DMA issue, the same ceiling the fused cross-attention
// kernels run into.  Starting the tiles that share an operand panel apart in time (so that the later ones
// find the panel's lines in L2) changes nothing either: up to 11 us of skew is caught up within the launch, then the tiles
// run in step again (profiles/r02_tn_stagger.log).  Nor does the length of the contiguous global runs of a piece: rotating a
// row by tn_swz(row) slots instead of XOR-permuting its 16-B chunks (same bank-conflict freedom, 288-480-B runs instead of
// 32-B pairs) measured 825 / 868 / 854 / 726 TFLOP/s against 826-834 / 868-882 / 860-863 / 735 on the four wgrad shapes.
// And staging through REGISTERS instead of LDS-DMA (global_load_dwordx4 in iteration c, ds_write_b128 in c + 1, 16 staging
// registers per wave -- all the kernel has left) is 4 % slower: 784 / 825-834 / 808-811 / 707-714 against 818 / 857-863 /
// 849-853 / 732-736 (bit-identical results).  For calibration: torch.matmul (hipBLASLt) runs these four wgrad shapes at
// 699 / 721 / 550 / 347 TFLOP/s on the same box (tools/vendor_gemm_ref.py, profiles/r02_vendor_gemm_reference.log).
// ---------------------------------------------------------------------------------------------------------
#ifdef M3AE_TN_TRACE   // diagnostic build only: in-loop stamps of one chunk of the TN ping-pong kernel
__device__ uint64_t g_tn_trace[512 * 2 * 16];
#define TN_STAMP(k) do { if (tn_tr) g_tn_trace[((size_t)blockIdx.x * 2 + wr) * 16 + (k)] = __builtin_readcyclecounter(); } while (0)
extern "C" int m3ae_tn_trace_dump(uint64_t* out) {
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tn_trace), sizeof(uint64_t) * 512 * 2 * 16);
    static uint64_t zeros[512 * 2 * 16];
    hipMemcpyToSymbol(HIP_SYMBOL(g_tn_trace), zeros, sizeof(zeros));
    return 0;
}
#else
#define TN_STAMP(k) do { } while (0)
#endif
template <bool DET>   // DET: partial planes instead of atomics, see gemm_tn_bf16_kernel
__global__ __launch_bounds__(512, 2) void gemm_tn_pp_kernel(MfmaArgs a) {
    constexpr int CK = 32, NW = 8, A_BYTES = 256 * CK * 2, SLOT = 2 * A_BYTES;
    constexpr int DEPTH = 3, G = 4;   // chunks requested ahead; LDS-DMA pieces per wave and chunk (pp_ring.h)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    const unsigned tiles_n = (unsigned)(a.N / 256);
    const unsigned tiles = (unsigned)(a.M / 256) * tiles_n;
    const unsigned wg = xcd_remap(blockIdx.x, gridDim.x);
    const unsigned tile_id = wg % tiles, split = wg / tiles;
    const int64_t m0 = (int64_t)(tile_id / tiles_n) * 256;
    const int64_t n0 = (int64_t)(tile_id % tiles_n) * 256;
    const int64_t r_begin = (int64_t)split * a.k_chunk;
    int64_t r_end = r_begin + a.k_chunk;
    if (r_end > a.K) r_end = a.K;
    if (r_begin >= r_end) return;  // whole workgroup: uniform
    const int nc = (int)((r_end - r_begin + CK - 1) / CK);

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool do_rowsum = a.a_rowsum != nullptr && n0 == 0 && wc == 0;
    f32x4 rsum[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) rsum[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const s16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c < nc) {
            const int64_t r0 = r_begin + (int64_t)c * CK;
            tn_stage<256, 2, NW>(a.B, a.ldb, r0, r_end, n0, smem + c * SLOT + A_BYTES, wave, lane);
            tn_stage<256, 2, NW>(a.A, a.lda, r0, r_end, m0, smem + c * SLOT, wave, lane);
        }
    }
    wait_vm_chunks<G, DEPTH - 1>(pp_inflight_prologue<DEPTH>(nc));
    PP_FENCE();
    __builtin_amdgcn_s_barrier();
    PP_FENCE();
    if (wr == 1) { __builtin_amdgcn_s_barrier(); PP_FENCE(); }

    for (int c = 0; c < nc; ++c) {
#ifdef M3AE_TN_TRACE
        const bool tn_tr = (c == 64 || c == 65) && lane == 0 && wc == 0 && blockIdx.x < 512;
        if (tn_tr && c == 65) g_tn_trace[((size_t)blockIdx.x * 2 + wr) * 16 + 8] = __builtin_readcyclecounter();
#undef TN_STAMP
#define TN_STAMP(k) do { if (tn_tr && c == 64) g_tn_trace[((size_t)blockIdx.x * 2 + wr) * 16 + (k)] = __builtin_readcyclecounter(); } while (0)
#endif
        TN_STAMP(0);
        const char* At = smem + (c & 3) * SLOT;
        const char* Bt = At + A_BYTES;
        char* nxt = smem + ((c + 3) & 3) * SLOT;
        const bool more = c + 3 < nc;
        const int64_t r3 = r_begin + (int64_t)(c + 3) * CK;
        s16x8 bfr[4], af[4];
        // ---------------- phase 2c: output rows 0..63 of the wave's sub-tile
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = tn_frag<256>(Bt, 0, wc * 64 + j * 16, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = tn_frag<256>(At, 0, wr * 128 + i * 16, lane);
        if (more) tn_stage<256, 2, NW>(a.B, a.ldb, r3, r_end, n0, nxt + A_BYTES, wave, lane);
        PP_FENCE();
        TN_STAMP(1);
        __builtin_amdgcn_s_barrier();
        PP_FENCE();
        TN_STAMP(2);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, bfr[j]), acc[i][j], 0, 0, 0);
        }
        if (do_rowsum) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                rsum[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, ones), rsum[i], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        PP_FENCE();
        TN_STAMP(3);
        __builtin_amdgcn_s_barrier();
        PP_FENCE();
        TN_STAMP(4);
        // ---------------- phase 2c + 1: output rows 64..127 (the B fragments stay in registers)
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = tn_frag<256>(At, 0, wr * 128 + 64 + i * 16, lane);
        if (more) tn_stage<256, 2, NW>(a.A, a.lda, r3, r_end, m0, nxt, wave, lane);
        wait_vm_chunks<G, DEPTH - 1>(pp_inflight_next<DEPTH>(nc, c));   // chunk c + 1 must have landed before the next phase
        PP_FENCE();
        TN_STAMP(5);
        __builtin_amdgcn_s_barrier();
        PP_FENCE();
        TN_STAMP(6);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, bfr[j]), acc[4 + i][j], 0, 0, 0);
        }
        if (do_rowsum) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                rsum[4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    __builtin_bit_cast(bf16x8_t, af[i]), __builtin_bit_cast(bf16x8_t, ones), rsum[4 + i], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        PP_FENCE();
        __builtin_amdgcn_s_barrier();
        PP_FENCE();
    }
    if (wr == 0) { __builtin_amdgcn_s_barrier(); PP_FENCE(); }   // re-align; the ring is free (pp_ring.h)

    if constexpr (DET) {
        if (do_rowsum && (lane & 15) == 0) {
            float* rs = a.a_rowsum + (int64_t)split * a.M + m0 + wr * 128 + 4 * (lane >> 4);
#pragma unroll
            for (int i = 0; i < 8; ++i) *(f32x4*)(rs + i * 16) = rsum[i];
        }
        float* P = (float*)a.C + ((int64_t)split * tiles + tile_id) * (256 * 256) + ((int64_t)wave * 8 * 4 * 64 + lane) * 4;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) *(f32x4*)(P + (i * 4 + j) * 256) = acc[i][j];
        return;
    }
    if (do_rowsum && (lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) atomicAdd(a.a_rowsum + m0 + wr * 128 + i * 16 + 4 * (lane >> 4) + r, rsum[i][r]);
    }
    // lane holds D[n1 = .. + 4 * (lane >> 4) + reg][n2 = .. + (lane & 15)]
    float* C = (float*)a.C;
    const bool atomic = a.splits > 1;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t n1 = m0 + wr * 128 + i * 16 + 4 * (lane >> 4) + r;
                const int64_t n2 = n0 + wc * 64 + j * 16 + (lane & 15);
                float* p = C + n1 * a.ldc + n2;
                const float x = acc[i][j][r] * a.alpha;
#ifdef M3AE_EXP_TN_NOATOMIC   // timing experiment: the split-K epilogue's share of the kernel
                asm volatile("" ::"v"(x), "v"(p));
#else
                if (atomic) atomicAdd(p, x);
                else if (a.accumulate) *p += x;
                else *p = x;
#endif
            }
}

// Deterministic mode: fold the partial planes the DET kernels wrote (accumulator order, see gemm_tn_bf16_kernel) into C in
// ASCENDING SPLIT ORDER, one thread per accumulator quad (16 B per lane and plane, consecutive lanes consecutive bytes), and
// the partial a_rowsum rows into a_rowsum:  C (+)= alpha * (((p_0 + p_1) + p_2) + ...).  One writer per output element.
__global__ __launch_bounds__(256) void tn_det_fold_kernel(const float* __restrict__ part, const float* __restrict__ rs_part,
                                                          float* __restrict__ C, float* __restrict__ rowsum, int64_t ldc,
                                                          int64_t M, int64_t N, int splits, int bm, int wm, float alpha,
                                                          int accumulate) {
    const int64_t plane = M * N, quads = plane / 4;
    const int waves_n = bm / 64, mi = wm / 16;           // square tiles: bm x bm, one wm x 64 sub-tile per wave
    const int64_t tile_quads = (int64_t)bm * bm / 4, tiles_n = N / bm;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < quads; e += stride) {
        f32x4 v = *(const f32x4*)(part + e * 4);
#pragma unroll 4
        for (int sp = 1; sp < splits; ++sp) {
            const f32x4 p = *(const f32x4*)(part + sp * plane + e * 4);
            v[0] += p[0]; v[1] += p[1]; v[2] += p[2]; v[3] += p[3];
        }
        const int64_t tile = e / tile_quads;
        const int w = (int)(e - tile * tile_quads);
        const int lane = w & 63, j = (w >> 6) & 3, i = (w >> 8) % mi, wave = (w >> 8) / mi;
        const int64_t n1 = (tile / tiles_n) * bm + (wave / waves_n) * wm + i * 16 + 4 * (lane >> 4);
        const int64_t n2 = (tile % tiles_n) * bm + (wave % waves_n) * 64 + j * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float* p = C + (n1 + r) * ldc + n2;
            *p = accumulate ? *p + v[r] * alpha : v[r] * alpha;
        }
    }
    if (rowsum) {
        for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += stride) {
            float t = rs_part[m];
            for (int sp = 1; sp < splits; ++sp) t += rs_part[sp * M + m];
            rowsum[m] += t;
        }
    }
}

// split-K fan-out of the 256 x 256 ping-pong TN kernel
static int64_t tn_pp_splits(const m3ae_gemm_desc& d, int64_t* k_chunk) {
    const int64_t tiles = (d.M / 256) * (d.N / 256);
    const int64_t ksteps = cdiv(d.K, 64);
    int64_t splits = 256 / tiles;  // one workgroup per CU, one round
    if (splits > ksteps / 8) splits = ksteps / 8;
    if (splits < 1) splits = 1;
    if (!d.accumulate) splits = 1;
    const int64_t steps_per = cdiv(ksteps, splits);
    *k_chunk = steps_per * 64;
    return cdiv(ksteps, steps_per);
}

// the partial planes of a deterministic call: [splits][M * N] accumulators, then [splits][M] a_rowsum rows
static int64_t tn_det_bytes(const m3ae_gemm_desc& d, int64_t splits) { return splits * (d.M * d.N + d.M) * (int64_t)sizeof(float); }

static int tn_det_fold(const MfmaArgs& part, const m3ae_gemm_desc& d, int bm, int wm, hipStream_t s) {
    int64_t grid = cdiv(d.M * d.N / 4, 256);
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(tn_det_fold_kernel, dim3((unsigned)grid), dim3(256), 0, s, (const float*)part.C, part.a_rowsum, (float*)d.C,
                       d.a_rowsum, d.c_sm, d.M, d.N, part.splits, bm, wm, d.alpha, d.accumulate);
    return hip_launch_status();
}

// Launch one TN kernel instance over grid = tiles * splits workgroups.  det_ws != nullptr (KERNEL is then a DET instance):
// deterministic mode, the kernel writes its partial planes into the caller's workspace of tn_det_bytes(d, a.splits) bytes and
// tn_det_fold sums them into C and a_rowsum.
template <void (*KERNEL)(MfmaArgs)>
static int tn_run(MfmaArgs a, const m3ae_gemm_desc& d, int64_t grid, int threads, int lds, int bm, int wm, float* det_ws,
                  hipStream_t s) {
    if (det_ws) {
        a.C = det_ws;
        a.a_rowsum = d.a_rowsum ? det_ws + a.splits * d.M * d.N : nullptr;
    }
    const int rc = launch_dyn<KERNEL>(dim3((unsigned)grid), dim3(threads), lds, s, a);
    return rc || !det_ws ? rc : tn_det_fold(a, d, bm, wm, s);
}

static int launch_tn_pp(MfmaArgs a, const m3ae_gemm_desc& d, hipStream_t s, float* det_ws = nullptr) {
    constexpr int lds = 4 * (256 + 256) * 32 * 2;
    const int64_t tiles = (d.M / 256) * (d.N / 256);
    const int64_t splits = tn_pp_splits(d, &a.k_chunk);
    a.splits = (int)splits;
    if (det_ws) return tn_run<gemm_tn_pp_kernel<true>>(a, d, tiles * splits, 512, lds, 256, 128, det_ws, s);
    return tn_run<gemm_tn_pp_kernel<false>>(a, d, tiles * splits, 512, lds, 256, 128, nullptr, s);
}

// LDS bytes of the 128 x 128 TN kernels: an NST-deep ring of BKR-row bf16 slices of both operand tiles
constexpr int tn_t_lds(int nst, int bkr) { return nst * (128 + 128) * bkr * 2; }

// split-K fan-out of the 128 x 128 TN kernels (lds = their LDS bytes)
static int64_t tn_t_splits(const m3ae_gemm_desc& d, int lds, int64_t* k_chunk) {
    const int64_t tiles = (d.M / 128) * (d.N / 128);
    const int64_t ksteps = cdiv(d.K, 64);
#ifdef M3AE_EXP_TN_TARGET   // timing experiment: split-K fan-out of the 128 x 128 kernel (workgroups per launch)
    const int64_t target = M3AE_EXP_TN_TARGET;
#else
    // workgroups in flight: 1 or ~3 per CU; a 768 x 768 output (36 tiles) is bound by its splits' fp32 atomic tiles, not by
    // parallelism: 10-14 splits instead of 17-21 measured -10..17 % at 18464 / 36928 rows (profiles/r04_tn_split_fanout_small_batch.log)
    // (long reductions keep the full fan-out: their atomics are a small share and 3 workgroups per CU balance better)
    const int64_t target = lds > 65536 ? 256 : (tiles <= 48 && ksteps <= 1024 ? 448 : 768);
#endif
    // >= 1024 reduction rows per split (K = 8192, 768 x 768: 42 -> 31.5 us).  Shorter splits on the short reductions of the text
    // stream at small per-GPU batches (1024-4096 rows) were measured in round 3 and LOSE: 256 rows per split took 37-43 us against
    // 24-32 us (profiles/r03_tn_small_batch.log): the extra workgroups' atomic tiles cost more than the parallelism buys
    constexpr int64_t min_steps = 16;
    int64_t splits = target / tiles;
    if (splits > ksteps / min_steps) splits = ksteps / min_steps;
    if (splits < 1) splits = 1;
    if (!d.accumulate) splits = 1;
    const int64_t steps_per = cdiv(ksteps, splits);
    *k_chunk = steps_per * 64;
    return cdiv(ksteps, steps_per);
}

template <int BM_, int BN_, int WM, int BKR, int NST>
static int launch_tn_t(MfmaArgs a, const m3ae_gemm_desc& d, hipStream_t s, float* det_ws = nullptr) {
    static_assert(BM_ == 128 && BN_ == 128, "tn_t_splits and tn_det_fold assume the 128 x 128 tile");
    constexpr int lds = tn_t_lds(NST, BKR);
    constexpr int threads = (BM_ / WM) * (BN_ / 64) * 64;
    const int64_t tiles = (d.M / BM_) * (d.N / BN_);
    const int64_t splits = tn_t_splits(d, lds, &a.k_chunk);
    a.splits = (int)splits;
    if (det_ws) return tn_run<gemm_tn_bf16_kernel<BM_, BN_, WM, BKR, NST, true>>(a, d, tiles * splits, threads, lds, BM_, WM, det_ws, s);
    return tn_run<gemm_tn_bf16_kernel<BM_, BN_, WM, BKR, NST>>(a, d, tiles * splits, threads, lds, BM_, WM, nullptr, s);
}

// which TN kernel a descriptor takes: 5 = 256 x 256 ping-pong, 2 = 128 x 128 with 32-row steps, 0 = with 64-row steps
static int tn_kernel_choice(const m3ae_gemm_desc& d) {
    // variant 1: 256x256 tile, 8 waves x (128x64): half the operand re-read traffic of the 128x128 tile
    const bool pp_ok = d.M % 256 == 0 && d.N % 256 == 0 && d.K >= 4096;
    const int g_tn_variant = ((d.launch_flags >> 12) & 0xf) - 1;
    if (g_tn_variant == 5 && pp_ok) return 5;
    if (g_tn_variant < 0 || g_tn_variant == 6) {
        // auto (default).  Re-measured in round 4 after both kernels' LDS-DMA moved to inline asm (mfma_tiles.h: the 128 x 128 kernel
        // gained as much as the ping-pong one): the 256 x 256 ping-pong kernel wins on the 768 x 3072 / 3072 x 768 outputs from 65536
        // reduction rows (+3..4 % at 110784-147712, equal at 73856) and nowhere else -- 2304 x 768 and 768 x 768 are equal at
        // 147712 and 5-15 % SLOWER on it at 36928-110784, the large outputs 8 % slower at 36928
        // (profiles/r04_tn_kernel_choice_by_batch.log).  Variant 6 = the rule of rounds 1-3, kept for A/B runs.
        const bool r3_rule = pp_ok && (d.K >= 65536 || (d.K >= 32768 && d.M * d.N >= 768 * 3072));
        const bool r4_rule = pp_ok && d.K >= 65536 && d.M * d.N >= 768 * 3072;
        if (g_tn_variant == 6 ? r3_rule : r4_rule) return 5;
        return 2;
    }
    if (g_tn_variant == 2) return 2;  // 32 KiB LDS: 3 workgroups / CU
    return 0;
}

static int launch_tn(const m3ae_gemm_desc& d, hipStream_t s, float* det_ws = nullptr) {
    // C[M=N1][N=N2] += alpha * sum_k A[m][k] B[k][n] with a_sm == 1 (A stored [K][N1]) and b_sn == 1
    MfmaArgs a{};
    a.A = (const bf16_t*)d.A; a.lda = d.a_sk;
    a.B = (const bf16_t*)d.B; a.ldb = d.b_sk;
    a.C = d.C; a.ldc = d.c_sm;
    a.M = d.M; a.N = d.N; a.K = d.K;
    a.c_f32 = 1; a.alpha = d.alpha; a.accumulate = d.accumulate; a.a_rowsum = d.a_rowsum;
    const int k = tn_kernel_choice(d);
    if (k == 5) return launch_tn_pp(a, d, s, det_ws);
    if (k == 2) return launch_tn_t<128, 128, 64, 32, 2>(a, d, s, det_ws);
    return launch_tn_t<128, 128, 64, 64, 2>(a, d, s, det_ws);
}


// The routing rule, in one place: which kernel family takes a descriptor.  m3ae_gemm dispatches on it; deterministic mode
// (m3ae_gemm_det, m3ae_gemm_det_workspace_bytes) asks it whether the descriptor is one of the split-K TN family, the only one
// with several writers per output element.  Pointers are looked at for alignment only, so a size query with null operands and
// no device classifies like the call it precedes.
enum GemmRoute { ROUTE_BAD_DIMS, ROUTE_F32X3, ROUTE_NT, ROUTE_TN, ROUTE_GENERIC };
static GemmRoute gemm_route(const m3ae_gemm_desc& d) {
    if (d.M <= 0 || d.N <= 0 || d.K <= 0 || d.batch1 <= 0 || d.batch2 <= 0) return ROUTE_BAD_DIMS;
    if ((d.launch_flags & M3AE_GEMM_F32_X3) && !d.force_generic) return ROUTE_F32X3;   // fp32x3 mode (csrc/gemm_f32x3.hip)
    const bool bf = d.dtype_a == M3AE_BF16 && d.dtype_b == M3AE_BF16;
    const bool single = d.batch1 == 1 && d.batch2 == 1;
    if (bf && single && !d.force_generic && d.c_sn == 1) {
        const bool ptr_ok = aligned16(d.A) && aligned16(d.B) && aligned16(d.C) &&
                            (!d.preact || aligned16(d.preact)) && (!d.residual || aligned16(d.residual)) &&
                            (!d.dact_aux || aligned16(d.dact_aux)) && (!d.bias || aligned16(d.bias));
        // NT: both operands K-contiguous
        if (ptr_ok && !d.a_rowsum && d.a_sk == 1 && d.b_sk == 1 && d.K % BK == 0 && d.N % 4 == 0 && d.a_sm % 8 == 0 &&
            d.b_sn % 8 == 0 && d.c_sm % 4 == 0)
            return ROUTE_NT;
        // TN: both operands reduction-strided (wgrad), fp32 output
        if (ptr_ok && d.a_sm == 1 && d.b_sn == 1 && d.dtype_c == M3AE_F32 && d.M % BM == 0 && d.N % BN == 0 &&
            d.a_sk % 8 == 0 && d.b_sk % 8 == 0 && !d.bias && d.act == M3AE_ACT_NONE && !d.preact && !d.residual &&
            !d.dact_aux)
            return ROUTE_TN;
    }
    return ROUTE_GENERIC;
}

extern "C" int m3ae_gemm(const m3ae_gemm_desc* dp, void* stream) { return m3ae_gemm_rows(dp, 0, 1, stream); }

extern "C" int m3ae_gemm_rows(const m3ae_gemm_desc* dp, int64_t row_base, int64_t row_step, void* stream) {
    if (!dp || !dp->A || !dp->B || !dp->C) return M3AE_ERR_ARG;
    const m3ae_gemm_desc& d = *dp;
    const GemmRoute route = gemm_route(d);
    if (route == ROUTE_BAD_DIMS) return M3AE_ERR_ARG;
    const DropRows rows{row_base, row_step};
    if (!drop_rows_ok(rows, d.M, d.N)) return M3AE_ERR_ARG;
    // a_rowsum is one fp32 [M] vector with no batch stride: every batch of a batched call would add into the same rows
    if (d.a_rowsum && (d.batch1 != 1 || d.batch2 != 1)) return M3AE_ERR_UNSUPPORTED;
    // the tiled weight copy (tiled_b.h) is defined for one K-contiguous bf16 matrix with K % 32 == 0; the NT and the generic kernels read it
    if ((d.launch_flags & M3AE_GEMM_B_TILED) &&
        (d.dtype_a != M3AE_BF16 || d.dtype_b != M3AE_BF16 || d.b_sk != 1 || d.b_sn != d.K || d.K % 32 != 0 || d.batch1 != 1 ||
         d.batch2 != 1 || (d.launch_flags & M3AE_GEMM_F32_X3) || !aligned16(d.B)))
        return M3AE_ERR_UNSUPPORTED;
    // the split-K wgrad kernels have no dropout site: a mapped call that asks for one is refused, not run without it
    if (route == ROUTE_TN && d.dropout_p > 0.f && (row_base != 0 || row_step != 1)) return M3AE_ERR_UNSUPPORTED;
    // deterministic mode needs a workspace for its partial planes: m3ae_gemm_det takes one, this call cannot, and it never
    // runs the atomic kernels under that flag
    if (d.launch_flags & M3AE_GEMM_DETERMINISTIC) return M3AE_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    switch (route) {
    case ROUTE_F32X3:   // fp32 operands only
        if (d.dtype_a != M3AE_F32 || d.dtype_b != M3AE_F32 || d.dtype_c != M3AE_F32) return M3AE_ERR_UNSUPPORTED;
        g_last_path = "f32x3";
        return m3ae_gemm_f32x3(d, s, rows);
    case ROUTE_NT:
        return launch_nt(d, s, rows);   // (launch_nt_v names the path)
    case ROUTE_TN:
        g_last_path = "mfma_tn";
        return launch_tn(d, s);
    default:
        g_last_path = "generic";
        return m3ae_gemm_generic(d, s, rows);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Deterministic mode (M3AE_GEMM_DETERMINISTIC): the TN kernels with ordered split-K.
// ---------------------------------------------------------------------------------------------------------
extern "C" int64_t m3ae_gemm_det_workspace_bytes(const m3ae_gemm_desc* dp) {
    if (!dp) return M3AE_ERR_ARG;
    const m3ae_gemm_desc& d = *dp;
    if (gemm_route(d) != ROUTE_TN) return 0;   // every other kernel family has one writer per output element already
    int64_t k_chunk = 0;
    const int k = tn_kernel_choice(d);
    const int64_t splits = k == 5 ? tn_pp_splits(d, &k_chunk) : tn_t_splits(d, tn_t_lds(2, k == 2 ? 32 : 64), &k_chunk);
    return tn_det_bytes(d, splits);
}

extern "C" int m3ae_gemm_det(const m3ae_gemm_desc* dp, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!dp || !dp->A || !dp->B || !dp->C) return M3AE_ERR_ARG;
    const m3ae_gemm_desc& d = *dp;
    if (!(d.launch_flags & M3AE_GEMM_DETERMINISTIC)) return M3AE_ERR_ARG;
    if (d.launch_flags & M3AE_GEMM_B_TILED) return M3AE_ERR_UNSUPPORTED;   // the wgrad family's B is reduction-strided
    if (gemm_route(d) != ROUTE_TN) return M3AE_ERR_UNSUPPORTED;   // (such a descriptor needs no ordered form: plain m3ae_gemm, flag clear)
    if (!workspace || !aligned16(workspace) || workspace_bytes < m3ae_gemm_det_workspace_bytes(dp)) return M3AE_ERR_WORKSPACE;
    g_last_path = "mfma_tn";
    return launch_tn(d, (hipStream_t)stream, (float*)workspace);
}
