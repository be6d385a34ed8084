// Tiled ("block-major") layout of a K-contiguous bf16 weight W[N][K], K % 32 == 0: the B operand of the NT GEMM kernels under
// M3AE_GEMM_B_TILED.  Written down once; shared by the kernels that read it (gemm_nt_pp2.hip, gemm_mfma.hip, gemm_generic.hip) and
// the kernel that writes it (misc.hip: m3ae_tile_bf16_batched).  Python mirror for the tests: m3ae_amd/tiled_b.py.
//
//   block  = 16 rows x 32 k = 1 KiB = one LDS-DMA piece of the 256 x 256 ping-pong kernels;
//   chunk  = the 16 blocks of rows [256 T, 256 T + 256) x k [32 c, 32 c + 32), consecutive: 16 KiB;
//   tile T = its K / 32 chunks, consecutive along k; tiles follow each other.  N is padded to a multiple of 256 with zero rows
//            (the kernels load rows past the edge and never store their products).
//   Inside a block, 16-B unit u (8 k) of row r sits at unit position u ^ nt_swz<32>(r): the source-side swizzle of the LDS image
//   is part of the layout, so lane i of a piece reads bytes [16 i, 16 i + 16) of its KiB and the LDS image is the one the
//   row-major path builds.
// A 128-row half of a chunk (the 128 x 128 kernel's tile rows) is blocks 8 h .. 8 h + 7 of the chunk: 8 KiB, consecutive.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M3AE_TB_FN __host__ __device__ __forceinline__
#else
#define M3AE_TB_FN static inline
#endif

enum { M3AE_TB_ROWS = 256, M3AE_TB_CK = 32, M3AE_TB_BLOCK_ROWS = 16, M3AE_TB_BLOCK_ELEMS = 512, M3AE_TB_CHUNK_ELEMS = 8192 };

// rows of the padded copy; its size is m3ae_tiled_b_rows(N) * K elements
M3AE_TB_FN int64_t m3ae_tiled_b_rows(int64_t N) { return (N + M3AE_TB_ROWS - 1) / M3AE_TB_ROWS * M3AE_TB_ROWS; }

// element index of W[n][k] in the tiled copy (0 <= n < m3ae_tiled_b_rows(N), 0 <= k < K)
M3AE_TB_FN int64_t m3ae_tiled_b_index(int64_t n, int64_t k, int64_t K) {
    const int64_t T = n >> 8, c = k >> 5;
    const int p = (int)(n >> 4) & 15, r = (int)n & 15, u = (int)(k >> 3) & 3;
    const int swz = (4 - ((r >> 2) & 3)) & 3;   // nt_swz<32>(row): bits 2-3 of the row, the same for n and n & 15
    return (T * (K >> 5) + c) * M3AE_TB_CHUNK_ELEMS + p * M3AE_TB_BLOCK_ELEMS + r * 32 + ((u ^ swz) << 3) + (int)(k & 7);
}
