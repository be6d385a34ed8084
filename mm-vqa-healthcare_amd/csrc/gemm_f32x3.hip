// fp32-accurate GEMM on the bf16 matrix cores ("fp32x3" mode, m3ae_gemm_desc.launch_flags & M3AE_GEMM_F32_X3).
//
// gfx950 has no xf32 MFMA and its exact-fp32 MFMA runs at 1/16 of the bf16 rate.  Every fp32 operand element is split
// once, when it is staged, into two bf16 parts:
//     x = hi + lo + r,   hi = bf16_rne(x),   lo = bf16_rne(x - hi)   (x - hi is exact in fp32),   |r| <= 2^-16 |x|
// and each product is a_hi b_hi + a_hi b_lo + a_lo b_hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: three bf16
// MFMAs per k-step.  The dropped terms (a_lo b_lo, and the r parts) are below 3 * 2^-16 |a b|.  All three products go into ONE
// accumulator, cross terms first: per 32-wide k-step that is three fp32 roundings of the running sum instead of one, i.e. a
// worst-case accumulation bound of 3K * 2^-24 sum|a b| against K * 2^-24 with a second accumulator.  The first is still inside
// the budget the mode is held to (3 (2^-16 + K 2^-23) |A||B|, tests/test_gpu_f32x3.py) at every K the model issues, and the
// second accumulator would cost 64 more VGPRs per lane (two waves per SIMD no longer fit next to the staging registers).
//
// Tile: 128 x 128 x 32 per workgroup, four waves in 2 x 2, each wave 64 x 64 = 4 x 4 MFMA tiles of 16 x 16.  Operands are
// loaded fp32 global -> registers (issued before the MFMAs of the previous k-step), split, and written as hi / lo bf16 planes
// [128 rows][32 k] into a double-buffered LDS image in the K-contiguous swizzled layout of the NT kernels (mfma_tiles.h nt_swz):
// the transpose for operands whose rows are contiguous (dgrad's B, wgrad's A and B, P^T of the attention) happens at that LDS
// store, so one kernel covers NT, NN, TN and the batched strided products.  Ragged M / N / K are predicated (zero fill); vector
// loads are taken where the host has proven the alignment.
//
// The epilogue (from an LDS image of the accumulator tile) is gemm_generic_kernel's, element for element (alpha, bias, preact store, act, dropout with the mask index
// gm * drop_ld(N) + gn, residual, dact_aux, accumulate), so the two kernels differ only in how the dot products are formed.
// a_rowsum sums the fp32 A values (not hi + lo): the workgroups of the first column tile keep per-thread partial sums of the
// values they stage and reduce them in a fixed order.
#include "common.h"
#include "mfma_tiles.h"

namespace {

constexpr int X3_BM = 128, X3_BN = 128, X3_BK = 32;
constexpr int X3_PLANE = X3_BM * X3_BK * 2;   // one bf16 plane [128][32]: 8 KiB
constexpr int X3_STAGE = 4 * X3_PLANE;        // A hi, A lo, B hi, B lo
enum { X3_KFAST = 0, X3_RFAST = 1 };          // operand layout in global memory: k contiguous, or rows (m / n) contiguous

struct X3Operand {
    const float* p;
    int64_t s_r, s_k;   // element strides along the tile row (m for A, n for B) and along k
    int64_t rows;       // M or N
    int vec;            // 16-B loads are aligned wherever a whole float4 lies in range (checked by the host)
};

DEVINL f32x4 ld4_pred(const X3Operand& o, int64_t r, int64_t k, int64_t K, int64_t dr, int64_t dk, bool full) {
    // four elements (r, k) + e * (dr, dk), e = 0..3; out of range -> 0
    if (full && o.vec) return *(const f32x4*)(o.p + r * o.s_r + k * o.s_k);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t re = r + e * dr, ke = k + e * dk;
        v[e] = (re < o.rows && ke < K) ? o.p[re * o.s_r + ke * o.s_k] : 0.f;
    }
    return v;
}

// hi / lo bf16 pair of two fp32 values, packed (element 0 in bits 0..15)
DEVINL void split2(float x0, float x1, uint32_t& hi, uint32_t& lo) {
    hi = pack2bf(x0, x1);
    float r0 = x0 - __uint_as_float(hi << 16), r1 = x1 - __uint_as_float(hi & 0xffff0000u);
    // an infinite hi leaves inf - inf = NaN: the product is already +-inf through hi
    r0 = fabsf(r0) <= 3.0e38f ? r0 : 0.f;
    r1 = fabsf(r1) <= 3.0e38f ? r1 : 0.f;
    lo = pack2bf(r0, r1);
}

DEVINL int x3_off(int row, int k) {   // byte offset of (row, k) in a [128][32] bf16 plane, nt_swz<32> chunk order
    return row * (X3_BK * 2) + (((k >> 3) ^ nt_swz<X3_BK>(row)) << 4) + (k & 7) * 2;
}

// Per thread 16 staged values: KFAST: 4 float4 along k (rows (t >> 3) + 32 i, k quad t & 7);
//                              RFAST: 2 x 2 float4 along rows (rows 4 (t & 31) .. + 3, k pair (t >> 5) + 8 i).
// Both mappings give a thread 4 fixed rows in every k-step (a_rowsum) and coalesce along the contiguous index.
template <int MODE>
DEVINL void x3_load(const X3Operand& o, int64_t row0, int64_t k0, int64_t K, int t, f32x4 (&v)[4]) {
    if (MODE == X3_KFAST) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t r = row0 + (t >> 3) + 32 * i, k = k0 + (t & 7) * 4;
            v[i] = ld4_pred(o, r, k, K, 0, 1, r < o.rows && k + 3 < K);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t r = row0 + 4 * (t & 31), k = k0 + 2 * ((t >> 5) + 8 * i);
            v[2 * i] = ld4_pred(o, r, k, K, 1, 0, r + 3 < o.rows && k < K);
            v[2 * i + 1] = ld4_pred(o, r, k + 1, K, 1, 0, r + 3 < o.rows && k + 1 < K);
        }
    }
}

template <int MODE>
DEVINL void x3_store(char* hi_plane, char* lo_plane, int t, const f32x4 (&v)[4]) {
    if (MODE == X3_KFAST) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (t >> 3) + 32 * i, k = (t & 7) * 4;
            uint32_t h0, l0, h1, l1;
            split2(v[i][0], v[i][1], h0, l0);
            split2(v[i][2], v[i][3], h1, l1);
            *(u32x2*)(hi_plane + x3_off(row, k)) = (u32x2){h0, h1};
            *(u32x2*)(lo_plane + x3_off(row, k)) = (u32x2){l0, l1};
        }
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = 2 * ((t >> 5) + 8 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = 4 * (t & 31) + j;
                uint32_t h, l;
                split2(v[2 * i][j], v[2 * i + 1][j], h, l);
                *(uint32_t*)(hi_plane + x3_off(row, k)) = h;
                *(uint32_t*)(lo_plane + x3_off(row, k)) = l;
            }
        }
    }
}

// rows of the thread's 4 rowsum partials and its slot (0..7) among the 8 threads that share them
template <int MODE> DEVINL int x3_rs_row(int t, int j) { return MODE == X3_KFAST ? (t >> 3) + 32 * j : 4 * (t & 31) + j; }
template <int MODE> DEVINL int x3_rs_slot(int t) { return MODE == X3_KFAST ? (t & 7) : (t >> 5); }
template <int MODE> DEVINL void x3_rs_add(float (&rs)[4], const f32x4 (&v)[4]) {
    if (MODE == X3_KFAST) {
#pragma unroll
        for (int i = 0; i < 4; ++i) rs[i] += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) rs[j] += (v[0][j] + v[1][j]) + (v[2][j] + v[3][j]);
    }
}

DEVINL f32x4 mfma16(s16x8 a, s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

template <int AM, int BM>
__global__ __launch_bounds__(256, 2) void gemm_f32x3_kernel(m3ae_gemm_desc d, X3Operand oa, X3Operand ob, int64_t row_base, int64_t row_step) {
    __shared__ __attribute__((aligned(16))) char smem[2 * X3_STAGE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.y * X3_BM, n0 = (int64_t)blockIdx.x * X3_BN;
    const int64_t b1 = blockIdx.z / d.batch2, b2 = blockIdx.z % d.batch2;
    oa.p += b1 * d.a_sb1 + b2 * d.a_sb2;
    ob.p += b1 * d.b_sb1 + b2 * d.b_sb2;
    const int64_t K = d.K;
    const int nk = (int)((K + X3_BK - 1) / X3_BK);
    const bool do_rowsum = d.a_rowsum != nullptr && blockIdx.x == 0;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float rs[4] = {0.f, 0.f, 0.f, 0.f};

    f32x4 va[4], vb[4];
    x3_load<AM>(oa, m0, 0, K, t, va);
    x3_load<BM>(ob, n0, 0, K, t, vb);
    if (do_rowsum) x3_rs_add<AM>(rs, va);
    x3_store<AM>(smem, smem + X3_PLANE, t, va);
    x3_store<BM>(smem + 2 * X3_PLANE, smem + 3 * X3_PLANE, t, vb);
    __syncthreads();

    // fragment byte offsets inside a plane: lane reads 16 B at (row base + (lane & 15), k chunk lane >> 4)
    int offa[4], offb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        offa[i] = nt_frag_off<X3_BK>(wm * 64 + i * 16 + (lane & 15), lane >> 4);
        offb[i] = nt_frag_off<X3_BK>(wn * 64 + i * 16 + (lane & 15), lane >> 4);
    }

    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) {
            x3_load<AM>(oa, m0, (int64_t)(kt + 1) * X3_BK, K, t, va);
            x3_load<BM>(ob, n0, (int64_t)(kt + 1) * X3_BK, K, t, vb);
        }
        const char* st = smem + (kt & 1) * X3_STAGE;
        s16x8 bh[4], bl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bh[j] = nt_frag_at(st + 2 * X3_PLANE, offb[j]);
            bl[j] = nt_frag_at(st + 3 * X3_PLANE, offb[j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {   // cross terms first, then hi * hi (one accumulator, see the top of the file)
            const s16x8 ah = nt_frag_at(st, offa[i]), al = nt_frag_at(st + X3_PLANE, offa[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(ah, bl[j], acc[i][j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(al, bh[j], acc[i][j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(ah, bh[j], acc[i][j]);
        }
        if (more) {
            if (do_rowsum) x3_rs_add<AM>(rs, va);
            char* nx = smem + ((kt + 1) & 1) * X3_STAGE;
            x3_store<AM>(nx, nx + X3_PLANE, t, va);
            x3_store<BM>(nx + 2 * X3_PLANE, nx + 3 * X3_PLANE, t, vb);
        }
        __syncthreads();
    }

    if (do_rowsum) {   // 8 partials per row, summed in slot order (deterministic); one writer per row
        float* red = (float*)smem;   // [8][128], free after the last barrier of the loop
#pragma unroll
        for (int j = 0; j < 4; ++j) red[x3_rs_slot<AM>(t) * X3_BM + x3_rs_row<AM>(t, j)] = rs[j];
        __syncthreads();
        if (t < X3_BM) {
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) s += red[q * X3_BM + t];
            if (m0 + t < d.M) d.a_rowsum[m0 + t] += s;
        }
    }

    // accumulators -> LDS [128][128] fp32 (the whole 64 KiB; the 16-column groups of a row are XOR-swizzled by (row >> 2) & 3 so
    // the four 16-lane groups of an MFMA store hit different banks), then the epilogue by rows: consecutive threads own consecutive
    // columns (coalesced loads and stores) and one copy of the activation code serves the 64 elements of a thread
    float* ct = (float*)smem;
    if (do_rowsum) __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {   // 16x16 C/D map: col = lane & 15, row = 4 (lane >> 4) + r
                const int row = wm * 64 + i * 16 + 4 * (lane >> 4) + r, col = wn * 64 + j * 16 + (lane & 15);
                ct[row * X3_BN + (col ^ (((row >> 2) & 3) << 4))] = acc[i][j][r];
            }
    __syncthreads();

    DropState drop = make_drop_dev(d.dropout_p, d.dropout_seed, d.dropout_salt, row_base, row_step);
    drop_resolve(drop);
    const int64_t coff = b1 * d.c_sb1 + b2 * d.c_sb2;
    float* C = (float*)d.C + coff;
    float* P = d.preact ? (float*)d.preact + coff : nullptr;
    const float* R = d.residual ? (const float*)d.residual + coff : nullptr;
    const float* X = d.dact_aux ? (const float*)d.dact_aux + coff : nullptr;
    const int col = t & (X3_BN - 1);
    const int64_t gn = n0 + col;
    if (gn >= d.N) return;
    const float bias = d.bias ? d.bias[gn] : 0.f;
#pragma unroll 2
    for (int row = t >> 7; row < X3_BM; row += 2) {
        const int64_t gm = m0 + row;
        if (gm >= d.M) break;
        const int64_t off = gm * d.c_sm + gn * d.c_sn;
        float x = ct[row * X3_BN + (col ^ (((row >> 2) & 3) << 4))] * d.alpha;
        if (d.bias) x += bias;
        if (P) P[off] = d.preact_grad ? act_bwd(x, d.act) : x;
        x = act_fwd(x, d.act);
        if (d.dropout_p > 0.f) x = drop_apply(drop, (uint64_t)(drop_row(drop, gm) * drop_ld(d.N) + gn), x);
        if (R) x += R[off];
        if (X) x *= act_bwd(X[off], d.dact);
        if (d.accumulate) x += C[off];
        C[off] = x;
    }
}

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// layout of one operand: rows contiguous -> RFAST (transposed at the LDS store), otherwise KFAST (k contiguous, or any strides
// through scalar loads)
X3Operand x3_operand(const void* p, int64_t s_r, int64_t s_k, int64_t rows, int64_t sb1, int64_t sb2, int& mode) {
    X3Operand o{(const float*)p, s_r, s_k, rows, 0};
    mode = (s_k != 1 && s_r == 1) ? X3_RFAST : X3_KFAST;
    const int64_t other = mode == X3_RFAST ? s_k : s_r;   // stride of the non-contiguous index
    const bool unit = mode == X3_RFAST ? true : s_k == 1;
    o.vec = (unit && al16(p) && other % 4 == 0 && sb1 % 4 == 0 && sb2 % 4 == 0) ? 1 : 0;
    return o;
}

template <int AM, int BM>
int launch_x3(const m3ae_gemm_desc& d, const X3Operand& oa, const X3Operand& ob, hipStream_t s, DropRows rows) {
    dim3 grid((unsigned)cdiv(d.N, X3_BN), (unsigned)cdiv(d.M, X3_BM), (unsigned)(d.batch1 * d.batch2));
    hipLaunchKernelGGL((gemm_f32x3_kernel<AM, BM>), grid, dim3(256), 0, s, d, oa, ob, rows.base, rows.step);
    return hip_launch_status();
}

}  // namespace

int m3ae_gemm_f32x3(const m3ae_gemm_desc& d, hipStream_t s, DropRows rows) {
    if (d.dtype_a != M3AE_F32 || d.dtype_b != M3AE_F32 || d.dtype_c != M3AE_F32) return M3AE_ERR_UNSUPPORTED;
    if (cdiv(d.M, X3_BM) > 65535 || d.batch1 * d.batch2 > 65535 || cdiv(d.N, X3_BN) > 0x7fffffff) return M3AE_ERR_UNSUPPORTED;
    int am, bm;
    const X3Operand oa = x3_operand(d.A, d.a_sm, d.a_sk, d.M, d.a_sb1, d.a_sb2, am);
    const X3Operand ob = x3_operand(d.B, d.b_sn, d.b_sk, d.N, d.b_sb1, d.b_sb2, bm);
    if (am == X3_KFAST && bm == X3_KFAST) return launch_x3<X3_KFAST, X3_KFAST>(d, oa, ob, s, rows);
    if (am == X3_KFAST && bm == X3_RFAST) return launch_x3<X3_KFAST, X3_RFAST>(d, oa, ob, s, rows);
    if (am == X3_RFAST && bm == X3_KFAST) return launch_x3<X3_RFAST, X3_KFAST>(d, oa, ob, s, rows);
    return launch_x3<X3_RFAST, X3_RFAST>(d, oa, ob, s, rows);
}
