// Device image transform: Pillow's 8-bit bicubic resize (libImaging/Resample.c) + centre crop + ToTensor / Normalize for a batch
// of decoded sources of any sizes, in two launches.  Both passes are the same fixed-point sum
//     out = clamp((2^21 + sum_t pixel[min + t] * k[t]) >> 22, 0, 255)        int32, arithmetic shift
// with bounds (min, taps) and 22-bit coefficients k per output column / row that the host built in float64 (m3ae_amd/resample.py:
// the tables are data, so no device rounding or contraction can move a coefficient) with the crop folded in.  Integer arithmetic
// has one answer: the bytes are PIL's, and the fp32 output uses image_normalize_u8_kernel's expression (misc.hip) on them.
//
// Pass 1 (horizontal), grid (row blocks, image): a workgroup stages up to RS_ROWS source rows in LDS as one dword per pixel
// (byte loads from the packed RGB rows, any pitch or alignment -> R | G << 8 | B << 16), then one thread per output column runs
// the taps for all staged rows at once: one coefficient load and one ds_read_b32 per row serve three channels.  Writes the uint8
// intermediate [nrows][size][3] (its rounding is part of Pillow's result).
// Pass 2 (vertical), grid (output row blocks, image): threads along the intermediate row's dwords (4 consecutive x * 3 + c bytes:
// contiguous reads), vertical taps, clamp, the row goes to LDS as bytes; then threads along x per channel plane read it back
// and store the normalised planar fp32 row (and the uint8 NHWC row) contiguously.
// Images of different sizes share a launch: blockIdx.y is the image, workgroups beyond an image's extent leave at once.
// Every plan field and table bound is checked against the buffer sizes before it is used as an address: a wrong plan leaves its
// image unwritten instead of reading or writing outside the caller's buffers.
//
// Tables built on the device (train transform "clip_resizedcrop": a random crop box per image and epoch, so every image has its
// own tables and the host's Python loop per output cannot keep up).  resample_tables_kernel restates resample.axis_table --
// Pillow's precompute_coeffs + normalize_coeffs_8bpc -- one float64 operation per source operation, in the source's order, under
// `#pragma clang fp contract(off)`: no multiply-add is fused, division is the IEEE one, conversions truncate.  With every
// operation correctly rounded there is one answer again, and the tables equal the host's bit for bit.  One thread per (image, axis,
// output); the weights are not kept (ksize reaches 149): one loop over the taps sums them, a second recomputes each, divides,
// rounds to 22 bits and stores.
#include "common.h"

namespace {

constexpr int RS_THREADS = 128;     // pass 1: 384 = 3 x 128 and 224 = 2 x 112 output columns
constexpr int RS_LDS_PIX = 8192;    // staged pixels (32 KiB): the widest source row
constexpr int RS_ROWS = 8;          // source rows per workgroup pass (accumulators: 8 rows x 3 channels)
constexpr int RV_THREADS = 256;
constexpr int RV_ROWS = 4;          // output rows per workgroup of pass 2
constexpr int RT_THREADS = 256;     // table build: threads along (axis, output index)
constexpr int PLAN_FIELDS = 16;
constexpr int PLAN_BUILD = 13;      // plan field: this record owns a table set the table kernel writes
constexpr int PREC = 22;

struct Img {
    int64_t src, pitch, irow0;
    int w, h, row0, nrows, ksx, ksy;
    const int32_t *xb, *xk, *yb, *yk;
    bool ok;
};
// plan record of image b -> Img; ok = every extent lies inside the buffers (wave-uniform: the record is read with scalar loads)
DEVINL Img load_plan(const int64_t* plan, int b, int size, int64_t src_bytes, const int32_t* tab, int64_t tab_ints,
                     int64_t ws_rows) {
    const int64_t* p = plan + (int64_t)b * PLAN_FIELDS;
    Img g;
    g.src = p[0]; g.pitch = p[3]; g.irow0 = p[12];
    const int64_t w = p[1], h = p[2], row0 = p[4], nrows = p[5], ksx = p[6], ksy = p[7], xb = p[8], xk = p[9], yb = p[10], yk = p[11];
    g.ok = w > 0 && w <= RS_LDS_PIX && h > 0 && h < (1 << 24) && g.pitch >= 3 * w && g.pitch < ((int64_t)1 << 31) && g.src >= 0 &&
           g.src + (h - 1) * g.pitch + 3 * w <= src_bytes && row0 >= 0 && nrows > 0 && row0 + nrows <= h && ksx > 0 &&
           ksx < (1 << 20) && ksy > 0 && ksy < (1 << 20) && g.irow0 >= 0 && g.irow0 + nrows <= ws_rows && xb >= 0 &&
           xb + 2 * size <= tab_ints && xk >= 0 && xk + size * ksx <= tab_ints && yb >= 0 && yb + 2 * size <= tab_ints && yk >= 0 &&
           yk + size * ksy <= tab_ints;
    g.w = (int)w; g.h = (int)h; g.row0 = (int)row0; g.nrows = (int)nrows; g.ksx = (int)ksx; g.ksy = (int)ksy;
    g.xb = tab + xb; g.xk = tab + xk; g.yb = tab + yb; g.yk = tab + yk;
    return g;
}
DEVINL int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
DEVINL uint32_t clip8(int acc) { return (uint32_t)clamp_i(acc >> PREC, 0, 255); }

__global__ __launch_bounds__(RS_THREADS) void resample_h_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                const int64_t* __restrict__ plan, const int32_t* __restrict__ tab,
                                                                int64_t tab_ints, int size, int ipitch, uint8_t* __restrict__ ws,
                                                                int64_t ws_rows) {
    __shared__ uint32_t pix[RS_LDS_PIX];
    const Img g = load_plan(plan, blockIdx.y, size, src_bytes, tab, tab_ints, ws_rows);
    if (!g.ok) return;
    const int tid = threadIdx.x, w = g.w;
    const int R = RS_LDS_PIX / w < RS_ROWS ? RS_LDS_PIX / w : RS_ROWS;   // >= 1: w <= RS_LDS_PIX
    const int nblk = (g.nrows + R - 1) / R;
    int rowoff[RS_ROWS];   // LDS row of accumulator j; rows beyond R alias the last one (computed, never stored)
#pragma unroll
    for (int j = 0; j < RS_ROWS; ++j) rowoff[j] = (j < R ? j : R - 1) * w;
    for (int rb = blockIdx.x; rb < nblk; rb += gridDim.x) {
        const int r0 = rb * R, nr = g.nrows - r0 < R ? g.nrows - r0 : R;
        __syncthreads();   // the previous block of rows has been read
        for (int r = 0; r < nr; ++r) {
            const uint8_t* row = src + g.src + (int64_t)(g.row0 + r0 + r) * g.pitch;
            for (int x = tid; x < w; x += RS_THREADS) {
                const uint8_t* p = row + 3 * x;
                pix[r * w + x] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            }
        }
        __syncthreads();
        for (int x = tid; x < size; x += RS_THREADS) {
            const int xmin = clamp_i(g.xb[2 * x], 0, w);
            const int lim = w - xmin < g.ksx ? w - xmin : g.ksx;
            const int cnt = clamp_i(g.xb[2 * x + 1], 0, lim);
            const int32_t* k = g.xk + (int64_t)x * g.ksx;
            const uint32_t* base = pix + xmin;
            int acc[RS_ROWS][3];
#pragma unroll
            for (int j = 0; j < RS_ROWS; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (PREC - 1);
            for (int t = 0; t < cnt; ++t) {
                const int kk = k[t];
#pragma unroll
                for (int j = 0; j < RS_ROWS; ++j) {
                    const uint32_t p = base[rowoff[j] + t];
                    acc[j][0] += __mul24((int)(p & 0xff), kk);
                    acc[j][1] += __mul24((int)((p >> 8) & 0xff), kk);
                    acc[j][2] += __mul24((int)(p >> 16), kk);
                }
            }
#pragma unroll
            for (int j = 0; j < RS_ROWS; ++j) {
                if (j < nr) {
                    uint8_t* o = ws + (g.irow0 + r0 + j) * ipitch + 3 * x;
                    o[0] = (uint8_t)clip8(acc[j][0]);
                    o[1] = (uint8_t)clip8(acc[j][1]);
                    o[2] = (uint8_t)clip8(acc[j][2]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(RV_THREADS) void resample_v_kernel(const int64_t* __restrict__ plan, const int32_t* __restrict__ tab,
                                                                int64_t tab_ints, int size, int ipitch,
                                                                const uint8_t* __restrict__ ws, int64_t ws_rows,
                                                                float* __restrict__ out, uint8_t* __restrict__ out_u8, float m0,
                                                                float m1, float m2, float s0, float s1, float s2) {
    extern __shared__ uint32_t rowbuf[];   // [RV_ROWS][ipitch] bytes
    const int b = blockIdx.y;
    const Img g = load_plan(plan, b, size, (int64_t)1 << 62, tab, tab_ints, ws_rows);
    if (!g.ok) return;
    const int tid = threadIdx.x, y0 = blockIdx.x * RV_ROWS, nd = ipitch >> 2;
    for (int item = tid; item < RV_ROWS * nd; item += RV_THREADS) {
        const int yy = item / nd, j = item - yy * nd, y = y0 + yy;
        if (y >= size) break;
        const int ymin = clamp_i(g.yb[2 * y], g.row0, g.row0 + g.nrows);
        const int lim = g.row0 + g.nrows - ymin < g.ksy ? g.row0 + g.nrows - ymin : g.ksy;
        const int cnt = clamp_i(g.yb[2 * y + 1], 0, lim);
        const int32_t* k = g.yk + (int64_t)y * g.ksy;
        const uint8_t* col = ws + (g.irow0 + (ymin - g.row0)) * ipitch + 4 * j;
        int acc[4] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
        for (int t = 0; t < cnt; ++t) {
            const int kk = k[t];
            const uint32_t d = *(const uint32_t*)(col + (int64_t)t * ipitch);
            acc[0] += __mul24((int)(d & 0xff), kk);
            acc[1] += __mul24((int)((d >> 8) & 0xff), kk);
            acc[2] += __mul24((int)((d >> 16) & 0xff), kk);
            acc[3] += __mul24((int)(d >> 24), kk);
        }
        rowbuf[item] = clip8(acc[0]) | (clip8(acc[1]) << 8) | (clip8(acc[2]) << 16) | (clip8(acc[3]) << 24);
    }
    __syncthreads();
    const uint8_t* bytes = (const uint8_t*)rowbuf;
    const int plane = 3 * size;
    for (int item = tid; item < RV_ROWS * plane; item += RV_THREADS) {
        const int yy = item / plane, rem = item - yy * plane, c = rem / size, x = rem - c * size, y = y0 + yy;
        if (y >= size) break;
        const float u = (float)bytes[yy * ipitch + 3 * x + c];
        const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
        out[(((int64_t)b * 3 + c) * size + y) * size + x] = (u / 255.0f - mean) / sd;   // image_normalize_u8_kernel's expression
    }
    if (out_u8) {
        for (int item = tid; item < RV_ROWS * plane; item += RV_THREADS) {
            const int yy = item / plane, i = item - yy * plane, y = y0 + yy;
            if (y >= size) break;
            out_u8[((int64_t)b * size + y) * plane + i] = bytes[yy * ipitch + i];
        }
    }
}

// Pillow's bicubic_filter, a = -0.5, in its two Horner forms (resample._bicubic)
DEVINL double bicubic_weight(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    x = __builtin_fabs(x);
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
// row length Pillow gives the coefficients of in -> out (resample.axis_ksize); in < 2^24, out >= 1: fits an int
DEVINL int axis_ksize(int in, int out) {
#pragma clang fp contract(off)
    if (in == out) return 1;
    const double scale = (double)in / (double)out;
    return (int)__builtin_ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

__global__ __launch_bounds__(RT_THREADS) void resample_tables_kernel(const int64_t* __restrict__ plan, int size,
                                                                     int32_t* __restrict__ tab, int64_t tab_ints) {
#pragma clang fp contract(off)
    const int64_t* p = plan + (int64_t)blockIdx.y * PLAN_FIELDS;
    if (p[PLAN_BUILD] == 0) return;
    const int64_t w = p[1], h = p[2], ksx = p[6], ksy = p[7], xb = p[8], xk = p[9], yb = p[10], yk = p[11];
    // the whole record or nothing (wave-uniform): sizes, row lengths and the four extents inside tab, as load_plan checks them
    if (!(w > 0 && w < (1 << 24) && h > 0 && h < (1 << 24) && ksx > 0 && ksx < (1 << 20) && ksy > 0 && ksy < (1 << 20) && xb >= 0 &&
          xb + 2 * size <= tab_ints && xk >= 0 && xk + size * ksx <= tab_ints && yb >= 0 && yb + 2 * size <= tab_ints && yk >= 0 &&
          yk + size * ksy <= tab_ints))
        return;
    if (axis_ksize((int)w, size) > ksx || axis_ksize((int)h, size) > ksy) return;   // a row of taps would not fit the plan's rows
    const int idx = blockIdx.x * RT_THREADS + threadIdx.x;
    if (idx >= 2 * size) return;
    const int axis = idx >= size, i = idx - axis * size;
    const int in = (int)(axis ? h : w), ks = (int)(axis ? ksy : ksx);
    int32_t* bounds = tab + (axis ? yb : xb) + 2 * i;
    int32_t* k = tab + (axis ? yk : xk) + (int64_t)i * ks;
    int xmin = i, xmax = 1;
    if (in == size) {   // Pillow skips the pass: the identity row
        k[0] = 1 << PREC;
    } else {
        const double scale = (double)in / (double)size;
        const double filterscale = scale < 1.0 ? 1.0 : scale;
        const double support = 2.0 * filterscale, ss = 1.0 / filterscale;
        const double center = (i + 0.5) * scale;
        xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        if (xmax > ks) return;   // cannot happen: xmax <= axis_ksize(in, size) <= ks
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) ww += bicubic_weight((x + xmin - center + 0.5) * ss);   // ascending x
        for (int x = 0; x < xmax; ++x) {
            double v = bicubic_weight((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) v = v / ww;
            k[x] = (int)(v < 0 ? -0.5 + v * (double)(1 << PREC) : 0.5 + v * (double)(1 << PREC));
        }
    }
    for (int x = xmax; x < ks; ++x) k[x] = 0;
    bounds[0] = xmin;
    bounds[1] = xmax;
}

inline int64_t inter_pitch(int64_t size) { return (size * 3 + 3) & ~(int64_t)3; }

}  // namespace

extern "C" int64_t m3ae_image_resample_workspace_bytes(int64_t total_rows, int64_t size) {
    if (total_rows <= 0 || size <= 0) return 0;
    return total_rows * inter_pitch(size);
}

extern "C" int m3ae_image_resample_u8(const uint8_t* src, int64_t src_bytes, const int64_t* plan, const int32_t* tab,
                                      int64_t tab_ints, int64_t B, int64_t size, uint8_t* workspace, int64_t workspace_bytes,
                                      float* out, uint8_t* out_u8, const float* mean3, const float* std3, void* stream) {
    if (!src || !plan || !tab || !workspace || !out || !mean3 || !std3 || B <= 0 || size <= 0 || src_bytes <= 0 || tab_ints <= 0)
        return M3AE_ERR_ARG;
    if (B > 65535 || size > 4096) return M3AE_ERR_UNSUPPORTED;   // grid.y; RV_ROWS rows of 3 * size bytes in LDS (48 KiB)
    if ((uintptr_t)workspace & 3) return M3AE_ERR_ALIGN;
    const int64_t ipitch = inter_pitch(size), ws_rows = workspace_bytes / ipitch;
    if (ws_rows <= 0) return M3AE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    int64_t gx = 4096 / B;   // pass 1 strides over an image's row blocks: enough workgroups for small batches, no tail of idle ones
    gx = gx < 8 ? 8 : (gx > 128 ? 128 : gx);
    hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)gx, (unsigned)B), dim3(RS_THREADS), 0, s, src, src_bytes, plan, tab,
                       tab_ints, (int)size, (int)ipitch, workspace, ws_rows);
    int rc = hip_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)cdiv(size, RV_ROWS), (unsigned)B), dim3(RV_THREADS),
                       (size_t)(RV_ROWS * ipitch), s, plan, tab, tab_ints, (int)size, (int)ipitch, workspace, ws_rows, out, out_u8,
                       mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
    return hip_launch_status();
}

extern "C" int m3ae_image_resample_tables(const int64_t* plan, int64_t B, int64_t size, int32_t* tab, int64_t tab_ints, void* stream) {
    if (!plan || !tab || B <= 0 || size <= 0 || tab_ints <= 0) return M3AE_ERR_ARG;
    if (B > 65535 || size > 4096) return M3AE_ERR_UNSUPPORTED;   // grid.y; the size cap of m3ae_image_resample_u8
    hipLaunchKernelGGL(resample_tables_kernel, dim3((unsigned)cdiv(2 * size, RT_THREADS), (unsigned)B), dim3(RT_THREADS), 0,
                       (hipStream_t)stream, plan, (int)size, tab, tab_ints);
    return hip_launch_status();
}
