// RandAugment(2, 9) on the uploaded source bytes of a batch (m3ae_amd/randaug.py is the specification; the reference:
// transforms/randaug.py:164-272 in front of the CLIP transform, transforms/transform.py:80-91).  Two stages per image, ping-pong
// between the pack's source buffer and a scratch buffer of the same layout (every image at a 16-byte aligned offset, rows packed,
// 3 bytes per pixel): stage 0 reads src and writes scratch, stage 1 reads scratch and writes src, where the resample finds it.
// Per stage up to three launches, blockIdx.y = image:
//   1. randaug_hist_kernel    histograms of R, G, B and L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 of the stage's input, for the
//                             images whose operation reads one (AutoContrast, Equalize, Contrast).  Integer LDS atomics, then integer
//                             global atomics: sums of integers, the same in any order.
//   2. randaug_lut_kernel     one workgroup per image: the 3 x 256 byte table of a point operation, Pillow's Python restated one
//                             operation at a time (ImageOps.autocontrast: float64; equalize: integers; ImageEnhance.Contrast /
//                             Brightness: Image.blend's float32 on a constant) under `#pragma clang fp contract(off)`.
//   3. randaug_apply_kernel   point: table in LDS, 16 bytes per access (the channel of byte i of an image is i % 3);
//                             Color / Sharpness / the five affine maps: four pixels = three dwords per thread and store.
// Every operation is integer arithmetic or single correctly rounded float operations in Pillow's order, so the bytes are Pillow's.
// A record is checked whole against the buffer size before anything is addressed through it (load_aug); a record that fails,
// and the identity record (both stages 0: an image the host augmented already), is passed over by every kernel.
#include "common.h"

namespace {

constexpr int AUG_FIELDS = 24, AUG_STAGE0 = 4, AUG_STAGE_FIELDS = 10;   // randaug.py: AUG_*
constexpr int RA_THREADS = 256;
constexpr int MAX_W = 8192, MAX_H = 16384;                               // resample.MAX_SOURCE_WIDTH, randaug.MAX_AUG_HEIGHT
enum Op { OP_IDENTITY, OP_AUTOCONTRAST, OP_EQUALIZE, OP_ROTATE, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD, OP_COLOR, OP_CONTRAST,
          OP_BRIGHTNESS, OP_SHARPNESS, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y, OP_COUNT };
// the values of magnitude 9 (randaug.VALUE): enhance factor (9 / 30) * 1.8 + 0.1 -> 0.64f, Solarize 76.8 (i < 76.8 <=> i < 77),
// SolarizeAdd 33 then 128, Posterize int(1.2) = 1 bit
constexpr float ENHANCE = 0.64f;
constexpr int SOLARIZE_BELOW = 77, SOLARIZE_ADD = 33, POSTERIZE_MASK = 0x80;

DEVINL bool is_geometric(int op) { return op == OP_ROTATE || (op >= OP_SHEAR_X && op <= OP_TRANSLATE_Y); }
DEVINL bool reads_hist(int op) { return op == OP_AUTOCONTRAST || op == OP_EQUALIZE || op == OP_CONTRAST; }
DEVINL bool is_point(int op) { return reads_hist(op) || op == OP_POSTERIZE || op == OP_SOLARIZE || op == OP_SOLARIZE_ADD || op == OP_BRIGHTNESS; }

struct Aug {
    int64_t off;
    int w, h, op;
    int64_t a[6];
    bool ok;
};
// record of image b, stage s -> Aug; ok = the whole record (both stages) is sound and has work to do (wave-uniform)
DEVINL Aug load_aug(const int64_t* plan, int b, int s, int64_t buf_bytes) {
    const int64_t* p = plan + (int64_t)b * AUG_FIELDS;
    Aug g;
    g.off = p[0];
    const int64_t w = p[1], h = p[2];
    bool ok = g.off >= 0 && (g.off & 15) == 0 && w > 0 && w <= MAX_W && h > 0 && h <= MAX_H;
    ok = ok && g.off + 3 * w * h <= buf_bytes;
    bool work = false;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int64_t* q = p + AUG_STAGE0 + AUG_STAGE_FIELDS * t;
        ok = ok && q[0] >= 0 && q[0] < OP_COUNT;
        work = work || q[0] != OP_IDENTITY;
#pragma unroll
        for (int i = 0; i < 6; ++i) ok = ok && q[2 + i] > -((int64_t)1 << 40) && q[2 + i] < ((int64_t)1 << 40);   // sums stay below 2^56
    }
    const int64_t* q = p + AUG_STAGE0 + AUG_STAGE_FIELDS * s;
    g.ok = ok && work;
    g.w = (int)w; g.h = (int)h; g.op = (int)q[0];
#pragma unroll
    for (int i = 0; i < 6; ++i) g.a[i] = q[2 + i];
    return g;
}

DEVINL uint32_t luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }
// Image.blend, 0 <= alpha <= 1: (uint8)(a + alpha * (b - a)) in float32, the product and the sum rounded separately
DEVINL uint32_t blend8(int a, int b) {
#pragma clang fp contract(off)
    const float prod = ENHANCE * (float)(b - a);
    return (uint32_t)(int)((float)a + prod) & 0xffu;
}

// ---- 1. histograms ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RA_THREADS) void randaug_hist_kernel(const uint8_t* __restrict__ in, int64_t buf_bytes,
                                                                  const int64_t* __restrict__ plan, int stage,
                                                                  uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[4 * 256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const Aug g = load_aug(plan, b, stage, buf_bytes);
    if (!g.ok || !reads_hist(g.op)) return;
    for (int i = tid; i < 4 * 256; i += RA_THREADS) lh[i] = 0;
    __syncthreads();
    const uint8_t* img = in + g.off;
    const int npix = g.w * g.h, ngroups = npix >> 2;
    auto count = [&](uint32_t r, uint32_t gg, uint32_t bb) {
        atomicAdd(&lh[r], 1u);
        atomicAdd(&lh[256 + gg], 1u);
        atomicAdd(&lh[512 + bb], 1u);
        atomicAdd(&lh[768 + luma(r, gg, bb)], 1u);
    };
    const uint32_t* dw = (const uint32_t*)img;
    for (int k = blockIdx.x * RA_THREADS + tid; k < ngroups; k += gridDim.x * RA_THREADS) {   // 4 pixels = 3 aligned dwords
        const uint32_t d0 = dw[3 * k], d1 = dw[3 * k + 1], d2 = dw[3 * k + 2];
        count(d0 & 0xff, (d0 >> 8) & 0xff, (d0 >> 16) & 0xff);
        count(d0 >> 24, d1 & 0xff, (d1 >> 8) & 0xff);
        count((d1 >> 16) & 0xff, d1 >> 24, d2 & 0xff);
        count((d2 >> 8) & 0xff, (d2 >> 16) & 0xff, d2 >> 24);
    }
    if (blockIdx.x == 0 && tid < (npix & 3)) {
        const uint8_t* p = img + 3 * (4 * ngroups + tid);
        count(p[0], p[1], p[2]);
    }
    __syncthreads();
    uint32_t* out = hist + (int64_t)b * 1024;
    for (int i = tid; i < 4 * 256; i += RA_THREADS)
        if (lh[i]) atomicAdd(&out[i], lh[i]);
}

// ---- 2. tables ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RA_THREADS) void randaug_lut_kernel(const int64_t* __restrict__ plan, int64_t buf_bytes, int stage,
                                                                 const uint32_t* __restrict__ hist, uint8_t* __restrict__ lut) {
#pragma clang fp contract(off)
    __shared__ uint32_t lh[4 * 256];
    const int b = blockIdx.x, i = threadIdx.x;   // thread i owns entry i of the three channels
    const Aug g = load_aug(plan, b, stage, buf_bytes);
    if (!g.ok || !is_point(g.op)) return;
    uint8_t* out = lut + (int64_t)b * 768;
    if (reads_hist(g.op)) {
        for (int k = i; k < 4 * 256; k += RA_THREADS) lh[k] = hist[(int64_t)b * 1024 + k];
        __syncthreads();
    }
    if (g.op == OP_AUTOCONTRAST || g.op == OP_EQUALIZE) {
        for (int c = 0; c < 3; ++c) {
            const uint32_t* h = lh + 256 * c;
            int lo = -1, hi = -1, used = 0;
            uint32_t total = 0, below = 0, last = 0;   // pixels of the channel, pixels of the bins under i, the last used bin
            for (int j = 0; j < 256; ++j) {
                const uint32_t n = h[j];
                if (n) {
                    if (lo < 0) lo = j;
                    hi = j;
                    last = n;
                    ++used;
                }
                total += n;
                if (j < i) below += n;
            }
            int v = i;
            if (g.op == OP_AUTOCONTRAST) {   // ImageOps.autocontrast: scale = 255.0 / (hi - lo); offset = -lo * scale; int(ix * scale + offset)
                if (hi > lo) {
                    const double scale = 255.0 / (double)(hi - lo);
                    const double offset = (double)(-lo) * scale;
                    v = (int)((double)i * scale + offset);
                    v = v < 0 ? 0 : (v > 255 ? 255 : v);
                }
            } else if (used > 1) {           // ImageOps.equalize: step = (sum - last used bin) // 255; lut[i] = (step // 2 + sum below i) // step
                const uint32_t step = (total - last) / 255u;
                if (step) {
                    const uint32_t q = (step / 2u + below) / step;
                    v = q > 255u ? 255 : (int)q;   // point() clips the table to bytes
                }
            }
            out[256 * c + i] = (uint8_t)v;
        }
        return;
    }
    int v = i;
    if (g.op == OP_POSTERIZE) {
        v = i & POSTERIZE_MASK;
    } else if (g.op == OP_SOLARIZE) {
        v = i < SOLARIZE_BELOW ? i : 255 - i;
    } else if (g.op == OP_SOLARIZE_ADD) {
        const int j = i + SOLARIZE_ADD > 255 ? 255 : i + SOLARIZE_ADD;
        v = j < 128 ? j : 255 - j;
    } else if (g.op == OP_BRIGHTNESS) {
        v = (int)blend8(0, i);
    } else {   // OP_CONTRAST: the mean of L as ImageStat computes it (float64 sum and division), int(mean + 0.5)
        const uint32_t* h = lh + 768;
        uint64_t count = 0, sum = 0;
        for (int j = 0; j < 256; ++j) {
            count += h[j];
            sum += (uint64_t)j * h[j];
        }
        const int mean = count ? (int)((double)sum / (double)count + 0.5) : 0;
        v = (int)blend8(mean, i);
    }
    out[i] = out[256 + i] = out[512 + i] = (uint8_t)v;
}

// ---- 3. apply -----------------------------------------------------------------------------------------------------------
// ImageFilter.SMOOTH then Image.blend of pixel (x, y), channel c: float32 sum from 0.5 of the neighbourhood times 1/13 (5/13 the centre)
DEVINL uint32_t sharp8(const uint8_t* img, int pitch, int x, int y, int c) {
#pragma clang fp contract(off)
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
    const uint8_t* p = img + (int64_t)y * pitch + 3 * x + c;
    float ss = 0.5f;
    ss += (float)p[pitch - 3] * k1; ss += (float)p[pitch] * k1; ss += (float)p[pitch + 3] * k1;
    ss += (float)p[-3] * k1;        ss += (float)p[0] * k5;     ss += (float)p[3] * k1;
    ss += (float)p[-pitch - 3] * k1; ss += (float)p[-pitch] * k1; ss += (float)p[-pitch + 3] * k1;
    const int d = ss <= 0.f ? 0 : (ss >= 255.f ? 255 : (int)ss);
    return blend8(d, p[0]);
}
// output pixel idx of a Sharpness / affine stage -> R | G << 8 | B << 16
DEVINL uint32_t gather_pixel(const Aug& g, const uint8_t* img, int x, int y) {
    const int pitch = 3 * g.w;
    if (g.op == OP_SHARPNESS) {
        const uint8_t* p = img + (int64_t)y * pitch + 3 * x;
        if (x == 0 || y == 0 || x == g.w - 1 || y == g.h - 1) return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        return sharp8(img, pitch, x, y, 0) | (sharp8(img, pitch, x, y, 1) << 8) | (sharp8(img, pitch, x, y, 2) << 16);
    }
    // Geometry.c affine_fixed: 16.16 fixed point, nearest neighbour, black outside
    const int64_t xin = (g.a[2] + y * g.a[1] + x * g.a[0]) >> 16, yin = (g.a[5] + y * g.a[4] + x * g.a[3]) >> 16;
    if (xin < 0 || xin >= g.w || yin < 0 || yin >= g.h) return 0;
    const uint8_t* p = img + yin * pitch + 3 * xin;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}
DEVINL uint32_t color_pixel(uint32_t r, uint32_t gg, uint32_t bb) {
    const int l = (int)luma(r, gg, bb);
    return blend8(l, (int)r) | (blend8(l, (int)gg) << 8) | (blend8(l, (int)bb) << 16);
}

__global__ __launch_bounds__(RA_THREADS) void randaug_apply_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                                   int64_t buf_bytes, const int64_t* __restrict__ plan, int stage,
                                                                   const uint8_t* __restrict__ lut) {
    __shared__ uint8_t ll[768];
    const int b = blockIdx.y, tid = threadIdx.x;
    const Aug g = load_aug(plan, b, stage, buf_bytes);
    if (!g.ok) return;
    const uint8_t* src = in + g.off;
    uint8_t* dst = out + g.off;
    const int npix = g.w * g.h, first = blockIdx.x * RA_THREADS + tid, stride = gridDim.x * RA_THREADS;
    if (g.op == OP_IDENTITY || is_point(g.op)) {
        const bool map = g.op != OP_IDENTITY;
        if (map) {
            for (int k = tid; k < 768; k += RA_THREADS) ll[k] = lut[(int64_t)b * 768 + k];
            __syncthreads();
        }
        const int nbytes = 3 * npix, n16 = nbytes >> 4;
        const u32x4* s16 = (const u32x4*)src;
        u32x4* d16 = (u32x4*)dst;
        for (int k = first; k < n16; k += stride) {
            u32x4 v = s16[k];
            if (map) {
                int c = k % 3;   // byte 16 k of the image is channel (16 k) % 3 = k % 3
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    uint32_t o = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        o |= (uint32_t)ll[256 * c + ((v[d] >> (8 * j)) & 0xff)] << (8 * j);
                        c = c == 2 ? 0 : c + 1;
                    }
                    v[d] = o;
                }
            }
            d16[k] = v;
        }
        if (blockIdx.x == 0 && tid < (nbytes & 15)) {
            const int i = 16 * n16 + tid;
            dst[i] = map ? ll[256 * (i % 3) + src[i]] : src[i];
        }
        return;
    }
    // four pixels per thread: three dwords out (and, for Color, in)
    const int ngroups = npix >> 2;
    const uint32_t* sdw = (const uint32_t*)src;
    uint32_t* ddw = (uint32_t*)dst;
    for (int k = first; k < ngroups; k += stride) {
        uint32_t p0, p1, p2, p3;
        if (g.op == OP_COLOR) {
            const uint32_t d0 = sdw[3 * k], d1 = sdw[3 * k + 1], d2 = sdw[3 * k + 2];
            p0 = color_pixel(d0 & 0xff, (d0 >> 8) & 0xff, (d0 >> 16) & 0xff);
            p1 = color_pixel(d0 >> 24, d1 & 0xff, (d1 >> 8) & 0xff);
            p2 = color_pixel((d1 >> 16) & 0xff, d1 >> 24, d2 & 0xff);
            p3 = color_pixel((d2 >> 8) & 0xff, (d2 >> 16) & 0xff, d2 >> 24);
        } else {
            int y = (4 * k) / g.w, x = 4 * k - y * g.w;
            p0 = gather_pixel(g, src, x, y);
            if (++x == g.w) { x = 0; ++y; }
            p1 = gather_pixel(g, src, x, y);
            if (++x == g.w) { x = 0; ++y; }
            p2 = gather_pixel(g, src, x, y);
            if (++x == g.w) { x = 0; ++y; }
            p3 = gather_pixel(g, src, x, y);
        }
        ddw[3 * k] = p0 | (p1 << 24);
        ddw[3 * k + 1] = (p1 >> 8) | (p2 << 16);
        ddw[3 * k + 2] = (p2 >> 16) | (p3 << 8);
    }
    if (blockIdx.x == 0 && tid < (npix & 3)) {
        const int idx = 4 * ngroups + tid;
        uint32_t p;
        if (g.op == OP_COLOR) {
            p = color_pixel(src[3 * idx], src[3 * idx + 1], src[3 * idx + 2]);
        } else {
            const int y = idx / g.w;
            p = gather_pixel(g, src, idx - y * g.w, y);
        }
        dst[3 * idx] = (uint8_t)p;
        dst[3 * idx + 1] = (uint8_t)(p >> 8);
        dst[3 * idx + 2] = (uint8_t)(p >> 16);
    }
}

}  // namespace

extern "C" int64_t m3ae_image_randaug_workspace_bytes(int64_t B) {
    if (B <= 0) return 0;
    return B * (2 * 1024 * (int64_t)sizeof(uint32_t) + 768);
}

extern "C" int m3ae_image_randaug_u8(uint8_t* src, uint8_t* scratch, int64_t buf_bytes, const int64_t* plan, int64_t B,
                                     void* workspace, int64_t workspace_bytes, int flags, void* stream) {
    if (!src || !scratch || src == scratch || !plan || !workspace || B <= 0 || buf_bytes <= 0 || (flags & ~15)) return M3AE_ERR_ARG;
    if (B > 65535) return M3AE_ERR_UNSUPPORTED;   // grid.y
    if (((uintptr_t)src & 15) || ((uintptr_t)scratch & 15) || ((uintptr_t)workspace & 3)) return M3AE_ERR_ALIGN;
    if (workspace_bytes < m3ae_image_randaug_workspace_bytes(B)) return M3AE_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* hist = (uint32_t*)workspace;
    uint8_t* lut = (uint8_t*)(hist + 2 * B * 1024);
    int64_t gx = 4096 / B;   // the kernels stride over an image: enough workgroups for a small batch, no tail of idle ones
    gx = gx < 8 ? 8 : (gx > 128 ? 128 : gx);
    for (int stage = 0; stage < 2; ++stage) {
        const uint8_t* in = stage ? scratch : src;
        uint8_t* out = stage ? src : scratch;
        uint32_t* h = hist + (int64_t)stage * B * 1024;
        if (flags & (1 << stage)) {   // a stage without a histogram user skips the pass over its input
            hipError_t e = hipMemsetAsync(h, 0, (size_t)B * 1024 * sizeof(uint32_t), s);
            if (e != hipSuccess) return (int)e;
            hipLaunchKernelGGL(randaug_hist_kernel, dim3((unsigned)gx, (unsigned)B), dim3(RA_THREADS), 0, s, in, buf_bytes, plan, stage, h);
            int rc = hip_launch_status();
            if (rc) return rc;
        }
        if (flags & (4 << stage)) {
            hipLaunchKernelGGL(randaug_lut_kernel, dim3((unsigned)B), dim3(RA_THREADS), 0, s, plan, buf_bytes, stage, h, lut);
            int rc = hip_launch_status();
            if (rc) return rc;
        }
        hipLaunchKernelGGL(randaug_apply_kernel, dim3((unsigned)gx, (unsigned)B), dim3(RA_THREADS), 0, s, in, out, buf_bytes, plan, stage, lut);
        int rc = hip_launch_status();
        if (rc) return rc;
    }
    return 0;
}
