// Attention heatmaps: the bilinear upsample of a patch grid of received attention to the image (m3ae_decoder.py:225-290 calls
// torch.nn.functional.interpolate(mode="bilinear", align_corners=False) on the head-and-query mean of an attention map).
//
// The arithmetic is stated in include/m3ae_hip.h and is the whole contract: source coordinate, the two taps and their weights per
// axis in fp32, every product and sum rounded once (`#pragma clang fp contract(off)`: no multiply-add is fused, so a host model in
// np.float32 forms the same weights bit for bit).  scale = (float)g / (float)S is the host's IEEE division, passed as an argument.
// One thread per output element, lanes along the output row: the stores are dense dwords, the four taps of a wave come from at most
// two input rows of a grid that stays in cache (g * g floats per sample; 24 x 24 for the 384-pixel model).
#include "common.h"

namespace {

struct Tap { int i0, i1; float l0, l1; };
DEVINL Tap axis_tap(int d, int g, float scale) {
#pragma clang fp contract(off)
    float src = scale * ((float)d + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Tap t;
    t.i0 = (int)src;
    t.i0 = t.i0 < g - 1 ? t.i0 : g - 1;
    t.i1 = t.i0 + 1 < g - 1 ? t.i0 + 1 : g - 1;
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

__global__ __launch_bounds__(256) void heatmap_upsample_kernel(const float* __restrict__ in, int64_t in_sb, int g,
                                                                float* __restrict__ out, int S, float scale) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)S * S) return;
    const int y = (int)(idx / S), x = (int)(idx - (int64_t)y * S);
    const Tap ty = axis_tap(y, g, scale), tx = axis_tap(x, g, scale);
    const float* p = in + (int64_t)blockIdx.y * in_sb;
    const float* r0 = p + (int64_t)ty.i0 * g;
    const float* r1 = p + (int64_t)ty.i1 * g;
    const float top = tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1];
    const float bot = tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1];
    out[(int64_t)blockIdx.y * S * S + idx] = ty.l0 * top + ty.l1 * bot;
}

}  // namespace

extern "C" int m3ae_heatmap_upsample(const float* in, int64_t in_sb, int64_t g, float* out, int64_t B, int64_t S, void* stream) {
    if (!in || !out || B < 1 || g < 1 || S < 1) return M3AE_ERR_ARG;
    if (g > 16384 || S > 16384) return M3AE_ERR_UNSUPPORTED;   // int tap indices; grid.x = S * S / 256
    if (in_sb < g * g) return M3AE_ERR_ARG;
    if (B > 65535) return M3AE_ERR_UNSUPPORTED;                // grid.y
    hipLaunchKernelGGL(heatmap_upsample_kernel, dim3((unsigned)cdiv(S * S, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, in,
                       in_sb, (int)g, out, (int)S, (float)g / (float)S);
    return hip_launch_status();
}
