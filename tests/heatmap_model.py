"""numpy models of the attention summaries and heatmaps (tests/test_attn_summary_host.py, tests/test_gpu_attn_summary.py).

recv: the received attention of a map P [B, H, Lq, Lk], its mean over heads and queries, in float64.
upsample: the bilinear upsample of m3ae_heatmap_upsample (include/m3ae_hip.h).  The source coordinate, the two taps and their
weights per axis are formed in np.float32 by the header's formula, one rounding per operation -- the bits the kernel forms --
and the combination of the four taps is float64."""
import numpy as np

U = 2.0 ** -24   # unit roundoff of fp32


def recv(p):
    p = np.asarray(p, dtype=np.float64)
    return p.mean(axis=(1, 2))


def recv_bound(ref, H, Lq):
    """|got - ref| allowed for a kernel that adds the H Lq non-negative fp32 entries in any order (H Lq - 1 additions, each
    within U of its exact sum, all partial sums <= the total), multiplies by the rounded reciprocal (U) and rounds the product (U)."""
    return (H * Lq + 2) * U * np.asarray(ref, dtype=np.float64)


def axis_taps(g, S):
    f = np.float32
    scale = f(g) / f(S)
    d = np.arange(S, dtype=np.float32)
    src = scale * (d + f(0.5)) - f(0.5)
    assert src.dtype == np.float32
    src = np.maximum(src, f(0))
    i0 = np.minimum(src.astype(np.int64), g - 1)
    i1 = np.minimum(i0 + 1, g - 1)
    l1 = src - i0.astype(np.float32)
    l0 = f(1) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def upsample(grid, S):
    """grid [B, g, g] -> [B, S, S] float64."""
    grid = np.asarray(grid, dtype=np.float64)
    g = grid.shape[-1]
    assert grid.shape[-2] == g
    i0, i1, l0, l1 = axis_taps(g, S)
    top = l0 * grid[:, i0][:, :, i0] + l1 * grid[:, i0][:, :, i1]     # [B, S(y), S(x)], weights along x
    bot = l0 * grid[:, i1][:, :, i0] + l1 * grid[:, i1][:, :, i1]
    return l0[None, :, None] * top + l1[None, :, None] * bot


def heatmap(recv_row, S):
    """The pipeline of M3AETransformerSS.attention_heatmaps on a summary [B, 1 + g * g]: class token off, grid, upsample."""
    r = np.asarray(recv_row)
    n = r.shape[1] - 1
    g = int(round(n ** 0.5))
    assert g * g == n
    return upsample(r[:, 1:].reshape(r.shape[0], g, g), S)
