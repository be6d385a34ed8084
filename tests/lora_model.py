"""numpy model of the LoRA kernels (csrc/lora.hip: m3ae_lora_merge, m3ae_lora_grad), shared by tests/test_lora_host.py and
tests/test_gpu_lora.py.  It restates the kernels' documented operation order with an exact fp32 fused multiply-add, so wherever the
order fixes the bits the kernel and the model agree bit for bit; and it derives, from that order, the bound on the distance to
float64.

fma32: a * b is exact in float64 (48 bits of product); the sum with c is formed in float64 with its rounding error recovered
(TwoSum) and, where inexact, moved to the neighbour with an odd last bit (round to odd); 53 >= 2 * 24 + 2 bits, so the final
rounding to fp32 is the single rounding of an fp32 fmaf -- no double rounding.

Merge (u = 2^-24, gamma_n = n u / (1 - n u), T = sum_j |B[n][j] A[j][k]|, E = W0 + s sum_j B A):
    acc = 0; for j ascending: acc = fmaf(B[n][j], A[j][k], acc)       |acc - sum| <= gamma_r T        (r roundings per term at most)
    W   = fmaf(s, acc, W0)                                            one rounding of W0 + s acc
    |W - E| <= u |E| + (1 + u) |s| gamma_r T
Projection (PANEL = 64 rows per plane, P planes):
    dB[n][j] = s * chain_k fmaf(dW[n][k], A[j][k], acc)               K roundings + the product:  <= gamma_{K+1} |s| sum_k |dW A|
    dA[j][k] = s * fold_p(chain_{n in panel p} fmaf(B[n][j], dW[n][k], acc))
                                                                      <= PANEL roundings in the chain, P - 1 in the fold, 1 product:
                                                                      <= gamma_{min(N, PANEL) + P} |s| sum_n |B dW|
The factor (1 + 2^-20) covers the second-order terms and the float64 arithmetic of the reference itself.  No absolute term: the
bounds hold while no intermediate is subnormal (the inputs below keep every product above 2^-60)."""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
PANEL = 64                                    # rows of one row panel of m3ae_lora_grad (M3AE_LORA_PANEL_ROWS)
ALIGN = 64
SHAPES = ((1, 1), (40, 72), (130, 70), (128, 128), (384, 128), (512, 128))      # (N, K) of one table: the issue's mix
RANKS = (1, 3, 16, 64)
GUARD = 256                                   # sentinel elements in front of and behind every buffer
SENTINEL = np.float32(-7.25)


def gamma(n):
    return n * U / (1.0 - n * U)


def fma32(a, b, c):
    """fp32 fmaf(a, b, c), exactly (see the module docstring); a, b, c broadcastable fp32 arrays."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def merge(W0, A, B, s):
    """The kernel's r + 1 fmafs per element."""
    W0, A, B = (np.asarray(x, np.float32) for x in (W0, A, B))
    acc = np.zeros(W0.shape, np.float32)
    for j in range(A.shape[0]):
        acc = fma32(B[:, j:j + 1], A[j:j + 1, :], acc)
    return fma32(np.float32(s), acc, W0)


def merge_exact(W0, A, B, s):
    W0, A, B = (np.asarray(x, np.float64) for x in (W0, A, B))
    return W0 + np.float64(np.float32(s)) * (B @ A)


def merge_bound(W0, A, B, s):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    T = np.abs(B) @ np.abs(A)
    return (U * np.abs(merge_exact(W0, A, B, s)) + (1.0 + U) * abs(float(np.float32(s))) * gamma(A.shape[0]) * T) * SLACK


def grad(dW, A, B, s, panel=PANEL):
    """(dA [r, K], dB [N, r]) in the kernels' order."""
    dW, A, B = (np.asarray(x, np.float32) for x in (dW, A, B))
    N, K = dW.shape
    s = np.float32(s)
    acc = np.zeros((N, A.shape[0]), np.float32)
    for k in range(K):
        acc = fma32(dW[:, k:k + 1], A[:, k][None, :], acc)
    with np.errstate(invalid="ignore", over="ignore"):
        dB = (s * acc).astype(np.float32)
        tot = None
        for n0 in range(0, N, panel):
            pl = np.zeros((A.shape[0], K), np.float32)
            for n in range(n0, min(n0 + panel, N)):
                pl = fma32(B[n, :][:, None], dW[n, :][None, :], pl)
            tot = pl if tot is None else (tot + pl).astype(np.float32)
        return (s * tot).astype(np.float32), dB


def grad_exact(dW, A, B, s):
    dW, A, B = (np.asarray(x, np.float64) for x in (dW, A, B))
    s = np.float64(np.float32(s))
    return s * (B.T @ dW), s * (dW @ A.T)


def grad_bound(dW, A, B, s, panel=PANEL):
    dW, A, B = (np.abs(np.asarray(x, np.float64)) for x in (dW, A, B))
    N, K = dW.shape
    s = abs(float(np.float32(s)))
    planes = (N + panel - 1) // panel
    return gamma(min(N, panel) + planes) * s * (B.T @ dW) * SLACK, gamma(K + 1) * s * (dW @ A.T) * SLACK


def bf16_bits(x):
    """Round-to-nearest-even bf16 bit patterns (uint16) of finite fp32 values."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def _align(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def layout(r, shapes=SHAPES):
    """Records (elem_offset, N, K, a_off, b_off, base_off) of one table and the buffer sizes {flat, lora, base}.  Offsets are
    64-element aligned as ParamStore's; between the targets of the flat buffer lies an extra 64-element gap (a bias row there), and
    the compact buffers are packed, so the three offsets of a target differ."""
    recs, flat, lora, base = [], 0, 0, 0
    for N, K in shapes:
        a = lora
        lora += _align(r * K)
        b = lora
        lora += _align(N * r)
        recs.append((flat, N, K, a, b, base))
        flat += _align(N * K) + ALIGN
        base += _align(N * K)
    return recs, dict(flat=flat, lora=lora, base=base)


def spread(rng, shape, lo=-20.0, hi=4.0):
    """fp32 values with magnitudes log-uniform in 2^lo .. 2^hi and random signs."""
    return (2.0 ** rng.uniform(lo, hi, shape) * rng.choice((-1.0, 1.0), shape)).astype(np.float32)


def case(r, seed=0, shapes=SHAPES):
    """One table's inputs as flat numpy buffers: {recs, sizes, s, base, lora, grad} with SENTINEL in every padding element."""
    rng = np.random.default_rng(1000 * seed + r)
    recs, sizes = layout(r, shapes)
    base = np.full(sizes["base"], SENTINEL, np.float32)
    lora = np.full(sizes["lora"], SENTINEL, np.float32)
    grad_ = np.full(sizes["flat"], SENTINEL, np.float32)
    for off, N, K, a, b, bo in recs:
        base[bo:bo + N * K] = spread(rng, N * K, -12.0, 2.0)
        lora[a:a + r * K] = spread(rng, r * K)
        lora[b:b + N * r] = spread(rng, N * r)
        grad_[off:off + N * K] = spread(rng, N * K, -16.0, 2.0)
    return dict(recs=recs, sizes=sizes, s=np.float32(16.0 / r), base=base, lora=lora, grad=grad_, r=r)


def parts(c, i):
    """(W0, A, B, dW) of target i of a case()."""
    off, N, K, a, b, bo = c["recs"][i]
    r = c["r"]
    return (c["base"][bo:bo + N * K].reshape(N, K), c["lora"][a:a + r * K].reshape(r, K), c["lora"][b:b + N * r].reshape(N, r),
            c["grad"][off:off + N * K].reshape(N, K))


def in_target_mask(recs, size, which):
    """Boolean mask over a buffer of `size` elements: True inside a target's matrices.  which: "flat" | "base" | "lora"."""
    m = np.zeros(size, bool)
    for off, N, K, a, b, bo in recs:
        if which == "flat":
            m[off:off + N * K] = True
        elif which == "base":
            m[bo:bo + N * K] = True
    return m


def lora_mask(recs, size, r):
    m = np.zeros(size, bool)
    for off, N, K, a, b, bo in recs:
        m[a:a + r * K] = True
        m[b:b + N * r] = True
    return m
