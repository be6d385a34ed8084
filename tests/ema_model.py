"""numpy model of the EMA kernels (csrc/misc.hip: m3ae_ema_update, m3ae_ema_swap) and of the decay schedule, shared by
tests/test_ema_host.py and tests/test_gpu_ema.py.

The update is two fp32 roundings around an exact float64 value:
    d  = fl32(p - e)
    e' = fl32(w * d + e)          (one fused multiply-add)
Against exact E = e + w (p - e):  d = (p - e)(1 + d1), e' = (E + w (p - e) d1)(1 + d2), |d1|, |d2| <= u = 2^-24, so
    |e' - E| <= u (w |p - e| + |E|) + u^2 w |p - e|
and the second-order term is at most 2^-24 of the first: the factor (1 + 2^-20) covers it with room for the float64 arithmetic of
the reference itself (2^-53 relative).  There is no absolute term: the bound holds while no intermediate is subnormal."""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
EW_CAP = 8192 * 256 * 4            # ew_grid's cap x EW_BLOCK x 4 elements per lane: above it the grid-stride loop runs twice
SIZES = (4, 4 * 256 + 4, EW_CAP + 12)
WEIGHTS = (np.float32(0.0), np.float32(1e-4), np.float32(1.0 - 2.0 / 11.0), np.float32(0.5))


def inputs(n, seed):
    """(p, e): normal fp32 values of mixed magnitude, 1e-6 .. 1e3 (log-uniform), both signs, independent of each other."""
    rng = np.random.default_rng(seed)

    def draw():
        mag = 10.0 ** rng.uniform(-6.0, 3.0, n)
        return (mag * rng.choice((-1.0, 1.0), n)).astype(np.float32)
    return draw(), draw()


def exact(p, e, w):
    """E = e + w (p - e) in float64 (p, e, w fp32 values: the difference and the product are exact or within 2^-53)."""
    p, e = np.asarray(p, np.float64), np.asarray(e, np.float64)
    return e + np.float64(w) * (p - e)


def bound(p, e, w):
    """The issue's bound on |got - E| for one update from fp32 (p, e)."""
    p, e = np.asarray(p, np.float64), np.asarray(e, np.float64)
    return U * (np.float64(w) * np.abs(p - e) + np.abs(exact(p, e, w))) * SLACK


def update(p, e, w):
    """The kernel's two roundings: fp32 subtraction, then the multiply-add formed in float64 (the product of two fp32 values is exact
    there) and rounded to fp32."""
    p, e = np.asarray(p, np.float32), np.asarray(e, np.float32)
    d = (p - e).astype(np.float32)
    return (np.float64(w) * d.astype(np.float64) + e.astype(np.float64)).astype(np.float32)


def accumulate(snapshots, weights):
    """(E, B) after len(weights) updates that start from snapshots[0] and see snapshots[k] at update k: the float64 recurrence and
    the budget on |got - E|.  One update from an average that is already B off:  the exact map moves the old error by (1 - w), and
    the arguments of the one-step bound are each within B of the reference's, so
        B_k = (1 - w_k) B_{k-1} + u (1 + 2^-20) (w_k |P_k - E_{k-1}| + |E_k| + B_{k-1})."""
    E = np.asarray(snapshots[0], np.float64).copy()
    B = np.zeros_like(E)
    for P, w in zip(snapshots[1:], weights):
        P, w = np.asarray(P, np.float64), np.float64(w)
        E_new = E + w * (P - E)
        B = (1.0 - w) * B + U * SLACK * (w * np.abs(P - E) + np.abs(E_new) + B)
        E = E_new
    return E, B


def bf16_bits(x):
    """Round-to-nearest-even bf16 bit patterns (uint16) of fp32 values; NaN is not modelled."""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_edge_values():
    """fp32 values at which a bf16 rounding can go wrong: exact ties with an even and an odd kept bit (up and down), just off the
    ties, +-0, subnormals (fp32 subnormals that stay bf16 subnormals, the smallest one, a tie among them), the largest finite fp32
    (rounds to inf), the largest value that stays finite, and inf.  Length is a multiple of 4."""
    pats = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001,      # ties around 1.0 and their neighbours
            0xBF808000, 0xBF818000, 0x00000000, 0x80000000,                              # negative ties, +-0
            0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80408000, 0x00010000,      # subnormals
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0x7F800000, 0xFF800000,      # largest finite, last finite bf16, inf
            0x42F6E979, 0xC479FFFF]                                                      # ordinary values
    assert len(pats) % 4 == 0
    return np.array(pats, dtype=np.uint32).view(np.float32)


def decay_at(decay, t, warmup):
    """decay_t of the t-th update (1-based)."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def weight(decay, t, warmup):
    """w = 1 - decay_t, formed in double and rounded to fp32 once."""
    return np.float32(1.0 - decay_at(decay, t, warmup))
