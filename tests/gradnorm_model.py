"""Float64 / float32 numpy models of csrc/gradnorm.hip and of the AdamW kernel's clipped form, shared by test_grad_clip_host.py
and test_gpu_grad_clip.py.  Nothing here touches a GPU or the library.

  * exact_sumsq: math.fsum of the exact squares (the square of an fp32 value is exact in float64) -- the correctly rounded sum;
  * piece_table / check_piece_table: the host's piece table restated, and the properties a piece table must have for m3ae_sumsq_segments to cover every element once;
  * finalize: m3ae_clip_finalize's formulas in float64 and its counters;
  * adamw: csrc/misc.hip's adamw_kernel operation by operation in float32, with the gradient factor given."""
import math

import numpy as np


def exact_sumsq(x):
    """Correctly rounded sum of squares of a float32 array (math.fsum over exact float64 squares)."""
    v = np.asarray(x, dtype=np.float32).astype(np.float64).ravel()
    return math.fsum((v * v).tolist())


def segment_sumsq(x, segments):
    return [exact_sumsq(x[b:e]) for b, e in segments]


def shape_lengths(piece):
    """The segment lengths at which the kernels change path: empty, below / at / above one 16-byte load, one wave, one workgroup,
    one piece, and several pieces with a ragged end."""
    return [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, piece - 1, piece, piece + 1, 3 * piece + 7]


def shape_segments(piece, first=5):
    """(segments, n): one segment per shape_lengths entry, twice over, so that every length occurs with two begin alignments and
    begins walk through offsets 0, 1, 2, 3 mod 4; gaps of 1..7 elements between segments and at both ends of the n elements."""
    segs, pos = [], first
    for k, n in enumerate(shape_lengths(piece) + shape_lengths(piece)[::-1]):
        pos += (k % 4 - pos) % 4          # begin = k (mod 4)
        segs.append((pos, pos + n))
        pos += n + 1 + (k * 3) % 7
    return segs, pos + 3


def piece_table(segments, piece):
    """The piece table as the host builds it, restated: segment s is cut at begin + k * piece; (pieces, seg_ptr) as lists."""
    pieces, ptr = [], [0]
    for b, e in segments:
        k = 0
        while b + k * piece < e:
            pieces.append((b + k * piece, min(b + (k + 1) * piece, e)))
            k += 1
        ptr.append(len(pieces))
    return pieces, ptr


def check_piece_table(segments, pieces, seg_ptr, piece):
    """Every element of every segment lies in exactly one piece, pieces never cross a segment, a segment's pieces are adjacent
    (consecutive rows, the CSR) and ascending, no piece is empty or longer than `piece`."""
    pieces, seg_ptr = np.asarray(pieces), np.asarray(seg_ptr)
    assert len(seg_ptr) == len(segments) + 1 and seg_ptr[0] == 0 and seg_ptr[-1] == len(pieces)
    for s, (b, e) in enumerate(segments):
        rows = pieces[seg_ptr[s]:seg_ptr[s + 1]]
        if b == e:
            assert len(rows) == 0
            continue
        assert len(rows) >= 1 and rows[0][0] == b and rows[-1][1] == e          # covers the segment's ends, stays inside it
        for k, (pb, pe) in enumerate(rows):
            assert b <= pb < pe <= e and pe - pb <= piece
            if k:
                assert pb == rows[k - 1][1]                                       # adjacent and ascending: no gap, no overlap
    return True


def finalize(seg_sums, grad_scale, max_norm, counters=(0, 0, 0)):
    """m3ae_clip_finalize in float64: (norm, coef, skip, (steps, clipped_steps, skipped_steps)).  norm / coef are the float64
    values the kernel rounds to fp32 once."""
    total = 0.0
    for v in seg_sums:           # ascending index
        total += float(v)
    steps, clipped, skipped = counters
    bad = not (total <= 1.7976931348623157e308)
    norm = math.sqrt(total) * abs(float(np.float32(grad_scale)))     # inf stays inf, nan stays nan
    coef = 0.0 if bad else min(1.0, float(np.float32(max_norm)) / (norm + 1e-6))
    clipped_now = (not bad) and np.float32(coef) < np.float32(1.0)
    return norm, coef, int(bad), (steps + 1, clipped + int(clipped_now), skipped + int(bad))


def adamw(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale, hyper=None):
    """adamw_kernel in float32, operation by operation (no fused multiply-add is assumed anywhere; compare with tolerance, or use
    it for properties).  Returns (p, m, v) as new float32 arrays.  `hyper` = (lr, step_size) replaces the host-computed pair."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f).copy() for a in (p, g, m, v))
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    step_size = f(float(f(lr)) * math.sqrt(bc2) / bc1)
    lr = f(lr)
    if hyper is not None:
        lr, step_size = f(hyper[0]), f(hyper[1])
    b1, b2, eps, wd, gs = f(b1), f(b2), f(eps), f(wd), f(grad_scale)
    gt = g * gs
    m = m * b1 + gt * (f(1.0) - b1)
    v = v * b2 + gt * gt * (f(1.0) - b2)
    denom = np.sqrt(v) + eps
    p = p - step_size * (m / denom)
    if wd > 0:
        p = p - lr * wd * p
    return p.astype(f), m.astype(f), v.astype(f)
