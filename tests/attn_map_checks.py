"""Perf-mode (bf16) bound of an attention map against the reference's, shared by the GPU test and its host-side self-check.

Derivation.  A row of probabilities is p = softmax(s).  If every score of the row moves by at most delta, then for every key
    p'_k / p_k = exp(ds_k) / sum_j p_j exp(ds_j)  lies in  [exp(-2 delta), exp(2 delta)],
so |log p'_k - log p_k| <= 2 delta exactly (not only to first order), and the row's L1 error and the relative error of a map's
Frobenius norm are both at most exp(2 delta) - 1.  The fused cross-attention kernels keep P in bf16 (unit roundoff 2^-8), which
adds 2^-8 to the relative terms.  delta = 0.1: in perf mode every stored activation carries bf16 rounding, the perf-mode bound
this project holds for the head's logits after the towers and six fusion layers is atol 0.05 (tests/test_gpu_model.py), and a
fusion-layer score is a 64-term dot product of two such activations scaled by 1/8; its error is held to twice that.
Entries the reference has at exactly 0 (padding keys, -10000 additive mask) must be exactly 0."""
import math

import numpy as np

DELTA = 0.1
LOG_BOUND = 2 * DELTA + 2.0 ** -8               # |log p - log p_ref| per entry
REL_BOUND = math.exp(2 * DELTA) - 1 + 2.0 ** -8  # row L1 error; relative error of a Frobenius norm


def map_errors(p, ref):
    """(worst |log p - log ref| over the entries, worst row L1 error, zero pattern equal) for arrays [..., Lk]."""
    p, ref = np.asarray(p, np.float64), np.asarray(ref, np.float64)
    live = ref > 0
    if not np.array_equal(live, p > 0):
        return math.inf, math.inf, False
    lr = np.abs(np.log(np.where(live, p, 1.0)) - np.log(np.where(live, ref, 1.0))).max()
    l1 = np.abs(p - ref).sum(-1).max()
    return lr, l1, True


def within_bf16_bound(p, ref):
    lr, l1, zeros = map_errors(p, ref)
    return zeros and lr <= LOG_BOUND and l1 <= REL_BOUND


def fro_within_bound(fro, fro_ref):
    fro, fro_ref = np.asarray(fro, np.float64), np.asarray(fro_ref, np.float64)
    return bool((np.abs(fro - fro_ref) <= REL_BOUND * fro_ref).all())


def uniform_like(ref):
    """The uniform map over the reference's live keys (the answer of a kernel that ignored the scores)."""
    live = (np.asarray(ref) > 0).astype(np.float64)
    return live / live.sum(-1, keepdims=True)


def keys_reversed(ref):
    return np.asarray(ref)[..., ::-1]
