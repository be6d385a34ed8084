"""numpy model of csrc/vqa_eval.hip: the ranking rule, the per-row hits, the record and the token subsequence match.

The rule is stated without the kernel's 64-bit key, as a three-level sort of a row's columns:
    1. every NaN (either sign) before every number;
    2. value descending, -0 == +0 (numpy's float compare);
    3. column ascending.
Rank 0 is torch.max(x, 1)[1] / torch.argmax on CPU (checked in tests/test_vqa_eval_host.py), ranks 0 .. k - 1 are the top-k.
The record is float64 [10]: {n, sum_top1, sum_topk} of (all, closed, open), then the number of updates (include/m3ae_hip.h).
"""
import numpy as np

ANS_CLOSED, ANS_OPEN = 0, 1      # my_metrics.py:180-181
REC = 10


def rank_row(x, k):
    """The columns of ranks 0 .. k - 1 of one fp32 row."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    val = np.where(nan, np.float32(0), x).astype(np.float64)
    order = np.lexsort((np.arange(x.shape[0]), -val, ~nan))    # last key first: NaN, then value descending, then column
    return order[:k]


def topk(x, k):
    """int64 [B, k] for fp32 rows [B, C]."""
    x = np.asarray(x, dtype=np.float32)
    return np.stack([rank_row(r, k) for r in x]).astype(np.int64).reshape(x.shape[0], k)


def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def evaluate(logits, targets, types, k, ranks=None):
    """-> dict(pred int64 [B], topk int64 [B, k], prob float64 [B, k], hit1 fp32 [B], hitk fp32 [B], rec float64 [10]: the
    increment of one update).  hit1 / hitk / rec are None without targets.  hitk with k = 0 is 0 (the maximum over no column).
    ranks: topk(logits, k') with k' >= max(k, 1) computed earlier (the top-k is its prefix), to rank a batch once for several k."""
    x = np.asarray(logits, dtype=np.float32)
    B = x.shape[0]
    ranks = topk(x, max(k, 1)) if ranks is None else ranks[:, :max(k, 1)]
    out = {"pred": ranks[:, 0].copy(), "topk": ranks[:, :k], "prob": sigmoid64(np.take_along_axis(x, ranks[:, :k], 1)),
           "hit1": None, "hitk": None, "rec": None}
    if targets is None:
        return out
    t = np.asarray(targets, dtype=np.float32)
    hit1 = t[np.arange(B), ranks[:, 0]]
    hitk = np.take_along_axis(t, ranks[:, :k], 1).max(axis=1) if k > 0 else np.zeros(B, dtype=np.float32)
    out["hit1"], out["hitk"], out["rec"] = hit1, hitk, record(hit1, hitk, types)
    return out


def record(hit1, hitk, types):
    """The increment of one update, summed in float64 in row order (any order gives the same bits under the exactness
    condition of tests/test_vqa_eval_host.py)."""
    rec = np.zeros(REC, dtype=np.float64)
    ty = np.full(len(hit1), -1) if types is None else np.asarray(types)
    for g, sel in enumerate((np.ones(len(hit1), dtype=bool), ty == ANS_CLOSED, ty == ANS_OPEN)):
        rec[3 * g] = float(sel.sum())
        for h1, hk in zip(np.asarray(hit1, dtype=np.float64)[sel], np.asarray(hitk, dtype=np.float64)[sel]):
            rec[3 * g + 1] += h1
            rec[3 * g + 2] += hk
    rec[9] = 1.0
    return rec


def result(rec):
    """What metrics.record_result defines: score / closed / open = sum_top1 / n of the group, 0.0 for an empty group."""
    def ratio(a, b):
        return float(a) / float(b) if b != 0 else 0.0
    return {"score": ratio(rec[1], rec[0]), "closed": ratio(rec[4], rec[3]), "open": ratio(rec[7], rec[6]),
            "score_at_k": ratio(rec[2], rec[0]), "n": int(rec[0]), "n_closed": int(rec[3]), "n_open": int(rec[6])}


def seq_match(gen, ref, skip):
    """int32 [B]: 1 where the ids of gen[r] outside `skip` equal, in order, the ids of ref[r] outside `skip`."""
    skip = set(int(s) for s in skip)
    out = []
    for g, f in zip(np.asarray(gen).tolist(), np.asarray(ref).tolist()):
        out.append(int([t for t in g if t not in skip] == [t for t in f if t not in skip]))
    return np.array(out, dtype=np.int32)


def match_record(match, types):
    m = np.asarray(match, dtype=np.float32)
    return record(m, m, types)


def special_rows(C, rng):
    """fp32 rows [n, C] that exercise the rule: ties, a tie with the maximum, all-equal, +-0, +-inf, one and several NaNs (both
    signs).  Needs C >= 1; entries that need more columns than C are clipped to the columns there are."""
    def col(i):
        return min(i, C - 1)
    base = rng.standard_normal(C).astype(np.float32)
    rows = []
    r = base.copy(); r[col(3)] = r[col(1)] = np.float32(0.25); rows.append(r)                       # a tie below the maximum
    r = base.copy(); r[col(4)] = r[col(2)] = np.float32(9.0); rows.append(r)                        # a tie with the maximum
    rows.append(np.full(C, np.float32(-1.5)))                                                      # all equal
    r = np.full(C, np.float32(-3.0)); r[col(2)] = np.float32(-0.0); r[col(5)] = np.float32(0.0); rows.append(r)   # -0 before +0: -0 wins
    r = np.full(C, np.float32(-3.0)); r[col(1)] = np.float32(0.0); r[col(4)] = np.float32(-0.0); rows.append(r)   # +0 before -0
    r = base.copy(); r[col(0)] = -np.inf; r[col(3)] = np.inf; r[col(5)] = np.inf; rows.append(r)   # +-inf, +inf twice
    rows.append(np.full(C, -np.inf, dtype=np.float32))                                             # all -inf
    r = base.copy(); r[col(4)] = np.nan; r[col(0)] = np.inf; rows.append(r)                        # one NaN beats +inf
    r = base.copy(); r[col(5)] = np.nan; r[col(2)] = np.nan; r[col(6)] = np.nan; rows.append(r)    # several NaNs: the first first
    r = base.copy(); r[col(3)] = np.float32(np.nan); rows.append(r)
    neg_nan = np.array([0xffc00001], dtype=np.uint32).view(np.float32)[0]
    r = base.copy(); r[col(1)] = neg_nan; r[col(6)] = np.nan; rows.append(r)                        # a negative NaN ranks as a NaN
    return np.stack(rows).astype(np.float32)
