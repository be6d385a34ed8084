"""numpy model of csrc/token_eval.hip: which rows are evaluated, the ranking rule, the label's rank, the top-k, the record and its
fold, and a float64 reference for lse / nll / the probabilities with the fp32 bound the kernel is held to.

The ranking rule is tests/vqa_eval_model.py's (every NaN first, value descending with -0 == +0, column ascending); the label's rank
is its position in that order, i.e. the number of columns ranked strictly above it.

The bound.  The kernel forms lse = m + logf(s) from fp32 pairs (m, s) = (maximum, sum of e(x, m)), e(x, m) = expf(x - m):
  per thread   an element is added as e(x, m_t) at the thread's running maximum m_t; when m_t rises, s is multiplied by e(m_old, m_new);
  per chunk    64 lanes merge in 6 butterfly stages, 4 waves in 3 sequential merges: s' = s1 e(m1, m') + s2 e(m2, m');
  per row      a thread merges its chunks in sequence, then the same 6 + 3 merges.
Every summand is >= 0, so the relative error of s is at most the greatest relative error any one element's term gathers on its
way into s.  Along that way:
  * subtractions.  Each e(a, b) rounds a - b once: a relative error |a - b| u on the factor.  The maxima along one element's way
    only rise, x_j <= m_1 <= m_2 <= ... <= M, so the differences add up to M - x_j = t_j:       t_j u     (u = 2^-24)
  * expf, 1 ulp in the ROCm device library (the figure tests/test_gpu_vqa_eval.py::prob_bound uses), 2 u relative, one per factor;
    a product rounds once (u), a sum rounds once (u).  The count of such operations on the longest way, P(V, chunk, dtype):
        thread:  the term's own expf 2; then at most n_t adds (1 each) and at most v_t rescales (expf + product: 3 each), with
                 v_t = ceil(nvec / 256) + 2 loads of a thread (vector loads, head, tail) and n_t = W ceil(nvec / 256) + 2 elements,
                 W = 16 bytes / element size, nvec <= chunk / W;
        merge:   expf + product + sum = 4, times 6 + 3 per level, two levels;
        row:     ceil(chunks / 256) sequential merges of 4.
    u P relative.
So  |s - S| / S  <=  rel_s = u (sum_j t_j e^-t_j / S  +  P)  +  u^2 sum_j t_j^2 e^-t_j / S,   S = sum_j e^-t_j in float64.
The first term weighs each element's t_j by its share of S (an element far below the maximum has a large t_j and a negligible
share); the last is the second order of e^(t u) - 1 <= t u + (t u)^2 for t u < 1, kept because V elements share it.  A term below
the normal range (t > 87) may be flushed to 0: at most V 2^-126 of S >= 1, far below the slack.
  lse = fl(M + logf(s)):  logf is 1 ulp = 2 u |log s|, moved by rel_s through d(log s) = ds / s;  the sum rounds once: u |lse|.
  nll = fl(lse - x_label):  one more rounding, u |nll|.
      |nll - NLL|  <=  (rel_s + 2 u |log S| + u |LSE| + u |NLL|) (1 + 2^-20)
  topk_prob = expf(fl(x_j - lse)):  the argument is off by the error of lse plus one rounding u |x_j - LSE|; expf adds 2 u relative:
      |p - P_j|  <=  P_j (rel_s + 2 u |log S| + u |LSE| + u |x_j - LSE| + 2 u) (1 + 2^-20) + 2^-126
  (2^-126: below the normal range the result may lose bits or be flushed, as in prob_bound).
The factor (1 + 2^-20) covers the second-order terms (P u < 2^-12 for every shape here) and the float64 reference's own arithmetic.
Nothing here is a multiple of an observed error.
"""
import numpy as np

from vqa_eval_model import rank_row, topk  # noqa: F401  (the ranking rule; topk(x, k) -> int64 [B, k])

IGNORE = -100
REC = 5                      # {n, hit1, hitk, sum_nll, calls}
T = 256                      # threads of the fold
DEF_CHUNK = 8192
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
FLOOR = 2.0 ** -126


def row_states(R, V, labels, select):
    """(evaluated bool [R], labelled bool [R], err): the kernel's row_state for every row."""
    lab = np.full(R, IGNORE, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    if select is not None:
        ev = np.asarray(select) != 0
    elif labels is not None:
        ev = lab != IGNORE
    else:
        ev = np.ones(R, dtype=bool)
    bad = ev & (lab != IGNORE) & ((lab < 0) | (lab >= V))
    ev = ev & ~bad
    return ev, ev & (lab != IGNORE), int(bad.any())


def full_order(x):
    """All columns of one fp32 row in rank order."""
    return rank_row(x, np.asarray(x).shape[0])


def path_units(V, chunk, itemsize):
    """P(V, chunk, dtype) of the module docstring."""
    chunk = DEF_CHUNK if chunk == 0 else chunk
    W = 16 // itemsize
    nvec = min(chunk, V) // W
    loads = -(-nvec // T)
    v_t, n_t = loads + 2, W * loads + 2
    thread = 2 + n_t + 3 * v_t
    merge = 4 * (6 + 3)
    nch = -(-V // chunk)
    return thread + 2 * merge + 4 * (-(-nch // T))


def lse64(x):
    """(LSE, S, M, tsum, t2sum) of one fp32 row with a finite maximum, in float64: S = sum e^-t, tsum = sum t e^-t, t2sum = sum t^2 e^-t,
    t = M - x (a -inf column has e^-t = 0 exactly, in the kernel too, and adds to none of them)."""
    x = np.asarray(x, dtype=np.float64)
    M = x.max()
    fin = np.isfinite(x)
    t = np.where(fin, M - x, 0.0)
    e = np.where(fin, np.exp(-t), 0.0)
    S = e.sum()
    return M + np.log(S), S, M, (t * e).sum(), (t * t * e).sum()


def lse_bound(x, V, chunk, itemsize):
    """(LSE, bound on |lse - LSE| before SLACK) for a finite row."""
    LSE, S, M, tsum, t2sum = lse64(x)
    rel_s = U * (tsum / S + path_units(V, chunk, itemsize)) + U * U * t2sum / S
    return LSE, rel_s + 2 * U * abs(np.log(S)) + U * abs(LSE)


def nll_bound(x, label, chunk, itemsize):
    """(NLL, bound) for a finite fp32 row and its label."""
    x = np.asarray(x, dtype=np.float32)
    LSE, b = lse_bound(x, x.shape[0], chunk, itemsize)
    NLL = LSE - np.float64(x[label])
    return NLL, (b + U * abs(NLL)) * SLACK


def prob_bound(x, cols, chunk, itemsize):
    """(P [k], bound [k]) for the softmax probabilities of `cols` of a finite fp32 row."""
    x = np.asarray(x, dtype=np.float32)
    LSE, b = lse_bound(x, x.shape[0], chunk, itemsize)
    d = x[cols].astype(np.float64) - LSE
    P = np.exp(d)
    return P, P * (b + U * np.where(np.isfinite(d), np.abs(d), 0.0) + 2 * U) * SLACK + FLOOR     # a -inf column: P = 0 exactly


def evaluate(logits, labels=None, select=None, k=0):
    """dict(ev bool [R], pred int64 [R], rank int32 [R], topk int64 [R, k], lse / nll float64 [R] (torch.logsumexp's value for a
    non-finite row), prob float64 [R, k], err 0 / 1).  A row that is not evaluated holds pred -1, rank -1, nll 0, topk -1, prob 0;
    an evaluated row without a label holds rank -1 and nll = lse."""
    x = np.asarray(logits, dtype=np.float32)
    R, V = x.shape
    ev, lab_ok, err = row_states(R, V, labels, select)
    out = {"ev": ev, "labelled": lab_ok, "err": err, "pred": np.full(R, -1, np.int64), "rank": np.full(R, -1, np.int32),
           "topk": np.full((R, k), -1, np.int64), "lse": np.zeros(R), "nll": np.zeros(R), "prob": np.zeros((R, k))}
    for r in np.nonzero(ev)[0]:
        order = full_order(x[r])
        out["pred"][r] = order[0]
        out["topk"][r] = order[:k]
        with np.errstate(all="ignore"):
            row = x[r].astype(np.float64)
            if np.isnan(row).any():
                lse = np.nan
            elif np.isinf(row.max()):
                lse = row.max()              # +inf, or -inf for a row of -inf alone
            else:
                lse = lse64(row)[0]
            out["lse"][r] = lse
            out["prob"][r] = np.exp(row[order[:k]] - lse)
            if lab_ok[r]:
                l = int(labels[r])
                out["rank"][r] = int(np.nonzero(order == l)[0][0])
                out["nll"][r] = lse - row[l]
            else:
                out["nll"][r] = lse
    return out


def fold(rank, nll, k, rec=None):
    """The record after one update from the per-row (rank int32, nll fp32) the kernel wrote, in the fold's fixed order: thread t
    adds rows t, t + 256, ... in float64; the 64 lanes of a wave combine in a butterfly (v += v[lane ^ o], o = 32 .. 1: every
    lane ends with the same bits, addition being commutative); (w0 + w1) + (w2 + w3); then rec += that, rec[4] += 1."""
    rank = np.asarray(rank)
    nll = np.asarray(nll, dtype=np.float32).astype(np.float64)
    rec = np.zeros(REC) if rec is None else np.array(rec, dtype=np.float64)
    acc = np.zeros((4, T))
    for t in range(T):
        for r in range(t, len(rank), T):
            if rank[r] >= 0:
                acc[0, t] += 1.0
                acc[1, t] += 1.0 if rank[r] == 0 else 0.0
                acc[2, t] += 1.0 if rank[r] < k else 0.0
                acc[3, t] = acc[3, t] + nll[r]
    lanes = np.arange(64)
    for i in range(4):
        w = acc[i].reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[:, lanes ^ o]
        rec[i] = rec[i] + ((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0]))
    rec[4] += 1.0
    return rec


def result(rec):
    """What metrics.token_result defines."""
    n = float(rec[0])
    if n == 0:
        return {"accuracy": 0.0, "accuracy_at_k": 0.0, "n": 0, "nll": 0.0, "perplexity": 0.0}
    nll = float(rec[3]) / n
    with np.errstate(over="ignore"):
        return {"accuracy": float(rec[1]) / n, "accuracy_at_k": float(rec[2]) / n, "n": int(n), "nll": nll, "perplexity": float(np.exp(nll))}
