"""numpy model of exhaustive answer-list scoring (csrc/tree_attn.hip, csrc/list_score.hip; include/m3ae_hip.h: m3ae_tree_attn,
m3ae_listscore_lse / _edges / _fold), with float64 references and the bounds the kernels are held to.  Logits and activations are
float32 arrays throughout: bf16 values widen to fp32 exactly.

Tree attention.  The kernel's order of operations (its file header): dot_j = a lane's one or two products, then a 6-stage butterfly
over the 64 lanes; s_j = fmaf(dot_j, scale, bias); m = max s; e_j = expf(s_j - m); den = butterfly sum of e; acc = fma chain over j
ascending; out = acc / den, one rounding to the output dtype.  With u = 2^-24 and gamma(n) = n u / (1 - n u) (Higham: valid for any
summation order of n terms):
    |s_j - S_j|     <= d_j = gamma(Dh) |scale| sum_c |q_c k_jc| + u |S_j|            (dot product, then one fused rounding)
    e_j rel. error  <= eps_j = expm1(d_j + d_max + u |S_j - M|) + 2 u                 (argument perturbation; expf within 2 ulp)
    den rel. error  <= eps_max + gamma(6)
    acc abs. error  <= sum_j E_j |v_j| (eps_j + gamma(n))
    |out - OUT|     <= sum_j P_j |v_j| (2 eps_max + gamma(n) + gamma(6) + 2 u) (1 + 2^-10) + u_out |OUT|
u_out = 2^-8 for a bf16 output (8 significand bits: half an ulp of 2^-7), 0 for fp32 (the division's rounding is the 2 u).  One key: exact.

List scores.  An edge term is fl(x[tok] - lse) with lse as m3ae_trie_step forms it: the per-term bound is
tests/answer_trie_model.py::step_bound (the smaller of its own bound and token_eval_model.nll_bound), and an entry's bound is the sum
of its path's term bounds plus len * 2^-53 |sum| for the float64 additions -- `teacher_forced` of tests/test_gpu_trie_beam.py.
score = logprob / len ** length_penalty adds 2^-53 |score| relative twice (pow by the host in double, one division).
log_mass = M + log(sum exp(lp - M)): given entry bounds b_i, |log_mass - LOG_MASS| <= max_i b_i + A 2^-50 (a log-sum-exp moves by at
most the largest move of a term; the A-term double sum, exp and log are each within a few 2^-53 relative, far inside A 2^-50).
probs = exp(lp - log_mass): absolute error <= P (expm1(b_i + bound(log_mass)) + 2^-50).
Non-finite rules (the file header of csrc/list_score.hip): an entry whose logprob is not finite has probability 0 and adds nothing to
the mass; no finite entry: log_mass = -inf, all probabilities 0; a NaN score ranks after every number, label ascending among NaNs.
Nothing here is a multiple of an observed error.
"""
import numpy as np

import answer_trie_model as AM

U = 2.0 ** -24
MAX_K = 16


def gamma(n):
    return n * U / (1 - n * U)


# ---------------------------------------------------------------------------------------------------------------------------------
# tree attention
# ---------------------------------------------------------------------------------------------------------------------------------
def tree_attn(q, k, v, anc, H, scale, rel_bias=None, out_bf16=False):
    """q, k, v float32 [G, Ni, H * Dh]; anc int32 [Ni, Dmax].  Returns (OUT float64 [G, Ni, H * Dh], bound, err, the largest |score|):
    rows whose anc is out of range are zeros with bound 0 and set err."""
    q64, k64, v64 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (q, k, v))
    G, Ni, D = q64.shape
    Dh = D // H
    out, bound, err, smax = np.zeros((G, Ni, D)), np.zeros((G, Ni, D)), 0, 0.0
    u_out = 2.0 ** -8 if out_bf16 else 0.0
    for i in range(Ni):
        row = anc[i]
        n = int(np.argmax(row < 0)) if (row < 0).any() else len(row)
        path = row[:n]
        if n < 1 or (path >= Ni).any():
            err = 1
            continue
        for g in range(G):
            for h in range(H):
                sl = slice(h * Dh, (h + 1) * Dh)
                K, Vv = k64[g, path, sl], v64[g, path, sl]
                prod = np.abs(q64[g, i, sl][None, :] * K).sum(1)
                S = (q64[g, i, sl][None, :] * K).sum(1) * scale
                if rel_bias is not None:
                    S = S + rel_bias[h, n - 1 - np.arange(n)].astype(np.float64)
                smax = max(smax, float(np.abs(S).max()))
                if n == 1:
                    out[g, i, sl] = Vv[0]
                    continue
                d = gamma(Dh) * abs(scale) * prod + U * np.abs(S)
                M = S.max()
                eps = np.expm1(d + d.max() + U * np.abs(S - M)) + 2 * U
                P = np.exp(S - M)
                P /= P.sum()
                O = (P[:, None] * Vv).sum(0)
                out[g, i, sl] = O
                bound[g, i, sl] = (P[:, None] * np.abs(Vv)).sum(0) * (2 * eps.max() + gamma(n) + gamma(6) + 2 * U) * (1 + 2.0 ** -10) \
                    + u_out * np.abs(O)
    return out, bound, err, smax


# ---------------------------------------------------------------------------------------------------------------------------------
# the edges: per logits row g * Ni + i the terms of the children of internal[i]
# ---------------------------------------------------------------------------------------------------------------------------------
def edges(x, trie, G, chunk=0, itemsize=4):
    """x float32 [G * Ni, V] -> (EDGE float64 [G, E], bound [G, E]).  A -inf logit adds exactly 0 to both sides' sums: the bound of
    the row's other edges is that of the row with -1e30 in its place (every term of the bound that it touches underflows to 0), and
    the edge of that token itself is -inf on both sides.  A row with a NaN or +inf gets term64's value and bound 0 (non-finite
    values are compared for equality by the caller)."""
    t = trie.score_tables()
    E = trie.num_edges
    Ni = len(t["internal"])
    edge, bound = np.zeros((G, E)), np.zeros((G, E))
    for g in range(G):
        for i, n in enumerate(t["internal"]):
            row = np.asarray(x[g * Ni + i], dtype=np.float32)
            lo, hi = int(trie.child_off[n]), int(trie.child_off[n + 1])
            finite = not (np.isnan(row).any() or np.isposinf(row).any())
            rowb = np.where(np.isneginf(row), np.float32(-1e30), row)
            for e in range(lo, hi):
                tok = int(trie.child_tok[e])
                edge[g, e] = AM.term64(row, tok)
                if finite and np.isfinite(row[tok]):
                    bound[g, e] = AM.step_bound(rowb, tok, chunk, itemsize)
    return edge, bound


# ---------------------------------------------------------------------------------------------------------------------------------
# the fold
# ---------------------------------------------------------------------------------------------------------------------------------
def rank_order(score):
    """Labels by (score descending, label ascending), NaN after every number (label ascending among them), -0 == +0."""
    score = np.asarray(score, dtype=np.float64) + 0.0
    nan = np.isnan(score)
    nums = sorted(np.flatnonzero(~nan).tolist(), key=lambda i: (-score[i], i))
    return np.array(nums + np.flatnonzero(nan).tolist(), dtype=np.int64)


def fold(edge, trie, k, length_penalty=0.0, edge_bound=None):
    """edge float [B, E] (the device's fp32 terms, or float64 references) -> the arrays of m3ae_listscore_fold, computed in float64
    by the kernel's definition, and with edge_bound [B, E] the bounds of all_logprob / scores / log_mass / probs."""
    t = trie.score_tables()
    parent, depth, leaf = t["parent"], t["depth"], t["leaf_node"]
    edge = np.asarray(edge, dtype=np.float64)
    B, (N, A) = edge.shape[0], (trie.num_nodes, trie.num_answers)
    node = np.zeros((B, N))
    nb = np.zeros((B, N))
    with np.errstate(all="ignore"):
        for n in range(1, N):                       # a parent precedes its children: node order is level order
            node[:, n] = node[:, parent[n]] + edge[:, n - 1]
            if edge_bound is not None:
                nb[:, n] = nb[:, parent[n]] + edge_bound[:, n - 1]
        lens = depth[leaf].astype(np.int64)
        lp = node[:, leaf]
        lpb = nb[:, leaf] + lens[None, :] * 2.0 ** -53 * np.abs(np.where(np.isfinite(lp), lp, 0))
        pen = lens.astype(np.float64) ** float(length_penalty)
        score = lp / pen[None, :]
        sb = lpb / pen[None, :] + 2 * 2.0 ** -53 * np.abs(np.where(np.isfinite(score), score, 0))
        kk = min(k, A)
        r = dict(all_logprob=lp, all_bound=lpb, all_score=score, all_score_bound=sb, lens=lens,
                 labels=np.full((B, k), -1, dtype=np.int64), scores=np.zeros((B, k)), logprob=np.zeros((B, k)), probs=np.zeros((B, k)),
                 log_mass=np.zeros(B), mass_bound=np.zeros(B), n_hyp=np.full(B, kk, dtype=np.int64), best=np.zeros(B, dtype=np.int64),
                 len=np.zeros(B, dtype=np.int64), order=np.zeros((B, A), dtype=np.int64), all_probs=np.zeros((B, A)),
                 probs_bound=np.zeros((B, A)))
        for b in range(B):
            fin = np.isfinite(lp[b])
            if fin.any():
                M = lp[b][fin].max()
                r["log_mass"][b] = M + np.log(np.exp(lp[b][fin] - M).sum())
                r["mass_bound"][b] = lpb[b][fin].max() + A * 2.0 ** -50
                r["all_probs"][b][fin] = np.exp(lp[b][fin] - r["log_mass"][b])
                r["probs_bound"][b][fin] = r["all_probs"][b][fin] * (np.expm1(lpb[b][fin] + r["mass_bound"][b]) + 2.0 ** -50)
            else:
                r["log_mass"][b] = -np.inf
            order = rank_order(score[b])
            r["order"][b] = order
            top = order[:kk]
            r["labels"][b, :kk], r["scores"][b, :kk], r["logprob"][b, :kk] = top, score[b, top], lp[b, top]
            r["probs"][b, :kk] = r["all_probs"][b, top]
            r["best"][b], r["len"][b] = top[0], lens[top[0]]
    return r


def brute_force(seqs, edge_of, k, length_penalty=0.0):
    """The definition, without the trie: edge_of(prefix tuple, token) -> the term; per answer the sum along it, logsumexp over the
    finite ones, sorted by (score, label).  Returns (logprob [A], score [A], log_mass, order)."""
    lp = np.array([sum(edge_of(tuple(s[:j]), s[j]) for j in range(len(s))) for s in seqs], dtype=np.float64)
    with np.errstate(all="ignore"):
        score = lp / np.array([float(len(s)) ** float(length_penalty) for s in seqs])
    fin = np.isfinite(lp)
    mass = -np.inf
    if fin.any():
        M = lp[fin].max()
        mass = M + np.log(np.exp(lp[fin] - M).sum())
    return lp, score, mass, rank_order(score)


def margins(r, k):
    """Per sample the least of: the adjacent gaps of the first min(k, A) ranking scores and the gap between entry k and k + 1, each
    divided by the sum of the two entries' score bounds (inf where there is no such pair or a score is not finite)."""
    B, A = r["all_score"].shape
    out = np.full(B, np.inf)
    for b in range(B):
        o = r["order"][b]
        for j in range(min(k, A - 1)):
            s0, s1 = r["all_score"][b, o[j]], r["all_score"][b, o[j + 1]]
            if not (np.isfinite(s0) and np.isfinite(s1)):
                continue
            bb = r["all_score_bound"][b, o[j]] + r["all_score_bound"][b, o[j + 1]]
            out[b] = min(out[b], (s0 - s1) / bb if bb > 0 else np.inf)
    return out
