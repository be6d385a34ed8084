"""numpy model of csrc/trie_beam.hip (include/m3ae_hip.h: m3ae_triebeam_select, m3ae_triebeam_step): the candidate selection over
the children of a sample's live beams, the BeamSearchScorer step with a trie node per beam, the same fixed-size state arrays, the
hypothesis lists and the open counts.  Logits are float32 arrays throughout: bf16 values widen to fp32 exactly.

Order of operations of the device, per candidate (child entry e of live beam k of a sample, token tok):
    lse   = fl(m + logf(s))                       the (m, s) pairs of m3ae_trie_scan folded in ascending chunk order (fp32)
    term  = fl(x[tok] - lse)
    score = fl(term + beam_score[k])              beam_score = the score of the candidate that became this beam (fp32), 0 at the root
Kept: the best min(2 nb, candidates) by (rounded score descending with -0 == +0 and any NaN first, beam ascending, entry ascending).
The step walks the ranks: a leaf at rank >= nb is skipped, a leaf at rank < nb pushes (score / div, score, label, pos + 1) into the
hypothesis list (descending, after equal scores, cut to nb), the others fill the beam slots.  Done: nb hypotheses or no live beam.

Two ways to run the model:
  * lse=None: float64.  Scores are X[tok] - LSE + SCORE_of_the_beam in float64, with no fp32 rounding anywhere.  What it predicts for
    the device is exact in every integer PROVIDED the decision margin below is larger than the error bound; the tests assert that.
  * lse=fp32 array [R]: the device's arithmetic, fl(fl(x - lse) + beam_score) in float32, bit for bit given these lse inputs.

The derived bound.  With TERM = X[tok] - LSE in float64, tests/answer_trie_model.py::term_bound gives |term - TERM| <= tb (the scan
is m3ae_trie_scan itself and the fold of the pairs is m3ae_trie_step's: the same path count P_trie, the roundings of lse and of the
difference included).  The second addition rounds once: score = (term + beam_score)(1 + d), |d| <= u = 2^-24.  With err_k the bound
on |score_k - SCORE_k| after k accumulated steps along a beam's history,
    |score_k - SCORE_k| <= err_(k-1) + tb_k + u |score_k|  and  u |score_k| <= u (|SCORE_k| + err_k),  so
    err_k = (err_(k-1) + tb_k + u |SCORE_k|) (1 + 2^-20),     err_0 = 0
(the factor absorbs the second-order term u err_k, since 1 / (1 - u) < 1 + 2^-20).  That is token_eval's per-term bound plus one fp32
rounding per accumulated step.  The first step adds onto +0 exactly; it is counted all the same.  Nothing here is a multiple of an
observed error.  A hypothesis' logprob is (double)score: the same bound; its normalised score divides both by div (one float64
rounding, 2^-53 relative, below everything above).

The decision margin of a step: the smallest float64 gap between two candidates whose relative order matters -- adjacent ranks within
the kept set, and the last kept against the first dropped -- over the samples of the step.  Pairs that tie structurally are excluded:
the same beam and identical logit bits, whose device scores are bit-equal, so that the index rule decides on both sides.  `hyp_ratio`
is the same idea for the hypothesis lists: the smallest |new - old| / (bound_new + bound_old) over every push against every entry it
is compared with, all normalised.  A test may rely on the model's integers where margin >= 8 * bound and hyp_ratio >= 8.
"""
import numpy as np

import answer_trie_model as AM
import token_eval_model as TM

U = TM.U
MAX_BEAMS = 8


class RowStats:
    """The float64 quantities of one finite fp32 row that every candidate of the row shares."""

    def __init__(self, x, chunk, itemsize):
        self.LSE, S, _, tsum, t2sum = TM.lse64(x)
        rel_s = U * (tsum / S + AM.path_units(x.shape[0], chunk, itemsize)) + U * U * t2sum / S
        self.base = rel_s + 2 * U * abs(np.log(S)) + U * abs(self.LSE)

    def term_bound(self, TERM):
        return (self.base + U * abs(TERM)) * TM.SLACK          # answer_trie_model.term_bound


class State:
    """The arrays of ops.TrieBeamState; scores in float64."""

    def __init__(self, B, nb, max_len, start_id=101, pad_id=0):
        assert 1 <= nb <= MAX_BEAMS
        R = B * nb
        self.B, self.nb, self.max_len, self.pad_id = B, nb, max_len, pad_id
        self.node = np.full((B, nb), -1, dtype=np.int32)
        self.node[:, 0] = 0
        self.node = self.node.reshape(-1)
        self.beam_score = np.zeros(R, dtype=np.float64)
        self.beam_err = np.zeros(R, dtype=np.float64)            # the derived bound of each beam_score
        self.last_tok = np.full((B, nb), pad_id, dtype=np.int64)
        self.last_tok[:, 0] = start_id
        self.last_tok = self.last_tok.reshape(-1)
        self.order = np.repeat(np.arange(B, dtype=np.int64) * nb, nb)
        self.dead = (self.node < 0).astype(np.int32)
        self.done = np.zeros(B, dtype=np.int32)
        self.n_hyp = np.zeros(B, dtype=np.int64)
        self.labels = np.full((B, nb), -1, dtype=np.int64)
        self.scores = np.zeros((B, nb), dtype=np.float64)
        self.logprob = np.zeros((B, nb), dtype=np.float64)
        self.hyp_err = np.zeros((B, nb), dtype=np.float64)       # the derived bound of each logprob
        self.hyp_nerr = np.zeros((B, nb), dtype=np.float64)      # ... and of each normalised score
        self.hyp_len = np.zeros((B, nb), dtype=np.int64)
        self.best = np.zeros(B, dtype=np.int64)
        self.len = np.zeros(B, dtype=np.int64)
        self.open_count = np.zeros(max_len, dtype=np.int32)
        self.err = np.zeros(1, dtype=np.int64)
        K = 2 * nb
        self.top_s = np.zeros((B, K), dtype=np.float64)
        self.top_err = np.zeros((B, K), dtype=np.float64)
        self.top_beam = np.full((B, K), -1, dtype=np.int32)
        self.top_edge = np.full((B, K), -1, dtype=np.int32)
        self.n_cand = np.zeros(B, dtype=np.int32)
        self.margin, self.bound, self.hyp_ratio = [], [], []     # per step


def _rank_key(c):
    s, beam, edge = c[0], c[1], c[2]
    return (0, 0.0, beam, edge) if s != s else (1, -(s + 0.0), beam, edge)


def select(st, trie, x, chunk=0, itemsize=4, lse=None):
    """One m3ae_triebeam_select on logits x float32 [B * nb, V].  Returns (margin, bound) of the step: the smallest decision gap
    and the largest candidate bound over the samples (inf / 0 when nothing is compared)."""
    x = np.asarray(x, dtype=np.float32)
    N, E, V = len(trie.leaf_label), len(trie.child_tok), x.shape[1]
    nb, K = st.nb, 2 * st.nb
    margin, bound = np.inf, 0.0
    for b in range(st.B):
        cands = []                                               # (score, beam, edge, err, logit bits)
        for k in range(nb):
            r = b * nb + k
            nd = int(st.node[r])
            if nd < 0:
                continue
            lo, hi = (int(trie.child_off[nd]), int(trie.child_off[nd + 1])) if nd < N else (0, 0)
            if not (nd < N and 0 <= lo < hi <= E):
                st.err[0] = 1
                continue
            finite = bool(np.isfinite(x[r]).all())
            rs = RowStats(x[r], chunk, itemsize) if lse is None and finite else None
            for e in range(lo, hi):
                tok = int(trie.child_tok[e])
                if not 0 <= tok < V:
                    st.err[0] = 1
                    continue
                if lse is not None:
                    s = np.float32(np.float32(x[r, tok] - np.float32(lse[r])) + np.float32(st.beam_score[r]))
                    er = 0.0
                elif rs is not None:
                    TERM = np.float64(x[r, tok]) - rs.LSE
                    s = TERM + st.beam_score[r]
                    er = (st.beam_err[r] + rs.term_bound(TERM) + U * abs(s)) * TM.SLACK
                else:
                    s = AM.term64(x[r], tok) + st.beam_score[r]
                    er = np.inf
                cands.append((float(s), k, e, er, int(x[r, tok].view(np.uint32))))
        cands.sort(key=_rank_key)
        kept = cands[:K]
        for j, (a, c) in enumerate(zip(cands[:K], cands[1:K + 1])):
            if a[1] == c[1] and a[4] == c[4]:
                continue                                         # a structural tie: the index rule decides
            margin = min(margin, abs(a[0] - c[0]))
        for c in cands[:K + 1]:
            bound = max(bound, c[3])
        st.n_cand[b] = len(kept)
        st.top_s[b], st.top_err[b], st.top_beam[b], st.top_edge[b] = 0.0, 0.0, -1, -1
        for j, c in enumerate(kept):
            st.top_s[b, j], st.top_beam[b, j], st.top_edge[b, j], st.top_err[b, j] = c[0] + 0.0, c[1], c[2], c[3]
    st.margin.append(margin)
    st.bound.append(bound)
    return margin, bound


def _push(st, b, score, raw, err, div, lab, length, ratio):
    nb, n = st.nb, int(st.n_hyp[b])
    hs = st.scores[b]
    for q in range(n):                                           # every entry the new score is compared with
        den = err / div + st.hyp_nerr[b, q]
        if den > 0:
            ratio = min(ratio, abs(score - hs[q]) / den)
    p = 0
    while p < n and not (hs[p] < score):
        p += 1
    if p >= nb:
        return ratio
    last = n if n < nb else nb - 1
    for arr in (st.scores, st.logprob, st.labels, st.hyp_len, st.hyp_err, st.hyp_nerr):
        arr[b, p + 1:last + 1] = arr[b, p:last].copy()
    st.scores[b, p], st.logprob[b, p], st.labels[b, p], st.hyp_len[b, p] = score, raw, lab, length
    st.hyp_err[b, p], st.hyp_nerr[b, p] = err, err / div
    st.n_hyp[b] = n + 1 if n < nb else n
    return ratio


def step(st, trie, V, pos, length_penalty=0.0):
    """One m3ae_triebeam_step on the candidates `select` left in st.  Returns the step's hyp_ratio."""
    N, E, A = len(trie.leaf_label), len(trie.child_tok), trie.num_answers
    nb, K = st.nb, 2 * st.nb
    div = float(pos + 1) ** length_penalty
    ratio = np.inf
    open_ = 0
    for b in range(st.B):
        new = []
        done = bool(st.done[b])
        if not done:
            old_node = st.node[b * nb:(b + 1) * nb].copy()
            for rank in range(K):
                if len(new) >= nb:
                    break
                e, bm = int(st.top_edge[b, rank]), int(st.top_beam[b, rank])
                if e == -1 and bm == -1:
                    continue
                if not (0 <= bm < nb and 0 <= e < E):
                    st.err[0] = 1
                    continue
                nd = int(old_node[bm])
                lo, hi = (int(trie.child_off[nd]), int(trie.child_off[nd + 1])) if 0 <= nd < N else (0, 0)
                if not (0 <= nd < N and 0 <= lo < hi <= E and lo <= e < hi):
                    st.err[0] = 1
                    continue
                tok, nn = int(trie.child_tok[e]), int(trie.child_node[e])
                if not (0 <= tok < V and 0 <= nn < N):
                    st.err[0] = 1
                    continue
                s, er = st.top_s[b, rank], st.top_err[b, rank]
                lab = int(trie.leaf_label[nn])
                if lab >= A:
                    st.err[0] = 1
                    continue
                if lab >= 0:
                    if rank >= nb:
                        continue
                    ratio = _push(st, b, s / div, s, er, div, lab, pos + 1, ratio)
                else:
                    new.append((s, tok, b * nb + bm, nn, er))
            if st.n_hyp[b] > 0:
                st.best[b] = max(int(st.labels[b, 0]), 0)
                st.len[b] = st.hyp_len[b, 0]
            done = st.n_hyp[b] >= nb or not new
            if done:
                st.done[b] = 1
                new = []
        for j in range(nb):
            r = b * nb + j
            if j < len(new):
                st.beam_score[r], st.last_tok[r], st.order[r], st.node[r], st.beam_err[r] = new[j]
                st.dead[r] = 0
            else:
                st.beam_score[r], st.last_tok[r], st.order[r], st.node[r], st.beam_err[r] = 0.0, st.pad_id, b * nb, -1, 0.0
                st.dead[r] = 1
        open_ += 0 if done else 1
    st.open_count[pos] = open_
    st.hyp_ratio.append(ratio)
    return ratio


def search(logits_of, trie, B, nb, max_len, start_id, pad_id, length_penalty=0.0, chunk=0, itemsize=4, stop_early=True):
    """The whole search: logits_of(last_tok int64 [R], order int64 [R] or None, pos) -> float32 [R, V] (order: the re-ordering
    of the cached rows since the previous call).  Returns the final State and the steps run."""
    st = State(B, nb, max_len, start_id, pad_id)
    steps, order = 0, None
    for pos in range(trie.depth):
        x = np.asarray(logits_of(st.last_tok.copy(), order, pos), dtype=np.float32)
        select(st, trie, x, chunk, itemsize)
        step(st, trie, x.shape[1], pos, length_penalty)
        order = st.order.copy()
        steps += 1
        if stop_early and st.open_count[pos] == 0:
            break
    return st, steps


def answers_seq(trie, st):
    """seq int64 [B, max_len] of the best hypotheses (the device gathers it from the pad-filled answers table)."""
    return trie.answers_table(st.max_len, st.pad_id)[st.best]


def brute_force(sequences, row_of, length_penalty=0.0):
    """The definition on a closed list: for every entry a_i the float64 sum of log p(a_i[t] | a_i[<t]) from row_of(prefix tuple) ->
    float32 [V], and its normalised score sum / len ** length_penalty.  Returns (logprob [A], score [A])."""
    lp, sc = [], []
    for s in sequences:
        tot = 0.0
        for t in range(len(s)):
            tot += AM.term64(row_of(tuple(s[:t])), s[t])
        lp.append(tot)
        sc.append(tot / float(len(s)) ** length_penalty)
    return np.asarray(lp), np.asarray(sc)
