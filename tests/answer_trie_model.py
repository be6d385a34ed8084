"""numpy model of csrc/answer_trie.hip (include/m3ae_hip.h: m3ae_trie_scan, m3ae_trie_step): which child of a row's trie node is
chosen, the same fixed-size state arrays and the same update per step, and a float64 reference for the step's log-probability with
the fp32 bound the kernel is held to.  Logits are float32 arrays throughout: bf16 values widen to fp32 exactly.

The choice.  Among the children of the row's node (m3ae_amd/answer_trie.py: ascending in token) the greatest order key of
tests/greedy_model.py wins: every NaN above every number, value descending with -0 == +0, the lowest token among equals -- torch.argmax
restricted to the allowed columns.  Columns outside the children never take part.

The score.  term = fl(x[tok] - lse), lse = fl(m + logf(s)) from fp32 pairs, added onto a float64 sum.  The kernel's order of
operations is that of csrc/token_eval.hip per thread and per chunk (tests/token_eval_model.py: thread, 6 + 3 merges), but a row's
chunks are folded by ONE thread in ascending chunk order, not by 256 threads and a second tree.  The derivation of
token_eval_model's bound carries over word for word with the path count

    P_trie(V, chunk, dtype) = thread + 4 (6 + 3) + 4 chunks          (token_eval_model: thread + 2 * 4 (6 + 3) + 4 ceil(chunks / 256))

-- a merge is expf + product + sum = 4 units, the element of chunk 0 passes through all `chunks` sequential merges (the first one,
onto (-inf, 0), is exact but counted), and the second 6 + 3 tree does not exist.  Everything else (the t_j u subtraction term, the
second-order term, logf, the two roundings of lse and of the difference, the factor 1 + 2^-20) is token_eval_model.nll_bound's:
    |term - TERM|  <=  (rel_s + 2 u |log S| + u |LSE| + u |TERM|) (1 + 2^-20),  rel_s = u (sum t e^-t / S + P_trie) + u^2 sum t^2 e^-t / S.
For chunks <= 10 this is at most token_eval_model.nll_bound (asserted in tests/test_answer_trie_host.py); with more chunks it is the
larger of the two, because nll_bound counts 4 ceil(chunks / 256) for a fold this kernel does not have.  tests/test_gpu_answer_trie.py
holds every step to BOTH bounds, i.e. to the smaller one in every case.
The float64 sum of `steps` terms adds at most steps * 2^-53 * |sum| (one rounding per addition of numbers of one sign).
Nothing here is a multiple of an observed error.
"""
import numpy as np

import greedy_model as G
import token_eval_model as TM

DEF_CHUNK = 8192
U = TM.U


def children(trie, node):
    lo, hi = int(trie.child_off[node]), int(trie.child_off[node + 1])
    return lo, hi


def choose(trie, node, x):
    """(position within the node's children, token, next node) for one fp32 row x; position -1 when the node has no child range
    or a token is outside the row (the kernel's error path)."""
    N, E = len(trie.leaf_label), len(trie.child_tok)
    if not 0 <= node < N:
        return -1, -1, -1
    lo, hi = children(trie, node)
    if not (0 <= lo < hi <= E):
        return -1, -1, -1
    toks = trie.child_tok[lo:hi].astype(np.int64)
    ok = (toks >= 0) & (toks < x.shape[0])
    if not ok.any():
        return -1, -1, -1
    vals = np.where(ok, x[np.clip(toks, 0, x.shape[0] - 1)], np.float32(0)).astype(np.float32)
    keys = G.keys_of(vals[None, :])[0]                   # the column of a key here is the child position
    keys[~ok] = 0
    p = int(np.uint64(0xffffffff) - (keys.max() & np.uint64(0xffffffff)))
    return p, int(toks[p]), int(trie.child_node[lo + p])


def path_units(V, chunk, itemsize):
    """P_trie of the module docstring."""
    chunk = DEF_CHUNK if chunk == 0 else chunk
    W = 16 // itemsize
    nvec = min(chunk, V) // W
    loads = -(-nvec // TM.T)
    v_t, n_t = loads + 2, W * loads + 2
    return (2 + n_t + 3 * v_t) + 4 * (6 + 3) + 4 * (-(-V // chunk))


def term_bound(x, tok, chunk, itemsize):
    """(TERM = x[tok] - LSE in float64, bound on |term - TERM|) for a finite fp32 row."""
    x = np.asarray(x, dtype=np.float32)
    LSE, S, M, tsum, t2sum = TM.lse64(x)
    rel_s = U * (tsum / S + path_units(x.shape[0], chunk, itemsize)) + U * U * t2sum / S
    TERM = np.float64(x[tok]) - LSE
    return TERM, (rel_s + 2 * U * abs(np.log(S)) + U * abs(LSE) + U * abs(TERM)) * TM.SLACK


def step_bound(x, tok, chunk, itemsize):
    """What a step's term is held to: the smaller of this file's bound and token_eval_model.nll_bound."""
    return min(term_bound(x, tok, chunk, itemsize)[1], TM.nll_bound(x, tok, chunk, itemsize)[1])


def term64(x, tok):
    """The step's log-probability in float64, with torch.log_softmax's value for a non-finite row."""
    row = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if np.isnan(row).any():
            lse = np.nan
        elif np.isinf(row.max()):
            lse = row.max()              # +inf, or -inf for a row of -inf alone
        else:
            lse = TM.lse64(row)[0]
        return row[tok] - lse


class State:
    """The arrays of ops.TrieState."""

    def __init__(self, B, max_len, start_id=101, pad_id=0):
        self.B, self.max_len = B, max_len
        self.seq = np.full((B, max_len), pad_id, dtype=np.int64)
        self.len = np.full(B, max_len, dtype=np.int64)
        self.label = np.full(B, -1, dtype=np.int64)
        self.score = np.zeros(B, dtype=np.float64)
        self.bound = np.zeros(B, dtype=np.float64)       # the sum of the per-step bounds of the finite steps
        self.terms = [[] for _ in range(B)]
        self.err = np.zeros(1, dtype=np.int64)
        self.last_tok = np.full(B, start_id, dtype=np.int64)
        self.node = np.zeros(B, dtype=np.int32)
        self.finished = np.zeros(B, dtype=np.int32)
        self.open_count = np.zeros(max_len, dtype=np.int32)


def step(st, trie, x, pos, pad_id, chunk=0, itemsize=4):
    """One m3ae_trie_scan + m3ae_trie_step on logits x float32 [B, V]."""
    x = np.asarray(x, dtype=np.float32)
    for r in range(st.B):
        if st.finished[r]:
            st.seq[r, pos] = pad_id
            continue
        p, tok, nn = choose(trie, int(st.node[r]), x[r])
        if p < 0 or not 0 <= nn < len(trie.leaf_label):
            st.err[0] = 1
            st.last_tok[r] = 0
            st.seq[r, pos] = 0
            continue
        t = term64(x[r], tok)
        st.score[r] += t
        st.terms[r].append(t)
        if np.isfinite(x[r]).all():
            st.bound[r] += step_bound(x[r], tok, chunk, itemsize)
        st.last_tok[r] = tok
        st.seq[r, pos] = tok
        st.node[r] = nn
        lab = int(trie.leaf_label[nn])
        if lab >= 0:
            st.label[r] = lab
            st.len[r] = pos + 1
            st.finished[r] = 1
    st.open_count[pos] = int((st.finished == 0).sum())


def search(logits_of, trie, B, max_len, start_id, pad_id, chunk=0, itemsize=4, stop_early=True):
    """The whole search: logits_of(last_tok int64 [B], pos) -> float32 [B, V].  Returns the final State and the steps run."""
    st = State(B, max_len, start_id, pad_id)
    steps = 0
    for pos in range(trie.depth):
        step(st, trie, logits_of(st.last_tok.copy(), pos), pos, pad_id, chunk, itemsize)
        steps += 1
        if stop_early and st.open_count[pos] == 0:
            break
    return st, steps


def brute_force_token(sequences, prefix, x):
    """The definition: among the list entries that extend `prefix`, the next tokens allowed; of those the one with the greatest
    logit, the lowest id among equals (finite rows)."""
    n = len(prefix)
    allowed = sorted({s[n] for s in sequences if len(s) > n and tuple(s[:n]) == tuple(prefix)})
    best = allowed[0]
    for t in allowed[1:]:
        if x[t] > x[best]:
            best = t
    return best
