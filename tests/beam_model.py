"""numpy model of the three beam-search kernels of csrc/beam.hip (include/m3ae_hip.h: m3ae_beam_topk, m3ae_beam_step,
m3ae_beam_finalize): the same fixed-size state arrays, the same update order, fp32 score arithmetic and the order key
(rounded fp32 score descending, flat index beam * V + token ascending).  Also the scripted logits the beam tests share."""
import numpy as np

F32 = np.float32


def ulp32(x):
    return float(np.spacing(F32(abs(x))))


def tau(score, spread):
    """Tolerance of one fp32 candidate score against float64: three correctly rounded fp32 operations on magnitudes up to
    M = max(1, |score|, max|x - m|) give <= 1.5 ulp32(M); the log of a V-term fp32 sum gives <= (log2 V + 2) 2^-24 ~ 1e-6 at
    V = 32128; both with x2 to x3 headroom."""
    return 4.0 * ulp32(max(1.0, abs(float(score)), float(spread))) + 2e-6


def topk(logits, beam_scores, B, nb):
    """logits fp32 [B * nb, V], beam_scores fp32 [B * nb] -> top_s fp32 [B, 2 nb], top_i int32 [B, 2 nb]."""
    x = np.asarray(logits, dtype=F32)
    V = x.shape[1]
    m = x.max(axis=1, keepdims=True)
    d = (x - m).astype(F32)
    lse = np.log(np.exp(d.astype(np.float64)).sum(axis=1, keepdims=True)).astype(F32)
    sc = ((d - lse).astype(F32) + np.asarray(beam_scores, dtype=F32)[:, None]).astype(F32).reshape(B, nb * V)
    top_i = np.argsort(-sc, axis=1, kind="stable")[:, :2 * nb]          # stable: ties in ascending flat index
    return np.take_along_axis(sc, top_i, axis=1), top_i.astype(np.int32)


def reference_topk(logits, beam_scores, B, nb, k):
    """float64 log-softmax + beam score, stable sort: values [B, k], indices [B, k], and max |x - m| per sample."""
    x = np.asarray(logits, dtype=np.float64)
    V = x.shape[1]
    m = x.max(axis=1, keepdims=True)
    lp = x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    sc = (lp + np.asarray(beam_scores, dtype=np.float64)[:, None]).reshape(B, nb * V)
    idx = np.argsort(-sc, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(sc, idx, axis=1), idx, np.abs(x - m).reshape(B, -1).max(axis=1)


def live_gaps_ok(vals, spread):
    """The validity condition of a case: consecutive reference values differ by at least 2 tau.  vals [k], descending."""
    for a, b in zip(vals[:-1], vals[1:]):
        if a - b < 2.0 * max(tau(a, spread), tau(b, spread)):
            return False
    return True


class State:
    def __init__(self, B, nb, max_length, start_id=0, pad_id=0):
        R = B * nb
        self.B, self.nb, self.max_length = B, nb, max_length
        self.ids = np.full((2, R, max_length), pad_id, dtype=np.int64)
        self.ids[0, :, 0] = start_id
        self.cur = 0
        self.last_tok = np.full(R, start_id, dtype=np.int64)
        bs = np.zeros((B, nb), dtype=F32)
        bs[:, 1:] = -1e9
        self.beam_scores = bs.reshape(-1)
        self.order = np.zeros(R, dtype=np.int64)
        self.done = np.zeros(B, dtype=np.int32)
        self.n_hyp = np.zeros(B, dtype=np.int32)
        self.hyp_score = np.zeros((B, nb), dtype=np.float64)
        self.hyp_len = np.zeros((B, nb), dtype=np.int32)
        self.hyp_tok = np.zeros((B, nb, max_length), dtype=np.int64)
        self.open_count = np.zeros(max_length, dtype=np.int32)
        self.err = np.zeros(1, dtype=np.int64)
        self.seq = np.zeros((B, max_length), dtype=np.int64)
        self.len = np.zeros(B, dtype=np.int64)
        self.events = set()      # what the walk met: "eos_low_rank", "overflow", "open_at_end", ("done_at", step)

    def _push(self, b, score, row, length):
        nb, n = self.nb, int(self.n_hyp[b])
        hs, hl, ht = self.hyp_score[b], self.hyp_len[b], self.hyp_tok[b]
        p = 0
        while p < n and not (hs[p] < score):
            p += 1
        if n == nb:
            self.events.add("overflow")
        if p >= nb:
            return
        last = n if n < nb else nb - 1
        for q in range(last, p, -1):
            hs[q], hl[q], ht[q] = hs[q - 1], hl[q - 1], ht[q - 1]
        hs[p], hl[p] = score, length
        ht[p] = 0
        ht[p, :length] = row[:length]
        self.n_hyp[b] = min(n + 1, nb)


def step(st, top_s, top_i, V, cur_len, eos_id, pad_id, length_penalty=1.0):
    B, nb, ml = st.B, st.nb, st.max_length
    src_ids, dst_ids = st.ids[st.cur], st.ids[1 - st.cur]
    div = float(cur_len) ** length_penalty
    for b in range(B):
        src = np.full(nb, b * nb, dtype=np.int64)
        tok = np.full(nb, pad_id, dtype=np.int64)
        sc = np.zeros(nb, dtype=F32)
        if not st.done[b]:
            k = 0
            for rank in range(2 * nb):
                if k >= nb:
                    break
                i = int(top_i[b, rank])
                if i < 0 or i >= nb * V:
                    st.err[0] = 1
                    continue
                s_row, t = b * nb + i // V, i % V
                if t == eos_id:
                    if rank >= nb:
                        st.events.add("eos_low_rank")
                        continue
                    st._push(b, float(top_s[b, rank]) / div, src_ids[s_row], cur_len)
                else:
                    sc[k], tok[k], src[k] = top_s[b, rank], t, s_row
                    k += 1
            if st.n_hyp[b] >= nb:
                st.done[b] = 1
                st.events.add(("done_at", cur_len))
        rows = slice(b * nb, (b + 1) * nb)
        st.beam_scores[rows], st.order[rows], st.last_tok[rows] = sc, src, tok
        for k in range(nb):
            dst_ids[b * nb + k, :cur_len] = src_ids[src[k], :cur_len]
            dst_ids[b * nb + k, cur_len] = tok[k]
    st.open_count[cur_len] = int((st.done == 0).sum())
    st.cur = 1 - st.cur


def finalize(st, cur_len, eos_id, pad_id, length_penalty=1.0, len_offset=0):
    B, nb, ml = st.B, st.nb, st.max_length
    ids = st.ids[st.cur]
    div = float(cur_len - len_offset) ** length_penalty
    for b in range(B):
        if not st.done[b]:
            st.events.add("open_at_end")
            for j in range(nb):
                st._push(b, float(st.beam_scores[b * nb + j]) / div, ids[b * nb + j], cur_len)
        n = int(st.hyp_len[b, 0])
        st.len[b] = n
        st.seq[b] = pad_id
        st.seq[b, :n] = st.hyp_tok[b, 0, :n]
        if n < ml:
            st.seq[b, n] = eos_id
    return st.seq, st.len


def trimmed(seq, length, max_length):
    """generate's return value: the first min(max len + 1, max_length) columns."""
    return seq[:, :min(int(length.max()) + 1, max_length)]


# ---- scripted logits -------------------------------------------------------------------------------------------------------------
def tables(V, nb, max_length, eos_bias, B, seed, eos_id=1):
    """L(t, r, :) = T1[t, r, :] + T2[last_token(r), :], seeded ~ N(0, 1.4^2), EOS column of T1 raised by eos_bias."""
    rng = np.random.default_rng(seed)
    T1 = (rng.standard_normal((max_length, B * nb, V)) * 1.4).astype(F32)
    T2 = (rng.standard_normal((V, V)) * 1.4).astype(F32)
    T1[:, :, eos_id] += F32(eos_bias)
    return T1, T2


def scripted_logits(T1, T2, t, last_tok):
    return (T1[t] + T2[np.asarray(last_tok)]).astype(F32)


def search(T1, T2, B, nb, max_length, eos_id=1, pad_id=0, length_penalty=1.0, len_offset=0, on_step=None, stop_early=True):
    """The whole search on the model.  on_step(st, cur_len, logits, top_s, top_i, was_done) after every step."""
    V = T1.shape[-1]
    st = State(B, nb, max_length, 0, pad_id)
    cur_len = 1
    while cur_len < max_length:
        logits = scripted_logits(T1, T2, cur_len - 1, st.last_tok)
        was_done = st.done.copy()
        bs_in = st.beam_scores.copy()
        top_s, top_i = topk(logits, bs_in, B, nb)
        step(st, top_s, top_i, V, cur_len, eos_id, pad_id, length_penalty)
        if on_step is not None:
            on_step(st, cur_len, logits, bs_in, top_s, top_i, was_done)
        cur_len += 1
        if stop_early and st.done.all():
            break
    finalize(st, cur_len, eos_id, pad_id, length_penalty, len_offset)
    return st


# ---- the scripted cases the CPU and GPU beam tests share ---------------------------------------------------------------------------
# (V, nb, max_length, eos_bias) -> seed.  A seed is valid only if, at every step and for every sample not yet done, consecutive
# values among the float64 reference's top 2 nb + 1 differ by at least 2 tau (torch.topk leaves ties unspecified; done samples have
# nb identical rows, tie exactly and are ignored by every implementation).  The seeds were chosen to meet that; validate() asserts it.
SCRIPTED_B = 6
SCRIPTED = {(9, 4, 8, 1.0): 0, (9, 4, 8, 2.5): 0, (37, 4, 12, 3.0): 0, (1001, 4, 12, 6.0): 0, (37, 2, 6, 3.0): 0, (37, 1, 6, 3.0): 0,
            (64, 8, 10, 4.0): 0}


def validate(case, seed, B=SCRIPTED_B):
    """Runs the model's search on a scripted case; returns (state, minimum live gap / (2 tau) over the search)."""
    V, nb, ml, eos_bias = case
    T1, T2 = tables(V, nb, ml, eos_bias, B, seed)
    worst = [np.inf]

    def on_step(st, cur_len, logits, bs_in, top_s, top_i, was_done):
        vals, _, spread = reference_topk(logits, bs_in, B, nb, 2 * nb + 1)
        for b in range(B):
            if was_done[b]:
                continue
            for a, c in zip(vals[b, :-1], vals[b, 1:]):
                worst[0] = min(worst[0], (a - c) / (2.0 * max(tau(a, spread[b]), tau(c, spread[b]))))

    st = search(T1, T2, B, nb, ml, on_step=on_step)
    return st, worst[0]


def oracle_search(monkeypatch, T1, T2, B, nb, max_length, length_penalty=1.0, len_offset=0, eos_id=1):
    """oracle.m3ae_oracle.t5_beam_search on the scripted logits (its logits function replaced in the test process)."""
    import torch
    from oracle import m3ae_oracle as O

    def scripted(sd, enc, prefix, heads):
        return torch.from_numpy(scripted_logits(T1, T2, prefix.shape[1] - 1, prefix[:, -1].numpy()))
    monkeypatch.setattr(O, "t5_next_token_logits", scripted)
    return O.t5_beam_search(None, torch.zeros(B, 1, 1), None, num_beams=nb, max_length=max_length, eos_id=eos_id,
                            length_penalty=length_penalty, len_offset=len_offset).numpy()
