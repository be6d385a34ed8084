"""The device-resident decoding searches: ONE host loop (`run`) over a head, which turns the last tokens into the logits of the next
position (DecoderHead, T5Head: encoder-side keys / values once per call, the self-attention cache), and a search, which consumes
them on the device (Greedy, Beam, TrieGreedy, TrieBeam: its ops.*State, workspace and constants).  Decoder.search_path_async /
answer_path_async / answer_beam_async and T5's generate_async / constrained_greedy_async / constrained_beam_async build one of each."""
from types import SimpleNamespace as NS

import torch

from . import ops


def run(head, search, n_steps, lookahead, first=0):
    """Steps t = first .. first + n_steps - 1 of `search` (step t writes slot t of state.open_count) on the logits of `head` at
    positions t - first, enqueued with no blocking host call, then search.finish(the next t).  ops.OpenCountWatch ends the loop
    early unless lookahead is None; a search that `reorders` has the head's cache follow state.order between steps.  Returns the
    namespace of search.fields (views of the state, on the device), `steps` (steps enqueued) and `state`."""
    st, watch = search.state, ops.OpenCountWatch(first + n_steps, lookahead, first)
    logits, step, reorder = head.logits, search.step, head.reorder if search.reorders else None
    last, steps = first + n_steps - 1, 0
    for t in range(first, last + 1):
        step(logits(st.last_tok, t - first), t)
        steps += 1
        if watch.enqueued(st.open_count, t):
            break
        if reorder is not None and t < last:       # only when another step will read the cache
            reorder(st.order)
    search.finish(first + steps)
    return NS(**{f: getattr(st, f) for f in search.fields}, steps=steps, state=st)


class DecoderHead:
    """Decoder.step_logits at rows = B * nb: the live layer's encoder-side keys | values (each sample's nb times), one
    [rows, n_pos, 2 D] self-attention cache and every position's sinusoid row repeated `rows` times ([n_pos, rows, D])."""

    def __init__(self, dec, feats, n_pos, nb=1):
        self.dec, self.rows, D = dec, feats.shape[0] * nb, dec.target_embedding.weight.shape[1]
        enc_kv = dec.dec_layers[dec.num_layers - 1].cross_kv(feats.to(dec.head_dtype))
        self.enc_kv = enc_kv if nb == 1 else enc_kv.repeat_interleave(nb, dim=0)
        self.cache = torch.empty((self.rows, n_pos, 2 * D), dtype=dec.head_dtype, device=feats.device)
        self.pe_rows = dec.positional_encoding.pe[0, :n_pos].to(torch.float32)[:, None, :].expand(n_pos, self.rows, D).contiguous()

    def logits(self, last_tok, pos):
        return self.dec.step_logits(last_tok.view(self.rows, 1), pos, self.enc_kv, self.cache, self.pe_rows[pos])

    def reorder(self, order):
        self.cache = ops.gather_rows(self.cache.view(self.rows, -1), order).view_as(self.cache)


class T5Head:
    """T5ForConditionalGeneration.next_token_logits_cached at rows = B * nb: the encoder output and every block's cross keys / values,
    each sample's repeated nb times (its beams share them: re-ordering never touches either), and per block a self-attention cache."""

    def __init__(self, t5, enc, n_pos, nb=1):
        (B, Ls), self.step, self.rows = enc.shape[:2], t5.next_token_logits_cached, enc.shape[0] * nb
        self.enc, self.cross_kv = enc, t5.decoder.cross_kv(enc)
        if nb > 1:
            self.enc = enc.repeat_interleave(nb, dim=0).contiguous()
            self.cross_kv = [kv.view(B, Ls, -1).repeat_interleave(nb, dim=0).reshape(self.rows * Ls, -1) for kv in self.cross_kv]
        self.cache = t5.decoder.new_self_cache(self.rows, n_pos, enc.dtype, enc.device)

    def logits(self, last_tok, pos):
        return self.step(self.enc, last_tok.view(self.rows, 1), self.cross_kv, self.cache, pos)

    def reorder(self, order):
        self.cache = [ops.gather_rows(c.view(self.rows, -1), order).view_as(c) for c in self.cache]


class Greedy:
    """Free greedy search (csrc/greedy.hip); a row ends at sep_id or eos_id (None: no second end token).  Also the base of the other
    searches: `fields` = what of the state the result namespace names, `ws` = the workspace, sized at the first step (V is known)."""
    fields, reorders, ws = ("seq", "len", "err", "out"), False, None

    def __init__(self, B, max_len, device, start_id, sep_id, eos_id, pad_id, chunk=0):
        self.state, self.args, self.chunk = ops.GreedyState(B, max_len, device, start_id, pad_id), (sep_id, eos_id, pad_id), chunk

    def step(self, logits, t):
        V = logits.shape[-1]
        if self.ws is None:
            self.ws = ops.greedy_workspace(self.state.B, V, logits.device, self.chunk)
        ops.greedy_argmax(logits, self.chunk, self.ws)
        ops.greedy_step(self.state, self.ws, V, t, *self.args)

    def finish(self, t_end):
        pass


class Beam(Greedy):
    """Free beam search, HF's BeamSearchScorer (csrc/beam.hip).  Step t extends the prefixes of length t, so the driver runs it with
    first=1: cur_len = t, position t - 1, slot t of open_count; finish = ops.beam_finalize at the length reached."""
    reorders = True

    def __init__(self, B, nb, max_length, device, start_id, eos_id, pad_id, length_penalty=1.0, len_offset=0, chunk=0):
        self.state, self.chunk = ops.BeamState(B, nb, max_length, device, start_id, pad_id), chunk
        self.args, self.len_offset = (eos_id, pad_id, length_penalty), len_offset
        self.top = (torch.empty((B, 2 * nb), dtype=torch.float32, device=device), torch.empty((B, 2 * nb), dtype=torch.int32, device=device))

    def step(self, logits, t):
        st, V = self.state, logits.shape[-1]
        if self.ws is None:
            self.ws = ops.beam_topk_workspace(st.B, st.nb, V, logits.device, self.chunk)
        ops.beam_topk(logits, st.beam_scores, st.B, st.nb, self.chunk, self.ws, self.top)
        ops.beam_step(st, *self.top, V, t, *self.args)

    def finish(self, t_end):
        ops.beam_finalize(self.state, t_end, *self.args, self.len_offset)


class TrieGreedy(Greedy):
    """Greedy search on the answer list (csrc/answer_trie.hip) over `trie`, what AnswerTrie.to_device returned."""
    fields = ("label", "score") + Greedy.fields

    def __init__(self, B, max_len, trie, device, start_id, pad_id, chunk=0):
        self.state, self.trie, self.pad_id, self.chunk = ops.TrieState(B, max_len, device, start_id, pad_id), trie, pad_id, chunk

    def step(self, logits, t):
        if self.ws is None:
            self.ws = ops.trie_workspace(self.state.B, logits.shape[-1], logits.device, self.chunk)
        ops.trie_scan(logits, self.trie, self.state, self.chunk, self.ws)
        self.advance(logits, t)

    def advance(self, logits, t):
        ops.trie_step(logits, self.trie, self.state, self.ws, t, self.pad_id, self.chunk)


class TrieBeam(TrieGreedy):
    """Constrained beam search on the answer list (csrc/trie_beam.hip): the scan runs over the B * nb beam rows; finish =
    ops.trie_beam_result (`trie` was uploaded with pad_id, so it holds the answers table)."""
    fields, reorders = ("label", "score", "labels", "scores", "logprob", "n_hyp") + Greedy.fields, True

    def __init__(self, B, nb, max_len, trie, device, start_id, pad_id, length_penalty=0.0, chunk=0):
        self.state, self.trie = ops.TrieBeamState(B, nb, max_len, device, start_id, pad_id), trie
        self.length_penalty, self.chunk = length_penalty, chunk

    def advance(self, logits, t):
        ops.trie_beam_select(logits, self.trie, self.state, self.ws, self.chunk)
        ops.trie_beam_step(self.trie, self.state, logits.shape[-1], t, self.length_penalty)

    def finish(self, t_end):
        ops.trie_beam_result(self.trie, self.state)


def answer_result(r, label2ans=None, k=1):
    """One copy of an answer-list search's `out` buffer (`r`: the namespace of a TrieGreedy or TrieBeam run) -> (labels int64 [B],
    scores float64 [B]) on the host; raises if the error word is set.  With label2ans: a list of (answer, score) through
    label2ans[str(label)] (m3ae_module.answers_of's rule).  k > 1 (a beam search with num_beams >= k): the k best entries per row
    instead -- (labels [B, k] with -1 for a missing entry, scores [B, k]), or with label2ans B lists of up to k (answer, score)."""
    k, st, h = int(k), r.state, r.state.host()
    if not 1 <= k <= st.nb:
        raise ValueError(st.k_text.format(k=k, nb=st.nb))
    labels2, scores2 = h.labels[:, :k], h.scores[:, :k]
    if label2ans is None:
        return (labels2[:, 0], scores2[:, 0]) if k == 1 else (labels2, scores2)
    from .modules.m3ae_module import answers_of
    if k == 1:      # column 0 as it is: a row that ended without a label (-1) is a KeyError of answers_of, as it always was
        return [row[0] for row in answers_of(labels2.tolist(), scores2.tolist(), label2ans)]
    rows = [[(l, s) for l, s in zip(lr, sr) if l >= 0] for lr, sr in zip(labels2.tolist(), scores2.tolist())]   # -1 = no entry
    return answers_of([[l for l, _ in row] for row in rows], [[s for _, s in row] for row in rows], label2ans)
