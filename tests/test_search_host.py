"""CPU: the one driver of the device-resident searches (m3ae_amd/search.py: run) on a fake head and a fake search that record their
calls -- with lookahead=None it touches no CUDA object -- and the `out` layout of the four search states (ops.*State.views / host,
search.answer_result) on hand-filled CPU buffers, float64 bit-views and -1 labels included."""
from types import SimpleNamespace as NS

import pytest
import torch

from m3ae_amd import _lib, ops, search


class FakeHead:
    def __init__(self, calls):
        self.calls = calls

    def logits(self, last_tok, pos):
        self.calls.append(("logits", last_tok, pos))
        return ("logits of", pos)

    def reorder(self, order):
        self.calls.append(("reorder", order))


class FakeSearch:
    fields = ("seq", "out")

    def __init__(self, calls, reorders):
        self.calls, self.reorders = calls, reorders
        self.state = NS(last_tok="last_tok", open_count="open_count", order="order", seq="seq", out="out")

    def step(self, logits, t):
        self.calls.append(("step", logits, t))

    def finish(self, t_end):
        self.calls.append(("finish", t_end))


def drive(n_steps, reorders, first=0):
    calls = []
    s = FakeSearch(calls, reorders)
    r = search.run(FakeHead(calls), s, n_steps, None, first)
    assert r.state is s.state and r.seq == "seq" and r.out == "out" and sorted(vars(r)) == ["out", "seq", "state", "steps"]
    return r, calls


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("n_steps", [1, 2, 4])
def test_a_beam_search_reorders_after_every_step_but_the_last(n_steps, first):
    r, calls = drive(n_steps, True, first)
    want = []
    for i in range(n_steps):        # the head sees the position i = t - first, the search the step index t
        want += [("logits", "last_tok", i), ("step", ("logits of", i), first + i)]
        if i + 1 < n_steps:
            want.append(("reorder", "order"))
    assert calls == want + [("finish", first + n_steps)]
    assert r.steps == n_steps


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("n_steps", [1, 3])
def test_a_greedy_search_never_reorders(n_steps, first):
    r, calls = drive(n_steps, False, first)
    assert [c[0] for c in calls] == ["logits", "step"] * n_steps + ["finish"]
    assert [c[2] for c in calls if c[0] == "logits"] == list(range(n_steps))
    assert [c[2] for c in calls if c[0] == "step"] == list(range(first, first + n_steps))
    assert calls[-1] == ("finish", first + n_steps) and r.steps == n_steps


def test_one_step_runs_once_finishes_once_and_does_not_reorder():
    r, calls = drive(1, True)
    assert calls == [("logits", "last_tok", 0), ("step", ("logits of", 0), 0), ("finish", 1)] and r.steps == 1


def test_the_real_searches_name_their_result_fields():
    base = ("seq", "len", "err", "out")
    assert search.Greedy.fields == search.Beam.fields == base
    assert search.TrieGreedy.fields == ("label", "score") + base
    assert search.TrieBeam.fields == ("label", "score", "labels", "scores", "logprob", "n_hyp") + base
    assert [c.reorders for c in (search.Greedy, search.Beam, search.TrieGreedy, search.TrieBeam)] == [False, True, False, True]


def test_lookahead_zero_is_refused_by_the_two_free_searches_before_any_device_work():
    from m3ae_amd.modules.t5 import T5ForConditionalGeneration
    m = T5ForConditionalGeneration(dict(d_model=16, d_kv=4, d_ff=32, num_layers=1, num_decoder_layers=1, num_heads=2), 20)
    with pytest.raises(ValueError, match="lookahead"):
        m.generate_async(torch.zeros(2, 3, 16), lookahead=0)
    with pytest.raises(ValueError, match="lookahead"):
        search.run(None, NS(state=None, step=None, reorders=False), 3, 0)


# -----------------------------------------------------------------------------------------------------------------------------------
# the layout of `out`: one description per state, applied to the device buffer and to a host copy
# -----------------------------------------------------------------------------------------------------------------------------------
def bits(values):
    return torch.tensor(values, dtype=torch.float64).view(torch.int64).tolist()


@pytest.mark.parametrize("B", [2, 1])
@pytest.mark.parametrize("cls", [ops.GreedyState, ops.BeamState])
def test_free_search_layout_is_seq_len_err(cls, B):
    L = 3
    st = cls(B, L, "cpu") if cls is ops.GreedyState else cls(B, 2, L, "cpu")
    seq = list(range(10, 10 + B * L))
    lens = [2, 3][:B]
    buf = torch.tensor(seq + lens + [0])
    assert st.out.dtype == torch.int64 and st.out.shape == buf.shape
    st.out.copy_(buf)
    for v in (st, st.host(), st.views(buf)):        # the state's own fields, the host copy, any buffer of the same size
        assert v.seq.tolist() == [seq[b * L:(b + 1) * L] for b in range(B)] and v.len.tolist() == lens and v.err.tolist() == [0]
    assert st.seq.data_ptr() == st.out.data_ptr() and st.err.data_ptr() == st.out[-1:].data_ptr()
    st.out[-1] = 5
    with pytest.raises(_lib.M3AEHipError, match="greedy search" if cls is ops.GreedyState else "beam search"):
        st.host()


@pytest.mark.parametrize("B", [2, 1])
def test_trie_layout_is_seq_len_label_score_err(B):
    L = 3
    st = ops.TrieState(B, L, "cpu")
    assert st.label.tolist() == [-1] * B and st.len.tolist() == [L] * B       # as allocated: no label yet
    seq = list(range(20, 20 + B * L))
    lens, labels, scores = [1, 3][:B], [4, -1][:B], [-0.125, -1e300][:B]
    buf = torch.tensor(seq + lens + labels + bits(scores) + [0])
    assert st.out.shape == buf.shape
    st.out.copy_(buf)
    h = st.host()
    for v in (st, h):
        assert v.seq.tolist() == [seq[b * L:(b + 1) * L] for b in range(B)] and v.len.tolist() == lens
        assert v.labels.tolist() == [[l] for l in labels] and v.scores.dtype == torch.float64
        assert v.scores.tolist() == [[s] for s in scores]
    assert st.label.tolist() == labels and st.score.tolist() == scores and st.score.dtype == torch.float64
    assert st.label.data_ptr() == st.out[B * L + B:].data_ptr() and st.score.is_contiguous()
    l1, s1 = search.answer_result(NS(state=st))
    assert l1.tolist() == labels and s1.tolist() == scores
    for k in (0, 2):
        with pytest.raises(ValueError, match="needs a beam search"):
            search.answer_result(NS(state=st), k=k)
    st.out[-1] = 1
    with pytest.raises(_lib.M3AEHipError, match="answer table"):
        search.answer_result(NS(state=st), k=2)       # the error word is looked at first


@pytest.mark.parametrize("B", [2, 1])
def test_trie_beam_layout_is_seq_len_labels_scores_logprob_n_hyp_err(B):
    L, nb = 3, 2
    st = ops.TrieBeamState(B, nb, L, "cpu")
    assert st.labels.tolist() == [[-1] * nb] * B
    seq = list(range(30, 30 + B * L))
    lens, labels = [2, 3][:B], [7, -1, 0, 3][:B * nb]
    scores, logprob, n_hyp = [-0.5, -2.0 ** -60, -3.25, -1e10][:B * nb], [-1.0, -0.75, -6.5, -2.5][:B * nb], [1, 2][:B]
    buf = torch.tensor(seq + lens + labels + bits(scores) + bits(logprob) + n_hyp + [0])
    assert st.out.shape == buf.shape
    st.out.copy_(buf)
    rows = lambda x: [x[b * nb:(b + 1) * nb] for b in range(B)]    # noqa: E731
    for v in (st, st.host()):
        assert v.seq.tolist() == [seq[b * L:(b + 1) * L] for b in range(B)] and v.len.tolist() == lens
        assert v.labels.tolist() == rows(labels) and v.scores.tolist() == rows(scores) and v.logprob.tolist() == rows(logprob)
        assert v.n_hyp.tolist() == n_hyp and v.err.tolist() == [0]
    assert st.label.tolist() == labels[::nb] and st.score.tolist() == scores[::nb]
    l2, s2 = search.answer_result(NS(state=st), k=2)
    assert l2.tolist() == rows(labels) and s2.tolist() == rows(scores)
    l1, s1 = search.answer_result(NS(state=st))
    assert l1.tolist() == labels[::nb] and s1.tolist() == scores[::nb]
    with pytest.raises(ValueError, match="num_beams=2"):
        search.answer_result(NS(state=st), k=3)
    st.out[-1] = 2
    with pytest.raises(_lib.M3AEHipError, match="answer table"):
        search.answer_result(NS(state=st))
