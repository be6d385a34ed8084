"""CPU: the numpy model of the constrained beam search (tests/trie_beam_model.py) against a brute-force definition on small lists,
against the greedy model at one beam, the margin condition on every fixed input the GPU tests use (tests/trie_beam_cases.py), the
config keys and the shape handling of VQARADScore.update_labels."""
import numpy as np
import pytest
import torch

import answer_trie_model as AM
import trie_beam_cases as CS
import trie_beam_model as BM
from m3ae_amd import config as config_mod
from m3ae_amd import metrics
from m3ae_amd.answer_trie import AnswerTrie

V, END = 24, 1


def random_list(rng, A, longest=5):
    seqs = set()
    while len(seqs) < A:
        seqs.add(tuple(rng.integers(2, V, size=int(rng.integers(0, longest))).tolist()) + (END,))
    return sorted(seqs)


class Rows:
    """A logits row per prefix, drawn once; the search's rows are followed through `order`."""

    def __init__(self, rng, scale=3.0):
        self.rng, self.scale, self.rows, self.prefixes = rng, scale, {}, None

    def row_of(self, prefix):
        if prefix not in self.rows:
            self.rows[prefix] = (self.rng.standard_normal(V) * self.scale).astype(np.float32)
        return self.rows[prefix]

    def logits_of(self, last_tok, order, pos):
        if order is None:
            self.prefixes = [()] * len(last_tok)
        else:
            self.prefixes = [self.prefixes[o] + (int(t),) for o, t in zip(order, last_tok)]
        return np.stack([self.row_of(p) for p in self.prefixes])

    def greedy_logits_of(self, last_tok, pos):
        self.prefixes = [()] * len(last_tok) if pos == 0 else [p + (int(t),) for p, t in zip(self.prefixes, last_tok)]
        return np.stack([self.row_of(p) for p in self.prefixes])


@pytest.mark.parametrize("lp", [0.0, 1.0])
def test_enough_beams_enumerate_the_list_and_find_the_arg_max(lp):
    rng = np.random.default_rng(int(lp) + 7)
    better = 0
    for trial in range(60):
        A = int(rng.integers(1, 9))
        seqs = random_list(rng, A)
        trie = AnswerTrie(seqs, (END,))
        rows = Rows(rng)
        logprob, score = BM.brute_force(seqs, rows.row_of, lp)
        for nb in (A, 8):
            st, steps = BM.search(rows.logits_of, trie, 1, nb, 8, 0, 0, lp)
            n = int(st.n_hyp[0])
            assert n == A and sorted(st.labels[0, :n].tolist()) == list(range(A)) and (st.labels[0, n:] == -1).all()
            assert st.labels[0, 0] == int(np.argmax(score)) and st.best[0] == st.labels[0, 0]
            np.testing.assert_allclose(st.scores[0, :n], score[st.labels[0, :n]], rtol=0, atol=1e-12)
            np.testing.assert_allclose(st.logprob[0, :n], logprob[st.labels[0, :n]], rtol=0, atol=1e-12)
            assert (np.diff(st.scores[0, :n]) <= 0).all() and st.len[0] == len(seqs[st.best[0]])
            assert steps <= trie.depth and st.open_count[steps - 1] == 0 and st.done.all() and (st.node == -1).all()
            assert np.array_equal(BM.answers_seq(trie, st)[0, :st.len[0]], seqs[st.best[0]])
        g, _ = AM.search(rows.greedy_logits_of, trie, 1, 8, 0, 0)
        better += score.max() > score[g.label[0]] + 1e-9
    assert better > 0        # greedy on a trie is not the arg-max: the reason for this search


def test_one_beam_is_the_greedy_model():
    rng = np.random.default_rng(3)
    for trial in range(40):
        seqs = random_list(rng, int(rng.integers(1, 9)))
        trie = AnswerTrie(seqs, (END,))
        rows = Rows(rng)
        B = 3
        st, steps = BM.search(lambda l, o, p: np.repeat(rows.logits_of(l[:1], None if o is None else o[:1], p), B, 0), trie, B, 1, 8, 0, 0, 1.0)
        g, gsteps = AM.search(lambda l, p: np.repeat(rows.greedy_logits_of(l[:1], p), B, 0), trie, B, 8, 0, 0)
        assert steps == gsteps and np.array_equal(st.labels[:, 0], g.label) and np.array_equal(st.len, g.len)
        assert np.array_equal(BM.answers_seq(trie, st), g.seq) and (st.n_hyp == 1).all()
        np.testing.assert_allclose(st.logprob[:, 0], g.score, rtol=0, atol=1e-12)
        np.testing.assert_allclose(st.scores[:, 0], g.score / g.len, rtol=0, atol=1e-12)


def test_every_sample_ends_with_a_hypothesis_and_short_lists_work():
    """Fewer children than 2 nb at every node, beams in [1, 8], samples that finish at different depths."""
    rng = np.random.default_rng(11)
    for nb in range(1, 9):
        seqs = random_list(rng, int(rng.integers(1, 4)), longest=6)
        trie = AnswerTrie(seqs, (END,))
        B = 4
        rows = [Rows(rng) for _ in range(B)]

        def logits_of(last, order, pos):
            parts = []
            for b in range(B):
                sl = slice(b * nb, (b + 1) * nb)
                parts.append(rows[b].logits_of(last[sl], None if order is None else order[sl] - b * nb, pos))
            return np.concatenate(parts)
        st, steps = BM.search(logits_of, trie, B, nb, 8, 0, 0, 0.0, stop_early=False)
        assert steps == trie.depth and (st.n_hyp >= 1).all() and (st.n_hyp <= min(nb, len(seqs))).all() and st.err[0] == 0
        assert (st.n_cand <= 2 * nb).all() and st.done.all() and st.open_count[trie.depth - 1] == 0
        assert ((st.order >= 0) & (st.order < B * nb)).all() and (st.last_tok == 0).all()
        for b in range(B):
            assert (st.labels[b, :st.n_hyp[b]] >= 0).all() and (st.labels[b, st.n_hyp[b]:] == -1).all()


def test_the_fp32_form_follows_the_devices_order_of_operations():
    """With lse inputs the model computes fl(fl(x - lse) + beam_score) in float32: each kept score is within the derived bound of the
    float64 form, the two forms keep the same candidates, and -0 never appears."""
    rng = np.random.default_rng(5)
    seqs = random_list(rng, 8)
    trie = AnswerTrie(seqs, (END,))
    x = (rng.standard_normal((4, V)) * 3).astype(np.float32)
    a, b = BM.State(1, 4, 8, 0, 0), BM.State(1, 4, 8, 0, 0)
    lse = np.array([AM.TM.lse64(r)[0] for r in x]).astype(np.float32)
    BM.select(a, trie, x)
    BM.select(b, trie, x, lse=lse)
    assert np.array_equal(a.top_edge, b.top_edge) and np.array_equal(a.top_beam, b.top_beam) and a.n_cand[0] == b.n_cand[0]
    n = int(a.n_cand[0])
    assert (np.abs(a.top_s[0, :n] - b.top_s[0, :n]) <= a.top_err[0, :n]).all() and a.top_err[0, :n].max() < 1e-4
    assert not np.signbit(b.top_s[b.top_s == 0]).any()


@pytest.mark.parametrize("case", CS.all_cases(), ids=CS.case_id)
def test_every_gpu_case_has_a_margin_of_eight_bounds(case):
    """A condition on the INPUTS of tests/test_gpu_trie_beam.py::test_select_and_step_match_the_model: with it the float64 model's
    integers are the device's whatever its rounding does within the derived bound."""
    trie, steps, snaps, st = CS.run_model(*case)
    assert len(st.margin) == trie.depth
    for pos, (m, b, h) in enumerate(zip(st.margin, st.bound, st.hyp_ratio)):
        assert np.isfinite(b) and m >= CS.MARGIN_FACTOR * b, (pos, m, b)
        assert h >= CS.MARGIN_FACTOR, (pos, h)
    assert (st.n_hyp >= 1).all() and st.err[0] == 0 and max(st.bound) < 2e-4


def test_the_gpu_cases_cover_what_they_are_meant_to():
    """Over all cases: live beams in nodes of every child count, leaves at ranks below and at or above nb, samples of one case
    finishing at different depths, re-ordered beams."""
    counts, leaf_lo, leaf_hi, staggered, reordered = set(), False, False, False, False
    for case in CS.all_cases():
        B, nb = case[:2]
        trie, steps, snaps, st = CS.run_model(*case)
        for s in snaps:
            counts |= {int(trie.child_off[n + 1] - trie.child_off[n]) for n in s["live_nodes"]}
            for b in range(B):
                for rank in range(2 * nb):
                    e = s["top_edge"][b, rank]
                    if e >= 0 and trie.leaf_label[trie.child_node[e]] >= 0:
                        leaf_lo, leaf_hi = leaf_lo or rank < nb, leaf_hi or rank >= nb
            live = s["node"] >= 0
            reordered = reordered or bool((s["order"][live] != np.arange(B * nb)[live]).any())
        oc = st.open_count[:trie.depth]
        staggered = staggered or (B > 1 and len(set(oc.tolist())) > 2)
    assert set(CS.CHILD_COUNTS) <= counts and leaf_lo and leaf_hi and staggered and reordered


def test_answer_beams_config_is_validated():
    assert config_mod.answer_beams({}) == (1, 0.0)
    assert config_mod.answer_beams({"answer_beams": 8, "answer_length_penalty": 1}) == (8, 1.0)
    for bad in (0, 9, -1, 2.0, "4", True, None):
        with pytest.raises(ValueError, match="answer_beams"):
            config_mod.answer_beams({"answer_beams": bad})
    for bad in ("1", None, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="answer_length_penalty"):
            config_mod.answer_beams({"answer_length_penalty": bad})
    cfg = config_mod.parse_cli([])
    assert cfg["answer_beams"] == 1 and cfg["answer_length_penalty"] == 0.0
    assert config_mod.parse_cli(["answer_beams=4", "answer_length_penalty=1.0"])["answer_beams"] == 4
    with pytest.raises(ValueError, match="answer_beams"):
        config_mod.parse_cli(["answer_beams=9"])
    with pytest.raises(ValueError, match="answer_beams"):
        config_mod.compose(answer_beams=0)
    assert config_mod.compose(answer_beams=2)["answer_beams"] == 2


def test_update_labels_checks_its_shapes_without_a_device():
    met = metrics.VQARADScore.__new__(metrics.VQARADScore)          # no record: the shape rules run before anything touches a device
    tg = torch.zeros((4, 9))
    for labels in (torch.zeros((4, 17), dtype=torch.int64), torch.zeros((4, 0), dtype=torch.int64), torch.zeros((3, 2), dtype=torch.int64),
                   torch.zeros((4, 2), dtype=torch.int32), torch.zeros((4, 2, 1), dtype=torch.int64),
                   torch.zeros((2, 4), dtype=torch.int64).t()):
        with pytest.raises(ValueError):
            met.update_labels(labels, tg)
