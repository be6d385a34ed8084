"""The answer trie (m3ae_amd/answer_trie.py) against a dict-of-dicts trie, and the numpy model of the answer-list kernels
(tests/answer_trie_model.py) against a brute-force definition on the list itself.  The GPU tests (tests/test_gpu_answer_trie.py)
then hold the kernels to this model.  Also the host-side surface of the feature: the declared symbols, the config key, the sizing
and the argument checks that need no GPU."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import abi_header
import answer_trie_model as M
import token_eval_model as TM
from m3ae_amd.answer_trie import AnswerTrie

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 2


def random_list(n, rng, vocab=50, max_tokens=6, end=END):
    """n distinct sequences over [3, vocab) ending in `end`, with shared prefixes (a small alphabet makes them)."""
    seen, out = set(), []
    while len(out) < n:
        s = tuple(int(t) for t in rng.integers(3, vocab, size=int(rng.integers(1, max_tokens + 1)))) + (end,)
        if s not in seen:
            seen.add(s)
            out.append(list(s))
    return out


def lists():
    rng = np.random.default_rng(7)
    return {
        "shared_prefixes": random_list(40, rng, vocab=8),
        "prefix_of_another": [[5, 6, END], [5, 6, 7, END], [5, END], [9, 6, 7, END]],
        "one_token": [[END], [4, END], [4, 4, END]],
        "single_answer": [[11, 12, 13, END]],
        "vqa_rad_size": random_list(498, rng, vocab=60, max_tokens=8),
    }


LISTS = lists()


def dict_trie(seqs):
    root = {}
    for i, s in enumerate(seqs):
        n = root
        for t in s:
            n = n.setdefault(t, {})
        n["label"] = i
    return root


@pytest.mark.parametrize("name", list(LISTS))
def test_csr_arrays_equal_a_dict_trie(name):
    seqs = LISTS[name]
    t = AnswerTrie(seqs, (END,))
    assert t.depth == max(len(s) for s in seqs) and t.num_answers == len(seqs)
    for a in (t.child_off, t.child_tok, t.child_node, t.leaf_label):
        assert a.dtype == np.int32
    assert t.child_off.shape == (t.num_nodes + 1,) and t.child_tok.shape == t.child_node.shape == (t.num_edges,)
    assert t.child_off[0] == 0 and t.child_off[-1] == t.num_edges
    # breadth-first walk of both tries in step: same tokens in the same (ascending) order, node numbers in visiting order
    queue, head, seen_nodes = [(0, dict_trie(seqs))], 0, 1
    while head < len(queue):
        node, d = queue[head]
        head += 1
        toks, nodes = t.children(node)
        want = sorted(k for k in d if k != "label")
        assert toks.tolist() == want and np.all(np.diff(toks) > 0)
        assert nodes.tolist() == list(range(seen_nodes, seen_nodes + len(want)))     # numbered as they are met
        seen_nodes += len(want)
        assert t.leaf_label[node] == d.get("label", -1)
        assert (len(want) == 0) == ("label" in d)                                    # a leaf has no child, every other node has one
        queue += [(int(n), d[k]) for k, n in zip(want, nodes)]
    assert seen_nodes == t.num_nodes
    for i, s in enumerate(seqs):                                                      # every sequence reaches its own label
        assert t.leaf_label[t.walk(s)] == i
    assert t.walk([1]) == -1
    again = AnswerTrie(seqs, (END,))                                                  # a function of the list alone
    for a, b in zip((t.child_off, t.child_tok, t.child_node, t.leaf_label), (again.child_off, again.child_tok, again.child_node, again.leaf_label)):
        assert np.array_equal(a, b)


def test_from_answers_appends_the_end_token_and_takes_several_end_ids():
    t = AnswerTrie.from_answers([[5, 6], [5], []], END)
    assert t.sequences == [(5, 6, END), (5, END), (END,)]
    t2 = AnswerTrie([[5, 1], [5, END]], (1, END))
    assert sorted(t2.leaf_label[t2.leaf_label >= 0].tolist()) == [0, 1]


def test_value_errors():
    with pytest.raises(ValueError, match="empty"):
        AnswerTrie([], (END,))
    with pytest.raises(ValueError, match="does not end"):
        AnswerTrie([[4, 5]], (END,))
    with pytest.raises(ValueError, match="does not end"):
        AnswerTrie([[]], (END,))
    with pytest.raises(ValueError, match="before its last"):
        AnswerTrie([[4, END, 5, END]], (END,))
    with pytest.raises(ValueError, match="answers 1 and 3"):
        AnswerTrie([[4, END], [5, END], [6, END], [5, END]], (END,))
    with pytest.raises(ValueError, match="negative"):
        AnswerTrie([[4, -1, END]], (END,))


def test_to_device_checks_its_bounds_on_cpu():
    t = AnswerTrie([[4, 9, END], [4, END]], (END,))
    with pytest.raises(ValueError, match="vocabulary"):
        t.to_device("cpu", 9, 8)
    with pytest.raises(ValueError, match="room for 2"):
        t.to_device("cpu", 10, 2)
    d = t.to_device("cpu", 10, 3)
    assert d.buf.dtype == torch.int32 and d.N == t.num_nodes and d.E == t.num_edges and d.depth == 3
    assert d.child_off.tolist() == t.child_off.tolist() and d.child_tok.tolist() == t.child_tok.tolist()
    assert d.child_node.tolist() == t.child_node.tolist() and d.leaf_label.tolist() == t.leaf_label.tolist()
    assert d.buf.numel() == 2 * t.num_nodes + 1 + 2 * t.num_edges
    assert t.to_device("cpu", 10, 3).buf is d.buf                                    # one upload per device


@pytest.mark.parametrize("name", list(LISTS))
def test_model_equals_the_brute_force_definition(name):
    seqs = LISTS[name]
    t = AnswerTrie(seqs, (END,))
    V, B = 64, 6
    rng = np.random.default_rng(len(seqs))
    script = rng.standard_normal((t.depth, B, V)).astype(np.float32)
    script[:, 1] = np.round(script[:, 1])                       # a row with many equal values: the lowest id wins
    script[:, 2, :] = 0.5                                       # all equal
    prefixes = [[] for _ in range(B)]

    def logits_of(last_tok, pos):
        return script[pos]

    st = M.State(B, t.depth + 1, 101, 0)
    for pos in range(t.depth):
        open_before = st.finished == 0
        want = [M.brute_force_token(seqs, prefixes[r], script[pos, r]) if open_before[r] else None for r in range(B)]
        M.step(st, t, logits_of(None, pos), pos, 0)
        for r in range(B):
            if open_before[r]:
                assert st.seq[r, pos] == want[r] == st.last_tok[r]
                prefixes[r].append(want[r])
            else:
                assert st.seq[r, pos] == 0
        assert st.open_count[pos] == int((st.finished == 0).sum())
    assert st.err[0] == 0 and st.finished.all()
    for r in range(B):
        assert seqs[int(st.label[r])] == prefixes[r] and st.len[r] == len(prefixes[r])
        x = np.stack([script[p, r] for p in range(len(prefixes[r]))]).astype(np.float64)
        want_score = sum(x[p, tok] - np.log(np.exp(x[p]).sum()) for p, tok in enumerate(prefixes[r]))
        assert abs(st.score[r] - want_score) < 1e-9


def test_model_choice_rule_edges():
    t = AnswerTrie([[4, END], [7, END], [9, END]], (END,))
    x = np.zeros(12, dtype=np.float32)
    x[3] = 50.0                                                  # the row maximum is no child
    x[[7, 9]] = 1.0
    assert M.choose(t, 0, x)[1] == 7
    x = np.full(12, -1.0, dtype=np.float32); x[4] = -0.0; x[9] = 0.0
    assert M.choose(t, 0, x)[1] == 4                             # -0 == +0: the lower token
    x = np.zeros(12, dtype=np.float32); x[9] = np.nan; x[4] = np.inf
    assert M.choose(t, 0, x)[1] == 9 and np.isnan(M.term64(x, 9))
    x = np.zeros(12, dtype=np.float32); x[5] = np.nan; x[7] = 1.0
    assert M.choose(t, 0, x)[1] == 7 and np.isnan(M.term64(x, 7))
    x = np.zeros(12, dtype=np.float32); x[[4, 7, 9]] = -np.inf
    assert M.choose(t, 0, x)[1] == 4 and M.term64(x, 4) == -np.inf
    x = np.zeros(12, dtype=np.float32); x[3] = np.inf
    assert M.term64(x, 4) == -np.inf


def test_the_bound_of_this_fold_is_within_token_evals_up_to_ten_chunks():
    for itemsize in (4, 2):
        for V, chunk in ((9, 0), (257, 256), (1100, 256), (4099, 1000), (30522, 0), (30522, 4096)):
            nch = -(-V // (chunk or M.DEF_CHUNK))
            assert nch <= 10 and M.path_units(V, chunk, itemsize) <= TM.path_units(V, chunk, itemsize)
        assert M.path_units(30522, 256, itemsize) > TM.path_units(30522, 256, itemsize)      # 120 sequential merges
    x = np.random.default_rng(0).standard_normal(4099).astype(np.float32)
    assert M.term_bound(x, 5, 1000, 4)[1] <= TM.nll_bound(x, 5, 1000, 4)[1]
    assert abs(M.term_bound(x, 5, 1000, 4)[0] + TM.nll_bound(x, 5, 1000, 4)[0]) < 1e-12      # term = -nll


def test_config_key_and_signatures():
    from m3ae_amd import config
    from m3ae_amd.metrics import VQARADScore
    from m3ae_amd.modules.m3ae_decoder import Decoder, DecoderModel
    from m3ae_amd.modules.m3ae_t5_mm_encoder_input import T5VQA_MMEncoderInput
    from m3ae_amd.modules.t5 import T5ForConditionalGeneration
    from m3ae_amd.trainer import Trainer
    assert config.DEFAULTS["answer_decoding"] == "free"
    assert config.parse_cli(["with", "answer_decoding=list"])["answer_decoding"] == "list"
    assert config.tiny_config(answer_decoding="list")["answer_decoding"] == "list"
    assert config.answer_decoding({}) == "free"
    for bad in ("trie", "", None, 1):
        with pytest.raises(ValueError, match="answer_decoding"):
            config.tiny_config(answer_decoding=bad)
    with pytest.raises(ValueError, match="answer_decoding"):
        config.parse_cli(["with", "answer_decoding=List"])
    sig = inspect.signature(Decoder.answer_path_async)
    assert list(sig.parameters)[1:4] == ["cross_attn_feats", "trie", "cls_id"]
    assert sig.parameters["lookahead"].default == 2 and sig.parameters["chunk"].default == 0
    sig = inspect.signature(T5ForConditionalGeneration.constrained_greedy_async)
    assert list(sig.parameters)[1:5] == ["enc", "trie", "max_length", "pad_token_id"] and sig.parameters["lookahead"].default == 2
    for cls in (DecoderModel, T5VQA_MMEncoderInput):
        assert callable(cls.answer) and callable(cls.answer_async)
    assert callable(VQARADScore.update_labels) and callable(Trainer.set_answer_list)


def test_declared_symbols_and_sizing():
    from m3ae_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_integration_stub as gen
    names = {"m3ae_trie_workspace_bytes", "m3ae_trie_scan", "m3ae_trie_step"}
    assert {n for n in abi_header.prototypes() if n.startswith("m3ae_trie_")} == names
    assert {n for n in _lib.EXPORTS if n.startswith("m3ae_trie_")} == names
    assert set(gen.ANSWER_TRIE_ENTRIES) == names | {"m3ae_vqa_label_eval"}
    assert "m3ae_vqa_label_eval" in abi_header.prototypes() and "m3ae_vqa_label_eval" in _lib.EXPORTS
    L = _lib.lib()
    # 8 bytes per row for the child key + 8 per (row, chunk) for the (m, s) pair; 0 for a shape the launch would reject
    assert L.m3ae_trie_workspace_bytes(5, 30522, 0) == 5 * (1 + 4) * 8
    assert L.m3ae_trie_workspace_bytes(2, 1001, 256) == 2 * (1 + 4) * 8
    assert L.m3ae_trie_workspace_bytes(0, 9, 0) == L.m3ae_trie_workspace_bytes(1, 9, 32) == L.m3ae_trie_workspace_bytes(1, 2 ** 31, 0) == 0


def test_set_answer_list_goes_through_the_tokenizer():
    from types import SimpleNamespace as NS
    from m3ae_amd import trainer

    class Tok:
        def __call__(self, text, add_special_tokens=False):
            return NS(input_ids=[200 + ord(c) for c in text])
    tr = trainer.Trainer.__new__(trainer.Trainer)
    tr.model = NS(tokenizer=Tok(), tokens_of=None, sep_id=102)
    t = tr.set_answer_list({"0": "yes", "1": "no", "2": "y"})
    assert t is tr.answer_trie and t.sequences == [(321, 301, 315, 102), (310, 311, 102), (321, 102)]
    assert tr.set_answer_list(["no"]).sequences == [(310, 311, 102)]
    tr.model = NS(tokenizer=None, tokens_of=None, sep_id=102)
    with pytest.raises(ValueError, match="tokenizer"):
        tr.set_answer_list(["no"])


def test_ops_reject_cpu_tensors():
    from m3ae_amd import _lib, ops
    st = type("S", (), {"B": 2, "out": torch.zeros(1)})()
    with pytest.raises(_lib.M3AEHipError):
        ops.trie_scan(torch.zeros(2, 9), None, st)
    with pytest.raises(_lib.M3AEHipError):
        ops.trie_step(torch.zeros(2, 9), None, st, None, 0, 0)
    with pytest.raises(_lib.M3AEHipError):
        ops.vqa_label_eval(torch.zeros(2, dtype=torch.int64), torch.zeros(2, 4), None, None)
