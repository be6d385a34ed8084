"""CPU: the host tables of exhaustive answer-list scoring (AnswerTrie.score_tables) against a brute-force walk of the list, the numpy
model of the fold (tests/trie_score_model.py) against a brute-force definition with the non-finite rules, the margin condition on
every fixed input the GPU tests use (tests/trie_score_cases.py), the header / binding / stub sets of the new entry points, the
workspace arithmetic and the `answer_scoring` config key."""
import os
import sys

import numpy as np
import pytest

import abi_header
import trie_score_cases as CS
import trie_score_model as SM
from m3ae_amd import _lib, config as config_mod
from m3ae_amd.answer_trie import SCORE_MAX_DEPTH, AnswerTrie

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NEW = {"m3ae_tree_attn", "m3ae_listscore_workspace_bytes", "m3ae_listscore_lse", "m3ae_listscore_edges",
       "m3ae_listscore_fold_workspace_bytes", "m3ae_listscore_fold"}


def brute_tables(seqs):
    """The tables by definition: a node is a distinct non-empty prefix (plus the root), numbered by (length, then the breadth-first
    order the sorted-children walk gives); nothing of AnswerTrie's arrays is used."""
    order = [()]
    head = 0
    while head < len(order):
        p = order[head]
        head += 1
        nxt = sorted({s[len(p)] for s in seqs if len(s) > len(p) and tuple(s[:len(p)]) == p})
        order += [p + (t,) for t in nxt]
    idx = {p: n for n, p in enumerate(order)}
    has_child = [any(len(s) > len(p) and tuple(s[:len(p)]) == p for s in seqs) for p in order]
    internal = [n for n, h in enumerate(has_child) if h]
    row_of = {n: i for i, n in enumerate(internal)}
    D = max(len(s) for s in seqs)
    anc = np.full((len(internal), D), -1, dtype=np.int64)
    for i, n in enumerate(internal):
        p = order[n]
        for d in range(len(p) + 1):
            anc[i, d] = row_of[idx[p[:d]]]
    return dict(parent=[-1] + [idx[p[:-1]] for p in order[1:]], depth=[len(p) for p in order], in_tok=[-1] + [p[-1] for p in order[1:]],
                internal=internal, row_of=[row_of.get(n, -1) for n in range(len(order))], anc=anc,
                leaf_node=[idx[tuple(s)] for s in seqs])


@pytest.mark.parametrize("name", sorted(CS.LISTS))
def test_tables_match_a_brute_force_walk(name):
    seqs = CS.LISTS[name]()
    trie = AnswerTrie(seqs, (CS.END,))
    t, want = trie.score_tables(), brute_tables(seqs)
    for key, w in want.items():
        assert t[key].dtype == np.int32 and np.array_equal(t[key], np.asarray(w)), key
    Ni, N, D = len(t["internal"]), trie.num_nodes, trie.depth
    assert t["anc"].shape == (Ni, D) and (t["anc"][:, 0] == 0).all()                  # every path starts at the root
    for i in range(Ni):
        n = int((t["anc"][i] >= 0).sum())
        assert t["anc"][i, n - 1] == i and (t["anc"][i, n:] == -1).all() and n == t["depth"][t["internal"][i]] + 1
    lo = t["level_off"]
    assert lo.shape == (D + 2,) and lo[0] == 0 and lo[1] == 1 and lo[-1] == N and (np.diff(lo) >= 1).all()
    for d in range(D + 1):
        assert (t["depth"][lo[d]:lo[d + 1]] == d).all()
    assert np.array_equal(trie.child_node, np.arange(1, N))                          # the edge into node n is entry n - 1
    if name == "wide300":
        assert trie.child_off[1] > 256
    if name == "deep32":
        assert D == SCORE_MAX_DEPTH


def test_a_list_deeper_than_the_cap_is_refused():
    trie = AnswerTrie(CS.deep_list(CS.END, 33), (CS.END,))
    assert trie.depth == 33
    with pytest.raises(ValueError, match="room for 32"):
        trie.score_tables()


@pytest.mark.parametrize("lp", [0.0, 1.0])
def test_the_fold_model_is_the_brute_force_definition(lp):
    rng = np.random.default_rng(int(lp) + 3)
    for name in ("gen60", "prefix", "one", "wide300"):
        seqs = CS.LISTS[name]()
        trie = AnswerTrie(seqs, (CS.END,))
        terms = {}
        edge = np.zeros((2, trie.num_edges))
        t = trie.score_tables()
        prefix_of = [()]
        for n in range(1, trie.num_nodes):
            prefix_of.append(prefix_of[t["parent"][n]] + (int(t["in_tok"][n]),))
        for b in range(2):
            for n in range(1, trie.num_nodes):
                v = -abs(rng.standard_normal()) * 3
                if b == 1 and name == "gen60" and n in (1, 7):
                    v = -np.inf if n == 1 else np.nan
                terms[(b, prefix_of[n])] = v
                edge[b, n - 1] = v
        for k in (1, 5, 16):
            r = SM.fold(edge, trie, k, lp)
            for b in range(2):
                lpw, score, mass, order = SM.brute_force(seqs, lambda p, tok: terms[(b, p + (tok,))], k, lp)
                np.testing.assert_allclose(r["all_logprob"][b], lpw, rtol=0, atol=1e-12, equal_nan=True)
                kk = min(k, len(seqs))
                assert r["labels"][b, :kk].tolist() == order[:kk].tolist() and (r["labels"][b, kk:] == -1).all() and r["n_hyp"][b] == kk
                assert r["log_mass"][b] == pytest.approx(mass, abs=1e-12)
                np.testing.assert_allclose(r["scores"][b, :kk], score[order[:kk]], rtol=0, atol=1e-12, equal_nan=True)
                fin = np.isfinite(lpw)
                assert (r["all_probs"][b][~fin] == 0).all() and r["all_probs"][b].sum() == pytest.approx(1.0, abs=1e-12)
                assert r["len"][b] == len(seqs[order[0]])
                if b == 1 and name == "gen60":      # -inf and NaN entries exist; NaN ranks last, -inf before it
                    full = SM.rank_order(score)
                    n_nan = int(np.isnan(score).sum())
                    assert n_nan > 0 and np.isnan(score[full[-n_nan:]]).all() and np.isneginf(lpw).any()
                    assert (np.diff(full[-n_nan:]) > 0).all()


def test_no_finite_entry_gives_no_mass():
    trie = AnswerTrie(CS.LISTS["prefix"](), (CS.END,))
    edge = np.full((1, trie.num_edges), -np.inf)
    r = SM.fold(edge, trie, 3, 0.0)
    assert r["log_mass"][0] == -np.inf and (r["probs"] == 0).all() and r["labels"][0].tolist() == [0, 1, 2]
    assert SM.rank_order([np.nan, -np.inf, 0.0, -0.0, np.nan, 1.0]).tolist() == [5, 2, 3, 1, 0, 4]


@pytest.mark.parametrize("case", CS.CASES, ids=CS.case_id)
def test_every_gpu_case_has_a_margin_of_eight_bounds(case):
    """A condition on the INPUTS of tests/test_gpu_trie_score.py::test_list_scores_match_the_model: the adjacent gaps of the first k
    ranking scores and the gap to entry k + 1 are at least MARGIN_FACTOR times the two entries' derived bounds."""
    trie, x, edge, eb, r = CS.run_model(case)
    m = SM.margins(r, case[5])
    print(CS.case_id(case), "least margin / bound", m.min(), "largest entry bound", r["all_bound"].max())
    assert (m >= CS.MARGIN_FACTOR).all(), m
    assert np.isfinite(r["all_bound"]).all() and r["all_bound"].max() < 1e-3
    if case[7] == "nonfinite":
        assert np.isneginf(r["all_logprob"][0]).any() and np.isnan(r["all_logprob"][1]).any() and np.isfinite(r["all_logprob"][2]).all()


def test_the_new_entry_points_are_declared_bound_and_in_the_stub():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_integration_stub as gen
    protos = set(abi_header.prototypes())
    assert NEW <= protos and NEW <= set(_lib.EXPORTS) and set(gen.LIST_SCORE_ENTRIES) == NEW
    assert {n for n in protos if n.startswith(("m3ae_tree_attn", "m3ae_listscore_"))} == NEW
    assert not any(n.startswith(("m3ae_trie", "m3ae_greedy_")) for n in NEW)        # the prefixes other tests count launches by
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in NEW:
        assert f"lib.{n}.restype" in stub, n


def test_workspace_sizes():
    L = _lib.lib()
    assert L.m3ae_listscore_workspace_bytes(7, 1001, 256) == 7 * 4 * 8 and L.m3ae_listscore_workspace_bytes(7, 1001, 0) == 7 * 8
    assert L.m3ae_listscore_workspace_bytes(3, 30522, 0) == 3 * 4 * 8 == L.m3ae_trie_workspace_bytes(3, 30522, 0) - 3 * 8
    for bad in ((0, 10, 64), (1, 0, 64), (1, 10, 32), (1, 10, 65537), (1, 2 ** 31, 64)):
        assert L.m3ae_listscore_workspace_bytes(*bad) == 0, bad
    assert L.m3ae_listscore_fold_workspace_bytes(5, 4096) == 0 and L.m3ae_listscore_fold_workspace_bytes(5, 4097) == 5 * 4097 * 8
    assert L.m3ae_listscore_fold_workspace_bytes(0, 10) == -1 and L.m3ae_listscore_fold_workspace_bytes(1, 1) == -1


def test_answer_scoring_config_is_validated():
    assert config_mod.answer_scoring({}) == "search" and config_mod.answer_scoring({"answer_scoring": "exhaustive"}) == "exhaustive"
    for bad in ("", "beam", "Exhaustive", None, 1, True):
        with pytest.raises(ValueError, match="answer_scoring"):
            config_mod.answer_scoring({"answer_scoring": bad})
    assert config_mod.parse_cli([])["answer_scoring"] == "search"
    assert config_mod.parse_cli(["answer_scoring=exhaustive"])["answer_scoring"] == "exhaustive"
    with pytest.raises(ValueError, match="answer_scoring"):
        config_mod.parse_cli(["answer_scoring=all"])
    with pytest.raises(ValueError, match="answer_scoring"):
        config_mod.compose(answer_scoring="list")
    assert config_mod.compose(answer_scoring="exhaustive", answer_decoding="free")["answer_scoring"] == "exhaustive"
