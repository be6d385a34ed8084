"""GPU: constrained beam search on the answer list (csrc/trie_beam.hip, m3ae_vqa_labels_eval of csrc/vqa_eval.hip) --
m3ae_trie_scan + m3ae_triebeam_select + m3ae_triebeam_step against the numpy model of tests/trie_beam_model.py over several steps
(integers and state exactly, scores within the model's derived bound of float64; tests/test_trie_beam_host.py asserts on the CPU
that every case here has a decision margin of at least 8x that bound), exact ties, dead rows, broken tables, status codes, two runs
bit for bit; the n-best label score record against tests/vqa_eval_model.py; Decoder.answer_beam_async /
T5.constrained_beam_async against a host loop over the same cached logits, against the arg-max of teacher-forced sequence
log-probabilities and against the greedy list search; Trainer.test with answer_beams."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import answer_trie_model as AM  # noqa: E402
import trie_beam_cases as CS  # noqa: E402
import trie_beam_model as BM  # noqa: E402
import vqa_eval_model as VM  # noqa: E402
from m3ae_amd import _lib, metrics, ops, synth, trainer  # noqa: E402
from m3ae_amd.answer_trie import AnswerTrie  # noqa: E402
from oracle_util import gen_t5_weights, load_golden, tiny_batch, tiny_config  # noqa: E402

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
INT_FIELDS = ("node", "last_tok", "order", "done", "n_hyp", "labels", "hyp_len", "best", "len", "open_count", "err", "top_beam",
              "top_edge", "n_cand")


def on_device(x, dtype):
    """x float32 [R, ld] of values exact in `dtype` (NaN padding included) -> a device tensor of `dtype` with the same bits."""
    if dtype == torch.float32:
        return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    hi = (np.ascontiguousarray(x).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
    return torch.from_numpy(hi.copy()).view(torch.bfloat16).to(DEV)


def raw_table(t):
    """A table the test may corrupt: the arrays of `t` (an AnswerTrie or a namespace of numpy arrays) uploaded as they are."""
    return NS(child_off=torch.from_numpy(t.child_off).to(DEV), child_tok=torch.from_numpy(t.child_tok).to(DEV),
              child_node=torch.from_numpy(t.child_node).to(DEV), leaf_label=torch.from_numpy(t.leaf_label).to(DEV),
              N=len(t.leaf_label), E=len(t.child_tok), A=t.num_answers, depth=t.depth)


def dev_step(tab, st, xd, V, pos, chunk, lp, ws=None):
    xv = xd[:, :V]
    ws = ops.trie_scan(xv, tab, st, chunk, ws)
    ops.trie_beam_select(xv, tab, st, ws, chunk)
    ops.trie_beam_step(tab, st, V, pos, lp)
    return ws


def fetch(st):
    g = {k: getattr(st, k).cpu().numpy() for k in INT_FIELDS + ("beam_score", "scores", "logprob", "top_s")}
    g["dead"] = st.finished.cpu().numpy()
    return g


def assert_matches(got, snap, where, worst):
    """Integers exactly; every score within its derived bound of the float64 model.  worst[0] = the largest error / bound seen."""
    for k in INT_FIELDS + ("dead",):
        assert np.array_equal(got[k].reshape(-1), np.asarray(snap[k]).reshape(-1)), (where, k, got[k], snap[k])
    for k, e in (("top_s", "top_err"), ("beam_score", "beam_err"), ("logprob", "hyp_err"), ("scores", "hyp_nerr")):
        d = np.abs(got[k].astype(np.float64).reshape(-1) - np.asarray(snap[k], dtype=np.float64).reshape(-1))
        b = np.asarray(snap[e], dtype=np.float64).reshape(-1)
        assert (d <= b).all(), (where, k, d.max(), b)
        if (b > 0).any():
            worst[0] = max(worst[0], float((d[b > 0] / b[b > 0]).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CS.all_cases(), ids=CS.case_id)
def test_select_and_step_match_the_model(case):
    B, nb, V, ld, dname, chunk = case
    trie, steps, snaps, mod = CS.run_model(*case)
    for m_, b_ in zip(mod.margin, mod.bound):                      # asserted on the CPU too (tests/test_trie_beam_host.py)
        assert m_ >= CS.MARGIN_FACTOR * b_
    tab = trie.to_device(DEV, V, trie.depth + 1, pad_id=CS.PAD)
    st = ops.TrieBeamState(B, nb, trie.depth + 1, DEV, CS.START, CS.PAD)
    worst, ws = [0.0], None
    for pos, x in enumerate(steps):
        ws = dev_step(tab, st, on_device(x, DTYPES[dname]), V, pos, chunk, 1.0, ws)
        assert_matches(fetch(st), snaps[pos], (case, pos), worst)
    assert (mod.n_hyp >= 1).all() and mod.open_count[trie.depth - 1] == 0
    assert np.array_equal(ops.trie_beam_result(tab, st).cpu().numpy(), BM.answers_seq(trie, mod))
    print(f"{CS.case_id(case)}: largest |device - float64| / derived bound = {worst[0]:.3f}; bound <= {max(mod.bound):.3g}")


def test_two_runs_give_the_same_bits():
    case = (2, 8, 4099, 4100, "bf16", 256)
    B, nb, V = case[:3]
    trie, steps, _, _ = CS.run_model(*case)
    tab = trie.to_device(DEV, V, trie.depth + 1, pad_id=CS.PAD)
    outs = []
    for _ in range(2):
        st = ops.TrieBeamState(B, nb, trie.depth + 1, DEV, CS.START, CS.PAD)
        tops = []
        for pos, x in enumerate(steps):
            dev_step(tab, st, on_device(x, torch.bfloat16), V, pos, 256, 1.0)
            tops.append(torch.cat([st.top_s.view(torch.int32).flatten(), st.top_beam.flatten(), st.top_edge.flatten(),
                                   st.beam_score.view(torch.int32)]).clone())
        ops.trie_beam_result(tab, st)
        outs.append((st.out.clone(), torch.cat(tops)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_exact_ties_are_ordered_by_beam_and_token():
    """Equal logits at several children of one beam, and identical rows and scores in two beams: (beam, token) ascending, bit for
    bit.  Both beams sit at the same node with the same score, so their candidates tie pairwise; a -0 / +0 pair ties too."""
    V, nb = 300, 4
    seqs = [[t, 1] for t in (5, 9, 17, 33, 64, 65, 130, 299)]
    trie = AnswerTrie([[2] + s for s in seqs] + [[3, 7, 1]], (1,))
    tab = trie.to_device(DEV, V, 4, pad_id=0)
    node2 = trie.walk([2])
    lo = int(trie.child_off[node2])
    for dname, dtype in DTYPES.items():
        st = ops.TrieBeamState(1, nb, 4, DEV, 0, 0)
        st.node.copy_(torch.tensor([node2, -1, node2, node2], dtype=torch.int32))
        st.finished.copy_((st.node < 0).to(torch.int32))
        st.beam_score.copy_(torch.tensor([-1.5, 0.0, -1.5, -4.5]))
        x = np.full((nb, V), -3.0, dtype=np.float32)
        row = x[0]
        row[[9, 17, 130]] = 2.0                                 # a three-way tie at the top of a beam
        row[[5, 299]] = 0.5
        row[33], row[64] = 0.0, -0.0                            # equal values with different bits
        x[2] = row                                              # beam 2: the same row and the same score as beam 0
        x[3] = row                                              # beam 3: the same row, a lower score
        x[1] = np.nan                                           # the dead slot
        xd = on_device(x, dtype)
        ws = ops.trie_scan(xd, tab, st, 64)
        ops.trie_beam_select(xd, tab, st, ws, 64)
        beams, edges = st.top_beam.cpu().numpy()[0], st.top_edge.cpu().numpy()[0]
        toks = trie.child_tok[edges]
        assert list(zip(beams.tolist(), toks.tolist())) == [(0, 9), (0, 17), (0, 130), (2, 9), (2, 17), (2, 130), (0, 5), (0, 299)], dname
        s = st.top_s.cpu().numpy()[0].view(np.uint32)
        assert len(set(s[:6].tolist())) == 1 and len(set(s[6:].tolist())) == 1 and int(st.n_cand.cpu()) == 8
        assert (edges >= lo).all() and int(st.err.cpu()) == 0
        # the -0 / +0 pair: make them the best of a single live beam
        st.node.copy_(torch.tensor([node2, -1, -1, -1], dtype=torch.int32))
        x[0, [9, 17, 130, 5, 299]] = -3.0
        xd = on_device(x, dtype)
        ws = ops.trie_scan(xd, tab, st, 64)
        ops.trie_beam_select(xd, tab, st, ws, 64)
        toks = trie.child_tok[st.top_edge.cpu().numpy()[0]]
        assert toks[:2].tolist() == [33, 64] and st.top_s.cpu().numpy()[0, 0] == st.top_s.cpu().numpy()[0, 1], dname


def test_dead_and_done_rows_are_never_read_and_short_lists_leave_empty_slots():
    """A two-answer list at nb = 4: fewer than 2 nb candidates, n_cand and the -1 slots.  The logit rows of dead slots (and, once a
    sample is done, all of its rows) hold NaN in one run and numbers in the other: the same result, bit for bit."""
    V, nb, B = 257, 4, 2
    trie = AnswerTrie([[5, 6, 1], [5, 1]], (1,))
    tab = trie.to_device(DEV, V, 4, pad_id=0)
    rng = np.random.default_rng(3)
    xs = [rng.standard_normal((B * nb, V)).astype(np.float32) for _ in range(trie.depth)]
    runs = []
    for poison in (False, True):
        st = ops.TrieBeamState(B, nb, 4, DEV, 0, 0)
        mod = BM.State(B, nb, 4, 0, 0)
        log = []
        for pos, x in enumerate(xs):
            x = x.copy()
            if poison:
                x[mod.node < 0] = np.nan
            dev_step(tab, st, on_device(x, torch.float32), V, pos, 64, 0.0)
            BM.select(mod, trie, np.where(np.isnan(x), 0, x), 64)
            ncand = mod.n_cand.copy()
            BM.step(mod, trie, V, pos, 0.0)
            g = fetch(st)
            assert np.array_equal(g["n_cand"], ncand) and (ncand < 2 * nb).all()
            for b in range(B):
                assert (g["top_edge"][b, ncand[b]:] == -1).all() and (g["top_beam"][b, ncand[b]:] == -1).all()
                assert (g["top_s"][b, ncand[b]:] == 0).all() and (g["top_edge"][b, :ncand[b]] >= 0).all()
            assert np.array_equal(g["node"], mod.node) and np.array_equal(g["labels"], mod.labels)
            log.append(torch.cat([st.top_s.view(torch.int32).flatten(), st.top_edge.flatten(), st.beam_score.view(torch.int32)]).clone())
        assert int(st.err.cpu()) == 0 and (mod.n_hyp == 2).all() and mod.done.all()
        ops.trie_beam_result(tab, st)
        runs.append((st.out.clone(), torch.cat(log)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.isnan(runs[1][0][-2 * B * nb - B - 1:-B - 1].view(torch.float64)).any()


@pytest.mark.parametrize("what", ["node", "child_node"])
def test_a_table_value_out_of_range_sets_err_and_writes_nothing_out_of_range(what):
    V, nb, B = 300, 2, 2
    trie = AnswerTrie([[5, 6, 1], [5, 7, 1], [8, 1]], (1,))
    tab = raw_table(trie)
    st = ops.TrieBeamState(B, nb, 4, DEV, 0, 0)
    guard = torch.full((64,), 7, dtype=torch.int64, device=DEV)        # the state's neighbours in the allocator stay as they are
    if what == "node":
        st.node.copy_(torch.tensor([0, -1, tab.N + 5, -1], dtype=torch.int32))
    else:
        tab.child_node[:int(trie.child_off[1])] = tab.N + 9            # every child of the root points past the table
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B * nb, V)).astype(np.float32)).to(DEV)
    dev_step(tab, st, x, V, 0, 64, 0.0)
    g = fetch(st)
    assert int(g["err"][0]) == 1 and (guard == 7).all()
    assert ((g["node"] >= -1) & (g["node"] < tab.N)).all() and ((g["order"] >= 0) & (g["order"] < B * nb)).all()
    assert ((g["last_tok"] >= 0) & (g["last_tok"] < V)).all() and (g["best"] == 0).all()
    if what == "node":
        assert g["n_cand"].tolist() == [2, 0] and g["done"].tolist() == [0, 1] and g["node"][:2].min() >= 1
    else:
        assert g["n_cand"].tolist() == [2, 2] and g["done"].tolist() == [1, 1] and (g["node"] == -1).all() and (g["n_hyp"] == 0).all()


def test_bad_arguments_return_their_status():
    V, B, nb = 300, 2, 2
    tab = AnswerTrie([[5, 2], [6, 2]], (2,)).to_device(DEV, V, 4, pad_id=0)
    st = ops.TrieBeamState(B, nb, 4, DEV, 0, 0)
    R = B * nb
    x = torch.zeros((R, V), device=DEV)
    ws = ops.trie_scan(x, tab, st, 64)
    with pytest.raises(ValueError, match="num_beams"):
        ops.TrieBeamState(B, 9, 4, DEV)
    with pytest.raises(ValueError, match="pos"):
        ops.trie_beam_step(tab, st, V, 4)
    with pytest.raises(ValueError):
        ops.trie_beam_select(x[:1], tab, st, ws, 64)
    with pytest.raises(ValueError):
        ops.trie_beam_select(x, tab, st, ws[:, :2].contiguous(), 64)
    with pytest.raises(TypeError):
        ops.trie_beam_select(x.half(), tab, st, ws, 64)
    L = _lib.lib()
    p = lambda a: a.data_ptr()   # noqa: E731
    ARG, UNS, ALIGN, WS = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_ALIGN, _lib.ERR_WORKSPACE
    sel = [p(x), V, B, nb, V, 64, _lib.F32, p(tab.child_off), p(tab.child_tok), tab.N, tab.E, p(st.node), p(st.beam_score), p(ws),
           ws.numel() * 8, p(st.top_s), p(st.top_beam), p(st.top_edge), p(st.n_cand), p(st.err), None]
    for i, v, rc in ((0, None, ARG), (1, V - 1, ARG), (2, 0, ARG), (4, 0, ARG), (5, -1, ARG), (7, None, ARG), (8, None, ARG), (9, 0, ARG),
                     (10, 0, ARG), (11, None, ARG), (12, None, ARG), (15, None, ARG), (19, None, ARG), (6, 7, UNS), (3, 0, UNS), (3, 9, UNS),
                     (10, 2 ** 30, UNS), (5, 32, UNS), (5, 65537, UNS), (0, p(x) + 2, ALIGN), (12, p(st.beam_score) + 2, ALIGN),
                     (19, p(st.err) + 4, ALIGN), (13, None, WS), (13, p(ws) + 4, WS), (14, ws.numel() * 8 - 1, WS)):
        bad = list(sel)
        bad[i] = v
        assert L.m3ae_triebeam_select(*bad) == rc, (i, v)
    assert L.m3ae_triebeam_select(*sel) == 0
    step = [p(st.top_s), p(st.top_beam), p(st.top_edge), p(tab.child_off), p(tab.child_tok), p(tab.child_node), p(tab.leaf_label), tab.N,
            tab.E, p(st.node), p(st.beam_score), p(st.last_tok), p(st.order), p(st.finished), p(st.done), p(st.n_hyp), p(st.labels),
            p(st.scores), p(st.logprob), p(st.hyp_len), p(st.best), p(st.len), p(st.open_count), p(st.err), B, nb, V, tab.A, 4, 0, 0, 1.0,
            None]
    for i, v, rc in ((0, None, ARG), (6, None, ARG), (9, None, ARG), (23, None, ARG), (7, 0, ARG), (8, 0, ARG), (24, 0, ARG), (26, 0, ARG),
                     (27, 0, ARG), (28, 0, ARG), (29, -1, ARG), (29, 4, ARG), (31, 0.0, ARG), (31, float("nan"), ARG), (25, 0, UNS),
                     (25, 9, UNS), (8, 2 ** 30, UNS), (0, p(st.top_s) + 2, ALIGN), (17, p(st.scores) + 4, ALIGN), (11, p(st.last_tok) + 4, ALIGN)):
        bad = list(step)
        bad[i] = v
        assert L.m3ae_triebeam_step(*bad) == rc, (i, v)
    assert L.m3ae_triebeam_step(*step) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. m3ae_vqa_labels_eval
# ---------------------------------------------------------------------------------------------------------------------------------
SOFT = np.array([0.0, 0.0, 0.0, 0.3, 0.6, 0.9, 1.0, 0.1, 1.0 / 3.0, 2.0 ** -20], dtype=np.float32)   # {0} u [2^-20, 1]: exact sums


def labels_rows(tg, labels):
    """(hit1, hitk, err) of the n-best rule."""
    B, Cc = tg.shape
    h1, hk, err = np.zeros(B, np.float32), np.zeros(B, np.float32), 0
    for r in range(B):
        l0 = labels[r, 0]
        if 0 <= l0 < Cc:
            h1[r] = tg[r, l0]
        else:
            err = 1
        hk[r] = h1[r]
        for l in labels[r, 1:]:
            if l == -1:
                continue
            if not 0 <= l < Cc:
                err = 1
                continue
            hk[r] = max(hk[r], tg[r, l])
    return h1, hk, err


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_labels_eval_matches_the_fold_bit_for_bit(B, k):
    Cc = 498
    rng = np.random.default_rng(B * 100 + k)
    tg = rng.choice(SOFT, size=(B, Cc)).astype(np.float32)
    labels = rng.integers(0, Cc, size=(B, k)).astype(np.int64)
    labels[:, 1:][rng.random((B, k - 1)) < 0.3] = -1            # empty slots
    labels[0, 0] = Cc - 1
    buf = torch.full((B, Cc + 14), float("nan"), device=DEV)
    buf[:, :Cc] = torch.from_numpy(tg).to(DEV)
    td = buf[:, :Cc]
    wide = torch.full((B, 16), -7, dtype=torch.int64, device=DEV)   # a [B, k] view of a wider buffer: row stride 16
    wide[:, :k] = torch.from_numpy(labels).to(DEV)
    for ld_, lab in ((k, torch.from_numpy(labels).to(DEV)), (16, wide[:, :k])):
        for types in (None, rng.integers(0, 2, size=B).astype(np.int32)):
            h1, hk, e = labels_rows(tg, labels)
            assert e == 0
            one = VM.record(h1, hk, types)
            rec = ops.vqa_record(DEV)
            ty = None if types is None else torch.from_numpy(types).to(DEV)
            rows = ops.vqa_labels_eval(lab, td, ty, rec, want_rows=True)
            ops.vqa_labels_eval(lab, td, ty, rec)
            assert np.array_equal(rows.hit1.cpu().numpy(), h1) and int(rows.err.cpu()) == 0
            assert np.array_equal(rec.cpu().numpy(), 2 * one), (ld_, types is None)
    bad = labels.copy()                                          # one bad label: column 0 of a row (-1 there is no empty slot)
    bad[B // 2, 0] = -1
    if k > 1:
        bad[0, k - 1] = Cc
    h1, hk, e = labels_rows(tg, bad)
    rec = ops.vqa_record(DEV)
    rows = ops.vqa_labels_eval(torch.from_numpy(bad).to(DEV), td, None, rec, want_rows=True)
    assert e == 1 and int(rows.err.cpu()) == 1 and np.array_equal(rows.hit1.cpu().numpy(), h1)
    assert np.array_equal(rec.cpu().numpy(), VM.record(h1, hk, None))
    met = metrics.VQARADScore(DEV, k=5)
    met.update_labels(torch.from_numpy(labels).to(DEV), td, [1] * B)
    h1, hk, _ = labels_rows(tg, labels)
    assert met.result() == VM.result(VM.record(h1, hk, [1] * B)) and int(met.label_err.cpu()) == 0


def test_labels_eval_rejects_bad_arguments():
    lab, tg, rec = torch.zeros((4, 3), dtype=torch.int64, device=DEV), torch.zeros((4, 9), device=DEV), ops.vqa_record(DEV)
    for args in ((lab.int(), tg, None, rec), (lab[:, 0], tg, None, rec), (lab, tg[:3], None, rec), (lab, tg, None, None),
                 (torch.zeros((4, 17), dtype=torch.int64, device=DEV), tg, None, rec), (lab.t().contiguous().t(), tg, None, rec)):
        with pytest.raises(ValueError):
            ops.vqa_labels_eval(*args)
    L = _lib.lib()
    p = lambda a: a.data_ptr()   # noqa: E731
    err, ws = torch.zeros(1, dtype=torch.int64, device=DEV), torch.empty((4, 2), device=DEV)
    base = [p(lab), 3, 3, p(tg), 9, None, 4, 9, None, p(rec), p(err), p(ws), 32, None]
    for i, v, rc in ((0, None, -1), (3, None, -1), (9, None, -1), (10, None, -1), (6, 0, -1), (7, 0, -1), (2, 0, -1), (2, 17, -2), (1, 2, -2),
                     (4, 8, -2), (11, None, -2), (12, 31, -2), (0, p(lab) + 4, -3), (3, p(tg) + 2, -3), (9, p(rec) + 4, -3)):
        bad = list(base)
        bad[i] = v
        assert L.m3ae_vqa_labels_eval(*bad) == rc, (i, v)
    assert L.m3ae_vqa_labels_eval(*base) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the decoder head
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_LEN, SEP, START, PAD = 16, 102, 101, 0


def decoder_cfg(mode, **over):
    """The tiny decoder set-up of tests/test_gpu_greedy.py."""
    return tiny_config(compute_dtype=mode, image_size=64, hidden_size=768, num_heads=12, num_top_layer=1,
                       input_image_embed_size=128, input_text_embed_size=128, vocab_size=1000, vit_width=128,
                       vit_layers=2, text_hidden=128, text_layers=1, text_heads=2, text_inter=512,
                       mm_encoder_inputs_include_cls_feats=True, mm_encoder_inputs_include_imagetext_feats=False, **over)


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(mode):
        if mode not in cache:
            from m3ae_amd.modules import DecoderModel
            m = DecoderModel(decoder_cfg(mode), vocab_size=1200)
            synth.fill_deterministic(m)
            m.finalize("cuda", {"fp32": torch.float32, "bf16": torch.bfloat16, "fp32x3": torch.float32}[mode])
            m.eval()
            m.decoder.max_len = MAX_LEN
            cache[mode] = m
        return cache[mode]
    return get


@pytest.fixture(scope="module")
def feats():
    f = torch.from_numpy(load_golden("tiny_decoder.npz")["cls"]).to(DEV)
    return torch.cat([f, 0.5 * f, -f[:1]]).contiguous()


def answer_list(V, end, n=60, seed=11, longest=6):
    """n distinct answers of 1 .. `longest` tokens over a small alphabet (shared prefixes), one of them a prefix of another."""
    rng = np.random.default_rng(seed)
    alphabet = [int(a) for a in rng.permutation(V)[:12] if int(a) != end]
    seen = {(alphabet[0], end), (alphabet[0], alphabet[1], end), (end,)}
    while len(seen) < n:
        seen.add(tuple(int(rng.choice(alphabet)) for _ in range(int(rng.integers(1, longest + 1)))) + (end,))
    return [list(s) for s in sorted(seen)]


def check_against_host_loop(r, t, seqs, nb, B, logits_of, start, max_len, lp, itemsize):
    """The device search equals the numpy model run on the same cached step logits; the margin is asserted on the way."""
    mod, steps = BM.search(logits_of, t, B, nb, max_len, start, PAD, lp, 0, itemsize, stop_early=False)
    for m_, b_, h_ in zip(mod.margin, mod.bound, mod.hyp_ratio):
        assert m_ >= CS.MARGIN_FACTOR * b_ and h_ >= CS.MARGIN_FACTOR, (m_, b_, h_)
    assert steps == t.depth == r.steps and int(r.err.cpu()) == 0
    assert np.array_equal(r.labels.cpu().numpy(), mod.labels) and np.array_equal(r.n_hyp.cpu().numpy(), mod.n_hyp)
    assert np.array_equal(r.len.cpu().numpy(), mod.len) and np.array_equal(r.state.open_count.cpu().numpy(), mod.open_count)
    assert np.array_equal(r.seq.cpu().numpy(), BM.answers_seq(t, mod))
    assert (np.abs(r.logprob.cpu().numpy() - mod.logprob) <= mod.hyp_err).all()
    assert (np.abs(r.scores.cpu().numpy() - mod.scores) <= mod.hyp_nerr).all()
    assert torch.equal(r.label, r.labels[:, 0]) and torch.equal(r.score, r.scores[:, 0])
    for b in range(B):                                          # every returned sequence is the entry its label names
        assert r.seq[b, :int(r.len[b])].cpu().tolist() == seqs[int(r.label[b])]
    return mod


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_answer_beam_equals_a_host_loop_over_step_logits(models, feats, mode):
    d = models(mode).decoder
    nb, lp = 4, 1.0
    seqs = answer_list(1200, SEP, seed=16)      # a list whose decision margins are >= 8 bounds in all three modes (asserted below)
    t = AnswerTrie(seqs, (SEP,))
    r = d.answer_beam_async(feats, t, nb, lp, START, PAD, lookahead=None)
    B = feats.shape[0]
    R = B * nb
    enc_kv = d.dec_layers[d.num_layers - 1].cross_kv(feats.to(d.head_dtype)).repeat_interleave(nb, dim=0)
    cache = [torch.zeros((R, MAX_LEN, 2 * 768), dtype=d.head_dtype, device=DEV)]

    def logits_of(last_tok, order, pos):
        if order is not None:
            cache[0] = cache[0][torch.from_numpy(order).to(DEV)].contiguous()
        lg = d.step_logits(torch.from_numpy(last_tok).to(DEV).view(R, 1), pos, enc_kv, cache[0])
        assert lg.dtype == d.head_dtype
        return lg.float().cpu().numpy()

    check_against_host_loop(r, t, seqs, nb, B, logits_of, START, MAX_LEN, lp, 2 if d.head_dtype == torch.bfloat16 else 4)
    for la in (0, 2):                                           # at most depth steps, the same result
        q = d.answer_beam_async(feats, t, nb, lp, START, PAD, lookahead=la)
        assert q.steps <= t.depth and torch.equal(q.out, r.out), la
    q = d.answer_beam_async(feats, t, nb, lp, START, PAD, lookahead=None, chunk=256)
    assert torch.equal(q.labels, r.labels) and torch.equal(q.seq, r.seq)
    from m3ae_amd.search import answer_result
    labels, scores = answer_result(r)
    assert torch.equal(labels, r.label.cpu()) and torch.equal(scores, r.score.cpu())
    l3, s3 = answer_result(r, k=3)
    assert torch.equal(l3, r.labels.cpu()[:, :3]) and torch.equal(s3, r.scores.cpu()[:, :3])
    named = answer_result(r, {str(i): f"answer {i}" for i in range(len(seqs))}, k=3)
    assert [[a for a, _ in row] for row in named] == [[f"answer {l}" for l in row if l >= 0] for row in l3.tolist()]
    with pytest.raises(ValueError):
        answer_result(r, k=nb + 1)


FP32_LOGIT = lambda mx: 1e-5 + 1e-5 * mx     # noqa: E731  tests/test_gpu_model.py: cached step against full prefix, rtol = atol = 1e-5
BF16_LOGIT = lambda mx: 2.0 ** -7 * mx       # noqa: E731  one bf16 ulp of the row's largest logit (no documented tolerance: gap only)
EXACT_LOGIT = lambda mx: 0.0                 # noqa: E731  tests/test_gpu_model.py: T5's cached step equals the full-prefix pass bit for bit


def teacher_forced(seqs, logits_full_of, start, itemsize, per_logit):
    """Per list entry, from full-prefix logits (logits_full_of(prefix ids incl. start) -> [T, V]): the float64 sum of
    log p(a[t] | a[<t]); the derived bound of tests/trie_beam_model.py accumulated along the entry's OWN rows,
    err_k = (err_(k-1) + tb_k + u |SCORE_k|)(1 + 2^-20); and the allowance for cached-versus-full-prefix logits, 2 * per_logit(max |x|)
    per step (a log-probability moves by at most twice the largest logit error)."""
    lp, derived, cached = [], [], []
    for s in seqs:
        lg = np.ascontiguousarray(logits_full_of([start] + list(s[:-1])), dtype=np.float32)
        tot, err, cac = 0.0, 0.0, 0.0
        for t, tok in enumerate(s):
            rs = BM.RowStats(lg[t], 0, itemsize)
            term = np.float64(lg[t, tok]) - rs.LSE
            tot += term
            err = (err + rs.term_bound(term) + BM.U * abs(tot)) * BM.TM.SLACK
            cac += 2.0 * per_logit(float(np.abs(lg[t]).max()))
        lp.append(tot)
        derived.append(err)
        cached.append(cac)
    return np.asarray(lp), np.asarray(derived), np.asarray(cached)


def check_exhaustive(r, b, seqs, lp, derived, cached, check_scores, tag):
    """Sample b of an exhaustive search (num_beams >= entries, length_penalty 0) against the teacher-forced float64 scores: every
    entry is listed; where the best two entries are further apart than the tolerances of both (a condition on the inputs), the
    label is the arg-max; with check_scores every score is within the entry's derived bound plus its documented allowance.
    Returns whether the arg-max was decided."""
    labels, scores = r.labels[b].cpu().numpy(), r.scores[b].cpu().numpy()
    tol = derived + cached
    order = np.argsort(-lp, kind="stable")
    gap, need = lp[order[0]] - lp[order[1]], tol[order[0]] + tol[order[1]]
    worst = float(np.abs(scores - lp[labels]).max())
    print(f"{tag} sample {b}: top-two gap {gap:.3g}, needed {need:.3g}; largest |score - float64| {worst:.3g}, derived bound "
          f"{derived.max():.3g}, allowance {cached.max():.3g}")
    assert int(r.n_hyp[b]) == len(seqs) and sorted(labels.tolist()) == list(range(len(seqs)))
    assert np.array_equal(r.logprob[b].cpu().numpy(), scores)            # length_penalty 0: div = 1
    assert (np.diff(scores) <= 0).all()
    decided = bool(gap > need)
    if decided:
        assert labels[0] == order[0], (tag, b, labels, order)
    if check_scores:
        assert (np.abs(scores - lp[labels]) <= tol[labels]).all(), (tag, b, np.abs(scores - lp[labels]), tol[labels])
    return decided


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_eight_beams_find_the_maximum_likelihood_entry_of_a_short_list(models, feats, mode):
    """<= 8 answers, num_beams = 8, length_penalty = 0: exhaustive, so all entries are listed and label = arg-max of the
    teacher-forced sequence log-probabilities (float64, from the same mode's full-prefix forward).  fp32: the scores agree within
    the derived bound accumulated over the entry's rows plus the cached-versus-full-prefix tolerance of tests/test_gpu_model.py, and
    the arg-max is decided for every sample.  fp32x3 and bf16 have no documented cached-versus-full-prefix tolerance: no score
    comparison; the arg-max is held wherever the top-two gap exceeds the allowance (fp32's figure; one bf16 ulp per logit)."""
    d = models(mode).decoder
    seqs = answer_list(1200, SEP, n=8, seed=4, longest=4)
    t = AnswerTrie(seqs, (SEP,))
    r = d.answer_beam_async(feats, t, 8, 0.0, START, PAD, lookahead=None)
    assert int(r.err.cpu()) == 0
    bf16 = d.head_dtype == torch.bfloat16
    decided = 0
    for b in range(feats.shape[0]):
        def full(prefix):
            ids = torch.tensor([prefix], device=DEV)
            return d(ids, None, feats[b:b + 1])[0].detach().float().cpu().numpy()
        lp, derived, cached = teacher_forced(seqs, full, START, 2 if bf16 else 4, BF16_LOGIT if bf16 else FP32_LOGIT)
        decided += check_exhaustive(r, b, seqs, lp, derived, cached, mode == "fp32", f"decoder {mode}")
    assert decided == feats.shape[0], decided     # the fixture decides the arg-max of every sample in every mode


def blocking_guard(monkeypatch, run):
    """tests/test_gpu_answer_trie.py's: `run` under torch.cuda.set_sync_debug_mode("error") where that raises on this torch / ROCm
    pair; otherwise counts calls of Tensor.cpu / item / tolist / __bool__ and torch.cuda.synchronize."""
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            live = False
        except RuntimeError:
            live = True
        if live:
            r = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not live:
        calls = []
        for name in ("cpu", "item", "tolist", "__bool__"):
            real = getattr(torch.Tensor, name)
            monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _r=real, _n=name, **k: (calls.append(_n) if self.is_cuda else None, _r(self, *a, **k))[1])
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
        r = run()
        monkeypatch.undo()
        assert calls == [], calls
    return r


def test_one_beam_is_the_greedy_list_search_and_the_async_form_never_waits(models, feats, monkeypatch):
    d = models("fp32").decoder
    seqs = answer_list(1200, SEP)
    t = AnswerTrie(seqs, (SEP,))
    g = d.answer_path_async(feats, t, START, PAD, lookahead=None)
    r = d.answer_beam_async(feats, t, 1, 0.0, START, PAD, lookahead=None)
    assert torch.equal(r.label, g.label) and torch.equal(r.seq, g.seq) and torch.equal(r.len, g.len)
    gs, rs = g.score.cpu().numpy(), r.score.cpu().numpy()
    assert (np.abs(gs - rs) <= t.depth * 2.0 ** -23 * np.abs(gs)).all()     # fp32 running sum against greedy's double sum
    want = d.answer_beam_async(feats, t, 4, 0.0, START, PAD, lookahead=None)   # warm: the answers table is uploaded
    q = blocking_guard(monkeypatch, lambda: d.answer_beam_async(feats, t, 4, 0.0, START, PAD, lookahead=None))
    assert q.steps == t.depth and torch.equal(q.out, want.out)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the T5 head
# ---------------------------------------------------------------------------------------------------------------------------------
def build_t5(mode):
    from m3ae_amd.modules.t5 import T5ForConditionalGeneration
    from m3ae_amd.param_store import ParamStore, group_hparams_decoder, param_group_of_decoder
    m = T5ForConditionalGeneration(dict(d_model=512, d_kv=64, d_ff=2048, num_layers=2, num_decoder_layers=2, num_heads=8), 1100)
    sd = gen_t5_weights({"t5." + k: v for k, v in m.state_dict().items()})
    m.load_state_dict({k[3:]: v for k, v in sd.items()})
    dtype = DTYPES[mode]
    ParamStore(m, tiny_config(compute_dtype=mode), "cuda", dtype, m.weight_units, group_fn=param_group_of_decoder,
               hparams_fn=group_hparams_decoder)
    m.eval()
    return m, torch.from_numpy(load_golden("tiny_t5_generate.npz")["enc"]).to(DEV).to(dtype)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_constrained_beam_equals_a_host_loop_and_the_teacher_forced_arg_max(mode, monkeypatch):
    m, enc = build_t5(mode)
    EOS, ML, nb, lp = 1, 8, 4, 1.0
    seqs = answer_list(1100, EOS, n=40, seed=7)    # a list whose decision margins are >= 8 bounds in both modes (asserted below)
    t = AnswerTrie(seqs, (EOS,))
    r = m.constrained_beam_async(enc, t, nb, ML, lp, PAD, lookahead=None)
    B, Ls = enc.shape[0], enc.shape[1]
    R = B * nb
    assert tuple(r.seq.shape) == (B, ML)
    enc_r = enc.repeat_interleave(nb, dim=0).contiguous()
    cross_kv = [kv.view(B, Ls, -1).repeat_interleave(nb, dim=0).reshape(R * Ls, -1) for kv in m.decoder.cross_kv(enc)]
    cache = [m.decoder.new_self_cache(R, ML, enc.dtype, DEV)]
    for c in cache[0]:
        c.zero_()

    def logits_of(last_tok, order, pos):
        if order is not None:
            o = torch.from_numpy(order).to(DEV)
            cache[0] = [c[o].contiguous() for c in cache[0]]
        return m.next_token_logits_cached(enc_r, torch.from_numpy(last_tok).to(DEV).view(R, 1), cross_kv, cache[0], pos).cpu().numpy()

    check_against_host_loop(r, t, seqs, nb, B, logits_of, m.config.decoder_start_token_id, ML, lp, 4)
    for la in (0, 2):
        q = m.constrained_beam_async(enc, t, nb, ML, lp, PAD, lookahead=la)
        assert q.steps <= t.depth and torch.equal(q.out, r.out), la
    q = blocking_guard(monkeypatch, lambda: m.constrained_beam_async(enc, t, nb, ML, lp, PAD, lookahead=None))
    assert torch.equal(q.out, r.out)
    g = m.constrained_greedy_async(enc, t, max_length=ML, pad_token_id=PAD, lookahead=None)
    one = m.constrained_beam_async(enc, t, 1, ML, 0.0, PAD, lookahead=None)
    with pytest.raises(ValueError, match="room for"):
        m.constrained_beam_async(enc, t, nb, t.depth - 1)
    assert torch.equal(one.label, g.label) and torch.equal(one.seq, g.seq) and torch.equal(one.len, g.len)
    # exhaustive on a short list.  fp32: the cached step equals the full-prefix pass bit for bit (tests/test_gpu_model.py), so the
    # tolerance is the derived bound accumulated over the entry's rows alone.  bf16: no documented tolerance, so no score comparison;
    # the arg-max is held wherever the top-two gap exceeds one bf16 ulp per logit
    short = answer_list(1100, EOS, n=8, seed=9, longest=4)
    ts = AnswerTrie(short, (EOS,))
    e = m.constrained_beam_async(enc, ts, 8, ML, 0.0, PAD, lookahead=None)
    assert int(e.err.cpu()) == 0
    kv = m.decoder.cross_kv(enc)
    decided = 0
    for b in range(B):
        kvb = [k.view(B, Ls, -1)[b].contiguous() for k in kv]

        def full(prefix):
            rows = [m.next_token_logits(enc[b:b + 1], torch.tensor([prefix[:i + 1]], device=DEV), kvb)[0].cpu().numpy()
                    for i in range(len(prefix))]
            return np.stack(rows)
        lpv, derived, cached = teacher_forced(short, full, m.config.decoder_start_token_id, 4, EXACT_LOGIT if mode == "fp32" else BF16_LOGIT)
        decided += check_exhaustive(e, b, short, lpv, derived, cached, mode == "fp32", f"t5 {mode}")
    assert decided == B, decided                  # the fixture decides the arg-max of every sample in both modes


@pytest.mark.parametrize("depth", [3, 1])
def test_list_beam_searches_enqueue_scan_select_step_per_position(models, feats, monkeypatch, depth):
    """Decoder.answer_beam_async and T5.constrained_beam_async, B = 2, two beams, no early exit, under a recording proxy of the
    library: scan, select, step per position of the trie and nothing else of the search families; the caches are re-ordered between
    steps only and the best entries' rows are gathered at the end (depth 1: a single step, no re-ordering, the result still
    gathered).  Depth 3: three answers, every returned row is the entry its label names.  Depth 1: two one-token answers (a second
    end id), two beams = exhaustive, so `labels` is the float64 ranking of the two tokens' log-probabilities at position 0."""
    d = models("fp32").decoder
    t5, enc = build_t5("fp32")
    f2, enc, ML, nb = feats[:2].contiguous(), enc[:2].contiguous(), 4, 2
    enc_kv = d.dec_layers[d.num_layers - 1].cross_kv(f2.to(d.head_dtype))
    first_dec = d.step_logits(torch.full((2, 1), START, device=DEV), 0, enc_kv, torch.empty((2, 1, 2 * 768), dtype=d.head_dtype, device=DEV))
    start = t5.config.decoder_start_token_id
    first_t5 = t5.next_token_logits_cached(enc, torch.full((2, 1), start, device=DEV), t5.decoder.cross_kv(enc),
                                           t5.decoder.new_self_cache(2, 1, enc.dtype, DEV), 0)
    L = _lib.lib()
    for end, first, run in ((SEP, first_dec, lambda t: d.answer_beam_async(f2, t, nb, 0.0, START, PAD, lookahead=None)),
                            (1, first_t5, lambda t: t5.constrained_beam_async(enc, t, nb, ML, 0.0, PAD, lookahead=None))):
        seqs, ends = ([[7, 8, end], [7, 9, end], [11, end]], (end,)) if depth == 3 else ([[end], [7]], (end, 7))
        t = AnswerTrie(seqs, ends)
        run(t)                                                  # warm: the trie and its answers table are uploaded
        names = []

        class Recording:
            def __getattr__(self, name):
                names.append(name)
                return getattr(L, name)
        monkeypatch.setattr(_lib, "_lib", Recording())
        r = run(t)
        monkeypatch.undo()
        search = [n for n in names if n.startswith(("m3ae_greedy_", "m3ae_beam_", "m3ae_trie_", "m3ae_triebeam_")) and not n.endswith("_workspace_bytes")]
        assert search == ["m3ae_trie_scan", "m3ae_triebeam_select", "m3ae_triebeam_step"] * depth
        last = len(names) - 1 - names[::-1].index("m3ae_triebeam_step")
        assert names[last + 1:] == ["m3ae_gather_rows"]          # the result's rows; no re-ordering after the last step
        assert r.steps == depth == t.depth and int(r.err.cpu()) == 0
        assert torch.equal(r.label, r.labels[:, 0]) and r.n_hyp.cpu().tolist() == [2, 2]
        for b in range(2):
            assert r.seq[b, :int(r.len[b])].cpu().tolist() == seqs[int(r.label[b])]
        if depth == 1:
            logp = torch.log_softmax(first.double(), dim=-1)[:, [end, 7]].cpu()
            gap = (logp[:, 0] - logp[:, 1]).abs()
            print(f"end id {end}: float64 log-probabilities of the two answers {logp.tolist()}")
            assert (gap > 1e-4).all()                           # a condition on the inputs: far above fp32's error on one row
            assert r.labels.cpu().tolist() == torch.argsort(-logp, dim=1).tolist()
            assert (r.scores.cpu() - torch.sort(logp, dim=1, descending=True).values).abs().max() < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. Trainer.test
# ---------------------------------------------------------------------------------------------------------------------------------
class ListDM:
    train_samples = 8

    def __init__(self, batches):
        self.batches = batches

    def val_batches(self):
        return iter(self.batches)

    def train_batches(self, epoch):
        return iter(self.batches)


def to_dev(b):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and v
                and isinstance(v[0], torch.Tensor) else v) for k, v in b.items()}


def counting_lib(monkeypatch):
    L = _lib.lib()
    counts = {}

    class Counting:
        def __getattr__(self, name):
            if name.startswith("m3ae_trie") or name.startswith("m3ae_vqa_label"):
                counts[name] = counts.get(name, 0) + 1
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Counting())
    return counts


def test_trainer_test_with_answer_beams_logs_at_k_and_one_beam_launches_what_it_did(tmp_path, monkeypatch):
    from m3ae_amd.modules import DecoderModel
    out = {}
    for beams in (1, 4):
        cfg = decoder_cfg("fp32", vqa_metrics="device", answer_decoding="list", answer_beams=beams, answer_length_penalty=0.0, eval_topk=3,
                          per_gpu_batchsize=2, batch_size=2, max_steps=1, log_dir=str(tmp_path))
        m = DecoderModel(cfg, vocab_size=1200)
        synth.fill_deterministic(m)
        m.finalize(DEV, torch.float32)
        m.eval()
        m.decoder.max_len = 8
        b = to_dev(tiny_batch())
        b["decoder_tokens"] = torch.tensor([[m.cls_id, 1000, m.sep_id], [m.cls_id, 1001, m.sep_id]], device=DEV)
        b["answer_types"] = [0, 1]
        Cc = cfg["vqa_label_size"]
        seqs = answer_list(1200, m.sep_id, n=min(40, Cc), seed=2)
        b["vqa_targets"] = torch.from_numpy(np.random.default_rng(1).choice(SOFT[3:], size=(2, Cc)).astype(np.float32)).to(DEV)
        tr = trainer.Trainer(cfg, m, ListDM([b, b]), 0, 1, torch.device("cuda", torch.cuda.current_device()))
        assert tr.answer_beams == beams
        tr.answer_trie = AnswerTrie(seqs, (m.sep_id,))
        counts = counting_lib(monkeypatch)
        out[beams] = tr.test()
        monkeypatch.undo()
        m.eval()                                                # test() leaves the model in train(): the calls below must not draw dropout masks
        tg = b["vqa_targets"].cpu().numpy()
        if beams == 1:                                          # the launches of the greedy list search, and no new entry point
            assert set(counts) == {"m3ae_trie_workspace_bytes", "m3ae_trie_scan", "m3ae_trie_step", "m3ae_vqa_label_eval"}, counts
            assert counts["m3ae_vqa_label_eval"] == 2 and counts["m3ae_trie_scan"] == counts["m3ae_trie_step"] >= 2
            assert "@" not in tr.answer_text() and tr.answer_k == 1
            continue
        assert counts["m3ae_vqa_labels_eval"] == 2 and "m3ae_vqa_label_eval" not in counts and "m3ae_trie_step" not in counts
        assert counts["m3ae_trie_scan"] == counts["m3ae_triebeam_select"] == counts["m3ae_triebeam_step"] >= 2
        labels, scores = m.answer(b, tr.answer_trie, num_beams=4, k=3)
        assert tuple(labels.shape) == (2, 3) and (np.diff(scores.numpy(), axis=1) <= 0).all()
        h1, hk, e = labels_rows(tg, labels.numpy())
        want = VM.result(2 * VM.record(h1, hk, [0, 1]))
        assert e == 0 and tr.answer_metrics == want and tr.answer_k == 3
        assert tr.answer_text().endswith(f" @3 {want['score_at_k']:.4f}") and f"open {want['open']:.4f} (2)" in tr.answer_text()
        pairs = m.answer(b, tr.answer_trie, {str(i): f"a{i}" for i in range(len(seqs))}, num_beams=4, k=3)
        assert [[a for a, _ in row] for row in pairs] == [[f"a{l}" for l in row] for row in labels.tolist()]
    assert abs(out[1] - out[4]) <= 1e-5 * abs(out[1])           # the monitored quantity stays the negative loss
