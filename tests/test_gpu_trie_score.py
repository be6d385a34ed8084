"""GPU: exhaustive answer-list scoring (csrc/tree_attn.hip, csrc/list_score.hip) -- m3ae_tree_attn against float64 within the bound
derived from its documented order of operations, m3ae_listscore_lse / _edges / _fold against the numpy model of
tests/trie_score_model.py (integers exactly, floats within the derived bounds, two runs bit for bit, an entry's log-probability bit
for bit what m3ae_trie_scan + m3ae_trie_step accumulate along its path); Decoder.answer_scores_async against the float64
teacher-forced sums of the full-prefix forward and against the exhaustive beam search; Trainer.test with answer_scoring;
T5ForConditionalGeneration.list_scores_async against its own full-prefix pass and its exhaustive beam search."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import answer_trie_model as AM  # noqa: E402
import trie_score_cases as CS  # noqa: E402
import trie_score_model as SM  # noqa: E402
from m3ae_amd import _lib, ops, synth, trainer  # noqa: E402
from m3ae_amd.answer_trie import AnswerTrie  # noqa: E402
from oracle_util import load_golden, tiny_batch, tiny_config  # noqa: E402

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
START, PAD, SEP, MAX_LEN = 101, 0, 102, 16
GUARD = 12345.0


def dev_of(x, dtype):
    """float32 values exact in `dtype` -> a device tensor of that dtype with the same values (NaN stays NaN)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. m3ae_tree_attn
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CS.ATTN_CASES, ids=lambda c: "G{}-{}-H{}-Dh{}-{}-scale{}-bias{}-mag{}".format(*c))
def test_tree_attention_is_within_the_derived_bound_of_float64(case):
    G, name, H, Dh, dname, _, _, _ = case
    anc, q, k, v, rb, scale = CS.attn_inputs(*case)
    dtype, D = DTYPES[dname], H * Dh
    Ni = anc.shape[0]
    want, bound, err, smax = SM.tree_attn(q, k, v, anc, H, scale, rb, dname == "bf16")
    assert err == 0 and (smax > 80 if case[7] > 3 else True)                          # the large case: scores of magnitude 80
    ancd = torch.from_numpy(anc).to(DEV)
    rbd = None if rb is None else torch.from_numpy(rb).to(DEV)
    packed = torch.cat([dev_of(q, dtype), dev_of(k, dtype), dev_of(v, dtype)], dim=-1)          # strided thirds of one buffer
    errw = torch.zeros(1, dtype=torch.int64, device=DEV)
    for form in ("packed", "separate"):
        if form == "packed":
            qd, kd, vd = packed[..., :D], packed[..., D:2 * D], packed[..., 2 * D:]
        else:
            qd, kd, vd = (t.contiguous() for t in (packed[..., :D], packed[..., D:2 * D], packed[..., 2 * D:]))
        out = ops.tree_attention(qd, kd, vd, ancd, H, scale, rbd, errw)
        again = ops.tree_attention(qd, kd, vd, ancd, H, scale, rbd, errw)
        assert out.dtype == dtype and tuple(out.shape) == (G, Ni, D) and torch.equal(out, again)     # two runs: the same bits
        got = out.float().cpu().numpy().astype(np.float64)
        e = np.abs(got - want)
        ratio = float((e / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0
        print(f"tree_attn {case} {form}: largest error {e.max():.3g}, largest error / bound {ratio:.3g}")
        assert np.isfinite(got).all() and (e <= bound).all()
        one_key = (anc >= 0).sum(1) == 1                                                          # one key: the output is v
        assert np.array_equal(got[:, one_key], v[:, one_key].astype(np.float64))
    assert int(errw.cpu()) == 0
    if name == "deep32":
        assert (anc >= 0).sum(1).max() == 32
    if name in ("flat", "ni67"):                     # the row counts the issue names: one row, and 67 (more than a wave of rows)
        assert Ni == {"flat": 1, "ni67": 67}[name]


def test_tree_attention_with_a_table_value_out_of_range():
    """Row 3 names a row past Ni, row 5 has no entry at all: err is set, those rows are zeros, every other row is what the intact
    table gives, and the guard rows around the output keep their value."""
    anc, q, k, v, _, scale = CS.attn_inputs(1, "gen60", 2, 96, "fp32", None, False, 1.0)
    Ni, D = anc.shape[0], 192
    bad = anc.copy()
    bad[3, 1], bad[5, :] = Ni, -1
    L = _lib.lib()
    qd, kd, vd = (dev_of(a, torch.float32)[0].contiguous() for a in (q, k, v))
    buf = torch.full((Ni + 2, D), GUARD, device=DEV)
    errw = torch.zeros(1, dtype=torch.int64, device=DEV)
    p = lambda a: a.data_ptr()   # noqa: E731
    badd, ancd = torch.from_numpy(bad).to(DEV), torch.from_numpy(anc).to(DEV)
    args = [p(qd), D, p(kd), D, p(vd), D, p(buf[1:]), D, p(badd), anc.shape[1], None, scale, 1, Ni, 2, 96, _lib.F32, p(errw), None]
    assert L.m3ae_tree_attn(*args) == 0
    good = ops.tree_attention(qd, kd, vd, ancd, 2)
    torch.cuda.synchronize()
    assert int(errw.cpu()) == 1 and (buf[0] == GUARD).all() and (buf[-1] == GUARD).all()
    keep = [i for i in range(Ni) if i not in (3, 5)]
    assert (buf[1:][[3, 5]] == 0).all() and torch.equal(buf[1:][keep], good[keep])
    ARG, UNS, ALIGN = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_ALIGN
    args[8] = p(ancd)
    for i, val, rc in ((0, None, ARG), (6, None, ARG), (8, None, ARG), (17, None, ARG), (1, D - 1, ARG), (7, D - 1, ARG), (12, 0, ARG),
                       (13, 0, ARG), (9, 0, ARG), (9, 33, UNS), (15, 32, UNS), (16, 7, UNS), (0, p(qd) + 2, ALIGN), (17, p(errw) + 4, ALIGN)):
        b = list(args)
        b[i] = val
        assert L.m3ae_tree_attn(*b) == rc, (i, val)
    with pytest.raises(ValueError):
        ops.tree_attention(qd, kd, vd[:-1], ancd, 2)
    with pytest.raises(ValueError):
        ops.tree_attention(qd, kd, vd, ancd.long(), 2)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. m3ae_listscore_*
# ---------------------------------------------------------------------------------------------------------------------------------
def on_device(x, dtype, ld):
    """x float32 [R, ld] -> the [R, V] view of a device buffer with the same bits in `dtype` (the pad columns hold NaN)."""
    return dev_of(x, dtype)[:, :CS.V]


def run_kernels(trie, xd, G, k, lp, chunk):
    dt = trie.score_to_device(DEV, CS.V, MAX_LEN + 16, PAD)
    st = ops.ListScoreState(G, k, MAX_LEN + 16, dt, DEV, PAD)
    ws = ops.listscore_lse(xd, chunk)
    ops.listscore_edges(xd, dt, st, ws, 0, chunk)
    ops.listscore_fold(dt, st, lp)
    return dt, st, ws


def close(got, want, bound, what):
    """Finite values within the bound, non-finite values equal."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), what
    e = np.abs(got[fin] - want[fin])
    b = np.broadcast_to(bound, want.shape)[fin]
    if e.size:
        print(f"{what}: largest error {e.max():.3g}, largest error / bound {float((e / np.maximum(b, 1e-300)).max()):.3g}")
    assert (e <= b).all(), (what, e.max())


@pytest.mark.parametrize("case", CS.CASES, ids=CS.case_id)
def test_list_scores_match_the_model(case):
    name, ld, dname, chunk, G, k, lp, special = case
    trie, x, edge, eb, r = CS.run_model(case)
    xd = on_device(x, DTYPES[dname], ld)
    assert xd.stride(0) == ld
    dt, st, ws = run_kernels(trie, xd, G, k, lp, chunk)
    h = st.host()
    tag = CS.case_id(case)
    assert np.array_equal(h.labels.numpy(), r["labels"]) and np.array_equal(h.n_hyp.numpy(), r["n_hyp"])
    assert np.array_equal(h.len.numpy(), r["len"]) and np.array_equal(st.best.cpu().numpy(), r["best"])
    assert np.array_equal(h.seq.numpy(), trie.answers_table(MAX_LEN + 16, PAD)[r["best"]])
    close(st.edge_lp.cpu().numpy(), edge, eb, tag + " edge_lp")
    close(st.all_logprob.cpu().numpy(), r["all_logprob"], r["all_bound"], tag + " all_logprob")
    kk = int(r["n_hyp"][0])
    top = r["labels"][:, :kk]
    close(h.scores.numpy()[:, :kk], r["scores"][:, :kk], np.take_along_axis(r["all_score_bound"], top, 1), tag + " scores")
    close(h.logprob.numpy()[:, :kk], r["logprob"][:, :kk], np.take_along_axis(r["all_bound"], top, 1), tag + " logprob")
    close(h.probs.numpy()[:, :kk], r["probs"][:, :kk], np.take_along_axis(r["probs_bound"], top, 1), tag + " probs")
    close(h.log_mass.numpy(), r["log_mass"], r["mass_bound"], tag + " log_mass")
    assert (h.scores.numpy()[:, kk:] == 0).all() and (h.probs.numpy()[:, kk:] == 0).all() and (h.labels.numpy()[:, kk:] == -1).all()
    assert np.array_equal(h.labels.numpy()[:, 0], st.label.cpu().numpy()) and np.array_equal(h.scores.numpy()[:, 0], st.score.cpu().numpy())
    _, again, ws2 = run_kernels(trie, xd, G, k, lp, chunk)                     # two runs: the same bits
    assert torch.equal(again.out, st.out) and torch.equal(again.all_logprob.view(torch.int64), st.all_logprob.view(torch.int64))
    assert torch.equal(again.edge_lp.view(torch.int32), st.edge_lp.view(torch.int32)) and torch.equal(ws, ws2)
    if special == "nonfinite":
        alp = st.all_logprob.cpu().numpy()
        assert np.isneginf(alp[0]).any() and np.isnan(alp[1]).any() and np.isfinite(h.log_mass.numpy()).all()


def test_exact_ties_are_ordered_by_label():
    """Two root children with the same logit whose own rows are copies: their entries' log-probabilities have the same bits, and
    the lower label ranks first, whichever of the two sits at the top."""
    trie = AnswerTrie(CS.LISTS["wide300"](), (CS.END,))
    t = trie.score_tables()
    Ni = len(t["internal"])
    x = (np.random.default_rng(5).standard_normal((Ni, CS.V)) * 2).astype(np.float32)
    a, b = 40, 200                                   # root children = labels (one-token answers in token order)
    x[0, trie.child_tok[a]] = x[0, trie.child_tok[b]] = 30.0
    x[t["row_of"][1 + b]] = x[t["row_of"][1 + a]]
    _, st, _ = run_kernels(trie, torch.from_numpy(x).to(DEV), 1, 4, 0.0, 0)
    h = st.host()
    assert h.labels[0, :2].tolist() == [a, b] and h.scores[0, 0] == h.scores[0, 1] and h.scores[0, 1] > h.scores[0, 2]


def test_a_broken_table_sets_err_and_writes_nothing_outside_its_buffers():
    trie = AnswerTrie(CS.LISTS["prefix"](), (CS.END,))
    good = trie.score_to_device(DEV, CS.V, MAX_LEN, PAD)
    Ni = good.Ni
    x = torch.from_numpy((np.random.default_rng(1).standard_normal((2 * Ni, CS.V))).astype(np.float32)).to(DEV)
    for what in ("internal", "child_tok", "parent", "leaf_node", "level_off"):
        dt = NS(**vars(good))
        broken = getattr(good, what).clone()
        broken[1 if what != "level_off" else 2] = 10 ** 6
        setattr(dt, what, broken)
        st = ops.ListScoreState(2, 3, MAX_LEN, dt, DEV, PAD)
        L = _lib.lib()
        p = lambda a: a.data_ptr()   # noqa: E731
        ws = ops.listscore_lse(x, 0)
        edge = torch.full((2 + 2, trie.num_edges), GUARD, device=DEV)
        alp = torch.full((2 + 2, trie.num_answers), GUARD, dtype=torch.float64, device=DEV)
        assert L.m3ae_listscore_edges(p(x), x.stride(0), 2, Ni, CS.V, _lib.F32, p(ws), ws.numel() * 8, 1, p(dt.internal), p(dt.child_off),
                                      p(dt.child_tok), dt.N, dt.E, p(edge[1:]), p(st.err), None) == 0
        pen = torch.ones(trie.depth + 1, dtype=torch.float64, device=DEV)
        assert L.m3ae_listscore_fold(p(edge[1:]), p(dt.parent), p(dt.node_depth), p(dt.level_off), p(dt.leaf_node), p(pen), 2, dt.N, dt.A,
                                     trie.depth, 3, None, 0, p(alp[1:]), p(st.labels), p(st.scores), p(st.logprob), p(st.probs),
                                     p(st.log_mass), p(st.n_hyp), p(st.best), p(st.len), p(st.err), None) == 0
        torch.cuda.synchronize()
        assert int(st.err.cpu()) == 1, what
        assert (edge[0] == GUARD).all() and (edge[-1] == GUARD).all() and (alp[0] == GUARD).all() and (alp[-1] == GUARD).all(), what
        best = st.best.cpu().numpy()
        assert ((best >= 0) & (best < trie.num_answers)).all(), what
        with pytest.raises(_lib.M3AEHipError):
            st.host()


def test_bad_arguments_return_their_status():
    trie = AnswerTrie(CS.LISTS["prefix"](), (CS.END,))
    dt = trie.score_to_device(DEV, CS.V, MAX_LEN, PAD)
    Ni = dt.Ni
    x = torch.zeros((2 * Ni, CS.V), device=DEV)
    st = ops.ListScoreState(2, 3, MAX_LEN, dt, DEV, PAD)
    ws = ops.listscore_workspace(2 * Ni, CS.V, DEV, 64)
    with pytest.raises(ValueError, match="chunk"):
        ops.listscore_lse(x, 32)
    with pytest.raises(ValueError):
        ops.listscore_lse(x, 64, ws.int())
    with pytest.raises(ValueError):
        ops.listscore_lse(x, 64, ws[:1].contiguous())
    with pytest.raises(TypeError):
        ops.listscore_lse(x.half(), 64)
    with pytest.raises(ValueError):
        ops.listscore_edges(x[:Ni + 1], dt, st, ws, 0, 64)
    with pytest.raises(ValueError):
        ops.listscore_edges(x, dt, st, ws, 1, 64)
    with pytest.raises(ValueError, match="k=17"):
        ops.ListScoreState(2, 17, MAX_LEN, dt, DEV, PAD)
    with pytest.raises(ValueError):
        ops.listscore_workspace(0, CS.V, DEV)
    L = _lib.lib()
    p = lambda a: a.data_ptr()   # noqa: E731
    ARG, UNS, ALIGN, WS = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_ALIGN, _lib.ERR_WORKSPACE
    lse = [p(x), CS.V, 2 * Ni, CS.V, 64, _lib.F32, p(ws), ws.numel() * 8, None]
    for i, v, rc in ((0, None, ARG), (1, CS.V - 1, ARG), (2, 0, ARG), (3, 0, ARG), (4, -1, ARG), (5, 7, UNS), (4, 32, UNS), (4, 65537, UNS),
                     (0, p(x) + 2, ALIGN), (6, None, WS), (6, p(ws) + 4, WS), (7, ws.numel() * 8 - 1, WS)):
        bad = list(lse)
        bad[i] = v
        assert L.m3ae_listscore_lse(*bad) == rc, (i, v)
    assert L.m3ae_listscore_lse(*lse) == 0
    nch = ws.shape[1]
    edges = [p(x), CS.V, 2, Ni, CS.V, _lib.F32, p(ws), ws.numel() * 8, nch, p(dt.internal), p(dt.child_off), p(dt.child_tok), dt.N, dt.E,
             p(st.edge_lp), p(st.err), None]
    for i, v, rc in ((0, None, ARG), (9, None, ARG), (14, None, ARG), (15, None, ARG), (1, CS.V - 1, ARG), (2, 0, ARG), (8, 0, ARG),
                     (5, 7, UNS), (3, dt.N + 1, UNS), (14, p(st.edge_lp) + 2, ALIGN), (6, None, WS), (7, 8, WS)):
        bad = list(edges)
        bad[i] = v
        assert L.m3ae_listscore_edges(*bad) == rc, (i, v)
    assert L.m3ae_listscore_edges(*edges) == 0
    pen = torch.ones(trie.depth + 1, dtype=torch.float64, device=DEV)
    fold = [p(st.edge_lp), p(dt.parent), p(dt.node_depth), p(dt.level_off), p(dt.leaf_node), p(pen), 2, dt.N, dt.A, trie.depth, 3, None, 0,
            p(st.all_logprob), p(st.labels), p(st.scores), p(st.logprob), p(st.probs), p(st.log_mass), p(st.n_hyp), p(st.best), p(st.len),
            p(st.err), None]
    for i, v, rc in ((0, None, ARG), (5, None, ARG), (13, None, ARG), (22, None, ARG), (6, 0, ARG), (7, 1, ARG), (8, 0, ARG), (10, 0, ARG),
                     (10, 17, UNS), (9, 33, UNS), (8, dt.N, UNS), (5, p(pen) + 4, ALIGN), (13, p(st.all_logprob) + 4, ALIGN)):
        bad = list(fold)
        bad[i] = v
        assert L.m3ae_listscore_fold(*bad) == rc, (i, v)
    assert L.m3ae_listscore_fold(*fold) == 0
    torch.cuda.synchronize()


def test_an_entrys_log_probability_has_the_bits_of_the_greedy_list_search():
    """The same logits laid out so that m3ae_trie_scan + m3ae_trie_step walk one answer's path (the row of each node on the path,
    with that answer's token the greatest among the children): their double score equals that entry's all_logprob bit for bit."""
    for dname, chunk in (("fp32", 256), ("bf16", 0)):
        case = ("gen60", 1008, dname, chunk, 1, 5, 0.0, None)
        trie, x = CS.make_case(*case)
        t = trie.score_tables()
        label = int(np.argmax([len(s) for s in trie.sequences]))              # a longest answer
        seq = trie.sequences[label]
        nodes = [trie.walk(seq[:j]) for j in range(len(seq))]
        for n, tok in zip(nodes, seq):                                      # make the path the greedy choice at every node
            toks, _ = trie.children(n)
            x[t["row_of"][n], toks] = np.minimum(x[t["row_of"][n], toks], 1.0)
            x[t["row_of"][n], tok] = 3.0
        xd = on_device(x, DTYPES[dname], 1008)
        _, st, _ = run_kernels(trie, xd, 1, 5, 0.0, chunk)
        tab = trie.to_device(DEV, CS.V, MAX_LEN + 16)
        g = ops.TrieState(1, MAX_LEN + 16, DEV, START, PAD)
        for pos, n in enumerate(nodes):
            row = xd[int(t["row_of"][n]):int(t["row_of"][n]) + 1]
            ws = ops.trie_scan(row, tab, g, chunk)
            ops.trie_step(row, tab, g, ws, pos, PAD, chunk)
        assert int(g.label.cpu()) == label and int(g.err.cpu()) == 0
        assert torch.equal(g.score.view(torch.int64), st.all_logprob[0, label:label + 1].view(torch.int64)), (dname, g.score, st.all_logprob[0, label])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the decoder head
# ---------------------------------------------------------------------------------------------------------------------------------
def decoder_cfg(mode, **over):
    """The tiny decoder set-up of tests/test_gpu_greedy.py."""
    return tiny_config(compute_dtype=mode, image_size=64, hidden_size=768, num_heads=12, num_top_layer=1,
                       input_image_embed_size=128, input_text_embed_size=128, vocab_size=1000, vit_width=128,
                       vit_layers=2, text_hidden=128, text_layers=1, text_heads=2, text_inter=512,
                       mm_encoder_inputs_include_cls_feats=True, mm_encoder_inputs_include_imagetext_feats=False, **over)


def build_model(mode, **over):
    from m3ae_amd.modules import DecoderModel
    m = DecoderModel(decoder_cfg(mode, **over), vocab_size=1200)
    synth.fill_deterministic(m)
    m.finalize("cuda", {"fp32": torch.float32, "bf16": torch.bfloat16, "fp32x3": torch.float32}[mode])
    m.eval()
    m.decoder.max_len = MAX_LEN
    return m


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(mode):
        if mode not in cache:
            cache[mode] = build_model(mode)
        return cache[mode]
    return get


@pytest.fixture(scope="module")
def feats():
    f = torch.from_numpy(load_golden("tiny_decoder.npz")["cls"]).to(DEV)
    return torch.cat([f, 0.5 * f, -f[:1]]).contiguous()


FP32_LOGIT = lambda mx: 1e-5 + 1e-5 * mx     # noqa: E731  tests/test_gpu_model.py: a row computed another way than the full-prefix pass
BF16_LOGIT = lambda mx: 2.0 ** -7 * mx       # noqa: E731  one bf16 ulp of the row's largest logit (no documented tolerance: gap only)


def decoder_rows(d, feats1):
    """prefix (a tuple, without the start token) -> the fp32 next-token logits of the full-prefix Decoder.forward, computed once per
    prefix and shared by the entries through it."""
    rows = {}

    def row_of(prefix):
        if prefix not in rows:
            lg = d(torch.tensor([[START] + list(prefix)], device=DEV), None, feats1)[0].detach().float().cpu().numpy()
            for j in range(len(prefix) + 1):
                rows.setdefault(prefix[:j], np.ascontiguousarray(lg[j], dtype=np.float32))
        return rows[prefix]
    return row_of


def teacher_forced(d, feats1, seqs, itemsize, per_logit, row_of=None):
    """Per list entry, from full-prefix logits (row_of; default: Decoder.forward on feats1): the float64 sum of log p(a[t] | a[<t]),
    the derived bound (tests/trie_score_model.py: the path's term bounds plus the double additions) and the allowance
    2 * per_logit(max |x|) per step."""
    row_of = decoder_rows(d, feats1) if row_of is None else row_of
    lp, derived, allow = [], [], []
    for s in seqs:
        tot = err = al = 0.0
        for j, tok in enumerate(s):
            x = row_of(tuple(s[:j]))
            tot += AM.term64(x, tok)
            err += AM.step_bound(x, tok, 0, itemsize)
            al += 2.0 * per_logit(float(np.abs(x).max()))
        lp.append(tot)
        derived.append(err + len(s) * 2.0 ** -53 * abs(tot))
        allow.append(al)
    return np.asarray(lp), np.asarray(derived), np.asarray(allow)


def check_ranking(labels, beam_labels, lp, tol, order, tag):
    """Rank j is decided where the teacher-forced gaps to both neighbours in the float64 ranking exceed the two entries' allowances:
    there the exhaustive scoring, the float64 ranking and the exhaustive beam search name the same entry.  Returns the number of
    decided ranks."""
    gaps = lp[order[:-1]] - lp[order[1:]]
    clear = gaps > tol[order[:-1]] + tol[order[1:]]
    n = 0
    for j in range(len(order)):
        if (j == 0 or clear[j - 1]) and (j == len(order) - 1 or clear[j]):
            n += 1
            assert labels[j] == order[j] == beam_labels[j], (tag, j, labels, order, beam_labels)
    print(f"{tag}: adjacent gaps clear {int(clear.sum())}/{len(gaps)}, ranks compared {n}/{len(order)}")
    return n


def test_every_entry_of_the_list_has_its_teacher_forced_log_probability(models, feats):
    """fp32, the 60-entry list: all_logprob against the float64 teacher-forced sums within the entry's derived bound plus the fp32
    allowance (rtol = atol = 1e-5 per logit, twice per step)."""
    d = models("fp32").decoder
    seqs = CS.answer_list(1200, SEP)
    t = AnswerTrie(seqs, (SEP,))
    r = d.answer_scores_async(feats, t, 5, 0.0, START, PAD)
    assert int(r.err.cpu()) == 0 and r.groups == 1
    alp = r.all_logprob.cpu().numpy()
    worst = 0.0
    for b in range(feats.shape[0]):
        lp, derived, allow = teacher_forced(d, feats[b:b + 1], seqs, 4, FP32_LOGIT)
        e = np.abs(alp[b] - lp)
        worst = max(worst, float((e / (derived + allow)).max()))
        print(f"decoder fp32 sample {b}: largest |all_logprob - float64| {e.max():.3g}, largest error / tolerance {(e / (derived + allow)).max():.3g}")
        assert (e <= derived + allow).all(), (b, e.max())
        order = np.argsort(-lp, kind="stable")
        assert r.labels[b, 0].item() == order[0] or lp[order[0]] - lp[order[1]] <= (derived + allow)[order[:2]].sum()
    print("decoder fp32: largest error / tolerance over all samples", worst)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_the_label_is_the_teacher_forced_arg_max_of_a_short_list(models, feats, mode):
    d = models(mode).decoder
    seqs = CS.answer_list(1200, SEP, n=8, seed=4, longest=4)
    t = AnswerTrie(seqs, (SEP,))
    r = d.answer_scores_async(feats, t, 8, 0.0, START, PAD)
    beam = d.answer_beam_async(feats, t, 8, 0.0, START, PAD, lookahead=None)
    assert int(r.err.cpu()) == 0
    bf16 = d.head_dtype == torch.bfloat16
    labels, scores, beam_labels = r.labels.cpu().numpy(), r.scores.cpu().numpy(), beam.labels.cpu().numpy()
    decided = compared = 0
    for b in range(feats.shape[0]):
        lp, derived, allow = teacher_forced(d, feats[b:b + 1], seqs, 2 if bf16 else 4, BF16_LOGIT if bf16 else FP32_LOGIT)
        tol = derived + allow
        order = np.argsort(-lp, kind="stable")
        assert sorted(labels[b].tolist()) == list(range(8)) and (np.diff(scores[b]) <= 0).all() and int(r.n_hyp[b]) == 8
        if lp[order[0]] - lp[order[1]] > tol[order[0]] + tol[order[1]]:
            decided += 1
            assert labels[b, 0] == order[0] == int(r.label[b]), (mode, b)
        compared += check_ranking(labels[b], beam_labels[b], lp, tol, order, f"decoder {mode} sample {b}")
        print(f"decoder {mode} sample {b}: largest |score - float64| {np.abs(scores[b] - lp[labels[b]]).max():.3g}")
    assert decided == feats.shape[0], decided
    assert compared > 0                              # the ranking was compared somewhere


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_invariants_on_the_sixty_entry_list(models, feats, mode):
    m = models(mode)
    d = m.decoder
    seqs = CS.answer_list(1200, SEP)
    t = AnswerTrie(seqs, (SEP,))
    A, B = len(seqs), feats.shape[0]
    r = d.answer_scores_async(feats, t, 3, 0.0, START, PAD)
    alp, mass = r.all_logprob.cpu().numpy(), r.log_mass.cpu().numpy()
    assert np.abs(np.exp(alp - mass[:, None]).sum(1) - 1).max() <= A * 2.0 ** -50
    bf16 = d.head_dtype == torch.bfloat16
    for b in range(B):       # disjoint events: their mass cannot exceed 1 by more than the largest entry bound
        _, derived, _ = teacher_forced(d, feats[b:b + 1], seqs, 2 if bf16 else 4, FP32_LOGIT)
        assert mass[b] <= derived.max(), (b, mass[b])
    print(f"decoder {mode}: exp(log_mass) {np.exp(mass)}")
    assert np.allclose(r.probs.cpu().numpy(), np.exp(r.logprob.cpu().numpy() - mass[:, None]), rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="k=17"):
        d.answer_scores_async(feats, t, 17)
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else [x.cuda() for x in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor)
                 else v) for k, v in tiny_batch().items()}
    probs = m.answer_probs(batch, t)
    n = probs.shape[0]
    assert probs.dtype == torch.float32 and tuple(probs.shape) == (n, A) and (probs.sum(1).cpu() - 1).abs().max() <= A * 2.0 ** -23
    l2a = {str(i): f"answer {i}" for i in range(A)}
    named = m.answer(batch, t, l2a, k=3, exhaustive=True)
    rs = m.answer_scores_async(batch, t, 3)
    want = [[(f"answer {l}", s) for l, s in zip(lr, sr)] for lr, sr in zip(rs.labels.cpu().tolist(), rs.scores.cpu().tolist())]
    assert named == want and len(named) == n and all(len(row) == 3 for row in named)
    lab, sc = m.answer(batch, t, exhaustive=True)
    assert torch.equal(lab, rs.label.cpu()) and torch.equal(sc, rs.score.cpu()) and torch.equal(lab, probs.argmax(1).cpu())


def test_groups_give_the_one_group_result(models, feats):
    d = models("fp32").decoder
    seqs = CS.answer_list(1200, SEP)
    t = AnswerTrie(seqs, (SEP,))
    Ni = len(t.score_tables()["internal"])
    one = d.answer_scores_async(feats, t, 5, 1.0, START, PAD)
    two = d.answer_scores_async(feats, t, 5, 1.0, START, PAD, max_rows=2 * Ni)
    tiny = d.answer_scores_async(feats, t, 5, 1.0, START, PAD, max_rows=1)          # a group holds at least one sample
    B = feats.shape[0]                               # five samples: groups of 2 + 2 + 1, then one sample each
    assert (one.groups, two.groups, tiny.groups) == (1, -(-B // 2), B) and B % 2 == 1
    assert torch.equal(one.labels, two.labels) and torch.equal(one.seq, two.seq) and torch.equal(one.labels, tiny.labels)
    a, b = one.all_logprob.cpu().numpy(), two.all_logprob.cpu().numpy()
    print(f"groups 2 + 1 against one group: bits equal {np.array_equal(a, b)}, largest difference {np.abs(a - b).max():.3g}; Ni = {Ni}")
    for s in range(feats.shape[0]):      # the same arithmetic per row on both sides: the derived bound alone, once per computed side
        _, derived, _ = teacher_forced(d, feats[s:s + 1], seqs, 4, FP32_LOGIT)
        assert (np.abs(a[s] - b[s]) <= 2 * derived).all()


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
    print("sync guard:", "set_sync_debug_mode" if live else "call counting")
    return r


def test_answer_scores_async_never_waits_for_the_device(models, feats, monkeypatch):
    d = models("fp32").decoder
    t = AnswerTrie(CS.answer_list(1200, SEP), (SEP,))
    want = d.answer_scores_async(feats, t, 5, 1.0, START, PAD)          # warm: every lazy pack / cast / upload has happened
    r = blocking_guard(monkeypatch, lambda: d.answer_scores_async(feats, t, 5, 1.0, START, PAD))
    assert torch.equal(r.out, want.out) and torch.equal(r.all_logprob, want.all_logprob)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. Trainer.test
# ---------------------------------------------------------------------------------------------------------------------------------
class ListDM:
    train_samples = 8

    def __init__(self, batches):
        self.batches = batches

    def val_batches(self):
        return iter(self.batches)

    def train_batches(self, epoch):
        return iter(self.batches)


def counting_lib(monkeypatch):
    L = _lib.lib()
    counts = {}

    class Counting:
        def __getattr__(self, name):
            if name.startswith(("m3ae_trie", "m3ae_listscore_", "m3ae_tree_attn", "m3ae_vqa_label")) and not name.endswith("_workspace_bytes"):
                counts[name] = counts.get(name, 0) + 1
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Counting())
    return counts


def test_trainer_test_scores_the_list_exhaustively_when_asked(tmp_path, monkeypatch):
    from m3ae_amd.modules import DecoderModel
    SOFT = np.array([0.3, 0.6, 0.9, 1.0, 0.1, 1.0 / 3.0, 2.0 ** -20], dtype=np.float32)
    seen = {}
    for key, over in (("absent", {}), ("search1", dict(answer_scoring="search")), ("absent4", dict(answer_beams=4)),
                      ("search4", dict(answer_scoring="search", answer_beams=4)),
                      ("exhaustive", dict(answer_scoring="exhaustive", answer_beams=4))):
        cfg = decoder_cfg("fp32", vqa_metrics="device", answer_decoding="list", per_gpu_batchsize=2, batch_size=2, max_steps=1,
                          log_dir=str(tmp_path), **over)
        m = DecoderModel(cfg, vocab_size=1200)
        synth.fill_deterministic(m)
        m.finalize(DEV, torch.float32)
        m.eval()
        m.decoder.max_len = 8
        b = {k: (v.cuda() if isinstance(v, torch.Tensor) else [x.cuda() for x in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor)
                 else v) for k, v in tiny_batch().items()}
        b["decoder_tokens"] = torch.tensor([[m.cls_id, 1000, m.sep_id], [m.cls_id, 1001, m.sep_id]], device=DEV)
        b["answer_types"] = [0, 1]
        Cc = cfg["vqa_label_size"]
        seqs = CS.answer_list(1200, m.sep_id, n=min(40, Cc), seed=2)
        b["vqa_targets"] = torch.from_numpy(np.random.default_rng(1).choice(SOFT, size=(2, Cc)).astype(np.float32)).to(DEV)
        tr = trainer.Trainer(cfg, m, ListDM([b, b]), 0, 1, torch.device("cuda", torch.cuda.current_device()))
        tr.answer_trie = AnswerTrie(seqs, (m.sep_id,))
        tr.test()                                    # warm: uploads
        counts = counting_lib(monkeypatch)
        tr.test()
        monkeypatch.undo()
        seen[key] = (dict(counts), tr.answer_text(), tr.answer_metrics)
        if key == "exhaustive":
            k = min(int(cfg.get("eval_topk", 5)), 16, len(seqs))
            assert not any(n.startswith("m3ae_trie") for n in counts), counts
            assert counts["m3ae_tree_attn"] == 2 and counts["m3ae_listscore_lse"] == counts["m3ae_listscore_edges"] == counts["m3ae_listscore_fold"] == 2
            assert counts["m3ae_vqa_labels_eval"] == 2
            text = tr.answer_text()
            assert f" @{k} " in text and " mass " in text and 0.0 < tr.answer_mass <= 1.0 + 1e-6
            m.eval()                                 # the pass leaves the model in train mode
            r = m.answer_scores_async(b, tr.answer_trie, k)
            assert abs(tr.answer_mass - float(torch.exp(r.log_mass).mean().cpu())) < 1e-12
            hit = b["vqa_targets"].cpu().numpy()[np.arange(2), r.label.cpu().numpy()]
            assert abs(tr.answer_metrics["score"] - float(hit.mean())) < 1e-6
        else:
            assert not any(n.startswith(("m3ae_listscore_", "m3ae_tree_attn")) for n in counts) and tr.answer_mass is None and "mass" not in tr.answer_text()
    assert seen["absent"] == seen["search1"] and seen["absent4"] == seen["search4"]     # the key at its default changes nothing
    assert seen["absent"][0]["m3ae_trie_scan"] == seen["absent"][0]["m3ae_trie_step"] >= 2 and "m3ae_triebeam_step" not in seen["absent"][0]
    assert seen["search4"][0]["m3ae_triebeam_select"] == seen["search4"][0]["m3ae_triebeam_step"] == seen["search4"][0]["m3ae_trie_scan"] >= 2
    assert "m3ae_trie_step" not in seen["search4"][0]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the T5 head
# ---------------------------------------------------------------------------------------------------------------------------------
def build_t5(mode):
    """tests/test_gpu_answer_trie.py's tiny T5 with generated weights and the golden encoder output."""
    from m3ae_amd.modules.t5 import T5ForConditionalGeneration
    from m3ae_amd.param_store import ParamStore, group_hparams_decoder, param_group_of_decoder
    from oracle_util import gen_t5_weights
    m = T5ForConditionalGeneration(dict(d_model=512, d_kv=64, d_ff=2048, num_layers=2, num_decoder_layers=2, num_heads=8), 1100)
    sd = gen_t5_weights({"t5." + k: v for k, v in m.state_dict().items()})
    m.load_state_dict({k[3:]: v for k, v in sd.items()})
    dtype = DTYPES[mode]
    ParamStore(m, tiny_config(compute_dtype=mode), "cuda", dtype, m.weight_units, group_fn=param_group_of_decoder,
               hparams_fn=group_hparams_decoder)
    m.eval()
    return m, torch.from_numpy(load_golden("tiny_t5_generate.npz")["enc"]).to(DEV).to(dtype)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_t5_list_scores(mode, monkeypatch):
    """The tree pass of the T5 head against the float64 teacher-forced sums of its full-prefix pass: the arg-max wherever the top-two
    gap exceeds the allowances (FP32_LOGIT in fp32: the tree pass is not the bit-exact cached step; BF16_LOGIT in bf16), the ranking
    against the exhaustive beam search at the decided ranks, the invariants, two group sizes, no blocking call.  No T5 score is held
    to a tolerance the project does not have: the largest |score - float64| is printed."""
    m, enc = build_t5(mode)
    EOS, ML = 1, 8
    seqs = CS.answer_list(1100, EOS, n=8, seed=9, longest=4)
    t = AnswerTrie(seqs, (EOS,))
    B, Ls = enc.shape[:2]
    r = m.list_scores_async(enc, t, 8, ML, 0.0, PAD)
    beam = m.constrained_beam_async(enc, t, 8, ML, 0.0, PAD, lookahead=None)
    assert int(r.err.cpu()) == 0 and r.groups == 1 and tuple(r.seq.shape) == (B, ML)
    labels, scores, beam_labels = r.labels.cpu().numpy(), r.scores.cpu().numpy(), beam.labels.cpu().numpy()
    alp, mass = r.all_logprob.cpu().numpy(), r.log_mass.cpu().numpy()
    kv = m.decoder.cross_kv(enc)
    start = m.config.decoder_start_token_id
    decided = compared = 0
    worst = 0.0
    for b in range(B):
        kvb = [k.view(B, Ls, -1)[b].contiguous() for k in kv]
        rows = {}

        def row_of(prefix):
            if prefix not in rows:
                ids = torch.tensor([[start] + list(prefix)], device=DEV)
                rows[prefix] = np.ascontiguousarray(m.next_token_logits(enc[b:b + 1], ids, kvb)[0].cpu().numpy(), dtype=np.float32)
            return rows[prefix]
        lp, derived, allow = teacher_forced(None, None, seqs, 4, FP32_LOGIT if mode == "fp32" else BF16_LOGIT, row_of)
        tol = derived + allow
        order = np.argsort(-lp, kind="stable")
        assert sorted(labels[b].tolist()) == list(range(8)) and (np.diff(scores[b]) <= 0).all() and int(r.n_hyp[b]) == 8
        if lp[order[0]] - lp[order[1]] > tol[order[0]] + tol[order[1]]:
            decided += 1
            assert labels[b, 0] == order[0] == int(r.label[b]), (mode, b)
        compared += check_ranking(labels[b], beam_labels[b], lp, tol, order, f"t5 {mode} sample {b}")
        worst = max(worst, float(np.abs(alp[b] - lp).max()))
        assert r.seq[b, :int(r.len[b])].cpu().tolist() == seqs[labels[b, 0]]
        assert mass[b] <= derived.max()              # disjoint events: their mass cannot exceed 1
    print(f"t5 {mode}: largest |score - float64| {worst:.3g}; exp(log_mass) {np.exp(mass)}")
    assert decided == B and compared > 0, (decided, compared)
    assert np.abs(np.exp(alp - mass[:, None]).sum(1) - 1).max() <= len(seqs) * 2.0 ** -50
    Ni = len(t.score_tables()["internal"])
    two = m.list_scores_async(enc, t, 8, ML, 0.0, PAD, max_rows=Ni)                 # one sample a group
    assert two.groups == B and torch.equal(two.labels, r.labels)
    print(f"t5 {mode}: one sample a group against one group: bits equal {torch.equal(two.all_logprob, r.all_logprob)}")
    q = blocking_guard(monkeypatch, lambda: m.list_scores_async(enc, t, 8, ML, 0.0, PAD))
    assert torch.equal(q.out, r.out)
    with pytest.raises(ValueError, match="k=17"):
        m.list_scores_async(enc, t, 17, ML)
    with pytest.raises(ValueError, match="room for"):
        m.list_scores_async(enc, t, 1, t.depth - 1)
