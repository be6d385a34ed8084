"""GPU: answer-list decoding (csrc/answer_trie.hip, m3ae_vqa_label_eval of csrc/vqa_eval.hip) -- m3ae_trie_scan + m3ae_trie_step
against the numpy model of tests/answer_trie_model.py array by array (exactly: the choice compares integers), the score against
float64 within the derived bound of that file and of tests/token_eval_model.py, two runs bit for bit; the rejections;
Decoder.answer_path_async / T5.constrained_greedy_async against a host loop over the same logits; the label score record against
tests/vqa_eval_model.py; Trainer.test with answer_decoding="list" and "free"."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import answer_trie_model as M  # noqa: E402
import vqa_eval_model as VM  # noqa: E402
from m3ae_amd import _lib, metrics, ops, synth, trainer  # noqa: E402
from m3ae_amd.answer_trie import AnswerTrie  # noqa: E402
from oracle_util import gen_t5_weights, load_golden, tiny_batch, tiny_config  # noqa: E402

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
POS_NAN, NEG_NAN = 0x7fc00000, 0xffc00000   # bit patterns that are bf16 values too
START, PAD = 101, 0


def rounded(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).float().numpy()


def on_device(x, dtype, ld, pad_value, off=0):
    """x float32 [R, V] of values exact in `dtype` -> a [R, V] view, `off` elements into the rows of a [R, ld + off] device buffer,
    with the same bits (NaN signs included); every other element holds `pad_value`."""
    R, V = x.shape
    buf = torch.full((R, ld + off), pad_value, dtype=dtype, device=DEV)
    if dtype == torch.float32:
        body = torch.from_numpy(np.ascontiguousarray(x))
    else:
        hi = (np.ascontiguousarray(x).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
        body = torch.from_numpy(hi.copy()).view(torch.bfloat16)
        assert np.array_equal(body.float().numpy().view(np.uint32), x.view(np.uint32))
    buf[:, off:off + V] = body.to(DEV)
    return buf[:, off:off + V]


# ---------------------------------------------------------------------------------------------------------------------------------
# tries whose nodes have the child counts the kernel's loop is tested at
# ---------------------------------------------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 257, 600)
EDGES = (255, 256, 999, 1000, 8191, 8192)      # both sides of a chunk boundary of every split used here


def wide_trie(V):
    """(AnswerTrie, {count: node}) over tokens [0, V) with END = V - 1: first token i leads to a node with COUNTS[i] children
    (those that fit V), which hold token 0, token V - 2, the end token V - 1 and the chunk-boundary tokens wherever there is room."""
    end = V - 1
    rng = np.random.default_rng(V)
    seqs, first = [], {}
    for i, cnt in enumerate(COUNTS):
        if cnt > V or i >= end:
            continue
        must = [0, V - 2, end] + [e for e in EDGES if e < V - 2]
        toks = list(dict.fromkeys(must))[:cnt]
        rest = [int(t) for t in rng.permutation(V) if int(t) not in set(toks)]
        toks += rest[:cnt - len(toks)]
        first[cnt] = i
        for c in sorted(toks):
            seqs.append([i, end] if c == end else [i, c, end])
    t = AnswerTrie(seqs, (end,))
    nodes = {cnt: t.walk([i]) for cnt, i in first.items()}
    for cnt, n in nodes.items():
        assert len(t.children(n)[0]) == cnt
    return t, nodes


def table_on_device(t, V, max_len):
    if isinstance(t, AnswerTrie):
        return t.to_device(DEV, V, max_len)
    return NS(child_off=torch.from_numpy(t.child_off).to(DEV), child_tok=torch.from_numpy(t.child_tok).to(DEV),
              child_node=torch.from_numpy(t.child_node).to(DEV), leaf_label=torch.from_numpy(t.leaf_label).to(DEV),
              N=len(t.leaf_label), E=len(t.child_tok), depth=t.depth)


STATE_ARRAYS = ("seq", "len", "label", "err", "last_tok", "node", "finished", "open_count")


def device_state(mod):
    """ops.TrieState holding the arrays of a model State."""
    st = ops.TrieState(mod.B, mod.max_len, DEV, START, PAD)
    for name in STATE_ARRAYS + ("score",):
        getattr(st, name).copy_(torch.from_numpy(getattr(mod, name)).to(DEV))
    return st


def assert_state_equal(dev, mod, where, steps=1):
    for name in STATE_ARRAYS:
        got, want = getattr(dev, name).cpu().numpy(), getattr(mod, name)
        assert got.dtype == want.dtype and np.array_equal(got, want), (where, name, got, want)
    got, want = dev.score.cpu().numpy(), mod.score
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (where, got, want)
    err = np.abs(got[fin] - want[fin])
    bound = mod.bound[fin] + steps * 2.0 ** -53 * np.abs(want[fin])
    print(where, "score error", err.max() if err.size else 0.0, "bound", bound.min() if bound.size else 0.0)
    assert (err <= bound).all(), (where, err, bound)


def one_step(tab, dev, xd, pos, chunk):
    ws = ops.trie_scan(xd, tab, dev, chunk)
    ops.trie_step(xd, tab, dev, ws, pos, PAD, chunk)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. m3ae_trie_scan + m3ae_trie_step against the model
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 9, 12), (3, 257, 260), (3, 1100, 1101), (2, 4099, 4100), (2, 30522, 30592)]
CHUNKS = (0, 256, 1000)


@pytest.fixture(scope="module")
def tries():
    cache = {}

    def get(V):
        if V not in cache:
            cache[V] = wide_trie(V)
        return cache[V]
    return get


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R{}-V{}-ld{}".format(*s))
def test_scan_and_step_match_the_model(tries, shape, dname):
    """Rows placed at every wide node and at the root, random logits; after the step every state array equals the model's and the
    score is within the bound; the padding columns would win every comparison; a second run gives the same bits."""
    R, V, ld = shape
    dtype, itemsize = DTYPES[dname], 4 if dname == "fp32" else 2
    t, nodes = tries(V)
    tab = table_on_device(t, V, 4)
    rng = np.random.default_rng(V + R)
    seen = set()
    for chunk in CHUNKS:
        for cnt, node in [(0, 0)] + sorted(nodes.items()):
            x = rounded(rng.standard_normal((R, V)) * 2.0, dtype)
            off = 1 if (chunk == 256 and cnt in (0, 65)) else 0          # a base pointer one element off
            for pad_value in (1e30, float("nan")):
                mod = M.State(R, 4, START, PAD)
                mod.node[:] = node
                dev = device_state(mod)
                xd = on_device(x, dtype, ld, pad_value, off)
                pos = 1 if node else 0
                one_step(tab, dev, xd, pos, chunk)
                M.step(mod, t, x, pos, PAD, chunk, itemsize)
                assert_state_equal(dev, mod, (shape, dname, chunk, cnt, pad_value))
                again = device_state(M.State(R, 4, START, PAD))
                again.node[:] = node
                one_step(tab, again, xd, pos, chunk)
                assert torch.equal(again.out, dev.out) and torch.equal(again.node, dev.node)      # the same bits, the score included
            seen.add(cnt)
    assert seen == {0} | {c for c in COUNTS if c <= V and COUNTS.index(c) < V - 1}
    if V >= 1100:
        assert seen == {0, *COUNTS}


def edge_rows(t, node, V, dtype, rng):
    """(x [n, V] exact in dtype, the expected token of every row or None) at `node`, whose children include 0, V - 2 and V - 1."""
    toks = t.children(node)[0].astype(np.int64)
    outside = np.setdiff1d(np.arange(V), toks)
    base = rounded(rng.standard_normal(V), dtype)
    rows, want = [], []
    r = base.copy(); r[outside[0]] = 50.0; r[toks[-1]] = 9.0; rows.append(r); want.append(toks[-1])       # the row maximum is no child
    r = base.copy(); r[toks[[1, -1]]] = 9.0; rows.append(r); want.append(toks[1])                        # equal at two children
    r = rounded(-np.abs(base) - 1.0, dtype); r[toks[1]] = -0.0; r[toks[-1]] = 0.0; rows.append(r); want.append(toks[1])   # -0 == +0
    r = rounded(-np.abs(base) - 1.0, dtype); r[toks[1]] = 0.0; r[toks[-1]] = -0.0; rows.append(r); want.append(toks[1])
    r = base.copy(); r[toks[-1]] = np.array([NEG_NAN], dtype=np.uint32).view(np.float32)[0]; r[toks[0]] = np.inf; rows.append(r); want.append(toks[-1])
    r = base.copy(); r[outside[-1]] = np.array([POS_NAN], dtype=np.uint32).view(np.float32)[0]; r[toks[1]] = 9.0; rows.append(r); want.append(toks[1])
    r = base.copy(); r[toks] = -np.inf; rows.append(r); want.append(toks[0])                             # every child at -inf
    r = base.copy(); r[outside[0]] = np.inf; r[toks[1]] = 9.0; rows.append(r); want.append(toks[1])       # +inf outside the children
    r = base.copy(); r[toks[0]] = np.inf; rows.append(r); want.append(toks[0])                           # +inf at a child: inf - inf
    rows.append(np.full(V, -np.inf, dtype=np.float32)); want.append(toks[0])                             # a row of -inf alone
    return np.stack(rows), np.array(want)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("V,ld,cnt", [(257, 260, 64), (1100, 1101, 600), (30522, 30592, 257), (30522, 30592, 65)])
def test_edge_rows(tries, V, ld, cnt, dname):
    dtype, itemsize = DTYPES[dname], 4 if dname == "fp32" else 2
    t, nodes = tries(V)
    node = nodes[cnt]
    tab = table_on_device(t, V, 4)
    x, want = edge_rows(t, node, V, dtype, np.random.default_rng(V + cnt))
    R = x.shape[0]
    for chunk in CHUNKS:
        mod = M.State(R, 4, START, PAD)
        mod.node[:] = node
        dev = device_state(mod)
        one_step(tab, dev, on_device(x, dtype, ld, float("nan")), 1, chunk)
        M.step(mod, t, x, 1, PAD, chunk, itemsize)
        assert np.array_equal(mod.last_tok, want)
        assert_state_equal(dev, mod, (V, cnt, dname, chunk))
        s = dev.score.cpu().numpy()
        assert np.isfinite(s[:4]).all() and np.isnan(s[4]) and np.isnan(s[5]) and s[6] == -np.inf and s[7] == -np.inf
        assert np.isnan(s[8]) and np.isnan(s[9])


def test_finished_rows_leaves_and_open_counts():
    """A whole search on a small list, all depth steps: a leaf at pos 0 ([END] alone), one at pos max_len - 1 (depth == max_len),
    finished rows among open ones fed NaN logits -- pad written, node / score / label / last_tok unchanged."""
    V, END = 300, 2
    seqs = [[END], [5, END], [5, 6, 7, END], [5, 6, 8, 9, END], [9, 9, 9, 9, END], [9, END]]
    t = AnswerTrie(seqs, (END,))
    B, max_len = 70, t.depth                                                    # more rows than a wave
    tab = table_on_device(t, V, max_len)
    rng = np.random.default_rng(3)
    mod, dev = M.State(B, max_len, START, PAD), ops.TrieState(B, max_len, DEV, START, PAD)
    assert_state_equal(dev, mod, "initial")
    n = B * max_len
    assert dev.out.numel() == n + 3 * B + 1 and dev.seq.data_ptr() == dev.out.data_ptr() and dev.score.dtype == torch.float64
    for pos in range(max_len):
        x = rng.standard_normal((B, V)).astype(np.float32)
        x[:, END] += 0.3                                                        # rows end at different steps
        x[mod.finished != 0] = np.nan                                           # garbage where nothing may be read
        one_step(tab, dev, on_device(x, torch.float32, V + 3, float("nan")), pos, 64)
        M.step(mod, t, np.where(np.isnan(x), 0, x), pos, PAD, 64, 4)
        assert_state_equal(dev, mod, pos, steps=pos + 1)
    assert mod.finished.all() and mod.open_count[-1] == 0 and mod.open_count[0] > 0
    assert (mod.len == 1).any() and (mod.len == max_len).any() and np.isfinite(mod.score).all()
    for r in range(B):
        assert mod.seq[r, :mod.len[r]].tolist() == seqs[mod.label[r]] and (mod.seq[r, mod.len[r]:] == PAD).all()


def test_a_table_that_leads_nowhere_sets_the_error_word():
    """Node 1 is no leaf and has no child; node 2's child points past the table; a token past V.  None becomes an address."""
    raw = NS(child_off=np.array([0, 3, 3, 4, 5], np.int32), child_tok=np.array([3, 4, 5, 6, 400], np.int32),
             child_node=np.array([1, 2, 3, 9, 0], np.int32), leaf_label=np.array([-1, -1, -1, -1], np.int32), depth=3)
    tab = table_on_device(raw, 300, 4)
    x = np.random.default_rng(0).standard_normal((5, 300)).astype(np.float32)
    for nodes in ([0, 0, 0, 0, 0], [1, 2, 3, 0, 7]):
        mod = M.State(5, 4, START, PAD)
        mod.node[:] = nodes
        dev = device_state(mod)
        one_step(tab, dev, torch.from_numpy(x).to(DEV), 1, 0)
        M.step(mod, raw, x, 1, PAD, 0, 4)
        assert mod.err[0] == (0 if nodes[0] == 0 and nodes[1] == 0 else 1)
        assert_state_equal(dev, mod, nodes)


def test_bad_arguments_return_their_status():
    V, B = 300, 2
    t = AnswerTrie([[5, 2], [6, 2]], (2,))
    tab = table_on_device(t, V, 4)
    st = ops.TrieState(B, 4, DEV, START, PAD)
    x = torch.zeros((B, V), device=DEV)
    ws = ops.trie_workspace(B, V, DEV, 64)
    for pos in (-1, 4):
        with pytest.raises(ValueError, match="pos"):
            ops.trie_step(x, tab, st, ws, pos, PAD, 64)
    with pytest.raises(ValueError, match="chunk"):
        ops.trie_scan(x, tab, st, 32)
    with pytest.raises(ValueError):
        ops.trie_scan(x[:1], tab, st, 64)
    with pytest.raises(ValueError):
        ops.trie_scan(x, tab, st, 64, ws.int())
    with pytest.raises(ValueError):
        ops.trie_scan(x, tab, st, 64, ws[:, :2].contiguous())
    with pytest.raises(TypeError):
        ops.trie_scan(x.half(), tab, st, 64)
    with pytest.raises(ValueError):
        ops.trie_workspace(0, V, DEV)
    L = _lib.lib()
    p = lambda a: a.data_ptr()   # noqa: E731
    ARG, UNS, ALIGN, WS = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED, _lib.ERR_ALIGN, _lib.ERR_WORKSPACE
    scan = [p(x), V, B, V, 64, _lib.F32, p(tab.child_off), p(tab.child_tok), tab.N, tab.E, p(st.node), p(st.finished), p(ws), ws.numel() * 8, None]
    for i, v, rc in ((0, None, ARG), (1, V - 1, ARG), (2, 0, ARG), (3, 0, ARG), (4, -1, ARG), (6, None, ARG), (7, None, ARG), (8, 0, ARG),
                     (9, 0, ARG), (10, None, ARG), (11, None, ARG), (5, 7, UNS), (4, 32, UNS), (4, 65537, UNS), (0, p(x) + 2, ALIGN),
                     (6, p(tab.child_off) + 2, ALIGN), (12, None, WS), (12, p(ws) + 4, WS), (13, ws.numel() * 8 - 1, WS)):
        bad = list(scan)
        bad[i] = v
        assert L.m3ae_trie_scan(*bad) == rc, (i, v)
    assert L.m3ae_trie_scan(*scan) == 0
    nch = ws.shape[1] - 1
    step = [p(x), V, _lib.F32, p(ws), ws.numel() * 8, nch, p(tab.child_off), p(tab.child_tok), p(tab.child_node), p(tab.leaf_label), tab.N, tab.E,
            p(st.seq), p(st.len), p(st.label), p(st.score), p(st.last_tok), p(st.node), p(st.finished), p(st.open_count), p(st.err), B, V, 4, 0,
            PAD, None]
    for i, v, rc in ((0, None, ARG), (1, V - 1, ARG), (5, 0, ARG), (6, None, ARG), (9, None, ARG), (10, 0, ARG), (11, 0, ARG), (12, None, ARG),
                     (15, None, ARG), (20, None, ARG), (21, 0, ARG), (22, 0, ARG), (23, 0, ARG), (24, -1, ARG), (24, 4, ARG), (2, 7, UNS),
                     (0, p(x) + 2, ALIGN), (15, p(st.score) + 4, ALIGN), (12, p(st.seq) + 4, ALIGN), (3, None, WS), (3, p(ws) + 4, WS),
                     (4, ws.numel() * 8 - 1, WS)):
        bad = list(step)
        bad[i] = v
        assert L.m3ae_trie_step(*bad) == rc, (i, v)
    assert L.m3ae_trie_step(*step) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the decoder head
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_LEN, SEP = 16, 102


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


def answer_list(V, end, n=60, seed=11):
    """n distinct answers of 1 .. 6 tokens over a small alphabet (shared prefixes), one of them a prefix of another."""
    rng = np.random.default_rng(seed)
    alphabet = [int(a) for a in rng.permutation(V)[:12] if int(a) != end]
    seen = {(alphabet[0], end), (alphabet[0], alphabet[1], end), (end,)}
    while len(seen) < n:
        seen.add(tuple(int(rng.choice(alphabet)) for _ in range(int(rng.integers(1, 7)))) + (end,))
    return [list(s) for s in sorted(seen)]


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_answer_path_equals_a_host_loop_over_step_logits(models, feats, mode):
    m = models(mode)
    d = m.decoder
    seqs = answer_list(1200, SEP)
    t = AnswerTrie(seqs, (SEP,))
    r = d.answer_path_async(feats, t, START, PAD, lookahead=None)
    assert r.steps == t.depth <= MAX_LEN and int(r.err.cpu()) == 0
    B = feats.shape[0]
    enc_kv = d.dec_layers[d.num_layers - 1].cross_kv(feats.to(d.head_dtype))
    cache = torch.empty((B, MAX_LEN, 2 * 768), dtype=d.head_dtype, device=DEV)
    itemsize = 2 if d.head_dtype == torch.bfloat16 else 4

    def logits_of(last_tok, pos):
        lg = d.step_logits(torch.from_numpy(last_tok).to(DEV).view(B, 1), pos, enc_kv, cache)
        assert lg.dtype == d.head_dtype
        return lg.float().cpu().numpy()

    mod, steps = M.search(logits_of, t, B, MAX_LEN, START, PAD, 0, itemsize, stop_early=False)
    assert steps == t.depth
    assert np.array_equal(r.label.cpu().numpy(), mod.label) and np.array_equal(r.seq.cpu().numpy(), mod.seq)
    assert np.array_equal(r.len.cpu().numpy(), mod.len) and np.array_equal(r.state.open_count.cpu().numpy(), mod.open_count)
    score = r.score.cpu().numpy()
    assert r.score.dtype == torch.float64 and np.isfinite(score).all() and (score < 0).all()
    for b in range(B):                                          # every returned sequence is an entry of the list
        assert r.seq[b, :int(r.len[b])].cpu().tolist() == seqs[int(r.label[b])]
    for la in (None, 0, 2):                                     # at most depth steps, the same result
        q = d.answer_path_async(feats, t, START, PAD, lookahead=la)
        assert q.steps <= t.depth and torch.equal(q.out, r.out), la
    for chunk in (256, 1000):
        q = d.answer_path_async(feats, t, START, PAD, lookahead=None, chunk=chunk)
        assert torch.equal(q.seq, r.seq) and torch.equal(q.label, r.label)
    from m3ae_amd.search import answer_result
    labels, scores = answer_result(r)
    assert labels.tolist() == mod.label.tolist() and np.array_equal(scores.numpy(), score)
    pairs = answer_result(r, {str(i): f"answer {i}" for i in range(len(seqs))})
    assert pairs == [(f"answer {l}", s) for l, s in zip(labels.tolist(), scores.tolist())]
    with pytest.raises(KeyError):
        answer_result(r, {})


def test_a_single_entry_list_gives_the_free_searchs_own_output(models, feats):
    """The [SEP] bias is raised until every row of the free search finishes; the list whose only entry is a sample's free output then
    gives that output, and the score of the entry is the free search's own log-probability path (finite, negative)."""
    m = models("fp32")
    bias = m.decoder.final_linear.bias
    old = bias.data[SEP].clone()
    try:
        for delta in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 64.0):
            bias.data[SEP] = old + delta
            free = m.decoder.search_path_async(feats, lookahead=None)
            if int(free.state.finished.cpu().min()) == 1:
                break
        else:
            raise AssertionError("no [SEP] bias finishes every row")
        lens = free.len.cpu().tolist()
        print(f"[SEP] bias + {delta}: lengths {lens}")
        for b in range(feats.shape[0]):
            entry = free.seq[b, :lens[b]].cpu().tolist()
            assert entry[-1] == SEP and SEP not in entry[:-1]
            r = m.decoder.answer_path_async(feats[b:b + 1], AnswerTrie([entry], (SEP,)), START, PAD)
            assert torch.equal(r.seq, free.seq[b:b + 1]) and r.len.cpu().tolist() == [lens[b]] and r.label.cpu().tolist() == [0]
            assert r.steps <= lens[b] and int(r.err.cpu()) == 0
    finally:
        bias.data[SEP] = old


def blocking_guard(monkeypatch, run):
    """Runs `run` under torch.cuda.set_sync_debug_mode("error") where `.item()` under it raises on this torch / ROCm pair (checked
    first); otherwise counts calls of Tensor.cpu / item / tolist / __bool__ and torch.cuda.synchronize through monkeypatch."""
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


def test_answer_path_async_never_waits_for_the_device(models, feats, monkeypatch):
    m = models("fp32")
    t = AnswerTrie(answer_list(1200, SEP), (SEP,))
    want = m.decoder.answer_path_async(feats, t, START, PAD, lookahead=None)      # warm: every lazy pack / cast / upload has happened
    r = blocking_guard(monkeypatch, lambda: m.decoder.answer_path_async(feats, t, START, PAD, lookahead=None))
    assert r.steps == t.depth and torch.equal(r.out, want.out)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the T5 head
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
def test_constrained_greedy_equals_a_host_loop_over_cached_logits(mode, monkeypatch):
    m, enc = build_t5(mode)
    EOS, ML = 1, 8
    seqs = answer_list(1100, EOS, n=40, seed=5)
    t = AnswerTrie(seqs, (EOS,))
    r = m.constrained_greedy_async(enc, t, max_length=ML, pad_token_id=PAD, lookahead=None)
    B = enc.shape[0]
    assert r.steps == t.depth <= ML and int(r.err.cpu()) == 0 and tuple(r.seq.shape) == (B, ML)
    cross_kv = [kv.view(B, enc.shape[1], -1).reshape(B * enc.shape[1], -1) for kv in m.decoder.cross_kv(enc)]
    self_cache = m.decoder.new_self_cache(B, ML, enc.dtype, DEV)

    def logits_of(last_tok, pos):
        return m.next_token_logits_cached(enc, torch.from_numpy(last_tok).to(DEV).view(B, 1), cross_kv, self_cache, pos).cpu().numpy()

    mod, steps = M.search(logits_of, t, B, ML, m.config.decoder_start_token_id, PAD, 0, 4, stop_early=False)
    assert np.array_equal(r.label.cpu().numpy(), mod.label) and np.array_equal(r.seq.cpu().numpy(), mod.seq)
    assert np.array_equal(r.len.cpu().numpy(), mod.len)
    for b in range(B):
        assert r.seq[b, :int(r.len[b])].cpu().tolist() == seqs[int(r.label[b])]
    for la in (None, 0, 2):
        q = m.constrained_greedy_async(enc, t, max_length=ML, pad_token_id=PAD, lookahead=la)
        assert q.steps <= t.depth and torch.equal(q.out, r.out), la
    q = blocking_guard(monkeypatch, lambda: m.constrained_greedy_async(enc, t, max_length=ML, pad_token_id=PAD, lookahead=None))
    assert torch.equal(q.out, r.out)
    with pytest.raises(ValueError, match="room for"):
        m.constrained_greedy_async(enc, t, max_length=t.depth - 1)


def small_list(end, depth):
    """(answers, end ids): three answers of depth 3, or two of depth 1 (a second end id makes a second one-token answer possible)."""
    return ([[7, 8, end], [7, 9, end], [11, end]], (end,)) if depth == 3 else ([[end], [7]], (end, 7))


def recorded(monkeypatch, run):
    """`run()` under a recording proxy of the library -> (its result, the entry points of the search families it called, in order,
    the workspace-size query aside)."""
    L = _lib.lib()
    names = []

    class Recording:
        def __getattr__(self, name):
            names.append(name)
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Recording())
    r = run()
    monkeypatch.undo()
    return r, [n for n in names if n.startswith(("m3ae_greedy_", "m3ae_beam_", "m3ae_trie_", "m3ae_triebeam_")) and not n.endswith("_workspace_bytes")]


@pytest.mark.parametrize("depth", [3, 1])
def test_list_searches_enqueue_scan_and_step_per_position(models, feats, monkeypatch, depth):
    """Decoder.answer_path_async and T5.constrained_greedy_async, B = 2, no early exit: scan, step per position of the trie and
    nothing else of the search families (depth 1: a single step); label / seq / len against the numpy model on the same cached logits."""
    d = models("fp32").decoder
    t5, enc = build_t5("fp32")
    f2, enc, ML = feats[:2].contiguous(), enc[:2].contiguous(), 4
    enc_kv = d.dec_layers[d.num_layers - 1].cross_kv(f2.to(d.head_dtype))
    cache = torch.empty((2, MAX_LEN, 2 * 768), dtype=d.head_dtype, device=DEV)
    cross_kv, self_cache = t5.decoder.cross_kv(enc), t5.decoder.new_self_cache(2, ML, enc.dtype, DEV)
    ids = lambda last_tok: torch.from_numpy(last_tok).to(DEV).view(2, 1)    # noqa: E731
    for end, max_len, start, run, logits_of in (
            (SEP, MAX_LEN, START, lambda t: d.answer_path_async(f2, t, START, PAD, lookahead=None),
             lambda last_tok, pos: d.step_logits(ids(last_tok), pos, enc_kv, cache).float().cpu().numpy()),
            (1, ML, t5.config.decoder_start_token_id, lambda t: t5.constrained_greedy_async(enc, t, max_length=ML, pad_token_id=PAD, lookahead=None),
             lambda last_tok, pos: t5.next_token_logits_cached(enc, ids(last_tok), cross_kv, self_cache, pos).cpu().numpy())):
        seqs, ends = small_list(end, depth)
        t = AnswerTrie(seqs, ends)
        run(t)                                                  # warm: the trie is uploaded
        r, names = recorded(monkeypatch, lambda: run(t))
        assert names == ["m3ae_trie_scan", "m3ae_trie_step"] * depth and r.steps == depth == t.depth and int(r.err.cpu()) == 0
        mod, _ = M.search(logits_of, t, 2, max_len, start, PAD, 0, 4, stop_early=False)
        assert np.array_equal(r.label.cpu().numpy(), mod.label) and np.array_equal(r.seq.cpu().numpy(), mod.seq)
        assert np.array_equal(r.len.cpu().numpy(), mod.len)
        for b in range(2):
            assert r.seq[b, :int(r.len[b])].cpu().tolist() == seqs[int(r.label[b])]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. m3ae_vqa_label_eval
# ---------------------------------------------------------------------------------------------------------------------------------
SOFT = np.array([0.0, 0.0, 0.0, 0.3, 0.6, 0.9, 1.0, 0.1, 1.0 / 3.0, 2.0 ** -20], dtype=np.float32)   # {0} u [2^-20, 1]: exact sums


@pytest.mark.parametrize("B", [1, 5, 257])
def test_label_eval_matches_the_fold_bit_for_bit(B):
    Cc = 498
    rng = np.random.default_rng(B)
    tg = rng.choice(SOFT, size=(B, Cc)).astype(np.float32)
    labels = rng.integers(0, Cc, size=B).astype(np.int64)
    labels[0] = Cc - 1
    for ldt in (Cc, Cc + 14):
        buf = torch.full((B, ldt), float("nan"), device=DEV)
        buf[:, :Cc] = torch.from_numpy(tg).to(DEV)
        td = buf[:, :Cc]
        for types in (None, rng.integers(0, 2, size=B).astype(np.int32), np.full(B, 7, dtype=np.int32)):
            hit = tg[np.arange(B), labels]
            one = VM.record(hit, hit, types)
            rec = ops.vqa_record(DEV)
            ty = None if types is None else torch.from_numpy(types).to(DEV)
            rows = ops.vqa_label_eval(torch.from_numpy(labels).to(DEV), td, ty, rec, want_rows=True)
            ops.vqa_label_eval(torch.from_numpy(labels).to(DEV), td, ty, rec)
            assert np.array_equal(rows.hit1.cpu().numpy(), hit) and int(rows.err.cpu()) == 0
            assert np.array_equal(rec.cpu().numpy(), 2 * one)
    # a label out of range scores 0 and sets the error word
    bad = labels.copy()
    bad[B // 2] = Cc
    bad[0] = -1 if B > 1 else Cc
    hit = np.where((bad >= 0) & (bad < Cc), tg[np.arange(B), np.clip(bad, 0, Cc - 1)], np.float32(0))
    rec = ops.vqa_record(DEV)
    rows = ops.vqa_label_eval(torch.from_numpy(bad).to(DEV), td, None, rec, want_rows=True)
    assert int(rows.err.cpu()) == 1 and np.array_equal(rows.hit1.cpu().numpy(), hit)
    assert np.array_equal(rec.cpu().numpy(), VM.record(hit, hit, None))
    met = metrics.VQARADScore(DEV, k=5)
    met.update_labels(torch.from_numpy(labels).to(DEV), td, [0] * B)
    want = VM.result(VM.record(tg[np.arange(B), labels], tg[np.arange(B), labels], [0] * B))
    assert met.result() == want and int(met.label_err.cpu()) == 0 and want["n_closed"] == B


def test_label_eval_rejects_bad_arguments():
    lab, tg, rec = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros((4, 9), device=DEV), ops.vqa_record(DEV)
    for args in ((lab.int(), tg, None, rec), (lab, tg.double(), None, rec), (lab, tg[:3], None, rec), (lab, tg, None, None),
                 (lab, tg.t().contiguous().t(), None, rec), (lab, tg, torch.zeros(4, device=DEV), rec)):
        with pytest.raises(ValueError):
            ops.vqa_label_eval(*args)
    L = _lib.lib()
    p = lambda a: a.data_ptr()   # noqa: E731
    err, ws = torch.zeros(1, dtype=torch.int64, device=DEV), torch.empty((4, 2), device=DEV)
    base = [p(lab), p(tg), 9, None, 4, 9, None, p(rec), p(err), p(ws), 32, None]
    for i, v, rc in ((0, None, -1), (1, None, -1), (7, None, -1), (8, None, -1), (4, 0, -1), (5, 0, -1), (2, 8, -2), (9, None, -2), (10, 31, -2),
                     (0, p(lab) + 4, -3), (1, p(tg) + 2, -3), (7, p(rec) + 4, -3)):
        bad = list(base)
        bad[i] = v
        assert L.m3ae_vqa_label_eval(*bad) == rc, (i, v)
    assert L.m3ae_vqa_label_eval(*base) == 0
    torch.cuda.synchronize()


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
            if name.startswith("m3ae_trie_") or name == "m3ae_vqa_label_eval":
                counts[name] = counts.get(name, 0) + 1
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Counting())
    return counts


def test_trainer_test_reports_closed_and_open_for_the_decoder_head(tmp_path, monkeypatch):
    from m3ae_amd.modules import DecoderModel
    out = {}
    for mode in ("free", "list"):
        cfg = decoder_cfg("fp32", vqa_metrics="device", answer_decoding=mode, per_gpu_batchsize=2, batch_size=2, max_steps=1,
                          log_dir=str(tmp_path))
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
        assert tr.answer_decoding == mode and tr.answer_trie is None
        if mode == "list":
            with pytest.raises(ValueError, match="answer_trie"):
                tr.test()
            tr.answer_trie = AnswerTrie(seqs, (m.sep_id,))
        counts = counting_lib(monkeypatch)
        out[mode] = tr.test()
        monkeypatch.undo()
        if mode == "free":
            assert counts == {} and tr.answer_metrics is None and tr.answer_text() == ""
            continue
        assert counts["m3ae_vqa_label_eval"] == 2 and counts["m3ae_trie_scan"] == counts["m3ae_trie_step"] >= 2
        labels, scores = m.answer(b, tr.answer_trie)
        hit = b["vqa_targets"].cpu().numpy()[np.arange(2), labels.numpy()]
        want = VM.result(2 * VM.record(hit, hit, [0, 1]))
        assert tr.answer_metrics == want and want["n_closed"] == want["n_open"] == 2 and want["closed"] > 0 and want["open"] > 0
        assert f"closed {want['closed']:.4f} (2) open {want['open']:.4f} (2)" in tr.answer_text()
        assert tr.exact_match is not None                          # next to the token exact match it reports today
        pairs = m.answer(b, tr.answer_trie, {str(i): f"a{i}" for i in range(len(seqs))})
        assert [a for a, _ in pairs] == [f"a{l}" for l in labels.tolist()]
    assert abs(out["free"] - out["list"]) <= 1e-5 * abs(out["free"])   # the monitored quantity stays the negative loss
