"""GPU: device-resident greedy search (csrc/greedy.hip) -- m3ae_greedy_argmax against the numpy model's argmax rule (exactly: the
kernel compares integers), m3ae_greedy_step against the model array by array, and Decoder.search_path(search="device") /
search_path_async / DecoderModel against the host form and the reference fixture.  No tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import greedy_model as M  # noqa: E402
from m3ae_amd import _lib, ops, synth  # noqa: E402
from oracle_util import load_golden, tiny_config  # noqa: E402

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
POS_NAN, NEG_NAN, NEG_NAN_PAYLOAD = 0x7fc00000, 0xffc00000, 0xffc10000   # bit patterns that are bf16 values too


def bits(v):
    return np.array(v, dtype=np.uint32).view(np.float32)


def rounded(x, dtype):
    """float32 array -> the float32 array of the values `dtype` holds (bf16: round to nearest even; NaN bits are patched in later)."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype).float().numpy()


def on_device(x, dtype, ld, pad_value, off=0):
    """x float32 [R, V] of values exact in `dtype` -> a [R, V] view, `off` elements into the rows of a [R, ld + off] device buffer,
    with the same bits (NaN signs and payloads included); every other element holds `pad_value`."""
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


def tokens(xd, chunk=0):
    return ops.greedy_argmax(xd, chunk, out=torch.empty(xd.shape[0], dtype=torch.int64, device=DEV)).cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. m3ae_greedy_argmax
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 9, 9), (3, 9, 12), (5, 257, 260), (2, 1001, 1004), (3, 1100, 1101), (1, 4099, 4100), (2, 30522, 30592)]
CHUNKS = (0, 256, 1000, 4096)


def edge_rows(V, dtype, rng):
    """The tie / zero / infinity / NaN rows of tests/test_greedy_host.py plus the chunk-boundary ones: [n, V] float32, exact in dtype."""
    base = rounded(rng.standard_normal(V) * 2.0, dtype)
    rows = [base.copy(), np.full(V, 0.75, dtype=np.float32), np.full(V, -np.inf, dtype=np.float32)]
    r = base.copy(); r[V - 1] = 50.0; rows.append(r)                          # the maximum in the last element of the last (partial) chunk
    r = base.copy(); r[[V // 3, V - 2]] = 50.0; rows.append(r)                # the maximum twice
    for edge in (256, 1000, 2048, 4096):                                      # ... on either side of a chunk boundary of every split
        if edge < V:
            r = base.copy(); r[[edge - 1, edge]] = 50.0; rows.append(r)
            r = base.copy(); r[[edge, min(V - 1, 2 * edge)]] = 50.0; rows.append(r)
    r = np.full(V, -0.0, dtype=np.float32); r[V // 2] = 0.0; rows.append(r)   # +0 == -0: column 0
    r = rounded(-np.abs(base) - 1.0, dtype); r[3] = -0.0; r[V - 1] = 0.0; rows.append(r)
    r = base.copy(); r[V - 1] = np.inf; r[2] = bits([POS_NAN])[0]; rows.append(r)
    r = base.copy(); r[V // 2] = bits([NEG_NAN])[0]; rows.append(r)
    r = base.copy(); r[[4, V // 2, V - 1]] = bits([NEG_NAN_PAYLOAD, POS_NAN, NEG_NAN]); r[1] = np.inf; rows.append(r)
    r = base.copy(); r[[V - 2, V - 1]] = bits([POS_NAN, NEG_NAN]); rows.append(r)
    return np.stack(rows)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R{}-V{}-ld{}".format(*s))
def test_argmax_equals_the_rule(shape, dname):
    R, V, ld = shape
    dtype = DTYPES[dname]
    rng = np.random.default_rng(V + R)
    x = rounded(rng.standard_normal((R, V)) * 2.0, dtype)
    want = M.argmax_rule(x)
    assert want.tolist() == torch.argmax(torch.from_numpy(x), dim=-1).tolist()
    for pad_value in (1e30, float("nan")):        # padding columns that would win every comparison
        xd = on_device(x, dtype, ld, pad_value)
        keys = ops.greedy_argmax(xd)
        again = ops.greedy_argmax(xd)
        assert keys.data_ptr() != again.data_ptr() and torch.equal(keys, again)                  # two calls: the same bits
        assert np.array_equal(keys.cpu().numpy().view(np.uint64), M.chunk_keys(x))              # every chunk's key, not only the winner
        for chunk in CHUNKS:
            assert np.array_equal(tokens(xd, chunk), want), (chunk, pad_value)
        xd = on_device(x, dtype, ld, pad_value, off=1)                                           # a base pointer one element off
        assert np.array_equal(ops.greedy_argmax(xd).cpu().numpy().view(np.uint64), M.chunk_keys(x))
        for chunk in CHUNKS:
            assert np.array_equal(tokens(xd, chunk), want), (chunk, pad_value, "off=1")


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("V,ld", [(9, 12), (257, 260), (1100, 1101), (4099, 4100), (30522, 30592)])
def test_argmax_edge_inputs(V, ld, dname):
    dtype = DTYPES[dname]
    x = edge_rows(V, dtype, np.random.default_rng(V))
    want = M.argmax_rule(x)
    assert want.tolist() == torch.argmax(torch.from_numpy(x), dim=-1).tolist()
    assert want[1] == 0 and want[2] == 0 and want[3] == V - 1 and want[4] == V // 3
    for pad_value in (1e30, float("nan")):
        xd = on_device(x, dtype, ld, pad_value)
        for chunk in CHUNKS:
            assert np.array_equal(tokens(xd, chunk), want), (chunk, pad_value)
        assert np.array_equal(ops.greedy_argmax(xd).cpu().numpy().view(np.uint64), M.chunk_keys(x))


def test_argmax_bf16_natural_ties_at_full_vocabulary():
    """bf16 random normals at V = 30522: the maximum of a row is shared by two columns often enough that a seed below 50 has such
    a row (asserted); the lowest column wins, in every split."""
    R, V, ld = 8, 30522, 30592
    for seed in range(50):
        x = rounded(np.random.default_rng(seed).standard_normal((R, V)), torch.bfloat16)
        tied = (x == x.max(axis=1, keepdims=True)).sum(axis=1)
        if (tied >= 2).any():
            break
    else:
        raise AssertionError("no seed below 50 gives a row whose maximum occurs twice")
    print(f"seed {seed}: columns at the row maximum {tied.tolist()}")
    want = M.argmax_rule(x)
    assert want.tolist() == [int(np.flatnonzero(x[r] == x[r].max())[0]) for r in range(R)]
    xd = on_device(x, torch.bfloat16, ld, 1e30)
    for chunk in CHUNKS:
        assert np.array_equal(tokens(xd, chunk), want), chunk
    assert tokens(xd).tolist() == torch.argmax(xd, dim=-1).cpu().tolist()


def test_argmax_rejects_bad_arguments():
    x = torch.zeros(3, 300, device=DEV)
    with pytest.raises(TypeError):
        ops.greedy_argmax(x.half())
    with pytest.raises(TypeError):
        ops.greedy_argmax(x.long())
    with pytest.raises(ValueError):
        ops.greedy_argmax(x.t())                                 # column stride != 1
    with pytest.raises(ValueError):
        ops.greedy_argmax(x[0])                                  # not [R, V]
    with pytest.raises(ValueError):
        ops.greedy_argmax(x, out=torch.empty(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.greedy_argmax(x, out=torch.empty(4, dtype=torch.int64, device=DEV))
    for chunk in (32, 1 << 17):
        with pytest.raises(ValueError):
            ops.greedy_workspace(3, 300, DEV, chunk)
        with pytest.raises(_lib.M3AEHipError, match="unsupported"):
            ops.greedy_argmax(x, chunk, ws=torch.empty(3, 64, dtype=torch.int64, device=DEV))
    with pytest.raises(_lib.M3AEHipError, match="invalid argument"):
        ops.greedy_argmax(x, -1, ws=torch.empty(3, 64, dtype=torch.int64, device=DEV))
    with pytest.raises(_lib.M3AEHipError, match="workspace too small"):
        ops.greedy_argmax(x, 64, ws=torch.empty(3, 4, dtype=torch.int64, device=DEV))      # 5 chunks per row
    L = _lib.lib()
    ws = torch.empty(3, 8, dtype=torch.int64, device=DEV)
    args = lambda **k: [k.get("p", x.data_ptr()), k.get("ld", 300), k.get("R", 3), k.get("V", 300), 0, k.get("dt", 0),  # noqa: E731
                        k.get("ws", ws.data_ptr()), k.get("n", ws.numel() * 8), None, None]
    assert L.m3ae_greedy_argmax(*args()) == 0
    assert L.m3ae_greedy_argmax(*args(p=None)) == L.m3ae_greedy_argmax(*args(ld=299)) == L.m3ae_greedy_argmax(*args(R=0)) == -1
    assert L.m3ae_greedy_argmax(*args(V=0)) == -1
    assert L.m3ae_greedy_argmax(*args(dt=2)) == -2
    assert L.m3ae_greedy_argmax(*args(p=x.data_ptr() + 2)) == -3                           # fp32 logits off a 4-byte boundary
    assert L.m3ae_greedy_argmax(*args(ws=None)) == L.m3ae_greedy_argmax(*args(ws=ws.data_ptr() + 4)) == -4
    assert L.m3ae_greedy_argmax(*args(n=23)) == -4
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. m3ae_greedy_step against the numpy model
# ---------------------------------------------------------------------------------------------------------------------------------
STATE_ARRAYS = ("seq", "len", "err", "last_tok", "finished", "open_count")


def assert_state_equal(dev, mod, where):
    for name in STATE_ARRAYS:
        a, b = getattr(dev, name).cpu().numpy(), getattr(mod, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype)
        assert np.array_equal(a, b), (name, where)


def keys_on_device(toks, V):
    return torch.from_numpy(M.keys_for_tokens(toks, V).view(np.int64)).to(DEV)


@pytest.mark.parametrize("eos_id", [None, M.EOS])
@pytest.mark.parametrize("B", [1, 3, 70, 300])
@pytest.mark.parametrize("kind", M.SCRIPT_KINDS)
def test_step_matches_the_model(kind, B, eos_id):
    """After every step every state array equals the model's.  All steps run, so finished rows are stepped too (B = 70: more rows
    than a wave, 300: more than the workgroup)."""
    sc = M.script(kind, B)
    dev = ops.GreedyState(B, M.SCRIPT_LEN, DEV, M.CLS, M.PAD)
    assert_state_equal(dev, M.State(B, M.SCRIPT_LEN, M.CLS, M.PAD), "initial")
    assert dev.out.numel() == B * M.SCRIPT_LEN + B + 1 and dev.seq.data_ptr() == dev.out.data_ptr()

    def on_step(st, pos):
        ops.greedy_step(dev, keys_on_device(sc[pos], M.SCRIPT_V), M.SCRIPT_V, pos, M.SEP, eos_id, M.PAD)
        assert_state_equal(dev, st, (kind, pos))

    M.search(sc, M.SCRIPT_V, M.CLS, M.SEP, eos_id, M.PAD, stop_early=False, on_step=on_step)


def test_step_from_argmax_keys_and_token_out_of_range():
    """The keys of greedy_argmax drive the step; a vocabulary smaller than the columns the keys carry sets the error word and the
    row goes on with token 0 (never an address)."""
    B, V, ml = 4, 300, 4
    x = np.full((B, V), -1.0, dtype=np.float32)
    x[np.arange(B), [5, 299, M.SEP, 150]] = 2.0
    keys = ops.greedy_argmax(torch.from_numpy(x).to(DEV), 64)
    for Vstep in (V, 200):
        dev, mod = ops.GreedyState(B, ml, DEV, M.CLS, M.PAD), M.State(B, ml, M.CLS, M.PAD)
        ops.greedy_step(dev, keys, Vstep, 0, M.SEP, None, M.PAD)
        M.step(mod, [5, 299, M.SEP, 150], 0, Vstep, M.SEP, None, M.PAD)
        assert mod.err[0] == (0 if Vstep == V else 1) and mod.last_tok[1] == (299 if Vstep == V else 0)
        assert_state_equal(dev, mod, Vstep)


def test_step_rejects_bad_arguments():
    st = ops.GreedyState(2, 4, DEV)
    keys = keys_on_device([1, 2], 300)
    for pos in (-1, 4):
        with pytest.raises(ValueError, match="pos"):
            ops.greedy_step(st, keys, 300, pos, M.SEP, None, M.PAD)
    with pytest.raises(ValueError):
        ops.greedy_step(st, keys[:1], 300, 0, M.SEP, None, M.PAD)
    with pytest.raises(ValueError):
        ops.greedy_step(st, keys.int(), 300, 0, M.SEP, None, M.PAD)
    L = _lib.lib()
    p = lambda t: t.data_ptr()   # noqa: E731
    base = [p(keys), 3, p(st.seq), p(st.len), p(st.last_tok), p(st.finished), p(st.open_count), p(st.err), 2, 300, 4, 0, M.SEP, -1, M.PAD, None]
    for i, v in ((0, None), (0, p(keys) + 4), (1, 0), (1, -3), (2, None), (7, None), (8, 0), (9, 0), (10, 0), (11, -1), (11, 4)):
        bad = list(base)
        bad[i] = v
        assert L.m3ae_greedy_step(*bad) == -1, (i, v)
    assert L.m3ae_greedy_step(*base) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the decoder head
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_LEN = 16


def decoder_cfg(mode, **over):
    """The tiny decoder set-up of tests/test_gpu_model.py::test_tiny_decoder_generative_head_against_reference_fixture."""
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
    """The fixture's two feature rows and three variants of them: B = 5."""
    f = torch.from_numpy(load_golden("tiny_decoder.npz")["cls"]).to(DEV)
    return torch.cat([f, 0.5 * f, -f[:1]]).contiguous()


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_search_path_device_equals_host(models, feats, mode):
    m = models(mode)
    g = load_golden("tiny_decoder.npz")
    host = m.decoder.search_path(feats)
    dev = m.decoder.search_path(feats, search="device")
    assert dev.dtype == host.dtype == torch.int64 and dev.device == host.device and tuple(dev.shape) == (5, MAX_LEN)
    assert torch.equal(dev, host)
    if mode == "fp32":
        assert np.array_equal(dev[:2].cpu().numpy(), g["greedy"])
        assert np.array_equal(m.decoder.search_path(feats[:2], search="device").cpu().numpy(), g["greedy"])
    if mode == "bf16":      # the argmax reads the bf16 logits as the padded vocabulary GEMM left them
        layer = m.decoder.dec_layers[m.decoder.num_layers - 1]
        cache = torch.empty((5, MAX_LEN, 2 * 768), dtype=torch.bfloat16, device=DEV)
        lg = m.decoder.step_logits(torch.full((5, 1), 101, device=DEV), 0, layer.cross_kv(feats.to(torch.bfloat16)), cache)
        assert lg.dtype == torch.bfloat16 and lg.stride(0) > lg.shape[1] == 1200


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_lookahead_changes_no_token_and_end_tokens(models, feats, mode):
    """lookahead 1, 2 and None give the same tokens; with an end token the fixture's rows do emit (eos_id = a token of g["greedy"])
    the device form equals the host form, rows ending at different steps."""
    m = models(mode)
    full = m.decoder.search_path_async(feats, lookahead=None)
    assert full.steps == MAX_LEN and int(full.err.cpu()) == 0
    oc, lens, fin = full.state.open_count.cpu().tolist(), full.len.cpu().numpy(), full.state.finished.cpu().numpy()
    assert oc == [int(((fin == 0) | (lens > t + 1)).sum()) for t in range(MAX_LEN)]
    assert torch.equal(full.seq, m.decoder.search_path(feats))
    for la in (1, 2):
        r = m.decoder.search_path_async(feats, lookahead=la)
        assert torch.equal(r.seq, full.seq) and torch.equal(r.len, full.len), la
        assert r.steps == MAX_LEN or min(oc) == 0
    for chunk in (256, 1000):
        assert torch.equal(m.decoder.search_path_async(feats, lookahead=None, chunk=chunk).seq, full.seq)
    seen = sorted(set(full.seq.cpu().view(-1).tolist()))
    for eos in seen[:4]:
        host = m.decoder.search_path(feats, eos_id=eos)
        assert torch.equal(m.decoder.search_path(feats, eos_id=eos, search="device"), host), eos
        assert torch.equal(m.decoder.search_path(feats, sep_id=eos, search="device"), m.decoder.search_path(feats, sep_id=eos)), eos


def test_early_exit_runs_at_most_lookahead_steps_past_the_last_row(models, feats):
    """The [SEP] bias is raised until every row finishes well before max_len (asserted on the full run's open counts); the loop then
    enqueues at most `lookahead` steps past the step that finished the last row, and the tokens are the full run's and the host's."""
    m = models("fp32")
    bias = m.decoder.final_linear.bias
    old = bias.data[M.SEP].clone()
    try:
        for delta in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 64.0):
            bias.data[M.SEP] = old + delta
            full = m.decoder.search_path_async(feats, lookahead=None)
            oc = full.state.open_count.cpu().tolist()
            closed_at = next((t for t in range(MAX_LEN) if oc[t] == 0), None)
            if closed_at is not None and closed_at + 2 < MAX_LEN - 1:
                break
        else:
            raise AssertionError("no [SEP] bias finishes every row early")
        print(f"[SEP] bias + {delta}: open rows after each step {oc}, lengths {full.len.cpu().tolist()}")
        assert full.steps == MAX_LEN and full.len.cpu().max().item() == closed_at + 1
        host = m.decoder.search_path(feats)
        assert torch.equal(full.seq, host)
        for la in (1, 2):
            r = m.decoder.search_path_async(feats, lookahead=la)
            assert closed_at + 1 <= r.steps <= closed_at + la < MAX_LEN, (la, r.steps, closed_at)
            assert torch.equal(r.seq, full.seq) and torch.equal(r.len, full.len)
            assert torch.equal(m.decoder.search_path(feats, search="device", lookahead=la), host)
    finally:
        bias.data[M.SEP] = old


def test_search_path_async_never_waits_for_the_device(models, feats, monkeypatch):
    """Guard in use: torch.cuda.set_sync_debug_mode("error") where `.item()` under it raises on this torch / ROCm pair (checked
    first); otherwise calls of Tensor.cpu / item / tolist / __bool__ and torch.cuda.synchronize are counted through monkeypatch."""
    m = models("fp32")
    want = m.decoder.search_path_async(feats, lookahead=None)      # warm: every lazy pack / cast has happened
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
            r = m.decoder.search_path_async(feats, lookahead=None)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not live:
        calls = []
        for name in ("cpu", "item", "tolist", "__bool__"):
            real = getattr(torch.Tensor, name)
            monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _r=real, _n=name, **k: (calls.append(_n) if self.is_cuda else None, _r(self, *a, **k))[1])
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
        r = m.decoder.search_path_async(feats, lookahead=None)
        monkeypatch.undo()
        assert calls == [], calls
    print("sync guard:", "set_sync_debug_mode" if live else "call counting")
    assert r.steps == MAX_LEN and torch.equal(r.seq, want.seq) and torch.equal(r.len, want.len)


def test_default_search_calls_no_greedy_entry_point(models, feats, monkeypatch):
    m = models("fp32")
    L = _lib.lib()
    counts = {}

    class Counting:
        def __getattr__(self, name):
            if name.startswith("m3ae_greedy_"):
                counts[name] = counts.get(name, 0) + 1
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Counting())
    m.decoder.search_path(feats)
    assert counts == {}, counts
    m.decoder.search_path(feats, search="device")
    assert counts.get("m3ae_greedy_argmax") == counts.get("m3ae_greedy_step") == MAX_LEN, counts


def test_search_path_async_enqueues_argmax_and_step_per_position(models, feats, monkeypatch):
    """One call without early exit under a recording proxy of the library: the ordered search entry points (the workspace-size
    query aside) are argmax, step per position -- nothing else of the search families, nothing after the last step."""
    d = models("fp32").decoder
    L = _lib.lib()
    names = []

    class Recording:
        def __getattr__(self, name):
            names.append(name)
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Recording())
    r = d.search_path_async(feats[:2], lookahead=None)
    monkeypatch.undo()
    search = [n for n in names if n.startswith(("m3ae_greedy_", "m3ae_beam_", "m3ae_trie_", "m3ae_triebeam_")) and not n.endswith("_workspace_bytes")]
    assert search == ["m3ae_greedy_argmax", "m3ae_greedy_step"] * MAX_LEN and names[-1] == "m3ae_greedy_step"
    assert r.steps == MAX_LEN and torch.equal(r.seq, d.search_path(feats[:2]))


def test_decoder_model_passes_the_mode_and_generates(models):
    """DecoderModel with decoder_search=device returns the generated_ids it returns with the default; generate / generate_async."""
    b = {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and v
             and isinstance(v[0], torch.Tensor) else v)
         for k, v in synth.synthetic_batch(2, text_len=32, image_size=64, vocab_size=1000, rank=0).items()}
    host_m = models("fp32")
    dev_m = build_model("fp32", decoder_search="device")
    assert host_m.decoder_search == "host" and dev_m.decoder_search == "device"
    host = host_m(b, test=True)["generated_ids"]
    dev = dev_m(b, test=True)["generated_ids"]
    assert tuple(host.shape) == (2, MAX_LEN) and torch.equal(dev, host)
    assert torch.equal(dev_m.generate(b), host) and torch.equal(host_m.generate(b), host) and torch.equal(host_m.generate(b, search="device"), host)
    r = host_m.generate_async(b)
    assert torch.equal(r.seq, host) and int(r.err.cpu()) == 0 and r.steps == MAX_LEN

    class Tok:
        def batch_decode(self, ids, skip_special_tokens=True):
            return [" ".join(str(t) for t in row if t != 0) for row in ids]
    dev_m.tokenizer = Tok()
    try:
        ids, text = dev_m.generate(b)
    finally:
        dev_m.tokenizer = None
    assert torch.equal(ids, host) and text == [" ".join(str(t) for t in row if t != 0) for row in host.cpu().tolist()]
