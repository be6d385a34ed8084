"""GPU: attention summaries -- the received attention recv[b, k] = mean over heads and queries of an attention map, formed
without the map (m3ae_attn_colmean, m3ae_xattn_probs_colmean) -- the heatmap upsample (m3ae_heatmap_upsample), and what the
modules build on them: infer(output_attention_summary=True), attention_heatmaps and the heads' heatmap entry points.

Bounds are derived, not observed.  A summary is held to the float64 mean of the fp32 map the library returns for the same inputs
(ops.attn_probs / ops.xattn_probs): the summed entries are those entries bit for bit (same expression in the bf16 kernel, the same
kernels in parity mode, exact widening of the stored bf16 P), so what is left is the summation: H Lq - 1 fp32 additions of
non-negative terms in some order, the rounded reciprocal of H Lq and one product: (H Lq + 2) 2^-24 relative
(heatmap_model.recv_bound).

The upsample is held to tests/heatmap_model.py, which forms the kernel's weights in np.float32 and combines in float64.  With
m = max|in|, u = 2^-24 and weights l0 + l1 <= 1 + u: a row interpolation fl(fl(l0 a) + fl(l1 b)) is within u (|l0 a| + |l1 b|) + u m of
exact, 2 u m; the column interpolation carries the two row errors with weights l0y + l1y, 2 u m, and adds 2 u m of its own: 4 u m, up
to terms in u^2.  The tests allow 5 u m (the issue's first estimate was 8)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import heatmap_model as hm  # noqa: E402
from m3ae_amd import _lib, ops, synth  # noqa: E402
from m3ae_amd.config import finetune_vqa_rad_config, tiny_config  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from oracle_util import full_batch, load_golden, tiny_batch  # noqa: E402
from test_gpu_attn_maps import build, cross_inputs, make_cross, to_dev  # noqa: E402

U = hm.U
P_DROP = 0.1
NEW_ENTRIES = ("m3ae_attn_colmean_workspace_bytes", "m3ae_attn_colmean", "m3ae_xattn_probs_colmean", "m3ae_heatmap_upsample")


def assert_recv(got, p, what=""):
    """got [B, Lk] against the float64 mean of the map p [B, H, Lq, Lk] (both on the device), within the summation bound."""
    B, H, Lq, Lk = p.shape
    assert got.shape == (B, Lk) and got.dtype == torch.float32 and got.is_contiguous() and not got.requires_grad, what
    ref = p.double().mean(dim=(1, 2))
    err = (got.double() - ref).abs()
    bound = (H * Lq + 2) * U * ref
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what} [{B}, {H}, {Lq}, {Lk}]: max err / bound = {worst:.3f}")
    assert (err <= bound).all(), (what, worst)
    dead = (p == 0).all(dim=1).all(dim=1)
    assert (got[dead] == 0).all(), what


# ------------------------------------------------------------------------------------------------------------------------
# 1. ops.attn_colmean against the map of ops.attn_probs
# ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (17, 17), (33, 31), (129, 577), (577, 32), (577, 577)]


def qk_inputs(B, Lq, Lk, H, dtype, pad=0):
    g = torch.Generator(device="cuda").manual_seed(1000 * Lq + Lk + B)
    q = torch.randn(B, Lq, 64 * H, device="cuda", generator=g).to(dtype)
    k = torch.randn(B, Lk, 64 * H, device="cuda", generator=g).to(dtype)
    v = torch.randn(B, Lk, 64 * H, device="cuda", generator=g).to(dtype)
    mask = None
    if pad:
        mask = torch.zeros(B, Lk, device="cuda")
        mask[:, Lk - pad:] = -10000.0
    return q, k, v, mask


@pytest.mark.parametrize("Lq,Lk,B,pad", [(*s, 2, 0) for s in SHAPES] + [(577, 577, 1, 5)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_attn_colmean_is_the_mean_of_the_map(dtype, Lq, Lk, B, pad):
    H = 3
    q, k, v, mask = qk_inputs(B, Lq, Lk, H, dtype, pad)
    for drop in (None, (P_DROP, 0x5EED0 + Lq)):
        with torch.no_grad():
            _, lse = ops.attn_forward(q, k, v, H, mask, dropout=drop)
            p = ops.attn_probs(q, k, lse, H, mask, dropout=drop)
            got = [ops.attn_colmean(q, k, lse, H, mask, dropout=drop) for _ in range(10)]
        torch.cuda.synchronize()
        assert_recv(got[0], p, f"drop={drop is not None}")
        if pad:
            assert (got[0][:, Lk - pad:] == 0).all() and (got[0][:, :Lk - pad] > 0).all()
        for g in got[1:]:
            assert torch.equal(g, got[0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_attn_colmean_refusals_leave_out_untouched(dtype):
    B, H, Lq, Lk = 2, 3, 33, 31
    q, k, v, _ = qk_inputs(B, Lq, Lk, H, dtype)
    with torch.no_grad():
        _, lse = ops.attn_forward(q, k, v, H)
    L = _lib.lib()
    out = torch.full((B, Lk), -7.0, device="cuda")
    bias = torch.zeros(H, Lq, Lk, device="cuda")

    def call(pos_bias=None, causal=False, short=0):
        d = ops._attn_desc(B, H, Lq, Lk, 64, q, k, k, q, None, pos_bias, 0.125, causal, lse, lse.shape[-1], ops._dt(q))
        n = L.m3ae_attn_colmean_workspace_bytes(C.byref(d))
        assert n > 0
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        return L.m3ae_attn_colmean(C.byref(d), C.c_void_p(out.data_ptr()), out.stride(0), C.c_void_p(ws.data_ptr()), n - short,
                                   ops._stream())

    assert call(short=1) == -4         # M3AE_ERR_WORKSPACE
    assert call(pos_bias=bias) == -2   # M3AE_ERR_UNSUPPORTED
    assert call(causal=True) == -2
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (out > 0).all()


def test_attn_colmean_workspace_is_the_documented_size():
    q = torch.empty(1, 1, 64, device="cuda", dtype=torch.bfloat16)
    L = _lib.lib()
    for B, H, Lq, Lk in ((256, 12, 577, 577), (2, 3, 129, 577), (1, 1, 1, 1)):
        d = ops._attn_desc(B, H, Lq, Lk, 64, q, q, q, q, None, None, 0.125, False, None, 0, _lib.BF16)
        assert L.m3ae_attn_colmean_workspace_bytes(C.byref(d)) == B * H * -(-Lq // 128) * Lk * 4
        d.dtype = _lib.F32   # a function of the chunk (4 samples), not of B
        assert L.m3ae_attn_colmean_workspace_bytes(C.byref(d)) == min(B, 4) * H * (Lq + 1) * Lk * 4


# ------------------------------------------------------------------------------------------------------------------------
# 2. ops.xattn_colmean against ops.xattn_probs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("need_bwd", [False, True], ids=["forward_only", "training"])
@pytest.mark.parametrize("pdrop", [0.0, P_DROP], ids=["eval", "dropout"])
@pytest.mark.parametrize("L,Lo", [(32, 577), (577, 32), (1025, 32)])
def test_xattn_colmean_is_the_mean_of_the_exported_map(L, Lo, pdrop, need_bwd):
    B = 3
    att, _ = make_cross(seed=L + Lo)
    x, y, mask = cross_inputs(B, L, Lo, L * Lo + 1)
    P = att.block_params()
    h2, o2 = x.reshape(B * L, 768), y.reshape(B * Lo, 768)
    old, ops.XATTN = ops.XATTN, "always"
    try:
        assert ops.xattn_supported(h2, L, o2, Lo, mask, P)
        with torch.no_grad():
            _, saved = ops.xattn_fwd(h2, B, L, o2, Lo, mask, P, pdrop, need_bwd=need_bwd, want_probs=True)
            p = ops.xattn_probs(saved)
            got = [ops.xattn_colmean(saved) for _ in range(3)]
    finally:
        ops.XATTN = old
    torch.cuda.synchronize()
    assert_recv(got[0], p, f"xattn pdrop={pdrop} need_bwd={need_bwd}")
    assert torch.equal(got[1], got[0]) and torch.equal(got[2], got[0])
    if mask is not None:
        pad = mask < -1
        assert (got[0][pad] == 0).all()


def test_xattn_colmean_needs_the_stored_probabilities():
    B, L, Lo = 2, 577, 32
    att, _ = make_cross(seed=5)
    x, y, mask = cross_inputs(B, L, Lo, 9)
    old, ops.XATTN = ops.XATTN, "always"
    try:
        with torch.no_grad():
            _, saved = ops.xattn_fwd(x.reshape(B * L, 768), B, L, y.reshape(B * Lo, 768), Lo, mask, att.block_params(), 0.0,
                                     need_bwd=False)
    finally:
        ops.XATTN = old
    with pytest.raises(_lib.M3AEHipError, match="on chip"):
        ops.xattn_colmean(saved)


# ------------------------------------------------------------------------------------------------------------------------
# 3. ops.heatmap_upsample against the model
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g,S", [(1, 8), (2, 7), (4, 64), (24, 384), (24, 100), (24, 385)])
def test_heatmap_upsample_against_the_model(g, S):
    B = 3
    gen = torch.Generator(device="cuda").manual_seed(g * 1000 + S)
    row = torch.rand(B, 1 + g * g, device="cuda", generator=gen)
    row[:, 0] = 1e6   # the class token: must not leak into any output
    out = ops.heatmap_upsample(row[:, 1:], S)
    torch.cuda.synchronize()
    assert out.shape == (B, S, S) and out.dtype == torch.float32 and out.is_contiguous()
    x = row[:, 1:].cpu().numpy()
    m = np.abs(x).max()
    want = hm.upsample(x.reshape(B, g, g), S)
    err = np.abs(out.cpu().numpy().astype(np.float64) - want).max()
    print(f"{g} -> {S}: err / (u max|in|) = {err / (U * m):.3f}")
    assert err <= 5 * U * m, err / (U * m)
    assert out.max().item() <= float(m) * (1 + 5 * U) and out.min().item() >= 0   # convex weights: nothing of token 0's 1e6
    assert torch.equal(out, ops.heatmap_upsample(row[:, 1:].reshape(B, g, g).contiguous(), S))
    if S % g == 0:   # ATen forms the same weights on integer ratios (tests/test_attn_summary_host.py)
        aten = torch.nn.functional.interpolate(torch.from_numpy(x.reshape(B, 1, g, g)), size=(S, S), mode="bilinear",
                                               align_corners=False)[:, 0]
        assert (out.cpu() - aten).abs().max().item() <= 16 * U * m


def test_heatmap_upsample_refusals():
    L = _lib.lib()
    x = torch.rand(2, 16, device="cuda")
    out = torch.full((2, 8, 8), -7.0, device="cuda")
    f = lambda in_sb, g, B, S: L.m3ae_heatmap_upsample(C.c_void_p(x.data_ptr()), in_sb, g, C.c_void_p(out.data_ptr()), B, S,
                                                      ops._stream())
    assert f(16, 0, 2, 8) == -1 and f(16, 4, 2, 0) == -1 and f(16, 4, 0, 8) == -1 and f(15, 4, 2, 8) == -1
    assert L.m3ae_heatmap_upsample(None, 16, 4, C.c_void_p(out.data_ptr()), 2, 8, ops._stream()) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    with pytest.raises(ValueError):
        ops.heatmap_upsample(torch.rand(2, 15, device="cuda"), 8)


# ------------------------------------------------------------------------------------------------------------------------
# 4. - 8. the model
# ------------------------------------------------------------------------------------------------------------------------
SIDES = (("t2i", "text2image"), ("i2t", "image2text"))
KINDS = ("self", "cross")
FEATS = ("multi_modal_cls_feats", "multi_modal_text_feats", "multi_modal_image_feats")


def check_summary_structure(summ, n_layers, B, T, I):
    assert set(summ) == {"text2image", "image2text"}
    keys = {"text2image": (T, I), "image2text": (I, T)}
    for side, (ks, kc) in keys.items():
        assert isinstance(summ[side], list) and len(summ[side]) == n_layers
        for entry in summ[side]:
            assert isinstance(entry, tuple) and len(entry) == 2
            for r, Lk in zip(entry, (ks, kc)):
                assert r.dtype == torch.float32 and tuple(r.shape) == (B, Lk) and r.is_contiguous() and not r.requires_grad


@pytest.mark.parametrize("two_streams", [True, False])
def test_tiny_fp32_summaries_equal_the_mean_of_the_reference_maps(two_streams):
    m = build(tiny_config(compute_dtype="fp32"), torch.float32)
    m.two_streams = two_streams
    g = load_golden("attn_maps.npz")
    with torch.no_grad():
        ret = m.infer(to_dev(tiny_batch()), output_attention_summary=True)
    torch.cuda.synchronize()
    assert ret["attentions"] is None
    summ = ret["attention_summary"]
    check_summary_structure(summ, 2, 2, 32, 17)
    for tag, side in SIDES:
        for l, entry in enumerate(summ[side]):
            for kind, r in zip(KINDS, entry):
                # the maps are held to rtol 1e-4, atol 1e-6 (tests/test_gpu_attn_maps.py): a mean of entries inside is inside
                np.testing.assert_allclose(r.cpu().numpy(), hm.recv(g[f"tiny_{tag}_{l}_{kind}"]), rtol=1e-4, atol=1e-6,
                                           err_msg=f"{tag} layer {l} {kind}")


def test_fp32x3_and_deterministic_summaries_are_the_mean_of_their_maps():
    b = to_dev(tiny_batch())
    m = build(tiny_config(compute_dtype="fp32x3"), torch.float32)
    with torch.no_grad():
        ret = m.infer(b, output_attentions=True, output_attention_summary=True)
    torch.cuda.synchronize()
    compare_with_own_maps(ret, "fp32x3")
    m = build(tiny_config(compute_dtype="bf16"), torch.bfloat16)
    with torch.no_grad():
        plain = m.infer(b, output_attention_summary=True)
        with ops.deterministic_mode():
            det = m.infer(b, output_attentions=True, output_attention_summary=True)
    torch.cuda.synchronize()
    compare_with_own_maps(det, "deterministic")
    for side in ("text2image", "image2text"):   # the summary kernels have one form: the mode changes nothing
        for e0, e1 in zip(plain["attention_summary"][side], det["attention_summary"][side]):
            assert torch.equal(e0[0], e1[0]) and torch.equal(e0[1], e1[1])


def compare_with_own_maps(ret, what):
    for _, side in SIDES:
        for l, (maps, recvs) in enumerate(zip(ret["attentions"][f"{side}_attns"], ret["attention_summary"][side])):
            for kind, p, r in zip(KINDS, maps, recvs):
                assert_recv(r, p, f"{what} {side} layer {l} {kind}")


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(size):
        if size not in cache:
            if size == "tiny":
                cache[size] = build(tiny_config(compute_dtype="bf16", drop_rate=P_DROP), torch.bfloat16), to_dev(tiny_batch())
            else:
                cache[size] = (build(finetune_vqa_rad_config(compute_dtype="bf16", drop_rate=P_DROP), torch.bfloat16),
                               to_dev(full_batch()))
        return cache[size]
    return get


@pytest.mark.parametrize("two_streams", [True, False])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("size", ["tiny", "full"])
def test_bf16_summaries_are_the_mean_of_the_maps_of_the_same_call(models, size, train, two_streams):
    m, b = models(size)
    m.two_streams = two_streams
    m.train(train)

    def run(**kw):
        ops.set_dropout_seed(1234)
        return m.infer(b, **kw)
    try:
        with torch.no_grad():
            plain, summ, both = run(), run(output_attention_summary=True), run(output_attentions=True,
                                                                               output_attention_summary=True)
        torch.cuda.synchronize()
        if train:   # a call that will be differentiated: the composition's saved projections serve the summaries
            both_grad = run(output_attentions=True, output_attention_summary=True)
            torch.cuda.synchronize()
            compare_with_own_maps(both_grad, f"{size} train, grad enabled")
    finally:
        m.two_streams = M3AETransformerSS.two_streams
        m.eval()
    dims = (2, 2, 32, 17) if size == "tiny" else (6, 2, 32, 577)
    check_summary_structure(both["attention_summary"], *dims)
    compare_with_own_maps(both, f"{size} train={train}")
    assert plain["attentions"] is None and "attention_summary" not in plain and summ["attentions"] is None
    for k in FEATS:
        assert torch.equal(plain[k], summ[k]) and torch.equal(plain[k], both[k]), k
    for side in ("text2image", "image2text"):
        for e0, e1 in zip(summ["attention_summary"][side], both["attention_summary"][side]):
            assert torch.equal(e0[0], e1[0]) and torch.equal(e0[1], e1[1])


def test_summary_with_image_dedup_is_per_sample(models):
    m, b = models("tiny")
    img = b["image"][0]
    B = b["text_ids"].shape[0]
    dedup = dict(b, image=[img[:1].contiguous()], image_index=torch.zeros(B, dtype=torch.int64, device="cuda"))
    same = dict(b, image=[img[:1].expand(B, -1, -1, -1).contiguous()])
    with torch.no_grad():
        r0 = m.infer(same, output_attention_summary=True)
        r1 = m.infer(dedup, output_attention_summary=True)
    torch.cuda.synchronize()
    check_summary_structure(r1["attention_summary"], 2, B, 32, 17)
    for side in ("text2image", "image2text"):
        for e0, e1 in zip(r0["attention_summary"][side], r1["attention_summary"][side]):
            assert torch.equal(e0[0], e1[0]) and torch.equal(e0[1], e1[1])


def test_summary_infer_stays_below_one_map_of_extra_memory():
    """Full size, B = 4, bf16, forward-only: the summary infer may cost less than ONE fp32 image self-attention map
    (4 * 12 * 577 * 577 * 4 B = 64 MB) over the plain infer; the maps infer, measured the same way, costs more than that."""
    B = 4
    one_map = B * 12 * 577 * 577 * 4
    m = build(finetune_vqa_rad_config(compute_dtype="bf16"), torch.bfloat16)
    b = to_dev(full_batch(B))

    def peak(**kw):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            ret = m.infer(b, **kw)
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated() - base
        del ret
        return top
    peak()   # (first call: lazily built operand copies)
    plain, summ, maps = peak(), peak(output_attention_summary=True), peak(output_attentions=True)
    print(f"peak over the resident state: plain {plain / 2**20:.1f} MiB, summary +{(summ - plain) / 2**20:.1f} MiB, "
          f"maps +{(maps - plain) / 2**20:.1f} MiB (one map: {one_map / 2**20:.1f} MiB)")
    assert summ - plain < one_map
    assert maps - plain > one_map


@pytest.mark.parametrize("size", [None, 100])
@pytest.mark.parametrize("layer", [0, -1])
@pytest.mark.parametrize("which", ["image_self", "text2image"])
def test_attention_heatmaps_are_the_pipeline_on_the_calls_own_summaries(models, which, layer, size):
    m, b = models("tiny")
    out = m.attention_heatmaps(b, layer=layer, which=which, size=size)
    with torch.no_grad():
        summ = m.infer(b, output_attention_summary=True)["attention_summary"]
    torch.cuda.synchronize()
    S = 64 if size is None else size
    assert out.shape == (2, S, S) and out.dtype == torch.float32 and out.is_cuda and not out.requires_grad
    r = (summ["image2text"][layer][0] if which == "image_self" else summ["text2image"][layer][1]).cpu().numpy()
    assert r.shape == (2, 17)
    want = hm.heatmap(r, S)
    assert np.abs(out.cpu().numpy() - want).max() <= 5 * U * np.abs(r[:, 1:]).max()


def test_decoder_head_heatmap_is_the_models():
    from m3ae_amd.modules import DecoderModel
    from test_gpu_greedy import decoder_cfg
    m = DecoderModel(decoder_cfg("bf16"), vocab_size=1200)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    m.eval()
    b = to_dev(tiny_batch())
    got = m.visualize_attention_heatmap(b, layer_idx=-1)
    want = m.m3ae.attention_heatmaps(b, layer=-1, which="image_self")
    torch.cuda.synchronize()
    assert set(got) == {"heatmaps", "images"}
    assert torch.equal(got["heatmaps"], want) and got["heatmaps"].shape == (2, 64, 64)
    assert got["images"] is b["image"][0]


def test_flag_off_reaches_none_of_the_new_entry_points(models, monkeypatch):
    m, b = models("tiny")
    L = _lib.lib()
    counts = {}

    class Counting:
        def __getattr__(self, name):
            if name in NEW_ENTRIES:
                counts[name] = counts.get(name, 0) + 1
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Counting())
    with torch.no_grad():
        m.infer(b)
        maps = m.infer(b, output_attentions=True)
    m.train()
    try:
        m.store.zero_grad()
        m.training_step(b).backward()
    finally:
        m.eval()
    torch.cuda.synchronize()
    assert counts == {}, counts
    with torch.no_grad():
        both = m.infer(b, output_attentions=True, output_attention_summary=True)
    torch.cuda.synchronize()
    assert counts.get("m3ae_attn_colmean", 0) > 0, counts
    for key in ("text2image_attns", "image2text_attns"):   # the maps are what they were without the summary flag
        for e0, e1 in zip(maps["attentions"][key], both["attentions"][key]):
            assert torch.equal(e0[0], e1[0]) and torch.equal(e0[1], e1[1])
