"""GPU: fusion-layer attention maps, infer(batch, output_attentions=True) (the reference's visualisation hook,
m3ae_module.py:266-283), and the two library entry points behind it (m3ae_attn_probs, m3ae_xattn_probs_export).

Bounds of the bf16 (perf-mode) checks are derived rather than observed.  Against the reference (model level): per entry in log
space, per row in L1 and per map on the Frobenius norm, from a score error of at most 0.1 (tests/attn_map_checks.py, whose
host-side self-check, tests/test_attn_maps_host.py, shows that the bound rejects a uniform and a key-reversed map wherever the
reference's map is farther than the bound from them).  Op-level checks start from bf16-rounded inputs, where the score error is
the rounding of the kernel's own bf16 intermediates only (Q' of the fused path: 2^-9 relative on a score of |s| <= 8 at these
scales -> 0.016; softmax moves a probability by at most half the largest score error): atol 0.01 on probabilities."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import ops, synth  # noqa: E402
from m3ae_amd.config import finetune_vqa_rad_config, tiny_config  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from m3ae_amd.modules.bert_model import BertAttention  # noqa: E402
from m3ae_amd.param_store import ParamStore  # noqa: E402
from attn_map_checks import fro_within_bound, map_errors, within_bf16_bound  # noqa: E402
from oracle_util import full_batch, load_golden, tiny_batch  # noqa: E402

DIRS = (("t2i", "text2image_attns"), ("i2t", "image2text_attns"))
KINDS = ("self", "cross")


def to_dev(batch, dev="cuda"):
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to(dev)
        elif isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            out[k] = [t.to(dev) for t in v]
        else:
            out[k] = v
    return out


def build(cfg, dtype):
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", dtype)
    m.eval()
    return m


def check_structure(att, n_layers, B, H, T, I):
    assert set(att) == {"text2image_attns", "image2text_attns"}
    shapes = {"t2i": ((B, H, T, T), (B, H, T, I)), "i2t": ((B, H, I, I), (B, H, I, T))}
    for tag, key in DIRS:
        assert isinstance(att[key], list) and len(att[key]) == n_layers
        for entry in att[key]:
            assert isinstance(entry, tuple) and len(entry) == 2
            for p, shape in zip(entry, shapes[tag]):
                assert p.dtype == torch.float32 and tuple(p.shape) == shape and p.is_contiguous() and not p.requires_grad


def infer_maps(m, b, **kw):
    with torch.no_grad():
        ret = m.infer(b, output_attentions=True, **kw)
    torch.cuda.synchronize()
    return ret


# ------------------------------------------------------------------------------------------------------------------------
# 1. reference parity, parity mode
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_streams", [True, False])
def test_tiny_fp32_maps_equal_the_reference(two_streams):
    m = build(tiny_config(compute_dtype="fp32"), torch.float32)
    m.two_streams = two_streams
    g = load_golden("attn_maps.npz")
    ret = infer_maps(m, to_dev(tiny_batch()))
    att = ret["attentions"]
    check_structure(att, 2, 2, 2, 32, 17)
    for tag, key in DIRS:
        for l, entry in enumerate(att[key]):
            for kind, p in zip(KINDS, entry):
                np.testing.assert_allclose(p.cpu().numpy(), g[f"tiny_{tag}_{l}_{kind}"], rtol=1e-4, atol=1e-6,
                                           err_msg=f"{tag} layer {l} {kind}")


# ------------------------------------------------------------------------------------------------------------------------
# 2. reference parity, perf mode
# ------------------------------------------------------------------------------------------------------------------------
# The fused cross-attention kernels keep P in bf16 (what multiplies V there): each entry carries bf16 rounding (unit roundoff
# 2^-8), so a row of them sums to 1 within sum_k p_k 2^-8 = 2^-8 on top of the fp32 error.  fp32 maps: 1e-3.
ROWSUM_FP32, ROWSUM_BF16 = 1e-3, 1e-3 + 2.0 ** -8


def rows_sum_to_one(p, key_mask, tol=ROWSUM_FP32):
    """Every query row sums to 1 over the keys; rows are never fully masked here (key 0 is always a real token)."""
    s = p.double().sum(-1)
    assert (s - 1).abs().max().item() < tol
    if key_mask is not None:   # padding keys carry the additive -10000 mask: exactly 0
        pad = (key_mask < -1).to(p.device)[:, None, None, :].expand_as(p)
        assert (p[pad] == 0).all()


def test_tiny_bf16_composition_maps_match_the_reference():
    """At the tiny dims (H * T = 64, 17 image tokens) the fused cross-attention kernels cover neither direction, so every map
    here comes from the composition (flash attention): the fused path is pinned at full size (CLS rows below) and at op level
    (test_fused_export_against_the_reference_formulation).  The tiny reference's layer-0 maps lie within 0.04 (log) of uniform,
    inside any bf16-derived bound: what pins their values is the parity-mode test above (rtol 1e-4)."""
    m = build(tiny_config(compute_dtype="bf16"), torch.bfloat16)
    g = load_golden("attn_maps.npz")
    b = to_dev(tiny_batch())
    ret = infer_maps(m, b)
    att = ret["attentions"]
    check_structure(att, 2, 2, 2, 32, 17)
    mt = ret["extended_text_masks"]
    for tag, key in DIRS:
        for l, entry in enumerate(att[key]):
            for kind, p in zip(KINDS, entry):
                got, ref = p.cpu().numpy(), g[f"tiny_{tag}_{l}_{kind}"]
                assert within_bf16_bound(got, ref), (tag, l, kind, map_errors(got, ref))
                text_keys = (tag == "t2i") == (kind == "self")
                rows_sum_to_one(p, mt if text_keys else None, ROWSUM_FP32 if kind == "self" else ROWSUM_BF16)


@pytest.fixture(scope="module")
def full_bf16():
    m = build(finetune_vqa_rad_config(compute_dtype="bf16"), torch.bfloat16)
    return m, to_dev(full_batch())


def test_full_size_bf16_cls_rows_match_the_reference(full_bf16):
    m, b = full_bf16
    g = load_golden("attn_maps.npz")
    ret = infer_maps(m, b)
    att = ret["attentions"]
    check_structure(att, 6, 2, 12, 32, 577)
    for tag, key in DIRS:
        for l, entry in enumerate(att[key]):
            for kind, p in zip(KINDS, entry):
                cls, ref = p[:, :, 0, :].cpu().numpy(), g[f"full_{tag}_{l}_{kind}_cls"]
                assert within_bf16_bound(cls, ref), (tag, l, kind, map_errors(cls, ref))
                # the whole map: every entry within the relative bound -> its Frobenius norm too
                fro = p.double().flatten(2).norm(dim=-1).cpu().numpy()
                assert fro_within_bound(fro, g[f"full_{tag}_{l}_{kind}_fro"]), (tag, l, kind)
                text_keys = (tag == "t2i") == (kind == "self")
                rows_sum_to_one(p, ret["extended_text_masks"] if text_keys else None,
                                ROWSUM_FP32 if kind == "self" else ROWSUM_BF16)


# ------------------------------------------------------------------------------------------------------------------------
# 3. the default path is untouched
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_streams", [True, False])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_features_bit_identical_with_and_without_maps(mode, two_streams, full_bf16):
    if mode == "bf16":   # full size: the image-query fused kernel (H * T = 384) runs its copy-out variant when maps are asked
        m, b = full_bf16
    else:
        m, b = build(tiny_config(compute_dtype="fp32"), torch.float32), to_dev(tiny_batch())
    m.two_streams = two_streams
    try:
        with torch.no_grad():
            plain = m.infer(b)
            maps = m.infer(b, output_attentions=True)
        torch.cuda.synchronize()
    finally:
        m.two_streams = M3AETransformerSS.two_streams
    assert plain["attentions"] is None and maps["attentions"] is not None
    for k in ("multi_modal_text_feats", "multi_modal_image_feats", "multi_modal_cls_feats"):
        assert torch.equal(plain[k], maps[k]), k


# ------------------------------------------------------------------------------------------------------------------------
# 4. training-mode maps are the dropped P the path used
# ------------------------------------------------------------------------------------------------------------------------
P_DROP = 0.1


def check_dropped(pd, pe, p=P_DROP):
    """Every entry of the dropped map is 0 or P_eval / (1 - p); the kept fraction is binomial(n, 1 - p) (5 sigma)."""
    live = pe > 0
    kept = pd != 0
    scaled = pe / (1 - p)
    assert torch.allclose(pd[kept], scaled[kept], rtol=1e-2, atol=1e-6)
    n = live.sum().item()
    frac = (kept & live).sum().item() / n
    assert abs(frac - (1 - p)) < 5 * math.sqrt(p * (1 - p) / n), frac
    assert not (kept & ~live).any()


def rand_qkv(B, Lq, Lk, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    D = 64 * H
    q = torch.randn(B, Lq, D, device="cuda", generator=g).to(torch.bfloat16)
    k = torch.randn(B, Lk, D, device="cuda", generator=g).to(torch.bfloat16)
    v = torch.randn(B, Lk, D, device="cuda", generator=g).to(torch.bfloat16)
    lens = torch.randint(1, Lk + 1, (B,), device="cuda", generator=g)
    mask = ((torch.arange(Lk, device="cuda")[None, :] >= lens[:, None]).float() * -10000.0).contiguous()
    return q, k, v, mask


def torch_probs(q, k, H, mask):
    B, Lq, D = q.shape
    sp = lambda t: t.float().view(B, t.shape[1], H, D // H).permute(0, 2, 1, 3)
    s = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(D // H)
    if mask is not None:
        s = s + mask[:, None, None, :]
    return torch.softmax(s, -1)


def test_flash_training_maps_are_the_dropped_p_that_multiplied_v():
    B, L, H = 3, 577, 4
    q, k, v, mask = rand_qkv(B, L, L, H, 7)
    seed = 0x1234
    with torch.no_grad():
        o, lse = ops.attn_forward(q, k, v, H, mask, dropout=(P_DROP, seed))
        pd = ops.attn_probs(q, k, lse, H, mask, dropout=(P_DROP, seed))
        oe, lse_e = ops.attn_forward(q, k, v, H, mask)
        pe = ops.attn_probs(q, k, lse_e, H, mask)
    torch.cuda.synchronize()
    sp = v.float().view(B, L, H, 64).permute(0, 2, 1, 3)
    ctx = (pd @ sp).permute(0, 2, 1, 3).reshape(B, L, H * 64)
    # the forward multiplies V by bf16(P) and rounds O to bf16: 2^-8 relative on each term and on the result
    assert torch.allclose(ctx, o.float(), rtol=2e-2, atol=2e-2), (ctx - o.float()).abs().max().item()
    check_dropped(pd, pe)


def make_cross(seed=0, wscale=1.0):
    D, H = 768, 12
    torch.manual_seed(seed)
    att = BertAttention(D, H, 1e-12, cross=True)
    with torch.no_grad():
        for n, p in att.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn_like(p) * (wscale / math.sqrt(p.shape[1])))
            elif "LayerNorm.weight" in n:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            else:
                p.copy_(0.1 * torch.randn_like(p))
    cfg = dict(learning_rate=1e-3, weight_decay=0.01, lr_multiplier_head=1, lr_multiplier_multi_modal=1)
    store = ParamStore(att, cfg, "cuda", torch.bfloat16, weight_units=att.weight_units)
    att.eval()
    return att, store


def cross_inputs(B, L, Lo, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, L, 768, device="cuda", generator=g).to(torch.bfloat16)
    y = torch.randn(B, Lo, 768, device="cuda", generator=g).to(torch.bfloat16)
    mask = None
    if Lo == 32:   # text keys carry the padding mask
        lens = torch.randint(1, Lo + 1, (B,), device="cuda", generator=g)
        mask = ((torch.arange(Lo, device="cuda")[None, :] >= lens[:, None]).float() * -10000.0).contiguous()
    return x, y, mask


def fused_probs(att, x, y, mask, pdrop=0.0, need_bwd=False):
    P = att.block_params()
    B, L, D = x.shape
    Lo = y.shape[1]
    h2, o2 = x.reshape(B * L, D), y.reshape(B * Lo, D)
    old = ops.XATTN
    ops.XATTN = "always"
    try:
        assert ops.xattn_supported(h2, L, o2, Lo, mask, P)
        with torch.no_grad():
            _, saved = ops.xattn_fwd(h2, B, L, o2, Lo, mask, P, pdrop, need_bwd=need_bwd, want_probs=True)
            return ops.xattn_probs(saved)
    finally:
        ops.XATTN = old


@pytest.mark.parametrize("L,Lo", [(32, 577), (577, 32)])
def test_fused_training_maps_are_the_dropped_p(L, Lo):
    att, _ = make_cross(seed=L)
    x, y, mask = cross_inputs(2, L, Lo, 11)
    pe = fused_probs(att, x, y, mask)
    pd = fused_probs(att, x, y, mask, pdrop=P_DROP, need_bwd=True)
    torch.cuda.synchronize()
    check_dropped(pd, pe)


# ------------------------------------------------------------------------------------------------------------------------
# 5. shapes
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("Lq,Lk", [(32, 32), (577, 577), (1025, 1025), (32, 577), (577, 32), (32, 1025)])
def test_attn_probs_against_torch_softmax(B, Lq, Lk):
    H = 2 if B == 32 else 3
    q, k, v, mask = rand_qkv(B, Lq, Lk, H, B * 7919 + Lq + Lk)
    with torch.no_grad():
        _, lse = ops.attn_forward(q, k, v, H, mask)
        p = ops.attn_probs(q, k, lse, H, mask)
    ref = torch_probs(q, k, H, mask)
    torch.cuda.synchronize()
    assert p.shape == (B, H, Lq, Lk) and p.dtype == torch.float32 and p.is_contiguous()
    # same bf16 inputs: only fp32 evaluation order and exp2 differ
    assert (p - ref).abs().max().item() < 1e-4
    rows_sum_to_one(p, mask)


@pytest.mark.parametrize("Lq,Lk", [(32, 32), (577, 577), (32, 577)])
def test_attn_probs_fp32_parity_mode_against_torch_softmax(Lq, Lk):
    B, H = 3, 2
    q, k, v, mask = (t.float() if t.dtype == torch.bfloat16 else t for t in rand_qkv(B, Lq, Lk, H, Lq + 3 * Lk))
    with torch.no_grad():
        _, lse = ops.attn_forward(q, k, v, H, mask)
        p = ops.attn_probs(q, k, lse, H, mask)
    ref = torch_probs(q, k, H, mask)
    torch.cuda.synchronize()
    torch.testing.assert_close(p, ref, rtol=1e-5, atol=1e-6)
    rows_sum_to_one(p, mask)


@pytest.mark.parametrize("L,Lo", [(32, 17), (32, 577), (17, 32), (577, 32), (1025, 32)])
def test_fused_export_against_the_reference_formulation(L, Lo):
    """T = 32 text tokens, I in {17, 577} image tokens both ways, and 1025 image queries.  The shorter side is the text side
    of the fused kernels: with 17 image tokens it is the image side, which they do not cover (those layers take the
    composition, pinned by test_attn_probs_against_torch_softmax); above 640 keys the text-query direction leaves them too."""
    B = 3
    att, _ = make_cross(seed=L + Lo)
    x, y, mask = cross_inputs(B, L, Lo, L * Lo)
    if min(L, Lo) == 17:
        old, ops.XATTN = ops.XATTN, "always"
        try:
            assert not ops.xattn_supported(x.reshape(B * L, 768), L, y.reshape(B * Lo, 768), Lo, mask, att.block_params())
        finally:
            ops.XATTN = old
        return
    p = fused_probs(att, x, y, mask)
    f = lambda w: w.m3ae_c.float()
    sa = att.self
    qf = x.float() @ f(sa.query.weight).t() + sa.query.bias
    kf = y.float() @ f(sa.key.weight).t() + sa.key.bias
    ref = torch_probs(qf, kf, 12, mask)
    torch.cuda.synchronize()
    assert p.shape == (B, 12, L, Lo) and p.dtype == torch.float32 and p.is_contiguous()
    err = (p - ref).abs().max().item()
    assert err < 0.01, err
    rows_sum_to_one(p, mask, ROWSUM_BF16)
