"""GPU: the fused cross-attention sub-block (csrc/xattn.hip, csrc/xflash.hip: m3ae_xattn_fwd / m3ae_xattn_bwd through ops.xattn_fwd /
ops.xattn_bwd) against a float64 reference of the REFERENCE'S formulation, held to an error budget that a rounding model of the
kernels computes on every run (tests/xattn_accuracy.py; tests/test_xattn_accuracy_host.py shows on the host that the criteria pass
the model and reject twelve subtly wrong kernels).  The yardsticks are plain torch on the GPU (float64 / fp32).
  A. out, dx, dother and every parameter gradient within the budget, both directions, at image-token counts on the tile and wave
     boundaries, 32 and 64 text tokens, one sample, split-K shapes, with and without key mask and dropout, in three input regimes
     (unit, peaked, masked); the key bias gradient buffer bit for bit what it held before the call; a forward-only call's output
     bit for bit the training call's.
  B. The saved probabilities (and the dropped, rescaled ones) entry by entry against the float64 softmax at the boundary shapes in
     the masked regime; direction 0's padded columns Lk .. 639 of probs, probs_drop and ws_dscores exactly 0 in buffers pre-filled
     with NaN.  (Every call of this file runs on NaN-pre-filled buffers and checks the padding.)
  C. Buffer contracts: x, y, d_out and every output, saved buffer and workspace as views of NaN-fenced buffers: the same bits as the
     tight call, every fence intact.
  D. The envelope of m3ae_xattn_supported: every (direction, text tokens, head width) class it accepts runs criterion A at a small
     member; what lies outside (head widths above 256 among others) is refused.
Every test prints the kernel's and the model's figures; DESIGN.md (6e, item 2c "Cross-attention accuracy") tabulates the worst ones."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, ops  # noqa: E402
from m3ae_amd.modules.bert_model import BertAttention  # noqa: E402
from m3ae_amd.param_store import ParamStore  # noqa: E402

import xattn_accuracy as xa  # noqa: E402

DROP_SEED = 4321
SEEDS = ((DROP_SEED << 32) | 1, (DROP_SEED << 32) | 2)     # ops.next_dropout_seed after set_dropout_seed: attention probabilities, hidden
NAN_BITS = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}   # quiet NaNs with a payload of their own
_BLOCKS = {}


def ids(s):
    return "dir{}-B{}-T{}-I{}".format(*s)


def bits(t):
    return t.contiguous().view(NAN_BITS[t.dtype][0])


def nan_filled(n, dt):
    word, pattern = NAN_BITS[dt]
    return torch.full((n,), pattern, dtype=word, device="cuda").view(dt)


def block(D, H):
    """One BertAttention with its ParamStore per (D, H); load() puts a case's parameters into it."""
    if (D, H) not in _BLOCKS:
        att = BertAttention(D, H, xa.LN_EPS, cross=True)
        cfg = dict(learning_rate=1e-3, weight_decay=0.01, lr_multiplier_head=1, lr_multiplier_multi_modal=1)
        _BLOCKS[(D, H)] = (att, ParamStore(att, cfg, "cuda", torch.bfloat16, weight_units=att.weight_units))
    return _BLOCKS[(D, H)]


def load(case):
    att, store = block(case["D"], case["H"])
    params = dict(att.named_parameters())
    with torch.no_grad():
        for k, n in xa.PARAMS.items():
            params[n].data.copy_(case[k])
    store.sync_shadows()          # the bf16 compute copies (exact: the case's weights are bf16 values) and their transposes
    return att, store


def gpu_case(shape, regime, masked, drop, seed=2000, **kw):
    case = xa.to_device(xa.make_case(*shape, regime=regime, masked=masked, p=xa.DROP_P if drop else 0.0, seed=seed + 7 * shape[3] + shape[0], **kw),
                        "cuda")
    if drop:   # the library's own masks of (p, seed), with the index conventions of its dropout sites
        B, H, Lq, Lk, D = (case[k] for k in ("B", "H", "Lq", "Lk", "D"))
        case["keep_a"] = ops.dropout_keep_mask(B * H * Lq, Lk, xa.DROP_P, SEEDS[0]).view(B, H, Lq, Lk)
        case["keep_h"] = ops.dropout_keep_mask(B * Lq, D, xa.DROP_P, SEEDS[1]).view(B, Lq, D)
    return case


class Buffers:
    """The allocator handed to ops.xattn_fwd / ops.xattn_bwd: every buffer pre-filled with NaN bit patterns and kept by name; with
    fence > 0 each is a view into a larger NaN-filled buffer with `fence` rows of its last dimension before and after it."""

    def __init__(self, fence=0):
        self.fence, self.views, self.whole = fence, {}, {}

    def __call__(self, name, shape, dt=torch.bfloat16):
        n = math.prod(shape)
        pad = self.fence * ((shape[-1] + 7) // 8 * 8)
        buf = nan_filled(n + 2 * pad, dt)
        self.whole[name], self.views[name] = buf, buf[pad:pad + n].view(shape)
        return self.views[name]

    def put(self, name, t):
        self(name, tuple(t.shape), t.dtype).copy_(t)
        return self.views[name]

    def fences_intact(self, name):
        buf, n = self.whole[name], self.views[name].numel()
        pad = (buf.numel() - n) // 2
        word, pattern = NAN_BITS[buf.dtype]
        b = buf.view(word)
        return bool((b[:pad] == pattern).all()) and bool((b[pad + n:] == pattern).all())


def kernels(case, bufs=None, need_bwd=True):
    """ops.xattn_fwd + ops.xattn_bwd on the case as it stands, with ops.XATTN = "always".  Returns a result dict like the rounding
    model's (tensors on the GPU) plus "bufs", the named buffers of the call, and "g_bk_intact"."""
    att, store = load(case)
    P = att.block_params()
    B, Lq, Lk, D, H, p = (case[k] for k in ("B", "Lq", "Lk", "D", "H", "p"))
    bufs = bufs or Buffers()
    bf = lambda n: bufs.put(n, case[n].to(torch.bfloat16).view(-1, D))
    x2, y2, dout2 = bf("x"), bf("y"), bf("dout")
    store.zero_grad()
    params = dict(att.named_parameters())
    gbk = params[xa.KEY_BIAS].grad
    gbk.copy_(torch.arange(D, device="cuda", dtype=torch.float32) * 0.25 - 3.0)
    gbk_before = gbk.clone()
    ops.set_dropout_seed(DROP_SEED)
    old = ops.XATTN
    ops.XATTN = "always"
    try:
        assert ops.xattn_supported(x2, Lq, y2, Lk, case["mask"], P, backward=need_bwd)
        out, saved = ops.xattn_fwd(x2, B, Lq, y2, Lk, case["mask"], P, p, need_bwd=need_bwd, alloc=bufs)
        res = dict(out=out.float().view(B, Lq, D), bufs=bufs)
        if not need_bwd:
            torch.cuda.synchronize()
            return res
        dx, dother = ops.xattn_bwd(dout2, saved, B, Lq, Lk, P, alloc=bufs)
        exported = ops.xattn_probs(saved)
    finally:
        ops.XATTN = old
    torch.cuda.synchronize()
    res.update(dx=dx.float().view(B, Lq, D), dother=dother.float().view(B, Lk, D), g_bk_intact=torch.equal(bits(gbk), bits(gbk_before)))
    res.update({g: params[n].grad.clone() for g, n in xa.GRADS.items()})
    t = saved[4]
    T, I = case["T"], case["I"]
    if case["direction"] == 0:     # [B][rows t H + h][640 key columns]
        probs = lambda b: b.view(B, T, H, 640)[..., :I].permute(0, 2, 1, 3).float()
    else:                          # [B][I][columns h T + j]
        probs = lambda b: b.view(B, I, H, T).permute(0, 2, 1, 3).float()
    res["P0"] = probs(t["probs"])
    res["P"] = probs(t["probs_drop"]) if p > 0 else res["P0"]
    res["export_ok"] = torch.equal(exported, res["P"])
    return res


def padding_is_zero(res, case):
    """Direction 0: columns Lk .. 639 of probs, probs_drop and ws_dscores are exactly 0 (the backward products Z = drop(P) y and
    dQ' = dS y reduce over ceil32(Lk) of them); the buffers were pre-filled with NaN bit patterns."""
    if case["direction"] != 0:
        return []
    v = res["bufs"].views
    return [n for n in ("probs", "probs_drop", "ws_dscores") if n in v and not bool((v[n][..., case["Lk"]:] == 0).all())]


def check(case, label, figures=None, probs=True):
    """Criterion A (and B with probs) of one case; returns the failures and the kernels' result."""
    res = kernels(case)
    bad = xa.check_budget(res, case, label, figures) + (xa.check_probs(res, case, label, figures) if probs else [])
    bad += [n + " padding" for n in padding_is_zero(res, case)]
    finite = all(bool(torch.isfinite(res[n]).all()) for n in xa.TENSORS)
    return bad + [n for n, ok in (("finite", finite), ("key.bias gradient touched", res["g_bk_intact"]), ("xattn_probs export", res["export_ok"]))
                  if not ok], res


def configs(regime):
    return [(m, d) for m in ((True,) if regime == "masked" else (False, True)) for d in (False, True)]


# ------------------------------------------------------------------------------------------------------------------------
# A. budget against the rounding model
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", xa.REGIMES)
@pytest.mark.parametrize("shape", xa.A_SHAPES + xa.SPLITK_SHAPES, ids=ids)
def test_cross_attention_within_the_rounding_budget(shape, regime):
    if shape in xa.SPLITK_SHAPES:     # the shape really splits the reduction of the XE_ATOMIC weight gradients, raggedly where it can
        ksplit, kchunks, last = xa.pick_split(shape[1], shape[2], 12, 768)
        assert ksplit == (3 if shape[1] == 13 else 2) and (last < kchunks or shape[1:3] == (9, 64)), (ksplit, kchunks, last)
    for masked, drop in configs(regime):
        case = gpu_case(shape, regime, masked, drop)
        label = f"A {ids(shape)} {regime} mask {int(masked)} drop {int(drop)}"
        bad, res = check(case, label, probs=False)
        assert not bad, f"{label}: {bad}"
        if regime == "masked":     # the other stream's gradient at masked rows is what the reference gives: through the budget above, and
            hidden = (case["mask"] < 0) & (case["mask"] == 0).any(-1, keepdim=True)   # exactly 0 where the probability is exactly 0
            assert bool((xa.yardsticks(case)[0]["dother"][hidden] == 0).all()) and bool((res["dother"][hidden] == 0).all()), label


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("shape", [(0, 2, 32, 577), (0, 2, 64, 65), (1, 2, 32, 129), (1, 2, 64, 129)], ids=ids)
def test_forward_only_call_computes_the_training_call_bit_for_bit(shape, drop):
    case = gpu_case(shape, "unit", True, drop)
    train = kernels(case)["out"]
    assert torch.equal(kernels(case, need_bwd=False)["out"], train)


# ------------------------------------------------------------------------------------------------------------------------
# B. the saved probabilities entry by entry
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("shape", xa.B_SHAPES, ids=ids)
def test_saved_probabilities_entry_by_entry(shape, drop):
    case = gpu_case(shape, "masked", True, drop)
    label = f"B {ids(shape)} masked drop {int(drop)}"
    res = kernels(case)
    bad = xa.check_probs(res, case, label) + [n + " padding" for n in padding_is_zero(res, case)]
    assert not bad and res["export_ok"], f"{label}: {bad}"


# ------------------------------------------------------------------------------------------------------------------------
# C. buffer contracts (everything inside memory the test allocated)
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("shape", xa.C_SHAPES, ids=ids)
def test_fenced_buffers_give_the_same_bits_and_keep_their_fences(shape, drop):
    """x, y, d_out and every output, saved buffer and workspace of the descriptor are views into larger buffers whose other bytes
    hold NaN bit patterns -- 64 rows before and after each, the rows right after the last sample included.  After forward + backward
    every buffer holds the bits of the call on tight allocations and every fence is intact.  (The parameter gradients accumulate
    with fp32 atomics into the ParamStore's buffer; criterion A holds them.)"""
    case = gpu_case(shape, "unit", True, drop)
    tight, fenced = kernels(case)["bufs"], kernels(case, bufs=Buffers(fence=64))["bufs"]
    assert set(tight.views) == set(fenced.views) and {"out", "dx", "dy", "probs", "ws_dscores", "ws_vec", "ws_ln"} <= set(fenced.views)
    for n in fenced.views:
        assert fenced.fences_intact(n), f"{n}: a store outside the buffer"
        assert torch.equal(bits(fenced.views[n]), bits(tight.views[n])), f"{n}: differs from the call on tight allocations"


# ------------------------------------------------------------------------------------------------------------------------
# D. the envelope of m3ae_xattn_supported
# ------------------------------------------------------------------------------------------------------------------------
def supported(direction, D, H, T, I=65, backward=False):
    d = _lib.XattnDesc()
    d.dir, d.B, d.D, d.H = direction, 1, D, H
    d.Lq, d.Lk = (T, I) if direction == 0 else (I, T)
    fwd, bwd = (bool(f(C.byref(d))) for f in (_lib.lib().m3ae_xattn_supported, _lib.lib().m3ae_xattn_bwd_supported))
    assert bwd == (fwd and D <= 2048), "the backward covers what the forward does, up to the LayerNorm backward's 2048 columns"
    return bwd if backward else fwd


@pytest.mark.parametrize("cls", xa.D_CLASSES, ids=lambda c: "dir{}-D{}-H{}-T{}-I{}".format(*c))
def test_every_supported_class_runs_within_the_budget(cls):
    """Forward + backward where m3ae_xattn_bwd_supported says so; the classes whose members are all wider than 2048 (direction 1 at
    head widths 192 and 256: D = 12 dh) exist as forward-only calls: their out is held to the budget."""
    direction, D, H, T, I = cls
    assert supported(direction, D, H, T, I)
    for masked, drop in ((False, False), (True, False), (True, True)):
        case = gpu_case((direction, 2, T, I), "unit", masked, drop, D=D, H=H)
        label = f"D dir{direction} D{D} H{H} T{T} mask {int(masked)} drop {int(drop)}"
        if supported(direction, D, H, T, I, backward=True):
            bad, _ = check(case, label)
        else:
            bad = xa.check_budget(kernels(case, need_bwd=False), case, label + " forward only", names=("out",))
        assert not bad, f"{label}: {bad}"


def test_everything_supported_belongs_to_a_tested_class():
    """Over hidden widths up to 4608, 1 .. 64 heads and text lengths around the covered ones: what m3ae_xattn_supported answers 1
    for lies in a class (direction, text tokens, head width) of xattn_accuracy.D_CLASSES, and what m3ae_xattn_bwd_supported answers 1
    for in one whose member runs the backward; head widths above 256 and hidden widths above 4096 are refused."""
    tested = {(d, T, D // H): D <= 2048 for d, D, H, T, _ in xa.D_CLASSES}
    seen = set()
    for direction in (0, 1):
        for D in range(128, 4609, 128):
            for H in range(1, 65):
                for T in (16, 32, 48, 64, 96):
                    if supported(direction, D, H, T):
                        cls = (direction, T, D // H)
                        assert D % H == 0 and D <= 4096 and cls in tested, (direction, D, H, T)
                        assert tested[cls] or not supported(direction, D, H, T, backward=True), (direction, D, H, T)
                        seen.add(cls)
    assert seen == set(tested)
    assert not supported(0, 1152, 4, 32) and not supported(1, 3840, 12, 32) and not supported(1, 3840, 12, 64)     # dh = 288, 320
    assert not supported(0, 768, 12, 32, I=641) and supported(0, 768, 12, 32, I=640) and supported(1, 768, 12, 32, I=4097)
