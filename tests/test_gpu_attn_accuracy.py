"""GPU: the bf16 flash attention kernels (csrc/attention.hip) against a float64 reference, held to an error budget that a
rounding model of the kernels computes on every run (tests/attn_accuracy.py; tests/test_attn_accuracy_host.py shows on the host that
the criteria pass two models and reject nine subtly wrong kernels).
  A. o, dq, dk, dv within the budget at the workload's shapes and ragged ones, with and without key mask and dropout, both backward
     generations, on the layers' packed q | k | v layouts.
  B. Probes that make an output element equal ONE probability: the P that the forward's P.V product and the dK/dV kernels use is read
     entry by entry at tile edges and tails; a one-row dO makes dk a one-term product.
  C. Every key mask | position bias | causal instance without dropout, the two biased dropout instances at ragged shapes, d_pos_bias
     included, in two input regimes; the T5 generation step's exact call.
  D. Buffer contracts: outputs as strided views of sentinel-filled buffers, and a log-sum-exp table wider than ceil32(Lq).
Every test prints the kernel's and the model's figures; DESIGN.md (6e, item 2b "Attention accuracy") tabulates the worst ones."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, ops  # noqa: E402

import attn_accuracy as aa  # noqa: E402

B, H = 2, 2
D = H * aa.DH
DROP_SEED = 0xA77E57


def gpu_case(Lq, Lk, seed, drop=False, **kw):
    case = aa.make_case(B, H, Lq, Lk, seed, p=aa.DROP_P if drop else 0.0, drop_seed=DROP_SEED, **kw)
    if drop:   # the library's own mask of (p, seed), as the existing dropout tests take it
        case["keep"] = ops.dropout_keep_mask(B * H * Lq, Lk, aa.DROP_P, DROP_SEED).view(B, H, Lq, Lk).cpu()
    return case


def device_views(bufs):
    """The case's packed buffers on the device and the q, k, v views the layers take of them."""
    bufs = [b.cuda() for b in bufs]
    if len(bufs) == 1:
        return bufs, (bufs[0][..., :D], bufs[0][..., D:2 * D], bufs[0][..., 2 * D:])
    return bufs, (bufs[0], bufs[1][..., :D], bufs[1][..., D:])


def kernels(case):
    """The candidate of the criteria: ops.attn_forward + ops.attn_backward on the case as it stands."""
    bufs, (q, k, v) = device_views(case["bufs"])
    gbufs, (dq, dk, dv) = device_views([torch.zeros_like(b) for b in case["bufs"]])
    mask = case["key_mask"].cuda() if case["key_mask"] is not None else None
    bias = case["pos_bias"].cuda().contiguous() if case["pos_bias"] is not None else None
    drop = (case["p"], case["drop_seed"]) if case["p"] > 0 else None
    kw = dict(scale=case["scale"], causal=case["causal"], dropout=drop)
    o, lse = ops.attn_forward(q, k, v, H, mask, bias, **kw)
    dbias = torch.zeros_like(bias) if bias is not None else None
    ops.attn_backward(q, k, v, o, lse, case["do"].cuda(), dq, dk, dv, H, mask, bias, d_pos_bias=dbias, **kw)
    torch.cuda.synchronize()
    return aa.Result(o.cpu(), dq.cpu(), dk.cpu(), dv.cpu(), dbias.cpu() if dbias is not None else None, None)


def ids(s):
    return f"{s[0]}x{s[1]}"


# ------------------------------------------------------------------------------------------------------------------------
# A. budget against the rounding model
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "keymask"])
@pytest.mark.parametrize("shape", aa.A_SHAPES, ids=ids)
def test_attention_within_the_rounding_budget(shape, masked, drop):
    case = gpu_case(*shape, seed=300, drop=drop, masked=masked)
    bad = aa.check_budget(kernels, case, f"A {ids(shape)} mask {int(masked)} drop {int(drop)}")
    assert not bad, f"over the rounding-model budget: {bad}"


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "keymask"])
@pytest.mark.parametrize("shape", [(577, 577), (33, 65)], ids=ids)
def test_legacy_backward_within_the_rounding_budget(shape, masked, drop):
    case = gpu_case(*shape, seed=300, drop=drop, masked=masked)
    try:
        ops.ATTN_LEGACY = True
        bad = aa.check_budget(kernels, case, f"A legacy {ids(shape)} mask {int(masked)} drop {int(drop)}")
    finally:
        ops.ATTN_LEGACY = False
    assert not bad, f"over the rounding-model budget: {bad}"


# ------------------------------------------------------------------------------------------------------------------------
# B. probes
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", aa.B_VARIANTS)
@pytest.mark.parametrize("shape", aa.B_SHAPES, ids=ids)
def test_probabilities_entry_by_entry_at_tile_edges(shape, variant):
    kw = dict(seed=aa.PROBE_SEED, masked=variant == "masked", probe_mask=True, drop=variant == "dropout")
    label = f"B {ids(shape)} {variant}"
    bad, _ = aa.check_v_probe_case(kernels, gpu_case(*shape, **kw), label)
    assert not bad, bad
    bad, _ = aa.check_do_probe_case(kernels, gpu_case(*shape, **kw), label)
    assert not bad, bad


@pytest.mark.parametrize("variant", aa.B_VARIANTS)
@pytest.mark.parametrize("shape", aa.B_SHAPES, ids=ids)
def test_dk_of_a_single_query_row_is_a_one_term_product(shape, variant):
    kw = dict(seed=aa.PROBE_SEED, masked=variant == "masked", probe_mask=True, drop=variant == "dropout")
    case = gpu_case(*shape, **kw)
    for row in aa.single_rows(shape[0]):
        bad, _ = aa.check_single_row_case(kernels, case, row, f"B {ids(shape)} {variant}")
        assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# C. the instances with a position bias and / or causal, and the generation step
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["unit", "t5"])
@pytest.mark.parametrize("inst", aa.c_cases(), ids=lambda c: c[0])
def test_mask_bias_causal_instances_within_the_rounding_budget(inst, regime):
    label, Lq, Lk, drop, kw = inst
    case = gpu_case(Lq, Lk, seed=400, drop=drop, **(aa.t5_regime(kw) if regime == "t5" else kw))
    bad = aa.check_budget(kernels, case, f"C {regime} {label}")
    assert not bad, f"over the rounding-model budget: {bad}"


@pytest.mark.parametrize("Lk", [1, 32, 33, 70])
def test_t5_generation_step_call(Lk):
    """The attention call of ops.t5_self_attn_step at position t = Lk - 1: one query per sequence out of a packed [B, 3 inner]
    projection (batch stride 3 inner), keys / values as views of the [B, Tmax, 2 inner] cache, bias [H, 1, t + 1], scale 1."""
    inner, Tmax = D, 72
    qkv = aa.randn_bf16(B, 3 * inner, seed=600, scale=0.35).cuda()
    cache = aa.randn_bf16(B, Tmax, 2 * inner, seed=601).cuda()
    cache[..., :inner] = (cache[..., :inner].float() * 0.35).to(torch.bfloat16)
    bias = (0.5 * torch.randn(H, 1, Lk, generator=torch.Generator().manual_seed(602))).cuda()
    q = qkv[:, :inner].unsqueeze(1)
    k, v = cache[:, :Lk, :inner], cache[:, :Lk, inner:]
    assert q.stride(0) == 3 * inner and k.stride() == (Tmax * 2 * inner, 2 * inner, 1)
    o, _ = ops.attn_forward(q, k, v, H, None, bias, scale=1.0, causal=False, dropout=None)
    torch.cuda.synchronize()
    args = dict(q=q.cpu(), k=k.cpu(), v=v.cpu(), do=torch.zeros(B, 1, inner, dtype=torch.bfloat16), H=H, pos_bias=bias.cpu(), scale=1.0)
    ref, model = aa.reference(**args), aa.rounding_model(**args)
    if Lk == 1:   # P = 1: the output is v, bit for bit
        assert torch.equal(o.view(torch.int16), v.contiguous().view(torch.int16))
        assert aa.max_abs(model.o, ref.o) == 0
    else:
        got = aa.Result(o.cpu(), None, None, None, None, None)
        assert not aa.budget_report(got, model, ref, ("o",), f"C generation step Lk {Lk}")


# ------------------------------------------------------------------------------------------------------------------------
# D. buffer contracts (everything inside memory the test allocated)
# ------------------------------------------------------------------------------------------------------------------------
SENTINEL = 768.0   # exact in bf16 and fp32


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


GEO = {"q": (2, 8, 8), "k": (3, 16, 8), "v": (1, 0, 8), "o": (2, 8, 24)}   # spare rows after L, spare columns before / after the heads


def live(buf, L, g):
    return buf[:, :L, GEO[g][1]:GEO[g][1] + D]


def fenced(x, g):
    """(buffer, view): x [B, L, D] as a view of a larger sentinel-filled buffer, with spare rows after L and spare columns on both
    sides of the head range.  Token stride and base offset stay multiples of 8 elements (16 bytes)."""
    rows_after, c0, c1 = GEO[g]
    buf = torch.full((x.shape[0], x.shape[1] + rows_after, c0 + D + c1), SENTINEL, dtype=x.dtype, device=x.device)
    live(buf, x.shape[1], g).copy_(x)
    return buf, live(buf, x.shape[1], g)


def fence_intact(buf, L, g, before):
    """Everything of `buf` outside the live view still holds what it held before the call."""
    chk = buf.clone()
    live(chk, L, g).copy_(live(before, L, g))
    return torch.equal(bits(chk), bits(before))


def attn_desc(q, k, v, o, mask, lse, lse_stride, drop):
    d = ops._attn_desc(B, H, q.shape[1], k.shape[1], aa.DH, q, k, v, o, mask, None, 1.0 / 8, False, lse, lse_stride, ops.BF16)
    ops._set_dropout(d, drop)
    return d


def contiguous_call(Lq, Lk, masked, drop):
    q, k, v, do = (aa.randn_bf16(B, L, D, seed=700 + i).cuda() for i, L in enumerate((Lq, Lk, Lk, Lq)))
    mask = aa.tail_key_mask(B, Lk).cuda() if masked else None
    o, lse = ops.attn_forward(q, k, v, H, mask, dropout=drop)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ops.attn_backward(q, k, v, o, lse, do, dq, dk, dv, H, mask, dropout=drop)
    return (q, k, v, do, mask), (o, lse, dq, dk, dv)


D_SHAPES = [(33, 65), (100, 45), (128, 128), (577, 577)]


@pytest.mark.parametrize("drop", [None, (0.1, DROP_SEED)], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("shape", D_SHAPES, ids=ids)
def test_outputs_as_strided_views_leave_their_neighbours_alone(shape, drop):
    Lq, Lk = shape
    (q, k, v, do, mask), (o0, lse0, dq0, dk0, dv0) = contiguous_call(Lq, Lk, True, drop)
    (_, qs), (_, ks), (_, vs), (_, dos) = fenced(q, "q"), fenced(k, "k"), fenced(v, "v"), fenced(do, "o")
    out = {n: fenced(torch.full_like(t, SENTINEL), g) for n, t, g in (("o", o0, "o"), ("dq", q, "q"), ("dk", k, "k"), ("dv", v, "v"))}
    stride = (Lq + 31) // 32 * 32
    lse = torch.full((B, H, stride + 32), SENTINEL, device="cuda")   # the call's table is the first B H stride entries of this
    lse_call = lse.view(-1)[:B * H * stride].view(B, H, stride)
    before = {n: b.clone() for n, (b, _) in out.items()}
    ops.check(_lib.lib().m3ae_attn_fwd(C.byref(attn_desc(qs, ks, vs, out["o"][1], mask, lse_call, stride, drop)), ops._stream()), "m3ae_attn_fwd")
    ops.attn_backward(qs, ks, vs, out["o"][1], lse_call, dos, out["dq"][1], out["dk"][1], out["dv"][1], H, mask, dropout=drop)
    torch.cuda.synchronize()
    for n, base, g in (("o", o0, "o"), ("dq", dq0, "q"), ("dk", dk0, "k"), ("dv", dv0, "v")):
        assert fence_intact(out[n][0], base.shape[1], g, before[n]), f"{n}: a store outside the [L, H*64] view"
        assert torch.equal(bits(out[n][1]), bits(base)), f"{n}: differs from the contiguous call"
    assert torch.equal(bits(lse_call[..., :Lq]), bits(lse0[..., :Lq]))
    assert bool((lse.view(-1)[B * H * stride:] == SENTINEL).all()), "a store past the log-sum-exp table"


@pytest.mark.parametrize("legacy", [False, True], ids=["gen4", "legacy"])
@pytest.mark.parametrize("drop", [None, (0.1, DROP_SEED)], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("shape", D_SHAPES, ids=ids)
def test_log_sum_exp_table_wider_than_the_padded_query_count(shape, drop, legacy):
    """include/m3ae_hip.h: lse is [B, H, lse_stride] with any lse_stride >= Lq that is a multiple of 32 (delta has its layout).
    With 32 spare rows per (b, h), pre-filled with NaN, every output equals the tight-table call's bits, and the padding rows
    Lq .. ceil32(Lq) - 1, which the backward tiles read, come out finite."""
    Lq, Lk = shape
    try:
        ops.ATTN_LEGACY = legacy
        (q, k, v, do, mask), (o0, lse0, dq0, dk0, dv0) = contiguous_call(Lq, Lk, True, drop)
        tight = (Lq + 31) // 32 * 32
        stride = tight + 32
        lse, delta = (torch.full((B, H, stride), float("nan"), device="cuda") for _ in range(2))
        o, dq, dk, dv = (torch.full_like(t, SENTINEL) for t in (q, q, k, v))
        d = attn_desc(q, k, v, o, mask, lse, stride, drop)
        ops.check(_lib.lib().m3ae_attn_fwd(C.byref(d), ops._stream()), "m3ae_attn_fwd")
        d.d_o, d.dq, d.dk, d.dv, d.delta = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
        ops.check(_lib.lib().m3ae_attn_bwd(C.byref(d), ops._stream()), "m3ae_attn_bwd")
        torch.cuda.synchronize()
    finally:
        ops.ATTN_LEGACY = False
    assert torch.equal(bits(lse[..., :Lq]), bits(lse0[..., :Lq]))
    assert bool(torch.isfinite(lse[..., :tight]).all()) and bool(torch.isfinite(delta[..., :tight]).all())
    for n, got, base in (("o", o, o0), ("dq", dq, dq0), ("dk", dk, dk0), ("dv", dv, dv0)):
        assert torch.equal(bits(got), bits(base)), f"{n}: differs from the tight-table call"
