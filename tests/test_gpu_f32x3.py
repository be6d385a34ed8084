"""GPU: the fp32x3 GEMM (csrc/gemm_f32x3.hip, m3ae_gemm_desc.launch_flags & M3AE_GEMM_F32_X3) and the fp32 attention with
M3AE_ATTN_F32_X3, through the C ABI (ops.gemm / ops.attn_* inside ops.f32x3_mode), against float64 references.

Error bound of one GEMM entry, before the epilogue (the constant c is derived in tests/test_f32x3_host.py, which also checks
it on adversarial inputs with a bit-exact numpy model of the split):
    |C - C64| <= c (2^-16 + K 2^-23) (|A||B|)_mn,   c = 3
  * split: x = hi + lo + r with |x - hi| <= 2^-8 |x| and |r| <= 2^-8 |x - hi| <= 2^-16 |x|; a b - (hi hi + hi lo + lo hi) =
    lo_a lo_b + r_a b + hi_a r_b  ->  at most (2^-16 + 2^-16 + (1 + 2^-8) 2^-16) |a b| < 3 * 2^-16 |a b|;
  * accumulation: 3K fp32 additions (three MFMAs per k into one accumulator), each rounding at most 2^-24 of the running
    sum |.| <= sum |a b|: 3K 2^-24 = 1.5 K 2^-23 < 3 K 2^-23.
The epilogue adds its own fp32 roundings (alpha, bias, residual, accumulate: 2^-24 of each operand; the activations: a few
ulp), and an activation scales the pre-activation error by at most max|act'| (<= 1.13 for GELU / QuickGELU / ReLU).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, ops  # noqa: E402

C_BOUND = 3.0
U = 2.0 ** -24


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def qgelu64(x):
    return x * torch.sigmoid(1.702 * x)


def dqgelu64(x):
    s = torch.sigmoid(1.702 * x)
    return s * (1.0 + 1.702 * x * (1.0 - s))


ACTS = {ops.ACT_NONE: (lambda x: x, lambda x: torch.ones_like(x)), ops.ACT_GELU: (gelu64, dgelu64),
        ops.ACT_QUICKGELU: (qgelu64, dqgelu64), ops.ACT_RELU: (torch.relu, lambda x: (x > 0).double())}


def bf16_round64(t):
    return t.to(torch.bfloat16).double()


# layouts: (A's strides, B's strides) as functions of M, N, K; A is stored as `a_store` and B as `b_store` (shapes)
def operands(layout, M, N, K, seed):
    """Returns (a_storage, a_sm, a_sk, b_storage, b_sk, b_sn, A64 [M,K], B64 [K,N])."""
    if layout == "NT":     # forward: x [M, K] . W[N, K]^T
        a, b = rnd(M, K, seed=seed), rnd(N, K, seed=seed + 1, scale=K ** -0.5)
        return a, K, 1, b, 1, K, a.double(), b.double().t()
    if layout == "NN":     # dgrad: dy [M, K] . W [K, N]
        a, b = rnd(M, K, seed=seed), rnd(K, N, seed=seed + 1, scale=K ** -0.5)
        return a, K, 1, b, N, 1, a.double(), b.double()
    if layout == "TN":     # wgrad: dy^T [M, K] (dy stored [K, M]) . x [K, N]
        a, b = rnd(K, M, seed=seed), rnd(K, N, seed=seed + 1)
        return a, 1, M, b, N, 1, a.double().t(), b.double()
    raise ValueError(layout)


def run_gemm(a, a_sm, a_sk, b, b_sk, b_sn, c, M, N, K, **kw):
    with ops.f32x3_mode(True):
        ops.gemm(a, a_sm, a_sk, b, b_sk, b_sn, c, c.stride(-2), M, N, K, **kw)
    torch.cuda.synchronize()
    return ops.last_gemm_path()


def prod_bound(A64, B64):
    K = A64.shape[-1]
    return C_BOUND * (2.0 ** -16 + K * 2.0 ** -23) * (A64.abs() @ B64.abs())


SHAPES = [("NT", 1, 1, 1), ("NT", 17, 17, 17), ("NT", 577, 498, 1000), ("NT", 1000, 2304, 768), ("NT", 1, 498, 1536),
          ("NN", 498, 577, 17), ("NN", 1154, 768, 3072), ("NN", 17, 1000, 577),
          ("TN", 768, 768, 18464), ("TN", 498, 1536, 1000), ("TN", 17, 1, 577)]


@pytest.mark.parametrize("layout,M,N,K", SHAPES)
def test_f32x3_gemm_layouts_against_float64(layout, M, N, K):
    a, a_sm, a_sk, b, b_sk, b_sn, A64, B64 = operands(layout, M, N, K, seed=M + N + K)
    c = torch.empty(M, N, device="cuda")
    assert run_gemm(a, a_sm, a_sk, b, b_sk, b_sn, c, M, N, K) == "f32x3"
    ref = A64 @ B64
    err = (c.double() - ref).abs()
    bound = prod_bound(A64, B64)
    assert bool((err <= bound).all()), f"max err / bound {(err / bound).max().item():.3f}"
    if M * N >= 64:   # (a handful of entries can come out of bf16 rounding nearly exact by chance)
        err_bf16 = (bf16_round64(A64) @ bf16_round64(B64) - ref).abs().max().item()
        assert 30.0 * err.max().item() <= err_bf16, (err.max().item(), err_bf16)


def test_f32x3_batched_strided_attention_shapes():
    """The per-head products of the fp32 attention: [B, L, H*Dh] operands addressed in place, batch (B, H)."""
    Bt, H, L, Dh = 2, 3, 577, 64
    q, k = rnd(Bt, L, 3 * H * Dh, seed=7), rnd(Bt, L, 3 * H * Dh, seed=8)
    c = torch.empty(Bt, H, L, L, device="cuda")
    with ops.f32x3_mode(True):   # S = Q K^T (NT) and O = S V (NN, V rows strided)
        ops.gemm(q, 3 * H * Dh, 1, k[..., H * Dh:], 1, 3 * H * Dh, c, L, L, L, Dh, batch=(Bt, H),
                 a_sb=(L * 3 * H * Dh, Dh), b_sb=(L * 3 * H * Dh, Dh), c_sb=(H * L * L, L * L), alpha=0.125)
    assert ops.last_gemm_path() == "f32x3"
    qh = q[..., :H * Dh].double().view(Bt, L, H, Dh).permute(0, 2, 1, 3)
    kh = k[..., H * Dh:2 * H * Dh].double().view(Bt, L, H, Dh).permute(0, 2, 1, 3)
    ref = 0.125 * qh @ kh.transpose(-1, -2)
    bound = 0.125 * prod_bound(qh, kh.transpose(-1, -2)) + U * ref.abs()
    assert bool(((c.double() - ref).abs() <= bound).all())
    o = torch.empty(Bt, L, H * Dh, device="cuda")
    v = k[..., 2 * H * Dh:]
    with ops.f32x3_mode(True):
        ops.gemm(c, L, 1, v, 3 * H * Dh, 1, o, H * Dh, L, Dh, L, batch=(Bt, H), a_sb=(H * L * L, L * L), b_sb=(L * 3 * H * Dh, Dh),
                 c_sb=(L * H * Dh, Dh))
    assert ops.last_gemm_path() == "f32x3"
    vh = v.double().view(Bt, L, H, Dh).permute(0, 2, 1, 3)
    ref_o = (c.double() @ vh).permute(0, 2, 1, 3)
    bound_o = prod_bound(c.double(), vh).permute(0, 2, 1, 3)
    assert bool(((o.double().view(Bt, L, H, Dh) - ref_o).abs() <= bound_o).all())


@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_GELU, ops.ACT_QUICKGELU, ops.ACT_RELU])
@pytest.mark.parametrize("preact_grad", [False, True])
@pytest.mark.parametrize("layout,M,N,K", [("NT", 577, 498, 768), ("NN", 130, 1000, 3072), ("TN", 17, 768, 4616)])
def test_f32x3_epilogues(act, preact_grad, layout, M, N, K):
    """alpha, bias, activation with the pre-activation (or act'(pre)) stored, residual, accumulate -- against float64."""
    a, a_sm, a_sk, b, b_sk, b_sn, A64, B64 = operands(layout, M, N, K, seed=K)
    bias, res, c0 = rnd(N, seed=1), rnd(M, N, seed=2), rnd(M, N, seed=3)
    c, pre = c0.clone(), torch.empty(M, N, device="cuda")
    alpha = 0.37
    assert run_gemm(a, a_sm, a_sk, b, b_sk, b_sn, c, M, N, K, alpha=alpha, bias=bias, act=act, preact=pre,
                    preact_grad=preact_grad, residual=res, accumulate=True) == "f32x3"
    f, df = ACTS[act]
    p64 = alpha * (A64 @ B64) + bias.double()
    e_pre = alpha * prod_bound(A64, B64) + 2 * U * (p64.abs() + bias.double().abs())
    ref = f(p64) + res.double() + c0.double()
    e_out = 1.13 * e_pre + 8 * U * (p64.abs() + res.double().abs() + c0.double().abs())
    assert bool(((c.double() - ref).abs() <= e_out).all()), f"out: {((c.double() - ref).abs() / e_out).max().item():.3f}"
    ref_pre = df(p64) if preact_grad else p64
    if preact_grad and act == ops.ACT_RELU:   # a step: compare away from the kink
        keep = p64.abs() > e_pre
        assert bool((pre.double()[keep] == ref_pre[keep]).all())
    else:
        # act'(x) is evaluated in fp32 as a sum of terms of size up to 1 + |x| (cdf + x pdf): a few ulp of that, absolutely
        tol = (1.13 if preact_grad else 1.0) * e_pre + 8 * U * ref_pre.abs() + (16 * U * (1 + p64.abs()) if preact_grad else 0)
        assert bool(((pre.double() - ref_pre).abs() <= tol).all())


@pytest.mark.parametrize("dact", [ops.ACT_GELU, ops.ACT_MULAUX])
def test_f32x3_dact_aux_and_a_rowsum(dact):
    """dgrad with the activation derivative fused (dact_aux), and wgrad with the bias gradient fused (a_rowsum over fp32 A)."""
    M, N, K = 1154, 768, 3072
    a, a_sm, a_sk, b, b_sk, b_sn, A64, B64 = operands("NN", M, N, K, seed=11)
    aux = rnd(M, N, seed=12)
    c = torch.empty(M, N, device="cuda")
    assert run_gemm(a, a_sm, a_sk, b, b_sk, b_sn, c, M, N, K, dact_aux=aux, dact=dact) == "f32x3"
    d = dgelu64(aux.double()) if dact == ops.ACT_GELU else aux.double()
    ref = (A64 @ B64) * d
    bound = prod_bound(A64, B64) * d.abs() + 8 * U * ref.abs()
    if dact == ops.ACT_GELU:   # act'(aux) in fp32: a few ulp of its terms (cdf + aux pdf, up to 1 + |aux|), not of the result
        bound = bound + 16 * U * (1 + aux.double().abs()) * (A64 @ B64).abs()
    assert bool(((c.double() - ref).abs() <= bound).all()), ((c.double() - ref).abs() / bound).max().item()
    # wgrad: dW [768, 498] += dy^T x, db += rowsum(dy^T), K = 9232 rows
    M, N, K = 768, 498, 9232
    a, a_sm, a_sk, b, b_sk, b_sn, A64, B64 = operands("TN", M, N, K, seed=13)
    c0, rs0 = rnd(M, N, seed=14), rnd(M, seed=15)
    c, rs = c0.clone(), rs0.clone()
    assert run_gemm(a, a_sm, a_sk, b, b_sk, b_sn, c, M, N, K, accumulate=True, a_rowsum=rs) == "f32x3"
    ref = A64 @ B64 + c0.double()
    assert bool(((c.double() - ref).abs() <= prod_bound(A64, B64) + 2 * U * ref.abs()).all())
    ref_rs = A64.sum(1) + rs0.double()
    bound_rs = K * 2.0 ** -23 * A64.abs().sum(1) + 2 * U * rs0.double().abs()
    assert bool(((rs.double() - ref_rs).abs() <= bound_rs).all())


@pytest.mark.parametrize("layout,M,N,K", [("NT", 577, 498, 768), ("NN", 33, 130, 64)])
def test_f32x3_dropout_mask_equals_the_generic_kernels(layout, M, N, K):
    a, a_sm, a_sk, b, b_sk, b_sn, A64, B64 = operands(layout, M, N, K, seed=21)
    bias = rnd(N, seed=22)
    y3, yg = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    drop = (0.1, 0x5EED0001)
    assert run_gemm(a, a_sm, a_sk, b, b_sk, b_sn, y3, M, N, K, bias=bias, act=ops.ACT_GELU, dropout=drop) == "f32x3"
    ops.gemm(a, a_sm, a_sk, b, b_sk, b_sn, yg, N, M, N, K, bias=bias, act=ops.ACT_GELU, dropout=drop, force_generic=True)
    assert ops.last_gemm_path() == "generic"
    keep = ops.dropout_keep_mask(M, N, *drop).bool()
    assert torch.equal(y3 != 0, yg != 0)
    p64 = A64 @ B64 + bias.double()
    sel = p64.abs() < 4   # (fp32 GELU is exactly 0 below about -5.9: erff saturates)
    assert torch.equal((y3 != 0)[sel], keep[sel])
    ref = gelu64(p64) / 0.9 * keep.double()
    e = 1.13 / 0.9 * prod_bound(A64, B64) + 16 * U * (ref.abs() + bias.double().abs())
    assert bool(((y3.double() - ref).abs() <= e).all())


def test_f32x3_bit_is_refused_for_bf16_and_force_generic_wins():
    M, N, K = 64, 64, 64
    a, b = rnd(M, K, seed=1).bfloat16(), rnd(N, K, seed=2).bfloat16()
    c = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    with ops.f32x3_mode(True), pytest.raises(_lib.M3AEHipError):
        d = _lib.GemmDesc()
        d.M, d.N, d.K, d.batch1, d.batch2 = M, N, K, 1, 1
        d.A, d.a_sm, d.a_sk, d.B, d.b_sk, d.b_sn, d.C, d.c_sm, d.c_sn = a.data_ptr(), K, 1, b.data_ptr(), 1, K, c.data_ptr(), N, 1
        d.dtype_a = d.dtype_b = d.dtype_c = _lib.BF16
        d.alpha = 1.0
        d.launch_flags = _lib.GEMM_F32_X3
        _lib.check(_lib.lib().m3ae_gemm(_lib.C.byref(d), None), "m3ae_gemm")
    a32, b32, c32 = a.float(), b.float(), c.float()
    with ops.f32x3_mode(True):
        ops.gemm(a32, K, 1, b32, 1, K, c32, N, M, N, K, force_generic=True)
    assert ops.last_gemm_path() == "generic"
    with ops.f32x3_mode(True):
        ops.gemm(a, K, 1, b, 1, K, c, N, M, N, K)   # bf16 operands: ops never sets the bit for them
    assert ops.last_gemm_path().startswith("mfma")


# ---------------------------------------------------------------------------------------------------------------------
# fp32 attention with M3AE_ATTN_F32_X3
# ---------------------------------------------------------------------------------------------------------------------
def _attn64(q, k, v, H, mask, bias, causal, keep, p, scale):
    B, Lq, D = q.shape
    Lk, dh = k.shape[1], D // H
    sh = lambda t, L: t.view(B, L, H, dh).permute(0, 2, 1, 3)
    s = scale * sh(q, Lq) @ sh(k, Lk).transpose(-1, -2)
    if mask is not None:
        s = s + mask.double()[:, None, None, :]
    if bias is not None:
        s = s + bias[None]
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(Lq, Lk, dtype=torch.bool, device=q.device)), float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep / (1 - p)
    return (pr @ sh(v, Lk)).permute(0, 2, 1, 3).reshape(B, Lq, D), pr


@pytest.mark.parametrize("case", ["mask", "pos_bias", "causal", "dropout", "cross"])
def test_f32x3_attention_fwd_bwd_probs_against_float64(case):
    B, H, dh = 2, 3, 64
    Lq, Lk = (577, 577) if case != "cross" else (40, 577)
    D = H * dh
    q, k, v = rnd(B, Lq, D, seed=31), rnd(B, Lk, D, seed=32), rnd(B, Lk, D, seed=33)
    do = rnd(B, Lq, D, seed=34)
    mask = bias = None
    causal = case == "causal"
    p, seed = (0.1, 0xA77E) if case == "dropout" else (0.0, 0)
    if case in ("mask", "dropout", "cross"):
        mask = torch.zeros(B, Lk, device="cuda")
        mask[1, Lk // 2:] = -10000.0
    scale = 1.0 / math.sqrt(dh)
    if case == "pos_bias":
        bias, scale = (0.5 * rnd(H, Lq, Lk, seed=35)).contiguous(), 1.0
    drop = (p, seed) if p > 0 else None
    keep = ops.dropout_keep_mask(B * H * Lq, Lk, p, seed).double().view(B, H, Lq, Lk) if drop else None
    outs = {}
    for x3 in (True, False):
        with ops.f32x3_mode(x3):
            o, lse = ops.attn_forward(q, k, v, H, mask, bias, scale=scale, causal=causal, dropout=drop)
            dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            dbias = torch.zeros_like(bias) if bias is not None else None
            ops.attn_backward(q, k, v, o, lse, do, dq, dk, dv, H, mask, bias, scale=scale, causal=causal, d_pos_bias=dbias,
                              dropout=drop)
            probs = ops.attn_probs(q, k, lse, H, mask, scale=scale, dropout=drop) if bias is None and not causal else None
        torch.cuda.synchronize()
        outs[x3] = (o, dq, dk, dv, dbias, probs)
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    br = bias.double().requires_grad_(True) if bias is not None else None
    oref, pref = _attn64(qr, kr, vr, H, mask, br, causal, keep, p, scale)
    oref.backward(do.double())
    o, dq, dk, dv, dbias, probs = outs[True]
    checks = [("o", o, oref), ("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)]
    if bias is not None:
        checks.append(("d_pos_bias", dbias, br.grad))
    if probs is not None:
        checks.append(("probs", probs, pref))
    # the parity-mode attention tolerance (rtol 1e-4 of the largest entry): a score error of 3 (2^-16 + 64 2^-23) sum|q k| scale
    # moves P by that much relatively; a bf16-operand product would be ~2^-9
    bad = []
    for name, got, ref in checks:
        err = (got.double() - ref.detach()).abs().max().item()
        scale_ref = ref.detach().abs().max().item()
        if err > 1e-4 * scale_ref + 1e-7:
            bad.append(f"{name}: max err {err:.3e} (|ref| max {scale_ref:.3e})")
    assert not bad, bad
    # the bit took the products off the generic fp32 kernel: the outputs differ from parity mode's in the last bits
    assert not torch.equal(outs[True][0], outs[False][0])
    assert not torch.equal(outs[True][1], outs[False][1])
