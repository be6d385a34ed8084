"""GPU: parity mode (compute_dtype="fp32") held to float64 -- gemm_generic_kernel (csrc/gemm_generic.hip) on fp32 and mixed operands,
and the materialised-softmax attention of csrc/attention.hip -- by the yardsticks of tests/parity_accuracy.py (derivations there;
tests/test_parity_accuracy_host.py checks the yardsticks on models of the kernels and on their mutants).

  A1  exact tier: every layout, tile-straddling shape, epilogue, C geometry, batch stride pattern, a_rowsum; bit for bit, fenced.
  A2  ascending k, bit for bit on non-integer data: the header's "fp32 FMA accumulation in ascending k: deterministic".
  A3  bound tier: full-precision operands, element-wise bound + rms / max budgets against the sequential model.
  A4  contracts: grid limits, dtype_a != dtype_b, a_rowsum with a batch.
  B1  probabilities read exactly (V = I, dO = I), element by element, relative bound.
  B2  o, dq, dk, dv, d_pos_bias within the budget over the sequential fp32 model; packed layouts, fences, d_pos_bias adds.
  B3  the bf16 detour for Dh != 64.      B4  the workspace contract.

Figures are printed as PARITY_ACCURACY <form>: ... under pytest -s (for the record, not criteria: DESIGN.md section 4)."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, ops  # noqa: E402

import attn_accuracy as aa  # noqa: E402
import gemm_accuracy as ga  # noqa: E402
import parity_accuracy as pa  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
UNSUPPORTED, WORKSPACE = -2, -4   # include/m3ae_hip.h


# ------------------------------------------------------------------------------------------------------------------------
# one call of the generic kernel on views
# ------------------------------------------------------------------------------------------------------------------------
def call_gemm(a, b, c, *, abi=False, alpha=1.0, bias=None, act=ga.ACT_NONE, preact=None, preact_grad=False, residual=None, dact_aux=None,
              dact=ga.ACT_NONE, accumulate=False, dropout=None, rows=None, a_rowsum=None):
    """C = epi(alpha a . b) for views a [.., M, K], b [.., K, N], c [.., M, N] (2-D, or 4-D with the two batch levels in front); every
    stride is the view's own.  Through ops.gemm where it can express the call (c_sn == 1), else (or with abi) through a
    m3ae_gemm_desc of its own.  Returns the status; a status of 0 must have run the generic kernel."""
    (M, K), N = a.shape[-2:], b.shape[-1]
    batch = tuple(c.shape[:2]) if c.dim() == 4 else (1, 1)
    sb = lambda t: (t.stride(0), t.stride(1)) if t.dim() == 4 else (0, 0)
    for t in (preact, residual, dact_aux):
        assert t is None or (t.stride() == c.stride() and t.dtype == c.dtype)
    if c.stride(-1) == 1 and not abi:
        ops.gemm(a, a.stride(-2), a.stride(-1), b, b.stride(-2), b.stride(-1), c, c.stride(-2), M, N, K, alpha=alpha, accumulate=accumulate,
                 bias=bias, act=act, preact=preact, residual=residual, dact_aux=dact_aux, dact=dact, force_generic=a.dtype == BF, batch=batch,
                 a_sb=sb(a), b_sb=sb(b), c_sb=sb(c), a_rowsum=a_rowsum, dropout=dropout, preact_grad=preact_grad, rows=rows)
        rc = 0
    else:
        d = _lib.GemmDesc()
        d.M, d.N, d.K, (d.batch1, d.batch2) = M, N, K, batch
        d.A, d.a_sm, d.a_sk, (d.a_sb1, d.a_sb2) = a.data_ptr(), a.stride(-2), a.stride(-1), sb(a)
        d.B, d.b_sk, d.b_sn, (d.b_sb1, d.b_sb2) = b.data_ptr(), b.stride(-2), b.stride(-1), sb(b)
        d.C, d.c_sm, d.c_sn, (d.c_sb1, d.c_sb2) = c.data_ptr(), c.stride(-2), c.stride(-1), sb(c)
        dt = lambda t: _lib.BF16 if t.dtype == BF else _lib.F32
        d.dtype_a, d.dtype_b, d.dtype_c = dt(a), dt(b), dt(c)
        d.alpha, d.accumulate, d.act, d.dact, d.preact_grad = alpha, int(accumulate), act, dact, int(preact_grad)
        d.force_generic = int(a.dtype == BF)
        for name, t in (("bias", bias), ("preact", preact), ("residual", residual), ("dact_aux", dact_aux), ("a_rowsum", a_rowsum)):
            if t is not None:
                setattr(d, name, t.data_ptr())
        ops._set_dropout(d, dropout)
        rows = rows or (0, 1)
        rc = _lib.lib().m3ae_gemm_rows(C.byref(d), rows[0], rows[1], ops._stream())
    torch.cuda.synchronize()
    if rc == 0:
        assert ops.last_gemm_path() == "generic", ops.last_gemm_path()
    return rc


def fenced_out(shape, geometry="dense", dtype=F32):
    """A fenced output for a [.., M, N] result (batch levels in front): (buffer, view, fence shape).  dense: c_sm = N; ldc: c_sm = N + 5;
    transposed: c_sm = 1, c_sn = M + 3; heads: [b1, M, b2 * N] addressed in place (the per-head products of the attention)."""
    *bt, M, N = shape
    nb = math.prod(bt)
    if geometry == "transposed":
        buf, v = ga.fenced((nb * N, M), M + 3, dtype, DEV)
        return buf, v.view(*bt, N, M).transpose(-1, -2), (nb * N, M)
    if geometry == "heads":
        b1, b2 = bt
        buf, v = ga.fenced((b1 * M, b2 * N), b2 * N + 8, dtype, DEV)
        return buf, v.view(b1, M, b2, N).permute(0, 2, 1, 3), (b1 * M, b2 * N)
    buf, v = ga.fenced((nb * M, N), N + (5 if geometry == "ldc" else 0), dtype, DEV)
    return buf, v.view(*bt, M, N), (nb * M, N)


def run_epilogue(a, b, kw, geometry, seed, rows=None, abi=False):
    """One call for gemm_accuracy.reference keywords `kw`: every [M, N] operand and output in a fenced buffer of the geometry.
    Returns (c, preact, check_fences)."""
    shape = a.shape[:-2] + (a.shape[-2], b.shape[-1])
    fences = []

    def out(init=None):
        buf, v, fs = fenced_out(shape, geometry)
        fences.append((buf, fs))
        if init is not None:
            v.copy_(init.to(DEV))
        return v
    c = out(kw.get("c_old"))
    pre = out() if kw.get("want_preact") else None
    like = lambda t: None if t is None else out(t)
    dev = lambda t: None if t is None else t.to(DEV)
    rc = call_gemm(a, b, c, abi=abi, alpha=kw.get("alpha", 1.0), bias=dev(kw.get("bias")), act=kw.get("act", ga.ACT_NONE), preact=pre,
                   preact_grad=kw.get("preact_grad", False), residual=like(kw.get("residual")), dact_aux=like(kw.get("dact_aux")),
                   dact=kw.get("dact", ga.ACT_NONE), accumulate=kw.get("c_old") is not None,
                   dropout=(kw["p"], seed) if kw.get("keep") is not None else None, rows=rows)
    assert rc == 0, rc

    def check_fences(msg):
        for buf, fs in fences:
            ga.assert_fence_intact(buf, fs, msg)
    return c, pre, check_fences


def assert_bits(got, want, msg):
    bad = got.double() != want.to(got.device)
    assert not bad.any(), f"{msg}: not the exact result, " + ga.first_bad(bad.reshape(-1, bad.shape[-1]))


def mapped_keep(rows, cols, p, seed, row_map):
    base, step = row_map
    return ops.dropout_keep_mask(base + (rows - 1) * step + 1, cols, p, seed)[base::step]


# ------------------------------------------------------------------------------------------------------------------------
# A1. exact tier
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pa.EXACT_SHAPES, ids=str)
def test_a1_exact_every_layout_epilogue_and_c_geometry(shape):
    M, N, K = shape
    seed = pa.seed_of(shape)
    o = ga.exact_operands(M, N, K, seed, DEV)
    keeps = {False: ops.dropout_keep_mask(M, N, 0.5, seed), True: mapped_keep(M, N, 0.5, seed, pa.ROW_MAP)}
    A, B = o["a"].float(), o["b"].float().t()
    refs = {}
    for name in ga.EXACT_EPILOGUES + pa.EXACT_EXTRA_EPILOGUES:
        kw = pa.exact_epilogue(name, o, keeps[name.endswith("@rows")], lambda t: t.float())
        refs[name] = (kw, ga.reference(o["a"], o["b"], **kw))
    for layout in pa.LAYOUTS:
        a, b = pa.views(layout, A, B)
        for geometry in ("dense", "ldc", "transposed"):
            for name, (kw, ref) in refs.items():
                c, pre, check_fences = run_epilogue(a, b, kw, geometry, seed, rows=pa.ROW_MAP if name.endswith("@rows") else None)
                msg = f"{shape} {layout} {geometry} {name}"
                assert_bits(c, ref.c, msg + " C")
                if pre is not None:
                    assert_bits(pre, ref.preact, msg + " preact")
                check_fences(msg)
    # <bf16, bf16, float>: bf16 operands into an fp32 C, beyond the NT layout
    for layout in ("NT", "NN", "TN", "TT"):
        a, b = pa.views(layout, A.to(BF), B.to(BF))
        for name in ("plain", "bias+res", "alpha0.5+acc"):
            kw, ref = refs[name]
            c, _, check_fences = run_epilogue(a, b, kw, "ldc", seed)
            assert_bits(c, ref.c, f"{shape} bf16 operands {layout} {name}")
            check_fences(f"{shape} bf16 operands {layout} {name}")


def test_a1_exact_two_level_batch_strides():
    b1, b2 = pa.BATCH
    M, N, K = 33, 17, 72
    o = ga.exact_operands(b1 * b2 * M, b1 * b2 * N, K, 4242, DEV)
    A4 = o["a"].float().view(b1, b2, M, K)
    B4 = o["b"].float().view(b1, b2, N, K).transpose(-1, -2)
    ref = pa.batched_reference(A4, B4)
    assert not torch.equal(ref, pa.batched_reference(A4, B4, swapped=True))

    def run(a, b, want, geometry, msg, alpha=1.0):
        buf, c, fs = fenced_out((b1, b2, M, N), geometry)
        assert call_gemm(a, b, c, alpha=alpha) == 0
        assert_bits(c, want * alpha, msg)
        ga.assert_fence_intact(buf, fs, msg)

    # distinct strides per level, the levels stored in the other order (a_sb1 < a_sb2)
    a_swapped = A4.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)
    assert a_swapped.stride(0) < a_swapped.stride(1)
    for layout in ("NT", "NN", "TN", "S2"):
        a, b = pa.views(layout, A4, B4)
        run(a_swapped if layout in ("NT", "NN") else a, b, ref, "dense", f"batch, levels stored swapped, {layout}", alpha=0.5)
    # a zero stride on B: one weight shared by every batch
    shared = B4[1, 2].contiguous()
    run(A4.contiguous(), shared.expand(b1, b2, K, N), A4.double() @ shared.double(), "dense", "batch, shared B")
    # the per-head products of the attention: B and C are [b1, L, b2 * N] tensors addressed in place
    vbuf = torch.full((b1, K, b2 * N + 8), ga.FENCE, device=DEV)
    v = vbuf[..., :b2 * N].view(b1, K, b2, N).permute(0, 2, 1, 3)
    v.copy_(B4)
    run(A4.contiguous(), v, ref, "heads", "batch, heads interleaved in B and C")
    run(pa.views("TN", A4, B4)[0], v, ref, "heads", "batch, heads interleaved, A reduction-strided")


@pytest.mark.parametrize("shape", pa.ROWSUM_SHAPES, ids=str)
def test_a1_exact_a_rowsum_adds_once_per_row(shape):
    M, N, K = shape
    o = ga.exact_operands(M, N, K, pa.seed_of(shape) + 1, DEV)
    prior = (torch.arange(M, device=DEV) % 17 - 8).float()
    want_rs = prior.double() + o["a"].sum(1)
    ref = ga.reference(o["a"], o["b"], c_old=o["c_old"].float())
    for dtype in (F32, BF):
        for layout in ("NT", "TN", "S2"):
            a, b = pa.views(layout, o["a"].to(dtype), o["b"].to(dtype).t())
            rbuf, rv = ga.fenced((1, M), M + 5, F32, DEV)
            rv[0].copy_(prior)
            cbuf, c, fs = fenced_out((M, N), "ldc")
            c.copy_(o["c_old"])
            assert call_gemm(a, b, c, accumulate=True, a_rowsum=rv[0]) == 0
            msg = f"{shape} {layout} {dtype} a_rowsum"
            assert_bits(rv, want_rs[None], msg)
            assert_bits(c, ref.c, msg + " C")
            ga.assert_fence_intact(rbuf, (1, M), msg)
            ga.assert_fence_intact(cbuf, fs, msg + " C")


# ------------------------------------------------------------------------------------------------------------------------
# A2. ascending k, bit for bit
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pa.ASCENDING_CASES, ids=str)
def test_a2_ascending_k_bit_for_bit(shape):
    M, N, K = shape
    a, b = pa.twelve_bit_operands(M, N, K, pa.seed_of(shape))
    want = pa.seq_gemm(a, b.t())
    if K > 2:
        assert not torch.equal(want, pa.seq_gemm(a, b.t(), "descending"))   # the data tells the orders apart
    for layout in ("NT", "TN"):
        av, bv = pa.views(layout, a.to(DEV), b.t().to(DEV))
        buf, c, fs = fenced_out((M, N), "ldc")
        assert call_gemm(av, bv, c) == 0
        bad = c.cpu() != want
        assert not bad.any(), f"{shape} {layout}: not the ascending-k fp32 FMA chain, " + ga.first_bad(bad)
        ga.assert_fence_intact(buf, fs, f"{shape} {layout}")


def test_a2_three_term_probe_sums_in_ascending_order():
    a, b = pa.probe_operands(DEV)
    for layout in ("NT", "TN"):
        av, bv = pa.views(layout, a, b.t())
        buf, c, fs = fenced_out((a.shape[0], b.shape[0]), "ldc")
        assert call_gemm(av, bv, c) == 0
        assert bool((c == 0).all()), f"{layout}: (2^24 + 1) - 2^24 must come out as 0, got {c.flatten()[0].item()}"
        ga.assert_fence_intact(buf, fs, layout)


# ------------------------------------------------------------------------------------------------------------------------
# A3. bound tier
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pa.BOUND_SHAPES, ids=str)
def test_a3_bound_and_budgets_against_float64(shape):
    M, N, K = shape
    seed = pa.seed_of(shape)
    o = pa.bound_operands(M, N, K, seed)
    acc = pa.seq_gemm(o["a"], o["b"].t())
    A, B = o["a"].float().to(DEV), o["b"].float().t().to(DEV)
    figures, misses = {}, []
    for i, name in enumerate(pa.BOUND_CLASSES):
        kw = pa.bound_class(name, o)
        ref = ga.reference(o["a"], o["b"], **kw)
        model_c, model_pre = pa.epilogue32(acc, **kw)
        a, b = pa.views(("NT", "TN", "NN")[i % 3], A, B)
        c, pre, check_fences = run_epilogue(a, b, kw, "ldc", seed)
        check_fences(f"{shape} {name}")
        misses += [f"{shape} {name}: {m}" for m in pa.gemm_criteria(c, pre, model_c, model_pre, ref, figures)]
        if name == "relu+deriv":
            share = pa.kink_share(ref)
            figures["kink share"] = share
            assert share < pa.KINK_SHARE, f"{shape}: {share:.2e} of the ReLU-step comparison left out"
    print(f"PARITY_ACCURACY gemm {shape}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(figures.items())))
    assert not misses, "\n".join(misses)


# ------------------------------------------------------------------------------------------------------------------------
# A4. contracts (statuses only: none of these may launch)
# ------------------------------------------------------------------------------------------------------------------------
def tiny_desc(M=4, N=4, K=4, batch=(1, 1), dtype_a=None, dtype_b=None):
    """A descriptor on tiny real buffers with every stride 0: whatever M, N and the batch say, no address leaves the buffers."""
    keep = [torch.zeros(64, device=DEV) for _ in range(4)]
    d = _lib.GemmDesc()
    d.M, d.N, d.K, (d.batch1, d.batch2) = M, N, K, batch
    d.A, d.B, d.C = (t.data_ptr() for t in keep[:3])
    d.dtype_a, d.dtype_b, d.dtype_c = dtype_a or _lib.F32, dtype_b or _lib.F32, _lib.F32
    d.alpha = 1.0
    return d, keep


def status(d):
    rc = _lib.lib().m3ae_gemm(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    return rc


def test_a4_grid_limits_are_refused_without_a_launch():
    d, keep = tiny_desc(M=65536 * 64 + 1)           # grid.y = 65537
    assert status(d) == UNSUPPORTED
    d, keep = tiny_desc(batch=(256, 257))            # grid.z = 65792
    assert status(d) == UNSUPPORTED
    assert all(bool((t == 0).all()) for t in keep)


def test_a4_mixed_operand_dtypes_are_refused():
    d, keep = tiny_desc(dtype_a=_lib.F32, dtype_b=_lib.BF16)
    assert status(d) == UNSUPPORTED
    d, keep = tiny_desc(dtype_a=_lib.BF16, dtype_b=_lib.F32)
    assert status(d) == UNSUPPORTED


def test_a4_a_rowsum_with_a_batch_is_refused():
    """a_rowsum has no batch stride: every batch would add into the same rows.  The library refuses, not only the Python wrapper."""
    for batch in ((2, 1), (1, 3), (2, 3)):
        d, keep = tiny_desc(batch=batch)
        d.a_rowsum = keep[3].data_ptr()
        assert status(d) == UNSUPPORTED, batch
        assert bool((keep[3] == 0).all()) and bool((keep[2] == 0).all()), batch
    d, keep = tiny_desc()
    d.a_sk = d.b_sk = 1
    keep[0][:4] = 1.0
    d.a_rowsum = keep[3].data_ptr()
    assert status(d) == 0 and ops.last_gemm_path() == "generic"
    assert keep[3][:4].tolist() == [4.0] * 4 and bool((keep[3][4:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------
# B. fp32 attention
# ------------------------------------------------------------------------------------------------------------------------
B_, H_ = 2, 3
dev = lambda t: None if t is None else t.to(DEV)


def forward_probs(c, v, drop=None, rows=None):
    """o of ops.attn_forward on V = I per head, as [B, H, Lq, Lk] on the CPU, and the lse table."""
    o, lse = ops.attn_forward(dev(c["q"]), dev(c["k"]), dev(v), c["H"], dev(c["key_mask"]), dev(c["pos_bias"]), scale=c["scale"],
                              causal=c["causal"], dropout=drop, rows=rows)
    torch.cuda.synchronize()
    return aa.split(o.cpu(), c["H"]), lse


@pytest.mark.parametrize("Lq,Lk", pa.PROBE_SHAPES, ids=str)
def test_b1_probabilities_element_by_element(Lq, Lk):
    R = B_ * H_ * Lq
    worst = {}
    for i, variant in enumerate(pa.PROBE_VARIANTS):
        c = pa.probe_case(B_, H_, Lq, Lk, variant, 7000 + 31 * Lq + Lk + i)
        drop, rows, keep = None, None, None
        if variant.startswith("dropout"):
            drop = (pa.PROBE_P, 0xB1 + Lk)
            rows = pa.ROW_MAP if variant == "dropout_rows" else None
            keep = (mapped_keep(R, Lk, *drop, rows) if rows else ops.dropout_keep_mask(R, Lk, *drop)).view(B_, H_, Lq, Lk).cpu()
        P64, rel = pa.probs_bound(c["q"], c["k"], c["H"], c["key_mask"], c["pos_bias"], c["causal"], c["scale"], drop=drop is not None)
        if variant == "all_masked_row":   # finite, and the softmax of the row's unmasked scores
            plain = pa.probs_bound(c["q"], c["k"], c["H"], None, None, False, c["scale"])[0]
            assert torch.allclose(P64[0], plain[0], rtol=1e-9, atol=0)
        if variant == "causal":
            assert bool((P64[..., ~aa._visible(Lq, Lk)] == 0).all())
        got, lse = forward_probs(c, pa.identity_v(B_, H_, Lk), drop, rows)
        miss = pa.check_probs(got, P64, rel, keep, pa.PROBE_P, name=f"{Lq}x{Lk} {variant} o")
        assert miss is None, miss
        worst[variant] = pa.worst_ratio(got, P64, rel, keep, pa.PROBE_P)
        if c["pos_bias"] is None and not c["causal"] and rows is None:
            probs = ops.attn_probs(dev(c["q"]), dev(c["k"]), lse, c["H"], dev(c["key_mask"]), scale=c["scale"], dropout=drop)
            assert torch.equal(probs.cpu().view(torch.int32), got.contiguous().view(torch.int32)), f"{Lq}x{Lk} {variant}: attn_probs differs from o"
    print(f"PARITY_ACCURACY probs {Lq}x{Lk}: worst err / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("Lq,Lk", [(5, 65), (33, 129), (3, 2)], ids=str)
def test_b1_backward_probabilities_through_dv(Lq, Lk):
    """Dh = Lq and dO = I per head: dv[b, j, h Lq + c] = P[b, h, c, j], every product exact."""
    R = B_ * H_ * Lq
    for i, variant in enumerate(("plain", "tail_mask", "bias1", "causal", "dropout")):
        c = pa.probe_case(B_, H_, Lq, Lk, variant, 7500 + 31 * Lq + Lk + i)
        g = torch.Generator().manual_seed(i)
        D = H_ * Lq
        q, k, v = torch.randn(B_, Lq, D, generator=g), torch.randn(B_, Lk, D, generator=g), torch.randn(B_, Lk, D, generator=g)
        scale = 1.0 / math.sqrt(Lq)
        drop, keep = None, None
        if variant == "dropout":
            drop = (pa.PROBE_P, 0xB2 + Lk)
            keep = ops.dropout_keep_mask(R, Lk, *drop).view(B_, H_, Lq, Lk).cpu()
        P64, rel = pa.probs_bound(q, k, H_, c["key_mask"], c["pos_bias"], c["causal"], scale, drop=drop is not None)
        qd, kd, vd, do = dev(q), dev(k), dev(v), dev(pa.identity_v(B_, H_, Lq))
        mask, bias = dev(c["key_mask"]), dev(c["pos_bias"])
        o, lse = ops.attn_forward(qd, kd, vd, H_, mask, bias, scale=scale, causal=c["causal"], dropout=drop)
        dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
        dpb = torch.zeros_like(bias) if bias is not None else None
        ops.attn_backward(qd, kd, vd, o, lse, do, dq, dk, dv, H_, mask, bias, scale=scale, causal=c["causal"], d_pos_bias=dpb, dropout=drop)
        torch.cuda.synchronize()
        got = aa.split(dv.cpu(), H_).transpose(-1, -2)
        miss = pa.check_probs(got, P64, rel, keep, pa.PROBE_P, name=f"{Lq}x{Lk} {variant} dv")
        assert miss is None, miss


def run_attention(case):
    """Forward and backward of one parity_accuracy.make_case on the GPU, the gradients into fenced packed buffers, d_pos_bias onto its
    prior contents: (Result on the CPU, gradient buffers)."""
    H, D = case["H"], case["H"] * case["Dh"]
    bufs = tuple(b.to(DEV) for b in case["bufs"])
    q, k, v = pa.packed_views(bufs, D)
    mask, bias = dev(case["key_mask"]), dev(case["pos_bias"])
    drop = (case["p"], case["drop_seed"]) if case["p"] > 0 else None
    o, lse = ops.attn_forward(q, k, v, H, mask, bias, scale=case["scale"], causal=case["causal"], dropout=drop)
    gbufs, (dq, dk, dv) = pa.grad_views(case, DEV)
    dpb = case["dpb_prior"].to(DEV).clone() if bias is not None else None
    ops.attn_backward(q, k, v, o, lse, dev(case["do"]), dq, dk, dv, H, mask, bias, scale=case["scale"], causal=case["causal"], d_pos_bias=dpb,
                      dropout=drop)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu()
    return aa.Result(cpu(o), cpu(dq), cpu(dk), cpu(dv), cpu(dpb), None), gbufs


def with_keep(case, Lq, Lk):
    if case["p"] > 0:
        case["keep"] = ops.dropout_keep_mask(B_ * case["H"] * Lq, Lk, case["p"], case["drop_seed"]).view(B_, case["H"], Lq, Lk).cpu()
    return case


def report_budget(label, figures):
    print(f"PARITY_ACCURACY attention {label}: " + ", ".join(
        f"{n} rms ratio {max(f[0] / f[1] if f[1] else 0.0 for f in fs):.2f} max ratio {max(f[2] / f[3] if f[3] else 0.0 for f in fs):.2f}"
        for n, fs in figures.items()))


@pytest.mark.parametrize("label,Lq,Lk,Dh,kw", pa.budget_cases(), ids=[c[0] for c in pa.budget_cases()])
def test_b2_budget_over_the_sequential_model(label, Lq, Lk, Dh, kw):
    case = with_keep(pa.make_case(B_, H_, Lq, Lk, Dh, 8000 + Lq + 3 * Lk + Dh, **kw), Lq, Lk)
    _, ref = pa.attn_reference(case)
    model = pa.seq_attention(**pa.model_args(case), dpb_prior=case["dpb_prior"])
    got, gbufs = run_attention(case)
    figures = {}
    misses = pa.budget_misses(got, model, ref, figures)
    report_budget(label, figures)
    assert not misses, f"{label}: " + "; ".join(misses)
    assert pa.grads_fence_intact(gbufs), f"{label}: wrote outside the dq / dk / dv views of the packed buffers"
    for t, n in zip(pa.packed_views(gbufs, H_ * Dh), ("dq", "dk", "dv")):
        assert bool(torch.isfinite(t).all()), n
    if case["causal"] and case["pos_bias"] is not None:   # nothing reaches d_pos_bias above the diagonal: the prior contents, bit for bit
        above = ~aa._visible(Lq, Lk)
        assert torch.equal(got.d_pos_bias[:, above], case["dpb_prior"][:, above])


def test_b3_bf16_detour_for_head_width_96():
    """ops.attn_forward / attn_backward on bf16 tensors with Dh = 96, causal + bias (the decoder head's use): the fp32 kernels on
    fp32 copies, one bf16 rounding of each output."""
    Lq, Lk, Dh = 33, 65, 96
    case = pa.make_case(B_, H_, Lq, Lk, Dh, 9001, bias=True, causal=True, dtype=BF)
    _, ref = pa.attn_reference(case)
    model = pa.seq_attention(**pa.model_args(case), dpb_prior=case["dpb_prior"])
    got, gbufs = run_attention(case)
    assert got.o.dtype == BF and got.dq.dtype == BF
    worst = {}
    for n in aa.NAMES:
        err = (getattr(got, n).double() - getattr(ref, n).double()).abs()
        bnd = pa.detour_bound(ref, model, n)
        worst[n] = (err / bnd).max().item()
        assert bool((err <= bnd).all()), f"{n}: worst err / bound {worst[n]:.3f}"
    assert pa.grads_fence_intact(gbufs)
    print("PARITY_ACCURACY detour d96: worst err / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    # the detour's backward = a direct fp32 call on the same values, bit for bit before the final cast
    q, k, v = (dev(case[n]).float() for n in ("q", "k", "v"))
    o32, lse = ops.attn_forward(q, k, v, H_, None, dev(case["pos_bias"]), scale=case["scale"], causal=True)
    assert torch.equal(o32.to(BF).cpu().view(torch.int16), got.o.view(torch.int16))
    g = [torch.empty_like(t) for t in (q, k, v)]
    dpb = dev(case["dpb_prior"]).clone()
    ops.attn_backward(q, k, v, dev(got.o).float(), lse, dev(case["do"]).float(), *g, H_, None, dev(case["pos_bias"]), scale=case["scale"], causal=True,
                      d_pos_bias=dpb)
    torch.cuda.synchronize()
    for n, t in zip(("dq", "dk", "dv"), g):
        assert torch.equal(t.to(BF).cpu().view(torch.int16), getattr(got, n).contiguous().view(torch.int16)), n
    assert torch.equal(dpb.cpu().view(torch.int32), got.d_pos_bias.view(torch.int32))


def test_b4_workspace_one_byte_short_is_refused():
    Lq, Lk, Dh = 5, 7, 8
    D = H_ * Dh
    q, k, v, o = (torch.zeros(B_, L, D, device=DEV) for L in (Lq, Lk, Lk, Lq))
    lse = torch.zeros(B_, H_, 32, device=DEV)
    for backward in (False, True):
        d = ops._attn_desc(B_, H_, Lq, Lk, Dh, q, k, v, o, None, None, 1.0, False, lse, 32, _lib.F32)
        need = _lib.lib().m3ae_attn_workspace_bytes(C.byref(d), int(backward))
        assert need == (2 if backward else 1) * B_ * H_ * Lq * Lk * 4
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        grads = [torch.zeros_like(t) for t in (o, q, k, v)]
        d.d_o, d.dq, d.dk, d.dv, d.delta = (t.data_ptr() for t in grads + [lse])
        d.workspace, d.workspace_bytes = ws.data_ptr(), need - 1
        fn = _lib.lib().m3ae_attn_bwd if backward else _lib.lib().m3ae_attn_fwd
        assert fn(C.byref(d), ops._stream()) == WORKSPACE
        d.workspace_bytes = need
        assert fn(C.byref(d), ops._stream()) == 0
        torch.cuda.synchronize()
