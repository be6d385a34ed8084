"""GPU: the bf16 MFMA GEMMs (NT forward / dgrad kernels with their fused epilogues, TN wgrad kernels, the generic kernel on bf16
operands) against float64, by the yardsticks of tests/gemm_accuracy.py (derivations there; tests/test_gemm_accuracy_host.py checks the
yardsticks on a model of the kernels and on its mutants).

  A  exact tier, NT: integer-valued operands, every fp32 value of the kernel exact, the output known bit for bit; every output in a
     fenced buffer; every kernel variant at the shapes where its code paths differ (ragged tiles, both ring phases, persistent grids
     with fewer and more tiles than workgroups, the streaming store policy, strided operands and outputs).
  B  exact tier, TN (split-K atomics and their ordered form give the same bits: every sum is exact) and the generic kernel.
  C  bound tier: random operands, every epilogue class of launch_nt, element-wise bound + signed-error + rms budgets.
  D  contracts: bit-identical kernel variants; a descriptor that misses one NT precondition runs the generic kernel, exactly.

References are float64 on the GPU.  Worst figures observed (for the record, not criteria): DESIGN.md section 4."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import ops  # noqa: E402

import gemm_accuracy as ga  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


@contextlib.contextmanager
def pinned(nt=-1, tn=-1, policy=0, deterministic=False):
    old = ops.GEMM_NT_VARIANT, ops.GEMM_TN_VARIANT, ops.GEMM_ST_POLICY, ops.deterministic()
    ops.GEMM_NT_VARIANT, ops.GEMM_TN_VARIANT, ops.GEMM_ST_POLICY = nt, tn, policy
    ops.set_deterministic(deterministic)
    try:
        yield
    finally:
        ops.GEMM_NT_VARIANT, ops.GEMM_TN_VARIANT, ops.GEMM_ST_POLICY = old[:3]
        ops.set_deterministic(old[3])


def cdiv(a, b):
    return -(-a // b)


def expected_nt_path(M, N, K, ldc, variant):
    """nt_kernel_choice's rules (csrc/gemm_mfma.hip)."""
    rows_epi = N % 8 == 0 and ldc % 8 == 0
    both = M > 128 and N > 128
    t256, t128 = cdiv(M, 256) * cdiv(N, 256), cdiv(M, 128) * cdiv(N, 128)
    if variant < 0:
        eff256, eff128 = t256 / (cdiv(t256, 256) * 256), t128 / (cdiv(t128, 512) * 512)
        big = both and eff256 >= 0.93 * eff128
        if big and rows_epi and K >= 256:
            return "mfma_nt_pp2"
        return "mfma_nt_pp" if big else "mfma_nt"
    if variant in (9, 10) and both and rows_epi and K >= 256:
        return "mfma_nt_pp2"
    if variant == 7 and both:
        return "mfma_nt_pp"
    return "mfma_nt"


def storage(c_bf16):
    dt = BF if c_bf16 else F32
    return dt, (lambda t: t.to(dt))


def run_gemm(a, b, kw, c_bf16, ldc=None, seed=0, bias_off=0):
    """One ops.gemm call for reference() keywords `kw` on K-contiguous operands a [M, K], b [N, K] (any row strides).  The outputs are
    fenced; preact / residual / dact_aux share C's row stride.  Returns (c, preact, check_fences)."""
    (M, K), N = a.shape, b.shape[0]
    dt, _ = storage(c_bf16)
    ldc = ldc or N
    cbuf, c = ga.fenced((M, N), ldc, dt, DEV)
    if kw.get("c_old") is not None:
        c.copy_(kw["c_old"])
    pbuf, pre = ga.fenced((M, N), ldc, dt, DEV) if kw.get("want_preact") else (None, None)
    at_ld = lambda t: None if t is None else (t if t.stride(0) == ldc else ga.strided(t, ldc))
    bias = kw.get("bias")
    if bias is not None and bias_off:
        bias = torch.cat([bias.new_zeros(bias_off), bias])[bias_off:]   # the same values at a pointer 4 * bias_off bytes off 16
        assert bias.data_ptr() % 16 != 0
    ops.gemm(a, a.stride(0), 1, b, 1, b.stride(0), c, ldc, M, N, K, alpha=kw.get("alpha", 1.0), accumulate=kw.get("c_old") is not None,
             bias=bias, act=kw.get("act", ga.ACT_NONE), preact=pre, residual=at_ld(kw.get("residual")), dact_aux=at_ld(kw.get("dact_aux")),
             dact=kw.get("dact", ga.ACT_NONE), dropout=(kw["p"], seed) if kw.get("keep") is not None else None,
             preact_grad=kw.get("preact_grad", False))

    def check_fences(msg):
        ga.assert_fence_intact(cbuf, (M, N), msg + " C")
        if pbuf is not None:
            ga.assert_fence_intact(pbuf, (M, N), msg + " preact")
    return c, pre, check_fences


def label(what, variant, extra=""):
    return f"{what}: path {ops.last_gemm_path()}, variant {variant}{extra}"


def assert_exact(got, want, c_bf16, msg):
    want = ga.expected_store(want, c_bf16)
    bad = got.double() != want
    assert not bad.any(), f"{msg}: not the exact result, " + ga.first_bad(bad)


def exact_nt(shape, variant, policy=0, lda=None, ldb=None, ldc=None, bias_off=0, path=None, epilogues=ga.EXACT_EPILOGUES):
    M, N, K = shape
    seed = 77 + M + N + K
    o = ga.exact_operands(M, N, K, seed, DEV)
    keep = ops.dropout_keep_mask(M, N, 0.5, seed)
    a, b = ga.strided(o["a"].to(BF), lda or K), ga.strided(o["b"].to(BF), ldb or K)
    path = path or expected_nt_path(M, N, K, ldc or N, variant)
    with pinned(nt=variant, policy=policy):
        for c_bf16 in (True, False):
            _, cast = storage(c_bf16)
            for name in epilogues:
                kw = ga.exact_epilogue(name, o, keep, cast)
                ref = ga.reference(o["a"], o["b"], **kw)
                c, pre, check_fences = run_gemm(a, b, kw, c_bf16, ldc, seed, bias_off)
                msg = label(f"{shape} {name} {'bf16' if c_bf16 else 'fp32'} C", variant, f", store policy {policy}")
                assert ops.last_gemm_path() == path, f"{msg}: expected {path}"
                assert_exact(c, ref.c, c_bf16, msg + " C")
                if pre is not None:
                    assert_exact(pre, ref.preact, c_bf16, msg + " preact")
                check_fences(msg)


# ------------------------------------------------------------------------------------------------------------------------
# A. exact tier, NT
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,variant", [(s, v) for s, vs in ga.NT_EXACT_CASES for v in vs], ids=str)
def test_nt_exact(shape, variant):
    M, N, K = shape
    if (M, N) == (5125, 3336):
        assert M * N >= 16 << 20 and cdiv(M, 256) * cdiv(N, 256) == 294   # by-size streaming stores; more tiles than one round of CUs
    if (M, N) == (43557, 520):
        assert cdiv(M, 256) * cdiv(N, 256) == 513                          # more than 512 tiles: two full rounds of one workgroup per CU
    exact_nt(shape, variant)


@pytest.mark.parametrize("policy", [1, 3])
@pytest.mark.parametrize("variant", [0, 7, 9])
def test_nt_exact_pinned_store_policy(variant, policy):
    exact_nt((300, 264, 256), variant, policy=policy)


@pytest.mark.parametrize("variant", [0, 4, 7, 9, 10, -1])
def test_nt_exact_strided_operands_and_outputs(variant):
    """lda > K, ldb > K, ldc > N (mm_dgrad(out=, ld_out=) and the CLS-row calls): the padding of every operand holds the fence value."""
    M, N, K = 300, 264, 256
    exact_nt((M, N, K), variant, lda=K + 8, ldb=K + 16, ldc=N + 8)


# ------------------------------------------------------------------------------------------------------------------------
# B. exact tier, TN (wgrad) and the generic kernel
# ------------------------------------------------------------------------------------------------------------------------
def run_tn(dy, x, c_old, alpha, accumulate, rs_old, ldc):
    """C[M, N] (+)= alpha dy[K, M]^T x[K, N], a_rowsum += column sums of dy; C fenced at row stride ldc."""
    (K, M), N = dy.shape, x.shape[1]
    cbuf, c = ga.fenced((M, N), ldc, F32, DEV)
    c.copy_(c_old)
    rs = rs_old.clone()
    ops.gemm(dy, 1, dy.stride(0), x, x.stride(0), 1, c, ldc, M, N, K, accumulate=accumulate, alpha=alpha, a_rowsum=rs)
    return cbuf, c, rs


@pytest.mark.parametrize("shape,variant", [(s, v) for s, vs in ga.TN_EXACT_CASES for v in vs], ids=str)
def test_tn_exact(shape, variant):
    M, N, K = shape
    o = ga.exact_operands(M, N, K, 99 + K, DEV)
    dy, x = o["a"].t().contiguous().to(BF), o["b"].t().contiguous().to(BF)
    rs_old = (torch.arange(M, device=DEV) % 17 - 8).float()
    rs_want = rs_old.double() + o["a"].sum(1)
    if variant == 5:
        # the split rule of the 256 x 256 kernel (launch_tn_pp, accumulating call): one workgroup per CU, 8 and more 64-row steps per split
        assert M % 256 == 0 and N % 256 == 0 and K >= 4096 and K % 64 != 0   # several splits, ragged last chunk
        ksteps = cdiv(K, 64)
        steps_per = cdiv(ksteps, max(1, min(256 // ((M // 256) * (N // 256)), ksteps // 8)))
        splits = cdiv(ksteps, steps_per)
        assert splits >= 8 and cdiv(K - (splits - 1) * steps_per * 64, 32) == ga.TN_PP_TAIL_CHUNKS[shape]
    for det in (False, True):
        with pinned(tn=variant, deterministic=det):
            for accumulate in (True, False):
                for alpha in (0.5, 1.0):
                    for ldc in (N, N + 8):
                        kw = dict(alpha=alpha, **({"c_old": o["c_old"].float()} if accumulate else {}))
                        ref = ga.reference(o["a"], o["b"], **kw)
                        cbuf, c, rs = run_tn(dy, x, o["c_old"].float(), alpha, accumulate, rs_old, ldc)
                        msg = label(f"{shape} accumulate {accumulate} alpha {alpha} ldc {ldc} deterministic {det}", variant)
                        assert ops.last_gemm_path() == "mfma_tn", msg
                        assert_exact(c, ref.c, False, msg + " C")
                        assert_exact(rs[None], rs_want[None], False, msg + " a_rowsum")
                        ga.assert_fence_intact(cbuf, (M, N), msg)


@pytest.mark.parametrize("shape", ga.GENERIC_EXACT_SHAPES, ids=str)
def test_generic_exact_bf16_operands(shape):
    exact_nt(shape, -1, path="generic", epilogues=("plain", "bias+res"))


# ------------------------------------------------------------------------------------------------------------------------
# C. bound tier
# ------------------------------------------------------------------------------------------------------------------------
def report(kind, shape, variant, path, figures):
    print(f"GEMM_ACCURACY {kind} {shape} variant {variant} path {path}: " +
          ", ".join(f"{k} {v:.3g}" for k, v in sorted(figures.items())))


@pytest.mark.parametrize("shape,variant", [(s, v) for s, vs in ga.BOUND_CASES for v in vs], ids=str)
def test_nt_bound(shape, variant):
    M, N, K = shape
    seed = 177 + M + N + K
    o = ga.bound_operands(M, N, K, seed, DEV)
    keep = ops.dropout_keep_mask(M, N, ga.DROP_P, seed)
    assert 0.85 < keep.float().mean().item() < 0.95
    a, b = o["a"].to(BF), o["b"].to(BF)
    path = expected_nt_path(M, N, K, N, variant)
    figures, misses = {}, []
    with pinned(nt=variant):
        for c_bf16 in (True, False):
            _, cast = storage(c_bf16)
            for name in ga.BOUND_CLASSES:
                kw = ga.bound_class(name, o, keep, cast)
                ref = ga.reference(o["a"], o["b"], **kw)
                c, pre, check_fences = run_gemm(a, b, kw, c_bf16, None, seed)
                msg = label(f"{shape} {name} {'bf16' if c_bf16 else 'fp32'} C", variant)
                assert ops.last_gemm_path() == path, f"{msg}: expected {path}"
                check_fences(msg)
                misses += [f"{msg}: {m}" for m in ga.criteria(c, pre, ref, c_bf16, figures=figures)]
    report("nt", shape, variant, path, figures)
    assert not misses, "\n".join(misses)


@pytest.mark.parametrize("shape,variant", [(s, v) for s, vs in ga.TN_BOUND_CASES for v in vs], ids=str)
def test_tn_bound(shape, variant):
    M, N, K = shape
    o = ga.bound_operands(M, N, K, 277 + K, DEV)
    dy, x = o["a"].t().contiguous().to(BF), o["b"].t().contiguous().to(BF)
    rs_old = torch.zeros(M, device=DEV)
    rs_ref = ga.reference(o["a"], torch.ones(1, K, dtype=torch.float64, device=DEV), c_old=rs_old[:, None])
    figures, misses = {}, []
    for det in (False, True):
        with pinned(tn=variant, deterministic=det):
            for accumulate in (True, False):
                kw = dict(alpha=0.5, **({"c_old": o["c_old"].float()} if accumulate else {}))
                ref = ga.reference(o["a"], o["b"], **kw)
                cbuf, c, rs = run_tn(dy, x, o["c_old"].float(), 0.5, accumulate, rs_old, N)
                msg = label(f"{shape} accumulate {accumulate} deterministic {det}", variant)
                assert ops.last_gemm_path() == "mfma_tn", msg
                misses += [f"{msg}: {m}" for m in ga.criteria(c, None, ref, False, tn=True, figures=figures)]
                misses += [f"{msg} a_rowsum: {m}" for m in [ga.check_bound(rs[:, None], rs_ref.c, ga.bound(rs_ref, False, tn=True)[0])] if m]
    report("tn", shape, variant, "mfma_tn", figures)
    assert not misses, "\n".join(misses)


# ------------------------------------------------------------------------------------------------------------------------
# D. contracts
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gelu+deriv", "dgelu+res"])
def test_nt_variants_agree_bit_for_bit(name):
    M, N, K = 300, 264, 256
    o = ga.bound_operands(M, N, K, 377, DEV)
    a, b = o["a"].to(BF), o["b"].to(BF)
    for c_bf16 in (True, False):
        word, (_, cast) = (torch.int16 if c_bf16 else torch.int32), storage(c_bf16)
        kw = ga.bound_class(name, o, None, cast)
        first = None
        for variant in (0, 4, 7, 9, 10):
            with pinned(nt=variant):
                c, pre, _ = run_gemm(a, b, kw, c_bf16)
                assert ops.last_gemm_path() == expected_nt_path(M, N, K, N, variant)
            got = [t.contiguous().view(word) for t in (c, pre) if t is not None]
            if first is None:
                first = got
            for t0, t in zip(first, got):
                bad = t0 != t
                assert not bad.any(), label(f"{name} differs from variant 0", variant, ", " + (ga.first_bad(bad) if bad.any() else ""))


@pytest.mark.parametrize("miss", ["K % 64", "ldc % 4", "bias pointer"])
def test_missed_nt_precondition_runs_the_generic_kernel_exactly(miss):
    M, N, K = 300, 264, 200 if miss == "K % 64" else 256
    exact_nt((M, N, K), -1, ldc=N + 2 if miss == "ldc % 4" else None, bias_off=1 if miss == "bias pointer" else 0, path="generic",
             epilogues=("bias+res", "bias+relu+pre+drop+res") if miss == "bias pointer" else ga.EXACT_EPILOGUES)
