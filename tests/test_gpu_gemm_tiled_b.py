"""GPU: the tiled weight operand of the NT GEMMs (M3AE_GEMM_B_TILED, csrc/tiled_b.h).

  1  m3ae_tile_bf16_batched against the Python mirror of the index function, bit for bit (padding rows zero, nothing else written)
  2  m3ae_gemm with the tiled B against the same call with the row-major B: identical bits in C and in the second output, on the
     256 x 256 ping-pong kernel (both launch forms), the 128 x 128 kernel and the generic kernel, over the epilogue classes
  3  dgrad through the tiled transposed copy
  4  the refusals: M3AE_ERR_UNSUPPORTED before any launch
  5  one ClipBlockFn forward + backward with the switch on and off; ParamStore keeps the copies current

Which kernel a shape takes is the library's routing rule, unchanged: the MFMA NT kernels need K % 64 == 0, so K = 96 and K = 288
run the generic kernel (with either B); the test pins what it expects of every shape through ops.last_gemm_path().
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, ops, synth, tiled_b as tb  # noqa: E402
from m3ae_amd.modules.clip_model import ResidualAttentionBlock  # noqa: E402
from m3ae_amd.param_store import ParamStore  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
FENCE = 0x7FC1          # a bf16 NaN pattern no kernel produces
STORE_CFG = dict(learning_rate=1e-3, weight_decay=0.01, lr_multiplier_head=1, lr_multiplier_multi_modal=1)


@pytest.fixture(autouse=True)
def _restore_switches():
    old = ops.TILED_B, ops.GEMM_NT_VARIANT, ops.deterministic()
    yield
    ops.TILED_B, ops.GEMM_NT_VARIANT = old[0], old[1]
    ops.set_deterministic(old[2])


def rnd(*shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def fenced(n):
    """n bf16 elements between two 64-element fences; returns (buffer, view)."""
    buf = torch.full((n + 128,), FENCE, dtype=torch.int16, device=DEV).view(BF)
    return buf, buf[64:64 + n]


def fences_intact(buf, n):
    raw = buf.view(torch.int16)
    return bool((raw[:64] == FENCE).all()) and bool((raw[64 + n:] == FENCE).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the tiling kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _unit(N, K, seed):
    """A unit in[N][K] with every output the shapes allow, in fenced buffers."""
    w = rnd(N, K, seed=seed)
    out = dict(fwd=fenced(tb.tiled_rows(N) * K), t=fenced(N * K), tt=fenced(tb.tiled_rows(K) * N) if N % 32 == 0 else None)
    return w, out


def _check_unit(w, out):
    N, K = w.shape
    buf, v = out["fwd"]
    assert torch.equal(bits(v), bits(tb.tile_reference(w))), "tiled copy"            # padding rows included: zeros
    assert fences_intact(buf, v.numel())
    buf, v = out["t"]
    assert torch.equal(bits(v.view(K, N)), bits(w.t().contiguous())), "row-major transpose"
    assert fences_intact(buf, v.numel())
    if out["tt"] is not None:
        buf, v = out["tt"]
        assert torch.equal(bits(v), bits(tb.tile_reference(w.t().contiguous()))), "tiled copy of the transpose"
        assert fences_intact(buf, v.numel())


@pytest.mark.parametrize("K", [64, 96, 288])
@pytest.mark.parametrize("N", [128, 200, 384])
def test_tiling_kernel_equals_the_index_function(N, K):
    w, out = _unit(N, K, seed=N + K)
    jobs, n, tiles = tb.job_table([(w, out["fwd"][1], out["t"][1], None if out["tt"] is None else out["tt"][1])], DEV)
    tb.run(jobs, n, tiles)
    torch.cuda.synchronize()
    _check_unit(w, out)
    # the forward copy alone (no transposed outputs: the kernel's early exit), padding rows again written
    buf, v = fenced(tb.tiled_rows(N) * K)
    jobs, n, tiles = tb.job_table([(w, v, None, None)], DEV)
    tb.run(jobs, n, tiles)
    torch.cuda.synchronize()
    assert torch.equal(bits(v), bits(tb.tile_reference(w))) and fences_intact(buf, v.numel())


def test_tiling_kernel_two_jobs_in_one_call():
    (w0, o0), (w1, o1) = _unit(200, 96, seed=5), _unit(384, 288, seed=6)
    jobs, n, tiles = tb.job_table([(w0, o0["fwd"][1], o0["t"][1], None), (w1, o1["fwd"][1], o1["t"][1], o1["tt"][1])], DEV)
    assert n == 2 and tiles == tb.job_tiles(200, 96, True, False) + tb.job_tiles(384, 288, True, True)
    tb.run(jobs, n, tiles)
    torch.cuda.synchronize()
    _check_unit(w0, o0)
    _check_unit(w1, o1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. m3ae_gemm: tiled B against row-major B
# ---------------------------------------------------------------------------------------------------------------------------------
def _classes(M, N):
    b, aux = rnd(N, seed=31, dtype=F32), rnd(M, N, seed=32)
    return [("plain+bias", dict(bias=b), False),
            ("gelu+deriv", dict(bias=b, act=ops.ACT_GELU, preact_grad=True), True),
            ("qgelu+pre", dict(bias=b, act=ops.ACT_QUICKGELU), True),
            ("bias+res+drop", dict(bias=b, residual=aux, dropout=(0.1, 1234)), False),
            ("dmul", dict(dact_aux=aux, dact=ops.ACT_MULAUX), False),
            ("dgelu", dict(dact_aux=aux, dact=ops.ACT_GELU), False),
            ("dqgelu", dict(dact_aux=aux, dact=ops.ACT_QUICKGELU), False)]


def _tiled_against_row_major(M, N, K, variants, path):
    x = rnd(M, K, seed=1)
    w = rnd(N, K, seed=2, scale=K ** -0.5)
    wt = tb.tile_reference(w)                     # built by the index function: independent of the tiling kernel
    for name, kw, second in _classes(M, N):
        for v in variants:
            ops.GEMM_NT_VARIANT = v
            res = []
            for tiled in (False, True):
                ybuf, y = fenced(M * N)
                pbuf, pre = fenced(M * N)
                ops.gemm(x, K, 1, wt if tiled else w, 1, K, y.view(M, N), N, M, N, K, b_tiled=tiled,
                         preact=pre.view(M, N) if second else None, **kw)
                assert ops.last_gemm_path() == path, (name, v, tiled, ops.last_gemm_path())
                torch.cuda.synchronize()
                assert fences_intact(ybuf, M * N) and fences_intact(pbuf, M * N), (name, v, tiled)
                res.append((y, pre))
            msg = f"({M}, {N}, {K}) {name} variant {v}"
            assert not bool((bits(res[0][0]) == FENCE).all()), msg
            assert torch.equal(bits(res[0][0]), bits(res[1][0])), msg + ": C"
            assert torch.equal(bits(res[0][1]), bits(res[1][1])), msg + ": second output"   # (all fence when the class has none)


@pytest.mark.parametrize("K", [256, 288])
@pytest.mark.parametrize("N", [384, 512])
@pytest.mark.parametrize("M", [300, 512])
def test_gemm_tiled_b_256_tile_shapes(M, N, K):
    """Variants 9 / 10: the ping-pong kernel launched one workgroup per tile / persistent.  K = 288 is no multiple of 64: the
    routing rule sends it to the generic kernel, which reads the tiled copy through the index function."""
    _tiled_against_row_major(M, N, K, (9, 10), "mfma_nt_pp2" if K % 64 == 0 else "generic")


@pytest.mark.parametrize("kind", ["plain+bias", "bias+res+drop", "gelu+deriv"])
def test_gemm_tiled_b_persistent_form_walks_several_tiles(kind):
    """More tiles than compute units (44 x 7 = 308 > 256, ragged in M and N): the persistent workgroups re-point B per tile and
    prefetch the next tile's weight chunks under the epilogue."""
    M, N, K = 43 * 256 + 37, 6 * 256 + 72, 256
    x, w = rnd(M, K, seed=3), rnd(N, K, seed=4, scale=K ** -0.5)
    wt = tb.tile_reference(w)
    name, kw, second = [c for c in _classes(M, N) if c[0] == kind][0]
    outs = []
    for v, tiled in ((9, False), (10, False), (10, True), (9, True)):
        ops.GEMM_NT_VARIANT = v
        y = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
        pre = torch.full((M, N), float("nan"), dtype=BF, device=DEV) if second else None
        ops.gemm(x, K, 1, wt if tiled else w, 1, K, y, N, M, N, K, b_tiled=tiled, preact=pre, **kw)
        assert ops.last_gemm_path() == "mfma_nt_pp2"
        outs.append((y, pre))
    for y, pre in outs[1:]:
        assert torch.equal(bits(y), bits(outs[0][0]))
        assert pre is None or torch.equal(bits(pre), bits(outs[0][1]))
    assert bool(torch.isfinite(outs[0][0].float()).all())


@pytest.mark.parametrize("K", [64, 96])
@pytest.mark.parametrize("N", [128, 320])
def test_gemm_tiled_b_128_tile_shapes(N, K):
    """By shape (-1) and pinned (0): the 128 x 128 kernel; K = 96 is no multiple of 64 and runs the generic kernel."""
    _tiled_against_row_major(200, N, K, (-1, 0), "mfma_nt" if K % 64 == 0 else "generic")


@pytest.mark.parametrize("variant,shape", [(4, (300, 384, 256)), (7, (300, 384, 256)), (7, (64 * 256 + 11, 8 * 256 + 40, 128))],
                         ids=["4", "7", "7-585tiles"])
def test_gemm_tiled_b_on_the_other_256_tile_kernels(variant, shape):
    """The kernels a selector (or a shape the second-generation kernel does not take) can still reach: 2-stage (4) and first-generation
    ping-pong (7); the latter also at a short reduction with more than 512 tiles (65 x 9, four chunks, ragged in M and N)."""
    M, N, K = shape
    x, w = rnd(M, K, seed=7), rnd(N, K, seed=8, scale=K ** -0.5)
    wt, b, aux = tb.tile_reference(w), rnd(N, seed=9, dtype=F32), rnd(M, N, seed=10)
    ops.GEMM_NT_VARIANT = variant
    ys = []
    for tiled in (False, True):
        y = torch.full((M, N), float("nan"), dtype=BF, device=DEV)
        ops.gemm(x, K, 1, wt if tiled else w, 1, K, y, N, M, N, K, b_tiled=tiled, bias=b, residual=aux)
        assert ops.last_gemm_path() == ("mfma_nt" if variant == 4 else "mfma_nt_pp")
        ys.append(y)
    assert torch.equal(bits(ys[0]), bits(ys[1])) and bool(torch.isfinite(ys[0].float()).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. dgrad
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [-1, 9])
def test_dgrad_through_the_tiled_transposed_copy(variant):
    M, N, K = 300, 512, 256                      # dx[M, K] = dy[M, N] . W[N, K]
    dy, w, u = rnd(M, N, seed=11), rnd(N, K, seed=12, scale=N ** -0.5), rnd(M, K, seed=13)

    class P:
        pass
    p = P()
    p.m3ae_c, p.m3ae_t = w, w.t().contiguous()
    fwd, tt = tb.attach(p)
    torch.cuda.synchronize()
    assert torch.equal(bits(fwd), bits(tb.tile_reference(w))) and torch.equal(bits(tt), bits(tb.tile_reference(p.m3ae_t)))
    ops.GEMM_NT_VARIANT = variant
    res = []
    for on in (False, True):
        ops.TILED_B = on
        res.append((ops.mm_dgrad(dy, p, dact_aux=u, dact=ops.ACT_GELU), ops.mm_dgrad(dy, p, residual=u),
                    ops.mm_nt(u, K, M, w, bias=None)[0]))
        assert ops.last_gemm_path() == ("mfma_nt_pp2" if variant == 9 else "mfma_nt")
    for a, b in zip(*res):
        assert torch.equal(bits(a), bits(b))
    ref = (dy.float() @ w.float() + u.float())
    assert float((res[1][1].float() - ref).abs().max()) < 0.05 * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _desc(a, b, c, M, N, K, **over):
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch2 = M, N, K, 1, 1
    d.A, d.a_sm, d.a_sk = a.data_ptr(), K, 1
    d.B, d.b_sk, d.b_sn = b.data_ptr(), 1, K
    d.C, d.c_sm, d.c_sn = c.data_ptr(), N, 1
    d.dtype_a = d.dtype_b = d.dtype_c = _lib.BF16
    d.alpha = 1.0
    d.launch_flags = _lib.GEMM_B_TILED
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_tiled_flag_is_refused_where_the_layout_does_not_apply():
    M, N, K = 200, 256, 128
    a, w = rnd(M, K, seed=20), rnd(N, K, seed=21)
    wt = tb.tile_reference(w)
    a32, w32 = a.float(), w.float()
    L, s = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    c = torch.full((2 * M, N), 7.0, dtype=BF, device=DEV)
    c32 = torch.full((M, N), 7.0, dtype=F32, device=DEV)
    cases = {
        "fp32 operands": _desc(a32, w32, c32, M, N, K, dtype_a=_lib.F32, dtype_b=_lib.F32, dtype_c=_lib.F32),
        "fp32x3": _desc(a32, w32, c32, M, N, K, dtype_a=_lib.F32, dtype_b=_lib.F32, dtype_c=_lib.F32,
                        launch_flags=_lib.GEMM_B_TILED | _lib.GEMM_F32_X3),
        "reduction-strided B": _desc(a, wt, c, M, N, K, b_sk=N, b_sn=1),
        "K % 32 != 0": _desc(a, wt, c, M, N, K - 8, b_sn=K - 8),
        "row length is not K": _desc(a, wt, c, M, N, K, b_sn=K + 8),
        "batched B": _desc(a, wt, c, M // 2, N, K, batch1=2, a_sb1=(M // 2) * K, b_sb1=0, c_sb1=(M // 2) * N),
        "misaligned B": _desc(a, wt[4:], c, M, N - 16, K),
    }
    for name, d in cases.items():
        assert L.m3ae_gemm(C.byref(d), s) == -2, name                 # M3AE_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((c == 7.0).all()) and bool((c32 == 7.0).all())        # returned before any launch
    # the wgrad family (deterministic entry point included) has no tiled operand
    g = torch.zeros(K, N, dtype=F32, device=DEV)
    d = _desc(a, wt, g, K, N, M, a_sm=1, a_sk=K, b_sk=N, b_sn=1, dtype_c=_lib.F32, accumulate=1,
              launch_flags=_lib.GEMM_B_TILED | _lib.GEMM_DETERMINISTIC)
    ws = torch.empty(1 << 22, dtype=F32, device=DEV)
    assert L.m3ae_gemm_det(C.byref(d), C.c_void_p(ws.data_ptr()), ws.numel() * 4, s) == -2
    torch.cuda.synchronize()
    assert not bool(g.any())
    # and the accepted call next to them
    d = _desc(a, wt, c, M, N, K)
    assert L.m3ae_gemm(C.byref(d), s) == 0
    assert torch.equal(bits(c[:M]), bits(ops.mm_nt(a, K, M, w)[0])) and bool((c[M:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. one block, switch on and off; the store keeps the copies current
# ---------------------------------------------------------------------------------------------------------------------------------
def _block_run(blk, store, x0, dy, tiled, det):
    calls = []
    real = ops.gemm

    def counting(*a, **kw):
        calls.append(bool(kw.get("b_tiled")))
        return real(*a, **kw)
    ops.TILED_B = tiled
    ops.gemm = counting
    try:
        with ops.deterministic_mode(det):
            store.zero_grad()
            x = x0.clone().requires_grad_(True)
            y = blk(x)
            y.backward(dy)
            torch.cuda.synchronize()
    finally:
        ops.gemm = real
    return y.detach().clone(), x.grad.clone(), {n: q.grad.clone() for n, q in blk.named_parameters()}, sum(calls)


@pytest.mark.parametrize("B,L,D", [(2, 17, 128), (2, 577, 768)], ids=str)
def test_clip_block_with_the_tiled_weights_on_and_off(B, L, D):
    torch.manual_seed(3)
    blk = ResidualAttentionBlock(D, D // 64)
    synth.fill_deterministic(blk)
    ops.TILED_B = True                       # the store allocates and fills the tiled copies
    store = ParamStore(blk, STORE_CFG, DEV, BF, weight_units=blk.weight_units)
    x0, dy = rnd(B, L, D, seed=41), rnd(B, L, D, seed=42)
    for u in blk.weight_units():
        w = u.m3ae_c
        assert torch.equal(bits(w.m3ae_tb), bits(tb.tile_reference(w))) and torch.equal(bits(u.m3ae_t), bits(w.t().contiguous()))
        assert torch.equal(bits(u.m3ae_tt), bits(tb.tile_reference(u.m3ae_t)))
    # deterministic mode (ordered wgrad): everything bit for bit
    y1, dx1, g1, n1 = _block_run(blk, store, x0, dy, True, True)
    y0, dx0, g0, n0 = _block_run(blk, store, x0, dy, False, True)
    assert n1 == 8 and n0 == 0               # 4 forward GEMMs + 4 dgrads read tiled copies; none with the switch off
    assert torch.equal(bits(y1), bits(y0)) and torch.equal(bits(dx1), bits(dx0))
    for n in g1:
        assert torch.equal(g1[n], g0[n]), n
    assert bool(torch.isfinite(y1.float()).all()) and float(dx1.float().abs().max()) > 0
    # default mode: the wgrad kernels add their splits with atomics (untouched by the switch): outputs and input gradient equal,
    # parameter gradients within the block tests' bf16 tolerance (tests/test_gpu_ops.py: fused block against composition)
    y1, dx1, g1, _ = _block_run(blk, store, x0, dy, True, False)
    y0, dx0, g0, _ = _block_run(blk, store, x0, dy, False, False)
    assert torch.equal(bits(y1), bits(y0)) and torch.equal(bits(dx1), bits(dx0))
    for n in g1:
        scale = float(g0[n].abs().max()) + 1e-12
        err = (g1[n] - g0[n]).abs()
        assert bool((err <= 4e-2 * scale + 4e-2 * g0[n].abs()).all()), n
    # an optimizer step rewrites the shadows: the copies follow in the same call
    before = blk.mlp.c_fc.weight.m3ae_c.clone()
    store.adamw_step(max_steps=10, lr_factor=1.0)
    torch.cuda.synchronize()
    assert not torch.equal(bits(before), bits(blk.mlp.c_fc.weight.m3ae_c))
    for u in blk.weight_units():
        w = u.m3ae_c
        assert torch.equal(bits(w.m3ae_tb), bits(tb.tile_reference(w))) and torch.equal(bits(u.m3ae_t), bits(w.t().contiguous()))
        assert torch.equal(bits(u.m3ae_tt), bits(tb.tile_reference(u.m3ae_t)))
