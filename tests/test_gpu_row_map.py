"""GPU: the dropout row map of the `*_rows` entry points.  A call on every row_step-th row of a dropout site (mask row
row_base + row * row_step) must apply the masks the call on all rows applies to those rows -- so every check below is bit
equality between the mapped call and the matching rows of the full call, at the smallest shapes where each index can go wrong
(ld rounded up to a multiple of 4, a partial last tile, more than one key tile, the 577-key and the 32-key attention)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, ops  # noqa: E402

P, SEED = 0.5, 0x1234ABCD5678
BF = torch.bfloat16


def rnd(*shape, dtype=BF, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def _gemm_pair(B, N, K, dtype, step, **kw):
    """(full output rows 0::step, mapped output), each a tuple (y, preact or None), of one epilogue configuration."""
    x, w = rnd(B * step, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, scale=K ** -0.5, seed=2)
    b = rnd(N, dtype=torch.float32, seed=3)
    extra = {}
    for name in ("residual", "dact_aux"):
        if kw.pop("with_" + name, False):
            t = rnd(B * step, N, dtype=dtype, seed=4 + len(name))
            extra[name] = (t, t[0::step].contiguous())
    full = ops.mm_nt(x, K, B * step, w, bias=b, dropout=(P, SEED), **{k: v[0] for k, v in extra.items()}, **kw)
    path_full = ops.last_gemm_path()
    live = ops.mm_nt(x, step * K, B, w, bias=b, dropout=(P, SEED), rows=(0, step), **{k: v[1] for k, v in extra.items()}, **kw)
    assert ops.last_gemm_path() == path_full
    return [None if t is None else t[0::step] for t in full], live, path_full


def _assert_rows_equal(full, live, what):
    for f, l in zip(full, live):
        assert (f is None) == (l is None)
        if f is not None:
            assert torch.equal(f, l), f"{what}: {(f.float() - l.float()).abs().max().item():.3e}"


@pytest.mark.parametrize("case", ["plain", "gelu_preact", "dmul", "generic", "f32x3"])
def test_gemm_epilogue_dropout_rows(case):
    """A [5 * 7, 64] against rows 0::7, N = 72, p = 0.5, bias and residual (the dgrad class: the saved derivative instead).  The
    generic and fp32x3 kernels also take N = 70, where the mask's ld (72) differs from N."""
    B, step, K = 5, 7, 64
    if case == "plain":
        full, live, path = _gemm_pair(B, 72, K, BF, step, with_residual=True)
        assert path.startswith("mfma_nt")
    elif case == "gelu_preact":
        full, live, path = _gemm_pair(B, 72, K, BF, step, with_residual=True, act=ops.ACT_GELU, want_preact=True)
        assert path.startswith("mfma_nt")
    elif case == "dmul":   # the dgrad class that re-applies a mid-layer dropout before multiplying by the saved derivative
        full, live, path = _gemm_pair(B, 72, K, BF, step, with_dact_aux=True, dact=ops.ACT_MULAUX)
        assert path.startswith("mfma_nt")
    elif case == "generic":
        for N in (72, 70):   # 70: ld = 72 != N
            full, live, path = _gemm_pair(B, N, K, BF, step, with_residual=True, force_generic=True)
            assert path == "generic"
            _assert_rows_equal(full, live, f"{case} N={N}")
    else:
        with ops.f32x3_mode(True):
            for N in (72, 70):
                full, live, path = _gemm_pair(B, N, K, torch.float32, step, with_residual=True)
                assert path == "f32x3"
                _assert_rows_equal(full, live, f"{case} N={N}")
    _assert_rows_equal(full, live, case)
    # the mask is really applied: without the residual about half of the outputs are exact zeros
    if case == "dmul":
        z = (live[0].float() == 0).float().mean().item()
        assert 0.3 < z < 0.7, z


def test_gemm_epilogue_dropout_rows_on_the_pingpong_kernel():
    """M = 257 mapped rows (a partial last 256-row tile), row_step = 3, N = K = 768 on gemm_nt_pp2_kernel (pinned: at this size
    the shape rule takes the 128 x 128 kernel)."""
    ops.GEMM_NT_VARIANT = 9
    try:
        full, live, path = _gemm_pair(257, 768, 768, BF, 3, with_residual=True)
    finally:
        ops.GEMM_NT_VARIANT = -1
    assert path == "mfma_nt_pp2"
    _assert_rows_equal(full, live, "pp2")


@pytest.mark.parametrize("base", [0, 5])
def test_layernorm_bwd_drop_rows(base):
    D, n, step = 768, 6, 33
    M = base + (n - 1) * step + 1
    ln = torch.nn.LayerNorm(D, eps=1e-12).cuda()
    x, dy = rnd(M, D, seed=1), rnd(M, D, seed=2)
    _, mean, rstd = ops.ln_fwd_raw(x, ln)
    dx, dxd = ops.ln_bwd_raw(dy, x, ln, mean, rstd, drop=(0.1, SEED))
    sel = slice(base, None, step)
    xs, dys = x[sel].contiguous(), dy[sel].contiguous()
    dx1, dxd1 = ops.ln_bwd_raw(dys, xs, ln, mean[sel].contiguous(), rstd[sel].contiguous(), drop=(0.1, SEED), rows=(base, step))
    assert dx1.shape[0] == n and torch.equal(dx1, dx[sel]) and torch.equal(dxd1, dxd[sel])
    assert 0.02 < (dxd1.float() == 0).float().mean().item() < 0.25


def _attn_inputs(Lk, masked):
    B, D = 2, 768
    q, k, v = (rnd(B, Lk, D, seed=s) for s in (1, 2, 3))
    mask = None
    if masked:
        mask = torch.zeros(B, Lk, device="cuda")
        mask[0, Lk - 5:] = -10000.0
        mask[1, Lk // 2:] = -10000.0
    return q, k, v, mask


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Lk", [33, 145, 577, 32])
def test_attention_rows_forward_and_backward(Lk, masked):
    """Lq = 1 with row_step = Lq_full against query 0 of the Lq = Lk call: o, lse forward; dq[0], dk, dv backward with d_o zero
    outside query 0 in the full call (the other queries then contribute exact zeros)."""
    H, drop = 12, (0.1, SEED)
    q, k, v, mask = _attn_inputs(Lk, masked)
    o, lse = ops.attn_forward(q, k, v, H, mask, dropout=drop)
    q1 = q[:, :1]
    o1, lse1 = ops.attn_forward(q1, k, v, H, mask, dropout=drop, rows=(0, Lk))
    assert torch.equal(o1[:, 0], o[:, 0]) and torch.equal(lse1[:, :, 0], lse[:, :, 0])
    # a different map gives a different mask (the map is not ignored)
    o2, _ = ops.attn_forward(q1, k, v, H, mask, dropout=drop, rows=(1, Lk))
    assert not torch.equal(o2, o1)

    do = torch.zeros_like(o)
    do[:, 0] = rnd(2, 768, seed=9)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ops.attn_backward(q, k, v, o, lse, do, dq, dk, dv, H, mask, dropout=drop)
    dq1 = torch.empty_strided(q1.shape, q1.stride(), dtype=BF, device="cuda")
    dk1, dv1 = torch.empty_like(k), torch.empty_like(v)
    ops.attn_backward(q1, k, v, o1, lse1, do[:, :1].contiguous(), dq1, dk1, dv1, H, mask, dropout=drop, rows=(0, Lk))
    assert torch.equal(dq1[:, 0], dq[:, 0]) and torch.equal(dk1, dk) and torch.equal(dv1, dv)
    assert dk.float().abs().max().item() > 0


def test_attention_rows_fp32_path():
    """The materialised fp32 path draws its masks through m3ae_dropout_rows: same check, Lk = 33."""
    H, drop, Lk = 12, (0.1, SEED), 33
    q, k, v, mask = (None if t is None else t.float() for t in _attn_inputs(Lk, True))
    o, _ = ops.attn_forward(q, k, v, H, mask, dropout=drop)
    o1, _ = ops.attn_forward(q[:, :1], k, v, H, mask, dropout=drop, rows=(0, Lk))
    assert torch.equal(o1[:, 0], o[:, 0])


def test_dropout_rows_keep_mask():
    rows, cols, step, base = 6, 70, 33, 5     # cols = 70: ld = 72
    M = base + (rows - 1) * step + 1
    full = ops.dropout_keep_mask(M, cols, P, SEED)
    keep = torch.empty((rows, cols), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().m3ae_dropout_rows(None, None, C.c_void_p(keep.data_ptr()), rows, cols, P, SEED, None, _lib.BF16, base, step,
                                            ops._stream()), "m3ae_dropout_rows")
    assert torch.equal(keep, full[base::step].to(torch.uint8))
    assert 0.3 < keep.float().mean().item() < 0.7
