"""GPU: the fp32 residual stream of the image tower in bf16 mode (config key clip_residual_dtype="fp32").

  1, 2  the mixed LayerNorm kernels (fp32 rows <-> bf16 operands) against the fp32 kernels, bit for bit, in fenced buffers
  3     the GEMM class the block's two joins take (bf16 A / B, fp32 C, fp32 residual) at the tower's shapes, exact tier.
        tests/test_gpu_gemm_accuracy.py::test_nt_exact pins this class (its "bias+res" epilogue with fp32 C) on variants 9 and auto
        at (300, 264, 256 | 3072); what it lacks is M = 1154 with N = 768 and K = 768 | 3072, added here
  4     the fused block against the op-level composition
  5     the tower against float64: the stream's error, the gradients' error (figures printed; DESIGN.md section 4 tabulates them)
  6     the model fixtures within the bf16 bounds of tests/test_gpu_model.py
  7     the default is untouched; the key does nothing in the fp32 modes
  8     training: deterministic steps, a de-duplicated batch, GraphedStep
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_stream_model as CM  # noqa: E402
import gemm_accuracy as ga  # noqa: E402
from m3ae_amd import _lib, ops, synth  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from m3ae_amd.modules.clip_model import ResidualAttentionBlock, VisualTransformer  # noqa: E402
from m3ae_amd.param_store import ParamStore  # noqa: E402
from oracle_util import finetune_vqa_rad_config, full_batch, load_golden, tiny_batch, tiny_config  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(1, 128), (5, 768), (34, 128), (67, 1024), (300, 516), (1155, 768), (20011, 768)]
EPS = 1e-5
STORE_CFG = dict(learning_rate=1e-3, weight_decay=0.01, lr_multiplier_head=1, lr_multiplier_multi_modal=1)


@pytest.fixture(autouse=True)
def _restore_switches():
    old = ops.deterministic(), ops.GEMM_NT_VARIANT
    yield
    ops.set_deterministic(old[0])
    ops.GEMM_NT_VARIANT = old[1]


def rnd(*shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def fenced_vec(n):
    buf = torch.full((n + 8,), ga.FENCE, dtype=F32, device=DEV)
    return buf, buf[:n]


def vec_fence_intact(buf, n, msg):
    assert bool((buf[n:] == ga.FENCE).all()), f"{msg}: written past element {n}"


def ln_inputs(M, D):
    x = rnd(M, D, seed=11 + M, scale=2.0) + 0.3 * rnd(M, 1, seed=12 + M)
    return x, 1 + 0.1 * rnd(D, seed=13), 0.1 * rnd(D, seed=14)


def ln_fwd(x, g, b, mixed):
    """(y, mean, rstd) of the mixed kernel or of the fp32 kernel, every output fenced and the fences checked."""
    M, D = x.shape
    ybuf, y = ga.fenced((M, D), D, BF if mixed else F32, DEV)
    mbuf, mean = fenced_vec(M)
    rbuf, rstd = fenced_vec(M)
    L = _lib.lib()
    if mixed:
        _lib.check(L.m3ae_layernorm_fwd_mixed(p(x), p(g), p(b), p(y), p(mean), p(rstd), M, D, EPS, stream()), "fwd_mixed")
    else:
        _lib.check(L.m3ae_layernorm_fwd(p(x), p(g), p(b), p(y), p(mean), p(rstd), M, D, EPS, _lib.F32, 0, 0, stream()), "fwd")
    torch.cuda.synchronize()
    ga.assert_fence_intact(ybuf, (M, D), f"LayerNorm forward {'mixed' if mixed else 'fp32'} ({M}, {D}) y")
    vec_fence_intact(mbuf, M, "mean")
    vec_fence_intact(rbuf, M, "rstd")
    return y, mean, rstd


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. LayerNorm forward, fp32 rows in, bf16 rows out
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,D", SHAPES, ids=str)
def test_layernorm_forward_mixed_is_the_fp32_kernel_rounded_once(M, D):
    if M == 20011:   # past one sweep of the resident grid (at most 8 workgroups of 4 rows on each of 256 CUs), last workgroup ragged
        assert M > 8 * 256 * 4 and M % 4 != 0
    x, g, b = ln_inputs(M, D)
    y32, mean32, rstd32 = ln_fwd(x, g, b, mixed=False)
    y, mean, rstd = ln_fwd(x, g, b, mixed=True)
    assert y.dtype == BF and torch.equal(y, y32.to(BF))
    assert torch.equal(mean, mean32) and torch.equal(rstd, rstd32)
    # without beta, and through ops (the path the tower's ln_post takes)
    y, _, _ = ln_fwd(x, g, None, mixed=True)
    assert torch.equal(y, ln_fwd(x, g, None, mixed=False)[0].to(BF))
    assert torch.equal(ops.layer_norm(x, g, b, EPS, out_dtype=BF), y32.to(BF))
    # the numpy model (tests/clip_stream_model.py): one rounding of an fp32 LayerNorm; the kernel's sums run in another order
    if M <= 300:
        bits, _, _ = CM.np_layernorm_mixed(x.cpu().numpy(), g.cpu().numpy(), b.cpu().numpy(), EPS)
        model = torch.from_numpy(CM.np_bf16_to_f32(bits)).to(DEV)
        got = ops.layer_norm(x, g, b, EPS, out_dtype=BF).float()
        assert bool(((got - model).abs() <= 2.0 ** -7 * model.abs() + 1e-5).all())   # at most one bf16 step apart


def test_layernorm_mixed_refuses_what_it_has_no_kernel_for():
    x, g, b = ln_inputs(8, 130)    # D % 4 != 0
    y = torch.empty(8, 130, dtype=BF, device=DEV)
    st = torch.empty(8, device=DEV)
    assert _lib.lib().m3ae_layernorm_fwd_mixed(p(x), p(g), p(b), p(y), p(st), p(st), 8, 130, EPS, stream()) == -2
    with pytest.raises(_lib.M3AEHipError):
        ops.layer_norm(x.to(BF), g, b, EPS, out_dtype=F32)
    with pytest.raises(_lib.M3AEHipError):
        ops.layer_norm(ln_inputs(8, 128)[0], g[:128].contiguous(), None, EPS, rms=True, out_dtype=BF)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm backward on the fp32 stream
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_bwd(dy, x, g, mean, rstd, dx_add, mixed, det, want_lo=False):
    """(dx, dx_lo, dgamma, dbeta); dx / dx_lo fenced.  mixed: dy bf16 through the new entry points; else dy fp32 through the fp32
    kernel."""
    M, D = x.shape
    L = _lib.lib()
    dxbuf, dx = ga.fenced((M, D), D, F32, DEV)
    lobuf, lo = ga.fenced((M, D), D, BF, DEV) if want_lo else (None, None)
    dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    ws = torch.empty(2 * L.m3ae_layernorm_bwd_blocks(M) * D, device=DEV)
    if mixed:
        fn = L.m3ae_layernorm_bwd_mixed_det if det else L.m3ae_layernorm_bwd_mixed
        _lib.check(fn(p(dy), p(x), p(g), p(mean), p(rstd), p(dx), p(dx_add), p(lo), p(dg), p(db), p(ws), M, D, stream()), "bwd_mixed")
    else:
        fn = L.m3ae_layernorm_bwd_det if det else L.m3ae_layernorm_bwd
        _lib.check(fn(p(dy), p(x), p(g), None, p(mean), p(rstd), p(dx), p(dx_add), p(dg), p(db), p(ws), M, D, _lib.F32, 0, 0,
                      stream()), "bwd")
    torch.cuda.synchronize()
    ga.assert_fence_intact(dxbuf, (M, D), f"LayerNorm backward ({M}, {D}) dx")
    if lobuf is not None:
        ga.assert_fence_intact(lobuf, (M, D), f"LayerNorm backward ({M}, {D}) dx_lo")
    return dx, lo, dg, db


@pytest.mark.parametrize("M,D", SHAPES, ids=str)
def test_layernorm_backward_mixed_is_the_fp32_kernel_on_the_widened_dy(M, D):
    x, g, b = ln_inputs(M, D)
    _, mean, rstd = ln_fwd(x, g, b, mixed=False)
    mean, rstd = mean.clone(), rstd.clone()
    dy = rnd(M, D, seed=21 + M, dtype=BF)
    add = rnd(M, D, seed=22 + M)
    # float64 sums of the fp32 terms the kernels add: dgamma: dy * h with h = (x - mean) * rstd as fp32 forms it; dbeta: dy
    h = ((x - mean[:, None]) * rstd[:, None]).double()
    t_g, t_b = dy.double() * h, dy.double()
    bound_g, bound_b = (M * ga.U * t.abs().sum(0) for t in (t_g, t_b))   # n fp32 additions (products included), in any order
    det_ref = None
    for dx_add in (None, add):
        want_dx, _, want_dg, want_db = ln_bwd(dy.float(), x, g, mean, rstd, dx_add, mixed=False, det=True)
        for want_lo in (False, True):
            for det in (True, False):
                dx, lo, dg, db = ln_bwd(dy, x, g, mean, rstd, dx_add, mixed=True, det=det, want_lo=want_lo)
                msg = f"dx_add {dx_add is not None}, dx_lo {want_lo}, ordered {det}"
                assert torch.equal(dx, want_dx), msg
                if want_lo:
                    assert torch.equal(lo, dx.to(BF)), msg
                if det:
                    assert torch.equal(dg, want_dg) and torch.equal(db, want_db), msg
                    det_ref = det_ref or (dg, db)
                    assert torch.equal(dg, det_ref[0]) and torch.equal(db, det_ref[1]), msg
                err_g, err_b = (dg.double() - t_g.sum(0)).abs(), (db.double() - t_b.sum(0)).abs()
                assert bool((err_g <= bound_g).all()), (msg, (err_g / bound_g.clamp_min(1e-300)).max().item())
                assert bool((err_b <= bound_b).all()), (msg, (err_b / bound_b.clamp_min(1e-300)).max().item())
        if dx_add is not None:   # the stream's gradient is added once, after the LayerNorm's own
            plain = ln_bwd(dy, x, g, mean, rstd, None, mixed=True, det=True)[0]
            assert torch.equal(want_dx, plain + add)
    # through ops: LayerNormFn's backward (op-level composition) and the raw helper (fused block)
    xx = x.clone().requires_grad_(True)
    gp, bp = torch.nn.Parameter(g.clone()), torch.nn.Parameter(b.clone())
    with ops.deterministic_mode(True):
        ops.layer_norm(xx, gp, bp, EPS, out_dtype=BF).backward(dy)
    want = ln_bwd(dy.float(), x, g, mean, rstd, None, mixed=False, det=True)
    assert torch.equal(xx.grad, want[0]) and torch.equal(gp.grad, want[2]) and torch.equal(bp.grad, want[3])


def test_layernorm_backward_mixed_ordered_form_gives_one_bit_pattern_beside_a_large_gemm():
    M, D = 20011, 768
    x, g, b = ln_inputs(M, D)
    _, mean, rstd = ln_fwd(x, g, b, mixed=False)
    dy, add = rnd(M, D, seed=31, dtype=BF), rnd(M, D, seed=32)
    side = torch.cuda.Stream()
    nx, nw = rnd(8192, 3072, seed=901, dtype=BF), rnd(3072, 3072, seed=902, scale=3072 ** -0.5, dtype=BF)
    first = None
    for it in range(10):
        with torch.cuda.stream(side):
            for _ in range(2):
                ops.mm_nt(nx, 3072, 8192, nw)
        out = ln_bwd(dy, x, g, mean, rstd, add, mixed=True, det=True, want_lo=True)
        first = first or out
        for k, (a, c) in enumerate(zip(out, first)):
            assert torch.equal(a, c), f"call {it}, output {k}"
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the GEMM class of the two joins: bf16 A / B, fp32 C, fp32 residual
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 4, 7, 9, -1])
@pytest.mark.parametrize("K", [768, 3072])
def test_nt_exact_fp32_c_fp32_residual_at_the_tower_shapes(K, variant):
    M, N = 1154, 768
    o = ga.exact_operands(M, N, K, 77 + M + N + K, DEV)
    a, b = o["a"].to(BF), o["b"].to(BF)
    ops.GEMM_NT_VARIANT = variant
    for name in ("plain", "bias+res"):
        kw = ga.exact_epilogue(name, o, None, lambda t: t.to(F32))
        ref = ga.reference(o["a"], o["b"], **kw)
        cbuf, c = ga.fenced((M, N), N, F32, DEV)
        res = kw.get("residual")
        assert res is None or res.dtype == F32
        ops.gemm(a, K, 1, b, 1, K, c, N, M, N, K, alpha=kw.get("alpha", 1.0), bias=kw.get("bias"), residual=res)
        msg = f"({M}, {N}, {K}) {name} fp32 C: path {ops.last_gemm_path()}, variant {variant}"
        if variant == 9:   # the 256 x 256 kernel with a ragged last row tile (1154 = 4 * 256 + 130); auto: the product's own choice
            assert ops.last_gemm_path() == "mfma_nt_pp2", msg
        bad = c.double() != ga.expected_store(ref.c, False)
        assert not bad.any(), f"{msg}: not the exact result, " + ga.first_bad(bad)
        ga.assert_fence_intact(cbuf, (M, N), msg)
    # the call the block makes: ops.mm_nt(..., residual=fp32, out_dtype=float32)
    kw = ga.exact_epilogue("bias+res", o, None, lambda t: t.to(F32))
    y, _ = ops.mm_nt(a, K, M, b, bias=kw["bias"], residual=kw["residual"], out_dtype=F32, alpha=kw.get("alpha", 1.0))
    assert y.dtype == F32 and not (y.double() != ga.reference(o["a"], o["b"], **kw).c).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. block: fused fp32-stream path against the op-level composition
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,D", [(2, 17, 128), (2, 577, 768)], ids=str)
def test_fused_block_on_the_fp32_stream_equals_the_op_level_composition(B, L, D):
    torch.manual_seed(3)
    blk = ResidualAttentionBlock(D, D // 64)
    synth.fill_deterministic(blk)
    store = ParamStore(blk, STORE_CFG, DEV, BF, weight_units=blk.weight_units)
    x0 = rnd(B, L, D, seed=41)
    dy = rnd(B, L, D, seed=42)
    res = []
    for fused in (True, False):
        with ops.deterministic_mode(True):
            store.zero_grad()
            x = x0.clone().requires_grad_(True)
            y = (blk if fused else blk.forward_unfused)(x)
            assert y.dtype == F32
            y.backward(dy)
            torch.cuda.synchronize()
        res.append((y.detach().clone(), x.grad.clone(), {n: q.grad.clone() for n, q in blk.named_parameters()}))
    (yf, dxf, gf), (yu, dxu, gu) = res
    assert torch.equal(yf, yu)
    assert dxf.dtype == F32 and torch.equal(dxf, dxu)
    for n in gf:
        assert torch.equal(gf[n], gu[n]), n
    assert all(bool(torch.isfinite(t).all()) for t in (yf, dxf)) and float(dxf.abs().max()) > 0
    # the stream really is fp32: the output holds values bf16 cannot
    assert not torch.equal(yf, yf.to(BF).float())
    # and the default (bf16 x over the same weights) is another, coarser function of the same input
    with torch.no_grad():
        yb = blk(x0.to(BF))
    assert yb.dtype == BF and not torch.equal(yb.float(), yf)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. tower accuracy against float64
# ---------------------------------------------------------------------------------------------------------------------------------
def _tower(stream_dtype, cfg):
    torch.manual_seed(0)
    v = VisualTransformer(cfg["patch_size"], cfg["vit_width"], cfg["vit_layers"], cfg["vit_width"] // 64, cfg["image_size"],
                          residual_dtype=stream_dtype)
    # CLIP's init of the block weights (CLIP.initialize_parameters), the rest as constructed; masters rounded through bf16
    width, layers = cfg["vit_width"], cfg["vit_layers"]
    g = torch.Generator().manual_seed(7)
    stds = {"attn.in_proj_weight": width ** -0.5, "attn.out_proj.weight": width ** -0.5 * (2 * layers) ** -0.5,
            "mlp.c_fc.weight": (2 * width) ** -0.5, "mlp.c_proj.weight": width ** -0.5 * (2 * layers) ** -0.5}
    with torch.no_grad():
        for n, q in v.named_parameters():
            for suffix, std in stds.items():
                if n.endswith(suffix):
                    q.copy_(torch.randn(q.shape, generator=g) * std)
            if n.endswith("bias") and "ln_" not in n:
                q.copy_(torch.randn(q.shape, generator=g) * 0.02)
            if n == "conv1.weight":
                q.copy_(torch.randn(q.shape, generator=g) * (3 * cfg["patch_size"] ** 2) ** -0.5)
            q.copy_(q.to(BF).float())
    sd = {n: q.detach().double().clone() for n, q in v.named_parameters()}
    store = ParamStore(v, STORE_CFG, DEV, BF, weight_units=v.weight_units)
    return v, store, sd


@pytest.fixture(scope="module")
def tower_reference():
    """float64 on the CPU, once: tokens, ln_post input, output, and the gradients of the fixed scalar loss."""
    cfg = tiny_config(vit_layers=12, compute_dtype="bf16")
    _, _, sd = _tower("bf16", cfg)
    img = torch.randn(2, 3, cfg["image_size"], cfg["image_size"], generator=torch.Generator().manual_seed(5))
    L = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    probe = torch.randn(2, L, cfg["vit_width"], generator=torch.Generator().manual_seed(6)).double()
    leaves = {n: t.clone().requires_grad_(True) for n, t in sd.items()}
    tok, pre, out = CM.tower_f64(img.double(), leaves, cfg["vit_width"] // 64, cfg["patch_size"], cfg["vit_layers"] - 1)
    tok.retain_grad()
    (out * probe).sum().backward()
    return dict(cfg=cfg, img=img, probe=probe, pre=pre.detach(), out=out.detach(), d_tok=tok.grad.clone(),
                d_conv=leaves["conv1.weight"].grad.clone())


def _run_tower(stream_dtype, ref):
    cfg = ref["cfg"]
    v, store, _ = _tower(stream_dtype, cfg)
    seen = {}
    real_ln, real_tok = ops.layer_norm, ops.vit_tokens

    def spy_ln(x, gamma, *args, **kw):
        if gamma is v.ln_post.weight:
            seen["pre"] = x.detach().clone()
        return real_ln(x, gamma, *args, **kw)

    def spy_tok(*args, **kw):
        t = real_tok(*args, **kw)
        t.retain_grad()
        seen["tok"] = t
        return t
    ops.layer_norm, ops.vit_tokens = spy_ln, spy_tok
    try:
        store.zero_grad()
        out = v(ref["img"].to(DEV), BF)
        (out.float() * ref["probe"].to(DEV).float()).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.layer_norm, ops.vit_tokens = real_ln, real_tok
    want = torch.float32 if stream_dtype == "fp32" else BF
    assert seen["pre"].dtype == want and seen["tok"].dtype == want and out.dtype == BF and seen["tok"].grad.dtype == want
    return dict(pre=CM.rel_err(seen["pre"].cpu(), ref["pre"]), out=CM.rel_err(out.detach().cpu(), ref["out"]),
                d_tok=CM.rel_err(seen["tok"].grad.cpu(), ref["d_tok"]), d_conv=CM.rel_err(v.conv1.weight.grad.cpu(), ref["d_conv"]))


def test_tower_error_against_float64_with_either_stream(tower_reference):
    """Figures observed on MI355X: DESIGN.md section 4."""
    e = {s: _run_tower(s, tower_reference) for s in ("bf16", "fp32")}
    for k in ("pre", "out", "d_tok", "d_conv"):
        print(f"CLIP_RESIDUAL tower 128 x 11 blocks, 17 tokens, B = 2: {k:6s} bf16 stream {e['bf16'][k]:.3e}  fp32 stream {e['fp32'][k]:.3e}  "
              f"ratio {e['bf16'][k] / e['fp32'][k]:.2f}")
    assert e["bf16"]["pre"] / e["fp32"]["pre"] >= 3.0
    assert e["fp32"]["out"] <= e["bf16"]["out"]
    assert e["fp32"]["d_tok"] <= e["bf16"]["d_tok"]
    assert e["fp32"]["d_conv"] <= e["bf16"]["d_conv"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 6 / 7. model
# ---------------------------------------------------------------------------------------------------------------------------------
def to_dev(batch):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else [t.to(DEV) for t in v] if isinstance(v, list) and v and
                isinstance(v[0], torch.Tensor) else v) for k, v in batch.items()}


def build(cfg):
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize(DEV, BF if cfg["compute_dtype"] == "bf16" else F32)
    m.eval()
    return m


def test_tiny_fixture_with_the_key_within_the_bf16_bounds():
    """The bounds of tests/test_gpu_model.py::test_tiny_bf16_perf_mode_within_bf16_bounds."""
    m = build(tiny_config(compute_dtype="bf16", clip_residual_dtype="fp32"))
    g = load_golden("tiny_vqa.npz")
    m.store.zero_grad()
    m.set_task()
    ret = m(to_dev(tiny_batch()))
    logits = ret["vqa_logits"].detach().float().cpu().numpy()
    assert np.abs(logits - g["logits"]).max() < 0.05, np.abs(logits - g["logits"]).max()
    loss = ret["vqa_loss"]
    assert abs(loss.item() - float(g["loss"])) < 2e-3 * float(g["loss"])
    loss.backward()
    names, ref = g["grad_names"].tolist(), g["grad_norm"]
    params = dict(m.named_parameters())
    mine = np.array([params[n].grad.double().norm().item() for n in names])
    gn = np.sqrt((mine ** 2).sum())
    assert abs(gn - float(g["global_grad_norm"])) < 3e-2 * float(g["global_grad_norm"]), (gn, float(g["global_grad_norm"]))
    big = ref > 1e-3 * ref.max()
    rel = np.abs(mine[big] - ref[big]) / ref[big]
    assert rel.max() < 0.15, (rel.max(), np.array(names)[big][rel.argmax()])


def test_tiny_pretrain_step_with_the_key_within_the_bf16_bounds():
    """MLM + MIM + ITM (the MIM route gathers the kept rows of the fp32 tokens): the bounds of
    tests/test_gpu_model.py::test_tiny_pretrain_step_bf16_against_reference_gradients."""
    cfg = tiny_config(compute_dtype="bf16", clip_residual_dtype="fp32", loss_names={"mlm": 1, "mim": 1, "itm": 1, "vqa": 0, "cls": 0, "irtr": 0},
                      mim_layer=1, mim_decoder_hidden_size=128, mim_decoder_num_layers=2, mim_decoder_num_heads=2)
    m = build(cfg)
    g = load_golden("tiny_pretrain.npz")
    b = to_dev(tiny_batch(pretrain=True))
    b["itm_labels"] = torch.tensor([1.0, 0.0])
    m.store.zero_grad()
    loss = m.training_step(b)
    loss.backward()
    assert abs(loss.item() - float(g["step_loss"])) < 1e-2 * float(g["step_loss"])
    names, ref = g["grad_names"].tolist(), g["grad_norm"]
    params = dict(m.named_parameters())
    mine = np.array([params[n].grad.double().norm().item() for n in names])
    gn = np.sqrt((mine ** 2).sum())
    assert abs(gn - float(g["global_grad_norm"])) < 5e-2 * float(g["global_grad_norm"]), (gn, float(g["global_grad_norm"]))
    big = ref > 1e-2 * ref.max()
    rel = np.abs(mine[big] - ref[big]) / ref[big]
    assert rel.max() < 0.15, (rel.max(), np.array(names)[big][rel.argmax()])


def test_full_size_fixture_with_the_key_within_the_recorded_bf16_bounds():
    """configs[1] dimensions, B = 2: tests/test_gpu_model.py's BF16_FULL_SIZE_BOUNDS (unchanged), for the setting with the key.  The
    figures are printed beside those of the default, which
    tests/test_gpu_model.py::test_full_size_bf16_observed_errors_within_twice_the_recorded_ones prints; no order between the two
    settings is asserted.  Observed on MI355X: max |dlogits| 2.42e-2 (default 2.25e-2), rms 6.99e-3
    (7.32e-3), loss 4.3e-5 (7.5e-5), global gradient norm 7.4e-4 (1.39e-3), worst large per-parameter norm 2.8e-3 (4.0e-3), median
    9.5e-4 (1.64e-3)."""
    from m3ae_amd.parity import parity_report
    from test_gpu_model import BF16_FULL_SIZE_BOUNDS
    m = build(finetune_vqa_rad_config(compute_dtype="bf16", clip_residual_dtype="fp32"))
    rep = parity_report(m, load_golden("full_vqa.npz"), to_dev(full_batch()))
    print("CLIP_RESIDUAL full-size parity, stream fp32: " + ", ".join(f"{k} {rep[k]:.3e}" for k in (
        "max_abs_dlogits", "rms_dlogits", "loss_rel_err", "global_grad_norm_rel_err", "max_rel_err_large_param_grad_norms",
        "median_rel_err_param_grad_norms")) + f"; worst large parameter: {rep['worst_large_param']}")
    for k, bound in BF16_FULL_SIZE_BOUNDS.items():
        assert rep[k] <= bound, (k, rep[k], bound)


def _logits_and_grads(cfg, batch):
    m = build(cfg)
    with ops.deterministic_mode(True):
        m.store.zero_grad()
        m.set_task()
        ret = m(batch)
        ret["vqa_loss"].backward()
        torch.cuda.synchronize()
    return ret["vqa_logits"].detach().clone(), m.store.grad.clone()


def test_default_is_unchanged_and_the_key_does_nothing_in_the_fp32_modes():
    b = to_dev(tiny_batch())
    base = tiny_config(compute_dtype="bf16")
    without = {k: v for k, v in base.items() if k != "clip_residual_dtype"}
    assert "clip_residual_dtype" not in without
    l0, g0 = _logits_and_grads(without, b)
    l1, g1 = _logits_and_grads(tiny_config(compute_dtype="bf16", clip_residual_dtype="bf16"), b)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    l2, g2 = _logits_and_grads(tiny_config(compute_dtype="bf16", clip_residual_dtype="fp32"), b)
    assert not torch.equal(g0, g2)                                   # (the key does something in bf16 mode)
    for mode in ("fp32", "fp32x3"):
        la, ga_ = _logits_and_grads(tiny_config(compute_dtype=mode), b)
        lb, gb = _logits_and_grads(tiny_config(compute_dtype=mode, clip_residual_dtype="fp32"), b)
        assert torch.equal(la, lb) and torch.equal(ga_, gb), mode


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. training
# ---------------------------------------------------------------------------------------------------------------------------------
TINY_ARGS = ("image_size=64 hidden_size=128 num_heads=2 num_top_layer=2 input_image_embed_size=128 input_text_embed_size=128 "
             "vocab_size=1000 vit_width=128 vit_layers=3 text_hidden=128 text_layers=2 text_heads=2 text_inter=512").split()


def _fit(tmp_path, tag, steps, **over):
    from arrow_util import HashTokenizer, write_split
    from m3ae_amd import data, trainer
    root = str(tmp_path / "arrows")
    if not (tmp_path / "arrows").exists():
        write_split(root, "train", 12)
        write_split(root, "val", 4, seed=100)
    argv = (["with", f"data_root={root}", "num_gpus=1", "num_nodes=1", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta",
             "per_gpu_batchsize=8", "batch_size=8", f"max_steps={steps}", "num_workers=2", "deterministic=True", "learning_rate=0.0005",
             "clip_residual_dtype=fp32", f"log_dir={tmp_path / tag}", "seed=2"] + TINY_ARGS + [f"{k}={v}" for k, v in over.items()])
    cfg = trainer.config_mod.parse_cli(argv)
    assert cfg["clip_residual_dtype"] == "fp32" and cfg["compute_dtype"] == "bf16"
    dev = torch.device(DEV, 0)
    torch.manual_seed(cfg["seed"])
    model = trainer.build_model(cfg, "cls", dev)
    dm = data.ArrowDataModule(cfg, 0, 1, dev, tokenizer=HashTokenizer())
    out = trainer.Trainer(cfg, model, dm, 0, 1, dev, log_every=1).fit()
    assert out["global_step"] == steps
    torch.cuda.synchronize()
    return model, [h[1] for h in out["history"]]


def test_three_deterministic_trainer_steps_twice_give_the_same_parameters(tmp_path):
    runs = [_fit(tmp_path, f"run{i}", 3) for i in range(2)]
    (ma, la), (mb, lb) = runs
    assert la == lb and np.isfinite(la).all()
    assert torch.equal(ma.store.flat, mb.store.flat) and torch.equal(ma.store.shadow, mb.store.shadow)
    assert ma.vision_encoder.visual.residual_dtype == "fp32"


def test_deduplicated_step_with_the_key_has_the_loss_of_the_expanded_batch(tmp_path):
    (_, plain), (_, dedup) = (_fit(tmp_path, f"dedup{flag}", 1, image_dedup=flag) for flag in (False, True))
    assert np.isfinite(plain[0]) and plain[0] == dedup[0]


def test_graphed_step_refuses_the_fp32_stream():
    from m3ae_amd.graph import GraphedStep
    b = to_dev(tiny_batch())
    m = build(tiny_config(compute_dtype="bf16", clip_residual_dtype="fp32"))
    with pytest.raises(ValueError, match="clip_residual_dtype"):
        GraphedStep(m, b, max_steps=10)
    GraphedStep(build(tiny_config(compute_dtype="bf16")), b, max_steps=10)                              # the default: as before
    GraphedStep(build(tiny_config(compute_dtype="fp32", clip_residual_dtype="fp32")), b, max_steps=10)  # no effect in fp32 mode
