"""GPU: deterministic mode (ops.set_deterministic / config key `deterministic`).

Run-to-run equality is checked over R = 10 calls in one process while a second stream keeps an unrelated large NT GEMM in flight:
it changes which workgroup of the kernel under test arrives first, which is exactly what decided the rounding of the fp32-atomic
forms.  Accuracy bounds are the ones the existing tests of the atomic forms use (cited where they are reused); nothing is asserted
about the atomic forms' own run-to-run behaviour."""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, ops, synth  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from oracle_util import finetune_vqa_rad_config, tiny_batch, tiny_config  # noqa: E402
from test_gpu_ops import close, rnd  # noqa: E402

R = 10
# tests/test_gpu_ops.py::test_gemm_wgrad_tn / ::test_gemm_wgrad_tn_pingpong_variant: close(g, ref, 1e-4, 1e-3 * sqrt(rows)), for the
# weight gradient and for the fused bias gradient alike
WGRAD_RTOL, WGRAD_ATOL_PER_SQRT_ROW = 1e-4, 1e-3


def dev():
    return torch.device("cuda")


@pytest.fixture(autouse=True)
def _mode_off_before_and_after():
    assert ops.deterministic() is False
    yield
    ops.set_deterministic(False)
    ops.GEMM_TN_VARIANT = -1


_noise = {}


@contextlib.contextmanager
def busy_second_stream():
    """Yields kick(): queues a few launches of a large NT GEMM (8192 x 3072 x 3072, bf16) on a second stream, unordered against the
    caller's stream, so the kernels the caller launches next share the chip with it."""
    if not _noise:
        _noise["s"] = torch.cuda.Stream()
        _noise["x"] = rnd(8192, 3072, dtype=torch.bfloat16, seed=901)
        _noise["w"] = rnd(3072, 3072, dtype=torch.bfloat16, scale=3072 ** -0.5, seed=902)
    side = _noise["s"]

    def kick(n=3):
        with torch.cuda.stream(side):
            for _ in range(n):
                ops.mm_nt(_noise["x"], 3072, 8192, _noise["w"])
    try:
        yield kick
    finally:
        torch.cuda.synchronize()


def to_dev(batch):
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to("cuda")
        elif isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            out[k] = [t.to("cuda") for t in v]
        else:
            out[k] = v
    return out


def build(cfg, dtype):
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", dtype)
    m.eval()
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the wgrad kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [2, 5])          # 128 x 128 tile (32-row steps) | 256 x 256 ping-pong (its 64-row 128 x 128
@pytest.mark.parametrize("with_bias", [False, True])  # stand-in below 4096 reduction rows): every TN kernel, pinned by selector
@pytest.mark.parametrize("rows", [36928, 2048, 1731])
@pytest.mark.parametrize("N,K", [(768, 768), (2304, 768), (3072, 768), (768, 3072)])
def test_wgrad_ordered_split_k_is_bit_reproducible_and_accurate(N, K, rows, with_bias, variant):
    """dW[N, K] += dY[rows, N]^T X[rows, K] (+ the bias gradient riding on it) onto a non-zero gradient, ten times: one bit
    pattern, within the atomic form's bound of an fp64 product of the same bf16 inputs, still on the MFMA TN kernels."""
    dy, x = rnd(rows, N, dtype=torch.bfloat16, seed=7), rnd(rows, K, dtype=torch.bfloat16, seed=8)
    g0, b0 = rnd(N, K, seed=9), rnd(N, seed=10)
    ref = (g0.double() + dy.double().t() @ x.double())
    refb = b0.double() + dy.double().sum(0)
    ops.GEMM_TN_VARIANT = variant
    ops.set_deterministic(True)
    outs = []
    with busy_second_stream() as kick:
        for it in range(R):
            g, db = g0.clone(), (b0.clone() if with_bias else None)
            kick()
            ops.gemm(dy, 1, N, x, K, 1, g, K, N, K, rows, accumulate=True, a_rowsum=db)
            assert ops.last_gemm_path() == "mfma_tn"
            outs.append((g, db))
    torch.cuda.synchronize()
    g, db = outs[0]
    for it, (gi, dbi) in enumerate(outs[1:], 1):
        assert torch.equal(gi, g), f"call {it}: {int((gi != g).sum())} elements of dW differ from call 0"
        if with_bias:
            assert torch.equal(dbi, db), f"call {it}: {int((dbi != db).sum())} elements of db differ from call 0"
    atol = WGRAD_ATOL_PER_SQRT_ROW * math.sqrt(rows)
    print(f"wgrad {N}x{K} rows {rows} variant {variant}: max |err| {(g.double() - ref).abs().max().item():.3e} (atol {atol:.3e})")
    close(g, ref, WGRAD_RTOL, atol, msg="ordered wgrad")
    if with_bias:
        close(db, refb, WGRAD_RTOL, atol, msg="ordered fused bias grad")


def test_wgrad_ordered_form_keeps_the_fan_out_and_needs_its_workspace():
    """The size query reports more than one split for a 768 x 768 wgrad over 36928 rows, m3ae_gemm refuses the flag, and
    m3ae_gemm_det refuses a short workspace -- on real device pointers."""
    N, K, rows = 768, 768, 36928
    dy, x = rnd(rows, N, dtype=torch.bfloat16, seed=7), rnd(rows, K, dtype=torch.bfloat16, seed=8)
    g = torch.zeros(N, K, device=dev())
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch2 = N, K, rows, 1, 1
    d.A, d.a_sm, d.a_sk = dy.data_ptr(), 1, N
    d.B, d.b_sk, d.b_sn = x.data_ptr(), K, 1
    d.C, d.c_sm, d.c_sn = g.data_ptr(), K, 1
    d.dtype_a, d.dtype_b, d.dtype_c = _lib.BF16, _lib.BF16, _lib.F32
    d.alpha, d.accumulate = 1.0, 1
    L = _lib.lib()
    n = L.m3ae_gemm_det_workspace_bytes(C.byref(d))
    assert n >= 2 * N * K * 4
    d.launch_flags = _lib.GEMM_DETERMINISTIC
    assert L.m3ae_gemm(C.byref(d), ops._stream()) == -2          # M3AE_ERR_UNSUPPORTED: never the atomic kernel under the flag
    ws = torch.empty(n, dtype=torch.uint8, device=dev())
    assert L.m3ae_gemm_det(C.byref(d), ops._p(ws), n - 4, ops._stream()) == -4
    torch.cuda.synchronize()
    assert float(g.abs().max()) == 0.0                            # nothing was launched by the refused calls
    assert L.m3ae_gemm_det(C.byref(d), ops._p(ws), n, ops._stream()) == 0
    close(g, dy.double().t() @ x.double(), WGRAD_RTOL, WGRAD_ATOL_PER_SQRT_ROW * math.sqrt(rows), msg="raw m3ae_gemm_det")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the small reductions
# ---------------------------------------------------------------------------------------------------------------------------------
def _ten_times(fn):
    """fn() -> tuple of tensors; ten calls under the busy second stream, every output bit-equal to the first call's."""
    with busy_second_stream() as kick:
        outs = []
        for _ in range(R):
            kick(2)
            outs.append(tuple(t.detach().clone() for t in fn()))
    for it, o in enumerate(outs[1:], 1):
        for k, (a, b) in enumerate(zip(o, outs[0])):
            assert torch.equal(a, b), f"call {it}, output {k}: {int((a != b).sum())} elements differ from call 0"
    return outs[0]


@pytest.mark.parametrize("M,N,dtype", [(147712, 768, torch.bfloat16), (1154, 498, torch.bfloat16), (1154, 498, torch.float32)])
def test_column_sum_ordered(M, N, dtype):
    """Bias gradients.  Bound: the one the existing wgrad tests put on the (fused) bias gradient, against an fp64 column sum."""
    x = rnd(M, N, dtype=dtype, seed=40)
    base = rnd(N, seed=41)
    ops.set_deterministic(True)

    def run():
        out = base.clone()
        ops.colsum(x, out, True)
        fresh = torch.empty(N, device=dev())
        ops.colsum(x, fresh, False)
        return out, fresh
    out, fresh = _ten_times(run)
    ref = x.double().sum(0)
    close(out, base.double() + ref, WGRAD_RTOL, WGRAD_ATOL_PER_SQRT_ROW * math.sqrt(M), msg="colsum accumulate")
    close(fresh, ref, WGRAD_RTOL, WGRAD_ATOL_PER_SQRT_ROW * math.sqrt(M), msg="colsum overwrite")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,D", [(1154, 768), (18464, 768)])
def test_layernorm_dgamma_dbeta_ordered(dtype, M, D):
    """tests/test_gpu_ops.py::test_layernorm_fwd_bwd's setting and tolerances; plus the dropout-fused backward's fold."""
    x = rnd(M, D, dtype=dtype, seed=12)
    gamma, beta = (1 + 0.1 * rnd(D, seed=13)), 0.1 * rnd(D, seed=14)
    dy = rnd(M, D, dtype=dtype, seed=15)
    ops.set_deterministic(True)

    def run():
        xx = x.clone().requires_grad_(True)
        g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        g.grad, b.grad = torch.zeros_like(g), torch.zeros_like(b)
        ops.layer_norm(xx, g, b, 1e-5).backward(dy)
        ln = torch.nn.LayerNorm(D, eps=1e-5).to(dev())
        with torch.no_grad():
            ln.weight.copy_(gamma)
            ln.bias.copy_(beta)
        ln.weight.grad, ln.bias.grad = torch.zeros_like(gamma), torch.zeros_like(beta)
        y, mean, rstd = ops.ln_fwd_raw(x, ln)
        ops.ln_bwd_raw(dy, x, ln, mean, rstd, drop=(0.1, 1234))
        return g.grad, b.grad, xx.grad, ln.weight.grad, ln.bias.grad
    gg, gb, dx, gg_drop, gb_drop = _ten_times(run)
    xr = x.detach().float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-5).backward(dy.float())
    gt = (1e-3, 1e-3 * math.sqrt(M)) if dtype == torch.float32 else (2e-2, 2e-2 * math.sqrt(M))
    close(gg, gr.grad, *gt, msg="ln dgamma")
    close(gb, br.grad, *gt, msg="ln dbeta")
    close(gg_drop, gr.grad, *gt, msg="ln dgamma (dropout-fused backward: the parameter gradients see the undropped dy)")
    close(gb_drop, br.grad, *gt, msg="ln dbeta (dropout-fused backward)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ids_kind", ["same", "random", "padded"])
@pytest.mark.parametrize("B,S,D", [(3, 32, 128), (64, 32, 768)])
def test_roberta_embedding_backward_ordered(dtype, ids_kind, B, S, D):
    """Duplicate ids: every token the same id (one row takes all B * S contributions), random ids, and padded samples (the
    position table's padding row collects the pads).  At the dimensions of tests/test_gpu_ops.py::test_roberta_embed_and_vit_tokens
    (3 x 32 tokens) with exactly its tolerances, and at 64 x 32 tokens of width 768."""
    V = 500
    gen = torch.Generator().manual_seed(0)
    if ids_kind == "same":
        ids = torch.full((B, S), 7, dtype=torch.long)
    else:
        ids = torch.randint(3, V, (B, S), generator=gen)
        if ids_kind == "padded":
            for b in range(B):
                ids[b, 4 + (b * 5) % 27:] = 1
    ids = ids.to(dev())
    word0, pos0, typ0 = rnd(V, D, seed=21), rnd(514, D, seed=22), rnd(1, D, seed=23)
    do = rnd(B, S, D, dtype=dtype, seed=24)
    ops.set_deterministic(True)

    def run():
        word, pos, typ = (t.clone().requires_grad_(True) for t in (word0, pos0, typ0))
        ops.roberta_embed(ids, word, pos, typ, 1, dtype).backward(do)
        return word.grad, pos.grad, typ.grad
    gw, gp, gt = _ten_times(run)
    word, pos, typ = (t.clone().requires_grad_(True) for t in (word0, pos0, typ0))
    ne = (ids != 1).long()
    pid = torch.cumsum(ne, 1) * ne + 1
    rw, rp, rt = torch.autograd.grad(word[ids] + typ[0] + pos[pid], (word, pos, typ), do.float())
    # the existing test adds at most 3 * 32 = 96 rows into a table row (scale = 1: its tolerances as they are); at 64 x 32 tokens up
    # to 2048 land on one, and the absolute term grows with the square root of the number of addends, as in the wgrad bound
    # (fp32 rounding of a sum of n terms of order one)
    scale = math.sqrt(B * S / 96.0)
    close(gw, rw, 1e-4, 1e-4 * scale, msg="dword")
    close(gp, rp, 1e-4, 1e-4 * scale, msg="dpos")
    close(gt, rt, 1e-4, 1e-3 * scale, msg="dtype")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_losses_ordered(dtype):
    """BCE, cross entropy and the MIM loss: loss scalar and gradient bit-reproducible; tests/test_gpu_ops.py::test_losses' and
    ::test_mim_bookkeeping_kernels_match_the_reference_formulas' tolerances against torch."""
    B, Cc = 64, 498
    x0 = rnd(B, Cc, dtype=dtype, seed=30)
    z = torch.zeros(B, Cc, device=dev())
    z[torch.arange(B), (torch.arange(B) * 7) % Cc] = 1.0
    V = 1000
    lg0 = rnd(B, 32, V, dtype=dtype, seed=31)
    lab = torch.randint(0, V, (B, 32), generator=torch.Generator().manual_seed(1))
    lab[0, :5] = -100
    lab[3] = -100
    lab = lab.to(dev())
    Bm, L, Dm = 16, 576, 768
    full = rnd(Bm, L + 1, Dm, dtype=dtype, seed=32)
    tgt = rnd(Bm, L, Dm, seed=33)
    mask = (torch.rand(Bm, L, generator=torch.Generator().manual_seed(2)) < 0.75).float().to(dev())
    ops.set_deterministic(True)

    def run():
        x = x0.clone().requires_grad_(True)
        l1 = ops.bce_with_logits_loss(x, z)
        l1.backward()
        lg = lg0.clone().requires_grad_(True)
        l2 = ops.cross_entropy(lg, lab)
        l2.backward()
        xd = full.clone().requires_grad_(True)
        l3 = ops.mim_loss(xd, tgt, mask)
        (3.0 * l3).backward()
        return l1, x.grad, l2, lg.grad, l3, xd.grad
    l1, gx, l2, glg, l3, gxd = _ten_times(run)
    xr = x0.float().requires_grad_(True)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(xr, z) * Cc
    ref.backward()
    assert abs(l1.item() - ref.item()) < 1e-4 * ref.item(), (l1.item(), ref.item())
    close(gx, xr.grad, 1e-2, 1e-5, msg="bce grad")
    lr_ = lg0.float().requires_grad_(True)
    r2 = torch.nn.functional.cross_entropy(lr_.view(-1, V), lab.view(-1), ignore_index=-100)
    r2.backward()
    assert abs(l2.item() - r2.item()) < 1e-4 * r2.item(), (l2.item(), r2.item())
    close(glg, lr_.grad, 1e-2, 1e-6, msg="xent grad")
    fr = full.float().requires_grad_(True)
    per = ((fr[:, 1:, :] - tgt) ** 2).mean(-1)
    r3 = (per * mask).sum() / mask.sum()
    (3.0 * r3).backward()
    assert abs(l3.item() - r3.item()) <= 1e-5 * abs(r3.item()) + 1e-6, (l3.item(), r3.item())
    close(gxd, fr.grad, 1e-5 if dtype == torch.float32 else 2e-2, 1e-7, msg="mim dlogits")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the step
# ---------------------------------------------------------------------------------------------------------------------------------
PRETRAIN = dict(drop_rate=0.1, loss_names={"mlm": 1, "mim": 1, "itm": 1, "vqa": 0, "cls": 0, "irtr": 0}, mim_layer=1,
                mim_decoder_hidden_size=128, mim_decoder_num_layers=2, mim_decoder_num_heads=2)


def _backward(m, b, two_streams=None, seed=5):
    if two_streams is not None:
        m.two_streams = two_streams
    m.train()
    m.store.zero_grad()
    ops.set_dropout_seed(seed)
    torch.manual_seed(3)            # the MIM masking noise of the pre-training step
    loss = m.training_step(b)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), m.store.grad.clone()


def test_full_size_step_is_bit_reproducible():
    """configs[1] dimensions, bf16, B = 8, train-mode dropout with a fixed dropout seed: two backward passes from the same state
    give the same flat gradient buffer and loss, bit for bit -- on one stream, on two, and across the two schedules (the comparison
    tests/test_gpu_model.py::test_two_stream_schedule_equals_the_single_stream_step makes with a tolerance); three optimizer steps
    run twice from the same initial state give the same parameters and bf16 shadows."""
    cfg = finetune_vqa_rad_config(compute_dtype="bf16", deterministic=True)
    b = to_dev(synth.synthetic_batch(8, text_len=32, image_size=384, rank=0))
    m = build(cfg, torch.bfloat16)
    assert ops.deterministic() is True          # the config key switched the mode on
    m.set_task()
    with busy_second_stream() as kick:
        l0, g0 = _backward(m, b, two_streams=False)
        assert len(m.store.streams) == 0
        assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
        kick()
        l1, g1 = _backward(m, b, two_streams=False)
        assert torch.equal(l0, l1) and torch.equal(g0, g1), int((g0 != g1).sum())
        for _ in range(2):
            kick()
            l2, g2 = _backward(m, b, two_streams=True)
            assert len(m.store.streams) == 2
            assert torch.equal(l0, l2), (l0.item(), l2.item())
            assert torch.equal(g0, g2), f"{int((g0 != g2).sum())} gradient elements differ between the schedules"
    m.two_streams = type(m).two_streams

    flat0, shadow0 = m.store.flat.detach().clone(), m.store.shadow.detach().clone()

    def three_steps():
        m2 = build(cfg, torch.bfloat16)
        m2.set_task()
        with torch.no_grad():
            assert torch.equal(m2.store.flat, flat0) and torch.equal(m2.store.shadow, shadow0)
        losses = []
        with busy_second_stream() as kick:
            for step in range(3):
                kick()
                m2.train()
                m2.store.zero_grad()
                ops.set_dropout_seed(11 + step)
                loss = m2.training_step(b)
                loss.backward()
                m2.store.adamw_step(max_steps=10, grad_scale=1.0)
                losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        return losses, m2.store.flat.detach().clone(), m2.store.shadow.detach().clone()

    la, pa, sa = three_steps()
    lb, pb, sb = three_steps()
    assert all(torch.equal(x, y) for x, y in zip(la, lb)), (la, lb)
    assert torch.equal(pa, pb), f"{int((pa != pb).sum())} parameters differ after three steps"
    assert torch.equal(sa, sb)
    assert not torch.equal(pa, flat0)


@pytest.mark.parametrize("mode", ["fp32", "fp32x3"])
def test_tiny_step_is_bit_reproducible_in_the_fp32_modes(mode):
    cfg = tiny_config(compute_dtype=mode, drop_rate=0.1, deterministic=True)
    m = build(cfg, mode)
    b = to_dev(tiny_batch())
    m.set_task()
    with busy_second_stream() as kick:
        l0, g0 = _backward(m, b)
        assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
        for _ in range(3):
            kick()
            l1, g1 = _backward(m, b)
            assert torch.equal(l0, l1) and torch.equal(g0, g1), int((g0 != g1).sum())


def test_tiny_pretraining_step_is_bit_reproducible():
    """MLM + MIM + ITM (the settings of test_two_stream_schedule_equals_the_single_stream_step[pretrain]) under a fixed
    torch.manual_seed: vocabulary projection, padded-vocabulary wgrad, cross entropy, MIM loss, embedding gradients."""
    cfg = tiny_config(compute_dtype="bf16", deterministic=True, **PRETRAIN)
    b = to_dev(tiny_batch(pretrain=True))
    b["itm_labels"] = torch.tensor([1.0, 0.0])
    m = build(cfg, torch.bfloat16)
    m.set_task()
    with busy_second_stream() as kick:
        l0, g0 = _backward(m, b, two_streams=False)
        assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
        for two in (False, True, True):
            kick()
            l1, g1 = _backward(m, b, two_streams=two)
            assert torch.equal(l0, l1), (two, l0.item(), l1.item())
            assert torch.equal(g0, g1), (two, int((g0 != g1).sum()))
    m.two_streams = type(m).two_streams


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the reducer
# ---------------------------------------------------------------------------------------------------------------------------------
def test_grad_reducer_run_equals_the_reducer_free_run_bit_for_bit():
    """Three steps with FlatGradReducer attached over a one-rank RCCL group (fp32 buckets) against the reducer-free run, in
    deterministic mode: tests/test_gpu_model.py::test_grad_reducer_over_rccl_single_rank_group's comparison, as torch.equal.
    (A one-rank all-reduce is the identity, and NT_NO_PERSISTENT, which the reducer sets, only changes which workgroup computes a
    tile of the NT kernels, never the order of the sum inside it.)"""
    import torch.distributed as dist
    from m3ae_amd.ddp import FlatGradReducer
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29547")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    own_group = not dist.is_initialized()
    if own_group:
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        cfg = tiny_config(compute_dtype="bf16", deterministic=True)
        b = to_dev(tiny_batch())

        def run(with_reducer):
            m = build(cfg, torch.bfloat16)
            m.train()
            red = None
            if with_reducer:
                red = FlatGradReducer(m.store, bucket_bytes=128 << 10)
                red.world = 2                      # take the hook path; the group itself has one rank
                red.attach()
            losses = []
            try:
                for step in range(3):
                    m.store.zero_grad()
                    ops.set_dropout_seed(11 + step)
                    loss = m.training_step(b)
                    loss.backward()
                    if red is not None:
                        red.finish()
                    m.store.adamw_step(max_steps=10, grad_scale=1.0)
                    losses.append(loss.item())
            finally:
                if red is not None:
                    red.detach()
            return losses, m.store.flat.detach().clone(), m.store.shadow.detach().clone()

        l0, p0, s0 = run(False)
        l1, p1, s1 = run(True)
        assert l0 == l1, (l0, l1)
        assert torch.equal(p0, p1), f"{int((p0 != p1).sum())} parameters differ, max {float((p0 - p1).abs().max()):.3e}"
        assert torch.equal(s0, s1)
    finally:
        if own_group:
            dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. ops without an ordered form raise
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ops_without_an_ordered_form_raise_by_name():
    B, H, L, D = 2, 2, 32, 128
    q, k, v = (rnd(B, L, D, dtype=torch.bfloat16, seed=50 + i) for i in range(3))
    bias = rnd(H, L, L, seed=53)
    o, lse = ops.attn_forward(q, k, v, H, pos_bias=bias)
    do = rnd(B, L, D, dtype=torch.bfloat16, seed=54)
    dq, dk, dv = (torch.empty_like(t) for t in (q, k, v))
    dbias = torch.zeros_like(bias)
    ops.set_deterministic(True)
    with pytest.raises(ops.DeterministicError, match="d_pos_bias"):
        ops.attn_backward(q, k, v, o, lse, do, dq, dk, dv, H, pos_bias=bias, d_pos_bias=dbias)
    torch.cuda.synchronize()
    assert float(dbias.abs().max()) == 0.0                       # the atomic kernel did not run
    ops.attn_backward(q, k, v, o, lse, do, dq, dk, dv, H, pos_bias=bias)   # without the bias gradient: fine (no atomics)
    ops.set_deterministic(False)
    ops.attn_backward(q, k, v, o, lse, do, dq, dk, dv, H, pos_bias=bias, d_pos_bias=dbias)
    assert float(dbias.abs().max()) > 0.0


def test_fused_cross_attention_backward_raises_when_the_mode_comes_on_after_its_forward(monkeypatch):
    """With the mode on, training calls of the cross-attention sub-block take the composition (the bit-equal steps above would
    raise otherwise).  A fused forward taken with the mode OFF cannot be differentiated with the mode ON: m3ae_xattn_bwd sums its
    weight gradients with fp32 atomics, so the backward raises instead of running it.  (Full last fusion pair, ops.CLS_ONLY off:
    the fused backward is then the first op of the backward without an ordered form.)  The same holds for the live-row form of
    the last pair: its LayerNorm backward under a dropout row map has no ordered form either, and raises where it used to run
    the atomic kernel."""
    cfg = finetune_vqa_rad_config(compute_dtype="bf16")
    b = to_dev(synth.synthetic_batch(2, text_len=32, image_size=384, rank=0))
    m = build(cfg, torch.bfloat16)
    m.set_task()
    m.train()
    m.store.zero_grad()
    calls = []
    real = ops.xattn_fwd
    monkeypatch.setattr(ops, "xattn_fwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ops, "CLS_ONLY", False)
    loss = m.training_step(b)
    assert len(calls) > 0                       # mode off: the fused training path (the suite lowers its batch threshold to 0)
    ops.set_deterministic(True)
    with pytest.raises(ops.DeterministicError, match="m3ae_xattn_bwd"):
        loss.backward()
    torch.cuda.synchronize()
    n = len(calls)
    m.store.zero_grad()
    m.training_step(b).backward()               # mode on from the forward on: the composition, no fused call, no error
    torch.cuda.synchronize()
    assert len(calls) == n
    ops.set_deterministic(False)
    monkeypatch.setattr(ops, "CLS_ONLY", True)
    m.store.zero_grad()
    loss = m.training_step(b)                   # mode off: the last pair in its live-row form
    ops.set_deterministic(True)
    with pytest.raises(ops.DeterministicError, match="row map"):
        loss.backward()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. mode off is today's path
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mode_off_is_the_default_path(monkeypatch):
    """After a deterministic step and set_deterministic(False): the forward logits of a fixed batch equal those computed before
    the mode was ever switched on, bit for bit, and a default step never asks for a deterministic workspace (calls counted
    through the binding) while a deterministic step does."""
    cfg = tiny_config(compute_dtype="bf16", drop_rate=0.1)
    b = to_dev(tiny_batch())
    m = build(cfg, torch.bfloat16)
    m.set_task()
    assert ops.deterministic() is False
    with torch.no_grad():
        before = m(b)["vqa_logits"].float().clone()
    _, g_default = _backward(m, b)

    L = _lib.lib()
    counts = {"gemm": 0, "small": 0}

    class Counting:
        """The loaded library with the two size queries counted (ops reaches every entry point through _lib.lib())."""
        def __getattr__(self, name):
            fn = getattr(L, name)
            if name == "m3ae_gemm_det_workspace_bytes":
                def counted(*a):
                    counts["gemm"] += 1
                    return fn(*a)
                return counted
            if name == "m3ae_det_workspace_bytes":
                def counted(*a):
                    counts["small"] += 1
                    return fn(*a)
                return counted
            if name.endswith("_det"):
                counts[name] = counts.get(name, 0) + 1
            return fn
    monkeypatch.setattr(_lib, "_lib", Counting())

    _backward(m, b)
    assert counts == {"gemm": 0, "small": 0}, counts       # default step: not one deterministic entry point touched
    ops.set_deterministic(True)
    _, g_det = _backward(m, b)
    assert counts["gemm"] > 0 and counts["small"] > 0 and counts.get("m3ae_gemm_det", 0) > 0, counts
    ops.set_deterministic(False)
    seen = dict(counts)
    _, g_after = _backward(m, b)
    assert counts == seen, (seen, counts)
    m.eval()
    with torch.no_grad():
        after = m(b)["vqa_logits"].float()
    assert torch.equal(before, after)
    assert torch.isfinite(g_det).all() and g_det.abs().max().item() > 0
    # back on the atomic kernels: the default step's gradient up to the order of its fp32 atomics (the bound of
    # tests/test_gpu_model.py::test_two_stream_schedule_equals_the_single_stream_step)
    rel = ((g_after - g_default).double().norm() / g_default.double().norm()).item()
    assert rel <= 1e-5, rel
