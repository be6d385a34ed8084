"""GPU: LoRA in merged form (config key `lora_rank`): m3ae_lora_merge / m3ae_lora_grad (csrc/lora.hip) against the numpy model and
exact float64 (tests/lora_model.py: operation order, bounds and their derivation), LoraAdapters on the tiny model, adapter files, the
trainer's checkpoints and resume, the refusals.  Every test fails without the feature: m3ae_amd.lora and the entry points do not
exist there."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, lora, ops, synth  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from m3ae_amd.param_store import PackedParam  # noqa: E402
from oracle_util import tiny_batch, tiny_config  # noqa: E402
import lora_model as LM  # noqa: E402

G = LM.GUARD


@pytest.fixture(autouse=True)
def _deterministic_mode_off_afterwards():
    yield
    ops.set_deterministic(False)      # (a model built with deterministic=True switches the process-wide mode on)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def guarded(values=None, n=None, dtype=torch.float32):
    """(whole, view): a device buffer of n elements (or a copy of `values`) between two guards of SENTINEL."""
    n = len(values) if values is not None else n
    whole = torch.full((n + 2 * G,), float(LM.SENTINEL), dtype=dtype, device="cuda")
    if values is not None:
        whole[G:G + n].copy_(torch.from_numpy(np.array(values)).to("cuda"))
    return whole, whole[G:G + n]


def guards_intact(whole):
    s = torch.tensor(float(LM.SENTINEL), dtype=whole.dtype, device="cuda")
    return bool((whole[:G] == s).all() and (whole[-G:] == s).all())


@functools.lru_cache(maxsize=None)
def reference(r):
    """The case of rank r with the model's and float64's results per target, computed once and shared; nobody writes to it."""
    c = LM.case(r)
    out = []
    for i in range(len(c["recs"])):
        W0, A, B, dW = LM.parts(c, i)
        out.append(dict(merge=LM.merge(W0, A, B, c["s"]), merge_exact=LM.merge_exact(W0, A, B, c["s"]), merge_bound=LM.merge_bound(W0, A, B, c["s"]),
                        grad=LM.grad(dW, A, B, c["s"]), grad_exact=LM.grad_exact(dW, A, B, c["s"]), grad_bound=LM.grad_bound(dW, A, B, c["s"])))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c, out


def table_of(c):
    return lora.LoraTable(c["recs"], c["r"], c["sizes"], "cuda")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. merge, kernel level: one launch over the table of LM.SHAPES
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", LM.RANKS)
def test_merge_with_zero_B_returns_the_base_bits_and_the_cast_shadow(r):
    c, _ = reference(r)
    tab = table_of(c)
    lz = c["lora"].copy()
    for off, N, K, a, b, bo in c["recs"]:
        lz[b:b + N * r] = 0.0
    (bw, base), (lw, lo) = guarded(c["base"]), guarded(lz)
    (fw, flat), (sw, shadow) = guarded(n=c["sizes"]["flat"]), guarded(n=c["sizes"]["flat"], dtype=torch.bfloat16)
    tab.merge(c["s"], base, lo, flat, shadow, 0, stream())
    torch.cuda.synchronize()
    for off, N, K, a, b, bo in c["recs"]:
        assert same_bits(flat[off:off + N * K], base[bo:bo + N * K]), (N, K)
        src = base[bo:bo + N * K].clone()
        dst = torch.empty(N * K, dtype=torch.bfloat16, device="cuda")
        _lib.check(_lib.lib().m3ae_cast(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), N * K, _lib.F32, _lib.BF16, stream()), "m3ae_cast")
        assert same_bits(shadow[off:off + N * K], dst), (N, K)


@pytest.mark.parametrize("with_shadow", [True, False], ids=["shadow", "no_shadow"])
@pytest.mark.parametrize("r", LM.RANKS)
def test_merge_is_the_model_bit_for_bit_inside_the_bound_and_writes_nothing_else(r, with_shadow):
    c, ref = reference(r)
    tab = table_of(c)
    (bw, base), (lw, lo) = guarded(c["base"]), guarded(c["lora"])
    (fw, flat), (sw, shadow) = guarded(n=c["sizes"]["flat"]), guarded(n=c["sizes"]["flat"], dtype=torch.bfloat16)
    tab.merge(c["s"], base, lo, flat, shadow if with_shadow else None, 0, stream())
    torch.cuda.synchronize()
    got, sh = flat.cpu().numpy(), shadow.view(torch.int16).cpu().numpy().view(np.uint16)
    worst = 0.0
    for (off, N, K, a, b, bo), want in zip(c["recs"], ref):
        w = got[off:off + N * K].reshape(N, K)
        err = np.abs(w.astype(np.float64) - want["merge_exact"])
        worst = max(worst, float((err / want["merge_bound"]).max()))
        assert (err <= want["merge_bound"]).all(), (N, K)
        # the order fixes every bit: r + 1 fmafs, modelled with a single rounding each
        assert np.array_equal(w.view(np.uint32), want["merge"].view(np.uint32)), (N, K)
        if with_shadow:
            assert np.array_equal(sh[off:off + N * K], LM.bf16_bits(w.reshape(-1))), (N, K)      # RNE bf16 of the fp32 written
    print(f"merge r={r}: largest error / bound {worst:.3f}")
    # padding between the targets, the guards, and the inputs
    pad = ~LM.in_target_mask(c["recs"], c["sizes"]["flat"], "flat")
    assert pad.any() and (got[pad] == LM.SENTINEL).all()
    sent16 = LM.bf16_bits(np.array([LM.SENTINEL], np.float32))[0]
    assert (sh[pad] == sent16).all() and (with_shadow or (sh == sent16).all())
    assert guards_intact(fw) and guards_intact(sw) and guards_intact(bw) and guards_intact(lw)
    assert np.array_equal(base.cpu().numpy(), c["base"]) and np.array_equal(lo.cpu().numpy(), c["lora"])


@pytest.mark.parametrize("r", [3, 64])
def test_merge_mode_1_returns_the_base_bits_whatever_the_adapters_hold(r):
    c, _ = reference(r)
    tab = table_of(c)
    li = np.full_like(c["lora"], np.inf)
    (bw, base), (lw, lo) = guarded(c["base"]), guarded(li)
    (fw, flat), (sw, shadow) = guarded(n=c["sizes"]["flat"]), guarded(n=c["sizes"]["flat"], dtype=torch.bfloat16)
    tab.merge(c["s"], base, lo, flat, shadow, 1, stream())
    for off, N, K, a, b, bo in c["recs"]:
        assert same_bits(flat[off:off + N * K], base[bo:bo + N * K])
        assert np.array_equal(shadow[off:off + N * K].view(torch.int16).cpu().numpy().view(np.uint16), LM.bf16_bits(c["base"][bo:bo + N * K]))
    tab.merge(c["s"], base, None, flat, None, 1, stream())           # mode 1 reads no adapters: a NULL buffer is accepted
    torch.cuda.synchronize()
    assert guards_intact(fw) and guards_intact(sw)
    pad = ~LM.in_target_mask(c["recs"], c["sizes"]["flat"], "flat")
    assert (flat.cpu().numpy()[pad] == LM.SENTINEL).all()


def test_bad_arguments_are_refused_before_any_launch():
    c, _ = reference(3)
    tab = table_of(c)
    L = _lib.lib()
    base, lo, flat = (torch.zeros(c["sizes"][k], device="cuda") for k in ("base", "lora", "flat"))
    t, s = C.c_void_p(tab.dev.data_ptr()), stream()
    p = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
    assert L.m3ae_lora_merge(t, tab.n, 0, 1.0, p(base), p(lo), p(flat), None, 0, s) == _lib.ERR_ARG
    assert L.m3ae_lora_merge(t, tab.n, 65, 1.0, p(base), p(lo), p(flat), None, 0, s) == _lib.ERR_UNSUPPORTED
    assert L.m3ae_lora_merge(t, 513, 3, 1.0, p(base), p(lo), p(flat), None, 0, s) == _lib.ERR_UNSUPPORTED
    assert L.m3ae_lora_merge(t, tab.n, 3, 1.0, p(base), p(lo), p(flat), None, 2, s) == _lib.ERR_ARG
    assert L.m3ae_lora_merge(t, tab.n, 3, float("inf"), p(base), p(lo), p(flat), None, 0, s) == _lib.ERR_ARG
    assert L.m3ae_lora_merge(t, tab.n, 3, 1.0, p(base), None, p(flat), None, 0, s) == _lib.ERR_ARG
    assert L.m3ae_lora_merge(t, tab.n, 3, 1.0, C.c_void_p(base.data_ptr() + 4), p(lo), p(flat), None, 0, s) == _lib.ERR_ALIGN
    assert L.m3ae_lora_grad(t, tab.n, 3, 1.0, p(lo), p(flat), p(lo), None, s) == _lib.ERR_WORKSPACE
    assert L.m3ae_lora_grad(t, tab.n, 3, float("nan"), p(lo), p(flat), p(lo), p(tab.workspace), s) == _lib.ERR_ARG
    assert L.m3ae_lora_grad(t, tab.n, 3, 1.0, p(lo), C.c_void_p(flat.data_ptr() + 8), p(lo), p(tab.workspace), s) == _lib.ERR_ALIGN
    torch.cuda.synchronize()
    assert not flat.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. projection, kernel level: the same tables.  N = 512 at the kernel's panel size of 64 rows (LM.PANEL == _lib.LORA_PANEL_ROWS) is 8
#    row panels: the fold runs over 8 planes; N = 130 is 3 planes with a partial last panel; K = 70 and 72 leave a partial last chunk
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", LM.RANKS)
def test_projection_is_the_model_inside_the_bound_overwrites_and_repeats_bit_for_bit(r):
    assert LM.PANEL == _lib.LORA_PANEL_ROWS == 64 and max(N for N, _ in LM.SHAPES) // LM.PANEL == 8
    c, ref = reference(r)
    tab = table_of(c)
    (lw, lo), (gw, gr) = guarded(c["lora"]), guarded(c["grad"])
    (ow, out), (ww, ws) = guarded(n=c["sizes"]["lora"]), guarded(n=max(tab.ws_bytes // 4, 1))
    out.fill_(3.0e38)                                       # were the outputs accumulated, this would show
    in_lora = LM.lora_mask(c["recs"], c["sizes"]["lora"], r)
    out[torch.from_numpy(~in_lora).to("cuda")] = float(LM.SENTINEL)
    tab.grad(c["s"], lo, gr, out, stream(), workspace=ws)
    first = out.clone()
    ws.fill_(float("nan"))                                  # the workspace carries nothing from call to call
    tab.grad(c["s"], lo, gr, out, stream(), workspace=ws)
    torch.cuda.synchronize()
    assert same_bits(first, out)                            # two runs, the same bits
    got = out.cpu().numpy()
    worst = [0.0, 0.0]
    for (off, N, K, a, b, bo), want in zip(c["recs"], ref):
        dA, dB = got[a:a + r * K].reshape(r, K), got[b:b + N * r].reshape(N, r)
        for k, (g, m, e, lim) in enumerate(zip((dA, dB), want["grad"], want["grad_exact"], want["grad_bound"])):
            err = np.abs(g.astype(np.float64) - e)
            assert (err <= lim).all(), (N, K, "dA dB".split()[k])
            worst[k] = max(worst[k], float((err / lim).max()))
            assert np.array_equal(g.view(np.uint32), m.view(np.uint32)), (N, K, "dA dB".split()[k])      # the order fixes every bit
    print(f"projection r={r}: largest error / bound  dA {worst[0]:.3f}  dB {worst[1]:.3f}")
    assert (got[~in_lora] == LM.SENTINEL).all()             # padding of the output
    assert guards_intact(ow) and guards_intact(ww) and guards_intact(lw) and guards_intact(gw)
    assert np.array_equal(gr.cpu().numpy(), c["grad"]) and np.array_equal(lo.cpu().numpy(), c["lora"])


def test_a_nan_in_the_weight_gradient_reaches_both_adapter_gradients():
    r = 3
    c, _ = reference(r)
    tab = table_of(c)
    g = c["grad"].copy()
    hit = []
    for off, N, K, a, b, bo in c["recs"]:
        n, k = N // 2, K // 3
        g[off + n * K + k] = np.nan
        hit.append((n, k))
    lo, gr = torch.from_numpy(c["lora"].copy()).to("cuda"), torch.from_numpy(g).to("cuda")
    out = torch.zeros(c["sizes"]["lora"], device="cuda")
    tab.grad(c["s"], lo, gr, out, stream())
    got = out.cpu().numpy()
    for (off, N, K, a, b, bo), (n, k) in zip(c["recs"], hit):
        dA, dB = got[a:a + r * K].reshape(r, K), got[b:b + N * r].reshape(N, r)
        assert np.isnan(dA[:, k]).all() and np.isnan(dB[n, :]).all()
        assert np.isnan(dA).sum() == r and np.isnan(dB).sum() == r           # ... and nothing else


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the adapters on the tiny model
# ---------------------------------------------------------------------------------------------------------------------------------
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


class StubTrainer:
    max_steps = 40


def build(mode="fp32", attach=True, **over):
    over.setdefault("learning_rate", 1e-3)
    cfg = tiny_config(compute_dtype=mode, deterministic=True, drop_rate=0.0, **over)
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16 if mode == "bf16" else torch.float32)
    m.eval()
    m.trainer_ref = StubTrainer()
    if attach and cfg["lora_rank"] > 0:
        m.attach_lora()
    return m


def step(m, b):
    m.store.zero_grad()
    loss = m.training_step(b)
    loss.backward()
    m.store.optimizer_step(max_steps=40, lr_factor=1.0)
    return loss.detach().clone()


def logits(m, b):
    m.set_task()
    with torch.no_grad():
        return m(b)["vqa_logits"].float().clone()


def device_copies(m):
    st = m.store
    out = {"flat": st.flat, "shadow": st.shadow}
    for i, u in enumerate(st.units):
        out[f"t{i}"] = getattr(u, "m3ae_t", None)
        out[f"tt{i}"] = getattr(u, "m3ae_tt", None)
        out[f"tb{i}"] = u.m3ae_tb if isinstance(u, PackedParam) else getattr(getattr(u, "m3ae_c", None), "m3ae_tb", None)
    return {k: v for k, v in out.items() if v is not None}


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_attaching_changes_no_bit_and_the_first_step_moves_only_B_and_the_heads(mode):
    b = to_dev(tiny_batch())
    plain, m = build(mode, lora_rank=0), build(mode, lora_rank=8, attach=False)
    before = {k: v.clone() for k, v in device_copies(m).items()}
    want = logits(plain, b)
    ad = m.attach_lora()
    assert m.lora is ad is m.store.lora and plain.lora is None
    torch.cuda.synchronize()
    for k, v in device_copies(m).items():
        assert same_bits(v, before[k]), k                                  # B = 0: the merge rewrites the base bits
    assert torch.equal(logits(m, b), want)
    st, base0, lora0 = m.store, ad.base.clone(), ad.lora.clone()
    flat0 = st.flat.clone()
    l_a, l_b = step(m, b), step(plain, b)                                   # the twin takes a full fine-tuning step from the same weights
    torch.cuda.synchronize()
    assert same_bits(l_a.float().reshape(1), l_b.float().reshape(1))       # forward and backward were identical
    assert torch.equal(st.grad, plain.store.grad)
    target_ids = {id(p) for p in ad.params}
    moved = 0
    for gi in range(6):
        for n, p in st.groups[gi]:
            o, cnt = st.offset[id(p)], p.numel()
            mine, twin, old = st.flat[o:o + cnt], plain.store.flat[o:o + cnt], flat0[o:o + cnt]
            if gi in (2, 3):
                assert same_bits(mine, twin), n                             # heads: the ordinary rule, bit for bit
                moved += int(not torch.equal(mine, old))
            elif id(p) not in target_ids:
                assert same_bits(mine, old), n                              # norms, biases, embeddings: untouched
    assert moved > 0 and same_bits(st.flat[st.trainable_end:], flat0[st.trainable_end:])
    assert same_bits(ad.base, base0)
    # every target equals the merge recomputed on copies of base and the stepped adapters; dA = s B^T dW is exactly zero while
    # B = 0, so only B moves (but for AdamW's decoupled decay of A itself, lr * wd * A: see the next test, which runs without decay)
    flat2, sh2 = torch.zeros_like(st.flat), None if st.shadow is None else torch.zeros_like(st.shadow)
    ad.table.merge(ad.scale, ad.base.clone(), ad.lora.clone(), flat2, sh2, 0, stream())
    changed = 0
    for i, (off, N, K, a, bb, bo) in enumerate(ad.records):
        assert same_bits(st.flat[off:off + N * K], flat2[off:off + N * K]), ad.names[i]
        if sh2 is not None:
            assert same_bits(st.shadow[off:off + N * K], sh2[off:off + N * K]), ad.names[i]
        A, B = ad.views(i)
        A0, _ = ad.views(i, lora0)
        assert not ad.views(i, ad.lora_grad)[0].any(), ad.names[i]          # dA is exactly zero
        changed += int(bool(B.any()))
        if st.cfg["weight_decay"] == 0:
            assert same_bits(A, A0), ad.names[i]
    assert changed == len(ad.records)
    if mode == "bf16":                                                      # shadow == bf16(flat) and the copies agree with the shadow
        clone = {k: v.clone() for k, v in device_copies(m).items()}
        st.sync_shadows()
        torch.cuda.synchronize()
        for k, v in device_copies(m).items():
            assert same_bits(v, clone[k]), k


def test_the_first_step_leaves_A_bit_for_bit_without_weight_decay():
    b = to_dev(tiny_batch())
    m = build("fp32", lora_rank=4, weight_decay=0.0)
    ad, lora0 = m.lora, m.lora.lora.clone()
    step(m, b)
    for i in range(len(ad.records)):
        assert same_bits(ad.views(i)[0], ad.views(i, lora0)[0]) and ad.views(i)[1].any()


@pytest.mark.parametrize("rule", ["adamw", "adam", "sgd"])
def test_thirty_steps_on_one_batch_lower_the_loss(rule):
    """Base learning rate 1e-5, the fine-tuning default (heads x100 = 1e-3, adapters x10 = 1e-4).  With a fixed batch, no dropout and
    deterministic kernels the objective is a fixed smooth function.  It starts far from its optimum: freshly initialised 498-way
    logits near 0 against targets that are almost all 0, a summed BCE near 498 ln 2.  Under adamw / adam every head weight moves by
    about 1e-3 per step, so a logit (256 features of order 1) moves by a few tenths per step at most -- 30 steps walk toward the
    targets without overshooting them; under sgd the head's effective rate 1e-3 / (1 - 0.9) = 1e-2 is below 2 / L for the head's
    curvature L <= 0.25 * |features|^2 ~ 64.  The adapters at 1e-4 move the towers by far less than the head moves the logits.  So a
    working implementation ends below its start; one whose head or adapter update has the wrong sign or scale does not."""
    b = to_dev(tiny_batch())
    m = build("fp32", lora_rank=8, optim_type=rule, learning_rate=1e-5)
    losses = [float(step(m, b)) for _ in range(30)]
    print(f"lora {rule}: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert all(m.lora.views(i)[1].any() for i in range(len(m.lora.records)))


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_disabled_is_the_base_model_and_leaving_restores_every_bit(mode):
    b = to_dev(tiny_batch())
    plain, m = build(mode, lora_rank=0), build(mode, lora_rank=8)
    for _ in range(3):
        step(m, b)
    torch.cuda.synchronize()
    ad, st = m.lora, m.store
    before = {k: v.clone() for k, v in device_copies(m).items()}
    merged = logits(m, b)
    with ad.disabled() as inside:
        assert inside is ad and not torch.is_grad_enabled()
        off = logits(m, b)
        with pytest.raises(RuntimeError, match="disabled"):
            st.optimizer_step(max_steps=40, lr_factor=1.0)
        with pytest.raises(RuntimeError, match="disabled"):
            with ad.disabled():
                pass
    # the heads have moved, so the base model here is the plain model with this model's heads
    for n, p in ad.head_items():
        dict(plain.named_parameters())[n].data.copy_(p.data)
    plain.store.sync_shadows()
    assert torch.equal(off, logits(plain, b)) and not torch.equal(off, merged)
    torch.cuda.synchronize()
    for k, v in device_copies(m).items():
        assert same_bits(v, before[k]), k
    with pytest.raises(KeyError):
        with ad.disabled():
            raise KeyError("inside")
    for k, v in device_copies(m).items():
        assert same_bits(v, before[k]), k
    assert torch.equal(logits(m, b), merged)


def test_adapter_file_round_trip_and_the_merged_state_dict(tmp_path):
    b = to_dev(tiny_batch())
    m = build("fp32", lora_rank=8)
    for _ in range(3):
        step(m, b)
    want = logits(m, b)
    path = str(tmp_path / "a.lora.pt")
    torch.save(m.lora.state_dict(), path)
    fresh = build("fp32", lora_rank=8, attach=False)                         # the same base
    fresh.attach_lora(path)
    assert torch.equal(logits(fresh, b), want) and torch.equal(fresh.store.flat, m.store.flat)
    merged = build("fp32", lora_rank=0)                                      # the ordinary state_dict holds the merged weights
    merged.load_state_dict(m.state_dict(), strict=False)
    merged.store.sync_shadows()
    assert torch.equal(logits(merged, b), want)
    other = build("fp32", lora_rank=8, attach=False)                         # a different base
    with torch.no_grad():
        other.multi_modal_vision_proj.weight.data[0, 0] += 0.25
    keep = other.store.flat.clone()
    with pytest.raises(ValueError, match="multi_modal_vision_proj"):
        other.attach_lora(path)
    assert torch.equal(other.store.flat, keep)


def test_adapter_file_is_under_5_percent_of_the_full_state_dict_at_rank_8(tmp_path):
    """Measured: 0.0140 (184320 adapter elements and 194290 head elements in the file)."""
    m = build("fp32", lora_rank=8)
    path, full = str(tmp_path / "a.lora.pt"), str(tmp_path / "full.pt")
    torch.save(m.lora.state_dict(), path)
    torch.save({k: v.detach().cpu() for k, v in m.state_dict().items()}, full)
    ratio = os.path.getsize(path) / os.path.getsize(full)
    heads = sum(p.numel() for _, p in m.lora.head_items())
    print(f"adapter file / full state_dict at r = 8 on the tiny model: {ratio:.4f} ({m.lora.elements} adapter elements, {heads} head elements)")
    assert ratio < 0.05


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. trainer: checkpoints, the adapter-only file, resume
# ---------------------------------------------------------------------------------------------------------------------------------
TINY = ("image_size=64 hidden_size=128 num_heads=2 num_top_layer=2 input_image_embed_size=128 input_text_embed_size=128 "
        "vocab_size=1000 vit_width=128 vit_layers=3 text_hidden=128 text_layers=2 text_heads=2 text_inter=512").split()


def make_trainer(tmp_path, tag, max_steps, *extra):
    from m3ae_amd import trainer
    dev = torch.device("cuda", 0)
    argv = (["with", "data_root=synthetic", "num_gpus=1", "num_nodes=1", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta",
             "per_gpu_batchsize=4", "batch_size=4", f"max_steps={max_steps}", "deterministic=True", "drop_rate=0.0", "learning_rate=0.001",
             "compute_dtype=fp32", "lora_rank=4", "exp_name=lora_run", "warmup_steps=0", f"log_dir={tmp_path / tag}", "seed=2"] + TINY + list(extra))
    cfg = trainer.config_mod.parse_cli(argv)
    torch.manual_seed(cfg["seed"])
    model = trainer.build_model(cfg, "cls", dev)
    for mod in model.modules():
        if hasattr(mod, "drop_rate"):
            mod.drop_rate = 0.0
    dm = trainer.SyntheticDataModule(cfg, 0, 1, dev, pool=1, train_samples=16, val_samples=8)
    return trainer.Trainer(cfg, model, dm, 0, 1, dev, log_every=1), model, cfg


def test_trainer_saves_the_adapters_and_resume_reproduces_the_next_step(tmp_path, capsys):
    tr, model, cfg = make_trainer(tmp_path, "run", 4)
    assert not tr.weights_only and model.lora is not None
    assert model.lora.describe() in capsys.readouterr().err                  # lora r=4 (n targets, m adapter elements)
    tr.plan["max_steps"] = 2
    tr.fit()
    torch.cuda.synchronize()
    last = str(tmp_path / "step2.ckpt")                                      # (the run that goes on overwrites last.ckpt)
    shutil.copy(os.path.join(tr.ckpt_dir, "last.ckpt"), last)
    flat_at_2, lora_at_2 = model.store.flat.clone(), model.lora.lora.clone()
    ck = torch.load(last, map_location="cpu", weights_only=False)
    assert "lora_state_dict" in ck and ck["lora_optimizer_state"]["exp_avg"].shape == (model.lora.total,)
    assert all(torch.equal(ck["state_dict"][k], v.detach().cpu()) for k, v in model.state_dict().items())      # the merged weights
    side = torch.load(os.path.join(tr.ckpt_dir, "last.lora.pt"), map_location="cpu", weights_only=False)
    assert set(side) == set(ck["lora_state_dict"]) and os.path.exists(os.path.join(tr.ckpt_dir, "best.lora.pt"))
    # steps 3 and 4 of the run that went on, against the same steps after a resume into a fresh model: the loss of step 3 reads the
    # restored weights, the loss of step 4 and the final buffers also the restored moments
    tr.plan["max_steps"] = 4
    tr.fit()
    torch.cuda.synchronize()
    want = [l for s, l in tr.history if s >= 3]
    tr2, model2, _ = make_trainer(tmp_path, "second", 4)
    tr2.resume(last)
    assert tr2.global_step == 2 and torch.equal(model2.store.flat, flat_at_2) and torch.equal(model2.lora.lora, lora_at_2)
    tr2.fit()
    torch.cuda.synchronize()
    got = [l for s, l in tr2.history if s >= 3]
    assert len(want) == len(got) == 2 and [np.float64(x).tobytes() for x in want] == [np.float64(x).tobytes() for x in got]
    assert torch.equal(model2.store.flat, model.store.flat) and torch.equal(model2.lora.lora, model.lora.lora)
    # a weights-only run keeps the adapters and drops their moments; a checkpoint without adapters does not resume a LoRA run
    tr.weights_only = True
    wo = torch.load(tr.save("wo.ckpt"), map_location="cpu", weights_only=False)
    assert "lora_state_dict" in wo and "lora_optimizer_state" not in wo
    plain = str(tmp_path / "plain.ckpt")
    torch.save({k: v for k, v in wo.items() if not k.startswith("lora_")}, plain)
    with pytest.raises(ValueError, match="lora_state_dict"):
        tr2.resume(plain)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_five_refusals():
    from m3ae_amd import trainer
    from m3ae_amd.ddp import FlatGradReducer
    from m3ae_amd.graph import GraphedStep
    b = to_dev(tiny_batch())
    m = build("bf16", lora_rank=4)
    with pytest.raises(ValueError, match="lora_rank"):
        GraphedStep(m, b, 10)
    with pytest.raises(ValueError, match="lora_rank"):
        FlatGradReducer(m.store, update_in_backward=True).arm_update()
    assert m.store.step_count == 0
    for over, what in ((dict(ema_decay=0.5), "ema_decay"), (dict(gradient_clip_val=1.0), "gradient_clip_val")):
        x = build("fp32", lora_rank=4, attach=False, **over)
        with pytest.raises(ValueError, match=what):
            x.attach_lora()
        assert x.lora is None and x.store.lora is None
    for head in ("t5", "decoder"):
        with pytest.raises(ValueError, match="lora_rank"):
            trainer.build_model(tiny_config(lora_rank=4), head, torch.device("cuda", 0))
