"""Host side of LoRA (config keys lora_rank / lora_alpha / lora_targets / lora_lr_multiplier / lora_path; m3ae_amd/lora.py): the
validators, target selection, key naming, the base fingerprint, which calls a step makes -- the library replaced by a recorder --
and the numpy model of the kernels held to the bound derived from their operation order.  No GPU."""
import numpy as np
import pytest
import torch

from m3ae_amd import _lib, config, lora
import lora_model as LM


# ---------------------------------------------------------------------------------------------------------------------------------
# config
# ---------------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_off():
    cfg = config.tiny_config()
    assert cfg["lora_rank"] == 0 and cfg["lora_alpha"] == 16.0 and cfg["lora_targets"] == "all-linear"
    assert cfg["lora_lr_multiplier"] == 10.0 and cfg["lora_path"] == ""
    assert config.lora_rank({}) == 0


@pytest.mark.parametrize("v", [-1, 65, 1.0, 8.5, True, "8", None])
def test_a_bad_rank_is_refused(v):
    with pytest.raises(ValueError, match="lora_rank"):
        config.tiny_config(lora_rank=v)


@pytest.mark.parametrize("key", ["lora_alpha", "lora_lr_multiplier"])
@pytest.mark.parametrize("v", [0, -1.0, float("inf"), float("nan"), "16", None, True])
def test_a_bad_alpha_or_multiplier_is_refused(key, v):
    with pytest.raises(ValueError, match=key):
        config.tiny_config(lora_rank=4, **{key: v})


@pytest.mark.parametrize("v", ["all", "qkv", "", None, 3, ["attention"]])
def test_a_bad_target_name_is_refused(v):
    with pytest.raises(ValueError, match="lora_targets"):
        config.tiny_config(lora_targets=v)
    with pytest.raises(ValueError, match="lora_targets"):
        lora.target_names(None, v)


def test_the_keys_pass_through_the_command_line_grammar():
    cfg = config.parse_cli("with task_finetune_vqa_vqa_rad clip16 text_roberta lora_rank=8 lora_alpha=32 lora_targets=attention "
                           "lora_lr_multiplier=5 lora_path=a.lora.pt".split())
    assert cfg["lora_rank"] == 8 and cfg["lora_alpha"] == 32.0 and type(cfg["lora_alpha"]) is float
    assert cfg["lora_targets"] == "attention" and cfg["lora_lr_multiplier"] == 5.0 and cfg["lora_path"] == "a.lora.pt"
    with pytest.raises(ValueError, match="lora_rank"):
        config.parse_cli("with task_finetune_vqa_vqa_rad lora_rank=65".split())


# ---------------------------------------------------------------------------------------------------------------------------------
# target selection and key naming
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_selection(model, cfg):
    names = lora.target_names(model, "all-linear")
    params = dict(model.named_parameters())
    assert names and len(set(names)) == len(names)
    for n in names:
        assert params[n].dim() == 2, n
        assert not any(h in n for h in ("vqa_head", "mlm_head", "itm_head", "mim_head", "embeddings", "embedding", "conv1", "LayerNorm")), n
        assert not n.endswith("bias"), n
    L, T, F = len(model.vision_encoder.visual.transformer.resblocks), cfg["text_layers"], cfg["num_top_layer"]
    assert L == cfg["vit_layers"] - 1                                      # (the reference's CLIP tower stops one block early)
    fused = [n for n in names if n.endswith("attn.in_proj_weight")]
    assert len(fused) == L and all(tuple(params[n].shape) == (3 * cfg["vit_width"], cfg["vit_width"]) for n in fused)   # one target, N = 3D
    for kind in ("query", "key", "value"):                                 # members of a packed unit: three targets, own names
        own = [n for n in names if n.startswith("language_encoder") and n.endswith(f"attention.self.{kind}.weight")]
        assert len(own) == T and all(tuple(params[n].shape) == (cfg["text_hidden"], cfg["text_hidden"]) for n in own)
    # CLIP block: in_proj, out_proj, c_fc, c_proj; RoBERTa layer: q k v o + 2 FFN; fusion layer: 2 x (q k v o) + 2 FFN, two stacks;
    # the two modality projections and the two fusion poolers (RoBERTa's own pooler never trains)
    assert len(names) == 4 * L + 6 * T + 2 * F * 10 + 2 + 2, len(names)
    assert "language_encoder.pooler.dense.weight" not in names
    attn = lora.target_names(model, "attention")
    assert set(attn) < set(names) and len(attn) == 2 * L + 4 * T + 2 * F * 8
    keys = [lora.adapter_key(n) for n in names]
    assert len(set(keys)) == len(keys)                                      # the naming is injective: it round-trips
    assert all((k + ".weight" in params) or (k + "_weight" in params) for k in keys)
    assert lora.adapter_key(fused[0]).endswith("attn.in_proj") and lora.adapter_key("a.b.weight") == "a.b"
    return names


def test_target_selection_on_the_tiny_model():
    from m3ae_amd.modules import M3AETransformerSS
    cfg = config.tiny_config()
    _check_selection(M3AETransformerSS(cfg), cfg)


def test_target_selection_on_the_full_size_model_on_the_meta_device():
    from m3ae_amd.modules import M3AETransformerSS
    cfg = config.finetune_vqa_rad_config()
    with torch.device("meta"):
        model = M3AETransformerSS(cfg)
    names = _check_selection(model, cfg)
    assert len(names) == 44 + 72 + 120 + 4 <= _lib.LORA_MAX_TARGETS


# ---------------------------------------------------------------------------------------------------------------------------------
# the adapters on the host: layout, calls of a step, state dict, fingerprint -- the library replaced by a recorder
# ---------------------------------------------------------------------------------------------------------------------------------
class Recording:
    """Stands in for the loaded library: records (name, args) of every call and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


def _recorder(monkeypatch):
    from m3ae_amd import ops
    rec = Recording()
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(_lib, "lib", lambda: _lib._lib)
    return rec


def _cpu_model(**over):
    from m3ae_amd.modules import M3AETransformerSS
    torch.manual_seed(0)
    model = M3AETransformerSS(config.tiny_config(compute_dtype="fp32", **over))
    return model.finalize("cpu", "fp32")


def _val(x):
    return getattr(x, "value", x)


def _plain_step_calls(store, hyper):
    return [("m3ae_" + store.optim, store.flat.data_ptr() + 4 * a, min(b, store.trainable_end) - a, hyper["lrs"][gi])
            for gi, (a, b) in enumerate(store.segments[:6]) if min(b, store.trainable_end) > a]


@pytest.mark.parametrize("rule", ["adamw", "adam", "sgd"])
def test_key_off_a_step_makes_the_calls_it_made_before(monkeypatch, rule):
    rec = _recorder(monkeypatch)
    model = _cpu_model(optim_type=rule)
    st = model.store
    assert st.lora is None and model.lora is None
    hyper = st.begin_update(max_steps=10, lr_factor=1.0)
    st.update_apply(hyper)
    got = [(name, _val(a[0]), a[4] if rule == "sgd" else a[5], a[5] if rule == "sgd" else a[6]) for name, a in rec.calls]
    assert got == _plain_step_calls(st, hyper)             # one rule launch per non-empty group segment, nothing else (fp32: no copies)


@pytest.mark.parametrize("rule", ["adamw", "adam", "sgd"])
def test_key_on_the_step_is_projection_two_adapter_ranges_heads_merge(monkeypatch, rule):
    rec = _recorder(monkeypatch)
    model = _cpu_model(optim_type=rule, lora_rank=4, lora_lr_multiplier=3.0)
    st = model.store
    ad = lora.LoraAdapters(st, model)
    assert st.lora is ad and [n for n, _ in rec.calls] == ["m3ae_lora_grad_workspace_bytes"]      # attaching launches nothing
    rec.calls.clear()
    hyper = st.begin_update(max_steps=10, lr_factor=1.0)
    st.update_apply(hyper)
    names = [n for n, _ in rec.calls]
    heads = [gi for gi in (2, 3) if st.segments[gi][1] > st.segments[gi][0]]
    assert names == ["m3ae_lora_grad"] + ["m3ae_" + rule] * (2 + len(heads)) + ["m3ae_lora_merge"]
    n_at, lr_at = (4, 5) if rule == "sgd" else (5, 6)
    (_, g0), (_, g4) = rec.calls[1], rec.calls[2]
    assert _val(g0[0]) == ad.lora.data_ptr() and g0[n_at] == ad.split and _val(g0[1]) == ad.lora_grad.data_ptr()
    assert _val(g4[0]) == ad.lora.data_ptr() + 4 * ad.split and g4[n_at] == ad.total - ad.split
    assert g0[lr_at] == hyper["lrs"][0] * 3.0 and g4[lr_at] == hyper["lrs"][4] * 3.0
    assert g0[3 if rule == "sgd" else 4] is None                                   # the adapters have no bf16 shadow
    for (_, a), gi in zip(rec.calls[3:3 + len(heads)], heads):
        assert _val(a[0]) == st.flat.data_ptr() + 4 * st.segments[gi][0] and a[lr_at] == hyper["lrs"][gi]
    proj, mrg = rec.calls[0][1], rec.calls[-1][1]
    assert proj[1] == mrg[1] == len(ad.names) and proj[2] == mrg[2] == 4 and proj[3] == mrg[3] == 4.0 and mrg[8] == 0
    assert _val(proj[5]) == st.grad.data_ptr() and _val(proj[6]) == ad.lora_grad.data_ptr() and _val(mrg[6]) == st.flat.data_ptr()
    # inside disabled() the optimizer entry points raise, and the merges are mode 1 on entry and mode 0 on exit
    rec.calls.clear()
    with ad.disabled():
        with pytest.raises(RuntimeError, match="disabled"):
            st.begin_update(max_steps=10, lr_factor=1.0)
        with pytest.raises(RuntimeError, match="disabled"):
            st.update_apply(hyper)
        with pytest.raises(RuntimeError, match="disabled"):
            ad.state_dict()
    assert [(n, a[8]) for n, a in rec.calls] == [("m3ae_lora_merge", 1), ("m3ae_lora_merge", 0)]


def test_layout_init_and_table(monkeypatch):
    _recorder(monkeypatch)
    model = _cpu_model(lora_rank=3, seed=5)
    st = model.store
    before = st.flat.clone()
    ad = lora.LoraAdapters(st, model)
    assert torch.equal(st.flat, before)                                           # attaching writes no weight
    in0 = {id(p) for _, p in st.groups[0]}
    n0 = sum(id(p) in in0 for p in ad.params)
    assert 0 < n0 < len(ad.params) and all(id(p) in in0 for p in ad.params[:n0])   # group-0 targets first, then group 4
    assert ad.split == ad.records[n0][3] and ad.total % 64 == 0 and ad.split % 64 == 0
    for i, (name, p, (off, N, K, a, b, bo)) in enumerate(zip(ad.names, ad.params, ad.records)):
        assert off == st.offset[id(p)] and (N, K) == tuple(p.shape) and a % 64 == b % 64 == bo % 64 == 0
        A, B = ad.views(i)
        assert torch.equal(A, lora.init_A(name, 3, K, 5)) and float(A.abs().max()) <= K ** -0.5 and not B.any()
        assert torch.equal(ad.base[bo:bo + N * K].view(N, K), p.data)
    assert not torch.equal(lora.init_A("x", 3, 16, 5), lora.init_A("y", 3, 16, 5))
    assert not torch.equal(lora.init_A("x", 3, 16, 5), lora.init_A("x", 3, 16, 6))
    assert ad.scale == 16.0 / 3 and ad.describe() == f"lora r=3 ({len(ad.names)} targets, {ad.elements} adapter elements)"
    assert ad.elements == sum(3 * (N + K) for _, N, K, _, _, _ in ad.records)
    with pytest.raises(ValueError, match="already"):
        lora.LoraAdapters(st, model)


def test_a_table_that_points_outside_its_buffers_is_refused(monkeypatch):
    _recorder(monkeypatch)
    recs, sizes = LM.layout(4)
    lora.LoraTable(recs, 4, sizes, "cpu")
    for what in ("flat", "lora", "base"):
        with pytest.raises(ValueError, match=what):
            lora.LoraTable(recs, 4, dict(sizes, **{what: sizes[what] - 128}), "cpu")
    bad = list(recs)
    bad[1] = (recs[1][0] + 2,) + recs[1][1:]
    with pytest.raises(ValueError, match="misaligned"):
        lora.LoraTable(bad, 4, dict(sizes, flat=sizes["flat"] + 64), "cpu")
    bad[1] = (recs[0][0],) + recs[1][1:]
    with pytest.raises(ValueError, match="overlap"):
        lora.LoraTable(bad, 4, sizes, "cpu")
    for r in (0, 65):
        with pytest.raises(ValueError, match="rank"):
            lora.LoraTable(recs, r, sizes, "cpu")


def test_workspace_bytes_is_the_sum_of_the_planes():
    recs, _ = LM.layout(16)
    tab = np.asarray(recs, np.int64)
    import ctypes as C
    got = _lib.lib().m3ae_lora_grad_workspace_bytes(tab.ctypes.data_as(C.c_void_p), len(recs), 16)
    assert got == 4 * sum(-(-N // _lib.LORA_PANEL_ROWS) * 16 * K for _, N, K, _, _, _ in recs)
    assert _lib.LORA_PANEL_ROWS == LM.PANEL
    assert _lib.lib().m3ae_lora_grad_workspace_bytes(tab.ctypes.data_as(C.c_void_p), len(recs), 65) == _lib.ERR_UNSUPPORTED
    assert _lib.lib().m3ae_lora_grad_workspace_bytes(None, len(recs), 4) == _lib.ERR_ARG


def test_state_dict_keys_round_trip_and_mismatches_are_named(monkeypatch):
    _recorder(monkeypatch)
    model = _cpu_model(lora_rank=2)
    ad = lora.LoraAdapters(model.store, model)
    ad.lora.normal_()
    sd = ad.state_dict()
    params = dict(model.named_parameters())
    adapter_keys = [k for k in sd if k.endswith((".lora_A", ".lora_B"))]
    assert len(adapter_keys) == 2 * len(ad.names)
    for k in adapter_keys:                                                          # every key leads back to its weight
        prefix = k.rsplit(".", 1)[0]
        assert (prefix + ".weight" in params) != (prefix + "_weight" in params), k
    assert any(k.endswith("attn.in_proj.lora_A") for k in sd)
    heads = {n for n in params if "vqa_head" in n}
    assert heads and heads <= set(sd) and sd["lora_config"] == dict(rank=2, alpha=16.0, targets="all-linear")
    assert set(sd["base_fingerprint"]) == set(ad.names)
    for i, n in enumerate(ad.names):
        w = params[n].detach().double()
        assert sd["base_fingerprint"][n] == pytest.approx((float(w.sum()), float((w * w).sum())), rel=1e-12)
    # the same base takes the file back, bit for bit
    torch.manual_seed(0)
    twin = _cpu_model(lora_rank=2)
    ad2 = lora.LoraAdapters(twin.store, twin)
    ad2.load_state_dict(sd)
    assert torch.equal(ad2.lora, ad.lora)
    # another base, rank or target set: a ValueError that names the first mismatch, and nothing is written
    other = _cpu_model(lora_rank=2)
    with torch.no_grad():
        dict(other.named_parameters())[ad.names[3]].data[0, 0] += 0.5
    ad3 = lora.LoraAdapters(other.store, other)
    kept = ad3.lora.clone()
    with pytest.raises(ValueError, match=ad.names[3].replace(".", r"\.")):
        ad3.load_state_dict(sd)
    assert torch.equal(ad3.lora, kept)
    r4 = _cpu_model(lora_rank=4)
    with pytest.raises(ValueError, match="rank"):
        lora.LoraAdapters(r4.store, r4).load_state_dict(sd)
    att = _cpu_model(lora_rank=2, lora_targets="attention")
    with pytest.raises(ValueError, match="targets"):
        lora.LoraAdapters(att.store, att).load_state_dict(sd)
    with pytest.raises(ValueError, match="lora_config"):
        ad2.load_state_dict({k: v for k, v in sd.items() if k != "lora_config"})
    with pytest.raises(ValueError, match="lora_A"):
        ad2.load_state_dict({k: v for k, v in sd.items() if k != adapter_keys[0]})


def test_fingerprint_tolerates_reduction_order_and_nothing_else():
    assert lora.fingerprint_mismatch("w", (1.0, 4.0), (1.0 + 1e-12, 4.0 * (1 + 1e-12)), 100) is None
    assert "w" in lora.fingerprint_mismatch("w", (1.0, 4.0), (1.0, 4.0 * (1 + 1e-6)), 100)
    assert "w" in lora.fingerprint_mismatch("w", (1.0, 4.0), (1.001, 4.0), 100)


def test_refusals_on_the_host(monkeypatch):
    _recorder(monkeypatch)
    for over, what in ((dict(ema_decay=0.9), "ema_decay"), (dict(gradient_clip_val=1.0), "gradient_clip_val")):
        m = _cpu_model(lora_rank=2, **over)
        with pytest.raises(ValueError, match=what):
            m.attach_lora()
        assert m.store.lora is None
    from m3ae_amd import trainer
    for head in ("t5", "decoder"):
        with pytest.raises(ValueError, match="lora_rank"):
            trainer.build_model(config.tiny_config(lora_rank=2), head, "cpu")
    with pytest.raises(ValueError, match="lora_rank"):
        lora.refuse_wrapper(config.tiny_config(lora_rank=2), "the T5 wrapper")
    lora.refuse_wrapper(config.tiny_config(), "the T5 wrapper")
    m = _cpu_model(lora_rank=2)
    m.store.lora = object()
    from m3ae_amd.ddp import FlatGradReducer
    with pytest.raises(ValueError, match="lora_rank"):
        FlatGradReducer(m.store, update_in_backward=True).arm_update()
    from m3ae_amd.graph import GraphedStep
    with pytest.raises(ValueError, match="lora_rank"):
        GraphedStep(m, {}, 10)


# ---------------------------------------------------------------------------------------------------------------------------------
# the model of the kernels against float64, on the inputs tests/test_gpu_lora.py uses
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fma32_is_a_single_rounding():
    a, b, c = np.float32(2.0 ** -30), np.float32(2.0 ** -30), np.float32(1.0 + 2.0 ** -23)
    assert LM.fma32(a, b, c) == c                                      # far below half an ulp
    a, b, c = np.float32(2.0 ** -12 + 2.0 ** -30), np.float32(2.0 ** -12), np.float32(1.0)
    assert LM.fma32(a, b, c) == np.float32(1.0 + 2.0 ** -23)           # 1 + 2^-24 + 2^-42: float64 holds it, above the tie -> up
    x = np.float32(1.0 + 2.0 ** -12)            # x * x = 1 + 2^-11 + 2^-24: a rounded product would lose the last term, fmaf keeps it
    assert float(LM.fma32(x, x, np.float32(-1.0))) == 2.0 ** -11 + 2.0 ** -24 != float(x * x - np.float32(1.0))
    p, q = np.float32(1.0 + 2.0 ** -12), np.float32(2.0 ** -12)        # p q = 2^-12 + 2^-24: with c = 1 an exact tie, which goes to even
    assert LM.fma32(p, q, np.float32(1.0)) == np.float32(1.0 + 2.0 ** -12)
    rng = np.random.default_rng(0)
    a, b, c = (LM.spread(rng, 4096, -10, 10) for _ in range(3))
    from fractions import Fraction
    got = LM.fma32(a, b, c)
    for i in range(0, 4096, 37):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))


@pytest.mark.parametrize("r", LM.RANKS)
def test_the_model_sits_inside_the_derived_bounds(r):
    """The model alone against float64: a bound the model missed would say nothing about the kernel.  Prints the largest observed
    error over bound (DESIGN.md section 4 quotes them)."""
    c = LM.case(r)
    worst = dict(merge=0.0, dA=0.0, dB=0.0)
    for i in range(len(c["recs"])):
        W0, A, B, dW = LM.parts(c, i)
        for x in (W0, A, B, dW):
            assert np.isfinite(x).all() and (np.abs(x) >= 2.0 ** -21).all() and (x.size < 64 or ((x > 0).any() and (x < 0).any()))
        err, lim = np.abs(LM.merge(W0, A, B, c["s"]).astype(np.float64) - LM.merge_exact(W0, A, B, c["s"])), LM.merge_bound(W0, A, B, c["s"])
        assert (err <= lim).all()
        worst["merge"] = max(worst["merge"], float((err / lim).max()))
        (dA, dB), (eA, eB), (bA, bB) = LM.grad(dW, A, B, c["s"]), LM.grad_exact(dW, A, B, c["s"]), LM.grad_bound(dW, A, B, c["s"])
        assert (np.abs(dA - eA) <= bA).all() and (np.abs(dB - eB) <= bB).all()
        worst["dA"] = max(worst["dA"], float((np.abs(dA - eA) / bA).max()))
        worst["dB"] = max(worst["dB"], float((np.abs(dB - eB) / bB).max()))
        zero = np.zeros_like(B)
        assert np.array_equal(LM.merge(W0, A, zero, c["s"]).view(np.uint32), W0.view(np.uint32))       # B = 0: W0 bit for bit
        dA0, _ = LM.grad(dW, A, zero, c["s"])
        assert not dA0.any()                                                                          # ... and dA = 0: only B moves first
    print(f"lora model r={r}: largest error / bound  merge {worst['merge']:.3f}  dA {worst['dA']:.3f}  dB {worst['dB']:.3f}")
