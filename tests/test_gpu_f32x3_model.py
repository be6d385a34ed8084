"""GPU: fp32x3 mode (compute_dtype="fp32x3") end to end: the reference fixtures at parity-mode tolerances, no GEMM left on the
generic fp32 kernel in forward or backward, and a parity-mode model in the same process unaffected."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import ops, synth  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from oracle_util import finetune_vqa_rad_config, full_batch, load_golden, tiny_batch, tiny_config  # noqa: E402


def to_dev(batch, dev="cuda"):
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to(dev)
        elif isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            out[k] = [t.to(dev) for t in v]
        else:
            out[k] = v
    return out


def build(cfg):
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.float32)
    m.eval()
    return m


def grad_worst(named, g, rtol, floor):
    params = dict(named)
    gn = float(g["global_grad_norm"]) if "global_grad_norm" in g else 0.0
    worst = (0.0, "")
    for n, r in zip(g["grad_names"].tolist(), g["grad_norm"]):
        mine = params[n].grad.double().norm().item()
        err = abs(mine - r)
        if err > rtol * r + floor * gn:
            worst = max(worst, (err / (r + 1e-30), f"{n}: {mine:.6e} vs {r:.6e}"))
    return worst


def test_full_size_fp32x3_logits_and_gradients_within_the_parity_contract():
    """configs[1] dims, B = 2: logits rtol 1e-3 and per-parameter gradient norms rtol 2e-3 against the reference fixture, with
    every GEMM and attention product on the fp32x3 kernel (no generic GEMM in forward or backward)."""
    cfg = finetune_vqa_rad_config(compute_dtype="fp32x3")
    m = build(cfg)
    assert m.f32x3 and m.store.compute_dtype == torch.float32
    g = load_golden("full_vqa.npz")
    b = to_dev(full_batch())
    m.store.zero_grad()
    m.set_task()
    ops.PROFILE = []
    try:
        ret = m(b)
        ret["vqa_loss"].backward()
        torch.cuda.synchronize()
        kinds = [k for k, *_ in ops.PROFILE]
    finally:
        ops.PROFILE = None
    gemms = [k for k in kinds if k.startswith("gemm:")]
    assert gemms and set(gemms) == {"gemm:f32x3"}, sorted(set(gemms))
    np.testing.assert_allclose(ret["vqa_logits"].detach().cpu().numpy(), g["logits"], rtol=1e-3, atol=1e-5)
    np.testing.assert_allclose(ret["multi_modal_cls_feats"].detach().cpu().numpy(), g["cls_feats"], rtol=1e-3, atol=1e-5)
    assert abs(ret["vqa_loss"].item() - float(g["loss"])) < 1e-4 * float(g["loss"])
    worst = grad_worst(m.named_parameters(), g, 2e-3, 1e-6)
    assert worst[0] == 0.0, worst


def test_tiny_vqa_fp32x3_against_reference_fixture():
    g = load_golden("tiny_vqa.npz")
    m = build(tiny_config(compute_dtype="fp32x3"))
    b = to_dev(tiny_batch())
    m.store.zero_grad()
    m.set_task()
    ret = m(b)
    np.testing.assert_allclose(ret["vqa_logits"].detach().cpu().numpy(), g["logits"], rtol=1e-3, atol=1e-5)
    ret["vqa_loss"].backward()
    worst = grad_worst(m.named_parameters(), g, 2e-3, 1e-6)
    assert worst[0] == 0.0, worst


def test_tiny_t5_fp32x3_against_reference_fixture():
    from m3ae_amd.modules import T5VQA_MMEncoderInput
    dims = dict(d_model=512, d_kv=64, d_ff=2048, num_layers=2, num_decoder_layers=2, num_heads=8)
    m = T5VQA_MMEncoderInput(tiny_config(compute_dtype="fp32x3"), t5_vocab=1100, t5_dims=dims)
    m.unfreeze_top_layers(4, 4)
    synth.fill_deterministic(m)
    m.finalize("cuda", "fp32x3")
    m.eval()
    assert m.f32x3
    g = load_golden("tiny_t5.npz")
    b = to_dev(tiny_batch())
    b["t5_labels"] = torch.from_numpy(g["labels"]).cuda()
    m.store.zero_grad()
    m.current_tasks = ["vqa"]
    out = m(b)
    np.testing.assert_allclose(out["vqa_logits"].detach().float().cpu().numpy(), g["logits"], rtol=1e-3, atol=1e-5)
    assert abs(out["vqa_loss"].item() - float(g["loss"])) < 1e-5 * float(g["loss"])
    ops.PROFILE = []
    try:
        m.training_step(b)["loss"].backward()
        torch.cuda.synchronize()
        gemms = {k for k, *_ in ops.PROFILE if k.startswith("gemm:")}
    finally:
        ops.PROFILE = None
    assert gemms == {"gemm:f32x3"}, gemms
    ref_total = float(np.sqrt((g["grad_norm"] ** 2).sum()))
    params = dict(m.named_parameters())
    for n, r in zip(g["grad_names"].tolist(), g["grad_norm"]):
        mine = params[n].grad.double().norm().item()
        assert abs(mine - r) <= 2e-3 * r + 2e-6 * ref_total, (n, mine, r)


def test_tiny_decoder_fp32x3_against_reference_fixture():
    from m3ae_amd.modules import DecoderModel
    g = load_golden("tiny_decoder.npz")
    cfg = tiny_config(compute_dtype="fp32x3", image_size=64, hidden_size=768, num_heads=12, num_top_layer=1,
                      input_image_embed_size=128, input_text_embed_size=128, vocab_size=1000, vit_width=128, vit_layers=2,
                      text_hidden=128, text_layers=1, text_heads=2, text_inter=512, mm_encoder_inputs_include_cls_feats=True,
                      mm_encoder_inputs_include_imagetext_feats=False)
    m = DecoderModel(cfg, vocab_size=1200)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.float32)
    m.eval()
    assert m.f32x3 and m.decoder.f32x3
    b = to_dev(synth.synthetic_batch(2, text_len=32, image_size=64, vocab_size=1000, rank=0))
    b["decoder_tokens"] = torch.from_numpy(g["tokens"]).cuda()
    # (parity mode's tiny-feature tolerance, tests/test_gpu_model.py: rtol 1e-3, atol 5e-5 on features of magnitude ~1)
    np.testing.assert_allclose(m.features(b).float().cpu().numpy(), g["cls"], rtol=1e-3, atol=5e-5)
    m.store.zero_grad()
    ops.PROFILE = []
    try:
        loss = m.training_step(b)["loss"]
        loss.backward()
        torch.cuda.synchronize()
        gemms = {k for k, *_ in ops.PROFILE if k.startswith("gemm:")}
    finally:
        ops.PROFILE = None
    assert gemms == {"gemm:f32x3"}, gemms
    assert abs(loss.item() - float(g["loss"])) < 1e-5 * float(g["loss"]), (loss.item(), float(g["loss"]))
    params = dict(m.named_parameters())
    for n, r in zip(g["grad_names"].tolist(), g["grad_norm"]):
        mine = params[n].grad.double().norm().item()
        assert abs(mine - r) <= 2e-3 * r + 1e-9, (n, mine, r)


def _fp32_step(b):
    m = build(tiny_config(compute_dtype="fp32"))
    m.store.zero_grad()
    m.set_task()
    ret = m(b)
    ret["vqa_loss"].backward()
    torch.cuda.synchronize()
    return ret["vqa_logits"].detach().clone(), m.store.grad.clone()


def test_parity_model_after_an_fp32x3_model_is_bit_identical_to_a_fresh_parity_run():
    b = to_dev(tiny_batch())
    logits0, grad0 = _fp32_step(b)
    m3 = build(tiny_config(compute_dtype="fp32x3"))
    m3.store.zero_grad()
    m3.set_task()
    r3 = m3(b)   # graph of the fp32x3 model alive while the parity model runs
    logits1, grad1 = _fp32_step(b)
    r3["vqa_loss"].backward()
    logits2, grad2 = _fp32_step(b)
    for lg, gr in ((logits1, grad1), (logits2, grad2)):
        assert torch.equal(lg, logits0) and torch.equal(gr, grad0)
    assert not torch.equal(r3["vqa_logits"].detach(), logits0)   # (the fp32x3 model did run on other kernels)
    assert not ops.f32x3_active()
