"""GPU: the live-row form of the last fusion pair (ops.CLS_ONLY, infer(cls_only=True)).  The VQA and ITM heads read token 0 of the
last pair's outputs only, so that pair computes K | V for all rows and everything else for the B token-0 rows -- with the dropout
seeds and masks of the full computation (the row map of tests/test_gpu_row_map.py).  Where both sides run the same kernels on the
same rows the comparison is bit equality; sums that reach the flat gradient through fp32 atomics are held to the tolerance
tests/test_gpu_model.py::test_two_stream_schedule_equals_the_single_stream_step uses for "equal up to the order of the fp32
atomics" (relative L2 of the flat gradient <= 1e-5, loss scalar <= 1e-6 relative)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import ops, synth  # noqa: E402
from m3ae_amd.config import finetune_vqa_rad_config, tiny_config  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from m3ae_amd.param_store import ParamStore  # noqa: E402

ATOMICS_REL = 1e-5     # test_two_stream_schedule_equals_the_single_stream_step: gradients
ATOMICS_LOSS = 1e-6    # ... and the loss scalar (m3ae_bce_logits / m3ae_xent add their partials with fp32 atomics)
D, H = 768, 12


def to_dev(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and v and
                isinstance(v[0], torch.Tensor) else v) for k, v in batch.items()}


def rel(a, b):
    return ((a - b).double().norm() / (b.double().norm() + 1e-30)).item()


@pytest.fixture
def composition():
    """Every call on the composition (no fused cross-attention sub-block): the live-row form runs the composition too, so the
    two sides of a comparison run the same kernels."""
    old = ops.XATTN_TRAIN, ops.XATTN
    ops.XATTN_TRAIN = ops.XATTN = "off"
    try:
        yield
    finally:
        ops.XATTN_TRAIN, ops.XATTN = old


@pytest.mark.parametrize("pdrop", [0.0, 0.1])
@pytest.mark.parametrize("L,Lo", [(33, 32), (32, 33)])
def test_block_live_rows_equal_row_0_of_the_full_layer(L, Lo, pdrop, composition):
    """BertCrossLayerFn, D = 768, H = 12, B = 3; the image side (33 queries over 32 text keys, key mask on the other stream) and
    the text side (32 masked queries over 33 keys).  Output: bit equal to row 0.  Backward with dy zero outside row 0: dother is
    one product (d(k | v) . W_kv) on both sides; so are the rows >= 1 of dh (the full call's packed d(q | k | v) . W_qkv has
    exact zeros in its q part there) and row 0 of dh (the live form runs the packed product on that row): all bit equal.
    Parameter gradients: the atomics-order tolerance, on the flat gradient and on each member of the packed self-attention
    projection (a slice written at a wrong offset moves a whole member)."""
    from m3ae_amd.modules.bert_model import BertCrossLayer
    torch.manual_seed(11)
    layer = BertCrossLayer(D, H, 4 * D, drop_rate=pdrop)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn_like(p) * (1.5 / math.sqrt(p.shape[1])))
            elif "LayerNorm.weight" in n:
                p.copy_(1.0 + 0.1 * torch.randn_like(p))
            else:
                p.copy_(0.1 * torch.randn_like(p))
    cfg = dict(learning_rate=1e-3, weight_decay=0.01, lr_multiplier_head=1, lr_multiplier_multi_modal=1)
    store = ParamStore(layer, cfg, "cuda", torch.bfloat16, weight_units=layer.weight_units)
    layer.train(pdrop > 0)
    B = 3
    h0 = torch.randn(B, L, D, device="cuda").to(torch.bfloat16)
    e0 = torch.randn(B, Lo, D, device="cuda").to(torch.bfloat16)
    text_mask = torch.zeros(B, 32, device="cuda")
    text_mask[:, 32 - 9:] = -10000.0
    ms, mo = (None, text_mask) if L == 33 else (text_mask, None)
    dy = torch.zeros(B, L, D, device="cuda", dtype=torch.bfloat16)
    dy[:, 0] = torch.randn(B, D, device="cuda").to(torch.bfloat16)
    res = []
    for live in (False, True):
        store.zero_grad()
        ops.set_dropout_seed(99)
        h, e = h0.clone().requires_grad_(True), e0.clone().requires_grad_(True)
        y = layer(h, e, ms, mo, cls_only=live)
        assert y.shape == ((B, 1, D) if live else (B, L, D))
        y.backward(dy[:, :1] if live else dy)
        torch.cuda.synchronize()
        res.append((y.detach()[:, 0].clone(), h.grad.clone(), e.grad.clone(), store.grad.clone(),
                    {n: q.grad.clone() for n, q in layer.named_parameters()}))
    (yf, dhf, def_, gf, pf), (yl, dhl, del_, gl, pl) = res
    assert torch.equal(yl, yf)
    assert torch.equal(del_, def_)
    assert torch.equal(dhl[:, 1:], dhf[:, 1:])
    assert torch.equal(dhl[:, 0], dhf[:, 0])
    assert rel(gl, gf) <= ATOMICS_REL, rel(gl, gf)
    for n in pf:   # no parameter lost its gradient: the Q and the K | V slice of the packed weight among them
        assert (pl[n].abs().max() > 0) == (pf[n].abs().max() > 0), n
    # the members of the packed Q | K | V weight and bias of the self-attention, which the live form writes slice by slice (Q
    # rows, then K | V rows) and the full layer in one product: each member on its own, to the same tolerance (key.bias is zero
    # in exact arithmetic -- softmax is invariant to it -- and rounding noise on both sides: not a relative comparison)
    packed = [n for n in pf if n.startswith("attention.self.") and n != "attention.self.key.bias"]
    assert len(packed) == 5, packed
    for n in packed:
        print(f"{n}: rel {rel(pl[n], pf[n]):.3e}")
        assert rel(pl[n], pf[n]) <= ATOMICS_REL, (n, rel(pl[n], pf[n]))


def _tiny(loss_names=None):
    over = dict(compute_dtype="bf16", drop_rate=0.1)
    if loss_names:
        over["loss_names"] = loss_names
    m = M3AETransformerSS(tiny_config(**over))
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    m.set_task()
    return m


def _step(m, b, key, live, two):
    old = ops.CLS_ONLY, m.two_streams
    ops.CLS_ONLY, m.two_streams = live, two
    try:
        m.train()
        m.store.zero_grad()
        ops.set_dropout_seed(5)
        ret = m(b)
        ret[key + "_loss"].backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        return ret, m.store.grad.clone(), grads
    finally:
        ops.CLS_ONLY, m.two_streams = old


def _ordered_loss(task, ret):
    """The step's loss from the step's own logits, reduced in a fixed order (the library's ordered loss kernels): the loss a
    step returns is summed with fp32 atomics, so two runs of the SAME code differ in its last bit from time to time."""
    with torch.no_grad(), ops.deterministic_mode():
        if task == "vqa":
            return ops.bce_with_logits_loss(ret["vqa_logits"].detach(), ret["vqa_targets"])
        return ops.cross_entropy(ret["itm_logits"].detach(), ret["itm_labels"].long())


@pytest.mark.parametrize("two", [True, False])
@pytest.mark.parametrize("task", ["vqa", "itm"])
def test_tiny_training_step_with_and_without_the_switch(task, two, composition):
    """tiny_vqa dimensions, B = 3, train mode (dropout 0.1), same seeds, two-stream and single-stream schedule; VQA head and the
    ITM pass of the pre-training head.  Logits and class features bit equal; the loss bit equal once its partials are added in
    a fixed order (_ordered_loss), and the returned scalar -- an fp32-atomics sum even between two runs of one build -- within
    the atomics-order tolerance of it; flat gradient to the atomics-order tolerance; every parameter that gets a gradient
    without the switch gets one with it."""
    if task == "vqa":
        m = _tiny()
        b = to_dev(synth.synthetic_batch(3, text_len=32, image_size=64, vocab_size=1000, rank=0))
    else:
        m = _tiny({"mlm": 0, "mim": 0, "itm": 1, "vqa": 0, "cls": 0, "irtr": 0})
        b = to_dev(synth.synthetic_batch(3, text_len=32, image_size=64, vocab_size=1000, rank=0, pretrain=True))
        b["itm_labels"] = torch.tensor([1.0, 0.0, 1.0])
    r0, g0, p0 = _step(m, b, task, False, two)
    r1, g1, p1 = _step(m, b, task, True, two)
    assert torch.equal(r1[task + "_logits"], r0[task + "_logits"])
    l0, l1 = _ordered_loss(task, r0), _ordered_loss(task, r1)
    assert torch.equal(l1, l0)
    for r in (r0, r1):
        assert abs(r[task + "_loss"].item() - l0.item()) <= ATOMICS_LOSS * abs(l0.item()), (r[task + "_loss"].item(), l0.item())
    if task == "vqa":
        assert torch.equal(r1["multi_modal_cls_feats"], r0["multi_modal_cls_feats"])
    assert rel(g1, g0) <= ATOMICS_REL, rel(g1, g0)
    assert set(p0) == set(p1)
    for n in p0:
        assert (p1[n].abs().max() > 0) or not (p0[n].abs().max() > 0), n


def test_full_width_pruned_against_fused_parent_by_their_fp32_errors():
    """configs[1] widths, one ViT block, one RoBERTa layer, two fusion layers, B = 2, eval mode, fused cross-attention in play
    (the suite's XATTN_TRAIN_MIN_BATCH = 0): without the switch the last layer runs the fused sub-block, with it the composition
    on the CLS rows; the two differ by bf16 roundings.  Both against the same model in compute_dtype fp32 (the mode held to the
    reference): the rms error of the class features and of the logits with the switch is <= 1.5 x the error without it
    (the rule of tests/test_gpu_xattn.py).  The fp32 target of this configuration was checked on the CPU oracle to be finite and
    non-degenerate (logits rms 0.53, class features rms 0.44, the two samples differ; no seed is involved: the weights and the
    batch come from the deterministic generators)."""
    over = dict(vit_layers=1, text_layers=1, num_top_layer=2)
    b = to_dev(synth.synthetic_batch(2, text_len=32, image_size=384, rank=0))

    def run(dtype_name, dtype, live):
        m = M3AETransformerSS(finetune_vqa_rad_config(compute_dtype=dtype_name, **over))
        synth.fill_deterministic(m)
        m.finalize("cuda", dtype)
        m.eval()
        m.set_task()
        old = ops.CLS_ONLY
        ops.CLS_ONLY = live
        try:
            ret = m(b)
        finally:
            ops.CLS_ONLY = old
        return ret["multi_modal_cls_feats"].detach().float().clone(), ret["vqa_logits"].detach().float().clone()

    ref = run("fp32", torch.float32, False)
    assert all(torch.isfinite(t).all() and t.std().item() > 1e-3 for t in ref)
    full, live = run("bf16", torch.bfloat16, False), run("bf16", torch.bfloat16, True)
    rms = lambda t: t.double().pow(2).mean().sqrt().item()
    for name, r, f, l in zip(("cls_feats", "logits"), ref, full, live):
        ef, el = rms(f - r), rms(l - r)
        print(f"{name}: rms error unpruned {ef:.6f}, pruned {el:.6f}, ref rms {rms(r):.4f}")
        assert el <= 1.5 * ef, (name, el, ef)


def test_consumers_that_need_sequences(composition):
    """infer() without the keyword returns the full sequences; cls_only leaves the two keys out; output_attentions with cls_only
    computes the full layer (the maps are full-layer outputs) and returns the sequences as well."""
    m = _tiny()
    m.eval()
    b = to_dev(synth.synthetic_batch(3, text_len=32, image_size=64, vocab_size=1000, rank=0))
    with torch.no_grad():
        full = m.infer(b)
        live = m.infer(b, cls_only=True)
        maps = m.infer(b, cls_only=True, output_attentions=True)
    Li = (64 // 16) ** 2 + 1
    assert full["multi_modal_text_feats"].shape == (3, 32, 128) and full["multi_modal_image_feats"].shape == (3, Li, 128)
    assert "multi_modal_text_feats" not in live and "multi_modal_image_feats" not in live
    assert torch.equal(live["multi_modal_cls_feats"], full["multi_modal_cls_feats"])
    assert maps["multi_modal_image_feats"].shape == (3, Li, 128) and maps["attentions"] is not None
    assert maps["attentions"]["image2text_attns"][-1][0].shape == (3, 2, Li, Li)
    assert torch.equal(maps["multi_modal_cls_feats"], full["multi_modal_cls_feats"])
