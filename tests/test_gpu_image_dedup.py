"""GPU: de-duplicated image batches (batch["image_index"], config key `image_dedup`).

1. the two kernels (csrc/samples.hip) against their numpy model (tests/dedup_model.py), bit for bit;
2. the model: a batch of 5 samples over 3 images against the same batch expanded to 5 images -- forward bit-equal, the image tower
   really runs on 3 images, gradients of everything after the expansion bit-equal and the tower's within the tiny fixture's
   tolerances of the CPU oracle (tests/test_gpu_model.py), deterministic mode, the generator head, no blocking host call;
3. the input pipeline and the trainer with the flag on and off.

Bit-equality of losses and gradients between two RUNS is asserted under ops.deterministic_mode: outside it the loss scalars and
the split-K weight gradients add with fp32 atomics and two runs of the very same batch differ in the last bits."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dedup_model as M  # noqa: E402
from m3ae_amd import _lib, data, ops, synth  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from m3ae_amd.modules import objectives  # noqa: E402
from oracle import m3ae_oracle as O  # noqa: E402
from oracle_util import load_golden, make_sd, oracle_cfg, tiny_config  # noqa: E402

DEV = "cuda"
INDEX = [2, 0, 2, 1, 2]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _buffer(rows, R, dtype, offset):
    """[rows, R] view of a flat buffer, its base `offset` elements past the allocation's (256-byte aligned) start."""
    flat = torch.zeros(rows * R + offset, dtype=dtype, device=DEV)
    return flat[offset:].view(rows, R)


def _bits(a):
    a = M.from_torch(a) if isinstance(a, torch.Tensor) else a
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run_expand(x, index, out):
    idx = torch.tensor(index, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().m3ae_expand_samples(C.c_void_p(x.data_ptr()), C.c_void_p(idx.data_ptr()), C.c_void_p(out.data_ptr()),
                                              len(index), x.shape[0], x.shape[1], ops._dt(x), _stream()), "m3ae_expand_samples")
    return out


def _run_segment_sum(d, offsets, members, out):
    off = torch.from_numpy(offsets).to(DEV)
    mem = torch.from_numpy(members).to(DEV)
    _lib.check(_lib.lib().m3ae_segment_sum_rows(C.c_void_p(d.data_ptr()), C.c_void_p(off.data_ptr()), C.c_void_p(mem.data_ptr()),
                                                C.c_void_p(out.data_ptr()), out.shape[0], d.shape[0], d.shape[1], ops._dt(d),
                                                _stream()), "m3ae_segment_sum_rows")
    return out


INTERLEAVED = [2, 1, 2, 0, 2, 2, 1, 2, 2, 2]   # B = 10: groups of 1, 2 and 7 samples, members not contiguous
KERNEL_CASES = {
    # name: (index, R, element offset of the input base, of the output base)
    "interleaved_aligned": (INTERLEAVED, 17 * 128, 0, 0),
    "interleaved_scalar": (INTERLEAVED, 1001, 0, 0),
    "one_image": ([0, 0, 0, 0], 17 * 128, 0, 0),
    "one_image_scalar": ([0, 0, 0, 0], 1001, 0, 0),
    "all_distinct": ([3, 1, 0, 2], 17 * 128, 0, 0),
    "all_distinct_scalar": ([3, 1, 0, 2], 1001, 0, 0),
    "output_base_off_by_one": (INTERLEAVED, 17 * 128, 0, 1),
    "input_base_off_by_one": (INTERLEAVED, 17 * 128, 1, 0),
    # more than one workgroup along a row, the last one partly filled (vector path: 16-byte units; scalar path: elements)
    "several_blocks_aligned": (INTERLEAVED, 24 * 1024 + 8, 0, 0),
    "several_blocks_scalar": (INTERLEAVED, 2051, 0, 0),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernels_equal_the_numpy_model_bit_for_bit(case, dtype):
    index, R, off_in, off_out = KERNEL_CASES[case]
    bf16 = dtype == torch.bfloat16
    B, U = len(index), max(index) + 1
    rng = np.random.RandomState(len(case) + R)
    to_repr = (lambda a: M.bf16_round(a)) if bf16 else (lambda a: a.astype(np.float32))
    x = to_repr(rng.standard_normal((U, R)).astype(np.float32) * 3.0)
    d = to_repr(rng.standard_normal((B, R)).astype(np.float32) * 3.0)
    d[0, :4] = to_repr(np.array([-0.0, 0.0, 1e-30, -1e30], dtype=np.float32))
    offsets, members = M.groups_of(index, U)
    # expansion (forward): input base offset by `off_in`, output base by `off_out`
    xin = _buffer(U, R, dtype, off_in)
    xin.copy_(M.to_torch(x, bf16))
    out = _run_expand(xin, index, _buffer(B, R, dtype, off_out))
    assert np.array_equal(_bits(out), _bits(M.expand(x, index)))
    # segment sum (backward): the roles swap, the gradient of the output is read and the gradient of the input written
    din = _buffer(B, R, dtype, off_out)
    din.copy_(M.to_torch(d, bf16))
    got = _run_segment_sum(din, offsets, members, _buffer(U, R, dtype, off_in))
    want = M.segment_sum(d, offsets, members, bf16)
    assert np.array_equal(_bits(got), _bits(want)), (case, int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_expansion_then_segment_sum_of_ones_counts_the_members(dtype):
    """Through the autograd node: d(expand_samples)/dx against all-ones is the number of samples per image, exactly."""
    g = ops.image_groups(INTERLEAVED).to(DEV)
    x = torch.randn(3, 7, 96, device=DEV).to(dtype).requires_grad_(True)
    y = ops.expand_samples(x, g)
    assert y.shape == (10, 7, 96) and torch.equal(y, x.detach()[torch.tensor(INTERLEAVED, device=DEV)])
    y.backward(torch.ones_like(y))
    want = torch.tensor([1.0, 2.0, 7.0], device=DEV).view(3, 1, 1).expand(3, 7, 96).to(dtype)
    assert torch.equal(x.grad, want)
    with pytest.raises(ValueError):
        ops.expand_samples(x.detach()[:2], g)


def test_rows_past_two_to_the_31_elements():
    """A bf16 output of 2560 rows of 2^20 elements (5.4 GB): row bases past 2^31 elements.  Rows are constant (their value names
    the row), so a wrong base shows as a wrong value; the per-image sums are small integers, exact in fp32 and in bf16."""
    U, B, R = 2, 2560, 1 << 20
    index = torch.arange(B, device=DEV) % U
    x = torch.tensor([3.0, 5.0], device=DEV).view(U, 1).expand(U, R).to(torch.bfloat16).contiguous()
    out = torch.empty(B, R, dtype=torch.bfloat16, device=DEV)
    _lib.check(_lib.lib().m3ae_expand_samples(C.c_void_p(x.data_ptr()), C.c_void_p(index.data_ptr()), C.c_void_p(out.data_ptr()),
                                              B, U, R, _lib.BF16, _stream()), "m3ae_expand_samples")
    rows = out.view(torch.int16)
    want = torch.where(index == 0, 3.0, 5.0).to(torch.bfloat16).view(torch.int16)
    assert torch.equal(rows.amin(dim=1), want) and torch.equal(rows.amax(dim=1), want)
    # backward: all rows zero but the last four, which hold 1, 2, 3, 4 -> image 0 sums rows 2556, 2558 (1 + 3), image 1 (2 + 4)
    out.zero_()
    out[B - 4:] = torch.tensor([1.0, 2.0, 3.0, 4.0], device=DEV).view(4, 1).to(torch.bfloat16)
    offsets = torch.tensor([0, B // 2, B], dtype=torch.int64, device=DEV)
    members = torch.cat([torch.arange(0, B, 2), torch.arange(1, B, 2)]).to(DEV)
    dx = torch.empty(U, R, dtype=torch.bfloat16, device=DEV)
    _lib.check(_lib.lib().m3ae_segment_sum_rows(C.c_void_p(out.data_ptr()), C.c_void_p(offsets.data_ptr()),
                                                C.c_void_p(members.data_ptr()), C.c_void_p(dx.data_ptr()), U, B, R, _lib.BF16,
                                                _stream()), "m3ae_segment_sum_rows")
    assert torch.equal(dx, torch.tensor([4.0, 6.0], device=DEV).view(U, 1).expand(U, R).to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. model
# ---------------------------------------------------------------------------------------------------------------------------------
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def build(mode, **over):
    m = M3AETransformerSS(tiny_config(compute_dtype=mode, **over))
    synth.fill_deterministic(m)
    m.finalize(DEV, DTYPES[mode])
    m.eval()
    m.set_task()
    return m


def to_dev(batch):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else [t.to(DEV) for t in v] if isinstance(v, list) and v and
                isinstance(v[0], torch.Tensor) else v) for k, v in batch.items()}


def batches(index=INDEX, tables=True, **extra):
    """(the batch of len(index) samples over its distinct images with the key, the same batch with one image per sample), on the
    CPU: the samples of synthetic_batch, sample b showing image index[b] of the first U images."""
    B, U = len(index), max(index) + 1
    full = synth.synthetic_batch(B, text_len=32, image_size=64, vocab_size=1000, rank=0)
    full.update(extra)
    imgs = full["image"][0][:U].clone()
    expanded = dict(full, image=[imgs[torch.tensor(index)].clone()])
    dedup = dict(full, image=[imgs], image_index=torch.tensor(index, dtype=torch.int64))
    if tables:
        dedup["image_groups"] = ops.image_groups(index, n_images=U)
    return dedup, expanded


@pytest.fixture
def deterministic():
    with ops.deterministic_mode(True):
        yield


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_forward_equals_the_expanded_batch_bit_for_bit(mode):
    m = build(mode, drop_rate=0.1)
    bd, be = (to_dev(b) for b in batches())
    seen = []
    hook = m.vision_encoder.register_forward_pre_hook(lambda mod, args: seen.append(args[0].shape[0]))
    with torch.no_grad():
        od, oe = m.infer(bd), m.infer(be)
        ld, le = m(bd)["vqa_logits"], m(be)["vqa_logits"]
    hook.remove()
    assert seen == [3, 5, 3, 5]                                   # the tower ran on the distinct images only
    for k in ("multi_modal_cls_feats", "multi_modal_image_feats", "multi_modal_text_feats"):
        assert od[k].shape[0] == 5 and torch.equal(od[k], oe[k]), k
    assert torch.equal(ld, le)
    assert od["images"] is bd["image"][0] and torch.equal(od["image_index"], bd["image_index"]) and "image_index" not in oe
    # a device index without tables: the same result (one copy of the index to the host)
    bd2 = {k: v for k, v in bd.items() if k != "image_groups"}
    with torch.no_grad():
        assert torch.equal(m.infer(bd2)["multi_modal_cls_feats"], oe["multi_modal_cls_feats"])
    # train mode, same dropout seed: the tower draws no seed, the fusion layers see the same masks
    m.train()
    losses = []
    with ops.deterministic_mode(True), torch.no_grad():
        for b in (bd, be):
            ops.set_dropout_seed(17)
            losses.append(m(b)["vqa_loss"])
    assert torch.equal(losses[0], losses[1]) and torch.isfinite(losses[0])
    m.eval()
    with torch.no_grad():
        assert not torch.equal(m(be)["vqa_loss"], losses[1])      # (dropout was on)


def _step_grads(m, b, train=False):
    m.train(train)
    m.store.zero_grad()
    ops.set_dropout_seed(23)
    loss = m(b)["vqa_loss"]
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), m.store.grad.clone()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_identity_index_is_the_path_without_the_key(mode, deterministic, monkeypatch):
    m = build(mode, drop_rate=0.1)
    _, be = (to_dev(b) for b in batches())
    bi = dict(be, image_index=torch.arange(5, device=DEV))
    bt = dict(bi, image_groups=ops.image_groups(list(range(5))).to(DEV))
    calls = []
    real = ops.expand_samples
    monkeypatch.setattr(ops, "expand_samples", lambda *a: (calls.append(1), real(*a))[1])
    l0, g0 = _step_grads(m, be, train=True)
    for b in (bi, bt):
        l1, g1 = _step_grads(m, b, train=True)
        assert torch.equal(l0, l1) and torch.equal(g0, g1)
    assert calls == []                                             # no new kernel
    _step_grads(m, to_dev(batches()[0]))
    assert calls == [1]                                            # (and exactly one node with a real index)


def test_callers_that_read_pixels_per_sample_refuse_the_key():
    from m3ae_amd.graph import GraphedStep
    m = build("bf16")
    bd, be = (to_dev(b) for b in batches())
    with pytest.raises(ValueError, match="image_index"):
        m.infer(bd, mask_image=True)
    with pytest.raises(ValueError, match="image_index"):
        m.infer(bd, img=be["image"][0])
    bd["false_image_0"] = be["image"]
    with pytest.raises(ValueError, match="image_index"):
        objectives.compute_itm(m, bd)
    with pytest.raises(ValueError, match="image_index"):
        objectives.compute_mim(m, bd)
    with pytest.raises(ValueError, match="image_index"):
        GraphedStep(m, bd, max_steps=10)
    # tables that do not fit the batch
    with pytest.raises(ValueError):
        m.infer(dict(bd, image_groups=ops.image_groups([0, 1, 1, 0, 0]).to(DEV)))
    with pytest.raises(ValueError, match="used by no sample"):
        m.infer({k: v for k, v in dict(bd, image_index=torch.tensor([0, 0, 2, 2, 0], device=DEV)).items() if k != "image_groups"})


def _oracle_grads(cfg, batch):
    sd = make_sd(cfg, requires_grad=True)
    loss, _, _ = O.training_loss(sd, oracle_cfg(cfg), batch)
    loss.backward()
    return float(loss.detach()), {n: t.grad for n, t in sd.items() if t.grad is not None}


def _hold_to_oracle(m, ref, mode, fixture_grad_names):
    """The checks tests/test_gpu_model.py applies to the tiny fixture's gradients in this mode, against the oracle's gradients."""
    params = dict(m.named_parameters())
    names = [n for n in ref if n in params and params[n].grad is not None]
    assert len(names) > 100
    rn = np.array([ref[n].double().norm().item() for n in names])
    mine = np.array([params[n].grad.double().norm().item() for n in names])
    gn_ref = float(np.sqrt((rn ** 2).sum()))
    if mode == "fp32":   # test_tiny_fp32_parity_against_reference_fixture_and_oracle: grad_report(m, g, 2e-3, 1e-6) + element-wise
        bad = [(n, a, r) for n, a, r in zip(names, mine, rn) if abs(a - r) > 2e-3 * r + 1e-6 * gn_ref]
        assert not bad, bad[:3]
        for n in fixture_grad_names:
            r = ref[n].numpy()
            np.testing.assert_allclose(params[n].grad.cpu().numpy(), r, rtol=5e-3, atol=1e-4 * np.abs(r).max() + 1e-9, err_msg=n)
    else:                # test_tiny_bf16_perf_mode_within_bf16_bounds
        gn = float(np.sqrt((mine ** 2).sum()))
        assert abs(gn - gn_ref) < 3e-2 * gn_ref, (gn, gn_ref)
        big = rn > 1e-3 * rn.max()
        rel = np.abs(mine[big] - rn[big]) / rn[big]
        assert rel.max() < 0.15, (rel.max(), np.array(names)[big][rel.argmax()])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_backward_against_the_expanded_batch_and_the_oracle(mode, deterministic):
    cfg = tiny_config(compute_dtype=mode)
    m = build(mode)
    bd_cpu, be_cpu = batches()
    bd, be = to_dev(bd_cpu), to_dev(be_cpu)
    loss_o, ref = _oracle_grads(cfg, be_cpu)
    fixture_names = [k[6:] for k in load_golden("tiny_vqa.npz").files if k.startswith("grad::")]
    params = dict(m.named_parameters())
    grads = {}
    for tag, b in (("expanded", be), ("dedup", bd)):
        loss, _ = _step_grads(m, b)
        assert abs(loss.item() - loss_o) < (1e-4 if mode == "fp32" else 2e-3) * loss_o
        _hold_to_oracle(m, ref, mode, fixture_names)             # each run on its own, the same bounds
        grads[tag] = {n: p.grad.clone() for n, p in params.items() if p.grad is not None}
    # everything after the expansion saw identical inputs: bit-equal gradients.  The tower and its projection got the per-image
    # sum of the samples' gradients in another order (and, in bf16, rounded once more): close, not equal.
    tower = [n for n in grads["dedup"] if n.startswith(("vision_encoder.", "multi_modal_vision_proj."))]
    rest = [n for n in grads["dedup"] if n not in tower and n != "modality_type_embeddings.weight"]
    assert len(tower) > 20 and len(rest) > 100
    for n in rest:
        assert torch.equal(grads["dedup"][n], grads["expanded"][n]), n
    a = torch.cat([grads["dedup"][n].flatten() for n in tower]).double()
    b = torch.cat([grads["expanded"][n].flatten() for n in tower]).double()
    rel = ((a - b).norm() / b.norm()).item()
    print(f"{mode}: tower gradient, de-duplicated against expanded: relative L2 {rel:.3e}")
    assert b.norm().item() > 0 and np.isfinite(rel)


def test_two_deduplicated_steps_from_the_same_state_give_the_same_bits(deterministic):
    flats = []
    for _ in range(2):
        m = build("bf16", drop_rate=0.1)
        m.train()
        bd = to_dev(batches()[0])
        ops.set_dropout_seed(5)
        for _ in range(2):
            m.store.zero_grad()
            m.training_step(bd).backward()
            m.store.adamw_step(max_steps=100, lr_factor=1.0)
        torch.cuda.synchronize()
        flats.append(m.store.flat.clone())
    assert torch.equal(flats[0], flats[1]) and torch.isfinite(flats[0]).all()


def test_generator_head_passes_the_key_through(deterministic):
    from m3ae_amd.modules import T5VQA_MMEncoderInput
    dims = dict(d_model=512, d_kv=64, d_ff=2048, num_layers=2, num_decoder_layers=2, num_heads=8)
    m = T5VQA_MMEncoderInput(tiny_config(compute_dtype="bf16"), t5_vocab=1100, t5_dims=dims)
    m.unfreeze_top_layers(4, 4)
    synth.fill_deterministic(m)
    m.finalize(DEV, torch.bfloat16)
    m.eval()
    m.current_tasks = ["vqa"]
    lab = synth.det_randint("t5_labels", 2, 1100, (5, 6), salt=31)
    lab[:, -1] = 1
    bd, be = (to_dev(b) for b in batches(t5_labels=lab))
    seen = []
    hook = m.m3ae.vision_encoder.register_forward_pre_hook(lambda mod, args: seen.append(args[0].shape[0]))
    ld, le = m(bd)["vqa_loss"], m(be)["vqa_loss"]
    hook.remove()
    assert seen == [3, 5] and torch.isfinite(ld) and torch.equal(ld, le)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. input pipeline and trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def _arrow_cfg(tmp_path, **over):
    from arrow_util import write_split
    root = str(tmp_path / "arrows")
    write_split(root, "train", 12)
    write_split(root, "val", 4, seed=100)
    return tiny_config(compute_dtype="bf16", data_root=root, per_gpu_batchsize=8, num_workers=3, seed=1, **over)


@pytest.mark.parametrize("transform", ["host", "device"])
def test_datamodule_batches_hold_each_distinct_image_once(tmp_path, transform):
    from arrow_util import HashTokenizer
    cfg = _arrow_cfg(tmp_path, image_transform=transform)
    out = {}
    for flag in (False, True):
        dm = data.ArrowDataModule(dict(cfg, image_dedup=flag), 0, 1, torch.device(DEV, 0), tokenizer=HashTokenizer())
        out[flag] = (list(dm.train_batches(0)) + list(dm.val_batches()), dm.transform_stats.decodes)
        torch.cuda.synchronize()
    (plain, n_plain), (dedup, n_dedup) = out[False], out[True]
    assert len(plain) == len(dedup) == 4 and n_plain == 24 + 7
    saved = 0
    for bp, bd in zip(plain, dedup):
        assert "image_index" not in bp and set(bd) == set(bp) | {"image_index", "image_groups"}
        ii, img = bd["image_index"], bd["image"][0]
        assert ii.is_cuda and ii.dtype == torch.int64 and bd["image_groups"].index is ii and bd["image_groups"].offsets.is_cuda
        assert img.shape[0] == bd["image_groups"].n_images == int(ii.max()) + 1 <= bp["image"][0].shape[0]
        assert torch.equal(img[ii], bp["image"][0])
        for k in ("text_ids", "text_masks", "text_labels"):
            assert torch.equal(bd[k], bp[k])
        assert bd["text"] == bp["text"] and bd["vqa_labels"] == bp["vqa_labels"] and bd["qid"] == bp["qid"]
        saved += bp["image"][0].shape[0] - img.shape[0]
    assert saved >= 3 and n_dedup == n_plain - saved          # (the validation table alone repeats three images)


def _no_host_wait(fn, monkeypatch):
    """Run fn() under torch.cuda.set_sync_debug_mode("error") where `.item()` under it raises on this torch / ROCm pair; otherwise
    count calls of Tensor.cpu / item / tolist / __bool__ and torch.cuda.synchronize (as tests/test_gpu_beam.py does)."""
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            live = False
        except RuntimeError:
            live = True
        if live:
            r = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not live:
        calls = []
        for name in ("cpu", "item", "tolist", "__bool__"):
            real = getattr(torch.Tensor, name)
            monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _r=real, _n=name, **k: (calls.append(_n) if self.is_cuda else None, _r(self, *a, **k))[1])
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
        r = fn()
        monkeypatch.undo()
        assert calls == [], calls
    print("sync guard:", "set_sync_debug_mode" if live else "call counting")
    return r


def test_training_step_on_a_datamodule_batch_makes_no_blocking_host_call(tmp_path, monkeypatch):
    from arrow_util import HashTokenizer
    cfg = _arrow_cfg(tmp_path, image_dedup=True, drop_rate=0.1)
    dm = data.ArrowDataModule(cfg, 0, 1, torch.device(DEV, 0), tokenizer=HashTokenizer())
    bs = list(dm.val_batches())                                   # the table in order: every image's questions back to back
    assert not bs[0]["image_groups"].identity and bs[0]["image"][0].shape[0] < bs[0]["text_ids"].shape[0]
    m = build("bf16", drop_rate=0.1)
    m.train()

    def step():
        m.store.zero_grad()
        ops.set_dropout_seed(3)
        loss = m.training_step(bs[0])
        loss.backward()
        return loss

    want = step()                                                 # warm: lazy buffers and kernel attributes exist
    torch.cuda.synchronize()
    loss = _no_host_wait(step, monkeypatch)
    torch.cuda.synchronize()
    # the same masks, the same step up to the summation order of the loss's fp32 atomics
    assert torch.isfinite(loss) and abs(loss.item() - want.item()) <= 1e-6 * abs(want.item())


@pytest.fixture
def restore_deterministic_switch():
    prev = ops.deterministic()
    try:
        yield
    finally:
        ops.set_deterministic(prev)


def test_two_trainer_steps_with_the_flag_on_and_off(tmp_path, restore_deterministic_switch):
    from arrow_util import HashTokenizer, write_split
    from m3ae_amd import trainer
    root = str(tmp_path / "arrows")
    write_split(root, "train", 12)
    write_split(root, "val", 4, seed=100)
    tiny = ("image_size=64 hidden_size=128 num_heads=2 num_top_layer=2 input_image_embed_size=128 "
            "input_text_embed_size=128 vocab_size=1000 vit_width=128 vit_layers=3 text_hidden=128 text_layers=2 "
            "text_heads=2 text_inter=512").split()
    losses, decodes, towers = {}, {}, {}
    for flag in (False, True):
        argv = (["with", f"data_root={root}", "num_gpus=1", "num_nodes=1", "task_finetune_vqa_vqa_rad", "clip16",
                 "text_roberta", "per_gpu_batchsize=8", "batch_size=8", "max_steps=2", "num_workers=2", "deterministic=True",
                 "learning_rate=0.0005", f"image_dedup={flag}", f"log_dir={tmp_path / str(flag)}", "seed=2"] + tiny)
        cfg = trainer.config_mod.parse_cli(argv)
        assert cfg["image_dedup"] is flag
        dev = torch.device(DEV, 0)
        torch.manual_seed(cfg["seed"])
        model = trainer.build_model(cfg, "cls", dev)
        seen = []
        model.vision_encoder.register_forward_pre_hook(lambda mod, args, seen=seen: seen.append(args[0].shape[0]))
        dm = data.ArrowDataModule(cfg, 0, 1, dev, tokenizer=HashTokenizer())
        out = trainer.Trainer(cfg, model, dm, 0, 1, dev, log_every=1).fit()
        assert out["global_step"] == 2
        losses[flag] = [h[1] for h in out["history"]]
        decodes[flag], towers[flag] = dm.transform_stats.decodes, sum(seen)
    print("losses", losses, "decodes", decodes, "tower images", towers)
    assert len(losses[True]) == 2 and np.isfinite(losses[True]).all()
    assert losses[True][0] == losses[False][0]                                        # same state, same batch: bit-equal
    assert abs(losses[True][1] - losses[False][1]) < 2e-3 * abs(losses[False][1])     # perf mode's loss tolerance (test_gpu_model.py)
    assert decodes[True] < decodes[False] and towers[True] < towers[False]
    with pytest.raises(SystemExit, match="image_dedup"):
        trainer.run(argv + ["loss_names={'vqa': 1, 'itm': 1, 'mlm': 0, 'mim': 0, 'cls': 0, 'irtr': 0}", "image_dedup=True"])
