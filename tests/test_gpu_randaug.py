"""RandAugment(2, 9) on the GPU (csrc/randaug.hip) against its numpy model (m3ae_amd/randaug.py, itself pinned to Pillow by
tests/test_randaug_host.py): the histograms, the tables of the seven point operations, every operation and sign through the
apply kernel, all ordered pairs, refused records, and the arrow pipeline / trainer under image_transform="device" against "host".
Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from randaug_cases import DEVICE_SIZES, OP_SIGNS, degenerate_images, image  # noqa: E402
from test_gpu_resample import restore_deterministic_switch  # noqa: E402,F401

from m3ae_amd import _lib, data, resample  # noqa: E402
from m3ae_amd import randaug as ra  # noqa: E402
from m3ae_amd.config import tiny_config  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 0xAB          # what scratch and the gaps between images hold before a call


def _run(images, augs, flags=None, edit=None):
    """Pack `images` (16-byte aligned offsets, FILL in the gaps), run the two stages of `augs` -> (source buffer after the call,
    scratch after the call, list of per-image views of the source buffer, histograms [2, B, 4, 256], tables [B, 3, 256], plan).
    `edit(plan)`: change records before the upload."""
    offs, total = [], 0
    for a in images:
        offs.append(total)
        total += resample._align16(a.size)
    total += 64                                              # spare bytes behind the last image
    src = np.full(total, FILL, dtype=np.uint8)
    for a, o in zip(images, offs):
        src[o:o + a.size] = a.reshape(-1)
    plan = ra.augment_plan([a.shape for a in images], offs, augs)
    if edit is not None:
        edit(plan)
    src_d, scratch_d = torch.from_numpy(src).to(DEV), torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    ws = ra.augment_on_device(src_d, torch.from_numpy(plan).to(DEV), ra.stage_flags(plan) if flags is None else flags, scratch=scratch_d)
    torch.cuda.synchronize()
    B = len(images)
    ws = ws.cpu().numpy()
    hist = ws[:2 * B * 4096].view(np.uint32).reshape(2, B, 4, 256)
    lut = ws[2 * B * 4096:].reshape(B, 3, 256)
    out = src_d.cpu().numpy()
    views = [out[o:o + a.size].reshape(a.shape) for a, o in zip(images, offs)]
    return out, scratch_d.cpu().numpy(), views, hist, lut, plan, src


def _gaps_untouched(before, after, images, plan):
    keep = np.ones(before.size, dtype=bool)
    for a, off in zip(images, plan[:, ra.AUG_OFF]):
        keep[off:off + a.size] = False
    return np.array_equal(before[keep], after[keep])


def _hist_images():
    out = list(degenerate_images().values())
    out += [image(w, h, kind, seed=4) for (w, h) in DEVICE_SIZES for kind in ("noise", "smooth")]
    return out


def test_histograms_are_exact():
    images = _hist_images()
    hist_ops = (ra.OP_AUTOCONTRAST, ra.OP_EQUALIZE, ra.OP_CONTRAST)
    # stage 0 reads the image's histogram; stage 1 the histogram of what stage 0 wrote
    augs = [((hist_ops[i % 3], 1), (hist_ops[(i + 1) % 3], 1)) for i in range(len(images))]
    augs[-1] = ((ra.OP_ROTATE, 1), (ra.OP_EQUALIZE, 1))
    augs[-2] = ((ra.OP_POSTERIZE, 1), (ra.OP_COLOR, 1))       # no histogram user: its rows stay zero
    _, _, _, hist, _, _, _ = _run(images, augs)
    for i, (a, ops) in enumerate(zip(images, augs)):
        for stage in range(2):
            want = ra.histograms(a).astype(np.uint32) if ops[stage][0] in hist_ops else np.zeros((4, 256), np.uint32)
            assert np.array_equal(hist[stage, i], want), (i, stage, a.shape)
            a = ra.apply_model(a, *ops[stage])


def test_tables_are_exact():
    images = _hist_images()
    for op in ra.POINT_OPS:
        _, _, views, _, lut, _, _ = _run(images, [((op, 1), (ra.OP_IDENTITY, 1))] * len(images))
        for i, a in enumerate(images):
            want = ra.point_lut(op, ra.histograms(a) if op in ra.HIST_OPS else None)
            assert np.array_equal(lut[i], want), (ra.OP_NAMES[op], i, a.shape)
            assert np.array_equal(views[i], ra.apply_model(a, op)), (ra.OP_NAMES[op], i, a.shape)


@pytest.mark.parametrize("stage", (0, 1))
def test_apply_equals_the_model_for_every_operation_and_sign(stage):
    images, augs = [], []
    for (w, h) in DEVICE_SIZES:
        for kind in ("noise", "smooth"):
            for op, sign in OP_SIGNS:
                images.append(image(w, h, kind, seed=op))
                augs.append(((op, sign), (ra.OP_IDENTITY, 1)) if stage == 0 else ((ra.OP_IDENTITY, 1), (op, sign)))
    before_out, scratch, views, _, _, plan, before = _run(images, augs)
    bad = [(a.shape, ra.OP_NAMES[ops[stage][0]], ops[stage][1], int((v != ra.apply_model(a, *ops[stage])).sum()))
           for a, ops, v in zip(images, augs, views) if not np.array_equal(v, ra.apply_model(a, *ops[stage]))]
    print(f"{len(images)} images, {len(bad)} differ: {bad[:8]}")
    assert not bad
    assert _gaps_untouched(before, before_out, images, plan) and _gaps_untouched(np.full_like(scratch, FILL), scratch, images, plan)


def test_all_ordered_pairs_in_one_batch():
    a = image(37, 23, "noise", seed=9)
    augs = [((op0, -1 if op0 in ra.GEOMETRIC and (op0 + op1) % 2 else 1), (op1, -1 if op1 in ra.GEOMETRIC and op0 % 2 else 1))
            for op0 in range(1, 15) for op1 in range(1, 15)]
    assert len(augs) == 196
    _, _, views, _, _, _, _ = _run([a] * 196, augs)
    bad = [[(ra.OP_NAMES[o], s) for o, s in ops] for ops, v in zip(augs, views) if not np.array_equal(v, ra.augment_model(a, ops))]
    print(f"{len(bad)} of 196 pairs differ: {bad[:6]}")
    assert not bad


def test_a_refused_record_and_its_neighbours():
    images = [image(37, 23, "noise", seed=i) for i in range(8)]
    ops = ((ra.OP_EQUALIZE, 1), (ra.OP_SHEAR_X, -1))
    total = sum(resample._align16(a.size) for a in images) + 64

    def edit(plan):
        plan[1, ra.AUG_OFF] = (total - images[1].size) // 16 * 16 + 16   # aligned; its last bytes would lie behind the buffer
        plan[2, ra.AUG_STAGE0 + ra.AUG_STAGE_FIELDS] = 15             # an unknown operation in stage 1: stage 0 is not run either
        plan[3, ra.AUG_W] = resample.MAX_SOURCE_WIDTH + 1
        plan[4, ra.AUG_OFF] += 4                                      # not 16-byte aligned
        plan[5, ra.AUG_STAGE0 + ra.AUG_STAGE_FIELDS + 2] = 1 << 40    # a coefficient beyond the range the sums are safe in
        plan[6, ra.AUG_H] = -1

    out, scratch, views, _, _, plan, before = _run(images, [ops] * 8, edit=edit)
    assert np.array_equal(views[0], ra.augment_model(images[0], ops)) and np.array_equal(views[7], ra.augment_model(images[7], ops))
    for i in range(1, 7):
        assert np.array_equal(views[i], images[i]), i                 # left as it was
    offs = np.cumsum([0] + [resample._align16(a.size) for a in images])
    assert (scratch[offs[1]:offs[7]] == FILL).all() and (scratch[offs[8]:] == FILL).all() and (out[offs[8]:] == FILL).all()
    # the identity record is passed over: nothing is copied
    out, scratch, views, _, _, _, _ = _run(images[:2], [None, ops])
    assert np.array_equal(views[0], images[0]) and (scratch[:offs[1]] == FILL).all()
    assert np.array_equal(views[1], ra.augment_model(images[1], ops))


def test_entry_point_refusals():
    lib = _lib.lib()
    buf = torch.zeros(256, dtype=torch.uint8, device=DEV)
    other = torch.zeros(256, dtype=torch.uint8, device=DEV)
    plan = torch.zeros((2, ra.AUG_FIELDS), dtype=torch.int64, device=DEV)
    nws = ra.workspace_bytes(2)
    assert nws == 2 * (2 * 4096 + 768) and ra.workspace_bytes(0) == 0
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    b, o, p, w = (C.c_void_p(t.data_ptr()) for t in (buf, other, plan, ws))
    call = lib.m3ae_image_randaug_u8
    assert call(None, o, 256, p, 2, w, nws, 0, s) == -1 and call(b, None, 256, p, 2, w, nws, 0, s) == -1
    assert call(b, b, 256, p, 2, w, nws, 0, s) == -1 and call(b, o, 256, None, 2, w, nws, 0, s) == -1
    assert call(b, o, 0, p, 2, w, nws, 0, s) == -1 and call(b, o, 256, p, 0, w, nws, 0, s) == -1
    assert call(b, o, 256, p, 2, w, nws, 16, s) == -1 and call(b, o, 256, p, 65536, w, nws, 0, s) == -2
    assert call(C.c_void_p(buf.data_ptr() + 4), o, 252, p, 2, w, nws, 0, s) == -3
    assert call(b, o, 256, p, 2, w, nws - 1, 0, s) == -4
    assert call(b, o, 256, p, 2, w, nws, 15, s) == 0           # identity records: launched, nothing written
    torch.cuda.synchronize()
    assert not buf.any() and not other.any()


# ------------------------------------------------------------------------------------------------------------
# the datamodule and the trainer
# ------------------------------------------------------------------------------------------------------------
def _dm(root, tok, **over):
    cfg = tiny_config(compute_dtype="bf16", data_root=root, per_gpu_batchsize=4, num_workers=3, seed=1, **over)
    return data.ArrowDataModule(cfg, 0, 1, torch.device("cuda", 0), tokenizer=tok)


def _same(xs, ys):
    assert len(xs) == len(ys) and len(xs) > 0
    for x, y in zip(xs, ys):
        assert x["qid"] == y["qid"] and x["text"] == y["text"]
        assert x["image"][0].shape == y["image"][0].shape and torch.equal(x["image"][0], y["image"][0])
        assert torch.equal(x["text_ids"], y["text_ids"]) and torch.equal(x["text_masks"], y["text_masks"])


@pytest.mark.parametrize("tail", ("clip", "clip_resizedcrop"))
def test_datamodule_train_batches(tmp_path, tail, monkeypatch):
    from arrow_util import HashTokenizer, write_split
    from test_gpu_resample import _append_rows, _vqa_row     # two images with real transparency: device sources under randaug
    root, tok = str(tmp_path / "vqa"), HashTokenizer()
    write_split(root, "train", 12)
    write_split(root, "val", 4, seed=100)
    _append_rows(os.path.join(root, "vqa_vqa_rad_train.arrow"), _vqa_row)
    aug = dict(randaug=True, train_transform_keys=[tail])
    host, dev = _dm(root, tok, image_transform="host", **aug), _dm(root, tok, image_transform="device", **aug)
    plain = _dm(root, tok, image_transform="device", train_transform_keys=[tail])
    h0, d0, d0_again, d1 = (list(dm.train_batches(e)) for dm, e in ((host, 0), (dev, 0), (dev, 0), (dev, 1)))
    c0 = list(plain.train_batches(0))
    torch.cuda.synchronize()
    _same(h0, d0)                                            # device == host, bit for bit
    _same(d0, d0_again)                                      # an epoch is a function of its number
    assert dev.transform_stats["fallback"] == 0 and dev.transform_stats["device"] == 3 * dev.train_samples
    by_qid = lambda bs: {q: b["image"][0][i] for b in bs for i, q in enumerate(b["qid"])}
    e0, e1, c = by_qid(d0), by_qid(d1), by_qid(c0)
    assert set(e0) == set(e1) == set(c) and len(e0) == dev.train_samples
    n_moved = sum(1 for q in e0 if not torch.equal(e0[q], e1[q]))
    n_changed = sum(1 for q in e0 if not torch.equal(e0[q], c[q]))
    print(f"{tail}: {len(e0)} samples: {n_moved} differ between epochs 0 and 1, {n_changed} differ from the transform without randaug")
    assert n_moved > len(e0) // 2 and n_changed > len(e0) // 2
    # val never augments
    _same(list(dev.val_batches()), list(plain.val_batches()))
    _same(list(host.val_batches()), list(plain.val_batches()))
    if tail != "clip":
        return
    # an image beyond the caps is augmented and transformed on the host and joins the batch through an identity record
    monkeypatch.setattr(ra, "MAX_AUG_HEIGHT", 400)           # the 200 x 640 images of the table are beyond it now
    capped = _dm(root, tok, image_transform="device", **aug)
    _same(list(capped.train_batches(0)), h0)
    assert capped.transform_stats["fallback"] > 0 and capped.transform_stats["device"] > 0
    monkeypatch.undo()
    # image_dedup: one draw per distinct image and epoch = the plain batches of datasets that key their draws per image
    for mode in ("host", "device"):
        dd = _dm(root, tok, image_transform=mode, image_dedup=True, **aug)
        per_image = _dm(root, tok, image_transform=mode, **aug)
        assert dd.train_set.box_key == "image" and per_image.train_set.box_key == "sample"
        per_image.train_set.box_key = "image"
        got, want = list(dd.train_batches(1)), list(per_image.train_batches(1))
        torch.cuda.synchronize()
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g["qid"] == w["qid"]
            assert torch.equal(g["image"][0][g["image_index"]], w["image"][0])
            assert g["image"][0].shape[0] == len(set(g["image_index"].tolist()))


def test_two_trainer_steps_give_equal_losses_under_host_and_device_randaug(tmp_path, restore_deterministic_switch):  # noqa: F811
    from arrow_util import HashTokenizer, write_split
    from m3ae_amd import trainer
    root = str(tmp_path / "arrows")
    write_split(root, "train", 12)
    write_split(root, "val", 4, seed=100)
    tiny = ("image_size=64 hidden_size=128 num_heads=2 num_top_layer=2 input_image_embed_size=128 "
            "input_text_embed_size=128 vocab_size=1000 vit_width=128 vit_layers=3 text_hidden=128 text_layers=2 "
            "text_heads=2 text_inter=512").split()
    losses = {}
    for mode, aug in (("host", True), ("device", True), ("device", False)):
        argv = (["with", f"data_root={root}", "num_gpus=1", "num_nodes=1", "task_finetune_vqa_vqa_rad", "clip16",
                 "text_roberta", "per_gpu_batchsize=4", "batch_size=8", "max_steps=2", "num_workers=2", "deterministic=True",
                 f"image_transform={mode}", f"randaug={aug}", f"log_dir={tmp_path / (mode + str(aug))}", "seed=2"] + tiny)
        cfg = trainer.config_mod.parse_cli(argv)
        dev = torch.device("cuda", 0)
        torch.manual_seed(cfg["seed"])
        model = trainer.build_model(cfg, "cls", dev)
        dm = data.ArrowDataModule(cfg, 0, 1, dev, tokenizer=HashTokenizer())
        out = trainer.Trainer(cfg, model, dm, 0, 1, dev, log_every=1).fit()
        assert out["global_step"] == 2
        losses[(mode, aug)] = torch.tensor([h[1] for h in out["history"]])
    print("losses", losses)
    assert torch.isfinite(losses[("host", True)]).all()
    assert torch.equal(losses[("host", True)], losses[("device", True)])
    assert not torch.equal(losses[("device", True)], losses[("device", False)])
