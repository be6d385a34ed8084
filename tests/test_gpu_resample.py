"""Device image transform on the GPU (csrc/image.hip): the resized, cropped bytes equal PIL's and the fp32 image equals
`normalize_on_device` of the host crop, bit for bit; the arrow pipeline and the trainer give the same batches and losses
under image_transform="device" as under "host"."""
import io
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_cases import SIZES, TARGETS, kind_of, source  # noqa: E402

from m3ae_amd import data, resample  # noqa: E402
from m3ae_amd.config import tiny_config  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pil(a):
    from PIL import Image
    return Image.fromarray(a, "L" if a.ndim == 2 else {3: "RGB", 4: "RGBA"}[a.shape[2]])


def _host(arrays, size):
    """The host path: clip_resize_crop per image, uploaded, normalize_on_device."""
    u8 = torch.from_numpy(np.stack([data.clip_resize_crop(_pil(a), size) for a in arrays])).to(DEV)
    return u8, data.normalize_on_device(u8)


def _device(arrays, size, want_u8=True):
    srcs = []
    for a in arrays:
        route, s = resample.prepare(_pil(a), size)
        assert route == "device"
        srcs.append(s)
    dp = resample.upload(resample.pack_batch(srcs, size, pin=True), DEV)
    return resample.resample_on_device(dp, want_u8=want_u8)


def _check(arrays, size):
    want_u8, want_f = _host(arrays, size)
    got_f, got_u8 = _device(arrays, size)
    torch.cuda.synchronize()
    diff = (got_u8.int() - want_u8.int()).abs()
    print(f"size {size}: {len(arrays)} images, max |d uint8| per image {diff.flatten(1).max(1).values.tolist()}")
    assert torch.equal(got_u8, want_u8)
    assert torch.equal(got_f, want_f)
    only_f = _device(arrays, size, want_u8=False)     # uint8 output pointer null
    assert isinstance(only_f, torch.Tensor) and torch.equal(only_f, want_f)


@pytest.mark.parametrize("size", TARGETS)
def test_one_batch_of_all_case_sizes_equals_pil(size):
    arrays = [source(w, h, kind_of(i), seed=size) for i, (w, h) in enumerate(SIZES)]
    arrays += [source(w, h, kind_of(i + 1), seed=size + 1) for i, (w, h) in enumerate(SIZES[:6])]   # the other kind, shared tables
    arrays.append(source(333, 280, "noise", channels=1))                                          # an "L" source
    _check(arrays, size)


def test_batch_of_one_image():
    _check([source(700, 500, "noise", seed=5)], 384)


def test_batch_of_no_op_images():
    _check([source(384, 384, kind_of(i), seed=i) for i in range(5)], 384)


@pytest.mark.parametrize("w", [301, 302, 303])
def test_source_row_bytes_not_a_multiple_of_four(w):
    assert (w * 3) % 4 != 0
    _check([source(w, 257, "noise", seed=w), source(w, 257, "smooth", seed=w)], 224)


# ------------------------------------------------------------------------------------------------------------
# the arrow pipeline
# ------------------------------------------------------------------------------------------------------------
def _png(a):
    buf = io.BytesIO()
    _pil(a).save(buf, format="PNG")
    return buf.getvalue()


def _alpha_images():
    """Two images with real transparency: a translucent RGBA image and a grey + alpha image."""
    a = np.concatenate([source(120, 90, "noise", seed=11), source(120, 90, "smooth", seed=12, channels=1)[..., None]], -1)
    from PIL import Image
    la = Image.merge("LA", (_pil(source(70, 130, "noise", seed=13, channels=1)), _pil(source(70, 130, "smooth", seed=14, channels=1))))
    buf = io.BytesIO()
    la.save(buf, format="PNG")
    return [_png(a), buf.getvalue()]


def _append_rows(path, make_row):
    """Append the two alpha images to the arrow table at `path`; returns the row numbers they got."""
    import pyarrow as pa
    t = pa.ipc.RecordBatchFileReader(pa.memory_map(path, "r")).read_all()
    rows = {name: t[name].to_pylist() for name in t.column_names}
    first = t.num_rows
    for i, raw in enumerate(_alpha_images()):
        for name, v in make_row(first + i, raw).items():
            rows[name].append(v)
    t2 = pa.table(rows, schema=t.schema)
    with pa.OSFile(path, "wb") as sink:
        with pa.RecordBatchFileWriter(sink, t2.schema) as writer:
            writer.write_table(t2)
    return {first, first + 1}


def _vqa_row(i, raw):
    return {"image": raw, "questions": [f"is image {i} translucent ?", f"how translucent is image {i} ?"],
            "answers": [["yes"], ["very"]], "answer_labels": [[1], [2]], "answer_scores": [[1.0], [1.0]],
            "image_id": f"img{i}", "question_id": [9000 + 2 * i, 9001 + 2 * i], "answer_type": [0, 1], "split": "x"}


def _caption_row(i, raw):
    return {"image": raw, "caption": [f"a translucent image {i}"], "image_id": f"roco{i}", "split": "x"}


def _batches(cfg, tok, alpha_rows, seed):
    """All batches of train_batches(0) and val_batches(), the rows fetched (train set), and the stats."""
    dm = data.ArrowDataModule(cfg, 0, 1, torch.device("cuda", 0), tokenizer=tok)
    fetched = []
    for ds in {id(d): d for d in (dm.train_set, dm.val_set)}.values():
        for part in getattr(ds, "parts", [ds]):
            inner = part.image_u8
            part.image_u8 = lambda row, inner=inner, part=part: (fetched.append((part.names[0], row)), inner(row))[1]
    random.seed(seed)
    out = list(dm.train_batches(0)) + list(dm.val_batches())
    torch.cuda.synchronize()
    n_alpha = sum(1 for name, row in fetched if row in alpha_rows.get(name, ()))
    return out, len(fetched), n_alpha, dict(dm.transform_stats)


def _same_batches(host, dev, keys):
    assert len(host) == len(dev)
    for hb, db in zip(host, dev):
        assert set(hb) == set(db)
        for k in keys:
            hv, dv = hb[k], db[k]
            if isinstance(hv, list):
                hv, dv = hv[0], dv[0]
            assert hv.dtype == dv.dtype and hv.shape == dv.shape and torch.equal(hv, dv), k
        assert hb["text"] == db["text"]


def test_vqa_table_batches_equal_the_host_path(tmp_path):
    from arrow_util import HashTokenizer, write_split
    root = str(tmp_path / "vqa")
    write_split(root, "train", 12)
    write_split(root, "val", 4, seed=100)
    alpha = {"vqa_vqa_rad_train": _append_rows(os.path.join(root, "vqa_vqa_rad_train.arrow"), _vqa_row)}
    res = {}
    for mode in ("host", "device"):
        cfg = tiny_config(compute_dtype="bf16", data_root=root, per_gpu_batchsize=4, num_workers=3, seed=1, image_transform=mode)
        res[mode] = _batches(cfg, HashTokenizer(), alpha, 0)
    _same_batches(res["host"][0], res["device"][0], ("image", "text_ids", "text_masks", "text_labels"))
    _, n, n_alpha, stats = res["device"]
    assert n_alpha == 4                                   # two alpha images, two questions each
    assert stats == {"device": n - n_alpha, "fallback": n_alpha}
    assert res["host"][3] == {"device": 0, "fallback": 0}


def test_caption_table_batches_with_false_images_equal_the_host_path(tmp_path):
    from arrow_util import HashTokenizer, write_caption_split
    root = str(tmp_path / "cap")
    write_caption_split(root, "roco", "train", 10, seed=3)
    write_caption_split(root, "roco", "val", 3, seed=77)
    alpha = {"roco_train": _append_rows(os.path.join(root, "roco_train.arrow"), _caption_row)}
    res = {}
    for mode in ("host", "device"):
        # one worker: the negatives are drawn from Python's global `random` stream inside the workers
        cfg = tiny_config(compute_dtype="bf16", data_root=root, per_gpu_batchsize=4, num_workers=1, seed=1, datasets=["roco"],
                          draw_false_image=1, image_transform=mode)
        res[mode] = _batches(cfg, HashTokenizer(), alpha, 1234)
    _same_batches(res["host"][0], res["device"][0], ("image", "false_image_0", "text_ids", "text_masks", "text_labels"))
    _, n, n_alpha, stats = res["device"]
    assert n_alpha == res["host"][2] and n_alpha >= 2 and n == res["host"][1]
    assert stats == {"device": n - n_alpha, "fallback": n_alpha}


@pytest.fixture
def restore_deterministic_switch():
    """A model built from a config with deterministic=True switches ordered reductions on process-wide
    (modules/m3ae_module.py); later tests must find the switch as it was."""
    from m3ae_amd import ops
    prev = ops.deterministic()
    try:
        yield
    finally:
        ops.set_deterministic(prev)


def test_two_trainer_steps_give_equal_losses_under_host_and_device_transform(tmp_path, restore_deterministic_switch):
    from arrow_util import HashTokenizer, write_split
    from m3ae_amd import trainer
    root = str(tmp_path / "arrows")
    write_split(root, "train", 12)
    write_split(root, "val", 4, seed=100)
    _append_rows(os.path.join(root, "vqa_vqa_rad_train.arrow"), _vqa_row)
    tiny = ("image_size=64 hidden_size=128 num_heads=2 num_top_layer=2 input_image_embed_size=128 "
            "input_text_embed_size=128 vocab_size=1000 vit_width=128 vit_layers=3 text_hidden=128 text_layers=2 "
            "text_heads=2 text_inter=512").split()
    losses = {}
    for mode in ("host", "device"):
        argv = (["with", f"data_root={root}", "num_gpus=1", "num_nodes=1", "task_finetune_vqa_vqa_rad", "clip16",
                 "text_roberta", "per_gpu_batchsize=4", "batch_size=8", "max_steps=2", "num_workers=2", "deterministic=True",
                 f"image_transform={mode}", f"log_dir={tmp_path / mode}", "seed=2"] + tiny)
        cfg = trainer.config_mod.parse_cli(argv)
        dev = torch.device("cuda", 0)
        torch.manual_seed(cfg["seed"])
        model = trainer.build_model(cfg, "cls", dev)
        dm = data.ArrowDataModule(cfg, 0, 1, dev, tokenizer=HashTokenizer())
        tr = trainer.Trainer(cfg, model, dm, 0, 1, dev, log_every=1)
        out = tr.fit()
        assert out["global_step"] == 2
        losses[mode] = torch.tensor([h[1] for h in out["history"]])
        assert (dm.transform_stats["device"] > 0) == (mode == "device")
    print("losses", losses)
    assert len(losses["host"]) == 2 and torch.isfinite(losses["host"]).all()
    assert torch.equal(losses["host"], losses["device"])
