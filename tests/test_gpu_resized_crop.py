"""Train transform "clip_resizedcrop" on the GPU: the coefficient tables `m3ae_image_resample_tables` builds equal
`resample.axis_table` bit for bit, a batch of boxed sources equals `img.crop(box).resize(...)` of Pillow bit for bit, and the
arrow pipeline gives the same train batches under image_transform="device" as under "host"."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resample_cases import kind_of, source  # noqa: E402

from m3ae_amd import _lib, data, resample  # noqa: E402
from m3ae_amd.config import tiny_config  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7777
# every in-size of the pairs the transform was specified on (identity, +-1 around it, 1 - 3 px sources, upscales, 4100 and the
# widest row), each against both targets and on either axis
INS = [384, 383, 385, 224, 223, 225, 1, 2, 3, 97, 150, 777, 1024, 4100, 8192]
_tables = {}


def _axis(n, size):
    if (n, size) not in _tables:
        _tables[(n, size)] = resample.axis_table(n, size, 0, size)
    return _tables[(n, size)]


def _pil(a):
    from PIL import Image
    return Image.fromarray(a, "RGB")


def _run_tables(plan, size, tab):
    lib = _lib.lib()
    plan_d, tab_d = torch.from_numpy(plan).to(DEV), torch.from_numpy(tab).to(DEV)
    rc = lib.m3ae_image_resample_tables(C.c_void_p(plan_d.data_ptr()), plan.shape[0], size, C.c_void_p(tab_d.data_ptr()), tab.size,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return tab_d.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------
# 1. the tables
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (384, 224))
def test_device_tables_equal_axis_table_bit_for_bit(size):
    n = len(INS)
    dims = [(INS[j], INS[(j + 5) % n]) for j in range(n)] + [(INS[j], INS[(j + 9) % n]) for j in range(n)]
    GAP = 5                                                  # sentinel ints between any two tables
    plan = np.zeros((len(dims) + 4, resample.PLAN_FIELDS), dtype=np.int64)
    want_parts, at = [], 0

    def region(w, h, ksx, ksy, fill):
        """Lay out one table set behind the previous one; `fill`: the expected content (None: stays sentinel)."""
        nonlocal at
        offs = []
        for ints, part in zip((2 * size, size * ksx, 2 * size, size * ksy), fill or (None,) * 4):
            offs.append(at)
            want_parts.append(np.full(ints, SENTINEL, dtype=np.int32) if part is None else part.astype(np.int32).ravel())
            want_parts.append(np.full(GAP, SENTINEL, dtype=np.int32))
            at += ints + GAP
        return offs

    def record(i, w, h, ksx, ksy, offs, build):
        plan[i, :14] = (0, w, h, 3 * w, 0, h, ksx, ksy, *offs, 0, build)

    def padded(k, ks):
        return np.concatenate([k, np.zeros((k.shape[0], ks - k.shape[1]), dtype=k.dtype)], 1)

    for i, (w, h) in enumerate(dims):
        (xb, xk), (yb, yk) = _axis(w, size), _axis(h, size)
        extra = 3 if i == 4 else 0                           # one record with longer rows than Pillow's: zero-filled to ks
        ksx, ksy = xk.shape[1] + extra, yk.shape[1] + extra
        assert xk.shape[1] == resample.axis_ksize(w, size) and yk.shape[1] == resample.axis_ksize(h, size)
        record(i, w, h, ksx, ksy, region(w, h, ksx, ksy, (xb, padded(xk, ksx), yb, padded(yk, ksy))), 1)
    i = len(dims)
    # PLAN_BUILD == 0: a valid record whose region stays as it was
    record(i, 700, 500, 9, 7, region(700, 500, 9, 7, None), 0)
    # a y-coefficient table that points beyond tab (offset set below, once tab's length is known): nothing of the record is written
    bad_off = region(777, 97, resample.axis_ksize(777, size), resample.axis_ksize(97, size), None)
    # ksx one too small: nothing of the record is written
    ks_small = resample.axis_ksize(1024, size) - 1
    record(i + 2, 1024, 300, ks_small, resample.axis_ksize(300, size),
           region(1024, 300, ks_small, resample.axis_ksize(300, size), None), 1)
    # and a good record behind the refused ones
    (xb, xk), (yb, yk) = _axis(150, size), _axis(97, size)
    record(i + 3, 150, 97, xk.shape[1], yk.shape[1], region(150, 97, xk.shape[1], yk.shape[1], (xb, xk, yb, yk)), 1)
    want = np.concatenate(want_parts)
    assert want.size == at
    ksy = resample.axis_ksize(97, size)
    bad_off[3] = at - size * ksy + 1                          # its last int would be tab[tab_ints]
    record(i + 1, 777, 97, resample.axis_ksize(777, size), ksy, bad_off, 1)
    assert len(plan) >= 30 and (plan[:, resample.PLAN_XB:resample.PLAN_YK + 1] >= 0).all()

    got = _run_tables(plan, size, np.full(at, SENTINEL, dtype=np.int32))
    bad = np.flatnonzero(got != want)
    print(f"size {size}: {len(plan)} records, {at} table ints, {bad.size} differ" +
          (f"; first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}, max |d| {np.abs(got[bad].astype(np.int64) - want[bad]).max()}"
           if bad.size else ""))
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------
# 2. end to end
# ------------------------------------------------------------------------------------------------------------
def _boxes(w, h, size, seed):
    out = [(0, 0, w, h), (1, 1, w - 2, h - 2), resample.random_resized_crop_box(w, h, resample.box_rng(seed, w, h))]
    if w >= size + 3 and h >= 100:
        out.append((3, 2, size, h - 5))                      # cw == size: the horizontal pass is the identity
    return out


@pytest.mark.parametrize("size", (384, 224))
def test_boxed_batch_equals_pillow_bit_for_bit(size):
    from PIL import Image
    arrays, boxes, want = [], [], []
    for i, (w, h) in enumerate([(512, 512), (700, 500), (383, 911), (150, 120), (1024, 777), (4100, 300)]):
        a = source(w, h, kind_of(i), seed=size)
        for left, top, cw, ch in _boxes(w, h, size, size):
            arrays.append(a)
            boxes.append((left, top, cw, ch))
            want.append(np.asarray(_pil(a).crop((left, top, left + cw, top + ch)).resize((size, size), Image.BICUBIC)))
    assert sum(1 for b in boxes if b[2] == size) >= 3 and len({b[2:] for b in boxes}) > 15
    pack = resample.pack_batch(arrays, size, True, map, boxes=boxes)
    assert "tab" not in pack
    got_f, got_u8 = resample.resample_on_device(resample.upload(pack, DEV), want_u8=True)
    want_u8 = torch.from_numpy(np.stack(want)).to(DEV)
    want_f = data.normalize_on_device(want_u8)
    torch.cuda.synchronize()
    diff = (got_u8.int() - want_u8.int()).abs().flatten(1).max(1).values.tolist()
    print(f"size {size}: {len(arrays)} images, max |d uint8| per image {diff}")
    assert torch.equal(got_u8, want_u8)
    assert torch.equal(got_f, want_f)


# ------------------------------------------------------------------------------------------------------------
# 3. the datamodule
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


def test_datamodule_train_batches(tmp_path):
    from arrow_util import HashTokenizer, write_split
    from test_gpu_resample import _append_rows, _vqa_row     # two images with real transparency: the fallback route
    root, tok = str(tmp_path / "vqa"), HashTokenizer()
    write_split(root, "train", 12)
    write_split(root, "val", 4, seed=100)
    _append_rows(os.path.join(root, "vqa_vqa_rad_train.arrow"), _vqa_row)
    crop = dict(train_transform_keys=["clip_resizedcrop"])
    host, dev = _dm(root, tok, image_transform="host", **crop), _dm(root, tok, image_transform="device", **crop)
    plain = _dm(root, tok, image_transform="device")
    h0, d0, d0_again, d1 = (list(dm.train_batches(e)) for dm, e in ((host, 0), (dev, 0), (dev, 0), (dev, 1)))
    c0 = list(plain.train_batches(0))
    torch.cuda.synchronize()
    _same(h0, d0)                                            # device == host, bit for bit
    _same(d0, d0_again)                                      # an epoch is a function of its number
    assert dev.transform_stats["fallback"] == 3 * 4 and dev.transform_stats["device"] > 0
    by_qid = lambda bs: {q: b["image"][0][i] for b in bs for i, q in enumerate(b["qid"])}
    e0, e1, c = by_qid(d0), by_qid(d1), by_qid(c0)
    assert set(e0) == set(e1) == set(c) and len(e0) == dev.train_samples
    n_moved = sum(1 for q in e0 if not torch.equal(e0[q], e1[q]))
    n_cropped = sum(1 for q in e0 if not torch.equal(e0[q], c[q]))
    print(f"{len(e0)} samples: {n_moved} differ between epochs 0 and 1, {n_cropped} differ from the clip transform")
    assert n_moved > len(e0) // 2 and n_cropped > len(e0) // 2
    # val never crops
    _same(list(dev.val_batches()), list(plain.val_batches()))
    _same(list(host.val_batches()), list(plain.val_batches()))

    # image_dedup: one box per distinct image and epoch = the plain batches of datasets that key their boxes per image
    for mode in ("host", "device"):
        dd = _dm(root, tok, image_transform=mode, image_dedup=True, **crop)
        per_image = _dm(root, tok, image_transform=mode, **crop)
        assert dd.train_set.box_key == "image" and per_image.train_set.box_key == "sample"
        per_image.train_set.box_key = "image"
        got, want = list(dd.train_batches(1)), list(per_image.train_batches(1))
        torch.cuda.synchronize()
        assert len(got) == len(want)
        distinct = 0
        for g, w in zip(got, want):
            assert g["qid"] == w["qid"]
            assert torch.equal(g["image"][0][g["image_index"]], w["image"][0])
            distinct += len(set(g["image_index"].tolist()))
            assert g["image"][0].shape[0] == len(set(g["image_index"].tolist()))
        assert dd.transform_stats.decodes == distinct and per_image.transform_stats.decodes == dd.train_samples


# ------------------------------------------------------------------------------------------------------------
# 4. refusals before any launch
# ------------------------------------------------------------------------------------------------------------
def test_entry_point_refusals():
    lib = _lib.lib()
    plan = torch.zeros((2, resample.PLAN_FIELDS), dtype=torch.int64, device=DEV)
    tab = torch.full((64,), SENTINEL, dtype=torch.int32, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, t = C.c_void_p(plan.data_ptr()), C.c_void_p(tab.data_ptr())
    call = lib.m3ae_image_resample_tables
    assert call(None, 2, 384, t, 64, s) == -1 and call(p, 2, 384, None, 64, s) == -1
    assert call(p, 0, 384, t, 64, s) == -1 and call(p, 2, 0, t, 64, s) == -1 and call(p, 2, 384, t, 0, s) == -1
    assert call(p, 2, 5000, t, 64, s) == -2 and call(p, 65536, 384, t, 64, s) == -2
    assert call(p, 2, 384, t, 64, s) == 0                     # PLAN_BUILD == 0 everywhere: launched, nothing written
    torch.cuda.synchronize()
    assert (tab == SENTINEL).all()
