"""Train transform "clip_resizedcrop", the part that needs no GPU: the config keys, the crop box of RandomResizedCrop, the
numpy model of the two kernels on a box against Pillow itself, the host transform, the plan of a pack made with boxes, and the
declaration of the table kernel's entry point."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header  # noqa: E402
from resample_cases import source  # noqa: E402

from m3ae_amd import _lib, resample  # noqa: E402
from m3ae_amd.config import compose, parse_cli  # noqa: E402
from m3ae_amd.data import clip_resized_crop  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = ["with", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta", "image_size=384"]


def _pil(a):
    from PIL import Image
    return Image.fromarray(a, {3: "RGB", 4: "RGBA"}[a.shape[2]])


def _pil_crop(img, box, size):
    from PIL import Image
    left, top, cw, ch = box
    return img.crop((left, top, left + cw, top + ch)).resize((size, size), Image.BICUBIC)


# ------------------------------------------------------------------------------------------------------------
# config
# ------------------------------------------------------------------------------------------------------------
def test_named_config_and_defaults():
    cfg = parse_cli(CLI + ["clip_resizedcrop"])
    assert cfg["train_transform_keys"] == ["clip_resizedcrop"] and cfg["val_transform_keys"] == ["clip"]
    for cfg in (parse_cli(CLI), compose()):
        assert cfg["train_transform_keys"] == ["clip"] and cfg["val_transform_keys"] == ["clip"]
    assert compose("clip_resizedcrop")["train_transform_keys"] == ["clip_resizedcrop"]
    # a val key loses the suffix before it is judged (base_dataset.py:39-41)
    assert parse_cli(CLI + ["val_transform_keys=['clip_resizedcrop']"])["val_transform_keys"] == ["clip_resizedcrop"]


@pytest.mark.parametrize("arg", ["train_transform_keys=['clip_randaug']", "train_transform_keys=['imagenet']",
                                 "train_transform_keys='clip'", "train_transform_keys=['clip','clip']", "train_transform_keys=[]",
                                 "val_transform_keys=['imagenet']", "val_transform_keys=['clip_randaug']"])
def test_bad_transform_key_is_a_value_error_that_names_the_allowed_values(arg):
    with pytest.raises(ValueError, match=r"clip"):
        parse_cli(CLI + [arg])
    with pytest.raises(ValueError, match=r"'clip'"):
        compose(**{arg.split("=")[0]: ["pixelbert"]})


def test_randaug_named_config_stays_unknown():
    for name in ("clip_randaug", "imagenet_randaug", "imagenet"):
        with pytest.raises(KeyError):
            parse_cli(CLI + [name])


# ------------------------------------------------------------------------------------------------------------
# the box
# ------------------------------------------------------------------------------------------------------------
def _fallback_box(w, h):
    if w / h < 3 / 4:
        cw, ch = w, int(round(w / (3 / 4)))
    elif w / h > 4 / 3:
        cw, ch = int(round(h * 4 / 3)), h
    else:
        cw, ch = w, h
    return (w - cw) // 2, (h - ch) // 2, cw, ch


def _a_try_can_fit(w, h):
    """Whether some (target, aspect) of the ranges gives a box inside w x h, rounding aside: sqrt(t a) <= w and sqrt(t / a) <= h
    <=> t / h^2 <= a <= w^2 / t, easiest at the smallest area t = 0.9 w h: 0.9 w / h <= a <= w / (0.9 h), a in [3/4, 4/3]."""
    return max(3 / 4, 0.9 * w / h) <= min(4 / 3, w / (0.9 * h))


@pytest.mark.parametrize("wh", [(512, 512), (700, 500), (383, 911), (150, 120)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_box_properties(wh):
    """The derived bounds of a box a try accepted.  A try draws t in [0.9, 1.0] w h and a in [3/4, 4/3] and sets
    cw = round(x), ch = round(y) with x = sqrt(t a), y = sqrt(t / a), so x y = t, x / y = a, and cw = x + dx, ch = y + dy with
    |dx|, |dy| <= 1/2.  Area: cw ch - t = cw ch - (cw - dx)(ch - dy) = cw dy + ch dx - dx dy, so
    |cw ch - t| <= (cw + ch) / 2 + 1/4 for the t that was drawn: the interval cw ch -+ that bound meets [0.9, 1.0] w h.
    Ratio: x in [cw - 1/2, cw + 1/2], y in [ch - 1/2, ch + 1/2] and 3/4 <= x / y <= 4/3 need
    (cw - 1/2) / (ch + 1/2) <= 4/3 and (cw + 1/2) / (ch - 1/2) >= 3/4 (ch >= 1).
    exp, log and sqrt are evaluated in float64: REL = 1e-9 covers their rounding (about 1e-16 relative each) and nothing else.
    383 x 911 is narrower than any box a try can accept (`_a_try_can_fit`: a <= w / (0.9 h) = 0.467 < 3/4), so all its boxes
    are the fallback; every source a try can fit must show a box that is not the fallback."""
    w, h = wh
    REL = 1e-9
    fallback, seen_other = _fallback_box(w, h), False
    for key in range(500):
        box = resample.random_resized_crop_box(w, h, resample.box_rng(7, 0, key, 0))
        assert box == resample.random_resized_crop_box(w, h, resample.box_rng(7, 0, key, 0))
        left, top, cw, ch = box
        assert all(isinstance(v, int) for v in box)
        assert cw >= 1 and ch >= 1 and 0 <= left and 0 <= top and left + cw <= w and top + ch <= h
        if box == fallback:
            continue
        seen_other = True
        e = 0.5 * (cw + ch) + 0.25
        assert cw * ch + e >= 0.9 * w * h * (1 - REL) and cw * ch - e <= w * h * (1 + REL), box
        assert (cw - 0.5) / (ch + 0.5) <= 4 / 3 * (1 + REL) and (cw + 0.5) / (ch - 0.5) >= 3 / 4 * (1 - REL), box
    assert seen_other == _a_try_can_fit(w, h)
    assert _a_try_can_fit(w, h) == (wh != (383, 911))
    # other keys, other boxes; and the generator is the key's alone (no global state)
    boxes = {resample.random_resized_crop_box(w, h, resample.box_rng(7, e, k, s)) for e in range(3) for k in range(3) for s in range(2)}
    assert len(boxes) > 1 or not _a_try_can_fit(w, h)
    assert resample.box_rng(1, 2, ("vqa_vqa_rad_train", 3)).random() == resample.box_rng(1, 2, ("vqa_vqa_rad_train", 3)).random()


@pytest.mark.parametrize("wh,want", [((97, 1300), (0, 585, 97, 129)), ((4100, 300), (1850, 0, 400, 300))])
def test_fallback_boxes_are_exact(wh, want):
    assert not _a_try_can_fit(*wh)
    for key in range(200):
        assert resample.random_resized_crop_box(*wh, resample.box_rng(3, key)) == want


# ------------------------------------------------------------------------------------------------------------
# the model on a box, and the host transform
# ------------------------------------------------------------------------------------------------------------
def _boxes(w, h, seed):
    return [(0, 0, w, h), (1, 1, w - 2, h - 2), resample.random_resized_crop_box(w, h, resample.box_rng(seed, w, h))]


def _model(rgb, box, size):
    left, top, cw, ch = box
    xb, xk = resample.axis_table(cw, size, 0, size)
    yb, yk = resample.axis_table(ch, size, 0, size)
    inter = resample._pass(rgb[top:top + ch, left:left + cw], xb, xk)
    return resample._pass(inter.transpose(1, 0, 2), yb, yk).transpose(1, 0, 2)


@pytest.mark.parametrize("size", (384, 224))
@pytest.mark.parametrize("wh", [(512, 512), (700, 500), (300, 200), (97, 131), (1024, 777)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_numpy_model_on_a_box_equals_pillow_bit_for_bit(wh, size):
    w, h = wh
    a = source(w, h, "noise", seed=size)
    boxes = _boxes(w, h, size)
    if wh == (512, 512):
        boxes.append((100, 17, size, size - 9))   # cw == size: Pillow skips the horizontal pass
    for box in boxes:
        want = np.asarray(_pil_crop(_pil(a), box, size))
        got = _model(a, box, size)
        assert got.shape == (size, size, 3) and np.array_equal(got, want), (wh, size, box)


def test_clip_resized_crop_on_an_image_with_real_transparency():
    rgba = np.concatenate([source(210, 160, "noise", seed=1), source(210, 160, "smooth", seed=2, channels=1)[..., None]], -1)
    img = _pil(rgba)
    assert img.getextrema()[3] != (255, 255)
    for size in (64, 224):
        for box in _boxes(210, 160, size):
            want = np.asarray(_pil_crop(img.convert("RGBA"), box, size).convert("RGB"))
            got = clip_resized_crop(img, size, box)
            assert got.dtype == np.uint8 and got.shape == (size, size, 3) and np.array_equal(got, want)
            route, crop, dev_box = resample.prepare(img, size, box)     # the device transform takes the finished crop as it is
            assert route == "fallback" and np.array_equal(crop, want) and dev_box == (0, 0, size, size)
    opaque = _pil(rgba[..., :3].copy())
    route, src, dev_box = resample.prepare(opaque, 64, (3, 4, 150, 120))
    assert route == "device" and np.array_equal(src, rgba[..., :3]) and dev_box == (3, 4, 150, 120)
    assert len(resample.prepare(opaque, 64)) == 2


# ------------------------------------------------------------------------------------------------------------
# the pack
# ------------------------------------------------------------------------------------------------------------
def test_pack_with_boxes_stays_inside_its_buffers():
    size = 224
    whs = [(300, 200), (97, 130), (224, 224), (300, 200), (512, 400)]
    boxes = [(10, 5, 280, 190), (0, 0, 97, 130), (0, 0, 224, 224), (20, 10, 280, 190), (100, 50, 224, 300)]
    srcs = [source(w, h, "noise") for w, h in whs]
    p = resample.pack_batch(srcs, size, False, map, boxes=boxes)
    assert "tab" not in p and p["plan"].shape == (5, resample.PLAN_FIELDS)
    plan, src = p["plan"].numpy(), p["src"].numpy()
    assert plan[:, resample.PLAN_BUILD].tolist() == [1, 1, 1, 0, 1] and (plan[:, 14:] == 0).all()
    assert np.array_equal(plan[0, resample.PLAN_KSX:resample.PLAN_YK + 1], plan[3, resample.PLAN_KSX:resample.PLAN_YK + 1])   # shared
    rows, used = 0, np.zeros(p["tab_ints"], dtype=np.int32)
    for i, (s, (left, top, cw, ch)) in enumerate(zip(srcs, boxes)):
        off, w, h, pitch, row0, nrows, ksx, ksy, xb, xk, yb, yk, irow0 = plan[i, :13].tolist()
        sh, sw = s.shape[:2]
        assert (w, h, pitch, row0, nrows, irow0) == (cw, ch, 3 * sw, 0, ch, rows)
        # every byte the passes read lies inside src, and is the box's
        assert 0 <= off and off + (h - 1) * pitch + 3 * w <= src.size
        got = np.stack([src[off + r * pitch:off + r * pitch + 3 * w].reshape(w, 3) for r in range(h)])
        assert np.array_equal(got, s[top:top + ch, left:left + cw])
        assert ksx == resample.axis_table(cw, size, 0, size)[1].shape[1] == resample.axis_ksize(cw, size)
        assert ksy == resample.axis_table(ch, size, 0, size)[1].shape[1] == resample.axis_ksize(ch, size)
        assert 0 <= xb and xb + 2 * size <= xk and xk + size * ksx <= yb and yb + 2 * size <= yk and yk + size * ksy <= p["tab_ints"]
        if plan[i, resample.PLAN_BUILD]:
            used[xb:yk + size * ksy] += 1
        rows += nrows
    assert p["rows"] == rows and (used == 1).all()        # the table sets tile tab: no overlap, nothing spare
    assert plan[2, resample.PLAN_KSX] == 1 and plan[4, resample.PLAN_KSX] == 1 and plan[4, resample.PLAN_KSY] == 7


def test_pack_without_boxes_is_the_pack_of_the_centre_crop():
    size = 224
    srcs = [source(w, h, "noise") for (w, h) in [(300, 200), (97, 130), (224, 224), (300, 200)]]
    for p in (resample.pack_batch(srcs, size), resample.pack_batch(srcs, size, False, map, None)):
        assert sorted(p) == ["plan", "rows", "size", "src", "tab"]
        plan, tab, src = p["plan"].numpy(), p["tab"].numpy(), p["src"].numpy()
        assert tab.dtype == np.int32 and (plan[:, 13:] == 0).all()
        rows, at, flat = 0, {}, []
        for i, s in enumerate(srcs):
            h, w, _ = s.shape
            t = resample.tables(w, h, size)
            if (w, h) not in at:
                at[(w, h)] = sum(f.size for f in flat)
                flat.append(t.flat)
            off = plan[i, resample.PLAN_SRC]
            assert off % 16 == 0 and np.array_equal(src[off:off + s.size].reshape(s.shape), s)
            assert plan[i, 1:13].tolist() == [w, h, 3 * w, t.row0, t.nrows, t.ksx, t.ksy, *(at[(w, h)] + o for o in t.offsets), rows]
            rows += t.nrows
        assert p["rows"] == rows and np.array_equal(tab, np.concatenate(flat))


# ------------------------------------------------------------------------------------------------------------
# the datasets: which key draws the box of which loaded image
# ------------------------------------------------------------------------------------------------------------
def test_datasets_key_their_boxes_per_loaded_image_or_per_image(tmp_path):
    import random
    from arrow_util import HashTokenizer, write_caption_split, write_split
    from m3ae_amd import data
    root, tok = str(tmp_path), HashTokenizer()
    write_split(root, "train", 5)
    write_split(root, "val", 3, seed=50)
    write_caption_split(root, "roco", "train", 6, seed=3)
    write_caption_split(root, "medicat", "train", 4, seed=4)
    crop = dict(train_transform="clip_resizedcrop", seed=11)

    def spy(ds):
        calls = []
        ds.image_u8 = lambda row, box_key=None: (calls.append((row, box_key)), np.zeros((2, 2, 3), np.uint8))[1]
        return calls

    vq = data.ArrowVQADataset(root, "train", 64, 32, tok, **crop)
    calls = spy(vq)
    row = vq.index_mapper[4][0]
    vq[4], vq.get(4, epoch=3), vq.get(4, epoch=3, key_index=40)
    vq.box_key = "image"
    vq.get(4, epoch=3), vq.image_by_key(("vqa_vqa_rad_train", row), 3), vq.image_by_key(("vqa_vqa_rad_train", row))
    image_key = (11, 3, ("vqa_vqa_rad_train", row))
    assert calls == [(row, None), (row, (11, 3, 4, 0)), (row, (11, 3, 40, 0)), (row, image_key), (row, image_key), (row, None)]
    for ds in (data.ArrowVQADataset(root, "val", 64, 32, tok, **crop), data.ArrowVQADataset(root, "train", 64, 32, tok, seed=11)):
        calls = spy(ds)                                       # another split, or the clip transform: never a box
        ds.get(1, epoch=3), ds.image_by_key((ds.names[0], 0), 3)
        assert not ds.augment and [k for _, k in calls] == [None, None]

    parts = [data.ArrowCaptionDataset(root, n, "train", 64, 32, tok, draw_false_image=2, **crop) for n in ("roco", "medicat")]
    both = data.ConcatDataset(parts)
    assert both.augment and not data.ConcatDataset([data.ArrowCaptionDataset(root, "roco", "train", 64, 32, tok)]).augment
    calls = spy(parts[1])
    index = len(parts[0]) + 2                                 # sample 2 of the second table: keyed by its GLOBAL index
    random.seed(5)
    both.get(index, 7)
    random.seed(5)
    false_rows = [parts[1].index_mapper[random.randint(0, len(parts[1]) - 1)][0] for _ in range(2)]
    assert calls == [(parts[1].index_mapper[2][0], (11, 7, index, 0)), (false_rows[0], (11, 7, index, 1)),
                     (false_rows[1], (11, 7, index, 2))]
    del calls[:]
    both[index]
    assert [k for _, k in calls] == [None] * 3
    # the real loader: the host transform of a keyed load is clip_resized_crop on the box the key draws
    from PIL import Image
    import io
    vq = data.ArrowVQADataset(root, "train", 64, 32, tok, **crop)
    img = Image.open(io.BytesIO(vq.table["image"][0].as_py()))
    box = resample.random_resized_crop_box(*img.size, resample.box_rng(11, 2, 0, 0))
    assert np.array_equal(vq.get(0, epoch=2)["image_u8"], clip_resized_crop(img, 64, box))
    vq.image_transform = "device"
    src, dev_box = vq.get(0, epoch=2)["image_u8"]
    assert dev_box == box and np.array_equal(src, np.asarray(img.convert("RGB")))


def test_entry_point_is_declared_and_bound():
    # bound as declared, and the ABI number: tests/test_host_logic.py, for the whole ABI
    assert abi_header.prototypes()["m3ae_image_resample_tables"] == ("int", [
        "const int64_t* plan", "int64_t B", "int64_t size", "int32_t* tab", "int64_t tab_ints", "void* stream"])
    assert resample.PLAN_BUILD == 13 and resample.PLAN_FIELDS == 16
    assert "lib.m3ae_image_resample_tables.argtypes" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
