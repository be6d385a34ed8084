"""RandAugment(2, 9) (config key `randaug`), the part that needs no GPU: the numpy model of every operation against Pillow itself,
the degenerate histograms, all ordered pairs through the host path, the keyed draw, the config key, the datasets' keys, the
augment plan of a pack and the declaration of the entry points."""
import io
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header  # noqa: E402
from randaug_cases import HOST_SIZES, OP_SIGNS, degenerate_images, image  # noqa: E402

from m3ae_amd import _lib, data, resample  # noqa: E402
from m3ae_amd import randaug as ra  # noqa: E402
from m3ae_amd.config import compose, parse_cli  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = ["with", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta", "image_size=384"]


def _pil(a):
    from PIL import Image
    return Image.fromarray(a, "RGB")


def _pillow(a, op, sign):
    return np.asarray(ra.apply_pil(_pil(a), op, sign))


# ------------------------------------------------------------------------------------------------------------
# the values and the model
# ------------------------------------------------------------------------------------------------------------
def test_values_are_the_references_expression_at_magnitude_9():
    want = {ra.OP_ROTATE: 9.0, ra.OP_POSTERIZE: 1.2, ra.OP_SOLARIZE: 76.8, ra.OP_SOLARIZE_ADD: 33.0, ra.OP_COLOR: 0.64,
            ra.OP_CONTRAST: 0.64, ra.OP_BRIGHTNESS: 0.64, ra.OP_SHARPNESS: 0.64, ra.OP_SHEAR_X: 0.09, ra.OP_SHEAR_Y: 0.09,
            ra.OP_TRANSLATE_X: 30.0, ra.OP_TRANSLATE_Y: 30.0}
    assert [op for op, _, _ in ra.AUGMENT_LIST] == list(range(1, 15)) and len(ra.OP_NAMES) == 15
    for op, lo, hi in ra.AUGMENT_LIST:
        assert ra.VALUE[op] == (float(9) / 30) * float(hi - lo) + lo
        if op in want:
            assert abs(ra.VALUE[op] - want[op]) < 1e-12
    # what the kernels hold as constants: the float32 of the enhance factor, the integer forms of the three thresholds
    assert all(np.float32(ra.VALUE[op]) == np.float32(0.64) for op in (ra.OP_COLOR, ra.OP_CONTRAST, ra.OP_BRIGHTNESS, ra.OP_SHARPNESS))
    assert ra.VALUE[ra.OP_SOLARIZE_ADD] == 33.0 and int(ra.VALUE[ra.OP_POSTERIZE]) == 1 and 76 < ra.VALUE[ra.OP_SOLARIZE] < 77
    assert ra.VALUE[ra.OP_TRANSLATE_X] == 30.0 and ra.VALUE[ra.OP_TRANSLATE_Y] == 30.0   # an integer shift (Pillow's translate path)


@pytest.mark.parametrize("wh", HOST_SIZES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_model_equals_pillow_per_operation(wh):
    w, h = wh
    for kind in ("noise", "smooth"):
        a = image(w, h, kind, seed=3)
        for op, sign in OP_SIGNS:
            got, want = ra.apply_model(a, op, sign), _pillow(a, op, sign)
            assert got.dtype == np.uint8 and got.shape == a.shape
            assert np.array_equal(got, want), (wh, kind, ra.OP_NAMES[op], sign, int((got != want).sum()))


def test_geometric_model_on_a_large_image():
    """4100 x 3000: x * 65536 passes 2^28 and the rotation's offsets are large -- the 16.16 coordinates near their range."""
    a = image(4100, 3000, "noise", seed=1)
    for op, sign in OP_SIGNS:
        if op in ra.GEOMETRIC:
            assert np.array_equal(ra.apply_model(a, op, sign), _pillow(a, op, sign)), (ra.OP_NAMES[op], sign)


def test_degenerate_histograms():
    cases = degenerate_images()
    # the cases are what they claim to be
    h = ra.histograms(cases["step0"])
    for c in range(3):
        used = np.flatnonzero(h[c])
        assert len(used) > 1 and (h[c].sum() - h[c][used[-1]]) // 255 == 0
    assert (np.count_nonzero(ra.histograms(cases["const"])[:3], axis=1) == 1).all()
    assert np.count_nonzero(ra.histograms(cases["one_bin"])[1]) == 1
    hf = ra.histograms(cases["full"])
    assert (hf[:3, 0] > 0).all() and (hf[:3, 255] > 0).all()
    ident = np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 256))
    assert np.array_equal(ra.point_lut(ra.OP_EQUALIZE, h), ident) and np.array_equal(ra.point_lut(ra.OP_AUTOCONTRAST, hf), ident)
    assert np.array_equal(ra.point_lut(ra.OP_EQUALIZE, ra.histograms(cases["const"])), ident)
    assert not np.array_equal(ra.point_lut(ra.OP_AUTOCONTRAST, ra.histograms(cases["narrow"])), ident)
    for name, a in cases.items():
        assert np.array_equal(ra.histograms(a)[3], np.asarray(_pil(a).convert("L").histogram())), name
        assert np.array_equal(ra.histograms(a)[:3].ravel(), np.asarray(_pil(a).histogram())), name
        for op in ra.POINT_OPS:
            assert np.array_equal(ra.apply_model(a, op), _pillow(a, op, 1)), (name, ra.OP_NAMES[op])


def test_all_ordered_pairs_model_against_the_host_path():
    a = image(37, 23, "noise", seed=9)
    n = 0
    for op0 in range(1, 15):
        for op1 in range(1, 15):
            ops = ((op0, -1 if op0 in ra.GEOMETRIC and (op0 + op1) % 2 else 1), (op1, -1 if op1 in ra.GEOMETRIC and op0 % 2 else 1))
            want = np.asarray(ra.augment_pil(_pil(a), ops))
            assert np.array_equal(ra.augment_model(a, ops), want), [(ra.OP_NAMES[o], s) for o, s in ops]
            n += 1
    assert n == 196


# ------------------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------------------
def test_draws_are_keyed_and_cover_every_operation_and_sign():
    random.seed(123)
    state = random.getstate()
    draws = [ra.draw(ra.aug_rng(7, 0, key, 0)) for key in range(500)]
    assert random.getstate() == state                                   # no global generator is read or advanced
    assert draws == [ra.draw(ra.aug_rng(7, 0, key, 0)) for key in range(500)]
    assert draws != [ra.draw(ra.aug_rng(7, 1, key, 0)) for key in range(500)]   # another epoch
    assert ra.draw(ra.aug_rng(1, 2, ("vqa_vqa_rad_train", 3))) == ra.draw(ra.aug_rng(1, 2, ("vqa_vqa_rad_train", 3)))
    for d in draws:
        assert len(d) == 2
        for op, sign in d:
            assert 1 <= op <= 14 and sign in (1, -1) and (sign == 1 or op in ra.GEOMETRIC)
    for slot in range(2):
        assert {d[slot][0] for d in draws} == set(range(1, 15))         # a fixed fact of these 500 keys, not a probability
        assert {d[slot] for d in draws if d[slot][0] in ra.GEOMETRIC} == {(op, s) for op in ra.GEOMETRIC for s in (1, -1)}
    # the stream: two choices, then one random() per geometric operation in applying order
    for key in range(50):
        r = ra.aug_rng(7, 0, key, 0)
        picked = [op for op, _, _ in r.choices(ra.AUGMENT_LIST, k=2)]
        want = tuple((op, (-1 if r.random() > 0.5 else 1) if op in ra.GEOMETRIC else 1) for op in picked)
        assert draws[key] == want
    # the crop box keeps its own key: the box of a key is the one it is without randaug
    assert resample.box_rng(7, 0, 3, 0).random() != ra.aug_rng(7, 0, 3, 0).random()


# ------------------------------------------------------------------------------------------------------------
# config
# ------------------------------------------------------------------------------------------------------------
def test_config_key():
    assert parse_cli(CLI)["randaug"] is False and compose()["randaug"] is False
    cfg = parse_cli(CLI + ["randaug=True"])
    assert cfg["randaug"] is True and cfg["train_transform_keys"] == ["clip"]
    cfg = parse_cli(CLI + ["randaug=True", "clip_resizedcrop"])
    assert cfg["randaug"] is True and cfg["train_transform_keys"] == ["clip_resizedcrop"]
    for bad in ("randaug=2", "randaug='yes'", "randaug=(2,9)"):
        with pytest.raises(ValueError, match="randaug"):
            parse_cli(CLI + [bad])
    with pytest.raises(KeyError):                                       # the reference's own names stay unknown
        parse_cli(CLI + ["clip_randaug"])
    assert "clip_randaug" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_graphed_step_refuses_randaug():
    import torch
    from m3ae_amd import graph
    from m3ae_amd.config import tiny_config
    from m3ae_amd.modules.m3ae_module import M3AETransformerSS, _HParams
    model = M3AETransformerSS.__new__(M3AETransformerSS)     # the refusal reads the config alone, before anything is built
    model.__dict__["hparams"] = _HParams(config=tiny_config(randaug=True))
    model.__dict__["_dtype"] = torch.bfloat16
    with pytest.raises(ValueError, match="randaug"):
        graph.GraphedStep(model, {}, 10)


def _open(ds, row):
    from PIL import Image
    return Image.open(io.BytesIO(ds.table["image"][row].as_py()))


def test_datasets_augment_train_fetches_only_and_key_them_like_the_box(tmp_path):
    from arrow_util import HashTokenizer, write_caption_split, write_split
    root, tok = str(tmp_path), HashTokenizer()
    write_split(root, "train", 5)
    write_split(root, "val", 3, seed=50)
    write_caption_split(root, "roco", "train", 6, seed=3)

    def spy(ds):
        calls = []
        ds.image_u8 = lambda row, box_key=None, aug_key=None: (calls.append((row, box_key, aug_key)), np.zeros((2, 2, 3), np.uint8))[1]
        return calls

    vq = data.ArrowVQADataset(root, "train", 64, 32, tok, seed=11, randaug=True)
    assert vq.augment and vq.randaug and not vq.crop
    calls = spy(vq)
    row = vq.index_mapper[4][0]
    vq[4], vq.get(4, epoch=3), vq.get(4, epoch=3, key_index=40)
    vq.box_key = "image"                                                # the dedup keying rule: one draw per distinct image and epoch
    vq.get(4, epoch=3), vq.image_by_key(("vqa_vqa_rad_train", row), 3), vq.image_by_key(("vqa_vqa_rad_train", row))
    image_key = (11, 3, ("vqa_vqa_rad_train", row))
    assert calls == [(row, None, None), (row, None, (11, 3, 4, 0)), (row, None, (11, 3, 40, 0)), (row, None, image_key),
                     (row, None, image_key), (row, None, None)]
    both = data.ArrowVQADataset(root, "train", 64, 32, tok, seed=11, randaug=True, train_transform="clip_resizedcrop")
    calls = spy(both)
    both.get(4, epoch=3)
    assert calls == [(row, (11, 3, 4, 0), (11, 3, 4, 0))]               # one key; the two generators differ by their prefix
    for ds in (data.ArrowVQADataset(root, "val", 64, 32, tok, seed=11, randaug=True), data.ArrowVQADataset(root, "train", 64, 32, tok, seed=11)):
        calls = spy(ds)                                                 # another split, or randaug off: never a key
        ds.get(1, epoch=3), ds.image_by_key((ds.names[0], 0), 3)
        assert not ds.augment and [c[1:] for c in calls] == [(None, None)] * 2
    cap = data.ArrowCaptionDataset(root, "roco", "train", 64, 32, tok, draw_false_image=1, seed=11, randaug=True)
    calls = spy(cap)
    random.seed(5)
    data.ConcatDataset([cap]).get(2, 7)
    assert [c[2] for c in calls] == [(11, 7, 2, 0), (11, 7, 2, 1)]      # false_image_0 has its own slot

    # the real loader.  randaug off: a train fetch is the plain transform, byte for byte, under either image_transform
    plain = data.ArrowVQADataset(root, "train", 64, 32, tok, seed=11)
    for i in range(len(plain)):
        r = plain.index_mapper[i][0]
        assert np.array_equal(plain.get(i, epoch=2)["image_u8"], data.clip_resize_crop(_open(plain, r), 64))
    plain.image_transform = "device"
    assert all(isinstance(plain.get(i, epoch=2)["image_u8"], np.ndarray) for i in range(len(plain)))
    # randaug on, host: Pillow's operations of the key's draw on the RGB image, then the tail
    vq = data.ArrowVQADataset(root, "train", 64, 32, tok, seed=11, randaug=True)
    changed = 0
    for i in range(len(vq)):
        r = vq.index_mapper[i][0]
        ops = ra.draw(ra.aug_rng(11, 2, i, 0))
        want = data.clip_resize_crop(ra.augment_pil(_open(vq, r), ops), 64)
        got = vq.get(i, epoch=2)["image_u8"]
        assert np.array_equal(got, want)
        assert np.array_equal(vq[i]["image_u8"], data.clip_resize_crop(_open(vq, r), 64))     # no epoch, no augmentation
        changed += not np.array_equal(got, vq[i]["image_u8"])
    assert changed > len(vq) // 2
    # device: the RGB source with its operations; the model of the plan's stages then equals the host's image
    vq.image_transform = "device"
    for i in range(len(vq)):
        r = vq.index_mapper[i][0]
        src, box, ops = vq.get(i, epoch=2)["image_u8"]
        assert box is None and ops == ra.draw(ra.aug_rng(11, 2, i, 0))
        assert np.array_equal(src, np.asarray(_open(vq, r).convert("RGB")))
        vq.image_transform = "host"
        assert np.array_equal(data.clip_resize_crop(_pil(ra.augment_model(src, ops)), 64), vq.get(i, epoch=2)["image_u8"])
        vq.image_transform = "device"
    both = data.ArrowVQADataset(root, "train", 64, 32, tok, seed=11, randaug=True, train_transform="clip_resizedcrop",
                                image_transform="device")
    crop_only = data.ArrowVQADataset(root, "train", 64, 32, tok, seed=11, train_transform="clip_resizedcrop", image_transform="device")
    src, box, ops = both.get(0, epoch=2)["image_u8"]
    assert box == crop_only.get(0, epoch=2)["image_u8"][1] and ops == ra.draw(ra.aug_rng(11, 2, 0, 0))


def test_an_image_beyond_the_caps_is_augmented_on_the_host(monkeypatch):
    a = image(101, 77, "noise", seed=2)
    ops = ((ra.OP_ROTATE, -1), (ra.OP_EQUALIZE, 1))
    route, src, box, got_ops = resample.prepare(_pil(a), 64, None, ops)
    assert route == "device" and np.array_equal(src, a) and box is None and got_ops == ops
    monkeypatch.setattr(ra, "MAX_AUG_HEIGHT", 50)
    route, crop, box, got_ops = resample.prepare(_pil(a), 64, None, ops)
    assert route == "fallback" and got_ops is None and box is None
    assert np.array_equal(crop, data.clip_resize_crop(ra.augment_pil(_pil(a), ops), 64))
    route, crop, box, got_ops = resample.prepare(_pil(a), 64, (3, 4, 90, 70), ops)
    assert route == "fallback" and got_ops is None and box == (0, 0, 64, 64)
    assert np.array_equal(crop, data.clip_resized_crop(ra.augment_pil(_pil(a), ops), 64, (3, 4, 90, 70)))
    # an image with real transparency is a device source under randaug: convert("RGB") comes first
    monkeypatch.undo()
    rgba = np.concatenate([a, image(101, 77, "smooth")[..., :1]], -1)
    from PIL import Image
    route, src, _, _ = resample.prepare(Image.fromarray(rgba, "RGBA"), 64, None, ops)
    assert route == "device" and np.array_equal(src, a)


# ------------------------------------------------------------------------------------------------------------
# the pack
# ------------------------------------------------------------------------------------------------------------
def test_pack_carries_the_augment_plan():
    size = 64
    srcs = [image(w, h, "noise") for (w, h) in [(101, 77), (37, 23), (64, 64), (5, 3)]]
    augs = [((ra.OP_ROTATE, -1), (ra.OP_EQUALIZE, 1)), None, ((ra.OP_COLOR, 1), (ra.OP_SHEAR_X, 1)), ((ra.OP_POSTERIZE, 1), (ra.OP_CONTRAST, 1))]
    p = resample.pack_batch(srcs, size, False, map, augs=augs)
    assert sorted(p) == ["aug", "aug_flags", "plan", "rows", "size", "src", "tab"]
    aug, plan = p["aug"].numpy(), p["plan"].numpy()
    assert aug.shape == (4, ra.AUG_FIELDS) and aug.dtype == np.int64
    for i, s in enumerate(srcs):
        h, w, _ = s.shape
        assert aug[i, :4].tolist() == [plan[i, resample.PLAN_SRC], w, h, 0] and aug[i, 0] % 16 == 0
        for st in range(2):
            rec = aug[i, ra.AUG_STAGE0 + ra.AUG_STAGE_FIELDS * st:ra.AUG_STAGE0 + ra.AUG_STAGE_FIELDS * (st + 1)].tolist()
            if augs[i] is None:
                assert rec == [0] * 10
                continue
            op, sign = augs[i][st]
            coeffs = list(ra.affine_coeffs(op, sign, w, h)) if op in ra.GEOMETRIC else [0] * 6
            assert rec == [op, sign, *coeffs, 0, 0]
    # stage 0: no histogram user, one table (Posterize); stage 1: Equalize and Contrast read histograms and are tables
    assert p["aug_flags"] == (0 << 0) | (1 << 1) | (1 << 2) | (1 << 3)
    # no operations anywhere: the pack is the plain one
    assert sorted(resample.pack_batch(srcs, size, False, map, augs=[None] * 4)) == ["plan", "rows", "size", "src", "tab"]
    assert sorted(resample.pack_batch(srcs, size)) == ["plan", "rows", "size", "src", "tab"]
    boxed = resample.pack_batch(srcs, size, False, map, boxes=[(0, 0, s.shape[1], s.shape[0]) for s in srcs], augs=augs)
    assert "tab" not in boxed and np.array_equal(boxed["aug"].numpy(), aug)


def test_entry_points_are_declared_and_bound():
    protos = abi_header.prototypes()            # bound as declared: tests/test_host_logic.py, for the whole ABI
    assert protos["m3ae_image_randaug_u8"] == ("int", [
        "uint8_t* src", "uint8_t* scratch", "int64_t buf_bytes", "const int64_t* plan", "int64_t B", "void* workspace",
        "int64_t workspace_bytes", "int flags", "void* stream"])
    assert protos["m3ae_image_randaug_workspace_bytes"] == ("int64_t", ["int64_t B"])
    for name in ("m3ae_image_randaug_u8", "m3ae_image_randaug_workspace_bytes"):
        assert f"lib.{name}.argtypes" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = open(os.path.join(ROOT, "mm-vqa-healthcare_amd", "csrc", "randaug.hip")).read()
    assert f"AUG_FIELDS = {ra.AUG_FIELDS}, AUG_STAGE0 = {ra.AUG_STAGE0}, AUG_STAGE_FIELDS = {ra.AUG_STAGE_FIELDS}" in src
    assert f"MAX_W = {resample.MAX_SOURCE_WIDTH}, MAX_H = {ra.MAX_AUG_HEIGHT}" in src
