"""Device image transform, host half: the plan and the coefficient tables of Pillow's 8-bit bicubic resample with the
centre crop folded in, a numpy model of the two passes (the specification of csrc/image.hip), the packing of a batch's
sources into one upload, and the binding of `m3ae_image_resample_u8`.

What is restated: `clip_resize_crop` (m3ae_amd/data.py; transforms/transform.py:60-64 of the reference) =
`img.convert("RGBA").resize((nw, nh), BICUBIC).crop(centre).convert("RGB")`.  Pillow's resize of an 8-bit image is
fixed-point integer arithmetic (libImaging/Resample.c): per axis `precompute_coeffs` builds float64 weights,
`normalize_coeffs_8bpc` rounds them to 22 fractional bits, and each pass computes
`clip8((2**21 + sum_x pixel[xmin + x] * k[x]) >> 22)` per channel -- horizontal pass first, into a uint8 image, then the
vertical pass.  An axis whose size does not change is skipped.  For an opaque image the premultiply / un-premultiply
Pillow wraps around an RGBA resize is the identity, so the RGB bytes can be resized alone.  The same integer arithmetic
on the GPU gives the same bytes; the float64 weights are built HERE, in Pillow's operation order (a device build could
contract a multiply-add and move a weight by one unit), and uploaded as data.

Folding the crop: only the `size` output columns / rows that survive `CenterCrop` get a table row, and `row0` / `nrows`
name the source rows those output rows read -- the horizontal pass runs on them alone.

Train transform "clip_resizedcrop" (transforms/transform.py:70-77): `RandomResizedCrop(size, scale=(0.9, 1.0), BICUBIC)` =
`img.crop(box).resize((size, size), BICUBIC)` with a box drawn per image and epoch (`random_resized_crop_box`).  To the kernels
a box is a plan record: the source offset of its corner, w = cw, h = ch and the full image's pitch.  Every image then has
tables of its own (two axes of Python loops per image, under the GIL), so a pack made with `boxes` carries no tables:
`m3ae_image_resample_tables` (csrc/image.hip) builds them on the GPU from the plan in front of the two passes, `axis_table`'s
float64 operations one by one with contraction off -- bit-equal tables, tests/test_gpu_resized_crop.py.
"""
import ctypes as C
import hashlib
import math
import random
import threading

import numpy as np

PRECISION_BITS = 22                # 32 - 8 - 2 (Resample.c)
PLAN_FIELDS = 16                   # int64 per image, see PLAN_* below; must match csrc/image.hip
(PLAN_SRC, PLAN_W, PLAN_H, PLAN_PITCH, PLAN_ROW0, PLAN_NROWS, PLAN_KSX, PLAN_KSY, PLAN_XB, PLAN_XK, PLAN_YB, PLAN_YK,
 PLAN_IROW0, PLAN_BUILD) = range(14)   # PLAN_BUILD: 1 = m3ae_image_resample_tables writes this record's tables
# Eligibility caps of the device path.  The horizontal pass stages whole source rows in LDS (one dword per pixel, 32 KiB),
# so a row may hold at most MAX_SOURCE_WIDTH pixels; MAX_SOURCE_PIXELS bounds one image's share of the pinned staging
# buffer (48 MiB of RGB).  Larger sources take the host path.
MAX_SOURCE_WIDTH = 8192
MAX_SOURCE_PIXELS = 1 << 24


def output_geometry(w, h, size):
    """(nw, nh, left, top) of `clip_resize_crop`: torchvision Resize(int) (shorter side -> size, the longer one truncated)
    and CenterCrop's rounding."""
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nw, nh = int(size * w / h), size
    return nw, nh, int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    lo = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    hi = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, lo, np.where(x < 2.0, hi, 0.0))


def axis_table(in_size, out_size, first, count):
    """Bounds int32 [count, 2] (xmin, taps) and coefficients int32 [count, ksize] of the outputs first .. first + count - 1
    of a resample in_size -> out_size (precompute_coeffs + normalize_coeffs_8bpc, float64, Pillow's operation order).
    in_size == out_size: Pillow skips the pass; the identity table (one tap of 2**22) gives the same bytes."""
    assert 0 <= first and first + count <= out_size
    if in_size == out_size:
        bounds = np.stack([np.arange(first, first + count), np.ones(count, dtype=np.int64)], 1).astype(np.int32)
        return bounds, np.full((count, 1), 1 << PRECISION_BITS, dtype=np.int32)
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((count, 2), dtype=np.int32)
    coeffs = np.zeros((count, ksize), dtype=np.int32)
    for i in range(count):
        center = (first + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = _bicubic((np.arange(xmax, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = 0.0
        for v in w.tolist():     # ascending x, one rounding per addition (np.sum adds pairwise)
            ww += v
        if ww != 0.0:
            w = w / ww
        k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)  # trunc
        assert np.abs(k).max() < 1 << 23, "a coefficient beyond 24 bits: the kernel multiplies with __mul24"
        bounds[i] = (xmin, xmax)
        coeffs[i, :xmax] = k
    return bounds, coeffs


def axis_ksize(in_size, out_size):
    """Row length of `axis_table`'s coefficients (Pillow's ksize; 1 for the identity table)."""
    if in_size == out_size:
        return 1
    return int(np.ceil(2.0 * max(in_size / out_size, 1.0))) * 2 + 1


# ------------------------------------------------------------------------------------------------------------
# the crop box of RandomResizedCrop
# ------------------------------------------------------------------------------------------------------------
def box_rng(*key):
    """`random.Random` seeded from an integer digest of `key` (ints, strings, tuples of them): the same key draws the same box in
    any process, and no global or torch generator state is read or advanced."""
    return random.Random(int.from_bytes(hashlib.blake2b(repr(key).encode(), digest_size=8).digest(), "little"))


def random_resized_crop_box(w, h, rng, scale=(0.9, 1.0), ratio=(3 / 4, 4 / 3)):
    """(left, top, cw, ch): torchvision's `RandomResizedCrop.get_params` restated on a `random.Random`.  Ten tries of an area
    uniform in scale * w * h and an aspect ratio log-uniform in `ratio`; the first box that fits gets a uniform position.
    If none fits: the central box of the nearest allowed ratio (the whole image when its ratio is allowed).  The reference's
    own draws depend on its worker processes, so it is the distribution that is restated, not a stream."""
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = w * h * rng.uniform(scale[0], scale[1])
        aspect = math.exp(rng.uniform(log_lo, log_hi))
        cw, ch = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
        if 0 < cw <= w and 0 < ch <= h:
            top = rng.randint(0, h - ch)
            left = rng.randint(0, w - cw)
            return left, top, cw, ch
    if w / h < min(ratio):
        cw, ch = w, int(round(w / min(ratio)))
    elif w / h > max(ratio):
        cw, ch = int(round(h * max(ratio))), h
    else:
        cw, ch = w, h
    return (w - cw) // 2, (h - ch) // 2, cw, ch


class Tables:
    """The four tables of one (w, h, size) and the source rows the vertical pass reads."""

    def __init__(self, w, h, size):
        nw, nh, left, top = output_geometry(w, h, size)
        assert nw >= size and nh >= size
        self.w, self.h, self.size, self.nw, self.nh, self.left, self.top = w, h, size, nw, nh, left, top
        self.xb, self.xk = axis_table(w, nw, left, size)
        self.yb, self.yk = axis_table(h, nh, top, size)
        self.ksx, self.ksy = self.xk.shape[1], self.yk.shape[1]
        self.row0 = int(self.yb[:, 0].min())
        self.nrows = int((self.yb[:, 0] + self.yb[:, 1]).max()) - self.row0
        assert (self.xb[:, 0] >= 0).all() and (self.xb[:, 0] + self.xb[:, 1] <= w).all() and (self.xb[:, 1] <= self.ksx).all()
        assert self.row0 >= 0 and self.row0 + self.nrows <= h and (self.yb[:, 1] <= self.ksy).all()
        self.flat = np.concatenate([self.xb.ravel(), self.xk.ravel(), self.yb.ravel(), self.yk.ravel()])
        o = np.cumsum([0, self.xb.size, self.xk.size, self.yb.size])
        self.offsets = tuple(int(v) for v in o)   # of xb, xk, yb, yk inside `flat`


_cache, _cache_lock = {}, threading.Lock()


def tables(w, h, size):
    """Cached per (w, h, size): data sets have few distinct source sizes."""
    key = (int(w), int(h), int(size))
    with _cache_lock:
        t = _cache.get(key)
    if t is None:
        t = Tables(*key)
        with _cache_lock:
            if len(_cache) > 4096:
                _cache.clear()
            _cache[key] = t
    return t


def _pass(src, bounds, coeffs):
    """One pass along axis 1 of src uint8 [n, len, ch] -> uint8 [n, outputs, ch]: int32 sums, arithmetic shift, clamp."""
    out = np.empty((src.shape[0], bounds.shape[0], src.shape[2]), dtype=np.uint8)
    for i, (xmin, cnt) in enumerate(bounds.tolist()):
        acc = np.full((src.shape[0], src.shape[2]), 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for x in range(cnt):
            acc += src[:, xmin + x, :].astype(np.int32) * coeffs[i, x]
        out[:, i, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resample_model(rgb, size, t=None):
    """uint8 [h, w, 3] -> uint8 [size, size, 3]: the slow numpy statement of what the two kernels compute, from the same
    tables.  Equals `clip_resize_crop` of the opaque image bit for bit."""
    h, w, _ = rgb.shape
    t = t or tables(w, h, size)
    inter = _pass(rgb[t.row0:t.row0 + t.nrows], t.xb, t.xk)                    # [nrows, size, 3]
    yb = t.yb.copy()
    yb[:, 0] -= t.row0
    return np.ascontiguousarray(_pass(inter.transpose(1, 0, 2), yb, t.yk).transpose(1, 0, 2))


# ------------------------------------------------------------------------------------------------------------
# eligibility
# ------------------------------------------------------------------------------------------------------------
def prepare(img, size, box=None, aug=None):
    """PIL image -> ("device", uint8 [h, w, 3] RGB source) if the image is opaque and within the caps, else
    ("fallback", uint8 [size, size, 3]): the finished `clip_resize_crop` of the host path, which the device path then
    carries through identity tables.
    With `box` (left, top, cw, ch; train transform "clip_resizedcrop") the answer has a third element, the box the device
    transform applies to the array: `box` itself next to the whole source, (0, 0, size, size) next to the finished
    `clip_resized_crop` of the fallback route.
    With `aug` (the drawn operations of randaug.draw; config key `randaug`) the answer is always (route, array, box or None,
    operations or None).  The chain starts with convert("RGB") (transform.py:90), so alpha is gone before the resize and every
    image within the caps is a device source, handed over with its operations; beyond them the host augments (randaug.augment_pil)
    and transforms, and the operations are None."""
    from .data import clip_resize_crop, clip_resized_crop
    if aug is not None:
        from . import randaug
        img = img.convert("RGB")
        w, h = img.size
        if w <= MAX_SOURCE_WIDTH and w * h <= MAX_SOURCE_PIXELS and randaug.eligible(w, h):
            return "device", np.asarray(img, dtype=np.uint8), box, aug
        img = randaug.augment_pil(img, aug)
        if box is not None:
            return "fallback", clip_resized_crop(img, size, box), (0, 0, size, size), None
        return "fallback", clip_resize_crop(img, size), None, None

    def with_box(route, a, b):
        return (route, a) if box is None else (route, a, b)

    w, h = img.size
    if w <= MAX_SOURCE_WIDTH and w * h <= MAX_SOURCE_PIXELS:
        if img.mode == "RGB" and "transparency" not in img.info:
            return with_box("device", np.asarray(img, dtype=np.uint8), box)   # convert("RGBA") would set alpha to 255
        rgba = img.convert("RGBA")                                    # base_dataset.py:92-93, as the host path
        if rgba.getextrema()[3] == (255, 255):
            return with_box("device", np.asarray(rgba.convert("RGB"), dtype=np.uint8), box)
        img = rgba
    if box is not None:
        return "fallback", clip_resized_crop(img, size, box), (0, 0, size, size)
    return "fallback", clip_resize_crop(img, size)


# ------------------------------------------------------------------------------------------------------------
# batch packing (host) and the device call
# ------------------------------------------------------------------------------------------------------------
def _align16(n):
    return (n + 15) & ~15


def pack_batch(sources, size, pin=False, pmap=map, boxes=None, augs=None):
    """uint8 [h_i, w_i, 3] sources -> the three host tensors the kernels read: `src` (bytes, every image at a 16-byte
    aligned offset, rows packed), `plan` (int64 [B, PLAN_FIELDS]) and `tab` (int32; one set of tables per distinct source
    size), plus `rows`, the number of intermediate rows of the batch (the workspace size).  `pmap`: a `map` that may run the copies into the staging buffer
    on several threads (numpy releases the GIL for them); a batch of 1024 x 1024 sources is 805 MB.
    `boxes` (one (left, top, cw, ch) per source; "clip_resizedcrop"): image i is `sources[i][top:top + ch, left:left + cw]`
    resized to size x size.  The plan names the box inside the whole source, images with equal (cw, ch) share a table set and
    PLAN_BUILD marks its first owner; the tables themselves are built on the device, so the pack has `tab_ints` (their length)
    in place of `tab`.
    `augs` (per source the drawn operations of randaug.draw, or None for a source the host augmented already; config key
    `randaug`): the pack also carries `aug`, the augment plan (randaug.augment_plan: int64 [B, AUG_FIELDS]), and `aug_flags`
    (randaug.stage_flags) -- unless no source has an operation."""
    import torch
    offs, total = [], 0
    for s in sources:
        assert s.dtype == np.uint8 and s.ndim == 3 and s.shape[2] == 3
        offs.append(total)
        total += _align16(s.size)
    plan = np.zeros((len(sources), PLAN_FIELDS), dtype=np.int64)
    tabs, tab_at, tab_len, rows = [], {}, 0, 0
    for i, s in enumerate(sources):
        h, w, _ = s.shape
        if boxes is not None:
            left, top, cw, ch = (int(v) for v in boxes[i])
            assert 0 <= left and 0 <= top and 0 < cw and 0 < ch and left + cw <= w and top + ch <= h, (boxes[i], (w, h))
            ksx, ksy = axis_ksize(cw, size), axis_ksize(ch, size)
            if (cw, ch) not in tab_at:
                tab_at[(cw, ch)] = tab_len
                tab_len += size * (2 + ksx) + size * (2 + ksy)
                plan[i, PLAN_BUILD] = 1
            xb = tab_at[(cw, ch)]
            xk, yb = xb + 2 * size, xb + size * (2 + ksx)
            yk = yb + 2 * size
            plan[i, :13] = (offs[i] + top * w * 3 + 3 * left, cw, ch, w * 3, 0, ch, ksx, ksy, xb, xk, yb, yk, rows)
            rows += ch
            assert plan[i, PLAN_SRC] + (ch - 1) * w * 3 + 3 * cw <= total and yk + size * ksy <= tab_len
            continue
        t = tables(w, h, size)
        if (w, h) not in tab_at:
            tab_at[(w, h)] = tab_len
            tabs.append(t.flat)
            tab_len += t.flat.size
        base = tab_at[(w, h)]
        plan[i, :13] = (offs[i], w, h, w * 3, t.row0, t.nrows, t.ksx, t.ksy, *(base + o for o in t.offsets), rows)
        rows += t.nrows
        assert offs[i] + h * w * 3 <= total and base + t.flat.size <= tab_len
    use_pin = pin and torch.cuda.is_available()
    src = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=use_pin)
    flat = src.numpy()
    def put(so):
        flat[so[1]:so[1] + so[0].size] = so[0].reshape(-1)
    list(pmap(put, zip(sources, offs)))
    plan_t = torch.from_numpy(plan)
    extra = {}
    if augs is not None and any(augs):
        from . import randaug
        aug = randaug.augment_plan([s.shape for s in sources], offs, augs)
        aug_t = torch.from_numpy(aug)
        extra = {"aug": aug_t.pin_memory() if use_pin else aug_t, "aug_flags": randaug.stage_flags(aug)}
    if boxes is not None:
        return {"src": src, "plan": plan_t.pin_memory() if use_pin else plan_t, "tab_ints": tab_len, "rows": rows, "size": int(size),
                **extra}
    tab_t = torch.from_numpy(np.concatenate(tabs).astype(np.int32))
    if use_pin:
        plan_t, tab_t = plan_t.pin_memory(), tab_t.pin_memory()
    return {"src": src, "plan": plan_t, "tab": tab_t, "rows": rows, "size": int(size), **extra}


def upload(pack, device):
    """The pack's tensors on `device` (non-blocking: call it under the copy stream)."""
    return {**pack, **{k: pack[k].to(device, non_blocking=True) for k in ("src", "plan", "tab", "aug") if k in pack}}


def workspace_bytes(rows, size):
    from . import _lib
    return int(_lib.lib().m3ae_image_resample_workspace_bytes(rows, size))


def build_tables_on_device(plan, size, tab, stream=None):
    """`m3ae_image_resample_tables`: fills int32 `tab` (device) with the tables of every plan record marked PLAN_BUILD."""
    import torch
    from . import _lib
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    _lib.check(_lib.lib().m3ae_image_resample_tables(C.c_void_p(plan.data_ptr()), plan.shape[0], size, C.c_void_p(tab.data_ptr()),
                                                     tab.numel(), s), "m3ae_image_resample_tables")
    return tab


def resample_on_device(dpack, want_u8=False, stream=None):
    """Device pack -> fp32 [B, 3, size, size] (ToTensor + Normalize of the resized crop; bit-equal to
    `normalize_on_device(clip_resize_crop(...))`), and with want_u8 also the uint8 [B, size, size, 3] crop.
    A pack made with boxes has no tables: they are built here, on the same stream, in front of the two passes (a record
    the table kernel refuses keeps zero tap counts).
    A pack with an augment plan (`aug`; config key `randaug`): the two RandAugment stages run first, on the same stream, and leave
    the augmented sources where they were (randaug.augment_on_device)."""
    import torch
    from . import _lib
    from .synth import CLIP_MEAN, CLIP_STD
    src, plan, size = dpack["src"], dpack["plan"], dpack["size"]
    if "aug" in dpack:
        from . import randaug
        randaug.augment_on_device(src, dpack["aug"], dpack["aug_flags"], stream)
    tab = dpack.get("tab")
    if tab is None:
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            tab = torch.zeros(max(dpack["tab_ints"], 1), dtype=torch.int32, device=src.device)
        build_tables_on_device(plan, size, tab, stream)
    B = plan.shape[0]
    out = torch.empty((B, 3, size, size), dtype=torch.float32, device=src.device)
    u8 = torch.empty((B, size, size, 3), dtype=torch.uint8, device=src.device) if want_u8 else None
    nbytes = workspace_bytes(dpack["rows"], size)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    mean, std = (C.c_float * 3)(*CLIP_MEAN), (C.c_float * 3)(*CLIP_STD)
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    vp = C.c_void_p
    _lib.check(_lib.lib().m3ae_image_resample_u8(vp(src.data_ptr()), src.numel(), vp(plan.data_ptr()), vp(tab.data_ptr()),
                                                 tab.numel(), B, size, vp(ws.data_ptr()), nbytes, vp(out.data_ptr()),
                                                 vp(u8.data_ptr()) if want_u8 else None, mean, std, s),
               "m3ae_image_resample_u8")
    return (out, u8) if want_u8 else out
