"""RandAugment(2, 9) of the reference's `clip_transform_randaug` (transforms/transform.py:80-91, transforms/randaug.py:164-272),
host half: the draw, the Pillow form the host path runs, a numpy model of every operation (the specification of csrc/randaug.hip),
the augment plan of a pack, and the binding of `m3ae_image_randaug_u8`.

What is restated: `RandAugment(2, 9)` in front of the CLIP transform, on the image converted to RGB, at source resolution: two
operations per image out of the 14 of `augment_list()` (with repetition), each at the value `(9 / 30) * (max - min) + min` of its
range.  The five geometric operations flip the sign of their value when a uniform draw exceeds 0.5.

The draw: a `random.Random` keyed like the crop box (resample.box_rng; the key is prefixed "randaug", so the box keeps its own
stream) gives two `choices` from the 14 and then one `random()` per geometric operation, in the order the operations apply.  The
reference reads Python's global generator in its worker processes; as for the crop box it is the distribution that is restated.

Pillow's arithmetic, piece by piece (each numpy model below equals Pillow byte for byte, tests/test_randaug_host.py):
  * `Image.blend(a, b, alpha)`, 0 <= alpha <= 1: per byte `(uint8)(a + alpha * (b - a))` in float32, multiply and add rounded
    separately, truncated (Color, Contrast, Brightness, Sharpness: `ImageEnhance` blends a degenerate image with the source);
  * `convert("L")`: `(19595 R + 38470 G + 7471 B + 0x8000) >> 16` (Color's degenerate, Contrast's mean);
  * `ImageFilter.SMOOTH` (Sharpness' degenerate): float32 sum starting at 0.5 of the 3 x 3 neighbourhood times (1,1,1,1,5,1,1,1,1)/13,
    clipped and truncated, border pixels copied.  13 * the exact sum is an integer S and the result changes at S = 13 k - 6.5 only,
    0.5 / 13 away from every reachable value: no float32 rounding order can move a byte;
  * nearest-neighbour `transform(AFFINE)`: 16.16 fixed point, `FIX(v) = floor(v * 65536 + 0.5)`, the half-pixel term folded into
    the two offsets, source pixel `(xx >> 16, yy >> 16)`, black outside.  A pure translation takes another path in Pillow
    (a table of source columns from float64 coordinates); for an integer shift both forms give `out[y][x] = in[y + ty][x + tx]`;
  * `rotate`: the matrix as Pillow's Python computes it (`round(cos, 15)`, centre (w / 2, h / 2));
  * autocontrast, equalize, posterize, solarize: 256-entry tables per channel built in Python from the histogram (integers, and
    float64 in autocontrast), applied with `point`.
Seven operations are a table per channel (AutoContrast, Equalize, Posterize, Solarize, SolarizeAdd, Contrast, Brightness), three of
them from the image's histogram; Color and Sharpness blend per pixel; five gather through an affine map.

Device form: `augment_plan` turns the drawn operations into records of AUG_FIELDS int64 per image (geometry, and per stage the
operation, its sign and the six fixed-point coefficients, which are computed HERE in float64 as Pillow's Python does);
`augment_on_device` runs the two stages ping-pong between the uploaded source buffer and a scratch buffer of the same layout.
"""
import ctypes as C
import math

import numpy as np

from .resample import box_rng

N_OPS, MAGNITUDE = 2, 9            # RandAugment(2, 9): the only setting offered
(OP_IDENTITY, OP_AUTOCONTRAST, OP_EQUALIZE, OP_ROTATE, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD, OP_COLOR, OP_CONTRAST,
 OP_BRIGHTNESS, OP_SHARPNESS, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y) = range(15)
# augment_list() of the reference, in its order: (code, min, max)
AUGMENT_LIST = ((OP_AUTOCONTRAST, 0, 1), (OP_EQUALIZE, 0, 1), (OP_ROTATE, 0, 30), (OP_POSTERIZE, 0, 4), (OP_SOLARIZE, 0, 256),
                (OP_SOLARIZE_ADD, 0, 110), (OP_COLOR, 0.1, 1.9), (OP_CONTRAST, 0.1, 1.9), (OP_BRIGHTNESS, 0.1, 1.9),
                (OP_SHARPNESS, 0.1, 1.9), (OP_SHEAR_X, 0.0, 0.3), (OP_SHEAR_Y, 0.0, 0.3), (OP_TRANSLATE_X, 0.0, 100),
                (OP_TRANSLATE_Y, 0.0, 100))
OP_NAMES = ("Identity", "AutoContrast", "Equalize", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast",
            "Brightness", "Sharpness", "ShearX", "ShearY", "TranslateXabs", "TranslateYabs")
VALUE = {op: (float(MAGNITUDE) / 30) * float(hi - lo) + lo for op, lo, hi in AUGMENT_LIST}   # RandAugment.__call__'s expression
GEOMETRIC = (OP_ROTATE, OP_SHEAR_X, OP_SHEAR_Y, OP_TRANSLATE_X, OP_TRANSLATE_Y)
HIST_OPS = (OP_AUTOCONTRAST, OP_EQUALIZE, OP_CONTRAST)                       # their table is built from the image's histogram
POINT_OPS = (OP_AUTOCONTRAST, OP_EQUALIZE, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD, OP_CONTRAST, OP_BRIGHTNESS)

# the plan record of one image; must match csrc/randaug.hip
AUG_FIELDS = 24
AUG_OFF, AUG_W, AUG_H, AUG_STAGE0, AUG_STAGE_FIELDS = 0, 1, 2, 4, 10   # stage s at 4 + 10 s: op, sign, a0 .. a5, two spare
# Device eligibility under randaug, on top of resample's caps: Pillow's fixed-point affine path holds while every source
# coordinate stays below 32768 (Geometry.c check_fixed; beyond it a float64 path with other roundings takes over).  With
# w <= 8192 and h <= MAX_AUG_HEIGHT the largest coordinate of the five maps is below 8192 + 16384.
MAX_AUG_HEIGHT = 16384


# ------------------------------------------------------------------------------------------------------------
# the draw
# ------------------------------------------------------------------------------------------------------------
def aug_rng(*key):
    """The generator of an image's operations: resample.box_rng's rule on the key prefixed "randaug"."""
    return box_rng("randaug", *key)


def draw(rng):
    """((op, sign), (op, sign)): two `choices` from the 14, then one `random()` per geometric operation in applying order
    (sign -1 when the draw exceeds 0.5; +1 for every other operation)."""
    picked = rng.choices(AUGMENT_LIST, k=N_OPS)
    return tuple((op, (-1 if rng.random() > 0.5 else 1) if op in GEOMETRIC else 1) for op, _, _ in picked)


# ------------------------------------------------------------------------------------------------------------
# the Pillow form (host path, and what every model is pinned to)
# ------------------------------------------------------------------------------------------------------------
def apply_pil(img, op, sign=1):
    """One operation of transforms/randaug.py on an RGB PIL image at the (2, 9) value, the sign given instead of drawn."""
    from PIL import Image, ImageEnhance, ImageOps
    if op == OP_IDENTITY:
        return img
    v = VALUE[op] * (sign if op in GEOMETRIC else 1)
    if op == OP_AUTOCONTRAST:
        return ImageOps.autocontrast(img)
    if op == OP_EQUALIZE:
        return ImageOps.equalize(img)
    if op == OP_ROTATE:
        return img.rotate(v)
    if op == OP_POSTERIZE:
        return ImageOps.posterize(img, max(1, int(v)))
    if op == OP_SOLARIZE:
        return ImageOps.solarize(img, v)
    if op == OP_SOLARIZE_ADD:   # randaug.py:86-92 (np.int there is the platform integer)
        a = np.clip(np.array(img).astype(np.int64) + v, 0, 255).astype(np.uint8)
        return ImageOps.solarize(Image.fromarray(a), 128)
    if op in (OP_COLOR, OP_CONTRAST, OP_BRIGHTNESS, OP_SHARPNESS):
        cls = {OP_COLOR: ImageEnhance.Color, OP_CONTRAST: ImageEnhance.Contrast, OP_BRIGHTNESS: ImageEnhance.Brightness,
               OP_SHARPNESS: ImageEnhance.Sharpness}[op]
        return cls(img).enhance(v)
    matrix = {OP_SHEAR_X: (1, v, 0, 0, 1, 0), OP_SHEAR_Y: (1, 0, 0, v, 1, 0), OP_TRANSLATE_X: (1, 0, v, 0, 1, 0),
              OP_TRANSLATE_Y: (1, 0, 0, 0, 1, v)}[op]
    return img.transform(img.size, Image.AFFINE, matrix)


def augment_pil(img, ops):
    """`RandAugment(2, 9)` with the drawn `ops` on a PIL image: convert("RGB") first (transform.py:90), then the operations."""
    img = img.convert("RGB")
    for op, sign in ops:
        img = apply_pil(img, op, sign)
    return img


# ------------------------------------------------------------------------------------------------------------
# the numpy model: the specification of the kernels
# ------------------------------------------------------------------------------------------------------------
def luminance(rgb):
    """convert("L") of uint8 [..., 3] -> uint8 [...]."""
    a = rgb.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def histograms(rgb):
    """int64 [4, 256]: the histograms of R, G, B and of L = convert("L")."""
    planes = [rgb[..., 0], rgb[..., 1], rgb[..., 2], luminance(rgb)]
    return np.stack([np.bincount(p.reshape(-1), minlength=256) for p in planes]).astype(np.int64)


def _blend_lut(base, alpha):
    """uint8 [256]: blend(constant `base`, i, alpha) per byte value i, float32 as Image.blend."""
    i = np.arange(256, dtype=np.int64)
    prod = np.float32(alpha) * (i - base).astype(np.float32)
    return (np.float32(base) + prod).astype(np.int64).astype(np.uint8)   # 0 <= value < 256: truncation


def point_lut(op, hist=None):
    """uint8 [3, 256]: the table per channel of a point operation; `hist` ([4, 256], `histograms`) for the three that read it."""
    ident = np.arange(256, dtype=np.int64)
    if op in (OP_AUTOCONTRAST, OP_EQUALIZE):
        out = []
        for c in range(3):
            h = [int(v) for v in hist[c]]
            used = [i for i in range(256) if h[i]]
            lut = ident
            if op == OP_AUTOCONTRAST and used and used[-1] > used[0]:   # ImageOps.autocontrast: float64, truncated, clipped
                lo, hi = used[0], used[-1]
                scale = 255.0 / (hi - lo)
                offset = -lo * scale
                lut = np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)], dtype=np.int64)
            if op == OP_EQUALIZE and len(used) > 1:                      # ImageOps.equalize: integers; point() clips to a byte
                step = (sum(h) - h[used[-1]]) // 255
                if step:
                    n, vals = step // 2, []
                    for i in range(256):
                        vals.append(min(n // step, 255))
                        n += h[i]
                    lut = np.array(vals, dtype=np.int64)
            out.append(lut)
        return np.stack(out).astype(np.uint8)
    if op == OP_POSTERIZE:
        lut = ident & ~(2 ** (8 - max(1, int(VALUE[op]))) - 1)
    elif op == OP_SOLARIZE:
        lut = np.where(ident < VALUE[op], ident, 255 - ident)
    elif op == OP_SOLARIZE_ADD:
        j = np.clip(ident + VALUE[op], 0, 255).astype(np.uint8).astype(np.int64)   # float64 sum, truncated (randaug.py:87-90)
        lut = np.where(j < 128, j, 255 - j)
    elif op == OP_BRIGHTNESS:
        lut = _blend_lut(0, VALUE[op])
    elif op == OP_CONTRAST:                                               # ImageStat mean of L (float64), rounded half up
        count = int(hist[3].sum())
        total = 0.0
        for j in range(256):
            total += j * int(hist[3][j])
        lut = _blend_lut(int(total / count + 0.5), VALUE[op])
    else:
        raise ValueError(f"operation {op} is not a table")
    return np.broadcast_to(np.asarray(lut, dtype=np.int64).astype(np.uint8), (3, 256)).copy()


def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def affine_coeffs(op, sign, w, h):
    """(a0 .. a5) of Geometry.c's affine_fixed for a geometric operation on a w x h image: source pixel of output (x, y) =
    ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16).  The float64 matrix is the one the reference hands to Pillow."""
    v = VALUE[op] * sign
    if op == OP_ROTATE:                                   # Image.rotate
        angle = -math.radians(v % 360.0)
        m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
        cx, cy = w / 2, h / 2
        m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
        m[2] += cx
        m[5] += cy
    else:
        m = [float(t) for t in {OP_SHEAR_X: (1, v, 0, 0, 1, 0), OP_SHEAR_Y: (1, 0, 0, v, 1, 0), OP_TRANSLATE_X: (1, 0, v, 0, 1, 0),
                                OP_TRANSLATE_Y: (1, 0, 0, 0, 1, v)}[op]]
    return (_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def _blend(degenerate, rgb, alpha):
    a, b = degenerate.astype(np.int64), rgb.astype(np.int64)
    prod = np.float32(alpha) * (b - a).astype(np.float32)
    return (a.astype(np.float32) + prod).astype(np.int64).astype(np.uint8)


def smooth(rgb):
    """ImageFilter.SMOOTH of uint8 [h, w, 3]."""
    h, w, _ = rgb.shape
    out = rgb.copy()
    if h < 3 or w < 3:
        return out
    a = rgb.astype(np.float32)
    k1, k5 = np.float32(1) / np.float32(13), np.float32(5) / np.float32(13)
    acc = np.full((h - 2, w - 2, 3), 0.5, dtype=np.float32)
    for dy in (1, 0, -1):
        for dx in (-1, 0, 1):
            acc = acc + a[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] * (k5 if dx == 0 and dy == 0 else k1)
    out[1:-1, 1:-1] = np.clip(acc, 0, 255).astype(np.int64).astype(np.uint8)
    return out


def apply_model(rgb, op, sign=1):
    """One operation on uint8 [h, w, 3] -> uint8 [h, w, 3]: what one stage of the device form computes."""
    if op == OP_IDENTITY:
        return rgb.copy()
    if op in POINT_OPS:
        lut = point_lut(op, histograms(rgb) if op in HIST_OPS else None)
        return np.stack([lut[c][rgb[..., c]] for c in range(3)], -1)
    if op == OP_COLOR:
        return _blend(np.repeat(luminance(rgb)[..., None], 3, -1), rgb, VALUE[op])
    if op == OP_SHARPNESS:
        return _blend(smooth(rgb), rgb, VALUE[op])
    h, w, _ = rgb.shape
    a0, a1, a2, a3, a4, a5 = affine_coeffs(op, sign, w, h)
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    xin, yin = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
    assert max(abs(a2) + h * abs(a1) + w * abs(a0), abs(a5) + h * abs(a4) + w * abs(a3)) < 1 << 31   # Pillow's ints are 32 bits
    inside = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = rgb[np.clip(yin, 0, h - 1), np.clip(xin, 0, w - 1)]
    out[~inside] = 0
    return out


def augment_model(rgb, ops):
    for op, sign in ops:
        rgb = apply_model(rgb, op, sign)
    return rgb


# ------------------------------------------------------------------------------------------------------------
# the plan and the device call
# ------------------------------------------------------------------------------------------------------------
def eligible(w, h):
    """Whether the device form takes a w x h source (next to resample's own caps)."""
    return h <= MAX_AUG_HEIGHT


def augment_plan(shapes, offsets, augs):
    """int64 [B, AUG_FIELDS] for sources of `shapes` (h, w, 3) at byte `offsets` of the pack; augs[i]: the drawn operations of
    image i, or None (a source the host already augmented): the identity record, which the kernels pass over."""
    plan = np.zeros((len(shapes), AUG_FIELDS), dtype=np.int64)
    for i, ((h, w, _), off, ops) in enumerate(zip(shapes, offsets, augs)):
        plan[i, :3] = (off, w, h)
        for s, (op, sign) in enumerate(ops or ()):
            at = AUG_STAGE0 + AUG_STAGE_FIELDS * s
            plan[i, at:at + 2] = (op, sign)
            if op in GEOMETRIC:
                plan[i, at + 2:at + 8] = affine_coeffs(op, sign, w, h)
    return plan


def stage_flags(plan):
    """Bit s: stage s has an operation that reads a histogram; bit 2 + s: stage s has an operation that is a table."""
    flags = 0
    for s in range(N_OPS):
        ops = plan[:, AUG_STAGE0 + AUG_STAGE_FIELDS * s]
        live = (plan[:, AUG_STAGE0] != OP_IDENTITY) | (plan[:, AUG_STAGE0 + AUG_STAGE_FIELDS] != OP_IDENTITY)
        flags |= int(np.isin(ops[live], HIST_OPS).any()) << s
        flags |= int(np.isin(ops[live], POINT_OPS).any()) << (2 + s)
    return flags


def workspace_bytes(B):
    from . import _lib
    return int(_lib.lib().m3ae_image_randaug_workspace_bytes(B))


def augment_on_device(src, aug, flags, stream=None, scratch=None):
    """`m3ae_image_randaug_u8`: the two stages of every record of `aug` (device int64 [B, AUG_FIELDS]) on `src` (device bytes of
    the pack), in place as far as the caller sees: stage 0 writes `scratch`, stage 1 writes `src` again.  Returns the workspace
    (uint32 histograms [2][B][4][256], then the uint8 tables [B][3][256] of the last stage that built any), for the tests."""
    import torch
    from . import _lib
    B = aug.shape[0]
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        if scratch is None:
            scratch = torch.empty_like(src)
        ws = torch.empty(workspace_bytes(B), dtype=torch.uint8, device=src.device)
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    vp = C.c_void_p
    _lib.check(_lib.lib().m3ae_image_randaug_u8(vp(src.data_ptr()), vp(scratch.data_ptr()), src.numel(), vp(aug.data_ptr()), B,
                                                vp(ws.data_ptr()), ws.numel(), int(flags), s), "m3ae_image_randaug_u8")
    return ws
