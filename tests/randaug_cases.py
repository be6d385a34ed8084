"""Shared cases of the RandAugment tests: the (operation, sign) list, seeded noise / smooth images of the small sizes, and the
images whose histograms are degenerate."""
import numpy as np

from m3ae_amd import randaug as ra

# every operation, the geometric ones with both signs
OP_SIGNS = [(op, s) for op in range(1, 15) for s in ((1, -1) if op in ra.GEOMETRIC else (1,))]
HOST_SIZES = [(1, 1), (2, 2), (3, 3), (5, 3), (1, 40), (37, 23), (64, 64), (101, 77)]        # (w, h)
DEVICE_SIZES = [(1, 1), (3, 3), (5, 3), (37, 23), (64, 64), (2051, 9)]


def image(w, h, kind, seed=0):
    """uint8 [h, w, 3]: seeded noise, or a smooth ramp per channel over the full range."""
    if kind == "noise":
        return np.random.RandomState(seed * 7919 + w * 31 + h).randint(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1).astype(np.uint8)


def degenerate_images():
    """name -> uint8 [23, 37, 3]: the histogram cases in which Pillow's table code takes another branch."""
    noise = image(37, 23, "noise", 5)
    const = np.full((23, 37, 3), (10, 128, 250), dtype=np.uint8)                     # every channel has one used bin
    one_bin = noise.copy()
    one_bin[..., 1] = 77                                                                # one channel with one used bin
    # Equalize with step 0: (pixels - last used bin) // 255 == 0 <=> fewer than 255 pixels outside the last used bin
    step0 = np.full((23, 37, 3), 200, dtype=np.uint8)
    step0.reshape(-1, 3)[:100] = noise.reshape(-1, 3)[:100] // 2                        # 100 pixels below 128, 751 at 200
    full = noise.copy()
    full[0, 0], full[0, 1] = 0, 255                                                     # AutoContrast: the band spans 0 - 255 already
    narrow = (noise // 4 + 90).astype(np.uint8)                                         # and one it does stretch
    return {"const": const, "one_bin": one_bin, "step0": step0, "full": full, "narrow": narrow}
