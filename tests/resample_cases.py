"""Shared cases of the device image transform tests: source sizes (w, h) and seeded noise / smooth images."""
import numpy as np

# the sizes the transform was checked on when it was specified, then an upscale on both axes and a source >= 4000 px on a side
SIZES = [(512, 512), (700, 500), (500, 700), (300, 200), (1024, 777), (384, 384), (383, 911), (97, 1300), (2048, 2500),
         (385, 384), (150, 120), (4100, 300)]
TARGETS = (384, 224)


def source(w, h, kind, seed=0, channels=3):
    """uint8 [h, w, channels] (channels 1 -> [h, w])."""
    rng = np.random.RandomState(seed * 7919 + w * 31 + h)
    if kind == "noise":
        a = rng.randint(0, 256, (h, w, channels), dtype=np.uint8)
    else:   # smooth: low-frequency waves per channel, full range
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        a = np.stack([127.5 + 127.5 * np.sin(x / (17.0 + 5 * c) + c) * np.cos(y / (23.0 - 3 * c) + rng.rand())
                      for c in range(channels)], -1).round().astype(np.uint8)
    return a[..., 0] if channels == 1 else a


def kind_of(i):
    return "noise" if i % 2 == 0 else "smooth"
