"""Attention summaries and heatmaps, the part that needs no GPU: the numpy models the GPU tests compare against
(tests/heatmap_model.py) are themselves held to ATen on the CPU and to the reference's attention maps, and the argument checks of
the heatmap entry points are shown to run before any library call."""
import numpy as np
import pytest
import torch

import heatmap_model as hm
from m3ae_amd import _lib
from m3ae_amd.config import tiny_config
from m3ae_amd.modules import M3AETransformerSS
from oracle_util import load_golden, tiny_batch

U = hm.U


# ATen forms the same weights as the model when the ratio S / g is an integer (its scale is then the same fp32 number and its
# source coordinates round the same way): what is left is ATen's own fp32 combination of the four taps, 4 U max|in| by the
# argument of tests/test_gpu_attn_summary.py, twice that allowed (seen: 1.3 - 1.9 U max|in| on these ratios, up to 2.8 on other
# inputs).  Other ratios (24 -> 100, 24 -> 385) differ by 16 - 22 U, because ATen computes the scale differently: they are held to
# the model only (GPU test).
@pytest.mark.parametrize("g,S", [(1, 8), (4, 64), (14, 224), (24, 384), (36, 576)])
def test_upsample_model_against_aten_on_integer_ratios(g, S):
    rng = np.random.default_rng(g * 1000 + S)
    x = rng.random((3, g, g), dtype=np.float32)
    want = torch.nn.functional.interpolate(torch.from_numpy(x)[:, None], size=(S, S), mode="bilinear", align_corners=False)[:, 0]
    got = hm.upsample(x, S)
    assert got.shape == (3, S, S)
    err = np.abs(got - want.double().numpy()).max()
    assert err <= 8 * U * np.abs(x).max(), err / (U * np.abs(x).max())


def test_upsample_model_edges():
    """A constant grid stays constant within the rounding of l0 = 1 - l1; g = 1 copies its one value; S = g is the identity."""
    c = np.full((1, 5, 5), 0.37, dtype=np.float32)
    assert np.abs(hm.upsample(c, 17) - np.float64(np.float32(0.37))).max() <= 2 * U
    one = np.array([[[2.5]]], dtype=np.float32)
    assert (hm.upsample(one, 8) == 2.5).all()
    x = np.random.default_rng(0).random((2, 6, 6), dtype=np.float32)
    assert (hm.upsample(x, 6) == x.astype(np.float64)).all()


def test_recv_of_the_reference_maps_is_a_distribution_over_the_keys():
    """Every row of a map sums to 1, so the mean of the rows does: each of the tiny fixtures' fp32 rows (17 or 32 keys) is within
    Lk 2^-24 of 1 after its softmax division, and the float64 mean adds nothing visible: 17 * 32 * 2^-24 covers both.  A key the
    map never attends to (the padding keys' exact zeros) receives exactly 0."""
    g = load_golden("attn_maps.npz")
    names = [n for n in g.files if n.startswith("tiny_")]
    assert len(names) == 8
    for n in names:
        p = g[n]
        r = hm.recv(p)
        assert r.shape == (p.shape[0], p.shape[3])
        assert np.abs(r.sum(-1) - 1).max() <= 17 * 32 * U, n
        dead = (p == 0).all(axis=(1, 2))
        assert (r[dead] == 0).all() and (r[~dead] > 0).all(), n
    assert any((g[n] == 0).all(axis=(1, 2)).any() for n in names)   # (the text keys of the fixtures do carry padding)


class _NoLibrary:
    """Stands in for the loaded library: any entry point reached is a failure of the test."""
    def __getattr__(self, name):
        raise AssertionError(f"library entry point {name} was reached")


def _host_model():
    return M3AETransformerSS(tiny_config(compute_dtype="fp32"))


def test_heatmap_arguments_are_checked_before_any_library_call(monkeypatch):
    m = _host_model()
    monkeypatch.setattr(_lib, "_lib", _NoLibrary())
    b = tiny_batch()
    with pytest.raises(ValueError, match="which"):
        m.attention_heatmaps(b, which="image2text")
    with pytest.raises(ValueError, match="which"):
        m.attention_heatmaps(b, which=None)
    # 64 x 48 pixels at patch 16: 4 x 3 = 12 patches, I - 1 is not a square
    odd = dict(b, image=[b["image"][0][:, :, :, :48]])
    with pytest.raises(ValueError, match="square"):
        m.attention_heatmaps(odd)
    with pytest.raises(ValueError, match="square"):
        m.attention_heatmaps(odd, which="text2image", size=100)
    # (and the spy is live: a well-formed call does reach for the library, or for the store that holds its weights)
    with pytest.raises((AssertionError, RuntimeError)):
        m.attention_heatmaps(b)
