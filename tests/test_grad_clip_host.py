"""Gradient clipping by global norm with the non-finite step guard, the part that needs no GPU: the C ABI additions (header, ctypes
binding and INTEGRATION.md stub agree, ABI number unchanged), the config key and its validator, the piece table of
m3ae_sumsq_segments, the two refusals (before any library call), and the finalize model against torch's clip_grad_norm_."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import abi_header
from m3ae_amd import _lib, config, gradnorm
import gradnorm_model as GM

P = gradnorm.PIECE


def test_header_binding_and_integration_stub_agree_and_the_abi_is_still_4():
    """m3ae_adamw_clip against m3ae_adamw and the shape of the record.  (Binding against header type by type, the values of the
    M3AE_CLIP_* words, the stub, the ABI number and the descriptor sizes: tests/test_host_logic.py, for the whole ABI.)"""
    # m3ae_adamw_clip is m3ae_adamw's argument list plus the record in front of the stream; m3ae_adamw keeps its signature
    a, c = _lib._SIGS["m3ae_adamw"][1], _lib._SIGS["m3ae_adamw_clip"][1]
    assert len(a) == 15 and c == a[:-1] + [C.c_void_p, a[-1]]
    pa, pc = abi_header.prototypes()["m3ae_adamw"][1], abi_header.prototypes()["m3ae_adamw_clip"][1]
    assert pc == pa[:-1] + ["const float* clip_dev", pa[-1]] and pa[-1] == "void* stream"
    # the record is plain 32-bit words named by an enum, not a descriptor struct
    values = {k: v for k, v in abi_header.constants().items() if k.startswith("M3AE_CLIP_")}
    assert values == {"M3AE_CLIP_NORM": _lib.CLIP_NORM, "M3AE_CLIP_COEF": _lib.CLIP_COEF, "M3AE_CLIP_SKIP": _lib.CLIP_SKIP,
                      "M3AE_CLIP_STEPS": _lib.CLIP_STEPS, "M3AE_CLIP_CLIPPED_STEPS": _lib.CLIP_CLIPPED_STEPS,
                      "M3AE_CLIP_SKIPPED_STEPS": _lib.CLIP_SKIPPED_STEPS, "M3AE_CLIP_RECORD_WORDS": _lib.CLIP_RECORD_WORDS}
    assert len(set(values.values())) == len(values) and max(values.values()) == _lib.CLIP_RECORD_WORDS


def test_entry_points_check_their_arguments_before_any_launch():
    """Made-up pointers are never read: the checks come first (no device is touched on this machine)."""
    L = _lib.lib()
    assert L.m3ae_sumsq_workspace_bytes(0) == 8 and L.m3ae_sumsq_workspace_bytes(1178) == 8 * 1178
    assert L.m3ae_sumsq_workspace_bytes(-1) < 0
    x, tab, ptr, out, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    assert L.m3ae_sumsq_segments(None, 8, tab, 1, ptr, 1, out, ws, 8, None) == -1
    assert L.m3ae_sumsq_segments(x, 8, tab, 1, ptr, 0, out, ws, 8, None) == -1          # no segments
    assert L.m3ae_sumsq_segments(x + 4, 8, tab, 1, ptr, 1, out, ws, 8, None) == -3      # x not 16-byte aligned
    assert L.m3ae_sumsq_segments(x, 8, tab, 2, ptr, 1, out, ws, 8, None) == -4          # short workspace
    assert L.m3ae_sumsq_segments(x, 8, tab, 1, ptr, 1, out, None, 8, None) == -4
    assert L.m3ae_clip_finalize(None, 1, 1.0, 1.0, out, None) == -1
    for bad in (0.0, -1.0, float("nan")):
        assert L.m3ae_clip_finalize(x, 1, 1.0, bad, out, None) == -1                    # max_norm in (0, +inf]
    assert L.m3ae_clip_finalize(x, 1, float("inf"), 1.0, out, None) == -1               # grad_scale finite
    assert L.m3ae_adamw_clip(x, x, x, x, None, 8, 1e-3, 0.9, 0.98, 1e-8, 0.0, 1, 1.0, None, None, None) == -1   # no record


def test_config_key_default_and_validator():
    assert config.DEFAULTS["gradient_clip_val"] == 0.0
    base = ["with", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta"]
    assert config.parse_cli(base)["gradient_clip_val"] == 0.0
    assert config.parse_cli(base + ["gradient_clip_val=1.5"])["gradient_clip_val"] == 1.5
    assert config.parse_cli(base + ["gradient_clip_val=1"])["gradient_clip_val"] == 1.0
    assert config.parse_cli(base + ["gradient_clip_val=inf"])["gradient_clip_val"] == float("inf")
    assert config.gradient_clip_val({"gradient_clip_val": float("inf")}) == float("inf")
    assert config.gradient_clip_val({}) == 0.0
    for bad in (-1.0, -0.5, float("nan"), "strong", "1.0", None, True):
        with pytest.raises(ValueError, match="gradient_clip_val"):
            config.gradient_clip_val({"gradient_clip_val": bad})
    with pytest.raises(ValueError, match="gradient_clip_val"):
        config.parse_cli(base + ["gradient_clip_val=-2"])
    with pytest.raises(ValueError, match="gradient_clip_val"):
        config.parse_cli(base + ["gradient_clip_val=nan"])
    with pytest.raises(ValueError, match="gradient_clip_val"):
        config.tiny_config(gradient_clip_val="big")


def test_piece_table_covers_every_element_once():
    segs, n = GM.shape_segments(P)
    assert {b % 4 for b, _ in segs} == {0, 1, 2, 3}
    pieces, ptr = gradnorm.piece_table(segs)
    assert GM.check_piece_table(segs, pieces, ptr, P)
    assert len(pieces) == sum(math.ceil((e - b) / P) for b, e in segs)
    assert (pieces.tolist(), ptr.tolist()) == tuple(map(lambda t: [list(r) if isinstance(r, tuple) else r for r in t], GM.piece_table(segs, P)))
    # element-level: mark every element a piece covers
    hits = np.zeros(n, dtype=np.int32)
    for b, e in pieces:
        hits[b:e] += 1
    want = np.zeros(n, dtype=np.int32)
    for b, e in segs:
        want[b:e] = 1
    assert np.array_equal(hits, want)
    rng = np.random.default_rng(0)
    for trial in range(50):
        piece = int(rng.choice([1, 3, 64, 1000]))
        lens = rng.integers(0, 4 * piece + 2, size=int(rng.integers(1, 40)))
        segs2, pos = [], int(rng.integers(0, 9))
        for ln in lens:
            segs2.append((pos, pos + int(ln)))
            pos += int(ln) + int(rng.integers(0, 6))
        pieces2, ptr2 = gradnorm.piece_table(segs2, piece)
        assert GM.check_piece_table(segs2, pieces2, ptr2, piece)
        hits = np.zeros(pos + 1, dtype=np.int32)
        for b, e in pieces2:
            hits[b:e] += 1
        want = np.zeros(pos + 1, dtype=np.int32)
        for b, e in segs2:
            want[b:e] += 1
        assert np.array_equal(hits, want)
    for bad in ([(4, 2)], [(0, 8), (4, 12)], [(8, 12), (0, 4)]):
        with pytest.raises(ValueError):
            gradnorm.piece_table(bad)


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached: {name}")


def _cpu_store(**over):
    """A ParamStore on the CPU in fp32 (no shadow: its construction makes no library call)."""
    from m3ae_amd.param_store import ParamStore
    torch.manual_seed(0)
    mod = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.LayerNorm(3), torch.nn.Linear(3, 70))
    return ParamStore(mod, config.tiny_config(compute_dtype="fp32", **over), "cpu", torch.float32), mod


def test_store_segment_table_leaves_the_padding_out(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", NoLibrary())
    monkeypatch.setattr(_lib, "lib", lambda: _lib._lib)
    st, mod = _cpu_store()
    segs = st.grad_segments
    names = dict(mod.named_parameters())
    assert sorted(n for _, _, n in segs) == sorted(names)
    for off, numel, name in segs:
        assert st.offset[id(names[name])] == off and names[name].numel() == numel and off % 64 == 0
    assert all(a[0] + a[1] <= b[0] for a, b in zip(segs, segs[1:]))                     # sorted, disjoint
    assert sum(n for _, n, _ in segs) < st.trainable_end                                # the ALIGN padding is in no segment
    assert st._sums is None and st._clip_record is None                                 # nothing uploaded at construction
    assert st.clip_val() == 0.0


def test_update_in_backward_and_graphed_step_refuse_the_key_before_any_library_call(monkeypatch):
    from m3ae_amd.ddp import FlatGradReducer
    from m3ae_amd.graph import GraphedStep
    monkeypatch.setattr(_lib, "_lib", NoLibrary())
    monkeypatch.setattr(_lib, "lib", lambda: _lib._lib)
    for val in (1.0, float("inf")):
        st, _ = _cpu_store(gradient_clip_val=val)
        red = FlatGradReducer(st, update_in_backward=True, world=1)
        with pytest.raises(ValueError, match="gradient_clip_val"):
            red.arm_update(max_steps=10)
        assert st.step_count == 0 and st.exp_avg is None                                # refused before the step began

        class Model:
            store = st
        with pytest.raises(ValueError, match="gradient_clip_val"):
            GraphedStep(Model(), {}, 10)

        class HP:
            config = {"gradient_clip_val": val}

        class Model2:
            hparams = HP()
        with pytest.raises(ValueError, match="gradient_clip_val"):
            GraphedStep(Model2(), {}, 10)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("max_norm", [0.0078125, 1.0, 1e3, float("inf")])     # fp32 values: max_norm is an fp32 argument
def test_finalize_model_matches_torch_clip_grad_norm(max_norm, grad_scale):
    """torch.nn.utils.clip_grad_norm_ on CPU tensors holding the averaged gradient, in float64 so that torch's own norm carries no
    fp32 error: the model's float64 coefficient equals torch's to float64 accuracy, and the fp32 word the kernel writes is within
    one fp32 rounding (2^-24 relative) of it."""
    rng = np.random.default_rng(3)
    shapes = [(7, 5), (130,), (3, 3, 3), (1,)]
    raw = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes]
    for p, g in zip(params, raw):
        p.grad = torch.from_numpy(g.astype(np.float64) * grad_scale)                    # exact: grad_scale is a power of two
    before = [p.grad.clone() for p in params]
    tnorm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    norm, coef, skip, counters = GM.finalize([GM.exact_sumsq(g) for g in raw], grad_scale, max_norm)
    assert skip == 0 and counters[0] == 1
    assert abs(norm - tnorm) <= 1e-13 * norm
    tcoef = min(1.0, max_norm / (tnorm + 1e-6))
    assert abs(coef - tcoef) <= 1e-13 * tcoef
    assert abs(float(np.float32(coef)) - tcoef) <= 2.0 ** -24 * tcoef * (1 + 1e-9)
    if norm + 1e-6 <= max_norm:
        assert np.float32(coef) == np.float32(1.0) and counters[1] == 0
        assert all(torch.equal(p.grad, b) for p, b in zip(params, before))
    else:
        assert counters[1] == 1 and np.float32(coef) < 1.0
        for p, b in zip(params, before):
            assert np.allclose(p.grad.numpy(), b.numpy() * float(np.float32(coef)), rtol=2.0 ** -23, atol=0)


def test_finalize_model_guard_and_counters():
    seq = [([1.0, 3.0], 1.0, 10.0), ([4.0, 12.0], 1.0, 2.0), ([1.0, float("inf")], 1.0, 2.0), ([float("nan")], 1.0, float("inf")),
           ([16.0], 0.125, 1.0)]
    c = (0, 0, 0)
    got = []
    for sums, gs, mx in seq:
        norm, coef, skip, c = GM.finalize(sums, gs, mx, c)
        got.append((norm, coef, skip))
    assert got[0] == (2.0, 1.0, 0)
    assert got[1][0] == 4.0 and got[1][1] == 2.0 / (4.0 + 1e-6) and got[1][2] == 0
    assert got[2][1:] == (0.0, 1) and math.isinf(got[2][0])
    assert got[3][1:] == (0.0, 1) and math.isnan(got[3][0])
    assert got[4] == (0.5, 1.0, 0)
    assert c == (5, 1, 2)
