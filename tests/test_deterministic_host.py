"""Deterministic mode, the part that needs no GPU: the C ABI additions (header, ctypes binding and the INTEGRATION.md stub agree;
ABI number and descriptor layouts unchanged), the config key, the mode switch, and the workspace size query of the ordered
split-K wgrad (which touches no device)."""
import ctypes as C
import os
import sys

import pytest

import abi_header
from m3ae_amd import _lib, config, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_integration_stub_agree_on_the_new_entry_points():
    """Signatures, constant values, the ABI number and the descriptor layouts: tests/test_host_logic.py, for the whole ABI."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_integration_stub as gen
    header = abi_header.constants()
    assert header["M3AE_GEMM_DETERMINISTIC"] == _lib.GEMM_DETERMINISTIC == 4
    assert _lib.GEMM_DETERMINISTIC & (_lib.GEMM_NO_PERSISTENT | _lib.GEMM_F32_X3) == 0
    assert _lib.GEMM_DETERMINISTIC & (0xF << 8 | 0xF << 12 | 0xF << 16 | 0x3 << 20) == 0   # clear of the selector fields
    assert {k: v for k, v in header.items() if k.startswith("M3AE_DET_")} == {
        "M3AE_DET_COLSUM": _lib.DET_COLSUM, "M3AE_DET_EMBED_BWD": _lib.DET_EMBED_BWD, "M3AE_DET_BCE": _lib.DET_BCE,
        "M3AE_DET_XENT": _lib.DET_XENT, "M3AE_DET_MIM": _lib.DET_MIM}
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = text[text.index(gen.BEGIN):text.index(gen.END)]
    assert f"GEMM_DETERMINISTIC = {_lib.GEMM_DETERMINISTIC}" in stub
    # the stub's section of the mode lists every ordered form the header declares (the mixed LayerNorm's sits with its family)
    declared = {n for n in abi_header.prototypes() if n.endswith("_det") or "_det_" in n}
    assert declared == set(gen.DET_ENTRIES) | {"m3ae_layernorm_bwd_mixed_det"} and len(gen.DET_ENTRIES) == 10


def test_config_key_and_mode_switch():
    assert config.DEFAULTS["deterministic"] is False
    assert config.parse_cli(["with", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta"])["deterministic"] is False
    cfg = config.parse_cli(["with", "deterministic=True", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta", "image_size=384"])
    assert cfg["deterministic"] is True
    assert ops.deterministic() is False          # off after import
    with ops.deterministic_mode():
        assert ops.deterministic() is True
        with ops.deterministic_mode(False):
            assert ops.deterministic() is False
        assert ops.deterministic() is True
    assert ops.deterministic() is False
    ops.set_deterministic(True)
    try:
        assert ops.deterministic() is True
        with pytest.raises(ops.DeterministicError, match="some op"):
            ops._no_ordered_form("some op")
    finally:
        ops.set_deterministic(False)
    ops._no_ordered_form("some op")               # mode off: nothing raises


def test_model_config_switches_the_mode_on():
    from m3ae_amd.config import tiny_config
    from m3ae_amd.modules import M3AETransformerSS
    assert ops.deterministic() is False
    M3AETransformerSS(tiny_config())
    assert ops.deterministic() is False
    try:
        M3AETransformerSS(tiny_config(deterministic=True))
        assert ops.deterministic() is True
    finally:
        ops.set_deterministic(False)


def test_layernorm_backward_with_a_row_map_is_refused_in_the_mode_before_the_library(monkeypatch):
    """The LayerNorm backward under a dropout row map (the live-row form) has no ordered entry point: with the mode on,
    ops.ln_bwd_raw raises DeterministicError where it picks the entry point -- before any library call and before any pointer is
    taken (CPU tensors; the library handle is a stub that fails on every attribute)."""
    import torch

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was reached: {name}")

    monkeypatch.setattr(_lib, "_lib", NoLibrary())
    monkeypatch.setattr(_lib, "lib", lambda: _lib._lib)
    ln = torch.nn.LayerNorm(64)
    x, dy = torch.randn(2, 64), torch.randn(2, 64)
    mean, rstd = torch.zeros(2), torch.ones(2)
    with ops.deterministic_mode():
        with pytest.raises(ops.DeterministicError, match="row map"):
            ops.ln_bwd_raw(dy, x, ln, mean, rstd, drop=(0.1, 7), rows=(0, 33))
    assert ln.weight.grad is None and ln.bias.grad is None     # refused before a gradient buffer was made
    with pytest.raises(AssertionError, match="the library was reached"):   # mode off: the call goes on to the library (the stub)
        ops.ln_bwd_raw(dy, x, ln, mean, rstd, drop=(0.1, 7), rows=(0, 33))


def _wgrad_desc(N1, N2, rows, flags=0):
    """dW[N1, N2] += dY[rows, N1]^T X[rows, N2], bf16 operands, fp32 accumulate: mm_wgrad's descriptor (no pointers)."""
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch2 = N1, N2, rows, 1, 1
    d.a_sm, d.a_sk, d.b_sk, d.b_sn, d.c_sm, d.c_sn = 1, N1, N2, 1, N2, 1
    d.dtype_a, d.dtype_b, d.dtype_c = _lib.BF16, _lib.BF16, _lib.F32
    d.alpha, d.accumulate, d.launch_flags = 1.0, 1, flags
    return d


@pytest.mark.parametrize("rows", [36928, 147712])
@pytest.mark.parametrize("N1,N2", [(768, 768), (2304, 768), (3072, 768), (768, 3072)])
@pytest.mark.parametrize("variant", [-1, 0, 2, 5])
def test_gemm_det_workspace_keeps_the_split_k_fan_out(N1, N2, rows, variant):
    """The ordered wgrad keeps its split-K fan-out (a 768 x 768 output is 36 tiles on 256 CUs: one split would idle the chip):
    the workspace holds at least two partial copies of the output for every wgrad of the step."""
    d = _wgrad_desc(N1, N2, rows, ((variant + 1) & 0xF) << 12)
    n = _lib.lib().m3ae_gemm_det_workspace_bytes(C.byref(d))
    assert n >= 2 * N1 * N2 * 4, (n, N1 * N2 * 4)
    assert n % (4 * (N1 * N2 + N1)) == 0        # whole planes: [splits][N1 * N2] accumulators + [splits][N1] row sums


def test_gemm_det_workspace_is_zero_for_descriptors_outside_the_wgrad_family():
    L = _lib.lib()
    d = _wgrad_desc(768, 768, 36928)
    d.a_sm, d.a_sk, d.b_sk, d.b_sn = 36928, 1, 1, 36928      # both operands K-contiguous: the NT family
    assert L.m3ae_gemm_det_workspace_bytes(C.byref(d)) == 0
    d = _wgrad_desc(768, 768, 36928)
    d.dtype_a = d.dtype_b = _lib.F32                          # fp32 operands: the generic kernel (one writer per element)
    assert L.m3ae_gemm_det_workspace_bytes(C.byref(d)) == 0
    d = _wgrad_desc(768, 768, 36928, _lib.GEMM_F32_X3)
    d.dtype_a = d.dtype_b = _lib.F32
    assert L.m3ae_gemm_det_workspace_bytes(C.byref(d)) == 0
    d = _wgrad_desc(770, 768, 36928)                          # not a multiple of the 128 x 128 tile: generic
    assert L.m3ae_gemm_det_workspace_bytes(C.byref(d)) == 0
    assert L.m3ae_gemm_det_workspace_bytes(None) < 0


def test_plain_gemm_rejects_the_deterministic_flag_before_any_launch():
    """m3ae_gemm cannot receive a workspace: with M3AE_GEMM_DETERMINISTIC it returns M3AE_ERR_UNSUPPORTED instead of running the
    atomic kernel (the check precedes every launch, so made-up pointers are never read)."""
    d = _wgrad_desc(768, 768, 36928, _lib.GEMM_DETERMINISTIC)
    d.A, d.B, d.C = 0x10000, 0x20000, 0x30000
    assert _lib.lib().m3ae_gemm(C.byref(d), None) == -2
    d.launch_flags = 0
    assert _lib.lib().m3ae_gemm_det(C.byref(d), None, 0, None) == -1          # the flag is part of the call's contract
    d.launch_flags = _lib.GEMM_DETERMINISTIC
    assert _lib.lib().m3ae_gemm_det(C.byref(d), None, 0, None) == -4          # no workspace
    assert _lib.lib().m3ae_gemm_det(C.byref(d), 0x40000, 16, None) == -4      # short workspace


def test_small_reduction_workspace_sizes():
    L = _lib.lib()
    assert L.m3ae_det_workspace_bytes(_lib.DET_COLSUM, 147712, 768) >= 2 * 768 * 4
    assert L.m3ae_det_workspace_bytes(_lib.DET_EMBED_BWD, 256 * 32, 768) >= 2 * 256 * 32 * 4
    assert L.m3ae_det_workspace_bytes(_lib.DET_XENT, 8192, 50265) >= (1 + 8192) * 4
    assert L.m3ae_det_workspace_bytes(_lib.DET_BCE, 8, 498) > 0 and L.m3ae_det_workspace_bytes(_lib.DET_MIM, 1000, 768) > 0
    assert L.m3ae_det_workspace_bytes(99, 8, 8) < 0 and L.m3ae_det_workspace_bytes(_lib.DET_COLSUM, 0, 8) < 0
