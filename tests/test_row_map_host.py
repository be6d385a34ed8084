"""Dropout row map, the part that needs no GPU: the additive `*_rows` entry points are their plain entry points plus the map, in the
header and in the binding (tests/test_host_logic.py holds binding, header and stub together for the whole ABI); and a bad map
(row_step < 1, negative row_base, a mapped index past 2^63 - 1) is rejected with M3AE_ERR_ARG before any HIP call (without a GPU a launch attempt would come back as
a positive hipError_t instead; with one, nothing is launched on the placeholder pointers)."""
import ctypes as C

import abi_header
from m3ae_amd import _lib

ROWS_ENTRIES = ("m3ae_gemm_rows", "m3ae_attn_fwd_rows", "m3ae_attn_bwd_rows", "m3ae_layernorm_bwd_drop_rows", "m3ae_dropout_rows")
ERR_ARG = _lib.ERR_ARG
FAKE = 0x1000   # a non-null "device pointer": the argument checks compare pointers with NULL and never dereference them


def test_header_binding_and_stub_agree_on_the_rows_entry_points():
    """A `_rows` entry point is its plain entry point plus `int64_t row_base, int64_t row_step` right before `void* stream`, in the
    header and in the binding.  (Binding against header type by type, and the stub: tests/test_host_logic.py, for the whole ABI.)"""
    protos = abi_header.prototypes()
    for name in ROWS_ENTRIES:
        base = name[:-len("_rows")]
        (res, args), (bres, bargs) = protos[name], _lib._SIGS[name]
        assert res == "int" and args[-3:] == ["int64_t row_base", "int64_t row_step", "void* stream"], (name, args)
        assert (res, args[:-3] + args[-1:]) == protos[base], name
        assert _lib._SIGS[base] == (bres, bargs[:-3] + bargs[-1:]), name


def _gemm_desc(M=8, N=64, K=64, p=0.5):
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch2 = M, N, K, 1, 1
    d.A, d.a_sm, d.a_sk = FAKE, K, 1
    d.B, d.b_sk, d.b_sn = FAKE, 1, K
    d.C, d.c_sm, d.c_sn = FAKE, N, 1
    d.dtype_a = d.dtype_b = d.dtype_c = _lib.BF16
    d.alpha, d.dropout_p, d.dropout_seed = 1.0, p, 7
    return d


def _attn_desc(B=2, H=12, Lq=1, Lk=33):
    d = _lib.AttnDesc()
    d.B, d.H, d.Lq, d.Lk, d.Dh = B, H, Lq, Lk, 64
    for f in ("q", "k", "v", "o", "d_o", "dq", "dk", "dv", "lse", "delta"):
        setattr(d, f, FAKE)
    d.dtype, d.dropout_p, d.lse_stride = _lib.BF16, 0.1, 32
    return d


# (row_base, row_step) that must be refused for a call of `rows` mask rows and `ld` mask columns
def _bad_maps(rows, ld):
    too_far = (2 ** 63 - 1) // ld          # base alone puts the first row's last index past 2^63 - 1
    big_step = (2 ** 63 - 1) // (ld * max(rows - 1, 1)) + 1
    return [(0, 0), (0, -1), (-1, 1), (too_far, 1)] + ([(0, big_step)] if rows > 1 else [])


def test_bad_row_maps_are_rejected_before_any_launch():
    lib = _lib.lib()
    for base, step in _bad_maps(8, 64):
        assert lib.m3ae_gemm_rows(C.byref(_gemm_desc()), base, step, None) == ERR_ARG, (base, step)
        assert lib.m3ae_dropout_rows(FAKE, FAKE, None, 8, 64, 0.5, 1, None, _lib.BF16, base, step, None) == ERR_ARG, (base, step)
        assert lib.m3ae_layernorm_bwd_drop_rows(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0.1, 1, None, None, None, FAKE, 8, 64,
                                                _lib.BF16, base, step, None) == ERR_ARG, (base, step)
    d = _attn_desc()
    for base, step in _bad_maps(d.B * d.H * d.Lq, 36):   # ld(33) = 36
        assert lib.m3ae_attn_fwd_rows(C.byref(d), base, step, None) == ERR_ARG, (base, step)
        assert lib.m3ae_attn_bwd_rows(C.byref(d), base, step, None) == ERR_ARG, (base, step)
