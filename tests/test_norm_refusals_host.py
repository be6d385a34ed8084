"""The refusals of the nine LayerNorm entry points, the part that needs no GPU: which code each fault gets, and the order of the
checks when a call has two faults -- M3AE_ERR_ARG (a required pointer is null, M <= 0, a bad row map) before
M3AE_ERR_UNSUPPORTED (D % 4, D over the form's limit, an unknown dtype) before M3AE_ERR_ALIGN, all before any HIP call (without a
GPU a launch attempt would come back as a positive hipError_t; with one, nothing is launched on the placeholder pointers).
Every call here carries at least one fault: a complete valid call would launch."""
import pytest

from m3ae_amd import _lib

ARG, UNSUPPORTED, ALIGN = -1, -2, -3
FAKE = 0x1000   # a non-null, 4096-byte aligned "device pointer": the checks compare and mask pointers, they never dereference them
F32, BF16 = _lib.F32, _lib.BF16

PLAIN = ("m3ae_layernorm_bwd", "m3ae_layernorm_bwd_det")
DROP = ("m3ae_layernorm_bwd_drop", "m3ae_layernorm_bwd_drop_det", "m3ae_layernorm_bwd_drop_rows")
MIXED = ("m3ae_layernorm_bwd_mixed", "m3ae_layernorm_bwd_mixed_det")
BWD = PLAIN + DROP + MIXED
ALL = ("m3ae_layernorm_fwd", "m3ae_layernorm_fwd_mixed") + BWD


def code(name, **faults):
    """Return code of entry point `name` for an otherwise valid call (8 rows of 64 fp32 elements, identity row map) with `faults`
    written over its arguments; pointer arguments the entry point does not have are ignored."""
    assert faults, "a complete valid call would launch"
    a = dict(dict.fromkeys(("x", "y", "dy", "gamma", "beta", "mean", "rstd", "dx", "dx_add", "dx_drop", "dx_lo", "dgamma", "dbeta", "ws"), FAKE),
             M=8, D=64, dtype=F32, rows=(0, 1))
    assert set(faults) <= set(a), faults
    a.update(faults)
    fn = getattr(_lib.lib(), name)
    if name == "m3ae_layernorm_fwd":
        return fn(a["x"], a["gamma"], a["beta"], a["y"], a["mean"], a["rstd"], a["M"], a["D"], 1e-5, a["dtype"], 0, 0, None)
    if name == "m3ae_layernorm_fwd_mixed":
        return fn(a["x"], a["gamma"], a["beta"], a["y"], a["mean"], a["rstd"], a["M"], a["D"], 1e-5, None)
    if name in PLAIN:
        return fn(a["dy"], a["x"], a["gamma"], a["beta"], a["mean"], a["rstd"], a["dx"], a["dx_add"], a["dgamma"], a["dbeta"], a["ws"],
                  a["M"], a["D"], a["dtype"], 0, 0, None)
    if name in DROP:
        rows = a["rows"] if name.endswith("_rows") else ()
        return fn(a["dy"], a["x"], a["gamma"], a["beta"], a["mean"], a["rstd"], a["dx"], a["dx_drop"], 0.1, 7, None, a["dgamma"], a["dbeta"],
                  a["ws"], a["M"], a["D"], a["dtype"], *rows, None)
    assert name in MIXED, name
    return fn(a["dy"], a["x"], a["gamma"], a["mean"], a["rstd"], a["dx"], a["dx_add"], a["dx_lo"], a["dgamma"], a["dbeta"], a["ws"],
              a["M"], a["D"], None)


def test_forward_refusals():
    f = "m3ae_layernorm_fwd"
    assert code(f, x=None) == ARG and code(f, M=0) == ARG
    assert code(f, D=6) == UNSUPPORTED and code(f, D=4100) == UNSUPPORTED
    assert code(f, dtype=7) == UNSUPPORTED                       # an unknown dtype, every pointer aligned
    assert code(f, x=FAKE + 4) == ALIGN and code(f, x=FAKE + 8) == ALIGN
    assert code(f, dtype=BF16, x=FAKE + 4) == ALIGN              # (bf16 rows off by 8 are aligned: not a refusal)
    assert code(f, gamma=FAKE + 8) == ALIGN and code(f, dtype=BF16, gamma=FAKE + 8) == ALIGN
    assert code(f, x=None, D=6) == ARG and code(f, D=6, x=FAKE + 4) == UNSUPPORTED
    m = "m3ae_layernorm_fwd_mixed"
    assert code(m, y=None) == ARG
    assert code(m, D=2052) == UNSUPPORTED                        # the mixed forward stops where its backward does
    assert code(m, x=FAKE + 8) == ALIGN and code(m, y=FAKE + 4) == ALIGN


@pytest.mark.parametrize("name", PLAIN)
def test_plain_backward_refusals(name):
    assert code(name, dy=None) == ARG and code(name, ws=None) == ARG
    assert code(name, D=2052) == UNSUPPORTED
    assert code(name, dx=FAKE + 4) == ALIGN and code(name, dtype=BF16, dx=FAKE + 4) == ALIGN
    assert code(name, dx_add=FAKE + 8) == ALIGN and code(name, beta=FAKE + 8) == ALIGN


@pytest.mark.parametrize("name", DROP)
def test_dropout_backward_refusals(name):
    assert code(name, dx_drop=None) == ARG
    assert code(name, D=2052) == UNSUPPORTED
    assert code(name, dx_drop=FAKE + 4) == ALIGN and code(name, dtype=BF16, dx_drop=FAKE + 4) == ALIGN


@pytest.mark.parametrize("name", MIXED)
def test_mixed_backward_refusals(name):
    assert code(name, mean=None) == ARG
    assert code(name, D=2052) == UNSUPPORTED
    for fault in (dict(dy=FAKE + 4), dict(x=FAKE + 8), dict(dx_lo=FAKE + 4), dict(dx_add=FAKE + 8)):
        assert code(name, **fault) == ALIGN, fault


@pytest.mark.parametrize("name", ALL)
def test_argument_errors_come_before_unsupported_before_alignment(name):
    out = "y" if "_fwd" in name else "dx"
    required = "x" if "_fwd" in name else "dy"
    assert code(name, **{required: None, "D": 6}) == ARG
    assert code(name, **{required: None, out: FAKE + 4}) == ARG
    assert code(name, **{"D": 6, out: FAKE + 4}) == UNSUPPORTED
    assert code(name, **{"D": 4100, out: FAKE + 4}) == UNSUPPORTED
    assert code(name, M=0, D=6) == ARG


@pytest.mark.parametrize("rows", [(-1, 1), (0, 0)])
def test_a_bad_row_map_comes_before_both(rows):
    f = "m3ae_layernorm_bwd_drop_rows"
    assert code(f, rows=rows) == ARG
    assert code(f, rows=rows, D=6) == ARG
    assert code(f, rows=rows, dx=FAKE + 4) == ARG
    assert code(f, rows=rows, D=6, dx=FAKE + 4) == ARG
