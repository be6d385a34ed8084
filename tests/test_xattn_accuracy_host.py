"""Host side (no GPU) of tests/test_gpu_xattn_accuracy.py: the criteria that file holds the fused cross-attention kernels to have
teeth.  The rounding models of both directions, and their exact-accumulation variants (the same bf16 roundings around float64 sums:
a correct kernel with another accumulation order), pass every criterion at every shape and input regime of the GPU tests, through
the same code; the `peaked` regime is as sharp as it claims and the split-K shapes give a ragged last split; twelve subtly wrong
kernels (xattn_accuracy.MUTANTS, each a one-line deviation of the model) miss at least one criterion in every configuration where
they apply."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import xattn_accuracy as xa  # noqa: E402

SHAPES = xa.A_SHAPES + xa.SPLITK_SHAPES
_CASES = {}


def ids(s):
    return "dir{}-B{}-T{}-I{}".format(*s)


def configs(regime):
    """(masked, drop) of a regime: with and without key mask, with and without dropout; the masked regime always has its mask."""
    return [(m, d) for m in ((True,) if regime == "masked" else (False, True)) for d in (False, True)]


def host_case(shape, regime, masked, drop, **kw):
    """One case per configuration, shared by the tests of this file: its reference and rounding model are computed once
    (xattn_accuracy.yardsticks) and left unchanged."""
    key = (shape, regime, masked, drop, tuple(sorted(kw.items())))
    if key not in _CASES:
        case = xa.make_case(*shape, regime=regime, masked=masked, p=xa.DROP_P if drop else 0.0, seed=1000 + 7 * shape[3] + shape[0], **kw)
        if drop:
            case["keep_a"], case["keep_h"] = xa.host_keep_masks(case, seed=11)
        _CASES[key] = case
    return _CASES[key]


@pytest.mark.parametrize("regime", xa.REGIMES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_model_is_within_its_own_criteria(shape, regime):
    for masked, drop in configs(regime):
        case = host_case(shape, regime, masked, drop)
        ref, model = xa.yardsticks(case)
        label = f"model {ids(shape)} {regime} mask {int(masked)} drop {int(drop)}"
        assert not xa.criteria(model, case, label), label
        assert all(bool(torch.isfinite(model[n]).all()) for n in xa.TENSORS), label
        if not drop:   # the same roundings around exact sums: a correct kernel with another accumulation order
            assert not xa.criteria(xa.rounding_model(case, acc=torch.float64), case, "exact-accumulation " + label), label
        assert not bool(ref["g_bk"].abs().max() > 1e-9 * ref["g_bv"].abs().max()), "d(b_k) of the reference is zero"
        if regime == "peaked":
            frac = xa.peaked_fraction(ref)
            print(f"[xattn-accuracy] {label}: row maximum of P above 0.9 on {frac:.2f} of the rows")
            assert frac >= 0.25, (label, frac)


@pytest.mark.parametrize("cls", [c for c in xa.D_CLASSES if c[1] <= 1536], ids=lambda c: "dir{}-D{}-H{}-T{}-I{}".format(*c))
def test_model_is_within_its_own_criteria_over_the_envelope(cls):
    """(The classes wider than 1536 are left to the GPU run: minutes of float64 on the host.)"""
    direction, D, H, T, I = cls
    for masked, drop in ((False, False), (True, False), (True, True)):
        case = host_case((direction, 2, T, I), "unit", masked, drop, D=D, H=H)
        assert not xa.criteria(xa.yardsticks(case)[1], case, f"model {cls} mask {int(masked)} drop {int(drop)}")


def test_split_k_shapes_give_a_ragged_last_split():
    """(17, 32): two splits, 9 + 8 chunks; (9, 64): two splits (18 chunks: 9 + 9, no two-way split of the even chunk count 2 B is
    ragged); (13, 64): three splits, 9 + 9 + 8."""
    for _, B, T, _ in xa.SPLITK_SHAPES:
        ksplit, kchunks, last = xa.pick_split(B, T, 12, 768)
        assert ksplit == (3 if B == 13 else 2) and 0 < last <= kchunks, (B, T, ksplit, kchunks, last)
        assert last < kchunks or (B, T) == (9, 64), (B, T, ksplit, kchunks, last)
    assert xa.pick_split(2, 32, 12, 768)[0] == 1 and xa.pick_split(128, 32, 12, 768)[0] >= 10


@pytest.mark.parametrize("mutant", xa.MUTANTS)
def test_mutant_is_rejected_wherever_it_applies(mutant):
    seen = 0
    for shape in SHAPES:
        for regime in xa.REGIMES:
            for masked, drop in configs(regime):
                case = host_case(shape, regime, masked, drop)
                if not xa.mutant_applies(mutant, case):
                    continue
                label = f"mutant {mutant} {ids(shape)} {regime} mask {int(masked)} drop {int(drop)}"
                assert xa.criteria(xa.rounding_model(case, mutant=mutant), case, label), f"tolerated: {label}"
                seen += 1
    assert seen


def test_per_entry_form_of_the_probability_bound_would_reject_a_correct_kernel():
    """Why check_probs takes the model's error per softmax row: with |P - P_ref| <= 3 |P_model - P_ref| + 2^-8 P_ref entry by entry,
    the exact-accumulation variant of the model itself is over the bound (about 2 x at these shapes) where the model's own roundings
    happen to cancel; the row form passes it (test_model_is_within_its_own_criteria)."""
    for shape in ((0, 2, 32, 159), (1, 2, 32, 128)):
        case = host_case(shape, "masked", True, False)
        ref, model = xa.yardsticks(case)
        r, m, g = ref["P0"], model["P0"].double(), xa.rounding_model(case, acc=torch.float64)["P0"].double()
        bound = xa.MAX_FACTOR * (m - r).abs() + xa.EPS * r
        assert bool(((g - r).abs() > bound).any())


def test_budget_rejects_nan():
    case = host_case((0, 2, 32, 33), "unit", False, False)
    got = dict(xa.yardsticks(case)[1])
    got["dx"] = torch.full_like(got["dx"], float("nan"))
    assert "dx" in xa.check_budget(got, case, "nan")
