"""Host side (no GPU) of tests/test_gpu_attn_accuracy.py: the criteria that file holds the bf16 attention kernels to have teeth.
The rounding model and an independently written second model (online softmax over 32-key tiles, unnormalised bf16 P) pass every
criterion at the shapes of the GPU tests, through the same code; nine subtly wrong kernels (attn_accuracy.MUTANTS) each miss at
least one criterion at every shape where they apply."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_accuracy as aa  # noqa: E402

B, H = 2, 2
PROBE_SEED = aa.PROBE_SEED


def candidate(fn, **extra):
    return lambda case: fn(**aa.model_args(case), **extra)


MODELS = {"rounding": candidate(aa.rounding_model), "online": candidate(aa.online_model)}


_CASES = {}


def host_case(Lq, Lk, seed, drop=False, role="budget", **kw):
    """One case per (arguments, role), shared by the tests of this file: its reference and rounding model are computed once
    (attn_accuracy._yardsticks) and left unchanged.  role: which probe overwrites the case's v / dO."""
    key = (Lq, Lk, seed, drop, role, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = _new_case(Lq, Lk, seed, drop, **kw)
    return _CASES[key]


def _new_case(Lq, Lk, seed, drop, **kw):
    case = aa.make_case(B, H, Lq, Lk, seed, p=aa.DROP_P if drop else 0.0, **kw)
    if drop:
        case["keep"] = aa.host_keep_mask(B, H, Lq, Lk, aa.DROP_P, seed + 11)
    return case


# ------------------------------------------------------------------------------------------------------------------------
# the models pass
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", aa.A_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_models_are_within_the_budget(shape):
    for masked in (False, True):
        for drop in (False, True):
            case = host_case(*shape, seed=300, drop=drop, masked=masked)
            for name, cand in MODELS.items():
                assert not aa.check_budget(cand, case, f"{name} {shape} mask {masked} drop {drop}"), (name, shape, masked, drop)


@pytest.mark.parametrize("regime", ["unit", "t5"])
def test_models_are_within_the_budget_with_bias_and_causal(regime):
    for label, Lq, Lk, drop, kw in aa.c_cases():
        case = host_case(Lq, Lk, seed=400, drop=drop, **(aa.t5_regime(kw) if regime == "t5" else kw))
        for name, cand in MODELS.items():
            assert not aa.check_budget(cand, case, f"{name} {regime} {label}"), (name, regime, label)


@pytest.mark.parametrize("variant", aa.B_VARIANTS)
@pytest.mark.parametrize("shape", aa.B_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_models_pass_the_probes(shape, variant):
    kw = dict(masked=variant == "masked", probe_mask=True, drop=variant == "dropout")
    vcase, docase = host_case(*shape, seed=PROBE_SEED, role="v", **kw), host_case(*shape, seed=PROBE_SEED, role="do", **kw)
    rowcases = {row: host_case(*shape, seed=PROBE_SEED, role=row, **kw) for row in aa.single_rows(shape[0])}
    for name, cand in MODELS.items():
        label = f"{name} {shape} {variant}"
        assert not aa.check_v_probe_case(cand, vcase, label)[0], label
        assert not aa.check_do_probe_case(cand, docase, label)[0], label
        for row, case in rowcases.items():
            assert not aa.check_single_row_case(cand, case, row, label)[0], (label, row)


# ------------------------------------------------------------------------------------------------------------------------
# the mutants do not
# ------------------------------------------------------------------------------------------------------------------------
def rejected_by_budget(mutant, Lq, Lk, drop=False, seed=300, **kw):
    case = host_case(Lq, Lk, seed=seed, drop=drop, **kw)
    return bool(aa.check_budget(candidate(aa.rounding_model, mutant=mutant), case, f"mutant {mutant} {Lq}x{Lk}"))


@pytest.mark.parametrize("mutant", ["pv_last_key", "dv_last_query", "ds_last_query", "truncate", "o_scale", "no_rescale", "norm_tail"])
def test_mutant_misses_the_budget_at_every_shape(mutant):
    for Lq, Lk in aa.A_SHAPES:
        drop = mutant == "no_rescale"
        if aa.mutant_applies(mutant, Lq, Lk, drop, False, False):
            assert rejected_by_budget(mutant, Lq, Lk, drop, masked=False), (mutant, Lq, Lk)


@pytest.mark.parametrize("mutant", ["causal_off_by_one", "dpb_transposed", "ds_last_query", "truncate"])
def test_mutant_misses_the_budget_with_bias_and_causal(mutant):
    seen = 0
    for label, Lq, Lk, drop, kw in aa.c_cases():
        if aa.mutant_applies(mutant, Lq, Lk, drop, kw.get("bias", False), kw.get("causal", False)):
            assert rejected_by_budget(mutant, Lq, Lk, drop, seed=400, **kw), (mutant, label)
            seen += 1
    assert seen


@pytest.mark.parametrize("shape", aa.B_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tail_mutants_are_caught_by_the_probes_alone(shape):
    """The element-wise probes see a dropped last key, a dropped last query row and a zeroed last dS row on their own, at every
    probe shape: an rms over random data only sees them as long as the sequence is short."""
    Lq, Lk = shape
    kw = dict(seed=PROBE_SEED, masked=False, probe_mask=True, drop=False)
    mutant = lambda m: candidate(aa.rounding_model, mutant=m)
    if Lk > 1:
        bad, _ = aa.check_v_probe_case(mutant("pv_last_key"), host_case(Lq, Lk, role="v", **kw), f"mutant pv_last_key {shape}")
        assert "V probe error" in bad
    bad, _ = aa.check_do_probe_case(mutant("dv_last_query"), host_case(Lq, Lk, role="do", **kw), f"mutant dv_last_query {shape}")
    assert "dO probe error" in bad
    bad, _ = aa.check_single_row_case(mutant("ds_last_query"), host_case(Lq, Lk, role=Lq - 1, **kw), Lq - 1, f"mutant ds_last_query {shape}")
    assert bad
    if Lk > 32:
        bad, _ = aa.check_v_probe_case(mutant("norm_tail"), host_case(Lq, Lk, role="v", **kw), f"mutant norm_tail {shape}")
        assert "V probe error" in bad


def test_budget_rejects_nan_and_a_scaled_tensor_and_the_edge_sets():
    x = torch.randn(1000, dtype=torch.float64)
    model = aa.bf16_nearest(x.float())
    assert aa.within_budget(model, model, x)[0]
    assert not aa.within_budget(torch.full_like(model, float("nan")), model, x)[0]
    assert not aa.within_budget(model * 1.01, model, x)[0]
    assert aa.edge_set(577) == [0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 95, 96, 127, 128, 129, 288, 543, 544, 545, 574, 575, 576]
    assert aa.edge_set(1) == [0] and aa.edge_set(33) == [0, 1, 16, 30, 31, 32]
