"""CPU: the yardsticks of tests/gemm_accuracy.py checked on themselves, at the shapes and epilogue classes of
tests/test_gpu_gemm_accuracy.py (row counts reduced to M <= 600, the ragged tails kept).

  * the fp32 torch model of a correct kernel (a.float() @ w.float().t(), fp32 epilogue, one rne_bf16 per store) meets the exact
    tier bit for bit, the element-wise bound with zero violations, the signed-error budget and the rms budget;
  * every mutant of that model is rejected by at least one criterion wherever it applies (gemm_accuracy.mutant_applies);
  * the exact tier has power: at least 10 % of the bf16 outputs of every case need rounding, at least 5 % are exact ties from
    K = 256 on; and exact_operands refuses operands whose sums could reach 2^24."""
import pytest
import torch

import gemm_accuracy as ga


def host_shape(shape):
    M, N, K = shape
    return (M if M <= ga.HOST_MAX_M else 256 + M % 256, N if N <= 600 else 256 + N % 256, K)


NT_SHAPES = sorted({host_shape(s) for s, _ in ga.NT_EXACT_CASES} | set(ga.GENERIC_EXACT_SHAPES))
TN_SHAPES = [s for s, _ in ga.TN_EXACT_CASES]
BOUND_SHAPES = [s for s, _ in ga.BOUND_CASES]
TN_BOUND_SHAPES = [s for s, _ in ga.TN_BOUND_CASES]
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def seed_of(shape):
    return 1000 + shape[0] + 7 * shape[1] + 13 * shape[2]


def exact_case(shape):
    def make():
        M, N, K = shape
        return ga.exact_operands(M, N, K, seed_of(shape)), ga.host_keep(M, N, 0.5, seed_of(shape) + 1)
    return cached(("exact", shape), make)


def exact_ref(shape, name, c_bf16):
    def make():
        ops, keep = exact_case(shape)
        cast = (lambda t: t.to(torch.bfloat16)) if c_bf16 else (lambda t: t.float())
        kw = ga.exact_epilogue(name, ops, keep, cast)
        return kw, ga.reference(ops["a"], ops["b"], **kw)
    return cached(("exact_ref", shape, name, c_bf16), make)


def exact_mismatch(shape, name, c_bf16, mutant=None):
    ops, _ = exact_case(shape)
    kw, ref = exact_ref(shape, name, c_bf16)
    c, pre = ga.model(ops["a"], ops["b"], c_bf16, mutant=mutant, **kw)
    bad = not torch.equal(c.double(), ga.expected_store(ref.c, c_bf16))
    if ref.preact is not None:
        bad = bad or not torch.equal(pre.double(), ga.expected_store(ref.preact, c_bf16))
    return bad


@pytest.mark.parametrize("shape", NT_SHAPES, ids=str)
def test_model_meets_the_exact_tier_bit_for_bit(shape):
    for name in ga.EXACT_EPILOGUES:
        for c_bf16 in (True, False):
            assert not exact_mismatch(shape, name, c_bf16), (shape, name, c_bf16)


@pytest.mark.parametrize("shape", NT_SHAPES, ids=str)
def test_exact_tier_has_rounding_and_ties(shape):
    """Over the bf16 stores of a case (C and, where the epilogue has one, preact).  The single-row shape has 8 outputs per store:
    the shares are taken over its five epilogues together."""
    M, N, K = shape
    small = []
    for name in ga.EXACT_EPILOGUES:
        _, ref = exact_ref(shape, name, True)
        vals = torch.cat([ref.c.reshape(-1)] + ([ref.preact.reshape(-1)] if ref.preact is not None else []))
        if vals.numel() < 1000:
            small.append(vals)
            continue
        inexact, ties = ga.rounding_shares(vals)
        assert inexact >= 0.10, (shape, name, inexact)
        assert K < 256 or ties >= 0.05, (shape, name, ties)
    if small:
        inexact, ties = ga.rounding_shares(torch.cat(small))
        assert inexact >= 0.10, (shape, inexact)
        assert K < 256 or ties >= 0.05, (shape, ties)


def rejected_everywhere(mutant, shape, cases, applies, misses):
    """At a shape of 10^4 outputs and more a mutant must be rejected in EVERY case (epilogue, store dtype) it applies to; at a
    smaller one (a handful of outputs per case) in at least one.  Returns the number of cases it applied to."""
    applied, rejected = 0, 0
    for name, c_bf16 in cases:
        if applies(name, c_bf16):
            applied += 1
            hit = bool(misses(name, c_bf16))
            rejected += hit
            assert hit or shape[0] * shape[1] < ga.MIN_AGGREGATE, (mutant, shape, name, c_bf16)
    assert rejected or not applied, (mutant, shape)
    return applied


@pytest.mark.parametrize("mutant", [m for m in ga.MUTANTS if m not in ("round_preact_before_act", "tanh_gelu")])
def test_mutant_misses_the_exact_tier_at_every_shape(mutant):
    cases = [(name, c_bf16) for name in ga.EXACT_EPILOGUES for c_bf16 in (True, False)]
    for shape in NT_SHAPES:
        applied = rejected_everywhere(mutant, shape, cases,
                                      lambda n, bf: ga.mutant_applies(mutant, *shape, bf, exact_ref(shape, n, bf)[0], exact=True),
                                      lambda n, bf: exact_mismatch(shape, n, bf, mutant))
        assert applied or (mutant == "residual_from_last_row" and (shape[0] - 1) % 8 == 0) or \
            (mutant == "alpha_after_bias" and exact_case(shape)[0]["alpha"] == 1.0), (mutant, shape)


def test_exact_operands_refuses_sums_that_could_reach_2_pow_24():
    with pytest.raises(AssertionError):
        ga.exact_operands(4, 8, 65536, 1)            # 65536 x 64 x 2 x 2 x 8 = 2^27
    with pytest.raises(AssertionError):
        ga.exact_operands(4, 8, 8192, 1, alpha=0.5, ab_max=16)
    ga.exact_operands(4, 8, 4133, 1)


def tn_kw(ops, accumulate, alpha):
    return dict(alpha=alpha, **({"c_old": ops["c_old"].float()} if accumulate else {}))


@pytest.mark.parametrize("shape", TN_SHAPES, ids=str)
def test_model_and_mutants_on_the_wgrad_exact_tier(shape):
    M, N, K = shape
    ops = ga.exact_operands(M, N, K, seed_of(shape))
    for accumulate in (True, False):
        for alpha in (0.5, 1.0):
            kw = tn_kw(ops, accumulate, alpha)
            ref = ga.reference(ops["a"], ops["b"], **kw)
            assert torch.equal(ga.model(ops["a"], ops["b"], False, **kw)[0].double(), ref.c)
            for mutant in ("scale_1p2m8", "drop_last_k", "accumulate_ignored"):
                if ga.mutant_applies(mutant, M, N, K, False, kw, exact=True):
                    assert not torch.equal(ga.model(ops["a"], ops["b"], False, mutant=mutant, **kw)[0].double(), ref.c), (mutant, shape)


# ------------------------------------------------------------------------------------------------------------------------
# bound tier
# ------------------------------------------------------------------------------------------------------------------------
def bound_case(shape):
    def make():
        M, N, K = shape
        return ga.bound_operands(M, N, K, seed_of(shape)), ga.host_keep(M, N, ga.DROP_P, seed_of(shape) + 1)
    return cached(("bound", shape), make)


def bound_ref(shape, name, c_bf16):
    def make():
        ops, keep = bound_case(shape)
        cast = (lambda t: t.to(torch.bfloat16)) if c_bf16 else (lambda t: t.float())
        kw = ga.bound_class(name, ops, keep, cast)
        return kw, ga.reference(ops["a"], ops["b"], **kw)
    return cached(("bound_ref", shape, name, c_bf16), make)


def bound_misses(shape, name, c_bf16, mutant=None):
    ops, _ = bound_case(shape)
    kw, ref = bound_ref(shape, name, c_bf16)
    c, pre = ga.model(ops["a"], ops["b"], c_bf16, mutant=mutant, **kw)
    return ga.criteria(c, pre, ref, c_bf16)


@pytest.mark.parametrize("shape", BOUND_SHAPES, ids=str)
def test_model_is_inside_every_bound_tier_criterion(shape):
    for name in ga.BOUND_CLASSES:
        for c_bf16 in (True, False):
            assert bound_misses(shape, name, c_bf16) == [], (shape, name, c_bf16)


@pytest.mark.parametrize("mutant", [m for m in ga.MUTANTS if m != "half_up"])
def test_mutant_misses_the_bound_tier_at_every_shape(mutant):
    cases = [(name, c_bf16) for name in ga.BOUND_CLASSES for c_bf16 in (True, False)]
    for shape in BOUND_SHAPES:
        applied = rejected_everywhere(mutant, shape, cases,
                                      lambda n, bf: ga.mutant_applies(mutant, *shape, bf, bound_ref(shape, n, bf)[0], exact=False),
                                      lambda n, bf: bound_misses(shape, n, bf, mutant))
        assert applied or (mutant == "tanh_gelu" and shape[2] > 256) or (mutant == "residual_from_last_row" and (shape[0] - 1) % 8 == 0), \
            (mutant, shape)


@pytest.mark.parametrize("shape", TN_BOUND_SHAPES, ids=str)
def test_model_and_mutants_on_the_wgrad_bound(shape):
    M, N, K = shape
    ops = ga.bound_operands(M, N, K, seed_of(shape))
    for accumulate in (True, False):
        kw = tn_kw(ops, accumulate, 0.5)
        ref = ga.reference(ops["a"], ops["b"], **kw)
        assert ga.criteria(ga.model(ops["a"], ops["b"], False, **kw)[0], None, ref, False, tn=True) == []
        for mutant in ("scale_1p2m8", "drop_last_k", "accumulate_ignored"):
            if ga.mutant_applies(mutant, M, N, K, False, kw, exact=False):
                assert ga.criteria(ga.model(ops["a"], ops["b"], False, mutant=mutant, **kw)[0], None, ref, False, tn=True), (mutant, shape)


def test_yardsticks_on_known_values():
    x = torch.tensor([0.0, 1.0, 1.5, 255.0, 256.0, 257.0, 258.0, -259.0, 3.0e-3], dtype=torch.float64)
    assert torch.equal(ga.hulp(x), torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 0.5, 1.0, 1.0, 1.0, 1.0, 2.0 ** -17], dtype=torch.float64))
    assert ga.rounding_shares(torch.tensor([256.0, 257.0, 258.0, 259.0, 513.0, 514.0], dtype=torch.float64)) == (4 / 6, 3 / 6)
    ref = torch.linspace(1.0, 3.0, 20000, dtype=torch.float64).reshape(100, 200)
    assert 2.0 ** -10 < -ga.signed_error(ga.bf16_truncate(ref), ref) < 2.0 ** -8
    assert abs(ga.signed_error(ga.rne_bf16(ref), ref)) < 2.0 ** -14
    assert abs(ga.rms_ratio(ga.rne_bf16(ref), ref) - 1.0) < 1e-6
    buf, view = ga.fenced((5, 8), 16, torch.bfloat16)
    view.zero_()
    ga.assert_fence_intact(buf, (5, 8))
    buf[5, 0] = 1.0
    with pytest.raises(AssertionError, match=r"\(5, 0\)"):
        ga.assert_fence_intact(buf, (5, 8))
