"""CPU: the yardsticks of tests/parity_accuracy.py checked on themselves, at the shapes, classes and flags of
tests/test_gpu_parity_accuracy.py.

  * the sequential fp32 model of the kernels and a second, differently ordered fp32 model (pairwise summation for the GEMM, torch's
    own softmax and matmul for the attention) are inside every criterion;
  * every mutant of the model is rejected by a NAMED criterion wherever it applies; each rejection is printed as
    PARITY_MUTANT <mutant>: <criterion> (<where>)  (pytest -s, or -rP);
  * the ReLU-kink share the bound tier leaves out stays under its cap on the reference alone, for the inputs the GPU test uses."""
import math

import pytest
import torch

import attn_accuracy as aa
import gemm_accuracy as ga
import parity_accuracy as pa

B_, H_ = 2, 3
_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def rejected(mutant, criterion, where):
    print(f"PARITY_MUTANT {mutant}: {criterion} ({where})")


# ------------------------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------------------------
def exact_case(shape):
    def make():
        M, N, K = shape
        o = ga.exact_operands(M, N, K, pa.seed_of(shape))
        return o, ga.host_keep(M, N, 0.5, 1), pa.seq_gemm(o["a"], o["b"].t())
    return cached(("exact", shape), make)


def exact_mismatch(shape, name, mutant=None, order="ascending"):
    o, keep, acc = exact_case(shape)
    kw = pa.exact_epilogue(name, o, keep, lambda t: t.float())
    ref = ga.reference(o["a"], o["b"], **kw)
    if mutant in ("drop_last_k", "descending_k") or order != "ascending":
        c, pre = pa.gemm_model(o["a"], o["b"], order=order, mutant=mutant, **kw)
    else:
        c, pre = pa.epilogue32(acc, mutant=mutant, **kw)
    bad = not torch.equal(c.double(), ref.c)
    if ref.preact is not None:
        bad = bad or not torch.equal(pre.double(), ref.preact)
    return bad, kw


EXACT_NAMES = ga.EXACT_EPILOGUES + pa.EXACT_EXTRA_EPILOGUES


@pytest.mark.parametrize("shape", pa.EXACT_SHAPES, ids=str)
def test_models_meet_the_exact_tier_bit_for_bit(shape):
    for name in EXACT_NAMES:
        for order in ("ascending", "pairwise", "descending"):   # integer sums below 2^24: any order
            assert not exact_mismatch(shape, name, order=order)[0], (shape, name, order)


@pytest.mark.parametrize("mutant", ["drop_last_k", "bias_shift_one_column", "residual_after_dact"])
def test_gemm_mutant_misses_the_exact_tier(mutant):
    """In EVERY case it applies to at a shape of 1000 outputs and more; in at least one at a smaller shape (a single output can
    survive a ReLU or a dropped element by chance)."""
    hit = 0
    for shape in pa.EXACT_SHAPES:
        applied = seen = 0
        for name in EXACT_NAMES:
            bad, kw = exact_mismatch(shape, name, mutant)
            if pa.gemm_mutant_applies(mutant, shape[2], kw) and not (mutant == "bias_shift_one_column" and shape[1] == 1):
                assert bad or shape[0] * shape[1] < 1000, (mutant, shape, name)
                applied, seen = applied + 1, seen + bad
        assert seen or not applied, (mutant, shape)
        hit += seen
    assert hit
    rejected(mutant, "A1 exact tier, bit for bit", f"{hit} shape x epilogue cases")


@pytest.mark.parametrize("shape", pa.ROWSUM_SHAPES, ids=str)
def test_a_rowsum_model_and_mutants(shape):
    M, N, K = shape
    o = ga.exact_operands(M, N, K, pa.seed_of(shape) + 1)
    prior = (torch.arange(M) % 17 - 8).float()
    want = prior.double() + o["a"].sum(1)
    blocks = -(-N // 64)
    assert torch.equal(pa.rowsum_model(o["a"], prior).double(), want)
    assert not torch.equal(pa.rowsum_model(o["a"], prior, mutant="rowsum_overwritten").double(), want)
    rejected("rowsum_overwritten", "A1 a_rowsum exact", shape)
    if blocks > 1:
        assert not torch.equal(pa.rowsum_model(o["a"], prior, blocks, mutant="rowsum_per_column_block").double(), want)
        rejected("rowsum_per_column_block", "A1 a_rowsum exact", shape)


def test_at_least_one_rowsum_shape_has_several_column_blocks():
    assert any(N > 64 for _, N, _ in pa.ROWSUM_SHAPES) and any(M % 4 for M, _, _ in pa.ROWSUM_SHAPES)


def test_batch_levels_swapped_is_seen():
    b1, b2 = pa.BATCH
    M, N, K = 33, 17, 72
    o = ga.exact_operands(b1 * b2 * M, b1 * b2 * N, K, 4242)
    A4, B4 = o["a"].view(b1, b2, M, K), o["b"].view(b1, b2, N, K).transpose(-1, -2)
    ref = pa.batched_reference(A4, B4)
    assert torch.equal(pa.seq_gemm(A4, B4).double(), ref)
    assert not torch.equal(pa.batched_reference(A4, B4, swapped=True), ref)
    rejected("batch_levels_swapped", "A1 exact tier, batched", (b1, b2, M, N, K))


@pytest.mark.parametrize("shape", pa.ASCENDING_CASES, ids=str)
def test_ascending_k_tier_tells_the_orders_apart(shape):
    M, N, K = shape
    a, b = pa.twelve_bit_operands(M, N, K, pa.seed_of(shape))
    want = pa.seq_gemm(a, b.t())
    # every product is exact in fp32: the two-rounding form acc + a * b gives the bits of the FMA
    x = torch.zeros(M, N)
    for k in range(K):
        x = x + a[:, k, None] * b[None, :, k]
    assert torch.equal(x, want)
    if K > 2:
        assert not torch.equal(pa.seq_gemm(a, b.t(), "descending"), want)
        rejected("descending_k", "A2 ascending k, bit for bit", shape)
    if K > 8:
        assert not torch.equal(pa.seq_gemm(a, b.t(), "pairwise"), want)
    if K % 16:
        assert not torch.equal(pa.seq_gemm(a, b.t(), "drop_last_k"), want)
        rejected("drop_last_k", "A2 ascending k, bit for bit", shape)


def test_three_term_probe():
    a, b = pa.probe_operands()
    assert bool((pa.seq_gemm(a, b.t()) == 0).all()) and bool((pa.seq_gemm(a, b.t(), "descending") == 1).all())
    rejected("descending_k", "A2 three-term probe", "[2^24, 1, -2^24] . 1")


def bound_case(shape):
    def make():
        o = pa.bound_operands(*shape, pa.seed_of(shape))
        return o, pa.seq_gemm(o["a"], o["b"].t()), pa.seq_gemm(o["a"], o["b"].t(), "pairwise")
    return cached(("bound", shape), make)


def bound_ref(shape, name):
    def make():
        o, _, _ = bound_case(shape)
        kw = pa.bound_class(name, o)
        return kw, ga.reference(o["a"], o["b"], **kw)
    return cached(("bound_ref", shape, name), make)


@pytest.mark.parametrize("shape", pa.BOUND_SHAPES, ids=str)
def test_models_are_inside_every_bound_tier_criterion(shape):
    o, seq, pairwise = bound_case(shape)
    for name in pa.BOUND_CLASSES:
        kw, ref = bound_ref(shape, name)
        model = pa.epilogue32(seq, **kw)
        assert pa.gemm_criteria(*model, *model, ref) == [], (shape, name)
        assert pa.gemm_criteria(*pa.epilogue32(pairwise, **kw), *model, ref) == [], (shape, name, "pairwise")
        if name == "relu+deriv":
            assert pa.kink_share(ref) < pa.KINK_SHARE, (shape, pa.kink_share(ref))


@pytest.mark.parametrize("mutant", ["bias_shift_one_column", "residual_after_dact", "descending_k"])
def test_gemm_mutant_misses_the_bound_tier(mutant):
    """(descending k is a correct kernel to this tier: it must stay inside -- only A2 tells it apart.)"""
    for shape in pa.BOUND_SHAPES:
        o, seq, _ = bound_case(shape)
        for name in pa.BOUND_CLASSES:
            kw, ref = bound_ref(shape, name)
            model = pa.epilogue32(seq, **kw)
            if mutant == "descending_k":
                assert pa.gemm_criteria(*pa.gemm_model(o["a"], o["b"], mutant=mutant, **kw), *model, ref) == [], (shape, name)
            elif pa.gemm_mutant_applies(mutant, shape[2], kw):
                misses = pa.gemm_criteria(*pa.epilogue32(seq, mutant=mutant, **kw), *model, ref)
                assert misses, (mutant, shape, name)
                rejected(mutant, "A3 " + misses[0].split(":")[0], f"{shape} {name}")


# ------------------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------------------
def probe_keep(Lq, Lk):
    return aa.host_keep_mask(B_, H_, Lq, Lk, pa.PROBE_P, 11)


@pytest.mark.parametrize("Lq,Lk", pa.PROBE_SHAPES, ids=str)
def test_probability_bound_accepts_the_models_and_rejects_the_mutants(Lq, Lk):
    applies = {"sum_misses_last_key": ("plain", Lk % 64 != 0 and Lk > 1), "no_max_subtraction": ("bias30", True),
               "mask_by_head": ("tail_mask", Lk > 1), "bias_q_h": ("bias1", Lq > 1 and Lk > 1), "causal_off_by_one": ("causal", Lq > 1 and Lk > 1)}
    for i, variant in enumerate(pa.PROBE_VARIANTS):
        c = pa.probe_case(B_, H_, Lq, Lk, variant, 7000 + 31 * Lq + Lk + i)
        args = (c["q"], c["k"], c["H"], c["key_mask"], c["pos_bias"], c["causal"], c["scale"])
        drop = variant.startswith("dropout")
        keep = probe_keep(Lq, Lk) if drop else None
        P64, rel = pa.probs_bound(*args, drop=drop)
        scale_p = (lambda P: P * keep * (torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(pa.PROBE_P)))) if drop else (lambda P: P)
        for second in (False, True):
            assert pa.check_probs(scale_p(pa.seq_probs(*args, torch_softmax=second)), P64, rel, keep, pa.PROBE_P) is None, (variant, second)
        for mutant, (where, ok) in applies.items():
            if where == variant and ok:
                miss = pa.check_probs(pa.seq_probs(*args, mutant=mutant), P64, rel)
                assert miss, (mutant, Lq, Lk)
                rejected(mutant, "B1 " + miss.split(",")[0][:60], f"{Lq}x{Lk} {variant}")
        if variant == "dropout":
            miss = pa.check_probs(pa.seq_probs(*args) * keep, P64, rel, keep, pa.PROBE_P)
            assert miss, ("dropout_no_rescale", Lq, Lk)
            rejected("dropout_no_rescale", "B1 " + miss.split(",")[0][:60], f"{Lq}x{Lk}")
            wrong_zeros = pa.check_probs(scale_p(pa.seq_probs(*args)).roll(1, -1), P64, rel, keep, pa.PROBE_P)
            assert wrong_zeros or Lk == 1


def budget_case(label, Lq, Lk, Dh, kw):
    def make():
        case = pa.make_case(B_, H_, Lq, Lk, Dh, 8000 + Lq + 3 * Lk + Dh, **kw)
        if case["p"] > 0:
            case["keep"] = aa.host_keep_mask(B_, H_, Lq, Lk, case["p"], case["drop_seed"])
        _, ref = pa.attn_reference(case)
        return case, ref, pa.seq_attention(**pa.model_args(case), dpb_prior=case["dpb_prior"])
    return cached(("budget", label), make)


CASES = pa.budget_cases()


@pytest.mark.parametrize("label,Lq,Lk,Dh,kw", CASES, ids=[c[0] for c in CASES])
def test_budget_accepts_the_second_model(label, Lq, Lk, Dh, kw):
    case, ref, model = budget_case(label, Lq, Lk, Dh, kw)
    assert pa.budget_misses(model, model, ref) == []
    second = pa.seq_attention(**pa.model_args(case), dpb_prior=case["dpb_prior"], second=True)
    assert pa.budget_misses(second, model, ref) == [], label


BUDGET_MUTANTS = [m for m in pa.ATTN_MUTANTS if m != "no_max_subtraction"]   # (the same function without overflow: B1's bias30 sees it)


@pytest.mark.parametrize("mutant", BUDGET_MUTANTS)
def test_attention_mutant_misses_the_budget_wherever_it_applies(mutant):
    hit = 0
    for label, Lq, Lk, Dh, kw in CASES:
        if not pa.attn_mutant_applies(mutant, B_, H_, Lq, Lk, kw.get("masked", False), kw.get("bias", False), kw.get("causal", False),
                                      kw.get("p", 0) > 0):
            continue
        case, ref, model = budget_case(label, Lq, Lk, Dh, kw)
        got = pa.seq_attention(**pa.model_args(case), dpb_prior=case["dpb_prior"], mutant=mutant)
        # one visible key: P = 1 and dS = 0 whatever the kernel does; one query: (q H + h) = (h Lq + q) and no row below the diagonal
        degenerate = Lk == 1 or (case["causal"] and Lq == 1) or (Lq == 1 and mutant in ("bias_q_h", "causal_off_by_one"))
        misses = pa.budget_misses(got, model, ref)
        if degenerate:
            continue
        assert misses, (mutant, label)
        hit += 1
        if hit == 1:
            rejected(mutant, "B2 " + misses[0][:40], label)
    assert hit >= 2, mutant


def test_detour_bound_accepts_a_bf16_rounding_of_the_fp32_path():
    case = pa.make_case(B_, H_, 33, 65, 96, 9001, bias=True, causal=True, dtype=torch.bfloat16)
    _, ref = pa.attn_reference(case)
    model = pa.seq_attention(**pa.model_args(case), dpb_prior=case["dpb_prior"])
    second = pa.seq_attention(**pa.model_args(case), dpb_prior=case["dpb_prior"], second=True)
    for n in aa.NAMES:
        got = getattr(second, n) if n == "d_pos_bias" else getattr(second, n).to(torch.bfloat16)
        assert bool(((got.double() - getattr(ref, n).double()).abs() <= pa.detour_bound(ref, model, n)).all()), n
        twice = got.double() * (1 + 2.0 ** -7)   # one bf16 ulp off everywhere
        assert not bool(((twice - getattr(ref, n).double()).abs() <= pa.detour_bound(ref, model, n)).all()), n


def test_yardsticks_on_known_values():
    assert pa.gamma(64) > 64 * pa.U and pa.C_SOFTMAX == 17
    P64, rel = pa.probs_bound(torch.zeros(1, 2, 4), torch.zeros(1, 3, 4), 1, None, None, False, 0.5)
    assert torch.equal(P64, torch.full((1, 1, 2, 3), 1 / 3, dtype=torch.float64)) and torch.allclose(rel, torch.full_like(rel, 20 * pa.U))
    bufs, _ = pa.grad_views(pa.make_case(1, 1, 3, 3, 4, 0))
    assert pa.grads_fence_intact(bufs)
    bufs[0][0, 0, -1] = 0.0
    assert not pa.grads_fence_intact(bufs)
    assert math.isclose(pa.TINY, 1.1754943508222875e-38)
