"""CPU: the yardsticks of tests/norm_accuracy.py checked on themselves, at the cases of tests/test_gpu_norm_accuracy.py (row counts
above 1100 reduced to 4096 + M % 4096: still odd, still past one sweep of the backward grid).

  * the two numpy fp32 models of a correct kernel (pairwise and strictly sequential sums) stay inside the element-wise bound, the
    aggregate yardstick and the exact tier on every case, forward and every backward variant;
  * every mutant is rejected by at least one criterion on at least one case it applies to (asserted per mutant, by name; on the
    reduced large cases only the mutant that needs more than one sweep is run);
  * the loss references: the fp32 models of the cross-entropy and BCE kernels stay inside their bounds at every case of the GPU
    test, and the naive softplus form does not.

The worst model / bound ratios are printed (pytest -s) and recorded in tests/norm_accuracy.py as the measured headroom."""
import pytest
import torch

import norm_accuracy as na

LARGE_CASE_MUTANTS = ("dgamma_dbeta_miss_second_sweep",)


def _stats(fwd):
    return torch.from_numpy(fwd["mean"]), torch.from_numpy(fwd["rstd"])


def _run_case(case):
    """dict(pair=[misses], seq=[misses], figures={order: {}}, mutants={name: [misses] for the mutants that apply})."""
    inp = na.case_inputs(case)
    small = case["M"] <= na.HOST_SMALL_M
    res = dict(pair=[], seq=[], figures={"pair": {}, "seq": {}}, mutants={})
    fkw = dict(rms=case["rms"], act=case["act"], out_bf16=na.fwd_bf16(case))
    fwd = {o: na.model_fwd(inp["x"], inp["gamma"], inp["beta"], case["eps"], order=o, **fkw) for o in ("seq", "pair")}
    for o in ("pair", "seq"):
        res[o] += na.fwd_misses(case, inp, fwd[o], fwd["seq"], res["figures"][o])
    for m in na.FWD_MUTANTS:
        if small and na.mutant_applies(m, case, "fwd"):
            got = na.model_fwd(inp["x"], inp["gamma"], inp["beta"], case["eps"], order="pair", mutant=m, **fkw)
            res["mutants"].setdefault(m, []).extend(na.fwd_misses(case, inp, got, fwd["seq"]))
    mean, rstd = _stats(fwd["seq"])
    for v in case["bwd"]:
        keep = na.host_keep(case["M"], case["D"], na.DROP_P, na.DROP_SEED) if v.get("drop") else None
        kw = dict(out_bf16=na.bwd_bf16(case), **na.bwd_kw(case, inp, v, keep))
        run = lambda **k: na.model_bwd(inp["dy"], inp["x"], inp["gamma"], inp["beta"], mean, rstd, **kw, **k)
        seq = run(order="seq")
        for o in ("pair", "seq"):
            got = seq if o == "seq" else run(order="pair")
            res[o] += na.bwd_misses(case, inp, v, mean, rstd, got, seq, keep, res["figures"][o])
        for m in na.MUTANTS:
            if (small or m in LARGE_CASE_MUTANTS) and na.mutant_applies(m, case, v):
                res["mutants"].setdefault(m, []).extend(na.bwd_misses(case, inp, v, mean, rstd, run(order="pair", mutant=m), seq, keep))
    return res


@pytest.fixture(scope="module")
def results():
    return {c["name"]: _run_case(na.host_case(c)) for c in na.CASES}


def test_case_table_reaches_every_instantiation_and_mode():
    names = [c["name"] for c in na.CASES]
    assert len(set(names)) == len(names)
    bwd_d = {c["D"] for c in na.CASES if c["bwd"]}
    assert {na.padded_d(D) // 256 for D in bwd_d} == {1, 2, 3, 4, 6, 8}
    assert {na.padded_d(c["D"]) // 256 for c in na.CASES} == {1, 2, 3, 4, 6, 8, 16}
    assert {na.padded_d(D) // 256 for D in (1028, 1540)} == {6, 8}          # cpl 5 -> <6>, 7 -> <8>: one whole chunk empty
    assert {c["D"] for c in na.CASES if c["route"] == "pair"} == {512, 768, 1024}
    assert na.BIG_M > na.SWEEP_FWD and na.BIG_M > na.SWEEP_BWD and na.BIG_M % 2 == 1 and na.MID_M > na.SWEEP_BWD
    for c in na.CASES:
        h = na.host_case(c)
        assert h["M"] % 2 == c["M"] % 2 and (h["M"] > na.SWEEP_BWD) == (c["M"] > na.SWEEP_BWD), c["name"]
    variants = [v for c in na.CASES for v in c["bwd"]]
    for key in ("dx_add", "drop", "det", "lo"):
        assert any(v.get(key) for v in variants), key
    assert any(v.get("dbeta") is False for v in variants) and any(v.get("drop") == "rows" for v in variants)
    assert any(c["rms"] for c in na.CASES) and any(c["act"] == na.ACT_GELU and c["bwd"] for c in na.CASES)


@pytest.mark.parametrize("order", ["pair", "seq"])
def test_models_are_inside_the_bound_the_yardstick_and_the_exact_tier_on_every_case(results, order):
    misses = [m for r in results.values() for m in r[order]]
    assert misses == [], "\n".join(misses[:20])
    worst = {}
    for r in results.values():
        for k, val in r["figures"][order].items():
            worst[k] = max(worst.get(k, 0.0), val)
    print(f"NORM_ACCURACY host, {order} model over {len(results)} cases: " + ", ".join(f"worst {k} {val:.3f}" for k, val in sorted(worst.items())))
    assert 0 < worst["err/bound"] <= 1.0


@pytest.mark.parametrize("mutant", na.MUTANTS)
def test_mutant_is_rejected(results, mutant):
    applied = [n for n, r in results.items() if mutant in r["mutants"]]
    rejected = [n for n in applied if results[n]["mutants"][mutant]]
    print(f"NORM_ACCURACY host, mutant {mutant}: rejected on {len(rejected)} of the {len(applied)} cases it applies to; survives on "
          f"{sorted(set(applied) - set(rejected))}")
    assert applied, f"{mutant} applies to no case"
    assert rejected, f"{mutant} survives every case it applies to: {applied}"


def test_sums_are_what_they_say():
    import numpy as np
    a = np.array([[2.0 ** 24, 1.0, 1.0, 1.0, 1.0]], np.float32)
    assert na.sum_seq(a)[0] == 2.0 ** 24            # every 1 is lost against the running sum
    assert na.sum_pair(a)[0] == 2.0 ** 24 + 4       # (2^24 + 1 -> 2^24), (1 + 1), (1 + 0); 2^24 + 2; + 1 is a tie, to even
    assert na.padded_d(4) == 256 and na.padded_d(1028) == 1536 and na.padded_d(1540) == 2048 and na.padded_d(2052) == 4096


# ------------------------------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_xent_model_is_inside_the_bound(bf16):
    worst = 0.0
    for rows in na.XENT_ROWS:
        for C in na.XENT_C:
            for labelled in ("some", "one", "none"):
                x, lab = na.xent_inputs(rows, C, bf16, labelled)
                loss, grad, m = na.xent_reference(x, lab, na.GRAD_SCALE)
                e_loss, e_grad = na.xent_bound(grad, m, bf16)
                got_loss, got_grad = na.xent_model(x, lab, na.GRAD_SCALE, bf16)
                assert torch.isfinite(loss) and abs(float(got_loss) - loss.item()) <= e_loss.item(), (rows, C, labelled)
                fig = {}
                assert na.check_bound(got_grad, grad, e_grad, "d_logits", fig) is None, (rows, C, labelled)
                worst = max(worst, fig["err/bound"])
                if labelled == "none":
                    assert loss.item() == 0.0 and not grad.any()
            if rows > 1:
                x, lab = na.xent_inputs(rows, C, bf16)
                mx = x.float().max(1).values
                top = 60.0 if bf16 else 80.0
                assert mx.max() == top and mx.min() == -top and (lab == na.IGNORE).any() and (lab == 0).any() and (lab == C - 1).any()
    print(f"NORM_ACCURACY host, xent model: worst gradient err/bound {worst:.3f}")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_bce_model_is_inside_the_bound_and_the_naive_form_is_not(bf16):
    for B, C in na.BCE_SHAPES:
        x, z = na.bce_inputs(B, C, bf16)
        loss, grad, m = na.bce_reference(x, z, na.GRAD_SCALE)
        e_loss, e_grad = na.bce_bound(loss, grad, m, bf16)
        got_loss, got_grad = na.bce_model(x, z, na.GRAD_SCALE, bf16)
        assert abs(float(got_loss) - loss.item()) <= e_loss.item(), (B, C, float(got_loss), loss.item(), e_loss.item())
        assert na.check_bound(got_grad, grad, e_grad, "d_logits") is None, (B, C)
        if B * C >= 8:
            assert (x.float().view(-1)[0] == 0) and x.float().abs().max() == (88.0 if bf16 else 100.0)
            if not bf16:   # exp(100) overflows fp32 (exp(88), the bf16 cases' extreme, does not)
                bad_loss, _ = na.bce_model(x, z, na.GRAD_SCALE, bf16, mutant="naive_softplus")
                assert not abs(float(bad_loss) - loss.item()) <= e_loss.item()
