"""Accuracy yardsticks of the bf16 MFMA GEMMs (csrc/gemm_mfma.hip, csrc/gemm_nt_pp2.hip, the epilogues of csrc/gemm_nt_common.h),
shared by tests/test_gpu_gemm_accuracy.py and its host-side self-check tests/test_gemm_accuracy_host.py.  Plain torch: nothing here
imports or calls the library.

A product of two bf16 values is exact in fp32, so a bf16 GEMM has three sources of error only: the fp32 accumulation, a handful of
fp32 epilogue operations and ONE bf16 rounding at each store.  Two tiers follow from that.

Exact tier (exact_operands): integer-valued operands small enough that every fp32 value the kernel forms -- every partial sum in any
order, split-K atomics included, and every epilogue value -- is an integer (or a multiple of 1/2) below 2^24 and therefore exact.  The
expected output is then known bit for bit: rne_bf16(exact) for a bf16 C, `exact` for an fp32 C.  Linear epilogues only (no erf / exp).

Bound tier (reference + bound): random operands against float64, element by element.  With
    U       = 2^-24                                  one fp32 rounding, relative (round to nearest)
    hulp(x) = 2^(floor(log2 |x|) - 8), hulp(0) = 0   half a bf16 ulp at x (bf16 keeps 8 significand bits)
and e = the bound on |kernel's fp32 value - float64 value| right before a store,
    bf16 store:  |got - ref| <= hulp(|ref| + e) + e          (the rounding acts on the fp32 value, which may sit one binade up)
    fp32 store:  |got - ref| <= e.
e is carried through the epilogue in the order of include/m3ae_hip.h (alpha, bias, preact store, act, dropout, residual, dact_aux
multiply, accumulate), from these constants -- every one follows from U, K and a number written in the sources:

  accumulation  2 K U |alpha| (|A||B|)_mn.  One fp32 rounding per reduction element of a running sum bounded by (|A||B|)_mn gives
                K U; the factor 2 is the one the fp32x3 bound carries for the same v_mfma_f32_16x16x32_bf16 (include/m3ae_hip.h,
                M3AE_GEMM_F32_X3: "K 2^-23" = 2 K U), which covers the instruction's internal summation order and the split-K
                additions (at most K / 512 of them: tn_pp_splits gives a split at least 8 steps of 64 rows, tn_t_splits 16).
  one fp32 op   + U |result|: the alpha multiply, the bias add, the residual add, the accumulate add, the dact_aux multiply.
  dropout       x * inv_keep: e * inv_keep + 2 U |result| (the product, and inv_keep = fl(1 / (1 - p)) itself, csrc/common.h make_drop;
                at p = 0.5 both are exact).
  accumulate    NT: one add, U |result|.  TN (split-K atomics into C): at most max(1, K / 512) adds, each rounding a running value
                bounded by |C_old| + |alpha| (|A||B|)_mn:  max(1, K / 512) U (|C_old| + |alpha| (|A||B|)_mn).
  activation    e <- LIP[act] e + eval(act, x) with LIP = max |act'|:
                  GELU       x Phi(x):    act' = Phi + x phi, maximal at x = sqrt 2: 0.92135 + 0.20755 = 1.1290 <= 1.13
                  QuickGELU  x s(1.702 x): act' = s + u s (1 - s), u = 1.702 x; the swish derivative peaks at 1.0998 <= 1.13
                  ReLU       1 (<= 1.13);   tanh  1
                eval(act, x), the error of the kernel's own evaluation at an exact argument (csrc/common.h):
                  GELU (gelu_terms_fast): cdf = 0.5 erfc by Abramowitz-Stegun 7.1.26, "|abs err| < 1.5e-7" on erf, so 0.75e-7 on the
                    cdf; its arithmetic: t = v_rcp(fma(c, |x|, 1)) has 2 roundings + 1 ulp (= 2 U) of v_rcp = 4 U relative; t poly(t)
                    is a degree-5 polynomial whose coefficient-weighted degree sum(k |a_k|) = 0.2548 + 2 x 0.2845 + 3 x 1.4214 +
                    4 x 1.4532 + 5 x 1.0614 = 16.2 bounds its condition number on (0, 1] (its value at t = 1 is 1.0): 4 U x 16.2 = 65 U;
                    the four fma roundings act on intermediates <= 1.5 against poly >= 0.2548: 4 x 1.5 / 0.2548 = 24 U; the exponent
                    x^2 c has two roundings, 2 U x 0.72 x^2 x ln 2 = U x^2 relative on e, and x^2 erfc(x / sqrt 2) / 2 <= 0.15, i.e.
                    < 1 U absolute; v_exp2 1 ulp = 2 U; three multiplies 3 U: (65 + 24 + 2 + 3) U = 94 U relative on a value <= 0.5,
                    47 U absolute, + 1 U (x^2 term) + 1 U (1 - h) = 49 U.  cdf error DCDF = 0.75e-7 + 49 U; x cdf: |x| DCDF + U |result|.
                  GELU' = fma(x, pdf, cdf), pdf = c e with e as above ((2 + x^2) U relative, + U for the multiply):
                    DCDF + |x| (3 + x^2) U phi(x) + U |result|.
                  QuickGELU: s = v_rcp(1 + v_exp2(k x)), k = fl(-1.702 log2 e): the constant and the product round the exponent twice,
                    2 U x 1.702 |x| relative on the exponential; v_exp2 2 U, the add U, v_rcp 2 U:  RS = (5 + 3.5 |x|) U relative on s.
                    x s: |x| s RS + U |result|.
                  QuickGELU' = s g, g = 1 + 1.702 x (1 - s): d(1 - s) = s RS + U; dg = 1.702 |x| (s RS + U) + 2 U 1.702 |x| (1 - s) + U |g|;
                    total |g| s RS + s dg + U |result|.
                  tanh (libm tanhf; OpenCL C full-profile limit 5 ulp = 10 U, which the ROCm device library meets): 10 U |t|;
                    tanh' = 1 - t^2: 2 |t| 10 U |t| + U t^2 + U |result|.
                  ReLU and its step: exact.
  derivatives   a derivative output (preact with preact_grad) or factor (dact) evaluated at an inexact argument moves by
                LIP2[act] e with LIP2 = max |act''|: GELU phi(x) (2 - x^2), maximal at 0: 2 phi(0) = 0.7979 <= 0.8; QuickGELU
                1.702 x max |swish''| = 1.702 / 2 = 0.851; tanh 4 / (3 sqrt 3) = 0.77.  ReLU's step is discontinuous: where
                |x| <= e either value is right and the bound is 1.  (dact_aux is a stored tensor: its argument is exact.)

Aggregate yardsticks, for cases of at least 10^4 elements:
  signed_error  sum((got - ref) sign(ref)) / sum |ref|, budget |.| <= 2^-12.  A truncating conversion loses between 0 and one bf16 ulp
                (2^-8 to 2^-7 relative) on every element, all with the sign of -ref: between 2^-10 and 2^-8 by construction.  Round to
                nearest has mean 0 and a spread of 2^-8 / sqrt(12 n): below 2^-14 from n = 10^4 on.  (One output is not spread
                evenly over its bf16 intervals: the GELU / QuickGELU derivative saturates just above 1 and just below 0, and
                rne_bf16 of the float64 reference itself has a signed error of 1e-4 to 2e-4 there -- inside the budget.)
  rel_rms       for a bf16 C, rel_rms(got - ref) <= 1.1 rel_rms(rne_bf16(ref) - ref), the right side computed from the reference on
                every run.  1.1 < sqrt(1 + 0.5^2): a second independent error of up to 0.46 of a bf16 rounding passes (far above e),
                one extra bf16 rounding (sqrt 2) does not.

When a kernel misses a budget it is wrong, or it rounds somewhere reference() and bound() do not model: then that rounding goes
into bound(), with the source line that performs it.  The factors stay.

Layouts: a [M, K] and b [N, K] (C = a b^T; the wgrad tests pass dY^T and X^T), bias [N], everything else [M, N]."""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24
ACT_NONE, ACT_GELU, ACT_QUICKGELU, ACT_TANH, ACT_RELU, ACT_MULAUX = 0, 1, 2, 3, 4, 5   # include/m3ae_hip.h
LIP = {ACT_NONE: 1.0, ACT_GELU: 1.13, ACT_QUICKGELU: 1.13, ACT_TANH: 1.0, ACT_RELU: 1.0}
LIP2 = {ACT_GELU: 0.8, ACT_QUICKGELU: 0.851, ACT_TANH: 0.77}
AS_CDF = 0.75e-7           # half of Abramowitz-Stegun 7.1.26's 1.5e-7 (csrc/common.h)
DCDF = AS_CDF + 49 * U
TANH_ULPS = 10 * U
QG = 1.702
SIGNED_BUDGET = 2.0 ** -12
RMS_FACTOR = 1.1
MIN_AGGREGATE = 10 ** 4    # the aggregate yardsticks need this many elements
EXACT_LIMIT = 2.0 ** 24
FENCE = 24576.0            # finite, exact in bf16 and fp32

Ref = namedtuple("Ref", "c preact absprod mags")


def rne_bf16(x):
    """Round to nearest even to bf16, returned in x's dtype.  (float64 goes through fp32 first: exact for the exact tier, whose values
    are fp32 values, and a 2^-29 relative effect on the rms yardstick.)"""
    return x.float().to(torch.bfloat16).to(x.dtype)


def bf16_truncate(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def bf16_half_up(x):
    """Adds half an ulp to the magnitude and truncates: ties go away from zero instead of to even."""
    return ((x.float().contiguous().view(torch.int32) + 0x8000) & -65536).view(torch.float32)


def hulp(x):
    x = x.abs().double()
    _, ex = torch.frexp(x)                       # x = m 2^ex, m in [0.5, 1): floor(log2 x) = ex - 1
    return torch.where(x > 0, torch.ldexp(torch.ones_like(x), ex - 9), torch.zeros_like(x))


def _phi(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _cdf(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def act_value(x, act):
    if act == ACT_GELU:
        return x * _cdf(x)
    if act == ACT_QUICKGELU:
        return x * torch.sigmoid(QG * x)
    if act == ACT_TANH:
        return torch.tanh(x)
    if act == ACT_RELU:
        return torch.clamp(x, min=0)
    return x


def act_grad(x, act):
    """act'(x); ACT_MULAUX: the value itself (the stored tensor already is the derivative)."""
    if act == ACT_GELU:
        return _cdf(x) + x * _phi(x)
    if act == ACT_QUICKGELU:
        s = torch.sigmoid(QG * x)
        return s * (1.0 + QG * x * (1.0 - s))
    if act == ACT_TANH:
        return 1.0 - torch.tanh(x) ** 2
    if act == ACT_RELU:
        return (x > 0).to(x.dtype)
    if act == ACT_MULAUX:
        return x
    return torch.ones_like(x)


def reference(a, b, *, alpha=1.0, bias=None, act=ACT_NONE, want_preact=False, preact_grad=False, keep=None, p=0.0, residual=None,
              dact_aux=None, dact=ACT_NONE, c_old=None):
    """float64 from the operands as given (bf16-rounded or fp32 tensors), in the epilogue order of include/m3ae_hip.h.  Returns
    Ref(c, preact, absprod, mags): preact is None unless want_preact; mags holds every intermediate bound() needs."""
    dt = torch.float64
    a, b = a.to(dt), b.to(dt)
    s = a @ b.t()
    absprod = a.abs() @ b.abs().t()
    m = {"alpha": float(alpha), "act": act, "dact": dact, "preact_grad": bool(preact_grad), "K": a.shape[1]}
    x = s * alpha
    m["acc"] = x
    if bias is not None:
        x = x + bias.to(dt)[None, :]
        m["bias"] = x
    m["pre"] = x
    preact = None
    if want_preact:
        preact = act_grad(x, act) if preact_grad else x
    x = act_value(x, act)
    m["act_out"] = x
    if keep is not None:
        inv = 1.0 / (1.0 - p)
        x = x * keep.to(dt) * inv
        m["inv_keep"], m["drop"], m["keep"] = inv, x, keep.to(torch.bool)
    if residual is not None:
        x = x + residual.to(dt)
        m["res"] = x
    if dact_aux is not None:
        g = act_grad(dact_aux.to(dt), dact)
        m["aux"], m["g"], m["before_g"] = dact_aux.to(dt), g, x
        x = x * g
        m["dmul"] = x
    if c_old is not None:
        m["c_old"] = c_old.to(dt)
        x = x + m["c_old"]
    return Ref(x, preact, absprod, m)


def _eval_act(x, act):
    """eval(act, x) of the module docstring: the kernel's evaluation error of act at an exact fp32 argument x."""
    ax = x.abs()
    if act == ACT_GELU:
        return ax * DCDF + U * act_value(x, act).abs()
    if act == ACT_QUICKGELU:
        s = torch.sigmoid(QG * x)
        return ax * s * (5 + 3.5 * ax) * U + U * (x * s).abs()
    if act == ACT_TANH:
        return TANH_ULPS * torch.tanh(x).abs()
    return torch.zeros_like(x)


def _eval_grad(x, act):
    """The same for act'(x)."""
    ax = x.abs()
    d = act_grad(x, act).abs()
    if act == ACT_GELU:
        return DCDF + ax * (3 + x * x) * U * _phi(x) + U * d
    if act == ACT_QUICKGELU:
        s = torch.sigmoid(QG * x)
        rs = (5 + 3.5 * ax) * U
        g = (1.0 + QG * x * (1.0 - s)).abs()
        dg = QG * ax * (s * rs + U) + 2 * U * QG * ax * (1.0 - s) + U * g
        return g * s * rs + s * dg + U * d
    if act == ACT_TANH:
        t = torch.tanh(x).abs()
        return 2 * t * TANH_ULPS * t + U * t * t + U * d
    return torch.zeros_like(x)


def _store_bound(ref, e, bf16):
    return hulp(ref.abs() + e) + e if bf16 else e


def bound(ref, c_bf16, tn=False):
    """Element-wise bounds (c_bound, preact_bound) on |got - ref| for the stores of a call whose float64 result is `ref`
    (reference()'s return value); preact_bound is None without a preact output.  tn: the split-K wgrad family (accumulate by
    atomics).  Derivation: module docstring."""
    m = ref.mags
    K, alpha, act = m["K"], abs(m["alpha"]), m["act"]
    e = 2 * K * U * alpha * ref.absprod + U * m["acc"].abs()
    if "bias" in m:
        e = e + U * m["bias"].abs()
    pre_bound = None
    if ref.preact is not None:
        if not m["preact_grad"]:
            pre_bound = _store_bound(ref.preact, e, c_bf16)
        elif act == ACT_RELU:
            pre_bound = torch.where(m["pre"].abs() <= e, torch.ones_like(e), torch.zeros_like(e))
        else:
            ed = LIP2.get(act, 0.0) * e + _eval_grad(m["pre"], act)
            pre_bound = _store_bound(ref.preact, ed, c_bf16)
    e = LIP[act] * e + _eval_act(m["pre"], act)
    if "drop" in m:
        e = torch.where(m["keep"], e * m["inv_keep"] + 2 * U * m["drop"].abs(), torch.zeros_like(e))   # a dropped element is exactly 0
    if "res" in m:
        e = e + U * m["res"].abs()
    if "dmul" in m:
        eg = _eval_grad(m["aux"], m["dact"]) if m["dact"] != ACT_MULAUX else torch.zeros_like(e)
        e = e * m["g"].abs() + m["before_g"].abs() * eg + U * m["dmul"].abs()
    if "c_old" in m:
        if tn:
            e = e + max(1.0, K / 512.0) * U * (m["c_old"].abs() + alpha * ref.absprod)
        else:
            e = e + U * ref.c.abs()
    return _store_bound(ref.c, e, c_bf16), pre_bound


def signed_error(got, ref):
    got, ref = got.double(), ref.double()
    return (((got - ref) * torch.sign(ref)).sum() / ref.abs().sum()).item()


def rel_rms(err, ref):
    return math.sqrt(((err.double() ** 2).mean() / (ref.double() ** 2).mean()).item())


def rms_ratio(got, ref):
    """rel_rms(got - ref) over the yardstick rel_rms(rne_bf16(ref) - ref); the budget is RMS_FACTOR."""
    ref = ref.double()
    num, den = rel_rms(got.double() - ref, ref), rel_rms(rne_bf16(ref) - ref, ref)
    if den == 0.0:   # every reference value is a bf16 value (ReLU's step): any error at all is over the budget
        return 0.0 if num == 0.0 else math.inf
    return num / den


def first_bad(bad):
    """(m, n) of the first set element of a 2-D mask, with the tile-relative coordinates the failure messages carry."""
    idx = torch.nonzero(bad.reshape(bad.shape[-2], bad.shape[-1]))[0]
    m_, n_ = int(idx[0]), int(idx[1])
    return f"first bad (m, n) = ({m_}, {n_}), m % 256 = {m_ % 256}, n % 256 = {n_ % 256}, {int(bad.sum())} of {bad.numel()} bad"


def check_bound(got, ref, bnd, figures=None, name="c"):
    """None, or the description of the violation.  figures: dict collecting the worst err / bound seen (for the record)."""
    err = (got.double() - ref).abs()
    if not torch.isfinite(got.float()).all():
        return f"{name}: non-finite output, " + first_bad(~torch.isfinite(got.float()))
    ratio = torch.where(bnd > 0, err / bnd, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    if figures is not None:
        figures["err/bound"] = max(figures.get("err/bound", 0.0), ratio.max().item())
    bad = err > bnd
    if bad.any():
        return f"{name}: element-wise bound violated, worst err / bound {ratio.max().item():.3f}, " + first_bad(bad)
    return None


def check_aggregate(got, ref, c_bf16, figures=None, name="c"):
    """Signed-error and rms budgets (cases of at least MIN_AGGREGATE elements); None or the description of the miss."""
    if ref.numel() < MIN_AGGREGATE:
        return None
    se = signed_error(got, ref)
    if figures is not None:
        figures["signed"] = max(figures.get("signed", 0.0), abs(se))
    if not abs(se) <= SIGNED_BUDGET:
        return f"{name}: signed error {se:.3e} (2^{math.log2(abs(se)):.1f}) over the budget 2^-12"
    if c_bf16:
        r = rms_ratio(got, ref)
        if figures is not None:
            figures["rms"] = max(figures.get("rms", 0.0), r)
        if not r <= RMS_FACTOR:
            return f"{name}: rel_rms {r:.3f} x the bf16 rounding of the reference, budget {RMS_FACTOR}"
    return None


def criteria(got_c, got_pre, ref, c_bf16, tn=False, figures=None):
    """Every bound-tier criterion on the outputs of one call; list of misses (empty = inside all of them)."""
    cb, pb = bound(ref, c_bf16, tn)
    out = [check_bound(got_c, ref.c, cb, figures, "c"), check_aggregate(got_c, ref.c, c_bf16, figures, "c")]
    if ref.preact is not None:
        out += [check_bound(got_pre, ref.preact, pb, figures, "preact"), check_aggregate(got_pre, ref.preact, c_bf16, figures, "preact")]
    return [o for o in out if o]


# ------------------------------------------------------------------------------------------------------------------------
# exact tier
# ------------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, lo, hi, device, skip_below=0):
    """Uniform integers in [lo, hi] as float64; skip_below: magnitudes below it are left out (drawn as sign x magnitude)."""
    if skip_below:
        mag = torch.randint(skip_below, hi + 1, shape, generator=g, device=device)
        sgn = torch.randint(0, 2, shape, generator=g, device=device) * 2 - 1
        return (mag * sgn).double()
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).double()


def exact_operands(M, N, K, seed, device="cpu", alpha=None, inv_keep=2.0, ab_max=8):
    """Integer-valued operands of the exact tier: a [M, K], b [N, K] in [-8, 8] (magnitudes 3..8: at K = 64 the sums then have a
    standard deviation of 265, so a good share of them lies beyond the 256 from which bf16 has to round), bias [N] in [-64, 64],
    residual, c_old [M, N] in [-128, 128], aux [M, N] in [-8, 8]; alpha from {0.5, 1, 2} (drawn, unless given).  All float64 tensors
    holding bf16-exact values.  Refuses (AssertionError) a configuration in which some fp32 value of the kernel could reach 2^24:
    the chain  ((K max|a| max|b| |alpha| + max|bias|) inv_keep + max|residual|) max|aux| + max|c_old|  bounds every partial sum, in any
    order, and every epilogue value of every epilogue of the tier; with alpha = 0.5 the values are multiples of 1/2, exact below 2^23."""
    g = torch.Generator(device=device).manual_seed(seed)
    a = _ints(g, (M, K), -ab_max, ab_max, device, skip_below=min(3, ab_max))
    b = _ints(g, (N, K), -ab_max, ab_max, device, skip_below=min(3, ab_max))
    bias = _ints(g, (N,), -64, 64, device)
    residual = _ints(g, (M, N), -128, 128, device)
    c_old = _ints(g, (M, N), -128, 128, device)
    aux = _ints(g, (M, N), -8, 8, device)
    if alpha is None:
        alpha = (0.5, 1.0, 2.0)[int(torch.randint(0, 3, (1,), generator=g, device=device).item())]
    ops = dict(a=a, b=b, bias=bias, residual=residual, c_old=c_old, aux=aux, alpha=alpha)
    assert_exact(ops, K, inv_keep)
    return ops


def assert_exact(ops, K, inv_keep=2.0, alphas=None):
    """The 2^24 condition of exact_operands, for every alpha the caller is going to use."""
    for alpha in alphas or (ops["alpha"], 0.5):
        top = K * ops["a"].abs().max().item() * ops["b"].abs().max().item() * abs(alpha) + ops["bias"].abs().max().item()
        top = (top * inv_keep + ops["residual"].abs().max().item()) * max(1.0, ops["aux"].abs().max().item()) + ops["c_old"].abs().max().item()
        limit = EXACT_LIMIT if float(alpha).is_integer() else EXACT_LIMIT / 2
        assert top < limit, f"exact tier: a partial sum or epilogue value could reach {top:.0f} >= {limit:.0f} (K = {K}, alpha = {alpha})"


def expected_store(exact, c_bf16):
    return rne_bf16(exact) if c_bf16 else exact


def rounding_shares(exact):
    """(share of values that bf16 has to round, share that are exact ties) of a float64 tensor of fp32-exact values."""
    lo, hi = bf16_truncate(exact).double(), None
    r = rne_bf16(exact)
    inexact = r != exact
    hi = torch.where(exact >= 0, lo + 2 * hulp(exact), lo - 2 * hulp(exact))
    tie = inexact & ((exact - lo).abs() == (hi - exact).abs())
    return inexact.double().mean().item(), tie.double().mean().item()


# epilogues of the exact tier (the linear classes of launch_nt: PLAIN, RELU, DMUL, and -- "dmul+pre": a derivative operand together
# with a stored preact, which only the catch-all class serves -- ANY), as keyword sets of reference() / model()
EXACT_EPILOGUES = ("plain", "bias+res", "bias+relu+pre+drop+res", "drop+res+dmul", "alpha0.5+acc", "dmul+pre")


def exact_epilogue(name, ops, keep, cast=lambda t: t):
    """reference() / model() keywords of a named exact-tier epilogue from exact_operands' tensors; cast: the storage dtype of the
    [M, N] operands (bf16 or fp32; integer values survive it)."""
    kw = dict(alpha=ops["alpha"])
    if name == "bias+res":
        kw.update(bias=ops["bias"].float(), residual=cast(ops["residual"]))
    elif name == "bias+relu+pre+drop+res":
        kw.update(bias=ops["bias"].float(), act=ACT_RELU, want_preact=True, keep=keep, p=0.5, residual=cast(ops["residual"]))
    elif name == "drop+res+dmul":
        kw.update(dact_aux=cast(ops["aux"]), dact=ACT_MULAUX, keep=keep, p=0.5, residual=cast(ops["residual"]))
    elif name == "alpha0.5+acc":
        kw.update(alpha=0.5, c_old=cast(ops["c_old"]))
    elif name == "dmul+pre":   # preact = alpha acc, C = preact * aux
        kw.update(dact_aux=cast(ops["aux"]), dact=ACT_MULAUX, want_preact=True)
    else:
        assert name == "plain", name
    return kw


# ------------------------------------------------------------------------------------------------------------------------
# fp32 model of the kernels, and its mutants
# ------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("truncate", "half_up", "scale_1p2m8", "round_preact_before_act", "drop_last_k", "bias_shift_one_column",
           "residual_from_last_row", "aux_from_residual", "alpha_after_bias", "dropout_after_residual", "tanh_gelu",
           "accumulate_ignored")


def mutant_applies(mutant, M, N, K, c_bf16, kw, exact):
    """Whether `mutant` changes what the model computes for this shape and these reference() keywords -- and, for the two mutants
    whose effect is a fraction of a bf16 rounding, whether the yardsticks resolve it there."""
    act, has = kw.get("act", ACT_NONE), lambda k: kw.get(k) is not None
    return {
        "truncate": c_bf16,
        # ties have measure zero among random operands: only the exact tier, which is full of them, tells half-up from half-even
        "half_up": c_bf16 and exact,
        # one more bf16 rounding in front of a smooth activation (ReLU commutes with it; tanh' < 1 shrinks it to a fraction of the
        # output's own rounding); an fp32 store has nothing to compare it with
        "round_preact_before_act": c_bf16 and not exact and act in (ACT_GELU, ACT_QUICKGELU),
        "bias_shift_one_column": has("bias") and N > 1,
        # the clamped prefetch row M - 1 in place of the rows of the last 8-row pass: needs a row beside M - 1 in that pass
        "residual_from_last_row": has("residual") and (M - 1) % 8 != 0,
        "aux_from_residual": has("residual") and has("dact_aux"),
        "alpha_after_bias": has("bias") and kw.get("alpha", 1.0) != 1.0,
        "dropout_after_residual": has("keep") and has("residual"),
        # the tanh form of GELU is within 5e-4 of the erf form: resolved while 2 K U (|A||B|) stays below that, K <= 256
        "tanh_gelu": act == ACT_GELU and K <= 256 and c_bf16 and not exact,
        "accumulate_ignored": has("c_old"),
    }.get(mutant, True)


def model(a, b, c_bf16, *, alpha=1.0, bias=None, act=ACT_NONE, want_preact=False, preact_grad=False, keep=None, p=0.0, residual=None,
          dact_aux=None, dact=ACT_NONE, c_old=None, mutant=None):
    """What a correct kernel computes, in fp32 torch: a.float() @ b.float().t(), the epilogue in fp32 in the header's order, one
    rne_bf16 at each bf16 store.  Returns (c, preact) as fp32 tensors holding the stored values.  mutant: one of MUTANTS."""
    f = torch.float32
    a, b = a.to(f), b.to(f)
    if mutant == "drop_last_k":
        a, b = a[:, :-1], b[:, :-1]
    store = {"truncate": bf16_truncate, "half_up": bf16_half_up}.get(mutant, lambda t: rne_bf16(t)) if c_bf16 else (lambda t: t)
    x = a @ b.t()
    if mutant != "alpha_after_bias":
        x = x * alpha
    if bias is not None:
        bb = bias.to(f)
        x = x + (torch.roll(bb, -1) if mutant == "bias_shift_one_column" else bb)[None, :]
    if mutant == "alpha_after_bias":
        x = x * alpha
    preact = None
    if want_preact:
        preact = store(act_grad(x, act) if preact_grad else x)
    if mutant == "round_preact_before_act":
        x = rne_bf16(x)
    if mutant == "tanh_gelu" and act == ACT_GELU:
        x = 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    else:
        x = act_value(x, act)
    inv = 1.0 / (1.0 - p)
    if keep is not None and mutant != "dropout_after_residual":
        x = x * keep.to(f) * inv
    if residual is not None:
        r = residual.to(f)
        if mutant == "residual_from_last_row":
            r = r.clone()
            r[(r.shape[0] - 1) // 8 * 8:] = r[-1]
        x = x + r
    if keep is not None and mutant == "dropout_after_residual":
        x = x * keep.to(f) * inv
    if dact_aux is not None:
        src = residual if (mutant == "aux_from_residual" and residual is not None) else dact_aux
        x = x * act_grad(src.to(f), dact)
    if c_old is not None and mutant != "accumulate_ignored":
        x = x + c_old.to(f)
    if mutant == "scale_1p2m8":
        x = x * (1.0 + 2.0 ** -8)
    return store(x), preact


# ------------------------------------------------------------------------------------------------------------------------
# fenced outputs
# ------------------------------------------------------------------------------------------------------------------------
SPARE_ROWS = 3


def fenced(shape, ld, dtype, device="cpu"):
    """(buffer, view): view [M, N] with row stride ld inside a buffer [M + SPARE_ROWS, ld] filled with FENCE: SPARE_ROWS rows after M
    and ld - N columns after N that no kernel may touch."""
    M, N = shape
    assert ld >= N
    buf = torch.full((M + SPARE_ROWS, ld), FENCE, dtype=dtype, device=device)
    return buf, buf[:M, :N]


def strided(t, ld, dtype=None):
    """A copy of the 2-D tensor t at row stride ld (the padding holds FENCE: an operand read past its row shows up in the result)."""
    buf, view = fenced(t.shape, ld, dtype or t.dtype, t.device)
    view.copy_(t)
    return view


def assert_fence_intact(buf, shape, msg=""):
    M, N = shape
    word = torch.int16 if buf.element_size() == 2 else torch.int32
    want = torch.full((1,), FENCE, dtype=buf.dtype, device=buf.device).view(word)
    bits = buf.view(word)
    bad = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    bad[M:, :] = bits[M:, :] != want
    bad[:M, N:] = bits[:M, N:] != want
    assert not bad.any(), f"{msg}: wrote outside the [{M}, {N}] output (row stride {buf.shape[1]}): " + first_bad(bad)


# ------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_gemm_accuracy.py (tests/test_gemm_accuracy_host.py runs the model on the same ones, M <= HOST_MAX_M)
# ------------------------------------------------------------------------------------------------------------------------
HOST_MAX_M = 600
NT_EXACT_CASES = [   # (M, N, K), NT variants
    ((1, 8, 64), (0,)),
    ((130, 132, 64), (0, 4, 7)),
    ((300, 264, 64), (0, 4, 7, -1)), ((300, 264, 128), (0, 4, 7, -1)), ((300, 264, 192), (0, 7, -1)),
    ((300, 264, 256), (0, 4, 7, 9, 10, -1)), ((300, 264, 320), (0, 7, 9, 10)), ((300, 264, 3072), (0, 4, 7, 9, 10, -1)),
    ((5125, 3336, 256), (10, -1)),
    ((43557, 520, 128), (7,)),
]
TN_EXACT_CASES = [((128, 128, 37), (0, 2)), ((128, 256, 1154), (0, 2)), ((256, 128, 1024), (0, 2)), ((256, 256, 4133), (0, 2, 5)),
                  ((256, 256, 4620), (0, 2, 5)), ((256, 256, 4650), (0, 2, 5)), ((256, 256, 4100), (0, 2, 5))]
# variant 5 (the 256 x 256 ping-pong kernel): 32-row chunks in the LAST split of an accumulating call -- 4 and more fill the ring's
# prologue, 1 / 2 / 3 take its short branches and the short-remainder waits of the loop
TN_PP_TAIL_CHUNKS = {(256, 256, 4133): 4, (256, 256, 4620): 1, (256, 256, 4650): 2, (256, 256, 4100): 3}
GENERIC_EXACT_SHAPES = [(33, 50, 72), (17, 498, 100)]
BOUND_CASES = [((130, 132, 64), (0, -1)), ((300, 264, 256), (0, 4, 7, 9, -1)), ((257, 136, 768), (0, 7, 9, -1))]
TN_BOUND_CASES = [((256, 256, 4133), (0, 5, -1)), ((128, 256, 1154), (0, -1))]
BOUND_CLASSES = ("plain", "gelu", "gelu+deriv", "qgelu+deriv", "qgelu", "relu+deriv", "dgelu+res", "dqgelu", "dmul", "any:tanh+pre+res",
                 "any:gelu+drop")
DROP_P = 0.1


def bound_operands(M, N, K, seed, device="cpu"):
    """x ~ N(0, 1), w ~ N(0, 1 / K), both rounded to bf16; bias fp32, residual / aux / c_old ~ N(0, 1) (float64 holding bf16 values)."""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)
    bf = lambda t: t.to(torch.bfloat16).double()
    return dict(a=bf(rn(M, K)), b=bf(rn(N, K) * K ** -0.5), bias=rn(N), residual=bf(rn(M, N)), aux=bf(rn(M, N)), c_old=bf(rn(M, N)))


def bound_class(name, ops, keep, cast=lambda t: t):
    """reference() / model() keywords of a class of launch_nt (csrc/gemm_mfma.hip) from bound_operands' tensors."""
    bias, res, aux = ops["bias"].float(), cast(ops["residual"]), cast(ops["aux"])
    return {
        "plain": dict(alpha=0.75, bias=bias, residual=res),
        "gelu": dict(bias=bias, act=ACT_GELU, want_preact=True),
        "gelu+deriv": dict(bias=bias, act=ACT_GELU, want_preact=True, preact_grad=True),
        "qgelu": dict(bias=bias, act=ACT_QUICKGELU, residual=res),
        "qgelu+deriv": dict(bias=bias, act=ACT_QUICKGELU, want_preact=True, preact_grad=True),
        "relu+deriv": dict(bias=bias, act=ACT_RELU, want_preact=True, preact_grad=True, keep=keep, p=DROP_P, residual=res),
        "dgelu+res": dict(dact_aux=aux, dact=ACT_GELU, residual=res),
        "dqgelu": dict(alpha=0.5, dact_aux=aux, dact=ACT_QUICKGELU, c_old=cast(ops["c_old"])),
        "dmul": dict(alpha=1.5, dact_aux=aux, dact=ACT_MULAUX, keep=keep, p=DROP_P),
        "any:tanh+pre+res": dict(bias=bias, act=ACT_TANH, want_preact=True, residual=res),
        "any:gelu+drop": dict(bias=bias, act=ACT_GELU, keep=keep, p=DROP_P),
    }[name]


def host_keep(M, N, p, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.rand(M, N, generator=g, device=device) >= p).to(torch.uint8)
