"""Accuracy yardsticks of parity mode (compute_dtype="fp32"): gemm_generic_kernel (csrc/gemm_generic.hip) on fp32 and mixed operands,
and the materialised-softmax attention at the bottom of csrc/attention.hip (softmax_rows_kernel, softmax_bwd_rows_kernel,
pos_bias_grad_kernel and the seven batched products around them).  Shared by tests/test_gpu_parity_accuracy.py and its host-side
self-check tests/test_parity_accuracy_host.py.  Plain torch / numpy: nothing here imports or calls the library.  The float64
references, the exact-tier operands and the fences are those of tests/gemm_accuracy.py and tests/attn_accuracy.py.

GEMM
  A1 exact tier   integer-valued fp32 operands (gemm_accuracy.exact_operands): the output is known bit for bit in any order.
  A2 ascending k  operands with at most 12 significant bits (bf16-rounded normals): every product is exact in fp32, so
                  fmaf(a, b, acc) = fl(acc + a b) and seq_gemm() below IS the kernel, bit for bit; the sums still round, so any other
                  order of summation gives other bits.
  A3 bound tier   full-precision fp32 operands against float64.  Element-wise |got - ref| <= e with e from bound(): the epilogue walk
                  of gemm_accuracy.bound for an fp32 store with two changes, both because this kernel is not the MFMA one:
                    accumulation  gamma_K |alpha| (|A||B|)_mn, gamma_K = K U / (1 - K U), U = 2^-24: a sequential FMA chain has ONE
                                  rounding per term (the MFMA bound carries 2 K U for the instruction's internal order and split-K).
                    evaluation    act_fwd / act_bwd of csrc/common.h call libm (erff, expf, tanhf) and divide; the constants are the
                                  OpenCL C full-profile limits the ROCm device library is held to -- erf 16 ulp = 32 U, exp 3 ulp = 6 U,
                                  tanh 5 ulp = 10 U, division 2.5 ulp = 5 U:
                      GELU   0.5f x (1 + erff(x c)): c and the product round the argument twice, which moves erf by at most
                             erf'(z) z 2 U <= (2 / sqrt pi) max(z exp(-z^2)) 2 U = 0.97 U < U; erff 32 U |erf| <= 32 U; the add
                             U (1 + erf) <= 2 U: 35 U absolute on (1 + erf), DCDF = 17.5 U on the cdf; the product U |result|:
                                 eval = |x| DCDF + U |gelu(x)|
                      GELU'  cdf + x pdf, pdf = c2 expf(-0.5f x x): the argument t = x^2 / 2 rounds once (t U relative on the
                             exponential), expf 6 U, c2 and two products 3 U:  DCDF + |x| phi(x) (9 + x^2 / 2) U + U |result|
                      QuickGELU  x / (1 + expf(-1.702f x)): the constant and the product round the argument twice (3.404 |x| U
                             relative on E = exp(-1.702 x)), expf 6 U; the add U; relative to 1 + E the error of E weighs
                             E / (1 + E) = 1 - s; the division 5 U:   RS = ((1 - s)(6 + 3.404 |x|) + 6) U relative, eval = |x s| RS
                      QuickGELU' s g, s = 1 / (1 + E) (RS relative), g = 1 + (1.702f x)(1 - s): d(1 - s) = s RS + U (1 - s);
                             dg = 1.702 |x| (d(1 - s) + 3 U (1 - s)) + U |g|;   total |g| s RS + s dg + U |result|
                      tanh   10 U |t|;   tanh' = 1 - t^2: 20 U t^2 + U t^2 + U |result|;   ReLU and its step: exact.
                  Aggregate budgets from 10^4 elements on, against the error of the sequential model (seq_gemm + epilogue32):
                  rel_rms(got) <= 1.1 rel_rms(model), max_abs(got) <= 3 max_abs(model) -- the factors of tests/norm_accuracy.py.
                  The ReLU step is compared where |pre| > e; the excluded share is capped at KINK_SHARE.

Attention (q, o, dO, dq [B, Lq, H Dh]; k, v, dk, dv [B, Lk, H Dh]; any Dh)
  B1 probabilities, element by element.  Dh = Lk and V = I per head make o = P bit for bit (one non-zero term per product).
                  P_j = E_j / sum_i E_i with E_i = exp(x_i - max); a score error |d_i| <= e_i gives
                      P^_j / P_j = exp(d_j) / sum_i P_i exp(d_i)  in  [exp(-e_j) / sum_i P_i exp(e_i), exp(e_j) / sum_i P_i exp(-e_i)]
                  -- the P-weighted form of the row-maximum bound 2 e_s, which it never exceeds; keys at -inf carry e = 0, P = 0.
                  e_i: the A3 bound of the scores product (gamma_Dh |scale| (|q||k|) + 2 U |scale s|: the alpha multiply, and
                  the descriptor's fp32 scale against the reference's float64 one), + U |x| for the mask add, + U |x|
                  for the bias add, + U |x - max| for the subtraction in front of expf.  On top, (Lk + C_SOFTMAX) U relative from
                  the three loops of softmax_rows_kernel:  expf 6 U in the numerator and 6 U through the denominator, at most Lk - 1
                  rounded additions on any path of the lane sums and the wave reduction, the division 1.0f / sum 5 U, the multiply
                  U:  C_SOFTMAX = 6 + 6 - 1 + 5 + 1 = 17.  Dropout adds 2 U (inv_keep and the product).  One absolute term: 2^-126,
                  the smallest normal fp32 -- a probability below it (position bias of scale 30) may come out denormal or 0.
  B2 budget tier  o, dq, dk, dv, d_pos_bias against float64; yardstick: seq_attention(), torch / numpy float32 in the kernels'
                  order.  rel_rms(got) <= max(2 rel_rms(model), 2^-26), max_abs(got) <= 3 max_abs(model) per tensor (the form of
                  attn_accuracy.within_budget; the floor is a quarter of one fp32 rounding).
  B3 the bf16 detour (Dh != 64): float64 from the bf16-rounded inputs; e = the B2 max budget, one bf16 rounding on top:
                  |got - ref| <= hulp(|ref| + e) + e.

When a kernel misses a criterion it is wrong, or it rounds where the model does not: then that rounding goes into the model,
with the line that does it.  The factors stay."""
import math

import numpy as np
import torch

import attn_accuracy as aa
import gemm_accuracy as ga

U = ga.U
ERF_U, EXP_U, TANH_U, DIV_U = 32 * U, 6 * U, 10 * U, 5 * U
DCDF = (ERF_U + 3 * U) / 2   # 17.5 U: the argument (< U), erff, the add (2 U), halved
QG = 1.702
RMS_FACTOR, MAX_FACTOR = 1.1, 3.0              # A3 aggregates
ATTN_RMS_FACTOR, ATTN_MAX_FACTOR, ATTN_RMS_FLOOR = 2.0, 3.0, 2.0 ** -26
C_SOFTMAX = 17
KINK_SHARE = 1e-3
TINY = 2.0 ** -126         # the smallest normal fp32: a probability below it may come out denormal or 0 (absolute term of B1)
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------
# GEMM: fp32 models
# ------------------------------------------------------------------------------------------------------------------------
def _np32(t):
    return t.detach().cpu().to(torch.float32).numpy()


def seq_gemm(a, b, order="ascending"):
    """a [..., M, K] . b [..., K, N] as gemm_generic_kernel forms it: acc = fmaf(a_k, b_k, acc) for k = 0 .. K - 1 (the product of two
    fp32 values is exact in float64; the float64 sum is rounded to fp32).  order: "descending" and "drop_last_k" are mutants,
    "pairwise" the differently ordered second model (halves down to runs of 8)."""
    a, b = _np32(a).astype(np.float64), _np32(b).astype(np.float64)
    K = a.shape[-1]

    def run(ks):
        acc = np.zeros(np.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (a.shape[-2], b.shape[-1]), dtype=f32)
        for k in ks:
            acc = (acc.astype(np.float64) + a[..., :, k, None] * b[..., k, None, :]).astype(f32)
        return acc

    def pair(lo, hi):
        if hi - lo <= 8:
            return run(range(lo, hi))
        mid = (lo + hi) // 2
        return (pair(lo, mid) + pair(mid, hi)).astype(f32)

    if order == "pairwise":
        return torch.from_numpy(pair(0, K))
    ks = {"ascending": range(K), "descending": range(K - 1, -1, -1), "drop_last_k": range(K - 1)}[order]
    return torch.from_numpy(run(ks))


def act32(x, act):
    """act_fwd of csrc/common.h in fp32 torch."""
    if act == ga.ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))
    if act == ga.ACT_QUICKGELU:
        return x / (1.0 + torch.exp(-QG * x))
    if act == ga.ACT_TANH:
        return torch.tanh(x)
    if act == ga.ACT_RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    return x


def act32_grad(x, act):
    """act_bwd of csrc/common.h in fp32 torch."""
    if act == ga.ACT_GELU:
        cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440))
        return cdf + x * (0.39894228040143267794 * torch.exp(-0.5 * x * x))
    if act == ga.ACT_QUICKGELU:
        s = 1.0 / (1.0 + torch.exp(-QG * x))
        return s * (1.0 + QG * x * (1.0 - s))
    if act == ga.ACT_TANH:
        t = torch.tanh(x)
        return 1.0 - t * t
    if act == ga.ACT_RELU:
        return (x > 0).to(x.dtype)
    if act == ga.ACT_MULAUX:
        return x
    return torch.ones_like(x)


GEMM_MUTANTS = ("drop_last_k", "descending_k", "bias_shift_one_column", "residual_after_dact", "rowsum_overwritten",
                "rowsum_per_column_block", "batch_levels_swapped")


def epilogue32(acc, *, alpha=1.0, bias=None, act=ga.ACT_NONE, want_preact=False, preact_grad=False, keep=None, p=0.0, residual=None,
               dact_aux=None, dact=ga.ACT_NONE, c_old=None, mutant=None):
    """The epilogue of gemm_generic_kernel on an fp32 accumulator, in its order, every operation in fp32: (c, preact)."""
    assert mutant is None or mutant in GEMM_MUTANTS
    t = torch.float32
    x = acc.to(t) * torch.tensor(alpha, dtype=t)
    if bias is not None:
        bb = bias.to(t)
        x = x + (torch.roll(bb, -1) if mutant == "bias_shift_one_column" else bb)
    preact = (act32_grad(x, act) if preact_grad else x.clone()) if want_preact else None
    x = act32(x, act)
    if keep is not None:
        inv = torch.tensor(1.0, dtype=t) / (torch.tensor(1.0, dtype=t) - torch.tensor(p, dtype=t))
        x = torch.where(keep.to(torch.bool), x * inv, torch.zeros_like(x))
    late = mutant == "residual_after_dact" and residual is not None and dact_aux is not None
    if residual is not None and not late:
        x = x + residual.to(t)
    if dact_aux is not None:
        x = x * act32_grad(dact_aux.to(t), dact)
    if late:
        x = x + residual.to(t)
    if c_old is not None:
        x = x + c_old.to(t)
    return x, preact


def gemm_model(a, b, order="ascending", mutant=None, **kw):
    """a [M, K], b [N, K] (gemm_accuracy's layouts) -> (c, preact) of the sequential fp32 model, or of one of its mutants."""
    order = {"drop_last_k": "drop_last_k", "descending_k": "descending"}.get(mutant, order)
    return epilogue32(seq_gemm(a, b.transpose(-1, -2), order), mutant=mutant, **kw)


def rowsum_model(a, prior, n_col_blocks=1, mutant=None):
    """a_rowsum of the kernel: the thread tx == 0 of column block 0 sums its row's A values in ascending k and adds the sum onto the
    prior contents."""
    a = _np32(a)
    rs = np.zeros(a.shape[0], dtype=f32)
    for k in range(a.shape[1]):
        rs = (rs + a[:, k]).astype(f32)
    rs = torch.from_numpy(rs)
    if mutant == "rowsum_overwritten":
        return rs
    if mutant == "rowsum_per_column_block":
        return prior.float() + rs * n_col_blocks
    return prior.float() + rs


def batched_reference(a4, b4, swapped=False):
    """float64 a4 [b1, b2, M, K] . b4 [b1, b2, K, N] (a size-1 level broadcasts: the zero batch stride).  swapped: the mutant that
    takes the two levels the other way round for C alone (the product of batch z lands where batch (z % b1) b2 + z / b1 belongs)."""
    a4, b4 = a4.double(), b4.double()
    out = a4 @ b4
    if swapped:
        b1, b2 = out.shape[:2]
        flat = out.reshape(b1 * b2, *out.shape[2:])
        idx = torch.tensor([(z % b1) * b2 + z // b1 for z in range(b1 * b2)])
        out = flat[idx].reshape(out.shape)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# GEMM: the element-wise bound of an fp32 store
# ------------------------------------------------------------------------------------------------------------------------
def _eval_act(x, act):
    ax = x.abs()
    if act == ga.ACT_GELU:
        return ax * DCDF + U * ga.act_value(x, act).abs()
    if act == ga.ACT_QUICKGELU:
        s = torch.sigmoid(QG * x)
        return (x * s).abs() * ((1.0 - s) * (EXP_U + 2 * QG * ax * U) + U + DIV_U)
    if act == ga.ACT_TANH:
        return TANH_U * torch.tanh(x).abs()
    return torch.zeros_like(x)


def _eval_grad(x, act):
    ax = x.abs()
    d = ga.act_grad(x, act).abs()
    if act == ga.ACT_GELU:
        return DCDF + ax * ga._phi(x) * (9 + 0.5 * x * x) * U + U * d
    if act == ga.ACT_QUICKGELU:
        s = torch.sigmoid(QG * x)
        rs = (1.0 - s) * (EXP_U + 2 * QG * ax * U) + U + DIV_U
        g = (1.0 + QG * x * (1.0 - s)).abs()
        d1s = s * rs + U * (1.0 - s)
        dg = QG * ax * (d1s + 3 * U * (1.0 - s)) + U * g
        return g * s * rs + s * dg + U * d
    if act == ga.ACT_TANH:
        t2 = torch.tanh(x) ** 2
        return 2 * TANH_U * t2 + U * t2 + U * d
    return torch.zeros_like(x)


def gamma(K):
    return K * U / (1.0 - K * U)


def bound(ref):
    """(c_bound, preact_bound) on |got - ref| of an fp32-store call of the generic kernel whose float64 result is `ref`
    (gemm_accuracy.reference's Ref).  Module docstring; the walk is gemm_accuracy.bound's."""
    m = ref.mags
    K, alpha, act = m["K"], abs(m["alpha"]), m["act"]
    e = gamma(K) * alpha * ref.absprod + U * m["acc"].abs()
    if "bias" in m:
        e = e + U * m["bias"].abs()
    pre_bound = None
    if ref.preact is not None:
        if not m["preact_grad"]:
            pre_bound = e
        elif act == ga.ACT_RELU:
            pre_bound = torch.where(m["pre"].abs() <= e, torch.ones_like(e), torch.zeros_like(e))
        else:
            pre_bound = ga.LIP2.get(act, 0.0) * e + _eval_grad(m["pre"], act)
    e = ga.LIP[act] * e + _eval_act(m["pre"], act)
    if "drop" in m:
        e = torch.where(m["keep"], e * m["inv_keep"] + 2 * U * m["drop"].abs(), torch.zeros_like(e))
    if "res" in m:
        e = e + U * m["res"].abs()
    if "dmul" in m:
        eg = _eval_grad(m["aux"], m["dact"]) if m["dact"] != ga.ACT_MULAUX else torch.zeros_like(e)
        e = e * m["g"].abs() + m["before_g"].abs() * eg + U * m["dmul"].abs()
    if "c_old" in m:
        e = e + U * ref.c.abs()
    return e, pre_bound


def kink_share(ref):
    """Share of the elements the ReLU-step comparison leaves out (|pre| <= e)."""
    return (bound(ref)[1] > 0).double().mean().item()


def check_aggregate(got, model, ref, figures=None, name="c"):
    """rel_rms(got) <= 1.1 rel_rms(model) and max_abs(got) <= 3 max_abs(model), from 10^4 elements on; None or the miss."""
    if ref.numel() < ga.MIN_AGGREGATE:
        return None
    rg, rm, mg, mm = aa.rel_rms(got, ref), aa.rel_rms(model, ref), aa.max_abs(got, ref), aa.max_abs(model, ref)
    if figures is not None:
        figures["rms"] = max(figures.get("rms", 0.0), rg / rm if rm else (0.0 if rg == 0 else math.inf))
        figures["max"] = max(figures.get("max", 0.0), mg / mm if mm else (0.0 if mg == 0 else math.inf))
    if not rg <= RMS_FACTOR * rm:
        return f"{name}: rel_rms {rg:.3e} over {RMS_FACTOR} x the sequential model's {rm:.3e}"
    if not mg <= MAX_FACTOR * mm:
        return f"{name}: max_abs {mg:.3e} over {MAX_FACTOR} x the sequential model's {mm:.3e}"
    return None


def gemm_criteria(got_c, got_pre, model_c, model_pre, ref, figures=None):
    """Every A3 criterion on the outputs of one call: list of misses, each beginning with the criterion's name."""
    cb, pb = bound(ref)
    out = []
    for name, got, mod, r, b in (("c", got_c, model_c, ref.c, cb), ("preact", got_pre, model_pre, ref.preact, pb)):
        if r is None:
            continue
        got, mod = got.detach().cpu(), mod.detach().cpu()
        r, b = r.cpu(), b.cpu()
        miss = ga.check_bound(got, r, b, figures, name)
        out.append("bound: " + miss if miss else None)
        if name == "preact" and ref.mags["preact_grad"] and ref.mags["act"] == ga.ACT_RELU:
            continue   # a step function: exact away from the kink (the bound above), no rounding error to budget
        miss = check_aggregate(got, mod, r, figures, name)
        out.append("aggregate: " + miss if miss else None)
    return [o for o in out if o]


# cases shared by the GPU tests and the host self-check
EXACT_SHAPES = [(1, 1, 1), (63, 65, 15), (64, 64, 16), (65, 63, 17), (33, 50, 72), (130, 129, 100), (5, 498, 33)]
LAYOUTS = ("NT", "NN", "TN", "TT", "S2")       # TT: both operands reduction-strided; S2: every-other-element views, no unit stride
EXACT_EXTRA_EPILOGUES = ("bias+relu+deriv", "bias+relu+pre+drop+res@rows")
ROW_MAP = (3, 2)                               # rows = (base, step) of the mapped dropout case
ASCENDING_CASES = [(70, 130, K) for K in (1, 15, 16, 17, 100)]
BOUND_SHAPES = [(130, 132, 64), (257, 136, 768), (17, 498, 1536)]
BOUND_CLASSES = ("plain", "gelu+pre", "qgelu+deriv", "relu+deriv", "tanh+res", "dgelu+res", "alpha+acc")
ROWSUM_SHAPES = [(33, 50, 72), (130, 129, 100), (5, 498, 33)]
BATCH = (2, 3)


def seed_of(shape):
    return 4000 + shape[0] + 7 * shape[1] + 13 * shape[2]


def exact_epilogue(name, ops, keep, cast=lambda t: t):
    """gemm_accuracy.exact_epilogue plus the two classes of this file."""
    if name == "bias+relu+deriv":
        return dict(alpha=ops["alpha"], bias=ops["bias"].float(), act=ga.ACT_RELU, want_preact=True, preact_grad=True)
    return ga.exact_epilogue(name.split("@")[0], ops, keep, cast)


def views(layout, A, B, fill=ga.FENCE):
    """Storage for op(A) [.., M, K] and op(B) [.., K, N] in a named layout: tensors of the same shapes and values whose last two strides
    are (K, 1) / (1, K)  NT,  (K, 1) / (N, 1)  NN,  (1, M) / (N, 1)  TN,  (1, M) / (1, K)  TT,  (2K, 2) / (2N, 2)  S2 (the skipped
    elements hold the fence value)."""
    t = lambda x: x.transpose(-1, -2).contiguous().transpose(-1, -2)

    def every_other(x):
        buf = torch.full(x.shape[:-1] + (2 * x.shape[-1],), fill, dtype=x.dtype, device=x.device)
        buf[..., ::2] = x
        return buf[..., ::2]
    return {"NT": lambda: (A.contiguous(), t(B)), "NN": lambda: (A.contiguous(), B.contiguous()), "TN": lambda: (t(A), B.contiguous()),
            "TT": lambda: (t(A), t(B)), "S2": lambda: (every_other(A), every_other(B))}[layout]()


def twelve_bit_operands(M, N, K, seed, device="cpu"):
    """fp32 a [M, K], b [N, K] of bf16-rounded normals: at most 8 significant bits each, every product exact in fp32."""
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=device).to(torch.bfloat16).float()
    return r(M, K), r(N, K)


def probe_operands(device="cpu"):
    """[2^24, 1, -2^24] against ones: 0 in ascending order (2^24 + 1 rounds to 2^24), 1 in descending order."""
    a = torch.tensor([[2.0 ** 24, 1.0, -2.0 ** 24]], device=device).repeat(5, 1)
    return a, torch.ones(7, 3, device=device)


def bound_operands(M, N, K, seed, device="cpu"):
    """Full-precision fp32 values held in float64: x ~ N(0, 1), w ~ N(0, 1 / K), bias, residual, aux, c_old ~ N(0, 1)."""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device).double()
    return dict(a=rn(M, K), b=(torch.randn(N, K, generator=g, device=device) * K ** -0.5).double(), bias=rn(N).float(), residual=rn(M, N),
                aux=rn(M, N), c_old=rn(M, N))


def bound_class(name, o):
    bias, res, aux = o["bias"], o["residual"].float(), o["aux"].float()
    return {
        "plain": dict(),
        "gelu+pre": dict(bias=bias, act=ga.ACT_GELU, want_preact=True),
        "qgelu+deriv": dict(bias=bias, act=ga.ACT_QUICKGELU, want_preact=True, preact_grad=True),
        # (bias x 4: the step is compared where |pre| > e, and e reaches 2e-3 at K = 1536; with the pre-activations spread to a
        # standard deviation of 4 the share inside +-e stays under KINK_SHARE at every shape -- asserted on the host)
        "relu+deriv": dict(bias=4.0 * bias, act=ga.ACT_RELU, want_preact=True, preact_grad=True),
        "tanh+res": dict(bias=bias, act=ga.ACT_TANH, residual=res),
        "dgelu+res": dict(dact_aux=aux, dact=ga.ACT_GELU, residual=res),
        "alpha+acc": dict(alpha=0.375, c_old=o["c_old"].float()),
    }[name]


def gemm_mutant_applies(mutant, K, kw):
    has = lambda k: kw.get(k) is not None
    return {"drop_last_k": K % 16 != 0, "bias_shift_one_column": has("bias"),
            "residual_after_dact": has("residual") and has("dact_aux")}.get(mutant, False)


# ------------------------------------------------------------------------------------------------------------------------
# attention: inputs
# ------------------------------------------------------------------------------------------------------------------------
PAD_COLS = 8   # trailing columns of every packed buffer that belong to no operand


def packed_views(bufs, D):
    if len(bufs) == 1:
        return bufs[0][..., :D], bufs[0][..., D:2 * D], bufs[0][..., 2 * D:3 * D]
    return bufs[0][..., :D], bufs[1][..., :D], bufs[1][..., D:2 * D]


def make_case(B, H, Lq, Lk, Dh, seed, masked=False, bias=False, causal=False, bias_scale=1.0, p=0.0, drop_seed=0, dtype=torch.float32):
    """Inputs of one attention call on the CPU, in the layers' layouts with PAD_COLS spare columns: for Lq == Lk one packed
    [B, L, 3D + pad] projection (Q | K | V), else q [B, Lq, D + pad] and a packed [B, Lk, 2D + pad] (K | V); q, k, v are views.
    `keep` is left None: with p > 0 the caller stores the keep mask [B, H, Lq, Lk] there.  dpb_prior: what d_pos_bias holds before
    the call (the kernel adds)."""
    D = H * Dh
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g).to(dtype)
    bufs = (rn(B, Lq, 3 * D + PAD_COLS),) if Lq == Lk else (rn(B, Lq, D + PAD_COLS), rn(B, Lk, 2 * D + PAD_COLS))
    q, k, v = packed_views(bufs, D)
    return dict(bufs=bufs, q=q, k=k, v=v, do=rn(B, Lq, D), H=H, Dh=Dh, key_mask=aa.tail_key_mask(B, Lk) if masked else None,
                pos_bias=torch.randn(H, Lq, Lk, generator=g) * bias_scale if bias else None, causal=causal, scale=1.0 / math.sqrt(Dh),
                dpb_prior=torch.randn(H, Lq, Lk, generator=g) if bias else None, keep=None, p=p, drop_seed=drop_seed)


def grad_views(case, device=None):
    """Fence-filled buffers shaped like case["bufs"] and the dq, dk, dv views into them (the strides of q, k, v)."""
    bufs = tuple(torch.full(b.shape, ga.FENCE, dtype=b.dtype, device=device or b.device) for b in case["bufs"])
    return bufs, packed_views(bufs, case["H"] * case["Dh"])


def grads_fence_intact(bufs):
    """Nothing outside the dq, dk, dv views was written: the spare columns still hold the fence value."""
    return all(bool((b[..., -PAD_COLS:] == ga.FENCE).all()) for b in bufs)


def model_args(case):
    assert case["p"] == 0 or case["keep"] is not None
    return dict(q=case["q"], k=case["k"], v=case["v"], do=case["do"], H=case["H"], key_mask=case["key_mask"], pos_bias=case["pos_bias"],
                causal=case["causal"], scale=case["scale"], keep=case["keep"] if case["p"] > 0 else None, p=case["p"])


def identity_v(B, H, Lk):
    """v [B, Lk, H Lk] with V = I per head: o[b, i, h Lk + c] = P[b, h, i, c]."""
    return torch.eye(Lk).repeat(1, H)[None].repeat(B, 1, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------------
# attention: the sequential fp32 model, the second model, the mutants
# ------------------------------------------------------------------------------------------------------------------------
ATTN_MUTANTS = ("sum_misses_last_key", "no_max_subtraction", "mask_by_head", "bias_q_h", "causal_off_by_one", "dropout_no_rescale",
                "softmax_bwd_no_dot", "dk_no_scale", "dpb_overwritten", "dpb_sum_over_heads")


def attn_mutant_applies(mutant, B, H, Lq, Lk, masked, bias, causal, drop):
    # (the last key of a tail-masked sample, or one no causal query sees, has probability 0: leaving it out of the sum changes nothing)
    return {"sum_misses_last_key": Lk % 64 != 0 and not masked and (not causal or Lq >= Lk), "no_max_subtraction": bias, "mask_by_head": masked, "bias_q_h": bias,
            "causal_off_by_one": causal, "dropout_no_rescale": drop, "dpb_overwritten": bias, "dpb_sum_over_heads": bias}.get(mutant, True)


def _seq_sum(x, dim_len=None):
    """fp32 sum over the last axis in ascending index, one rounding per term."""
    x = x.numpy()
    acc = np.zeros(x.shape[:-1], dtype=f32)
    with np.errstate(over="ignore", invalid="ignore"):   # (the mutant without the max subtraction overflows, on purpose)
        for j in range(x.shape[-1] if dim_len is None else dim_len):
            acc = (acc + x[..., j]).astype(f32)
    return torch.from_numpy(acc)


def seq_probs(q, k, H, key_mask, pos_bias, causal, scale, mutant=None, torch_softmax=False):
    """Undropped probabilities [B, H, Lq, Lk] in the order of attn_f32_scores: scaled scores (the generic GEMM with alpha = scale), then
    softmax_rows_kernel's three loops -- mask add, bias add, causal -inf, max; expf(x - max) and its sum; multiply by 1.0f / sum."""
    t = torch.float32
    qh, kh = aa.split(q, H).to(t), aa.split(k, H).to(t)
    B, _, Lq, _ = qh.shape
    Lk = kh.shape[2]
    if torch_softmax:
        x = (qh @ kh.transpose(-1, -2)) * scale
    else:
        x = seq_gemm(qh, kh.transpose(-1, -2)) * torch.tensor(scale, dtype=t)
    if key_mask is not None:
        km = key_mask.to(t)
        x = x + (km[torch.arange(H) % B][None, :, None, :] if mutant == "mask_by_head" else km[:, None, None, :])
    if pos_bias is not None:
        pb = pos_bias.to(t)
        if mutant == "bias_q_h":   # the row pointer (q H + h) Lk into the [H, Lq, Lk] table
            idx = torch.arange(Lq)[None, :] * H + torch.arange(H)[:, None]
            pb = pb.reshape(H * Lq, Lk)[idx]
        x = x + pb[None]
    if causal:
        x = x.masked_fill(~aa._visible(Lq, Lk, strict=mutant == "causal_off_by_one"), -math.inf)
    if torch_softmax:
        return torch.softmax(x, dim=-1)
    mx = torch.zeros_like(x[..., :1]) if mutant == "no_max_subtraction" else x.amax(-1, keepdim=True)
    e = torch.exp(x - mx)
    s = _seq_sum(e, Lk - 1 if mutant == "sum_misses_last_key" and Lk > 1 else None)[..., None]
    return e * (torch.tensor(1.0, dtype=t) / s)


def seq_attention(q, k, v, do, H, key_mask=None, pos_bias=None, causal=False, scale=None, keep=None, p=0.0, dpb_prior=None, mutant=None,
                  second=False):
    """The fp32 path of m3ae_attn_fwd / m3ae_attn_bwd in torch / numpy float32, in its order: probabilities (seq_probs), dropout
    (x * fl(1 / (1 - p)) or 0), and the products through seq_gemm: O = P V, dP = dO V^T, dV = P^T dO, [dropout of dP],
    softmax_bwd_rows_kernel (dot = sum_j P dP, dS = P (dP - dot)), pos_bias_grad_kernel (prior + sum_b dS),
    dQ = scale (dS K), dK = scale (dS^T Q).  second: the differently ordered model -- torch's softmax and torch's matmul.
    Returns attn_accuracy.Result; d_pos_bias includes dpb_prior."""
    assert mutant is None or mutant in ATTN_MUTANTS
    t = torch.float32
    mm = (lambda a, b: a @ b) if second else (lambda a, b: seq_gemm(a, b))
    P0 = seq_probs(q, k, H, key_mask, pos_bias, causal, scale, mutant, torch_softmax=second)
    qh, kh, vh, doh = (aa.split(x, H).to(t) for x in (q, k, v, do))
    if keep is not None:
        inv = torch.tensor(1.0, dtype=t) / (torch.tensor(1.0, dtype=t) - torch.tensor(p, dtype=t))
        mul = keep.to(t) if mutant == "dropout_no_rescale" else keep.to(t) * inv
    drop = (lambda x: x * mul) if keep is not None else (lambda x: x)
    P = drop(P0)
    o = mm(P, vh)
    dP = drop(mm(doh, vh.transpose(-1, -2)))
    dv = mm(P.transpose(-1, -2), doh)
    dot = (P0 * dP).sum(-1, keepdim=True) if second else _seq_sum(P0 * dP)[..., None]
    dS = P0 * dP if mutant == "softmax_bwd_no_dot" else P0 * (dP - dot)
    sc = torch.tensor(scale, dtype=t)
    dq = mm(dS, kh) * sc
    dk = mm(dS.transpose(-1, -2), qh) * (1.0 if mutant == "dk_no_scale" else sc)
    dpb = None
    if pos_bias is not None:
        if mutant == "dpb_sum_over_heads":   # the sample stride H Lq Lk taken as Lq Lk: entry h sums the planes h .. h + B - 1
            flat = dS.reshape(-1, *dS.shape[2:])
            acc = sum(flat[b:b + H] for b in range(dS.shape[0]))
        else:
            acc = dS.sum(0) if second else _seq_sum(dS.permute(1, 2, 3, 0).contiguous())
        prior = torch.zeros_like(acc) if dpb_prior is None or mutant == "dpb_overwritten" else dpb_prior.to(t)
        dpb = prior + acc
    return aa.Result(aa.merge(o), aa.merge(dq), aa.merge(dk), aa.merge(dv), dpb, P)


def attn_reference(case):
    """attn_accuracy.reference_parts in float64 from the inputs as given; d_pos_bias includes the prior contents."""
    parts = aa.reference_parts(**model_args(case))
    if parts["d_pos_bias"] is not None and case["dpb_prior"] is not None:
        parts["d_pos_bias"] = parts["d_pos_bias"] + case["dpb_prior"].double()
    return parts, aa.Result(*(parts[n] for n in aa.Result._fields))


def within_budget(got, model, ref):
    """(ok, (rel_rms got, rel_rms model, max_abs got, max_abs model)) of one tensor: the B2 criterion."""
    rg, rm, mg, mm = aa.rel_rms(got, ref), aa.rel_rms(model, ref), aa.max_abs(got, ref), aa.max_abs(model, ref)
    return bool(rg <= max(ATTN_RMS_FACTOR * rm, ATTN_RMS_FLOOR) and mg <= ATTN_MAX_FACTOR * mm), (rg, rm, mg, mm)


def budget_misses(got, model, ref, figures=None, names=aa.NAMES):
    """Names of the tensors of `got` (a Result) that miss within_budget."""
    bad = []
    for n in names:
        r = getattr(ref, n)
        if r is None:
            continue
        ok, fig = within_budget(getattr(got, n), getattr(model, n), r)
        if figures is not None:
            figures.setdefault(n, []).append(fig)
        if not ok:
            bad.append(f"budget: {n} rel_rms {fig[0]:.3e} (model {fig[1]:.3e}) max_abs {fig[2]:.3e} (model {fig[3]:.3e})")
    return bad


# ------------------------------------------------------------------------------------------------------------------------
# attention: B1, the probabilities element by element
# ------------------------------------------------------------------------------------------------------------------------
def probs_bound(q, k, H, key_mask, pos_bias, causal, scale, drop=False):
    """(P64 undropped [B, H, Lq, Lk], rel): |P - P64| <= rel P64 for the fp32 path's undropped probabilities (module docstring);
    with drop the survivors carry 2 U more."""
    dt = torch.float64
    qh, kh = aa.split(q, H).to(dt), aa.split(k, H).to(dt)
    s = (qh @ kh.transpose(-1, -2)) * scale
    # (the second U |s|: the descriptor holds fl32(scale), the reference the float64 value)
    e = gamma(qh.shape[-1]) * abs(scale) * (qh.abs() @ kh.abs().transpose(-1, -2)) + 2 * U * s.abs()
    x = s
    if key_mask is not None:
        x = x + key_mask.to(dt)[:, None, None, :]
        e = e + U * x.abs()
    if pos_bias is not None:
        x = x + pos_bias.to(dt)[None]
        e = e + U * x.abs()
    if causal:
        x = x.masked_fill(~aa._visible(x.shape[-2], x.shape[-1]), -math.inf)
    live = torch.isfinite(x)
    mx = x.amax(-1, keepdim=True)
    e = torch.where(live, e + U * (x - mx).abs(), torch.zeros_like(e))
    P = torch.softmax(x, dim=-1)
    hi = torch.exp(e) / (P * torch.exp(-e)).sum(-1, keepdim=True) - 1.0
    lo = 1.0 - torch.exp(-e) / (P * torch.exp(e)).sum(-1, keepdim=True)
    rel = torch.maximum(hi, lo) + (x.shape[-1] + C_SOFTMAX + (2 if drop else 0)) * U
    return P, rel


def check_probs(got, P64, rel, keep=None, p=0.0, name="P"):
    """None, or the miss: every probability within rel P64 of the float64 softmax (dropped: exact zeros, survivors P64 / (1 - p));
    exact zeros wherever P64 is 0."""
    got = got.detach().cpu().double()
    want = P64 if keep is None else P64 * keep.double() / (1.0 - p)
    if not torch.isfinite(got).all():
        return f"probs: {name} not finite"
    zero = want == 0
    if not bool((got[zero] == 0).all()):
        return f"probs: {name} non-zero where the reference is exactly 0 (masked, causal or dropped): {int((got[zero] != 0).sum())} entries"
    err, bnd = (got - want).abs(), rel * want + TINY / (1.0 - p)
    if bool((err > bnd).any()):
        worst = (err / torch.where(zero, torch.ones_like(bnd), bnd))[~zero].max().item()
        idx = torch.nonzero(err > bnd)[0].tolist()
        return f"probs: {name} over the relative bound, worst err / bound {worst:.2f}, first bad (b, h, q, k) = {idx}"
    return None


def worst_ratio(got, P64, rel, keep=None, p=0.0):
    got = got.detach().cpu().double()
    want = P64 if keep is None else P64 * keep.double() / (1.0 - p)
    nz = want > 0
    return ((got - want).abs()[nz] / (rel * want + TINY / (1.0 - p))[nz]).max().item() if nz.any() else 0.0


PROBE_SHAPES = [(5, 1), (3, 2), (33, 63), (2, 64), (5, 65), (1, 127), (33, 129), (33, 2)]     # (Lq, Lk): every Lk and Lq of the tier
PROBE_VARIANTS = ("plain", "tail_mask", "all_masked_row", "inf_mask", "bias1", "bias30", "causal", "dropout", "dropout_rows")
PROBE_P = 0.1


def probe_case(B, H, Lq, Lk, variant, seed):
    """q [B, Lq, H Lk], k [B, Lk, H Lk] (Dh = Lk), mask / bias / causal of a named B1 variant."""
    g = torch.Generator().manual_seed(seed)
    D = H * Lk
    q, k = torch.randn(B, Lq, D, generator=g), torch.randn(B, Lk, D, generator=g)
    mask = pos_bias = None
    if variant == "tail_mask":        # one sample only
        mask = torch.zeros(B, Lk)
        mask[1, Lk // 2:] = -10000.0
    elif variant == "all_masked_row":
        mask = torch.zeros(B, Lk)
        mask[0, :] = -10000.0
    elif variant == "inf_mask" and Lk > 1:   # some keys of a row, never all of them
        mask = torch.zeros(B, Lk)
        mask[0, Lk - 1] = -math.inf
        mask[1, 0::2] = -math.inf
    elif variant in ("bias1", "bias30"):
        pos_bias = torch.randn(H, Lq, Lk, generator=g) * (30.0 if variant == "bias30" else 1.0)
        if variant == "bias30":   # query 0 of every head: a score beyond expf's overflow at 88.7 -- only the max subtraction keeps it finite
            pos_bias[:, 0, 0] = 100.0
    return dict(q=q, k=k, H=H, key_mask=mask, pos_bias=pos_bias, causal=variant == "causal", scale=1.0 / math.sqrt(Lk))


# B2 cases: (label, Lq, Lk, Dh, make_case keywords)
def budget_cases():
    out = []
    for flags in range(8):
        out.append((f"flags{flags}-33x65-d96", 33, 65, 96, dict(masked=bool(flags & 1), bias=bool(flags & 2), causal=bool(flags & 4))))
    for i, (Lq, Lk) in enumerate([(33, 65), (100, 45), (1, 70), (5, 1), (129, 64)]):
        for Dh in (64, 96, 17):
            if (Lq, Lk, Dh) != (33, 65, 96):
                out.append((f"mask+bias-{Lq}x{Lk}-d{Dh}", Lq, Lk, Dh, dict(masked=True, bias=True, causal=(i + Dh) % 2 == 1)))
    out.append(("packed-qkv-33x33-d17", 33, 33, 17, dict(bias=True, causal=True)))
    out.append(("dropout+bias-33x65-d64", 33, 65, 64, dict(bias=True, p=0.1, drop_seed=0xA77E)))
    out.append(("dropout-100x45-d17", 100, 45, 17, dict(masked=True, p=0.1, drop_seed=0xA77F)))
    return out


def detour_bound(ref, model32, name):
    """B3: e = the B2 max budget of the fp32 path (3 max_abs of the sequential model on the same values); a bf16 output carries one
    rounding on top, the fp32 d_pos_bias none."""
    r = getattr(ref, name).double()
    e = ATTN_MAX_FACTOR * aa.max_abs(getattr(model32, name), r)
    return torch.full_like(r, e) if name == "d_pos_bias" else ga.hulp(r.abs() + e) + e
