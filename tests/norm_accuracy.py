"""Accuracy yardsticks of the row-statistics kernels (csrc/norm.hip: LayerNorm / RMSNorm forward and backward in all their forms) and
of the loss kernels of csrc/misc.hip (cross entropy, BCE with logits), shared by tests/test_gpu_norm_accuracy.py and its host-side
self-check tests/test_norm_accuracy_host.py.  numpy / torch only: nothing here imports or calls the library.  U, rne_bf16, hulp,
_store_bound, the fences and the activation helpers are those of tests/gemm_accuracy.py.

References: float64, from the exact fp32 / bf16 values the kernel reads.  The backward reads the SAVED fp32 mean / rstd: they are
inputs of its reference, not recomputed.

Element-wise bound, first order in u = U = 2^-24 (one fp32 rounding), valid for ANY summation order: an n-term fp32 sum of terms
t_i is within n u sum|t_i| of the exact sum.  n = D below; [x] marks the kernel's value of x, e_x a bound on |[x] - x|.

  forward   mean   [mean] = fl(fl(sum x) / n):                          e_mean = u sum|x| + u |mean|            (RMS: mean = 0, exact)
            d_i    = x_i - [mean], one rounding:                        e_d    = e_mean + u |d_i|               (RMS: d = x, exact)
            q      = sum d_i^2.  sum_i (x_i - [mean])^2 = q + n (mean - [mean])^2 EXACTLY (the cross term vanishes): the mean's
                   error enters the variance in second order only, but at |mean| / std = 256 that term is as large as the
                   first-order ones and is kept.  Each [d_i]^2 carries 3 roundings, the sum n more:
                                                                        e_q    = (n + 3) u (q + n e_mean^2) + n e_mean^2
            var    = q / n:  e_var = e_q / n + u var;   v = var + eps:  e_v    = e_var + u v
            rstd   = 1 / sqrt(v), both operations within 1 ulp = 2 u:   e_rstd = rstd (e_v / (2 (v - e_v)) + 4 u)  (inf if e_v >= v)
            h_i    = d_i rstd:                                          e_h    = e_d rstd + |d_i| e_rstd + e_d e_rstd + u |h_i|
            pre_i  = h_i g_i + b_i (2 roundings, fewer when contracted): e_pre  = e_h |g_i| + u |h_i g_i| + u |pre_i|
            y_i    = act(pre_i):  e_y = LIP[act] e_pre + eval(act, pre_i)   (gemm_accuracy: AS_CDF / DCDF / TANH_ULPS; norm.hip
                   calls erff / tanhf, whose error is below the documented figures of the fast forms)
            store  _store_bound(y, e_y, bf16).   mean and rstd are fp32 stores: e_mean, e_rstd.
  backward  h_i    = (x_i - mean) rstd from the saved statistics:       e_h    = 2 u |h_i|
            a_i    = act'(h_i g_i + b_i) (ACT form only, else 1):       e_a    = LIP2[act] (e_h |g_i| + u |h_i g_i| + u |pre_i|) + eval'(act, pre_i)
            dd_i   = dy_i a_i:  e_dd = |dy_i| e_a + u |dd_i|;   dh_i = dd_i g_i:   e_dh = e_dd |g_i| + u |dh_i|   (plain: e_dd = 0)
            c1     = sum dh / n:   e_c1 = (sum e_dh + n u sum|dh|) / n + u |c1|                                 (RMS: c1 = 0, exact)
            c2     = sum dh h / n: e_c2 = (sum (e_dh |h| + |dh| e_h + u |dh h|) + n u sum|dh h|) / n + u |c2|
            in_i   = dh_i - c1 - h_i c2:  e_in = e_dh + e_c1 + e_h |c2| + |h_i| e_c2 + u (|dh_i - c1| + |h_i c2| + |in_i|)
            dx_i   = rstd in_i (+ dx_add_i):  e_dx = rstd e_in + u |rstd in_i| (+ u |dx_i|);  store _store_bound.
            dx_drop_i = keep_i rstd in_i inv_keep, inv_keep = fl(1 / fl(1 - p)): (rstd e_in + u |rstd in_i|) / (1 - p) + 4 u |dx_drop_i|
            dgamma_j = sum over M rows of dd h:  sum (|dd| e_h + e_dd |h|) + M u sum|dd h|  (the form of
                   tests/test_gpu_clip_residual.py, extended by sum|dy| e_h);   dbeta_j = sum dd:  sum e_dd + M u sum|dd|.
                   (Wave partials, the LDS combine, the partial rows and the fold -- atomic or ordered -- are one sum of M terms in
                   some order.)

Aggregate yardstick.  The worst-case bound is about 100 x looser than real fp32 sums (1.2e-2 std at mean 64, D = 768), so the
kernel is also held against two numpy fp32 models of the same centred arithmetic: sums taken pairwise (a binary tree) and sums taken
strictly sequentially, the least accurate order a correct kernel could use.  Per output tensor of at least MIN_AGGREGATE elements
    rms(got - ref) <= RMS_FACTOR rms(sequential model - ref)     (RMS_FACTOR = 1.1 of gemm_accuracy)
    max|got - ref| <= MAX_FACTOR max|sequential model - ref|     (MAX_FACTOR = 3 of attn_accuracy)
Exact tier: a row equal to one small integer has exact sums, mean and a variance of exactly 0: y = beta bit for bit (rne_bf16(beta)
for bf16 rows) and rstd = 1 / sqrt(eps) within the fp32 rounding of that expression (4 u relative).  A row of +-1 in equal numbers
has mean 0 and variance 1 exactly and, at eps = 1e-12, rstd = 1: y = +-gamma + beta exactly, chosen to sit on bf16 ties, which is
what tells round-half-even from round-half-up.

Losses (float64 references xent_reference / bce_reference; bounds xent_bound / bce_bound), EXP = 4 u = 2 ulp for expf / logf /
log1pf:
  cross entropy  t_j = exp(x_j - max): e_t = t_j (u |x_j - max| + EXP);  s = sum t: e_s = sum e_t + C u s;  lse = max + log s:
                 e_lse = e_s / s + EXP |log s| + u |lse|;  row loss (lse - x_lab) / valid: (e_lse + u |lse - x_lab|) / valid +
                 2 u |row loss|;  loss: sum of the row bounds + rows u sum|row loss| (the atomic or ordered sum).
                 gradient p_j = exp(x_j - lse): e_p = p_j (e_lse + u |x_j - lse| + EXP);  g_j = (p_j - [j = label]) scale / valid:
                 (e_p + u |p_j - 1_j|) scale / valid + 3 u |g_j|, then the store.
  BCE            term = max(x, 0) - x z + log1p(exp(-|x|)) >= 0 for z in [0, 1]: e_term = u |x z| + u |max(x, 0) - x z| + 2 EXP sp + u term,
                 sp = log1p(exp(-|x|));  loss = sum term C / n (the scaling of ops.bce_with_logits_loss: the mean times C):
                 (sum e_term + n u sum term) C / n + (3 + n / 64) u loss (the products and one atomic per wave).
                 gradient sig = 1 / (1 + exp(-x)): e_sig = (EXP + 3 u) sig + 2^-126 (flush to zero);  g = (sig - z) C scale / n:
                 (e_sig + u |sig - z|) C scale / n + 4 u |g|, then the store.  Where the sigmoid saturates (|x| >= 100: exp(-|x|) is
                 0 in fp32) e_sig is 2^-126 alone: the gradient is (0 or 1 - z) C scale / n within the arithmetic's own 5 u and the store's
                 one rounding.

Measured headroom (tests/test_norm_accuracy_host.py prints it): over every case of CASES the worst model / bound ratio is 0.998 for
the pairwise model and 0.998 for the sequential one, both at bf16 stores, where a value next to a tie spends the whole store
rounding the bound grants; over the fp32 cases alone it is 0.25 (pairwise) and 0.23 (sequential), reached at D = 4, where the sums are
shortest and the bound is least pessimistic, and below 0.05 from D = 512 on.  The pairwise model reaches at most 1.00 x the sequential
model's rms and 1.45 x its max."""
import math

import numpy as np
import torch

import gemm_accuracy as ga
from attn_accuracy import MAX_FACTOR
from gemm_accuracy import (ACT_GELU, ACT_NONE, FENCE, LIP, LIP2, MIN_AGGREGATE, RMS_FACTOR, U, _eval_act, _eval_grad, _store_bound,  # noqa: F401
                           act_grad, act_value, assert_fence_intact, bf16_half_up, bf16_truncate, fenced, hulp, rne_bf16)

F64 = torch.float64
EXP = 4 * U
TINY = 2.0 ** -126
SWEEP_BWD = 4096          # rows of one sweep of the backward grid: m3ae_layernorm_bwd_blocks caps it at 1024 workgroups of 4 waves
SWEEP_FWD = 8 * 256 * 4   # forward: at most 8 resident workgroups of 4 rows on each of at most 256 CUs


def eps32(eps):
    return float(np.float32(eps))


def padded_d(D):
    """Elements the DISPATCH_CPL instantiation for D covers (CPL chunks of 4 elements on 64 lanes)."""
    cpl = -(-(D // 4) // 64)
    return next(c for c in (1, 2, 3, 4, 6, 8, 16) if cpl <= c) * 256


# ------------------------------------------------------------------------------------------------------------------------
# float64 references and bounds: LayerNorm / RMSNorm
# ------------------------------------------------------------------------------------------------------------------------
def ref_fwd(x, gamma, beta, eps, rms=False, act=ACT_NONE):
    """dict(y, mean, rstd) in float64 plus the magnitudes bound_fwd needs (keys starting with '_')."""
    x, g = x.to(F64), gamma.to(F64)
    b = beta.to(F64) if beta is not None else torch.zeros_like(g)
    n = x.shape[1]
    mean = torch.zeros(x.shape[0], dtype=F64, device=x.device) if rms else x.sum(1) / n
    d = x - mean[:, None]
    q = (d * d).sum(1)
    var = q / n
    v = var + eps32(eps)
    rstd = v.rsqrt()
    h = d * rstd[:, None]
    pre = h * g + b
    return dict(y=act_value(pre, act), mean=mean, rstd=rstd, _absx=x.abs().sum(1), _d=d, _q=q, _var=var, _v=v, _h=h, _pre=pre, _g=g,
                _n=n, _rms=rms, _act=act)


def bound_fwd(r, out_bf16):
    n, g = r["_n"], r["_g"]
    e_mean = torch.zeros_like(r["mean"]) if r["_rms"] else U * r["_absx"] + U * r["mean"].abs()
    e_d = torch.zeros_like(r["_d"]) if r["_rms"] else e_mean[:, None] + U * r["_d"].abs()
    e_q = (n + 3) * U * (r["_q"] + n * e_mean ** 2) + n * e_mean ** 2
    e_var = e_q / n + U * r["_var"]
    e_v = e_var + U * r["_v"]
    room = r["_v"] - e_v
    e_rstd = torch.where(room > 0, r["rstd"] * (e_v / (2 * room.clamp_min(1e-300)) + 4 * U), torch.full_like(room, math.inf))
    e_h = e_d * r["rstd"][:, None] + r["_d"].abs() * e_rstd[:, None] + e_d * e_rstd[:, None] + U * r["_h"].abs()
    e_pre = e_h * g.abs() + U * (r["_h"] * g).abs() + U * r["_pre"].abs()
    e_y = LIP[r["_act"]] * e_pre + _eval_act(r["_pre"], r["_act"])
    return dict(y=_store_bound(r["y"], e_y, out_bf16), mean=e_mean, rstd=e_rstd)


def ref_bwd(dy, x, gamma, beta, mean, rstd, rms=False, act=ACT_NONE, dx_add=None, keep=None, p=0.0):
    """dict(dx, dgamma, dbeta[, dx_drop]) in float64; mean / rstd: the saved fp32 statistics (mean ignored in RMS mode)."""
    dy, x, g = dy.to(F64), x.to(F64), gamma.to(F64)
    b = beta.to(F64) if beta is not None else torch.zeros_like(g)
    M, n = x.shape
    mu = torch.zeros(M, dtype=F64, device=x.device) if rms else mean.to(F64)
    rs = rstd.to(F64)[:, None]
    h = (x - mu[:, None]) * rs
    pre = h * g + b
    a = act_grad(pre, act) if act != ACT_NONE else torch.ones_like(h)
    dd = dy * a
    dh = dd * g
    c1 = torch.zeros(M, dtype=F64, device=x.device) if rms else dh.sum(1) / n
    c2 = (dh * h).sum(1) / n
    inner = dh - c1[:, None] - h * c2[:, None]
    o = rs * inner
    out = dict(dx=o if dx_add is None else o + dx_add.to(F64), dgamma=(dd * h).sum(0), dbeta=dd.sum(0), _o=o, _h=h, _pre=pre, _g=g, _dy=dy,
               _dd=dd, _dh=dh, _c1=c1, _c2=c2, _in=inner, _rs=rs, _n=n, _M=M, _act=act, _add=dx_add is not None, _p=p)
    out["dx_lo"] = out["dx"]   # the mixed form's second output: dx rounded to bf16 in the same pass
    if keep is not None:
        out["dx_drop"] = o * keep.to(F64) / (1.0 - p)
    return out


def bound_bwd(r, out_bf16):
    n, M, g, h, dh, act = r["_n"], r["_M"], r["_g"], r["_h"], r["_dh"], r["_act"]
    e_h = 2 * U * h.abs()
    if act != ACT_NONE:
        e_pre = e_h * g.abs() + U * (h * g).abs() + U * r["_pre"].abs()
        e_dd = r["_dy"].abs() * (LIP2[act] * e_pre + _eval_grad(r["_pre"], act)) + U * r["_dd"].abs()
    else:
        e_dd = torch.zeros_like(h)
    e_dh = e_dd * g.abs() + U * dh.abs()
    e_c1 = (e_dh.sum(1) + n * U * dh.abs().sum(1)) / n + U * r["_c1"].abs()
    e_c2 = ((e_dh * h.abs() + dh.abs() * e_h + U * (dh * h).abs()).sum(1) + n * U * (dh * h).abs().sum(1)) / n + U * r["_c2"].abs()
    c1, c2 = r["_c1"][:, None], r["_c2"][:, None]
    e_in = e_dh + e_c1[:, None] + e_h * c2.abs() + h.abs() * e_c2[:, None] + U * ((dh - c1).abs() + (h * c2).abs() + r["_in"].abs())
    e_o = r["_rs"] * e_in + U * r["_o"].abs()
    e_dx = e_o + U * r["dx"].abs() if r["_add"] else e_o
    out = dict(dx=_store_bound(r["dx"], e_dx, out_bf16), dx_lo=_store_bound(r["dx"], e_dx, True),
               dgamma=(r["_dd"].abs() * e_h + e_dd * h.abs()).sum(0) + M * U * (r["_dd"] * h).abs().sum(0),
               dbeta=e_dd.sum(0) + M * U * r["_dd"].abs().sum(0))
    if "dx_drop" in r:
        out["dx_drop"] = _store_bound(r["dx_drop"], e_o / (1.0 - r["_p"]) + 4 * U * r["dx_drop"].abs(), out_bf16)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# numpy fp32 models of a correct kernel (pairwise / strictly sequential sums) and the mutants
# ------------------------------------------------------------------------------------------------------------------------
f32 = np.float32
MUTANTS = ("one_pass_variance", "variance_over_d_minus_1", "eps_outside_sqrt", "mean_over_padded_chunks", "inactive_chunks_in_variance",
           "store_truncates", "store_half_up", "last_row_of_odd_m_dropped", "pair_second_row_with_first_rows_statistics", "c1_dropped",
           "c2_dropped", "dgamma_dbeta_miss_second_sweep", "beta_ignored_in_act_derivative", "rms_subtracts_mean", "dx_add_before_rstd")
FWD_MUTANTS = MUTANTS[:9] + ("rms_subtracts_mean",)


def sum_pair(a):
    """fp32 sum over the last axis as a binary tree."""
    a = np.ascontiguousarray(a, dtype=f32)
    while a.shape[-1] > 1:
        if a.shape[-1] & 1:
            a = np.concatenate([a, np.zeros(a.shape[:-1] + (1,), f32)], -1)
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def sum_seq(a):
    """fp32 sum over the last axis, one element after the other."""
    return np.cumsum(np.asarray(a, dtype=f32), axis=-1, dtype=f32)[..., -1]


SUMS = {"pair": sum_pair, "seq": sum_seq}


def np32(t):
    return None if t is None else np.ascontiguousarray(t.detach().float().cpu().numpy())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def act32(a, act, grad=False):
    """act_fwd / act_bwd of csrc/common.h in fp32 (torch's erff / expf)."""
    if act == ACT_NONE:
        return np.ones_like(a) if grad else a
    assert act == ACT_GELU
    t = _t(a)
    cdf = 0.5 * (1.0 + torch.erf(t * 0.70710678118654752440))
    if not grad:
        return (0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))).numpy()
    return (cdf + t * (0.39894228040143267794 * torch.exp(-0.5 * t * t))).numpy()


def store32(a, bf16, mutant=None):
    if not bf16:
        return a
    fn = {"store_truncates": bf16_truncate, "store_half_up": bf16_half_up}.get(mutant, rne_bf16)
    return fn(_t(a)).numpy()


def mutant_applies(mutant, case, part):
    """Whether `mutant` changes what the model computes for this case; part: 'fwd' or a backward variant (dict)."""
    M, D, bf = case["M"], case["D"], case["dtype"] != "f32"
    exact = case["inputs"] in ("const", "ties")
    if part == "fwd":
        return {
            "one_pass_variance": not case["rms"] and not exact,
            "variance_over_d_minus_1": case["inputs"] != "const",
            "eps_outside_sqrt": case["eps"] >= 1e-6 or case["inputs"] == "const",
            "mean_over_padded_chunks": padded_d(D) != D and not case["rms"] and case["inputs"] != "ties",
            "inactive_chunks_in_variance": padded_d(D) != D and not case["rms"] and case["inputs"] != "ties",
            "store_truncates": bf,
            "store_half_up": bf and case["inputs"] == "ties",
            "last_row_of_odd_m_dropped": M % 2 == 1,
            "pair_second_row_with_first_rows_statistics": M >= 2 and case["inputs"] != "ties",
            "rms_subtracts_mean": case["rms"],
        }.get(mutant, False)
    return {
        "store_truncates": case["dtype"] == "bf16",
        "c1_dropped": not case["rms"],
        "c2_dropped": True,
        "dgamma_dbeta_miss_second_sweep": M > SWEEP_BWD,
        "beta_ignored_in_act_derivative": case["act"] != ACT_NONE,
        "dx_add_before_rstd": bool(part.get("dx_add")),
    }.get(mutant, False)


def model_fwd(x, gamma, beta, eps, *, rms=False, act=ACT_NONE, out_bf16=False, order="seq", mutant=None):
    """dict(y, mean, rstd) as fp32 numpy arrays holding the stored values."""
    S = SUMS[order]
    x, g = np32(x), np32(gamma)
    b = np32(beta) if beta is not None else np.zeros_like(g)
    M, D = x.shape
    nd, pad = f32(D), padded_d(D)
    with np.errstate(all="ignore"):
        if rms and mutant != "rms_subtracts_mean":
            mean = np.zeros(M, f32)
        else:
            mean = S(x) / (f32(pad) if mutant == "mean_over_padded_chunks" else nd)

        def stats(mean):
            d = x - mean[:, None]
            if mutant == "one_pass_variance":
                var = S(x * x) / nd - mean * mean
            else:
                q = S(d * d)
                if mutant == "inactive_chunks_in_variance":
                    q = q + f32(pad - D) * (mean * mean)
                var = q / (f32(D - 1) if mutant == "variance_over_d_minus_1" else nd)
            e = f32(eps)
            rstd = f32(1) / (np.sqrt(var) + e) if mutant == "eps_outside_sqrt" else f32(1) / np.sqrt(var + e)
            return d, rstd.astype(f32)
        d, rstd = stats(mean)
        if mutant == "pair_second_row_with_first_rows_statistics":
            k = M // 2
            mean, rstd = mean.copy(), rstd.copy()
            mean[1:2 * k:2], rstd[1:2 * k:2] = mean[0:2 * k:2], rstd[0:2 * k:2]
            d = x - mean[:, None]
        y = store32(act32((d * rstd[:, None]) * g + b, act).astype(f32), out_bf16, mutant)
        if mutant == "last_row_of_odd_m_dropped" and M % 2 == 1:
            y, mean, rstd = y.copy(), mean.copy(), rstd.copy()
            y[-1], mean[-1], rstd[-1] = 0, 0, 0
    return dict(y=y, mean=mean, rstd=rstd)


def model_bwd(dy, x, gamma, beta, mean, rstd, *, rms=False, act=ACT_NONE, dx_add=None, keep=None, p=0.0, out_bf16=False, order="seq",
              mutant=None):
    """dict(dx, dgamma, dbeta[, dx_drop]) as fp32 numpy arrays."""
    S = SUMS[order]
    dy, x, g = np32(dy), np32(x), np32(gamma)
    b = np32(beta) if beta is not None else np.zeros_like(g)
    M, D = x.shape
    nd = f32(D)
    mu = np.zeros(M, f32) if rms else np32(mean)
    rs = np32(rstd)[:, None]
    with np.errstate(all="ignore"):
        h = (x - mu[:, None]) * rs
        dd = dy
        if act != ACT_NONE:
            dd = dy * act32(h * g + (0 if mutant == "beta_ignored_in_act_derivative" else b), act, grad=True).astype(f32)
        dh = dd * g
        c1 = np.zeros(M, f32) if (rms or mutant == "c1_dropped") else S(dh) / nd
        c2 = np.zeros(M, f32) if mutant == "c2_dropped" else S(dh * h) / nd
        inner = dh - c1[:, None] - h * c2[:, None]
        add = np32(dx_add)
        out = {}
        if add is not None and mutant == "dx_add_before_rstd":
            o = rs * (inner + add)
        else:
            o = rs * inner
            if keep is not None:
                inv = f32(1) / (f32(1) - f32(p))
                out["dx_drop"] = store32((o * np32(keep) * inv).astype(f32), out_bf16, mutant)
            if add is not None:
                o = o + add
        out["dx"] = store32(o.astype(f32), out_bf16, mutant)
        out["dx_lo"] = store32(o.astype(f32), True)
        tg, tb = dd * h, dd
        if mutant == "dgamma_dbeta_miss_second_sweep":
            tg, tb = tg.copy(), tb.copy()
            tg[SWEEP_BWD:2 * SWEEP_BWD], tb[SWEEP_BWD:2 * SWEEP_BWD] = 0, 0
        out["dgamma"], out["dbeta"] = S(tg.T), S(tb.T)
    return out


# ------------------------------------------------------------------------------------------------------------------------
# criteria
# ------------------------------------------------------------------------------------------------------------------------
def _d(a, device=None):
    t = _t(a) if isinstance(a, np.ndarray) else a
    return t.detach().to(device or t.device).to(F64)


def check_bound(got, ref, bnd, name, figures=None):
    got = _d(got, ref.device)
    if not torch.isfinite(got).all():
        return f"{name}: non-finite output ({int((~torch.isfinite(got)).sum())} of {got.numel()})"
    err = (got - ref).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    if figures is not None:
        figures["err/bound"] = max(figures.get("err/bound", 0.0), ratio.max().item())
    bad = err > bnd
    if bad.any():
        i = torch.nonzero(bad.reshape(-1))[0].item()
        where = (i // bad.shape[-1], i % bad.shape[-1]) if bad.dim() == 2 else (i,)
        return f"{name}: element-wise bound violated, worst err / bound {ratio.max().item():.3f}, first at {where}, {int(bad.sum())} of {bad.numel()} bad"
    return None


def _rms(e):
    return math.sqrt((e * e).mean().item())


def check_yardstick(got, seq, ref, name, figures=None):
    """rms and max error of `got` against those of the sequential model (tensors of at least MIN_AGGREGATE elements)."""
    if ref.numel() < MIN_AGGREGATE:
        return None
    eg, es = (_d(got, ref.device) - ref).abs(), (_d(seq, ref.device) - ref).abs()
    if not torch.isfinite(eg).all():
        return f"{name}: non-finite output"
    rg, rs_, mg, ms = _rms(eg), _rms(es), eg.max().item(), es.max().item()
    r_rms = rg / rs_ if rs_ > 0 else (0.0 if rg == 0 else math.inf)
    r_max = mg / ms if ms > 0 else (0.0 if mg == 0 else math.inf)
    if figures is not None:
        figures["rms/seq"] = max(figures.get("rms/seq", 0.0), r_rms)
        figures["max/seq"] = max(figures.get("max/seq", 0.0), r_max)
    if not r_rms <= RMS_FACTOR:
        return f"{name}: rms error {rg:.3e} = {r_rms:.3f} x the sequential model's {rs_:.3e}, budget {RMS_FACTOR}"
    if not r_max <= MAX_FACTOR:
        return f"{name}: max error {mg:.3e} = {r_max:.3f} x the sequential model's {ms:.3e}, budget {MAX_FACTOR}"
    return None


def criteria(got, ref, bnd, seq, names, figures=None, label=""):
    """Every criterion on the outputs `names` of one call; list of misses (empty = inside all of them).  got / seq: dicts of
    tensors or numpy arrays, ref / bnd: dicts of float64 tensors."""
    out = []
    for k in names:
        out.append(check_bound(got[k], ref[k], bnd[k], f"{label} {k}", figures))
        if seq is not None and out[-1] is None:
            out.append(check_yardstick(got[k], seq[k], ref[k], f"{label} {k}", figures))
    return [o for o in out if o]

def fwd_bf16(case):
    return case["dtype"] != "f32"


def bwd_bf16(case):
    return case["dtype"] == "bf16"


def fwd_names(case):
    return ("y", "rstd") if case["rms"] else ("y", "mean", "rstd")


def bwd_names(case, v):
    return ("dx", "dgamma") + (("dbeta",) if v.get("dbeta", True) else ()) + (("dx_drop",) if v.get("drop") else ()) + \
        (("dx_lo",) if v.get("lo") else ())


def fwd_misses(case, inp, got, seq=None, figures=None, device="cpu"):
    """Every criterion on the forward outputs of a case (the exact tier for 'const' / 'ties' inputs, whose bound is void: the
    variance is 0 or the result is known bit for bit)."""
    if case["inputs"] in ("const", "ties"):
        return [f"{case['name']} fwd: {m}" for m in exact_fwd_misses(case, inp, got)]
    to = lambda t: None if t is None else t.to(device)
    r = ref_fwd(to(inp["x"]), to(inp["gamma"]), to(inp["beta"]), case["eps"], case["rms"], case["act"])
    return criteria(got, r, bound_fwd(r, fwd_bf16(case)), seq, fwd_names(case), figures, case["name"] + " fwd")


def bwd_kw(case, inp, v, keep):
    return dict(rms=case["rms"], act=case["act"], dx_add=inp["dx_add"] if v.get("dx_add") else None, keep=keep,
                p=DROP_P if keep is not None else 0.0)


def bwd_misses(case, inp, v, mean, rstd, got, seq=None, keep=None, figures=None, device="cpu"):
    """The same for one backward variant; mean / rstd: the saved statistics the call read."""
    to = lambda t: None if t is None else t.to(device)
    kw = bwd_kw(case, inp, v, keep)
    r = ref_bwd(to(inp["dy"]), to(inp["x"]), to(inp["gamma"]), to(inp["beta"]), to(mean), to(rstd), kw["rms"], kw["act"], to(kw["dx_add"]),
                to(keep), kw["p"])
    return criteria(got, r, bound_bwd(r, bwd_bf16(case)), seq, bwd_names(case, v), figures, f"{case['name']} bwd {variant_tag(v)}")


def variant_tag(v):
    return "+".join(f"{k}={v[k]}" for k in sorted(v)) or "plain"


def exact_fwd_misses(case, inp, got):
    """The exact tier of a 'const' / 'ties' case: list of misses."""
    out, bf = [], case["dtype"] != "f32"
    y, dev = _d(got["y"]), None
    beta, gamma, x = inp["beta"].to(F64), inp["gamma"].to(F64), inp["x"].to(F64)
    dev = y.device
    if case["inputs"] == "const":
        want = beta.to(dev)[None, :].expand_as(y)
        target = 1.0 / math.sqrt(eps32(case["eps"]))
        rel = ((_d(got["rstd"]) - target).abs() / target).max().item()
        if not rel <= 4 * U:
            out.append(f"rstd of a constant row is {rel / U:.2f} u from 1 / sqrt(eps), allowed 4 u")
        if not torch.equal(_d(got["mean"]), x[:, 0].to(dev)):
            out.append("mean of a constant row is not that constant")
    else:
        want = (x * gamma + beta).to(dev)
        if not torch.equal(_d(got["rstd"]), torch.ones_like(_d(got["rstd"]))) or bool((_d(got["mean"]) != 0).any()):
            out.append("a +-1 row does not have mean 0 and rstd 1 exactly")
    want = rne_bf16(want) if bf else want
    if not torch.equal(y, want):
        out.append(f"y is not the exact result: {int((y != want).sum())} of {y.numel()} elements differ")
    return out


# ------------------------------------------------------------------------------------------------------------------------
# cases (shared by the host test and the GPU test) and their inputs
# ------------------------------------------------------------------------------------------------------------------------
def _case(name, M, D, dtype, inputs="normal", eps=1e-5, rms=False, act=ACT_NONE, bwd=({},), pair_off=False, offset8=False, beta=True,
          route=None):
    """dtype: 'f32' | 'bf16' | 'mixed' (fp32 rows, bf16 y / dy).  bwd: backward variants, each a dict of
    dx_add / dbeta (False: none) / drop ('plain' | 'rows') / det.  route: the forward kernel a bf16 case must take ('pair' | 'row')."""
    return dict(name=name, M=M, D=D, dtype=dtype, inputs=inputs, eps=eps, rms=rms, act=act, bwd=tuple(bwd), pair_off=pair_off,
                offset8=offset8, beta=beta and not rms, route=route)


SWEEP_D = (4, 128, 132, 256, 260, 512, 516, 768, 772, 1024, 1028, 1300, 1536, 1540, 2048)
FWD_ONLY_D = (2052, 4096)
REFUSED_D = (130, 4100)
DROP_P, DROP_SEED, DROP_ROWS = 0.1, 0x5EED1234, (3, 2)
BIG_M, MID_M = 20011, 8195


def _build_cases():
    c = []
    for dt in ("f32", "bf16"):
        for D in SWEEP_D:
            c.append(_case(f"sweep-{dt}-37x{D}", 37, D, dt))
        for D in FWD_ONLY_D:
            c.append(_case(f"sweep-{dt}-37x{D}-fwd", 37, D, dt, bwd=()))
    for D in (512, 768, 1024):
        for M in (1024, 1025, BIG_M):
            c.append(_case(f"pair-{M}x{D}", M, D, "bf16", bwd=(), route="pair"))
    c.append(_case("pair-1023x768-one-row", 1023, 768, "bf16", bwd=(), route="row"))
    c.append(_case("pair-1025x768-switched-off", 1025, 768, "bf16", bwd=(), pair_off=True, route="row"))
    c.append(_case("pair-1025x768-offset-8-bytes", 1025, 768, "bf16", bwd=(), offset8=True, route="row"))
    c.append(_case(f"stride-f32-{BIG_M}x768", BIG_M, 768, "f32", bwd=({}, {"dx_add": True})))
    c.append(_case(f"stride-bf16-{BIG_M}x768", BIG_M, 768, "bf16", bwd=({}, {"dbeta": False}), pair_off=True, route="row"))
    for dt in ("f32", "bf16"):
        for D in (768, 516):
            for M in (37, 1025):
                for eps in (1e-12, 1e-5):
                    c.append(_case(f"harsh-{dt}-{M}x{D}-eps{eps:g}", M, D, dt, inputs="harsh", eps=eps))
        for M, D in ((37, 516), (1025, 768)):
            c.append(_case(f"const-{dt}-{M}x{D}", M, D, dt, inputs="const", eps=1e-5, bwd=()))
            c.append(_case(f"ties-{dt}-{M}x{D}", M, D, dt, inputs="ties", eps=1e-12, bwd=()))
        for D in (512, 768):
            for M in (37, MID_M):
                c.append(_case(f"rms-{dt}-{M}x{D}", M, D, dt, rms=True, bwd=({"dx_add": True, "dbeta": False},)))
        for D in (1536, 260):
            c.append(_case(f"gelu-{dt}-37x{D}", 37, D, dt, act=ACT_GELU))
        for M, D in ((37, 516), (MID_M, 768)):
            c.append(_case(f"drop-{dt}-{M}x{D}", M, D, dt, bwd=({"drop": "plain"}, {"drop": "rows"})))
        c.append(_case(f"ordered-{dt}-{MID_M}x768", MID_M, 768, dt, bwd=({"det": True}, {"det": True, "drop": "plain"})))
    c.append(_case(f"mixed-{MID_M}x768", MID_M, 768, "mixed", bwd=({"dx_add": True, "lo": True}, {"det": True})))
    return c


CASES = _build_cases()
HOST_SMALL_M = 1100


def host_case(case):
    """The case at the row count the host test runs it at: above HOST_SMALL_M, 4096 + M % 4096 (still odd, still past one backward
    sweep)."""
    M = case["M"]
    return case if M <= HOST_SMALL_M else dict(case, M=SWEEP_BWD + M % SWEEP_BWD)


def case_inputs(case):
    """CPU tensors of a case: x, dy, dx_add in the storage dtype of the rows, gamma / beta fp32 (beta None without one)."""
    M, D, kind = case["M"], case["D"], case["inputs"]
    g = torch.Generator().manual_seed(7919 + 31 * M + D + len(case["name"]))
    rn = lambda *s: torch.randn(*s, generator=g)
    rows = torch.bfloat16 if case["dtype"] == "bf16" else torch.float32
    grad = torch.float32 if case["dtype"] == "f32" else torch.bfloat16
    r = torch.arange(M, dtype=torch.float32)[:, None]
    gamma, beta = 1 + 0.1 * rn(D), 0.1 * rn(D)
    if kind == "normal":
        x = 2.0 * rn(M, D) + 0.3 * rn(M, 1)
    elif kind == "harsh":   # neighbouring rows differ by +-50 % in their mean: statistics that cross the rows of a pair show
        base, std = (64.0, 0.25) if case["dtype"] != "bf16" else (4.0, 0.5)
        x = base * (1.0 + 0.5 * (1 - 2 * (r % 2))) + std * rn(M, D)
    elif kind == "const":
        x = ((r % 7) - 3).expand(M, D).clone()
    else:   # ties: +-1 in equal numbers, gamma a small integer, beta an odd multiple of 2^-8: +-gamma + beta sits between two bf16 values
        x = (1 - 2 * ((torch.arange(D)[None, :] + r.long()) % 2)).float()
        gamma = torch.randint(1, 4, (D,), generator=g).float()
        beta = (2 * torch.randint(0, 4, (D,), generator=g) + 1).float() * 2.0 ** -8
    out = dict(x=x.to(rows), gamma=gamma, beta=beta if case["beta"] else None, dy=rn(M, D).to(grad))
    out["dx_add"] = rn(M, D).to(torch.float32 if case["dtype"] == "mixed" else rows)
    return out


def host_keep(M, D, p, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M, D, generator=g) >= p).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------------------------------
IGNORE = -100
XENT_C, XENT_ROWS, XENT_PAD = (1, 7, 255, 256, 257, 1000), (1, 48), 24
BCE_SHAPES = ((1, 1), (6, 498), (3, 1025))
GRAD_SCALE = 0.375
POISON = 3.0e38


def xent_inputs(rows, C, bf16, labelled="some", seed=0):
    """(logits [rows, C] in the storage dtype, labels int64).  Row r has its maximum at a level between -top and +top (top = 80 for
    fp32, 60 for bf16; both ends are reached from 2 rows on, a single row sits at +top): there the log-sum-exp needs the max shift.
    Row 0 has one dominant logit `top` above the rest.  Labels include 0, C - 1 and the dominant column; every fifth row from row
    3 on is ignored.  labelled: 'some' | 'one' (exactly one labelled row) | 'none'."""
    g = torch.Generator().manual_seed(4242 + 17 * rows + C + seed)
    top = 60.0 if bf16 else 80.0
    x = torch.randn(rows, C, generator=g)
    level = torch.linspace(-top, top, rows)[:, None] if rows > 1 else torch.full((1, 1), top)
    x = x - x.max(1, keepdim=True).values + level
    x[0] = x[0] - level[0]              # row 0: the rest at 0 and below, one logit `top` above them
    x[0, (C - 1) // 2] = top
    if rows > 1:
        x[1] = x[1] - level[1] - top    # and row 1 takes the level -top
    lab = torch.randint(0, C, (rows,), generator=g)
    lab[0] = C - 1
    if rows > 3:
        lab[1], lab[2] = 0, (C - 1) // 2
        lab[3::5] = IGNORE
    if labelled == "one":
        lab[:] = IGNORE
        lab[rows // 2] = C - 1
    elif labelled == "none":
        lab[:] = IGNORE
    return x.to(torch.bfloat16 if bf16 else torch.float32), lab


def xent_reference(x, lab, grad_scale):
    """float64 (loss, grad [rows, C], row losses, magnitudes).  Every row ignored: loss 0 and zero gradients -- what the kernels leave
    (torch's F.cross_entropy returns NaN there); pinned by the GPU test for both forms."""
    x = x.to(F64)
    valid = lab != IGNORE
    nv = int(valid.sum())
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    mx = x.max(1).values
    t = torch.exp(x - mx[:, None])
    s = t.sum(1)
    lse = mx + torch.log(s)
    xl = x.gather(1, safe[:, None])[:, 0]
    rowloss = torch.where(valid, (lse - xl) / max(nv, 1), torch.zeros_like(lse))
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x).scatter_(1, safe[:, None], 1.0)
    grad = torch.where(valid[:, None], (p - onehot) * grad_scale / max(nv, 1), torch.zeros_like(p))
    return rowloss.sum(), grad, dict(x=x, mx=mx, t=t, s=s, lse=lse, xl=xl, rowloss=rowloss, p=p, onehot=onehot, valid=valid, nv=max(nv, 1),
                                     gs=grad_scale)


def xent_bound(grad, m, bf16):
    C, rows = m["x"].shape[1], m["x"].shape[0]
    e_t = m["t"] * (U * (m["x"] - m["mx"][:, None]).abs() + EXP)
    e_s = e_t.sum(1) + C * U * m["s"]
    e_lse = e_s / m["s"] + EXP * torch.log(m["s"]).abs() + U * m["lse"].abs()
    e_row = torch.where(m["valid"], (e_lse + U * (m["lse"] - m["xl"]).abs()) / m["nv"] + 2 * U * m["rowloss"].abs(), torch.zeros_like(e_lse))
    e_loss = e_row.sum() + rows * U * m["rowloss"].abs().sum()
    e_p = m["p"] * (e_lse[:, None] + U * (m["x"] - m["lse"][:, None]).abs() + EXP)
    e_g = (e_p + U * (m["p"] - m["onehot"]).abs()) * abs(m["gs"]) / m["nv"] + 3 * U * grad.abs()
    e_g = torch.where(m["valid"][:, None], e_g, torch.zeros_like(e_g))
    return e_loss, _store_bound(grad, e_g, bf16)


def xent_model(x, lab, grad_scale, bf16, mutant=None):
    """fp32 numpy model of xent_kernel (sequential sums)."""
    x, lab = np32(x), lab.numpy()
    rows, C = x.shape
    valid = lab != IGNORE
    iv = f32(1) / f32(max(int(valid.sum()), 1))
    with np.errstate(all="ignore"):
        mx = x.max(1)
        s = sum_seq(np.exp(x - mx[:, None]))
        lse = mx + np.log(s)
        xl = x[np.arange(rows), np.where(valid, lab, 0)]
        loss = sum_seq(np.where(valid, (lse - xl) * iv, f32(0)))
        onehot = np.zeros_like(x)
        onehot[np.arange(rows), np.where(valid, lab, 0)] = 1
        grad = np.where(valid[:, None], (np.exp(x - lse[:, None]) - onehot) * (f32(grad_scale) * iv), f32(0)).astype(f32)
    return loss, store32(grad, bf16)


def bce_inputs(B, C, bf16, seed=0):
    """Logits spanning +-100 (fp32) / +-88 (bf16) with exact 0 and both extremes; targets from {0, 1, 0.3}."""
    g = torch.Generator().manual_seed(9001 + 13 * B + C + seed)
    top = 88.0 if bf16 else 100.0
    x = (torch.rand(B, C, generator=g) * 2 - 1) * top
    z = torch.tensor([0.0, 1.0, 0.3])[torch.randint(0, 3, (B, C), generator=g)]
    flat, zf = x.view(-1), z.view(-1)
    flat[0] = 0.0
    if flat.numel() >= 8:
        flat[1:7] = torch.tensor([top, -top, top, -top, top, -top])
        zf[1:7] = torch.tensor([0.0, 0.0, 1.0, 1.0, 0.3, 0.3])
    return x.to(torch.bfloat16 if bf16 else torch.float32), z


def bce_reference(x, z, grad_scale):
    """float64 (loss, grad, magnitudes): loss = mean(bce) C, grad = (sigmoid(x) - z) C grad_scale / n (ops.bce_with_logits_loss)."""
    x, z = x.to(F64), z.to(F64)
    B, C = x.shape
    n = B * C
    sp = torch.log1p(torch.exp(-x.abs()))
    term = x.clamp_min(0) - x * z + sp
    sig = torch.sigmoid(x)
    scale = C * grad_scale / n
    return term.sum() * C / n, (sig - z) * scale, dict(x=x, z=z, sp=sp, term=term, sig=sig, scale=scale, n=n, C=C)


def bce_bound(loss, grad, m, bf16):
    x, z, n = m["x"], m["z"], m["n"]
    e_term = U * (x * z).abs() + U * (x.clamp_min(0) - x * z).abs() + 2 * EXP * m["sp"] + U * m["term"]
    e_loss = (e_term.sum() + n * U * m["term"].sum()) * m["C"] / n + (3 + n / 64.0) * U * loss.abs()
    saturated = x.abs() >= 100.0
    e_sig = torch.where(saturated, torch.full_like(x, TINY), (EXP + 3 * U) * m["sig"] + TINY)
    e_g = (e_sig + U * (m["sig"] - z).abs()) * abs(m["scale"]) + 4 * U * grad.abs()
    return e_loss, _store_bound(grad, e_g, bf16)


def bce_model(x, z, grad_scale, bf16, mutant=None):
    """fp32 numpy model of bce_kernel; mutant 'naive_softplus' (log(1 + exp(x)) - x z)."""
    x, z = np32(x), np32(z)
    B, C = x.shape
    n = B * C
    inv_n = f32(1) / f32(n)
    with np.errstate(all="ignore"):
        if mutant == "naive_softplus":
            term = np.log(f32(1) + np.exp(x)) - x * z
        else:
            term = np.maximum(x, f32(0)) - x * z + np.log1p(np.exp(-np.abs(x)))
        loss = sum_seq(term.reshape(-1).astype(f32)) * inv_n * f32(C)
        sig = f32(1) / (f32(1) + np.exp(-x))
        grad = ((sig - z) * inv_n * f32(C) * f32(grad_scale)).astype(f32)
    return loss, store32(grad, bf16)
