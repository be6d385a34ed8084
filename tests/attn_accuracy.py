"""Accuracy yardsticks of the bf16 flash attention kernels (csrc/attention.hip), shared by tests/test_gpu_attn_accuracy.py and
its host-side self-check tests/test_attn_accuracy_host.py.  Plain torch: nothing here imports or calls the library.

Three things:
  * reference():       float64 attention forward + backward from the bf16-rounded inputs.
  * rounding_model():  the same computation in fp32 with a bf16 round-to-nearest at every point where the kernels store a value
                       in bf16 or feed it to an MFMA as a bf16 operand.  Its error against the reference is what a correct
                       kernel's error looks like at the shape, inputs and flags of the test at hand.
  * within_budget():   the kernel's error against the reference may be at most a fixed margin over the model's,
                           rel_rms(got) <= max(2 rel_rms(model), 2^-10)   and   max_abs(got) <= 3 max_abs(model),
                       per tensor.  Factor 2: the kernel may differ from the model in accumulation order, exp2 against exp and up to
                       three further independent roundings of the same size, which add in quadrature (sqrt 4 = 2).  Factor 3: the
                       maximum is an extreme-value statistic of the same distribution.  Floor 2^-10: a quarter of one bf16 rounding,
                       below what any bf16 tensor on the path resolves (it matters for the fp32 d_pos_bias only).
                       The margins stand over a quantity computed from the reference on every run; they are not tuned to the kernel.
                       When a kernel misses the budget it is wrong, or it rounds somewhere the model does not: then that rounding
                       goes into the model, with the line that does it.  The factors stay.
Plus the probe inputs that read single probabilities out of the kernels (edge_set, v_probe, do_probe, single_row_do) and their
checks.

Layouts: q, o, dO, dq [B, Lq, H*64]; k, v, dk, dv [B, Lk, H*64]; key_mask additive [B, Lk]; pos_bias [H, Lq, Lk]; keep [B, H, Lq, Lk]
(1 = kept) with drop probability p; P [B, H, Lq, Lk].  Causal: key j is visible to query i iff j <= i (top-left aligned)."""
import math
from collections import namedtuple

import torch

DH = 64
EPS = 2.0 ** -8            # bound of one bf16 rounding (relative)
RMS_FACTOR, MAX_FACTOR, RMS_FLOOR = 2.0, 3.0, 2.0 ** -10
V_PROBE_BOUND = 3 * EPS    # one rounding of P, one of o, one spare (fp32 exp2 / divide, a rounding before the dropout rescale)
DO_PROBE_BOUND = 2 * EPS   # one rounding of P, one of dv
SINGLE_ROW_FACTOR = 4 * EPS
P_RANGE = (1e-5, 0.6)      # the probed probabilities: far from fp32 denormals in every form the kernels hold them

Result = namedtuple("Result", "o dq dk dv d_pos_bias P")
NAMES = ("o", "dq", "dk", "dv", "d_pos_bias")


def split(x, H):
    B, L, D = x.shape
    return x.reshape(B, L, H, D // H).permute(0, 2, 1, 3)


def merge(x):
    B, H, L, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, L, H * d)


def _visible(Lq, Lk, strict=False):
    i = torch.arange(Lq)[:, None]
    j = torch.arange(Lk)[None, :]
    return (j < i) | ((j == 0) & (i == 0)) if strict else j <= i


def _scores(q, k, H, key_mask, pos_bias, causal, scale, dt, strict=False):
    s = (split(q, H).to(dt) @ split(k, H).to(dt).transpose(-1, -2)) * scale
    if key_mask is not None:
        s = s + key_mask.to(dt)[:, None, None, :]
    if pos_bias is not None:
        s = s + pos_bias.to(dt)[None]
    if causal:
        s = s.masked_fill(~_visible(s.shape[-2], s.shape[-1], strict), -math.inf)
    return s


def reference_parts(q, k, v, do, H, key_mask=None, pos_bias=None, causal=False, scale=None, keep=None, p=0.0):
    """float64.  Everything reference() returns plus the undropped probabilities P0, dP (the gradient with respect to P0:
    dropped and rescaled like P), delta = rowsum(dO o) and dS."""
    dt = torch.float64
    scale = 1.0 / math.sqrt(DH) if scale is None else scale
    P0 = torch.softmax(_scores(q, k, H, key_mask, pos_bias, causal, scale, dt), dim=-1)
    mul = 1.0 if keep is None else keep.to(dt) / (1.0 - p)
    P = P0 * mul
    qh, kh, vh, doh = (split(t, H).to(dt) for t in (q, k, v, do))
    o = P @ vh
    dv = P.transpose(-1, -2) @ doh
    dP = (doh @ vh.transpose(-1, -2)) * mul
    delta = (doh * o).sum(-1, keepdim=True)
    delta_abs = (doh * o).abs().sum(-1, keepdim=True)
    dS = P0 * (dP - delta)
    dq = scale * (dS @ kh)
    dk = scale * (dS.transpose(-1, -2) @ qh)
    dpb = dS.sum(0) if pos_bias is not None else None
    return dict(o=merge(o), dq=merge(dq), dk=merge(dk), dv=merge(dv), d_pos_bias=dpb, P=P, P0=P0, dP=dP, delta=delta, delta_abs=delta_abs,
                dS=dS)


def reference(q, k, v, do, H, key_mask=None, pos_bias=None, causal=False, scale=None, keep=None, p=0.0):
    """float64 o, dq, dk, dv, d_pos_bias (None without a bias) and P, the dropped and rescaled probabilities that multiply V."""
    r = reference_parts(q, k, v, do, H, key_mask, pos_bias, causal, scale, keep, p)
    return Result(*(r[n] for n in Result._fields))


def bf16_nearest(x):
    return x.to(torch.bfloat16).to(torch.float32)


def bf16_truncate(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


MUTANTS = ("pv_last_key", "dv_last_query", "ds_last_query", "truncate", "o_scale", "no_rescale", "norm_tail", "causal_off_by_one",
           "dpb_transposed")


def mutant_applies(mutant, Lq, Lk, drop, bias, causal):
    return {"no_rescale": drop, "norm_tail": Lk > 32, "causal_off_by_one": causal, "dpb_transposed": bias and Lq == Lk,
            "pv_last_key": Lk > 1}.get(mutant, True)


def rounding_model(q, k, v, do, H, key_mask=None, pos_bias=None, causal=False, scale=None, keep=None, p=0.0, mutant=None):
    """fp32 torch with the kernels' bf16 roundings (csrc/attention.hip):
      * P, dropped and rescaled, before P.V: pack_acc(s[n], ss) in attn_fwd_coop_kernel (`const s16x8 pb = pack_acc(s[n], ss)`),
        after score_to_prob's drop_apply4; and before P^T.dO: `p0 = pack_acc(p, 0), p1 = pack_acc(p, 1)` in attn_bwd_dkdv2_kernel /
        attn_bwd_dkdv_coop_kernel, where p[reg] = keep ? pv * inv_keep : 0.
      * o on output: store_rows(a.o + ..., o[n][0], o[n][1], 1.0f / ltot, h) at the end of attn_fwd_coop_kernel; the backward reads
        that bf16 o for delta: `dlt = fmaf(bf2f(of[j]), bf2f(dof[ks][j]), dlt)` in attn_bwd_dq2_kernel / attn_bwd_dq_coop_kernel.
      * dS before the dQ and dK products: `d0 = pack_acc(s, 0), d1 = pack_acc(s, 1)` in all four backward kernels.  dS itself is
        the product of the fp32 p and the fp32 dP - delta (`s[reg] = pv * dp[reg]`), and that fp32 value is what d_pos_bias sums
        (`atomicAdd(dbrow + key, ds)` in attn_bwd_dq_coop_kernel), over b in fp32.
      * dq, dk, dv on output: store_rows(..., a.scale, h) / store_rows(..., 1.0f, h) at the end of the backward kernels (the scale
        is applied to the fp32 accumulator, before the rounding).
    The normaliser l, the log-sum-exp, dP, delta and every accumulation stay fp32 (f32x16 accumulators of mfma32).
    (The forward kernel rounds the UNnormalised exp2(x - running max) and divides the fp32 sum by l afterwards; the model rounds the
    normalised P: a relative rounding of the same size at the same place.  online_model() below does it the kernel's way.)

    mutant: one of MUTANTS, a subtly wrong kernel for the host-side self-check; None is the model itself."""
    assert mutant is None or mutant in MUTANTS
    f32 = torch.float32
    rnd = bf16_truncate if mutant == "truncate" else bf16_nearest
    scale = 1.0 / math.sqrt(DH) if scale is None else scale
    s = _scores(q, k, H, key_mask, pos_bias, causal, scale, f32, strict=mutant == "causal_off_by_one")
    P0 = torch.softmax(s, dim=-1)
    mul = 1.0 if keep is None else (keep.to(f32) if mutant == "no_rescale" else keep.to(f32) * (1.0 / (1.0 - p)))
    qh, kh, vh, doh = (split(t, H).to(f32) for t in (q, k, v, do))
    Lq, Lk = s.shape[-2:]

    P0f = P0
    if mutant == "norm_tail":   # the normaliser misses the last key tile
        e = torch.exp(s - s.amax(-1, keepdim=True))
        P0f = e / e[..., :32 * ((Lk - 1) // 32)].sum(-1, keepdim=True)
    Pb = rnd(P0f * mul)                       # bf16 operand of P.V
    Pv = Pb.clone()
    if mutant == "pv_last_key":
        Pv[..., Lk - 1] = 0
    o = Pv @ vh
    if mutant == "o_scale":
        o = o * 1.01
    o = rnd(o)                                # stored, and read back for delta

    Pt = rnd(P0 * mul)                        # bf16 operand of P^T.dO (recomputed from the log-sum-exp)
    if mutant == "dv_last_query":
        Pt = Pt.clone()
        Pt[..., Lq - 1, :] = 0
    dv = rnd(Pt.transpose(-1, -2) @ doh)
    delta = (doh * o).sum(-1, keepdim=True)
    dS = P0 * ((doh @ vh.transpose(-1, -2)) * mul - delta)
    if mutant == "ds_last_query":
        dS = dS.clone()
        dS[..., Lq - 1, :] = 0
    dSb = rnd(dS)
    dq = rnd(scale * (dSb @ kh))
    dk = rnd(scale * (dSb.transpose(-1, -2) @ qh))
    dpb = None
    if pos_bias is not None:
        dpb = dS.sum(0)
        if mutant == "dpb_transposed":
            dpb = dpb.transpose(-1, -2).contiguous()
    return Result(merge(o), merge(dq), merge(dk), merge(dv), dpb, Pb)


def online_model(q, k, v, do, H, key_mask=None, pos_bias=None, causal=False, scale=None, keep=None, p=0.0):
    """A second model, written on its own and in the kernels' order: the forward is an online softmax over 32-key tiles in the
    log2 domain with an UNnormalised bf16 P and the division by l at the end; the backward recomputes P from the log-sum-exp and
    walks the same tiles.  P of the result is o's effective probability matrix (bf16 numerators over the fp32 normaliser)."""
    f32 = torch.float32
    LOG2E = 1.4426950408889634
    sc = (1.0 / math.sqrt(DH) if scale is None else scale) * LOG2E
    B, Lq, D = q.shape
    Lk = k.shape[1]
    Q, K, V, DO = (t.view(t.shape[0], t.shape[1], H, DH).transpose(1, 2).to(f32) for t in (q, k, v, do))
    inv_keep = 1.0 / (1.0 - p) if keep is not None else 1.0
    rows = torch.arange(Lq)[:, None]

    def tile_scores(j0, j1):
        x = (Q @ K[:, :, j0:j1].transpose(2, 3)) * sc
        if key_mask is not None:
            x = x + (key_mask[:, None, None, j0:j1].to(f32) * LOG2E)
        if pos_bias is not None:
            x = x + (pos_bias[None, :, :, j0:j1].to(f32) * LOG2E)
        if causal:
            x = torch.where(torch.arange(j0, j1)[None, :] > rows, torch.full_like(x, -math.inf), x)
        return x

    def dropped(t, j0, j1, other=0.0):
        return t if keep is None else torch.where(keep[..., j0:j1] != 0, t * inv_keep, torch.full_like(t, other))

    m = torch.full((B, H, Lq, 1), -1e30)
    l = torch.zeros(B, H, Lq, 1)
    acc = torch.zeros(B, H, Lq, DH)
    nums = []
    for j0 in range(0, Lk, 32):
        j1 = min(j0 + 32, Lk)
        x = tile_scores(j0, j1)
        mnew = torch.maximum(m, x.amax(-1, keepdim=True))
        alpha = torch.exp2(m - mnew)
        pt = torch.exp2(x - mnew)
        l = l * alpha + pt.sum(-1, keepdim=True)
        pb = dropped(pt, j0, j1).to(torch.bfloat16).to(f32)
        acc = acc * alpha + pb @ V[:, :, j0:j1]
        nums = [n * alpha for n in nums] + [pb]
        m = mnew
    o = (acc / l).to(torch.bfloat16).to(f32)
    lse = m + torch.log2(l)
    Peff = torch.cat(nums, -1) / l

    delta = (DO * o).sum(-1, keepdim=True)
    dq = torch.zeros(B, H, Lq, DH)
    dk, dv, dsum = [], [], []
    for j0 in range(0, Lk, 32):
        j1 = min(j0 + 32, Lk)
        pn = torch.exp2(tile_scores(j0, j1) - lse)
        dp = DO @ V[:, :, j0:j1].transpose(2, 3)
        ds = pn * (dropped(dp, j0, j1) - delta) if keep is not None else pn * (dp - delta)
        dsb = ds.to(torch.bfloat16).to(f32)
        pdb = dropped(pn, j0, j1).to(torch.bfloat16).to(f32)
        dq = dq + dsb @ K[:, :, j0:j1]
        dk.append(dsb.transpose(2, 3) @ Q)
        dv.append(pdb.transpose(2, 3) @ DO)
        dsum.append(ds.sum(0))
    scale_ = sc / LOG2E
    back = lambda t: t.to(torch.bfloat16).to(f32).transpose(1, 2).reshape(B, -1, H * DH)
    return Result(back(o), back(dq * scale_), back(torch.cat(dk, 2) * scale_), back(torch.cat(dv, 2)),
                  torch.cat(dsum, -1) if pos_bias is not None else None, Peff)


# ------------------------------------------------------------------------------------------------------------------------
# metrics and the budget
# ------------------------------------------------------------------------------------------------------------------------
def rel_rms(x, ref):
    x, ref = x.detach().cpu().to(torch.float64), ref.detach().cpu().to(torch.float64)
    den = ref.norm().item()
    num = (x - ref).norm().item()
    return num / den if den > 0 else (0.0 if num == 0 else math.inf)


def max_abs(x, ref):
    return (x.detach().cpu().to(torch.float64) - ref.detach().cpu().to(torch.float64)).abs().max().item()


def within_budget(got, model, ref):
    """(ok, figures) of one tensor.  figures = (rel_rms got, rel_rms model, max_abs got, max_abs model).  NaN fails."""
    rg, rm, mg, mm = rel_rms(got, ref), rel_rms(model, ref), max_abs(got, ref), max_abs(model, ref)
    ok = rg <= max(RMS_FACTOR * rm, RMS_FLOOR) and mg <= MAX_FACTOR * mm
    return bool(ok), (rg, rm, mg, mm)


def budget_report(got, model, ref, names=NAMES, label=""):
    """within_budget over the named tensors of three Results (tensors the reference has as None are skipped): prints the figures
    and returns the names that miss the budget."""
    bad = []
    for n in names:
        r = getattr(ref, n)
        if r is None:
            continue
        ok, (rg, rm, mg, mm) = within_budget(getattr(got, n), getattr(model, n), r)
        print(f"[attn-accuracy] {label} {n}: rel_rms {rg:.3e} (model {rm:.3e}, ratio {rg / rm if rm else math.nan:.2f}) "
              f"max_abs {mg:.3e} (model {mm:.3e}, ratio {mg / mm if mm else math.nan:.2f}){'' if ok else '  OVER BUDGET'}")
        if not ok:
            bad.append(n)
    return bad


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def randn_bf16(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def packed_inputs(B, H, Lq, Lk, seed, qk_scale=1.0):
    """The layers' own layouts (CPU, bf16): for Lq == Lk one packed [B, L, 3D] projection (Q | K | V), else q [B, Lq, D] and a
    packed [B, Lk, 2D] (K | V).  Returns (buffers, q, k, v, dO) with q, k, v views of the buffers."""
    D = H * DH
    if Lq == Lk:
        qkv = randn_bf16(B, Lq, 3 * D, seed=seed)
        qkv[..., :2 * D] = (qkv[..., :2 * D].float() * qk_scale).to(torch.bfloat16)
        bufs, (q, k, v) = (qkv,), (qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:])
    else:
        q = randn_bf16(B, Lq, D, seed=seed, scale=qk_scale)
        kv = randn_bf16(B, Lk, 2 * D, seed=seed + 1)
        kv[..., :D] = (kv[..., :D].float() * qk_scale).to(torch.bfloat16)
        bufs, (k, v) = (q, kv), (kv[..., :D], kv[..., D:])
    return bufs, q, k, v, randn_bf16(B, Lq, D, seed=seed + 2)


def tail_key_mask(B, Lk):
    """Additive -10000 mask [B, Lk]: sample 0's last 3 keys and sample 1's second half are padding."""
    m = torch.zeros(B, Lk)
    m[0, max(Lk - 3, 1):] = -10000.0
    if B > 1:
        m[1, Lk // 2:] = -10000.0
    return m


def host_keep_mask(B, H, Lq, Lk, p, seed):
    """A keep mask for the host-side self-check (the GPU tests take the library's own)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, H, Lq, Lk, generator=g) >= p).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------------
# probes: inputs that make an output element equal ONE probability, so that the tile edges are read entry by entry
# ------------------------------------------------------------------------------------------------------------------------
def edge_set(L):
    """The rows / keys at which a 32-wide tile, a 64-row pair of tiles and a 128-row workgroup begin and end, the middle and the
    tail of the sequence; at most 64 (one probe per head channel)."""
    cand = [0, 1, 30, 31, 32, 33, 62, 63, 64, 65, 95, 96, 127, 128, 129, L // 2, L - 34, L - 33, L - 32, L - 3, L - 2, L - 1]
    return sorted({c for c in cand if 0 <= c < L})[:DH]


def v_probe(B, H, Lk):
    """v with v[b, j_c, h*64 + c] = 1 for the c-th key j_c of edge_set(Lk), 0 elsewhere: o[b, i, h*64 + c] = P[b, h, i, j_c]."""
    keys = edge_set(Lk)
    v = torch.zeros(B, Lk, H, DH)
    for c, j in enumerate(keys):
        v[:, j, :, c] = 1.0
    return v.reshape(B, Lk, H * DH).to(torch.bfloat16), keys


def do_probe(B, H, Lq):
    """dO with dO[b, i_c, h*64 + c] = 1 for the c-th query i_c of edge_set(Lq): dv[b, j, h*64 + c] = P[b, h, i_c, j]."""
    rows = edge_set(Lq)
    do = torch.zeros(B, Lq, H, DH)
    for c, i in enumerate(rows):
        do[:, i, :, c] = 1.0
    return do.reshape(B, Lq, H * DH).to(torch.bfloat16), rows


def single_row_do(B, H, Lq, row, seed):
    do = torch.zeros(B, Lq, H * DH, dtype=torch.bfloat16)
    do[:, row] = randn_bf16(B, H * DH, seed=seed)
    return do


def _probe_errors(got, want, rest):
    """got / want [..., n] (float64 reference probabilities); rest: the output channels no probe writes."""
    got = got.detach().cpu().to(torch.float64)
    live = want > 0
    rel = ((got - want).abs() / torch.where(live, want, torch.ones_like(want)))[live]
    zeros_ok = bool((got[~live] == 0).all()) and bool((rest.detach().cpu() == 0).all())
    return (rel.max().item() if rel.numel() else 0.0), zeros_ok


def check_v_probe(o, P, keys, H):
    """o of a forward call on v_probe's v against the reference P: (worst relative error over the live probed entries, zeros
    exact)."""
    oh = split(o, H)
    return _probe_errors(oh[..., :len(keys)], P[..., keys], oh[..., len(keys):])


def check_do_probe(dv, P, rows, H):
    """dv of a backward call on do_probe's dO against the reference P (same returns as check_v_probe)."""
    dvh = split(dv, H)
    return _probe_errors(dvh[..., :len(rows)], P[:, :, rows, :].transpose(-1, -2), dvh[..., len(rows):])


def dq_rows_outside_are_zero(dq, rows):
    """dP = 0 and delta = 0 on every query row without a probe: its dq is exactly 0."""
    out = torch.ones(dq.shape[1], dtype=torch.bool)
    out[rows] = False
    return bool((dq.detach().cpu()[:, out] == 0).all())


def single_row_dk_excess(dk, parts, q, H, row, scale):
    """dO lives on query `row` only, so dk[j, :] = scale dS[row, j] q[row, :] is a one-term product.  Returns the worst
    |err| / bound over the elements, bound = 4 2^-8 scale P[row, j] (|dP[row, j]| + |delta[row]|) |q[row, d]| from the reference's
    cancellation-free magnitudes (P: undropped; dP: dropped and rescaled; |delta| as sum_d |dO_d o_d|: the kernels sum delta from
    the bf16 o, so its error follows that sum -- with |sum_d dO_d o_d| the rounding model itself misses the bound wherever dP and
    delta both nearly cancel), and whether dk is exactly 0 where the bound is 0."""
    dkh = split(dk, H).detach().cpu().to(torch.float64)                                # [B, H, Lk, 64]
    qr = split(q, H).to(torch.float64)[:, :, row, :]                                   # [B, H, 64]
    mag = parts["P0"][:, :, row, :] * (parts["dP"][:, :, row, :].abs() + parts["delta_abs"][:, :, row, :])   # [B, H, Lk]
    bound = SINGLE_ROW_FACTOR * scale * mag[..., None] * qr.abs()[:, :, None, :]
    err = (dkh - split(parts["dk"], H)).abs()
    live = bound > 0
    worst = (err[live] / bound[live]).max().item() if live.any() else 0.0
    return worst, bool((err[~live] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------
# cases and criteria: the GPU tests and the host-side self-check run the SAME code on a `candidate`, a callable that takes a
# case (dict) and returns a Result (P unused) -- the kernels on the GPU; the models and the mutants on the host
# ------------------------------------------------------------------------------------------------------------------------
A_SHAPES = [(577, 577), (32, 577), (577, 32), (33, 65), (100, 45), (128, 128), (1, 70)]      # budget against the rounding model
B_SHAPES = [(577, 577), (33, 65), (100, 45), (129, 577), (577, 32), (1, 70)]                 # probes
B_VARIANTS = ("plain", "masked", "dropout")
DROP_P = 0.1
# Seed of the probe cases' q and k.  Unit randn inputs at scale 1/8 put the probed probabilities of these shapes in about [5e-6, 0.7]
# depending on the draw; this draw keeps them inside P_RANGE at every probe shape and mask (asserted on the reference in every run).
PROBE_SEED = 518


def make_case(B, H, Lq, Lk, seed, masked=False, probe_mask=False, bias=False, causal=False, scale=None, qk_scale=1.0, bias_scale=1.0, p=0.0,
              drop_seed=0):
    """Inputs of one attention call on the CPU (bf16 q, k, v, dO as views of the layers' packed buffers).  `keep` is left None:
    with p > 0 the caller stores the keep mask [B, H, Lq, Lk] of (p, drop_seed) there before any criterion runs."""
    bufs, q, k, v, do = packed_inputs(B, H, Lq, Lk, seed, qk_scale)
    g = torch.Generator().manual_seed(seed + 7)
    return dict(bufs=bufs, q=q, k=k, v=v, do=do, H=H, key_mask=(probe_key_mask if probe_mask else tail_key_mask)(B, Lk) if masked else None,
                pos_bias=(torch.randn(H, Lq, Lk, generator=g) * bias_scale) if bias else None, causal=causal,
                scale=1.0 / math.sqrt(DH) if scale is None else scale, keep=None, p=p, drop_seed=drop_seed)


def t5_regime(kw):
    """T5's unscaled scores: scale 1.0 with 0.35 randn q and k and a 0.5 randn relative-position bias."""
    return dict(kw, scale=1.0, qk_scale=0.35, bias_scale=0.5)


def c_cases():
    """(label, Lq, Lk, dropout, make_case arguments) of the key mask (1) | position bias (2) | causal (4) instances: all eight
    without dropout at 70 x 70, the non-causal ones at 33 x 65 as well, and the two dropout instances with a bias (2, 6)."""
    out = []
    for flags in range(8):
        for Lq, Lk in ((70, 70), (33, 65)):
            if flags & 4 and Lq != Lk:
                continue
            kw = dict(masked=bool(flags & 1), bias=bool(flags & 2), causal=bool(flags & 4))
            out.append((f"flags{flags}-{Lq}x{Lk}", Lq, Lk, False, kw))
    out.append(("flags2-33x65-dropout", 33, 65, True, dict(bias=True)))
    out.append(("flags6-33x33-dropout", 33, 33, True, dict(bias=True, causal=True)))
    return out


def model_args(case):
    assert case["p"] == 0 or case["keep"] is not None
    return dict(q=case["q"], k=case["k"], v=case["v"], do=case["do"], H=case["H"], key_mask=case["key_mask"], pos_bias=case["pos_bias"],
                causal=case["causal"], scale=case["scale"], keep=case["keep"] if case["p"] > 0 else None, p=case["p"])


def _yardsticks(case, tag):
    """reference_parts and rounding_model of the case as it stands, computed once per case and probe (tag) and left unchanged."""
    if case.get("_tag") != tag:
        parts = reference_parts(**model_args(case))
        case["_tag"], case["_parts"], case["_model"] = tag, parts, rounding_model(**model_args(case))
        case["_ref"] = Result(*(parts[n] for n in Result._fields))
    return case["_parts"], case["_ref"], case["_model"]


def check_budget(cand, case, label, names=NAMES, figures=None):
    """Criterion A / C: the names of the tensors of cand(case) that miss within_budget (empty = pass)."""
    _, ref, model = _yardsticks(case, "budget")
    got = cand(case)
    bad = budget_report(got, model, ref, names, label)
    if figures is not None:
        for n in names:
            if getattr(ref, n) is not None:
                figures.setdefault(n, []).append(within_budget(getattr(got, n), getattr(model, n), getattr(ref, n))[1])
    if case["causal"] and case["pos_bias"] is not None and "d_pos_bias" in names:
        above = ~_visible(*ref.d_pos_bias.shape[-2:])
        if not torch.equal((got.d_pos_bias.detach().cpu() == 0)[:, above], (ref.d_pos_bias == 0)[:, above]):
            print(f"[attn-accuracy] {label} d_pos_bias: nonzero above the causal diagonal")
            bad.append("d_pos_bias zero pattern")
    return bad


def probe_key_mask(B, Lk):
    """Additive -10000 mask [B, Lk] of the probe cases, with probed keys among the padding: sample 0's last 3 keys, sample 1's keys
    1, 32 and 33 (enough live keys stay at Lk = 32 for the probed probabilities to keep their range)."""
    m = torch.zeros(B, Lk)
    m[0, max(Lk - 3, 1):] = -10000.0
    if B > 1:
        m[1, [j for j in (1, 32, 33) if j < Lk - 1]] = -10000.0
    return m


def _assert_probed_range(P0sel, label):
    """The probe inputs keep the probed (undropped) probabilities inside P_RANGE, so that the relative bounds never meet a denormal."""
    live = P0sel[P0sel > 0]
    lo, hi = (live.min().item(), live.max().item()) if live.numel() else (P_RANGE[0], P_RANGE[1])
    print(f"[attn-accuracy] {label}: probed P in [{lo:.2e}, {hi:.2e}]")
    assert P_RANGE[0] <= lo and hi <= P_RANGE[1], f"{label}: probed reference probabilities [{lo}, {hi}] leave {P_RANGE}"


def check_v_probe_case(cand, case, label):
    """Criterion B, forward: case["v"] is overwritten with the probe.  Returns the failures (empty = pass) and the worst error."""
    vp, keys = v_probe(case["q"].shape[0], case["H"], case["k"].shape[1])
    if case.get("_tag") != "v":
        case["v"].copy_(vp)
    parts, ref, _ = _yardsticks(case, "v")
    _assert_probed_range(parts["P0"][..., keys], label + " V probe")
    rel, zeros_ok = check_v_probe(cand(case).o, ref.P, keys, case["H"])
    print(f"[attn-accuracy] {label} V probe: worst relative error {rel:.3e} (bound {V_PROBE_BOUND:.3e}), zeros exact {zeros_ok}")
    return [n for n, ok in (("V probe error", rel <= V_PROBE_BOUND), ("V probe zeros", zeros_ok)) if not ok], rel


def check_do_probe_case(cand, case, label):
    """Criterion B, backward: case["do"] is overwritten with the probe.  dv entry by entry, dq rows without a probe exactly 0, dq and
    dk within the budget."""
    dop, rows = do_probe(case["q"].shape[0], case["H"], case["q"].shape[1])
    if case.get("_tag") != "do":
        case["do"].copy_(dop)
    parts, ref, model = _yardsticks(case, "do")
    _assert_probed_range(parts["P0"][:, :, rows, :], label + " dO probe")
    got = cand(case)
    rel, zeros_ok = check_do_probe(got.dv, ref.P, rows, case["H"])
    dq_zero = dq_rows_outside_are_zero(got.dq, rows)
    print(f"[attn-accuracy] {label} dO probe: worst relative error {rel:.3e} (bound {DO_PROBE_BOUND:.3e}), zeros exact {zeros_ok}, "
          f"unprobed dq rows zero {dq_zero}")
    bad = [n for n, ok in (("dO probe error", rel <= DO_PROBE_BOUND), ("dO probe zeros", zeros_ok), ("dq rows", dq_zero)) if not ok]
    return bad + budget_report(got, model, ref, ("dq", "dk"), label + " dO probe"), rel


def single_rows(Lq):
    return sorted({r for r in (0, 31, 32, Lq - 1) if 0 <= r < Lq})


def check_single_row_case(cand, case, row, label):
    """Criterion B, dK path: case["do"] is overwritten with a dO that lives on one query row."""
    if case.get("_tag") != ("row", row):
        case["do"].copy_(single_row_do(case["q"].shape[0], case["H"], case["q"].shape[1], row, seed=900 + row))
    parts, _, _ = _yardsticks(case, ("row", row))
    worst, zeros_ok = single_row_dk_excess(cand(case).dk, parts, case["q"], case["H"], row, case["scale"])
    print(f"[attn-accuracy] {label} single-row dO (row {row}): worst |err| / bound {worst:.3f}, zeros exact {zeros_ok}")
    return [n for n, ok in ((f"dk of row {row}", worst <= 1.0), (f"dk zeros of row {row}", zeros_ok)) if not ok], worst
