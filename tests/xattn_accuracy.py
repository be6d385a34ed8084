"""Accuracy yardsticks of the fused cross-attention sub-block (csrc/xattn.hip, csrc/xflash.hip: m3ae_xattn_fwd / m3ae_xattn_bwd),
shared by tests/test_gpu_xattn_accuracy.py and its host-side self-check tests/test_xattn_accuracy_host.py.  Plain torch: nothing
here imports or calls the library.  Every function runs on the device its inputs live on (the GPU tests compute the yardsticks
on the GPU in float64 / fp32 torch; the host tests on the CPU).

  * reference():       float64 forward + backward (torch autograd) of the REFERENCE'S formulation (bert_model.py:253-350 cross
                       branch, :353-364): separate Q / K / V projections, softmax(Q K^T / sqrt(dh) + mask), attention dropout with
                       a given keep mask, P V, output dense, hidden dropout with a given keep mask, residual, LayerNorm -- from the
                       bf16-rounded inputs and the bf16 compute copies of the weights.  d(b_k) is exactly zero: the key bias adds the
                       same number to every key of a row.
  * rounding_model():  fp32 torch of the ABSORBED algebra of each direction (header of csrc/xattn.hip) with a bf16 round-to-nearest
                       wherever the kernels store bf16 or feed a bf16 MFMA operand; every rounding cites the line that does it.
  * criteria():        attn_accuracy.within_budget, unchanged, per tensor (out, dx, dother and every parameter gradient but the
                       LayerNorm bias's, a pure fp32 sum: ln_bias_excess), errors against reference():
                           rel_rms(got) <= max(2 rel_rms(model), 2^-10),   max_abs(got) <= 3 max_abs(model);
                       and the saved probabilities entry by entry (check_probs):   |P_got - P_ref| <= (3 r + 2^-8) P_ref with r the
                       model's largest relative entrywise error on the softmax row; exact zeros where the keep mask drops an entry.
                       When a kernel misses a budget it is wrong, or it rounds somewhere the model does not: then that rounding goes
                       into the model, with its line.  The factors stay.

Layouts: x [B, Lq, D] (the stream that is updated: queries and residual), y [B, Lk, D] (the other stream: keys and values), mask
additive [B, Lk], dout [B, Lq, D]; direction 0 = text queries over image keys (Lq = T, Lk = I), 1 = image queries over text keys
(Lq = I, Lk = T).  keep_a [B, H, Lq, Lk], keep_h [B, Lq, D] (1 = kept), drop probability p.  P [B, H, Lq, Lk].

Input regimes (make_case):
  unit    randn inputs, weights randn * 2 / sqrt(D), biases 0.1 randn (b_k included), LayerNorm weight 1 + 0.1 randn.
  peaked  the query and key weights scaled by PEAKED_QK each: the float64 row maximum of P exceeds 0.9 on at least a quarter of the
          rows (peaked_fraction(); asserted in tests/test_xattn_accuracy_host.py at every shape).
  masked  sample 0 keeps ONE key, sample 1 (where there is one) has EVERY key at -10000, the rest carry a tail mask.  The rows of
          the other stream under a mask hold MASKED_FILL x randn (finite, 16 x the live rows) in the samples that keep a visible
          key: their probabilities are exactly 0 in fp32 and in float64, so they may not move any result.  (NaN / Inf bit patterns
          cannot stand there: softmax(Q K^T + mask) is not defined on them -- the key projection of a NaN row is NaN, so is its
          score before the mask is added, and 0 x NaN = NaN in the P V product -- the float64 reference itself returns NaN.  The
          sample with every key masked is an ordinary softmax of its scores: its rows keep unit scale.)"""
import math

import torch

from attn_accuracy import EPS, MAX_FACTOR, RMS_FACTOR, RMS_FLOOR, bf16_nearest, bf16_truncate, max_abs, rel_rms, within_budget  # noqa: F401

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DROP_P = 0.1
LN_EPS = 1e-12
WSCALE = 2.0
PEAKED_QK = 2.0
MASKED_FILL = 16.0
MASK = -10000.0
REGIMES = ("unit", "peaked", "masked")

# the tensors the budget is applied to; g_bk is held to bit-identity instead (the fused path never touches its buffer)
GRADS = {"g_wq": "self.query.weight", "g_bq": "self.query.bias", "g_wk": "self.key.weight", "g_wv": "self.value.weight",
         "g_bv": "self.value.bias", "g_wo": "output.dense.weight", "g_bo": "output.dense.bias", "g_ln_g": "output.LayerNorm.weight",
         "g_ln_b": "output.LayerNorm.bias"}
KEY_BIAS = "self.key.bias"
TENSORS = ("out", "dx", "dother") + tuple(GRADS)
PARAMS = {"wq": "self.query.weight", "bq": "self.query.bias", "wk": "self.key.weight", "bk": KEY_BIAS, "wv": "self.value.weight",
          "bv": "self.value.bias", "wo": "output.dense.weight", "bo": "output.dense.bias", "ln_g": "output.LayerNorm.weight",
          "ln_b": "output.LayerNorm.bias"}

# ------------------------------------------------------------------------------------------------------------------------
# shapes of the GPU tests: (direction, B, T, I) at D = 768, H = 12 unless the entry says otherwise
# ------------------------------------------------------------------------------------------------------------------------
A_SHAPES = ([(0, 2, 32, I) for I in (33, 159, 160, 161, 577, 639, 640)] + [(1, 2, 32, I) for I in (33, 127, 128, 129, 577)]
            + [(0, 2, 64, I) for I in (65, 577)] + [(1, 2, 64, I) for I in (65, 129, 1025)]
            + [(0, 1, 32, 577), (1, 1, 32, 577)])
# split-K of the XE_ATOMIC weight gradients (pick_split below): B T = 544 rows are 17 chunks, split 9 + 8; at 64 text tokens the chunk
# count 2 B is even, so two splits are always equal (B = 9: 9 + 9) and a shorter last split needs three (B = 13: 9 + 9 + 8)
SPLITK_SHAPES = [(d, B, T, I) for d in (0, 1) for (B, T, I) in ((17, 32, 33), (9, 64, 65), (13, 64, 65))]
B_SHAPES = [(0, 2, T, I) for T in (32, 64) for I in (159, 160, 161, 639, 640)] + [(1, 2, T, I) for T in (32, 64) for I in (127, 128, 129)]
C_SHAPES = [(d, 2, 32, I) for d in (0, 1) for I in (33, 577)]
# the envelope of m3ae_xattn_supported: (direction, D, H, T, I), a small member of every class (direction, T, head width dh = D / H)
# it answers 1 for.  Direction 0: T in {32, 64}, dh a multiple of 32 up to 256, D % 128 == 0 -- dh = 64 takes the two-chunk
# operand build, every other width the general template with dh / 32 chunks.  Direction 1: H T in {384, 768}, i.e. H = 12, and
# D % 256 == 0: dh = 64 (one-launch build of K', V' and c), 128, 192 and 256 (separate builds, the general branch of xattn_colbias_kernel).
# m3ae_xattn_bwd_supported stops at D = 2048 (the LayerNorm backward's widest row): members wider than that are forward-only classes
def _lcm(a, b):
    return a * b // math.gcd(a, b)


HEAD_WIDTHS = {0: tuple(range(32, 257, 32)), 1: (64, 128, 192, 256)}     # the head widths m3ae_xattn_supported accepts, per direction
D_CLASSES = ([(0, max(_lcm(128, dh), 256), max(_lcm(128, dh), 256) // dh, T, 65) for T in (32, 64) for dh in HEAD_WIDTHS[0]]
             + [(1, 12 * dh, 12, T, 65) for T in (32, 64) for dh in HEAD_WIDTHS[1]])


def pick_split(B, T, H, D):
    """(ksplit, kchunks, chunks of the last split) of the XE_ATOMIC weight gradients: the arithmetic of pick_split() in csrc/xattn.hip
    with its call sites' arguments nchunks = ceil(B T / 32), tiles = H ceil(D / 384)."""
    nchunks, tiles = (B * T + 31) // 32, H * ((D + 383) // 384)
    ks = 256 // max(tiles, 1)
    ks = max(min(ks, nchunks // 8), 1)
    kchunks = (nchunks + ks - 1) // ks
    ksplit = (nchunks + kchunks - 1) // kchunks
    return ksplit, kchunks, nchunks - (ksplit - 1) * kchunks


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def _bf(t):
    return t.to(BF16).to(F32)


def key_mask(regime, masked, B, Lk):
    """Additive [B, Lk] mask, or None.  unit / peaked with masked: sample b hides its last Lk // 4 + 3 b keys (at least one stays).
    masked regime: sample 0 keeps key Lk // 3 only, sample 1 hides every key, the rest as above."""
    if regime != "masked" and not masked:
        return None
    m = torch.zeros(B, Lk)
    for b in range(B):
        m[b, Lk - min(Lk - 1, Lk // 4 + 3 * b):] = MASK
    if regime == "masked":
        m[0] = MASK
        m[0, Lk // 3] = 0.0
        if B > 1:
            m[1] = MASK
    return m


def make_case(direction, B, T, I, D=768, H=12, regime="unit", masked=False, p=0.0, seed=0):
    """One call's inputs on the CPU: fp32 tensors whose values are exact in bf16 where the kernels read bf16 (x, y, dout, the four
    weights); biases and LayerNorm parameters fp32.  keep_a / keep_h are left None: with p > 0 the caller stores the keep masks
    before any yardstick runs (the GPU tests take the library's own, the host tests host_keep_masks)."""
    assert regime in REGIMES and direction in (0, 1)
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    qk = PEAKED_QK if regime == "peaked" else 1.0
    w = lambda f: _bf(rn(D, D) * (WSCALE * f / math.sqrt(D)))
    case = dict(direction=direction, B=B, T=T, I=I, D=D, H=H, regime=regime, p=p, eps=LN_EPS, keep_a=None, keep_h=None,
                wq=w(qk), wk=w(qk), wv=w(1.0), wo=w(1.0), bq=0.1 * rn(D), bk=0.1 * rn(D), bv=0.1 * rn(D), bo=0.1 * rn(D),
                ln_g=1.0 + 0.1 * rn(D), ln_b=0.1 * rn(D))
    xt, xi = _bf(rn(B, T, D)), _bf(rn(B, I, D))
    x, y = (xt, xi) if direction == 0 else (xi, xt)
    mask = key_mask(regime, masked, B, y.shape[1])
    if regime == "masked":
        fill = _bf(MASKED_FILL * rn(*y.shape))
        hidden = (mask < 0) & (mask == 0).any(-1, keepdim=True)      # masked rows of the samples that keep a visible key
        y = torch.where(hidden[..., None], fill, y)
    case.update(x=x, y=y, mask=mask, dout=_bf(rn(*x.shape)), Lq=x.shape[1], Lk=y.shape[1])
    return case


def host_keep_masks(case, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, Lq, Lk, D = (case[k] for k in ("B", "H", "Lq", "Lk", "D"))
    return ((torch.rand(B, H, Lq, Lk, generator=g) >= case["p"]).to(torch.uint8), (torch.rand(B, Lq, D, generator=g) >= case["p"]).to(torch.uint8))


def to_device(case, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def _split(t, H):
    B, L, D = t.shape
    return t.reshape(B, L, H, D // H).permute(0, 2, 1, 3)


def _merge(t):
    B, H, L, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, H * d)


# ------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ------------------------------------------------------------------------------------------------------------------------
def reference(case):
    """dict: out, P0 (undropped), P (dropped and rescaled: what multiplies V), dx, dother, g_* of GRADS and g_bk (exactly 0)."""
    H, p = case["H"], case["p"]
    leaf = {n: case[n].to(F64).clone().requires_grad_(True) for n in list(PARAMS) + ["x", "y"]}
    x, y = leaf["x"], leaf["y"]
    q = x @ leaf["wq"].t() + leaf["bq"]
    k = y @ leaf["wk"].t() + leaf["bk"]
    v = y @ leaf["wv"].t() + leaf["bv"]
    s = _split(q, H) @ _split(k, H).transpose(-1, -2) / math.sqrt(case["D"] // H)
    if case["mask"] is not None:
        s = s + case["mask"].to(F64)[:, None, None, :]
    P0 = torch.softmax(s, -1)
    P = P0 * (case["keep_a"].to(F64) / (1.0 - p)) if p > 0 else P0
    dense = _merge(P @ _split(v, H)) @ leaf["wo"].t() + leaf["bo"]
    if p > 0:
        dense = dense * (case["keep_h"].to(F64) / (1.0 - p))
    out = torch.nn.functional.layer_norm(dense + x, (case["D"],), leaf["ln_g"], leaf["ln_b"], case["eps"])
    out.backward(case["dout"].to(F64))
    res = dict(out=out.detach(), P0=P0.detach(), P=P.detach(), dx=x.grad, dother=y.grad, g_bk=leaf["bk"].grad)
    res.update({g: leaf[g[2:]].grad for g in GRADS})
    return res


def peaked_fraction(ref):
    """Share of the softmax rows whose largest float64 probability exceeds 0.9."""
    return (ref["P0"].amax(-1) > 0.9).double().mean().item()


# ------------------------------------------------------------------------------------------------------------------------
# rounding model
# ------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("z_last_key", "c_no_mask", "c_no_bq", "bv_rowsum_one", "kprime_scale_twice", "t64_two_groups", "row_map", "truncate",
           "hidden_no_rescale", "dbq_no_dcb", "dy_no_dstq", "dx_no_residual")


def mutant_applies(mutant, case):
    """Where a mutant changes the computation at all.  Two properties of the key mask take mutants out: a sample-wise tail mask
    hides the LAST key (its probability is exactly 0 with or without the mutant), and where every sample keeps exactly one visible
    key that key's probability is 1 whatever the scores are and dS is exactly 0, so nothing that only moves scores or dS shows."""
    d, drop, mask = case["direction"], case["p"] > 0, case["mask"]
    masked = mask is not None
    visible = (mask == 0).sum(-1) if masked else None
    last_key_live = not masked or bool(((mask[:, -1] == 0) | (visible == 0)).any())
    one_key = masked and bool((visible == 1).all())
    return {"z_last_key": d == 0 and last_key_live, "dy_no_dstq": d == 0 and not one_key, "bv_rowsum_one": d == 0 and drop,
            "c_no_mask": d == 1 and masked, "c_no_bq": d == 1 and not one_key, "kprime_scale_twice": d == 1 and not one_key,
            "t64_two_groups": d == 1 and case["T"] == 64, "dbq_no_dcb": d == 1 and not one_key, "row_map": not one_key,
            "hidden_no_rescale": drop}.get(mutant, True)


def _layernorm_fwd_bwd(s, dout, ln_g, ln_b, eps, rnd, mul_h):
    """LayerNorm forward and backward on the bf16 pre-LayerNorm sum s (csrc/norm.hip): the statistics, dgamma and dbeta stay fp32;
    out is stored bf16 (m3ae_layernorm_fwd, the last call of m3ae_xattn_fwd); ds = ws_ds and dsd = ws_dsd are stored bf16 from the
    SAME fp32 value (`st4<T>(dx_drop + ...)` after drop_apply4 and `st4<T>(dx + ...)` in the backward kernel of norm.hip)."""
    mean = s.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((s - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (s - mean) * rstd
    out = rnd(xh * ln_g + ln_b)
    dxh = dout * ln_g
    ds32 = rstd * (dxh - dxh.mean(-1, keepdim=True) - xh * (dxh * xh).mean(-1, keepdim=True))
    ds = rnd(ds32)
    dsd = rnd(ds32 * mul_h) if mul_h is not None else ds
    return out, ds, dsd, (dout * xh).sum((0, 1)), dout.sum((0, 1))


def rounding_model(case, mutant=None, acc=F32):
    """fp32 torch of m3ae_xattn_fwd + m3ae_xattn_bwd with their bf16 roundings (csrc/xattn.hip unless another file is named; "rounded"
    = slab_put_bf16 / pack2bf of the fp32 accumulator after alpha, bias and dropout, i.e. one rounding of the finished value):

    direction 0 (text queries), forward
      proj         q = x Wq^T + bq: `dense_fwd(d, D, d.x, d.wq, d.bq, d.proj)`, bf16 C of m3ae_gemm.
      prime (Q')   scale q_h Wk_h, the scale BEFORE the rounding: `a.alpha = scale; launch_xbuild(a, H, s)`, xbuild_kernel's
                   `acc[i][j][0] * alpha` into slab_put_bf16.
      probs        XE_SOFTMAXROW: `v[r] = acc[i][j][r] * sm[i]` rounded; the mask is added to the fp32 score (`acc * a.alpha + c4[r]`).
      probs_drop   the same fp32 v after drop_apply4, rounded; rowsum = the fp32 sum of those values BEFORE the rounding (`dsum[i] +=`).
      zctx (Z)     drop(P) y: `launch_xg<128, 384, ..., XE_STORE>` rounded.
      ctx          Z_h Wv_h^T + rowsum bv: XE_STORE `fmaf(b4[r], rs, v[r])` rounded.
      s            dropout(ctx Wo^T + bo) + x: m3ae_gemm with `o.residual = d.x` and the dropout fields, one rounding at the end.
      out          m3ae_layernorm_fwd.
    direction 0, backward
      ws_ds / ws_dsd   m3ae_layernorm_bwd(_drop), see _layernorm_fwd_bwd.
      ws_dctx      dsd Wo: `dense_dgrad(d, D, dsd, d.wo_t, dctx)`.
      ws_dz (dZ)   dctx_h Wv_h: `launch_xbuild(a, H, s)` with alpha 1.
      dS           XE_DSOFT: `ds_[e] = p[e] * (dp[e] - dl)`, fp32 from the bf16 probs, dp = (acc + radd) dropped, dl = delta of
                   xattn_rowdot_kernel (fp32: dZ . Z + radd rowsum); rounded once (`pack2bf(ds_[0], ds_[1])`).
      ws_dprime    dQ' = dS y, XE_STORE.
      dy           drop(P)^T dZ + dS^T Q' in ONE accumulator (`a.A2 = dS; a.B2 = d.prime; a.k_switch = R / 32`), rounded once.
      ws_dproj     dq_h = scale dQ'_h Wk_h^T: XE_STORE with `a.alpha = scale`.
      dx           dq Wq + ds: `dense_dgrad(d, D, dq, d.wq_t, d.dx, d.ws_ds)`.
    direction 1 (image queries), forward
      proj         k | v = y Wkv^T + bkv: `dense_fwd(d, 2 * D, d.y, d.wkv, d.bkv, d.proj)`.
      prime        K' = scale k_h Wq_h (`a.alpha = scale`) and V' = v_h Wo[:, h]^T (`pr.alpha2 = 1.0f`): xbuild_kernel, or launch_xbuild
                   twice where dh != 64.
      colbias c    fp32: `s_ * pr.scale + pr.mask[m]` (xbuild_kernel) / `s_ * scale + mk` (xattn_colbias_kernel).
      probs        xf1_kernel (csrc/xflash.hip): `v[4 * t + r] * inv` into image_put(false)'s pack2bf; the fp32 score is acc + c.
      probs_drop   image_put(true): the same fp32 value after drop_apply4.
      s            dropout(drop(P) V' + bo) + x: the pass epilogue of xf1_kernel, one rounding (`pack2bf(x[0], x[1])`).
    direction 1, backward
      dS           XE_DSOFT without `delta`: dl = the fp32 sum of p dp over the head's T columns (`part = fmaf(p[e], dp[e], part)`).
      ws_dprime    dV' = drop(P)^T dsd and dK' = dS^T x: XE_STORE.
      dx           dS K' + ds: XE_DENSE with `a.residual = d.ws_ds`, one rounding.
      dcb          fp32: xattn_colsum_kernel sums the bf16 dS.
      ws_dproj     dk_h = scale dK'_h Wq_h^T + dcb bq_h (`a.alpha = scale; a.bias = d.bq; a.rowscale = dcb`) and dv_h = dV'_h Wo[:, h].
      dy           dkv Wkv: `dense_dgrad(d, 2 * D, dkv, d.wkv_t, d.dy)`.
    fp32 throughout: every accumulator, row sums, delta, radd, c, dcb, the LayerNorm statistics, all weight and bias gradients
    (XE_ATOMIC `atomicAdd(Cf + ...)`, dense_wgrad with `g.dtype_c = M3AE_F32`, xattn_headvec_kernel, m3ae_colsum).
    g_bk: direction 0 never computes it; direction 1 leaves it out of its bias-gradient column sums.  The model returns zeros.

    mutant: one of MUTANTS, a subtly wrong kernel for the host-side self-check; None is the model itself.
    acc: the dtype of everything between two roundings.  float64 gives the "exact accumulation" variant: the same bf16 roundings at
    the same places around exact sums -- a correct kernel with another accumulation order, which the criteria must let pass."""
    assert mutant is None or mutant in MUTANTS
    rnd32 = bf16_truncate if mutant == "truncate" else bf16_nearest
    rnd = rnd32 if acc == F32 else (lambda t: rnd32(t.to(F32)).to(acc))
    d0 = case["direction"] == 0
    B, T, I, D, H, p = (case[k] for k in ("B", "T", "I", "D", "H", "p"))
    dh = D // H
    x, y, dout = case["x"].to(acc), case["y"].to(acc), case["dout"].to(acc)
    dev = x.device
    scale = (1.0 / torch.sqrt(torch.tensor(float(dh), dtype=F32))).item()       # 1.0f / sqrtf((float)dh)
    drop = p > 0
    inv_keep = (1.0 / (torch.tensor(1.0, dtype=F32) - torch.tensor(p, dtype=F32))).item()
    mul_h = None
    if drop:
        mul_h = case["keep_h"].to(acc) * (1.0 if mutant == "hidden_no_rescale" else inv_keep)
    wq, wk, wv, wo = (case[n].to(acc) for n in ("wq", "wk", "wv", "wo"))
    bq, bv, bo, bk = (case[n].to(acc) for n in ("bq", "bv", "bo", "bk"))
    ln_g, ln_b = case["ln_g"].to(acc), case["ln_b"].to(acc)
    mask = case["mask"].to(acc) if case["mask"] is not None else None
    rows = lambda t: t.reshape(-1, t.shape[-1])
    res = {}

    if d0:
        wk_h, wv_h = wk.view(H, dh, D), wv.view(H, dh, D)
        mul = case["keep_a"].to(acc).permute(0, 2, 1, 3) * inv_keep if drop else None          # [B, T, H, I]
        proj = rnd(x @ wq.t() + bq)
        ph = proj.view(B, T, H, dh)
        Qp = rnd(torch.einsum("bthd,hdc->bthc", ph, wk_h) * scale)
        if mutant == "row_map":      # Q' written at rows h T + t, read at rows t H + h
            Qp = Qp.permute(0, 2, 1, 3).reshape(B, T, H, D)
        S = torch.einsum("bthc,bic->bthi", Qp, y)
        if mask is not None:
            S = S + mask[:, None, None, :]
        P32 = torch.softmax(S, -1)
        probs = rnd(P32)
        Pd = rnd(P32 * mul) if drop else probs
        rowsum = (P32 * mul).sum(-1) if drop else None
        if drop and mutant == "bv_rowsum_one":
            rowsum = torch.ones_like(rowsum)
        Pz = Pd
        if mutant == "z_last_key":
            Pz = Pd.clone()
            Pz[..., I - 1] = 0
        Z = rnd(torch.einsum("bthi,bic->bthc", Pz, y))
        ctx = torch.einsum("bthc,hdc->bthd", Z, wv_h)
        ctx = rnd(ctx + (rowsum[..., None] if drop else 1.0) * bv.view(H, dh)).reshape(B, T, D)
        dense = ctx @ wo.t() + bo
        s = rnd((dense * mul_h if drop else dense) + x)
        out, ds, dsd, res["g_ln_g"], res["g_ln_b"] = _layernorm_fwd_bwd(s, dout, ln_g, ln_b, case["eps"], rnd, mul_h)
        res["g_wo"], res["g_bo"] = rows(dsd).t() @ rows(ctx), rows(dsd).sum(0)
        dch = rnd(dsd @ wo).view(B, T, H, dh)
        dZ = rnd(torch.einsum("bthd,hdc->bthc", dch, wv_h))
        res["g_wv"] = torch.einsum("bthd,bthc->hdc", dch, Z).reshape(D, D)
        res["g_bv"] = ((rowsum[..., None] if drop else 1.0) * dch).sum((0, 1)).reshape(D)
        dP = torch.einsum("bthc,bic->bthi", dZ, y)
        delta = (dZ * Z).sum(-1)
        if drop:
            radd = (dch * bv.view(H, dh)).sum(-1)
            delta = delta + radd * rowsum
            dP = (dP + radd[..., None]) * mul
        dS = rnd(probs * (dP - delta[..., None]))
        dQp = rnd(torch.einsum("bthi,bic->bthc", dS, y))
        dy = torch.einsum("bthi,bthc->bic", Pd, dZ)
        if mutant != "dy_no_dstq":
            dy = dy + torch.einsum("bthi,bthc->bic", dS, Qp)
        res["dother"] = rnd(dy)
        dq = rnd(torch.einsum("bthc,hdc->bthd", dQp, wk_h) * scale).reshape(B, T, D)
        res["g_wk"] = (torch.einsum("bthd,bthc->hdc", ph, dQp) * scale).reshape(D, D)
        res["g_wq"], res["g_bq"] = rows(dq).t() @ rows(x), rows(dq).sum(0)
        res["dx"] = rnd(dq @ wq + (0.0 if mutant == "dx_no_residual" else ds))
        P_out, Pd_out = probs.permute(0, 2, 1, 3), Pd.permute(0, 2, 1, 3)
    else:
        wq_h, wo_h = wq.view(H, dh, D), wo.view(D, H, dh)
        mul = case["keep_a"].to(acc).permute(0, 2, 1, 3) * inv_keep if drop else None          # [B, I, H, T]
        kh = rnd(y @ wk.t() + bk).view(B, T, H, dh)
        vh = rnd(y @ wv.t() + bv).view(B, T, H, dh)
        Kp = rnd(torch.einsum("bjhd,hdc->bhjc", kh, wq_h) * (scale * scale if mutant == "kprime_scale_twice" else scale))
        Vp = rnd(torch.einsum("bjhd,nhd->bhjn", vh, wo_h))
        if mutant == "row_map":      # K' written at rows j H + h, read at rows h T + j
            Kp = Kp.permute(0, 2, 1, 3).reshape(B, H, T, D)
        c = torch.zeros(B, H, T, device=dev, dtype=acc) if mutant == "c_no_bq" else torch.einsum("bjhd,hd->bhj", kh, bq.view(H, dh)) * scale
        if mask is not None and mutant != "c_no_mask":
            c = c + mask[:, None, :]
        S = torch.einsum("bic,bhjc->bihj", x, Kp) + c[:, None]
        if mutant == "t64_two_groups" and T == 64:
            P32 = torch.softmax(S.view(B, I, H, 2, 32), -1).view(B, I, H, T)
        else:
            P32 = torch.softmax(S, -1)
        probs = rnd(P32)
        Pd = rnd(P32 * mul) if drop else probs
        dense = torch.einsum("bihj,bhjn->bin", Pd, Vp) + bo
        s = rnd((dense * mul_h if drop else dense) + x)
        out, ds, dsd, res["g_ln_g"], res["g_ln_b"] = _layernorm_fwd_bwd(s, dout, ln_g, ln_b, case["eps"], rnd, mul_h)
        res["g_bo"] = rows(dsd).sum(0)
        dP = torch.einsum("bin,bhjn->bihj", dsd, Vp)
        if drop:
            dP = dP * mul
        dS = rnd(probs * (dP - (probs * dP).sum(-1, keepdim=True)))
        dVp = rnd(torch.einsum("bihj,bin->bhjn", Pd, dsd))
        dKp = rnd(torch.einsum("bihj,bic->bhjc", dS, x))
        res["dx"] = rnd(torch.einsum("bihj,bhjc->bic", dS, Kp) + (0.0 if mutant == "dx_no_residual" else ds))
        dcb = dS.sum(1) * scale                                                                # [B, H, T]
        dk = rnd(torch.einsum("bhjc,hdc->bjhd", dKp, wq_h) * scale + dcb.permute(0, 2, 1)[..., None] * bq.view(H, dh)).reshape(B, T, D)
        dv = rnd(torch.einsum("bhjn,nhd->bjhd", dVp, wo_h)).reshape(B, T, D)
        res["g_wq"] = (torch.einsum("bjhd,bhjc->hdc", kh, dKp) * scale).reshape(D, D)
        res["g_wo"] = torch.einsum("bhjn,bjhd->nhd", dVp, vh).reshape(D, D)
        res["g_bq"] = torch.zeros(D, device=dev, dtype=acc) if mutant == "dbq_no_dcb" else torch.einsum("bhj,bjhd->hd", dcb, kh).reshape(D)
        res["g_wk"], res["g_wv"], res["g_bv"] = rows(dk).t() @ rows(y), rows(dv).t() @ rows(y), rows(dv).sum(0)
        res["dother"] = rnd(dk @ wk + dv @ wv)
        P_out, Pd_out = probs.permute(0, 2, 1, 3), Pd.permute(0, 2, 1, 3)
    res.update(out=out, P0=P_out, P=Pd_out, g_bk=torch.zeros(D, device=dev, dtype=acc))
    return res


# ------------------------------------------------------------------------------------------------------------------------
# criteria: the GPU tests and the host-side self-check run the SAME code on a candidate's result (a dict like the model's)
# ------------------------------------------------------------------------------------------------------------------------
def yardsticks(case):
    """(reference, rounding model) of the case as it stands, computed once and left unchanged."""
    if "_ref" not in case:
        assert case["p"] == 0 or (case["keep_a"] is not None and case["keep_h"] is not None)
        case["_ref"], case["_model"] = reference(case), rounding_model(case)
    return case["_ref"], case["_model"]


def ln_bias_excess(got, case):
    """d(LayerNorm bias) is the column sum of the bf16 dout over the M = B Lq rows: an fp32 sum with no bf16 rounding anywhere, so the
    rounding model has nothing to say about it -- its error and the kernel's are both the noise of an fp32 summation order.  It is
    held to the first-order bound of an M-term fp32 sum in ANY order, |err| <= M u sum|dout| with u = 2^-24 (the form of
    tests/norm_accuracy.py) plus one rounding of the result.  Returns the worst |err| / bound over the columns (NaN fails)."""
    dout = case["dout"].to(F64).reshape(-1, case["D"])
    ref = dout.sum(0)
    bound = 2.0 ** -24 * (dout.shape[0] * dout.abs().sum(0) + ref.abs())
    ratio = (got.to(F64).to(ref.device) - ref).abs() / bound.clamp_min(1e-300)
    return ratio.max().item() if bool(torch.isfinite(ratio).all()) else math.inf


def check_budget(got, case, label, figures=None, names=TENSORS):
    """The names of the tensors of `got` that miss within_budget (empty = pass); prints every figure."""
    ref, model = yardsticks(case)
    bad = []
    for n in names:
        if n == "g_ln_b":
            worst = ln_bias_excess(got[n], case)
            print(f"[xattn-accuracy] {label} {n}: worst |err| / (M u sum|dout|) {worst:.3f}{'' if worst <= 1.0 else '  OVER BOUND'}")
            if not worst <= 1.0:
                bad.append(n)
            continue
        ok, (rg, rm, mg, mm) = within_budget(got[n], model[n], ref[n])
        print(f"[xattn-accuracy] {label} {n}: rel_rms {rg:.3e} (model {rm:.3e}, ratio {rg / rm if rm else math.nan:.2f}) "
              f"max_abs {mg:.3e} (model {mm:.3e}, ratio {mg / mm if mm else math.nan:.2f}){'' if ok else '  OVER BUDGET'}")
        if figures is not None:
            figures.setdefault(n, []).append((rg, rm, mg, mm))
        if not ok:
            bad.append(n)
    return bad


P_LIVE = 1e-36      # entries above it carry a meaningful relative error in fp32 and bf16 (normal numbers start near 1.2e-38)
P_ABS = 1e-37


def check_probs(got, case, label, figures=None):
    """The saved probabilities entry by entry, the undropped P0 and the dropped, rescaled P (kept entries carry 1 / (1 - p)):
        |P - P_ref| <= (MAX_FACTOR r + EPS) P_ref + P_ABS,   r = the model's largest relative entrywise error on that softmax row
    (over the row's entries above P_LIVE), EPS P_ref one bf16 rounding of the entry itself; entries whose reference is exactly 0
    (keys at -10000 next to visible ones) and entries the keep mask drops must be exactly 0.
    Why the model's error enters per ROW and relative: a probability's error is its own score's error minus the row's weighted mean,
    times the probability -- multiplicative, and of one size along a row.  Taken per ENTRY it has zeros of its own: wherever the
    model's bf16 roundings happen to cancel, a correct kernel whose fp32 sums run in another order (and so rounds a few Q' / K'
    elements the other way) is left with EPS P alone; the exact-accumulation variant of the model misses that form by about 2 x
    (tests/test_xattn_accuracy_host.py), the kernels by up to 4.7 x.  Returns the failures (empty = pass)."""
    ref, model = yardsticks(case)
    bad = []
    for n in ("P0", "P") if case["p"] > 0 else ("P0",):
        g, r, m = got[n].to(F64), ref[n], model[n].to(F64)
        live = r > P_LIVE
        rel = torch.where(live, (m - r).abs() / r.clamp_min(P_LIVE), torch.zeros_like(r)).amax(-1, keepdim=True)
        bound = (MAX_FACTOR * rel + EPS) * r + torch.where(r > 0, P_ABS, 0.0)
        err = (g - r).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item() if bool((bound > 0).any()) else 0.0
        ok = bool((err <= bound).all())                    # NaN fails
        print(f"[xattn-accuracy] {label} {n} entry by entry: worst |err| / bound {worst:.3f}, largest |err| {err.max().item():.3e}, "
              f"largest relative error of the model {rel.max().item():.3e}{'' if ok else '  OVER BOUND'}")
        if figures is not None:
            figures.setdefault(n, []).append(worst)
        if not ok:
            bad.append(n + " entries")
    if case["p"] > 0 and not bool((got["P"][case["keep_a"] == 0] == 0).all()):
        print(f"[xattn-accuracy] {label} P: non-zero entries where the keep mask drops")
        bad.append("P dropped entries")
    return bad


def criteria(got, case, label, figures=None):
    return check_budget(got, case, label, figures) + check_probs(got, case, label, figures)
