"""Yardsticks of the streaming kernels of csrc/misc.hip (column sums, embeddings, ViT patches / tokens, casts, adds, transposes,
row gather / scatter, dropout, the MIM bookkeeping, the stand-alone activations, the uint8 image normalisation), shared by
tests/test_gpu_misc_accuracy.py and its host-side self-check tests/test_misc_accuracy_host.py.  numpy / torch only: nothing here
imports or calls the library.  U, rne_bf16, _store_bound, FENCE and the activation helpers are those of tests/gemm_accuracy.py; the
fenced buffers here are flat and carry FENCE in front of the output as well as behind it (fenced_flat).

EXACT TIER.  Kernels whose every operation and its order are fixed by the code have one right answer, bit for bit:
  cast            f32 -> bf16: rne_bf16 (NaN stays NaN, the largest finite fp32 rounds to inf, denormals round as any value);
                  bf16 -> f32 and the same-type forms: the bits themselves.
  add             fl32(a + b), then rne_bf16 for bf16 (two roundings: the sum of two bf16 values 17 or more binades apart is
                  not an fp32 value).
  gather / scatter  out[i] = in[idx[i]] (the bits: NaN payloads, -0);  d_in[idx[i]] = fl(d_in[idx[i]] + d_out[i]) for DISTINCT idx.
  patchify        the bits of img in (c, py, px) order (torch's unfold), rne_bf16 for bf16.
  embed forward   fl(fl(word[id] + type[0]) + pos[pid]), pid = (number of non-pad tokens up to and including s) if id != pad else
                  pad; then rne_bf16.
  ViT tokens      forward fl(base + pos), base = cls or the patch row; backward: d_patch the bits of d_out[:, 1:], d_pos[l] =
                  fl(old + acc), acc = the fp32 sum over b = 0, 1, ... in that order starting from 0 (d_cls: row 0 of the same).
  transposes      out_t = rne_bf16(in).t(), out = rne_bf16(in).
  mask_ranks      ranks = the stable argsort of the stable argsort (ties by index; -0 == +0 is a tie, +inf sorts last).
  MIM target      without norm_pix the bits of img in (p, q, c) order.
  dropout         keep(row, col) as csrc/common.h states it (keep_mask_model below); out = fl(x inv_keep), inv_keep =
                  fl32(1 / fl32(1 - p)), +0 where dropped; rne_bf16 for bf16.
  sums of small integers (|x| <= 8, exact in bf16): every partial sum of up to 2^24 / 8 terms is an integer below 2^24, so every
                  order gives the same bits.  This is the exact tier of the column sums and of the embedding backward.

BOUNDED TIER.  float64 references from the exact fp32 / bf16 values the kernel reads; element-wise bounds of first order in
u = U = 2^-24, valid for ANY order of summation (an n-term fp32 sum is within n u sum|t_i| of the exact sum):
  column sum      M u sum_m|x| + u |sum|, plus u |old + sum| when accumulating.  (old joins in one add per workgroup (atomic form) or
                  one add in all (ordered form); the cases keep |old| <= 8, far inside the M roundings the first term grants and of
                  which a kernel spends M / 8 + 8 + the number of workgroups.)
  image_normalize q = u8 / 255: u |q|;  d = q - mean: e_d = u |q| + u |d|;  out = d / std: e_d / |std| + u |out|.
  MIM target (norm_pix)  tests/norm_accuracy.py's forward chain with n = D, the divisor D - 1 in the variance, eps = 1e-6, no affine:
                  e_mean = u sum|x| + u |mean|;  e_d = e_mean + u |d|;  e_q = (n + 3) u (q + n e_mean^2) + n e_mean^2;
                  var = q / (n - 1): e_var = e_q / (n - 1) + u var;  v = var + eps: e_v = e_var + u v;
                  e_rstd = rstd (e_v / (2 (v - e_v)) + 4 u);  y = d rstd: e_d rstd + |d| e_rstd + e_d e_rstd + u |y|.
                  A constant patch of a small integer has exact sums: mean = the constant, d = 0, y = 0 exactly.
  MIM loss        e = x - t: u |e|;  e^2: 3 u e^2;  ss = sum_d e^2: e_ss = (D + 3) u ss;  row = m ss / D: e_row = m e_ss / D + 2 u row;
                  num = sum of the masked rows: sum e_row + R u num, R = the number of masked rows;  den = sum m, an integer: exact;
                  loss = num / den: e_num / den + u |loss|.
                  gradient k = gout 2 m / (D den) (three roundings), (x - t) one, the product one: 5 u |dx|, then the store.
                  Class rows and unmasked rows are exact zeros.
  act_fwd / act_bwd  y = act(x): _eval_act(x, act) of tests/gemm_accuracy.py, whose docstring states that the figures cover the libm
                  forms (erff / expf / tanhf) csrc/common.h's act_fwd / act_bwd call; dx = dy act'(x): |dy| _eval_grad(x, act) + u |dx|;
                  then the store (_store_bound).  ACT_NONE, ACT_RELU and ACT_MULAUX are exact up to the one product.
                  The grid holds denormals, where a rounding errs by half the FIXED spacing of the format and not by u |x|: the
                  bounds add the formats' floors, 2^-149 for each of up to four fp32 roundings of a denormal result (FLOOR32) and
                  2^-134, half the spacing of the bf16 denormals, for a bf16 store (FLOOR16).
Aggregate yardstick for the column sums of data of ONE SIGN (the mean-64 cases; tensors of at least MIN_COLS columns, so that an rms
means something): against the numpy fp32 model that adds the rows strictly one after the other,
    rms(got - ref) <= RMS_FACTOR rms(sequential - ref),   max|got - ref| <= MAX_FACTOR max|sequential - ref|.
With terms of one sign the running sum grows with every term and each of the M roundings is taken at its size: no order a kernel
could use is less accurate.  (For zero-mean data this does not hold: every rounding is taken at about the size of the final sum
in any order, so the 207 atomic adds of the whole-row form at 4133 x 768 err as much as the 4133 adds of the sequential model, and
only the element-wise bound is asserted there.)  At mean 64 the element-wise bound is 64 M^2 u -- more than one whole row -- and it
is this yardstick that sees a dropped row.

Measured headroom (tests/test_misc_accuracy_host.py prints it): worst model / bound over every bounded case, pairwise and sequential
model: column sums 0.64 and 0.64 (the one-row accumulating case, where the bound is three roundings and the model spends one; below
0.01 from 70 rows on; the pairwise model reaches 0.07 x the sequential model's rms and max at mean 64), image_normalize 0.945 (no sums:
one model), MIM target 0.07 and 0.18, MIM loss 0.02 and 0.08, MIM gradient 1.00 (a bf16 store on a tie spends the whole store
rounding), act_fwd and act_bwd 1.00 (a bf16 store of a denormal on a tie: exactly FLOOR16)."""
import math

import numpy as np
import torch

from attn_accuracy import MAX_FACTOR
from gemm_accuracy import (ACT_GELU, ACT_MULAUX, ACT_NONE, ACT_QUICKGELU, ACT_RELU, ACT_TANH, FENCE, RMS_FACTOR, U, _eval_act, _eval_grad,  # noqa: F401
                           _store_bound, act_grad, act_value, bf16_half_up, bf16_truncate, rne_bf16)

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
f32 = np.float32
ACTS = (ACT_NONE, ACT_GELU, ACT_QUICKGELU, ACT_TANH, ACT_RELU, ACT_MULAUX)
MIN_COLS = 512
INT_MAX = 8   # |x| <= 8: exact in bf16, and 2^24 / 8 terms sum exactly in any order


# ------------------------------------------------------------------------------------------------------------------------
# fences (in front and behind) and bit comparison
# ------------------------------------------------------------------------------------------------------------------------
def fence_value(dtype):
    return FENCE if dtype.is_floating_point else (0xA5 if dtype == torch.uint8 else -24576)


def fenced_flat(n, dtype, device="cpu", offset=0, front=64, back=64):
    """(buffer, view of n elements) with front + offset fence elements in front of the view and at least `back` behind it.  front
    = 64 elements keeps the view 16-byte aligned for every dtype when offset = 0."""
    buf = torch.full((front + offset + n + back,), fence_value(dtype), dtype=dtype, device=device)
    return buf, buf[front + offset:front + offset + n]


def flat_fence_intact(buf, view, msg=""):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    v = fence_value(buf.dtype)
    assert bool((buf[:lo] == v).all()), f"{msg}: written in front of the output"
    assert bool((buf[lo + view.numel():] == v).all()), f"{msg}: written behind the {view.numel()} output elements"


def bits_differ(got, want):
    """Number of elements whose raw bits differ; a NaN matches any NaN."""
    g, w = got.contiguous().reshape(-1), want.contiguous().reshape(-1).to(got.device)
    assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
    if g.is_floating_point():
        gn, wn = torch.isnan(g), torch.isnan(w)
        word = {2: torch.int16, 4: torch.int32, 8: torch.int64}[g.element_size()]
        return int(((g.view(word) != w.view(word)) & ~(gn & wn)).sum())
    return int((g != w).sum())


def store(x, bf16, mutant=None):
    """The stored value of an fp32 result, returned as an fp32 tensor (bf16: rounded to nearest even)."""
    if not bf16:
        return x.float()
    return {"store_truncates": bf16_truncate, "store_half_up": bf16_half_up}.get(mutant, rne_bf16)(x.float())


def small_ints(shape, seed, dtype=F32, lo=-INT_MAX, hi=INT_MAX):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


# ------------------------------------------------------------------------------------------------------------------------
# dropout keep mask: csrc/common.h (make_drop / drop_resolve / drop_hash / drop_keep) in numpy uint32 / uint64
# ------------------------------------------------------------------------------------------------------------------------
MASK_MUTANTS = ("rotation_reversed", "group_high_word_ignored", "ld_is_cols")
P_BELOW_ONE = float(np.nextafter(f32(1), f32(0)))
DROP_PS = (0.1, 0.5, P_BELOW_ONE)
DROP_COLS = (4, 577, 768)
DROP_ROW_MAPS = ((0, 1), (3, 5), (2 ** 40, 1))
DROP_SALTS = (None, 0, 12345)
DROP_SEED = 0x5EED1234ABCD9876
DROP_BIG = (2731, 768)   # 2731 x 768 = 2^21 + 256 elements: past one sweep of 8192 x 256 threads


def lowbias32(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def drop_threshold(p):
    t = float(f32(p)) * 4294967296.0   # the host's double product of the fp32 p
    return 4294967295 if t >= 4294967295.0 else int(t)


def inv_keep(p):
    return f32(1) / (f32(1) - f32(p)) if p > 0 else f32(1)


def keep_mask_model(rows, cols, p, seed, row_base=0, row_step=1, salt=None, mutant=None):
    """uint8 [rows, cols]: 1 where element (row, col) of the call is kept."""
    key_lo, key_hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    if salt is not None:
        key_hi = (key_hi + salt * 0x85EBCA6B) & 0xFFFFFFFF
    ld = cols if mutant == "ld_is_cols" else (cols + 3) & ~3
    r = np.uint64(row_base) + np.arange(rows, dtype=np.uint64) * np.uint64(row_step)
    idx = r[:, None] * np.uint64(ld) + np.arange(cols, dtype=np.uint64)[None, :]
    g = idx >> np.uint64(2)
    lo = (g & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = np.zeros_like(lo) if mutant == "group_high_word_ignored" else (g >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):
        h = lowbias32((lo ^ np.uint32(key_lo)) + hi * np.uint32(0x9E3779B9) + np.uint32(key_hi))
    j = (idx & np.uint64(3)).astype(np.uint32)
    rot = np.uint32(8) * ((np.uint32(3) - j) if mutant == "rotation_reversed" else j)
    rotated = (h >> rot) | (h << ((np.uint32(32) - rot) & np.uint32(31)))
    return (rotated >= np.uint32(drop_threshold(p))).astype(np.uint8)


def dropout_model(x, keep, p, bf16, mutant=None):
    y = (x.float() * float(inv_keep(p))).float()
    return torch.where(keep.bool(), store(y, bf16, mutant), torch.zeros_like(y))


# ------------------------------------------------------------------------------------------------------------------------
# exact tier: values and models
# ------------------------------------------------------------------------------------------------------------------------
CAST_SIZES = (1, 255, 257, 2 ** 21 + 259)
FLT_MAX = 3.4028234663852886e38
SPECIALS = (1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8),   # bf16 ties: to 1.0 (even) / up to 1.015625
            0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -134, 3 * 2.0 ** -134,   # fp32 denormals (ties too)
            FLT_MAX, -FLT_MAX, math.inf, -math.inf, math.nan, 3.3895313892515355e38, 1.0, -2.5)


def cast_values(n, seed=0):
    """fp32 values of a cast case: the specials at the head AND the tail (the tail of the largest size is moved by the grid-stride
    loop's second pass), Gaussians between."""
    g = torch.Generator().manual_seed(1000 + seed)
    v = torch.randn(n, generator=g)
    sp = torch.tensor(SPECIALS, dtype=F32)
    k = min(n, sp.numel())
    v[:k] = sp[:k]
    v[n - k:] = sp[:k].flip(0)
    return v


def cast_model(src, to_bf16, mutant=None):
    return store(src.float(), True, mutant).to(BF) if to_bf16 else src.float()


ADD_SIZES = (2048, 2051, 2 ** 21 * 8 + 8)


def add_values(n, bf16, seed=0):
    """(a, b) in the storage dtype.  Heads: sums on bf16 ties of both parities; b 2^-20 of a: a sum that is no fp32 value for fp32
    operands (one rounding) and far below half a bf16 ulp for bf16 ones."""
    g = torch.Generator().manual_seed(2000 + seed + n % 1000)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n >= 8:
        a[:4] = torch.tensor([1.0, 1.0078125, -1.0, -1.0078125])
        b[:4] = torch.tensor([2.0 ** -8, 2.0 ** -8, -2.0 ** -8, -2.0 ** -8])
        a[4:8], b[4:8] = a[:4], b[:4] * 2.0 ** -12
        a[n - 4:], b[n - 4:] = a[:4], b[:4]
    dt = BF if bf16 else F32
    return a.to(dt), b.to(dt)


def add_model(a, b, bf16, mutant=None):
    return store(a.float() + b.float(), bf16, mutant)


def position_ids(ids, pad_id, mutant=None):
    """int64 [B, S]: the serial scan of roberta_embed_fwd_kernel."""
    ids = ids.cpu().numpy()
    out = np.empty_like(ids)
    for b in range(ids.shape[0]):
        run = 0
        for s in range(ids.shape[1]):
            ne = int(ids[b, s] != pad_id)
            run += 1 if mutant == "pad_advances_position" else ne
            out[b, s] = run * ne + pad_id
    return torch.from_numpy(out)


def embed_fwd_model(ids, word, pos, typ, pad_id, bf16, mutant=None):
    """fp32 [B, S, D] holding the stored values."""
    pid = position_ids(ids, pad_id, mutant).to(word.device)
    return store((word[ids] + typ[0]) + pos[pid], bf16, mutant)


def embed_bwd_reference(ids, d_out, d_word, d_pos, d_type, pad_id):
    """float64 (d_word, d_pos, d_type) after the call; exact for integer operands."""
    pid = position_ids(ids, pad_id).to(d_out.device).reshape(-1)
    d = d_out.reshape(-1, d_out.shape[-1]).to(F64)
    w = d_word.to(F64).index_add(0, ids.reshape(-1), d)
    p = d_pos.to(F64).index_add(0, pid, d)
    return w, p, d_type.to(F64) + d.sum(0)


EMBED_FWD_D = (130, 768)
EMBED_VOCAB, EMBED_POS_ROWS = 64, 514


def embed_tables(D, seed=0):
    """(word [EMBED_VOCAB, D], pos [EMBED_POS_ROWS, D], type [1, D]) on a 2^-9 grid: the three-term sums land on bf16 ties of both
    parities."""
    g = torch.Generator().manual_seed(40 + D + seed)
    grid = lambda *s: torch.randint(-1024, 1025, s, generator=g).float() * 2.0 ** -9   # noqa: E731
    return grid(EMBED_VOCAB, D), grid(EMBED_POS_ROWS, D), grid(1, D)


def embed_fwd_cases():
    """name -> (ids [B, S], pad_id)."""
    g = torch.Generator().manual_seed(77)
    out = {}
    for pad in (1, 0):
        tok = lambda *s: torch.randint(2, EMBED_VOCAB, s, generator=g)   # noqa: E731  (never the pad id)
        out[f"full-512-pad{pad}"] = (tok(1, 512), pad)
        ids = tok(3, 40)
        ids[0, 33:], ids[1, 1:], ids[2, 39:] = pad, pad, pad
        out[f"pads-at-the-end-pad{pad}"] = (ids, pad)
        ids = tok(2, 40)
        ids[0, 5], ids[0, 17:20], ids[1, 0], ids[1, 38] = pad, pad, pad, pad
        out[f"pads-in-mid-sequence-pad{pad}"] = (ids, pad)
        ids = tok(3, 24)
        ids[1, :] = pad
        out[f"all-pad-sample-pad{pad}"] = (ids, pad)
        out[f"one-token-pad{pad}"] = (torch.tensor([[5], [pad], [7]]), pad)
    return out


EMBED_BWD_D = (300, 2048)
EMBED_BWD_REFUSED_D = 2049


def embed_bwd_cases():
    """name -> (ids [B, S] with B S = 300, pad_id)."""
    g = torch.Generator().manual_seed(78)
    rnd = torch.randint(2, 12, (3, 100), generator=g)          # ten ids over 300 tokens: every id repeats across the 256-token block
    padded = rnd.clone()
    padded[0, 60:], padded[2, 97:], padded[1, 10] = 1, 1, 1
    return {"one-id": (torch.full((3, 100), 5), 1), "repeats": (rnd, 1), "padded": (padded, 1)}


def vit_fwd_model(patch, cls, pos, bf16, mutant=None):
    """patch [B, G, D] (storage dtype), cls [D], pos [G + 1, D] fp32 -> fp32 [B, G + 1, D] holding the stored values."""
    B = patch.shape[0]
    base = torch.cat([cls[None, None, :].expand(B, 1, -1), patch.float()], 1)
    return store(base + pos[None], bf16, mutant)


def vit_bwd_model(d_out, d_cls, d_pos):
    """(d_patch in the storage dtype, d_cls, d_pos fp32) after the call: ascending-b fp32 sum, then one add onto the old contents."""
    acc = torch.zeros_like(d_pos)
    for b in range(d_out.shape[0]):
        acc = acc + d_out[b].float()
    return d_out[:, 1:].contiguous(), d_cls + acc[0], d_pos + acc


def scatter_add_model(d_out, idx, d_in, bf16, mutant=None):
    """d_in after d_in[idx[i]] = store(d_in[idx[i]] + d_out[i]) for i = 0, 1, ...: fp32 tensor of the stored values."""
    out = d_in.float().clone()
    for i, r in enumerate(idx.tolist()):
        out[r] = store(out[r] + d_out[i].float(), bf16, mutant)
    return out


def patchify_reference(img, P):
    """[B, G, 3 P P] fp32 by torch's unfold: column order (c, py, px), patches row-major over the grid."""
    return torch.nn.functional.unfold(img, kernel_size=P, stride=P).transpose(1, 2).contiguous()


PATCHIFY_SHAPES = ((32, 16), (16, 8), (8, 4), (12, 3))   # (R, P): P % 8 == 0 takes the 16-byte bf16 form


def mim_patches_reference(img, P):
    """[N, h w, P P C]: element order (p, q, c)."""
    N, C, H, W = img.shape
    h, w = H // P, W // P
    return img.reshape(N, C, h, P, w, P).permute(0, 2, 4, 3, 5, 1).reshape(N, h * w, P * P * C).contiguous()


MIM_TARGET_SHAPES = ((3, 32, 48, 16), (1, 8, 8, 4), (3, 24, 24, 4))   # (C, H, W, P): D = 768 non-square, 16, 48


def transpose_model(src, tile, mutant=None):
    """(out, out_t) as fp32 holding the stored bf16 values; tile: the kernel's tile edge.  The mutant tests an edge tile's elements
    against the bounds of the other axis: what it does not write keeps FENCE."""
    v = rne_bf16(src.float())
    if mutant != "edge_tile_bounds_swapped":
        return v, v.t().contiguous()
    R, C = v.shape
    r, c = torch.arange(R)[:, None], torch.arange(C)[None, :]
    inner = (r // tile < R // tile) & (c // tile < C // tile)
    ok = inner | ((r < C) & (c < R))
    return v, torch.where(ok, v, torch.full_like(v, FENCE)).t().contiguous()


TRANSPOSE_SHAPES = ((1, 1), (8, 8), (64, 64), (72, 64), (64, 72), (63, 65), (130, 66), (128, 192))


def ranks_model(noise, len_keep, mutant=None):
    """(ids_restore int64 [B, L], mask fp32 [B, L], keep_rows int64 [B, len_keep + 1]) by counting, as mask_ranks_kernel does."""
    x = noise.cpu().numpy().astype(np.float32)
    B, L = x.shape
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    ranks = np.empty((B, L), np.int64)
    for b in range(B):
        u, v = x[b][:, None], x[b][None, :]
        tie = (i > j) if mutant == "unstable_tie_break" else (i < j)
        ranks[b] = ((u < v) | ((u == v) & tie)).sum(0)
    keep = np.full((B, len_keep + 1), -1, np.int64)
    keep[:, 0] = np.arange(B) * (L + 1)
    for b in range(B):
        for jj in range(L):
            if ranks[b, jj] < len_keep:
                keep[b, 1 + ranks[b, jj]] = b * (L + 1) + 1 + jj
    return torch.from_numpy(ranks), torch.from_numpy((ranks >= len_keep).astype(np.float32)), torch.from_numpy(keep)


def ranks_reference(noise, len_keep):
    """The same three by the stable double argsort of random_masking."""
    B, L = noise.shape
    shuffle = torch.argsort(noise.double(), dim=1, stable=True)
    restore = torch.argsort(shuffle, dim=1, stable=True)
    keep = torch.cat([torch.zeros(B, 1, dtype=torch.int64), 1 + shuffle[:, :len_keep]], 1) + torch.arange(B)[:, None] * (L + 1)
    return restore, (restore >= len_keep).float(), keep


RANK_L = (1, 36, 576, 1000)


def rank_noise(L, seed=0):
    """[5, L]: all-equal, with ties, with +-0, with +inf, plain uniform."""
    g = torch.Generator().manual_seed(300 + L + seed)
    x = torch.rand(5, L, generator=g)
    x[0] = 0.25
    x[1] = torch.randint(0, max(L // 4, 1), (L,), generator=g).float() / 8
    x[2, ::2] = 0.0
    x[2, 1::4] = -0.0
    x[2] = x[2] - 0.5 * (torch.rand(L, generator=g) < 0.3).float() * (x[2] != 0).float()
    x[3, ::3] = math.inf
    return x


# ------------------------------------------------------------------------------------------------------------------------
# bounded tier: references, bounds, fp32 models
# ------------------------------------------------------------------------------------------------------------------------
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
    return np.ascontiguousarray(t.detach().float().cpu().numpy())


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def check_bound(got, ref, bnd, name, figures=None):
    """None, or the description of the first violation of |got - ref| <= bnd (every element; a non-finite output is one)."""
    got = (_t(got) if isinstance(got, np.ndarray) else got).detach().to(ref.device).to(F64).reshape(ref.shape)
    if not torch.isfinite(got).all():
        return f"{name}: non-finite output ({int((~torch.isfinite(got)).sum())} of {got.numel()})"
    err = (got - ref).abs()
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    if figures is not None:
        figures["err/bound"] = max(figures.get("err/bound", 0.0), ratio.max().item())
    bad = err > bnd
    if bad.any():
        i = torch.nonzero(bad.reshape(-1))[0].item()
        return (f"{name}: bound violated, worst err / bound {ratio.max().item():.3f}, first at flat index {i} (got {got.reshape(-1)[i].item()!r}, "
                f"reference {ref.reshape(-1)[i].item()!r}, bound {bnd.reshape(-1)[i].item():.3e}), {int(bad.sum())} of {bad.numel()} bad")
    return None


def check_yardstick(got, seq, ref, name, figures=None):
    """rms and max error of `got` against those of the sequential model (tensors of at least MIN_COLS elements)."""
    if ref.numel() < MIN_COLS:
        return None
    to = lambda a: (_t(a) if isinstance(a, np.ndarray) else a).detach().to(ref.device).to(F64).reshape(ref.shape)   # noqa: E731
    eg, es = (to(got) - ref).abs(), (to(seq) - ref).abs()
    rms = lambda e: math.sqrt((e * e).mean().item())   # noqa: E731
    rg, rs, mg, ms = rms(eg), rms(es), eg.max().item(), es.max().item()
    r_rms = rg / rs if rs > 0 else (0.0 if rg == 0 else math.inf)
    r_max = mg / ms if ms > 0 else (0.0 if mg == 0 else math.inf)
    if figures is not None:
        figures["rms/seq"] = max(figures.get("rms/seq", 0.0), r_rms)
        figures["max/seq"] = max(figures.get("max/seq", 0.0), r_max)
    if not r_rms <= RMS_FACTOR:
        return f"{name}: rms error {rg:.3e} = {r_rms:.3f} x the sequential model's {rs:.3e}, budget {RMS_FACTOR}"
    if not r_max <= MAX_FACTOR:
        return f"{name}: max error {mg:.3e} = {r_max:.3f} x the sequential model's {ms:.3e}, budget {MAX_FACTOR}"
    return None


# ---- column sums ----
COLSUM_MUTANTS = ("last_row_dropped", "last_column_group_dropped")
COLSUM_SMALL = ((70, 264), (1, 8), (70, 259), (33, 1), (4095, 768))            # the 256-column forms (vector: N % 8 == 0; else scalar)
COLSUM_ROWS = tuple((4096 + 37, N) for N in (8, 520, 768, 4096))               # the whole-row form: P = N / 8, R = 512 // P
COLSUM_SHAPES = COLSUM_SMALL + COLSUM_ROWS


def colsum_rows_geometry(M, N):
    """(P, R, rows per workgroup, workgroups) of colsum_rows_kernel as colsum_impl derives them."""
    P = N // 8
    R = 512 // P
    per = -(-(-(-M // 2048)) // (4 * R)) * 4 * R
    return P, R, per, -(-M // per)


def colsum_inputs(M, N, kind, bf16, seed=0):
    """x [M, N] in the storage dtype and old [N] fp32.  kind: 'ints' (exact tier) | 'mean0' | 'mean64'."""
    g = torch.Generator().manual_seed(500 + 7 * M + N + seed)
    if kind == "ints":
        return small_ints((M, N), 500 + M + N + seed, BF if bf16 else F32), small_ints((N,), 900 + N + seed)
    x = torch.randn(M, N, generator=g) + (64.0 if kind == "mean64" else 0.0)
    return x.to(BF if bf16 else F32), small_ints((N,), 900 + N + seed)


def colsum_reference(x, old=None):
    """(float64 reference [N], bound [N]); old: the previous contents when accumulating."""
    x = x.to(F64)
    M = x.shape[0]
    s = x.sum(0)
    bnd = M * U * x.abs().sum(0) + U * s.abs()
    if old is not None:
        s = s + old.to(F64).to(s.device)
        bnd = bnd + U * s.abs()
    return s, bnd


def colsum_model(x, old=None, order="seq", mutant=None):
    a = np32(x)
    if mutant == "last_row_dropped":
        a = a[:-1] if a.shape[0] > 1 else np.zeros_like(a)
    s = SUMS[order](a.T)
    if mutant == "last_column_group_dropped":
        s = s.copy()
        s[-8:] = 0
    return s if old is None else (np32(old) + s).astype(f32)


def colsum_misses(got, x, old, seq=None, figures=None, name="colsum", exact=False):
    ref, bnd = colsum_reference(x, old)
    if exact:   # integer operands: the reference is an fp32 value and the only right answer
        n = bits_differ(torch.as_tensor(got).float().to(ref.device), ref.float())
        return [f"{name}: {n} of {ref.numel()} exact integer sums differ"] if n else []
    out = [check_bound(got, ref, bnd, name, figures)]
    if seq is not None and out[0] is None:
        out.append(check_yardstick(got, seq, ref, name, figures))
    return [o for o in out if o]


# ---- uint8 image normalisation ----
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
NORMALIZE_SHAPE = (8, 5, 7)   # B, H, W: 280 pixels, the fewest 5 x 7 images in which a channel can take all 256 byte values


def normalize_input():
    """uint8 [B, H, W, 3] in which every channel takes all 256 byte values."""
    B, H, W = NORMALIZE_SHAPE
    px = torch.arange(B * H * W).reshape(B, H, W, 1)
    return ((px * 37 + torch.arange(3) * 85) % 256).to(torch.uint8)


def normalize_reference(u8):
    """(float64 [B, 3, H, W], bound) with the fp32 values of mean / std."""
    x = u8.permute(0, 3, 1, 2).to(F64)
    m = torch.tensor([float(f32(v)) for v in CLIP_MEAN], dtype=F64, device=x.device)[None, :, None, None]
    s = torch.tensor([float(f32(v)) for v in CLIP_STD], dtype=F64, device=x.device)[None, :, None, None]
    q = x / 255.0
    d = q - m
    out = d / s
    return out, (U * q.abs() + U * d.abs()) / s.abs() + U * out.abs()


def normalize_model(u8):
    x = np32(u8.permute(0, 3, 1, 2))
    m = np.array(CLIP_MEAN, f32)[None, :, None, None]
    s = np.array(CLIP_STD, f32)[None, :, None, None]
    return ((x / f32(255) - m) / s).astype(f32)


# ---- MIM target with norm_pix ----
MIM_EPS = float(f32(1e-6))


def mim_target_inputs(C, H, W, P, seed=0):
    """img [3, C, H, W] fp32: Gaussian patches, with patch 0 of image 1 a constant small integer and patch 1 of image 1 at mean / std
    = 256."""
    g = torch.Generator().manual_seed(600 + C + H + W + P + seed)
    img = torch.randn(3, C, H, W, generator=g) * 0.5 + torch.randn(3, C, 1, 1, generator=g)
    img[1, :, :P, :P] = 3.0
    if W >= 2 * P:
        img[1, :, :P, P:2 * P] = 64.0 + 0.25 * torch.randn(C, P, P, generator=g)
    return img


def mim_target_reference(img, P):
    """(float64 [N, L, D], bound) of the standardised patches."""
    x = mim_patches_reference(img.to(F64), P)
    n = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / n
    d = x - mean
    q = (d * d).sum(-1, keepdim=True)
    var = q / (n - 1)
    v = var + MIM_EPS
    rstd = v.rsqrt()
    y = d * rstd
    e_mean = U * x.abs().sum(-1, keepdim=True) + U * mean.abs()
    e_d = e_mean + U * d.abs()
    e_q = (n + 3) * U * (q + n * e_mean ** 2) + n * e_mean ** 2
    e_var = e_q / (n - 1) + U * var
    e_v = e_var + U * v
    room = v - e_v
    e_rstd = torch.where(room > 0, rstd * (e_v / (2 * room.clamp_min(1e-300)) + 4 * U), torch.full_like(room, math.inf))
    return y, e_d * rstd + d.abs() * e_rstd + e_d * e_rstd + U * y.abs()


def mim_target_model(img, P, order="seq", mutant=None):
    S = SUMS[order]
    x = np32(mim_patches_reference(img.float(), P))
    n = x.shape[-1]
    mean = (S(x) / f32(n))[..., None]
    d = x - mean
    var = S(d * d) / f32(n if mutant == "biased_variance" else n - 1)
    rstd = (f32(1) / np.sqrt(var + f32(1e-6)))[..., None]
    return (d * rstd).astype(f32)


# ---- MIM loss ----
MIM_LOSS_SHAPES = ((5, 36, 48), (2, 9, 768), (8, 576, 8))   # (B, L, D); the last: 4608 rows, past one sweep of 1024 workgroups x 4 rows
MIM_MASKS = ("random", "one_sample_unmasked", "single_patch")
MIM_GOUT = 0.75


def mim_loss_inputs(B, L, D, mask_kind, bf16, seed=0):
    """x [B, L + 1, D] (storage dtype), target [B, L, D] fp32, mask [B, L] fp32."""
    g = torch.Generator().manual_seed(700 + B + L + D + seed)
    x = torch.randn(B, L + 1, D, generator=g).to(BF if bf16 else F32)
    t = torch.randn(B, L, D, generator=g)
    mask = (torch.rand(B, L, generator=g) < 0.75).float()
    if mask_kind == "one_sample_unmasked":
        mask[B // 2] = 0
    elif mask_kind == "single_patch":
        mask[:] = 0
        mask[B - 1, L // 2] = 1
    if mask_kind != "single_patch":
        mask[0, 0] = 1.0   # never an empty mask
    return x, t, mask


def mim_loss_reference(x, t, mask, gout):
    """float64 (loss, e_loss, dx [B, L + 1, D], e_dx before the store)."""
    x, t, m = x.to(F64), t.to(F64), mask.to(F64)
    D = x.shape[-1]
    e = x[:, 1:] - t
    ss = (e * e).sum(-1)
    row = m * ss / D
    num, den = row.sum(), m.sum()
    loss = num / den
    e_row = m * ((D + 3) * U * ss) / D + 2 * U * row
    e_num = e_row.sum() + float((m != 0).sum()) * U * num
    dx = torch.zeros_like(x)
    dx[:, 1:] = gout * 2.0 * m[..., None] * e / (D * den)
    return loss, e_num / den + U * loss.abs(), dx, 5 * U * dx.abs()


def mim_loss_model(x, t, mask, gout, bf16, order="seq", mutant=None):
    """fp32 (loss, dx holding the stored values)."""
    S = SUMS[order]
    xx, tt, m = np32(x), np32(t), np32(mask)
    D = xx.shape[-1]
    e = xx[:, 1:] - tt
    row = m * S(e * e) / f32(D)
    num, den = S(row.reshape(-1)), S(m.reshape(-1))
    k = f32(gout) * f32(2) * m / (f32(D) * den)
    dx = np.zeros_like(xx)
    dx[:, 1:] = k[..., None] * e
    return num / den, store(_t(dx), bf16, mutant).numpy()


# ---- stand-alone activations ----
def act_grid(bf16):
    """+-0, denormals, +-1e-3 ... +-40 and +-1e4, in the storage dtype's values (fp32 tensor)."""
    mags = torch.cat([torch.tensor([0.0, 1e-40, 2.0 ** -130, 1e4]), torch.logspace(-3, math.log10(40.0), 120)])
    x = torch.cat([mags, -mags])
    return rne_bf16(x) if bf16 else x


FLOOR32, FLOOR16 = 4 * 2.0 ** -149, 2.0 ** -134   # four fp32 roundings of denormal results; half the spacing of the bf16 denormals


def act_fwd_reference(x, act, bf16):
    y = act_value(x.to(F64), act)
    return y, _store_bound(y, _eval_act(x.to(F64), act) + FLOOR32, bf16) + (FLOOR16 if bf16 else 0.0)


def act_bwd_reference(dy, x, act, bf16):
    g = act_grad(x.to(F64), act)
    dx = dy.to(F64) * g
    return dx, _store_bound(dx, dy.to(F64).abs() * _eval_grad(x.to(F64), act) + U * dx.abs() + FLOOR32, bf16) + (FLOOR16 if bf16 else 0.0)


def act32(x, act, grad=False):
    """act_fwd / act_bwd of csrc/common.h in fp32 with torch's erff / expf / tanhf."""
    t = x.float()
    if act == ACT_GELU:
        cdf = 0.5 * (1.0 + torch.erf(t * 0.70710678118654752440))
        return cdf + t * (0.39894228040143267794 * torch.exp(-0.5 * t * t)) if grad else 0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))
    if act == ACT_QUICKGELU:
        s = 1.0 / (1.0 + torch.exp(-1.702 * t))
        return s * (1.0 + 1.702 * t * (1.0 - s)) if grad else t / (1.0 + torch.exp(-1.702 * t))
    if act == ACT_TANH:
        th = torch.tanh(t)
        return 1.0 - th * th if grad else th
    if act == ACT_RELU:
        return (t > 0).float() if grad else torch.clamp(t, min=0)
    if act == ACT_MULAUX:
        return t
    return torch.ones_like(t) if grad else t
