"""Models of the image tower's residual stream (config key clip_residual_dtype), torch-CPU / numpy, for
tests/test_clip_residual_host.py and tests/test_gpu_clip_residual.py.

1. A rounding model of the pre-LN CLIP tower (m3ae_amd/ops.py: ClipBlockFn).  Every product and every LayerNorm is evaluated in
   float64; a value is rounded only where the layer STORES it:
     operand sites (bf16 in bf16 mode, whatever the stream does): the two LayerNorm outputs, q|k|v, the attention probabilities
       P that meet V, the attention output, the activation, and the tower output after ln_post;
     stream sites: the stream after each of a block's two joins (the out-proj and fc2 epilogues) and the tower's input.
   `stream` picks the rounding of the stream sites: "bf16" (what the default does), "fp32", or None together with ops=None: no
   rounding anywhere, the float64 reference -- that form is differentiable and serves as the float64 autograd reference on the GPU
   tower's own weights.  What the model leaves out: the order of the MFMA accumulation, v_exp in softmax and QuickGELU, the
   rescaling of flash attention.
2. A numpy model of the mixed LayerNorm kernel: the fp32 LayerNorm in the kernel's order of operations up to the lane-parallel
   sums (which numpy adds pairwise), followed by ONE round-to-nearest-even to bf16.
"""
import math

import numpy as np
import torch

F64 = torch.float64


def rne_bf16(x):
    """float64 -> nearest bf16 (ties to even), returned as float64.  Through fp32 first, as the kernels' fp32 registers are."""
    return x.float().to(torch.bfloat16).to(x.dtype)


def rne_f32(x):
    return x.float().to(x.dtype)


ROUND = {"bf16": rne_bf16, "fp32": rne_f32, None: (lambda x: x)}


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def block(x, w, heads, ops="bf16", stream="bf16"):
    """One ResidualAttentionBlock on x [B, L, D] (float64); w: dict of float64 tensors under the module's parameter names."""
    r, rs = ROUND[ops], ROUND[stream]
    B, L, D = x.shape
    dh = D // heads
    h = r(layer_norm(x, w["ln_1.weight"], w["ln_1.bias"]))
    qkv = r(h @ w["attn.in_proj_weight"].t() + w["attn.in_proj_bias"])
    q, k, v = (t.reshape(B, L, heads, dh).transpose(1, 2) for t in qkv.split(D, dim=-1))
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), dim=-1)
    o = r((r(p) @ v).transpose(1, 2).reshape(B, L, D))
    xa = rs(o @ w["attn.out_proj.weight"].t() + w["attn.out_proj.bias"] + x)
    h = r(layer_norm(xa, w["ln_2.weight"], w["ln_2.bias"]))
    g = r(quick_gelu(h @ w["mlp.c_fc.weight"].t() + w["mlp.c_fc.bias"]))
    return rs(g @ w["mlp.c_proj.weight"].t() + w["mlp.c_proj.bias"] + xa)


def blocks_and_post(x, blocks, post, heads, ops="bf16", stream="bf16"):
    """x: the stream entering the first block.  Returns (the input of ln_post, the tower output)."""
    x = ROUND[stream](x)
    for w in blocks:
        x = block(x, w, heads, ops, stream)
    return x, ROUND[ops](layer_norm(x, post["weight"], post["bias"]))


def clip_init_blocks(width, n_blocks, seed):
    """CLIP.initialize_parameters for n_blocks blocks of a tower of n_blocks + 1 `layers` (the tower runs layers - 1), rounded
    through bf16 (the weights the GEMMs read), as float64."""
    g = torch.Generator().manual_seed(seed)
    layers = n_blocks + 1
    proj_std, attn_std, fc_std = width ** -0.5 * (2 * layers) ** -0.5, width ** -0.5, (2 * width) ** -0.5
    n = lambda *shape, std: rne_bf16((torch.randn(*shape, generator=g) * std).to(F64))
    one, zero = (lambda k: torch.ones(k, dtype=F64)), (lambda k: torch.zeros(k, dtype=F64))
    out = []
    for _ in range(n_blocks):
        out.append({"ln_1.weight": one(width), "ln_1.bias": zero(width), "ln_2.weight": one(width), "ln_2.bias": zero(width),
                    "attn.in_proj_weight": n(3 * width, width, std=attn_std), "attn.in_proj_bias": zero(3 * width),
                    "attn.out_proj.weight": n(width, width, std=proj_std), "attn.out_proj.bias": zero(width),
                    "mlp.c_fc.weight": n(4 * width, width, std=fc_std), "mlp.c_fc.bias": zero(4 * width),
                    "mlp.c_proj.weight": n(width, 4 * width, std=proj_std), "mlp.c_proj.bias": zero(width)})
    return out, {"weight": one(width), "bias": zero(width)}


def rel_err(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


def stream_errors(width, heads, n_blocks, rows, seed):
    """(error of the bf16 stream, error of the fp32 stream) of what the blocks hand ln_post, against float64, ||d|| / ||ref||, on a
    unit-variance stream of `rows` token rows (what ln_pre hands the first block).  (ln_post's own bf16 store is the same one
    rounding under either setting: it adds its 1e-3 to both and says nothing about the stream.)"""
    blocks, post = clip_init_blocks(width, n_blocks, seed)
    x = torch.randn(1, rows, width, generator=torch.Generator().manual_seed(seed + 1000)).to(F64)
    ref = blocks_and_post(x, blocks, post, heads, None, None)[0]
    return tuple(rel_err(blocks_and_post(x, blocks, post, heads, "bf16", s)[0], ref) for s in ("bf16", "fp32"))


# ---- the whole tower in float64 from a VisualTransformer's parameters (differentiable: no rounding) --------------------------------
def tower_f64(img, sd, heads, patch, n_blocks, add_pos=True):
    """img [B, 3, R, R]; sd: name -> float64 tensor under VisualTransformer's parameter names.  Returns (tokens, the input of
    ln_post, the tower output)."""
    B = img.shape[0]
    width = sd["conv1.weight"].shape[0]
    pe = torch.nn.functional.conv2d(img, sd["conv1.weight"], stride=patch).reshape(B, width, -1).transpose(1, 2)
    tok = torch.cat([sd["class_embedding"].expand(B, 1, width), pe], dim=1)
    if add_pos:
        tok = tok + sd["positional_embedding"]
    x = layer_norm(tok, sd["ln_pre.weight"], sd["ln_pre.bias"])
    for i in range(n_blocks):
        pre = f"transformer.resblocks.{i}."
        x = block(x, {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, heads, None, None)
    return tok, x, layer_norm(x, sd["ln_post.weight"], sd["ln_post.bias"])


# ---- numpy model of the mixed LayerNorm --------------------------------------------------------------------------------------------
def np_rne_bf16_bits(x):
    """fp32 array -> uint16 bf16 bit patterns, round to nearest even (finite values)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint16)


def np_bf16_to_f32(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def np_layernorm_f32(x, g, b, eps):
    """The fp32 LayerNorm: two-pass statistics, rstd = 1 / sqrt(var + eps), y = (x - mean) * rstd * g + b, all in fp32."""
    f = np.float32
    x = x.astype(f)
    D = f(x.shape[-1])
    mean = (x.sum(-1, dtype=f) / D).astype(f)
    d = (x - mean[:, None]).astype(f)
    var = ((d * d).sum(-1, dtype=f) / D).astype(f)
    rstd = (f(1.0) / np.sqrt(var + f(eps), dtype=f)).astype(f)
    return ((d * rstd[:, None]).astype(f) * g.astype(f) + b.astype(f)).astype(f), mean, rstd


def np_layernorm_mixed(x, g, b, eps):
    """fp32 rows in, bf16 bit patterns out: the fp32 LayerNorm followed by ONE round-to-nearest-even."""
    y, mean, rstd = np_layernorm_f32(x, g, b, eps)
    return np_rne_bf16_bits(y), mean, rstd
