"""What the fusion-layer attention maps cost: infer() forward-only (bf16, eval) with and without output_attentions at per-GPU
batch 16 / 32 / 256, and m3ae_attn_probs alone on the image self-attention shape (577 x 577, 12 heads) against m3ae_zero writing
the same number of bytes (the write-bandwidth yardstick of the same box), and m3ae_xattn_probs_export of a fused cross-attention
call in both directions.
    python tools/attn_maps_bench.py [--batches 16,32,256] [--iters 5]
Log of a run: profiles/r05_attn_maps_bench.log"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))

from m3ae_amd import _lib, ops, synth  # noqa: E402
from m3ae_amd.config import finetune_vqa_rad_config  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def batch_on_gpu(B):
    b = synth.synthetic_batch(B, text_len=32, image_size=384, vocab_size=50265, rank=0)
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if isinstance(v, list) and v and
                                                               isinstance(v[0], torch.Tensor) else v)) for k, v in b.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,32,256")
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"[attn maps] device {torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)
    m = M3AETransformerSS(finetune_vqa_rad_config(compute_dtype="bf16"))
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    m.eval()
    for B in (int(x) for x in args.batches.split(",")):
        b = batch_on_gpu(B)

        def run(maps):
            with torch.no_grad():
                ret = m.infer(b, output_attentions=maps)
            del ret

        off, off_min = timed(lambda: run(False), args.iters)
        on, on_min = timed(lambda: run(True), args.iters)
        gb = 0.0
        with torch.no_grad():
            att = m.infer(b, output_attentions=True)["attentions"]
        for key in att:
            for entry in att[key]:
                gb += sum(p.numel() * 4 for p in entry) / 1e9
        del att
        print(f"[attn maps] infer B={B:4d}: without maps {off:8.2f} ms (min {off_min:.2f}), with maps {on:8.2f} ms "
              f"(min {on_min:.2f}): +{on - off:.2f} ms = +{100 * (on - off) / off:.1f} %, {gb:.2f} GB of maps "
              f"({gb / max(on - off, 1e-6):.2f} TB/s over the difference)", flush=True)
        del b
        torch.cuda.empty_cache()

    # m3ae_attn_probs alone: the image self-attention map of one layer, against a plain zero fill of the same bytes
    B, H, L = 256, 12, 577
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B, L, 64 * H, device="cuda", generator=g).to(torch.bfloat16)
    k = torch.randn(B, L, 64 * H, device="cuda", generator=g).to(torch.bfloat16)
    with torch.no_grad():
        _, lse = ops.attn_forward(q, k, k, H)
    out = torch.empty(B, H, L, L, dtype=torch.float32, device="cuda")
    nbytes = out.numel() * 4
    d = ops._attn_desc(B, H, L, L, 64, q, k, k, q, None, None, 0.125, False, lse, lse.shape[-1], _lib.BF16)
    lib = _lib.lib()

    def probs():
        _lib.check(lib.m3ae_attn_probs(C.byref(d), C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1), out.stride(2),
                                       ops._stream()), "m3ae_attn_probs")

    def zero():
        _lib.check(lib.m3ae_zero(C.c_void_p(out.data_ptr()), nbytes, ops._stream()), "m3ae_zero")

    for name, fn in (("m3ae_attn_probs", probs), ("m3ae_zero (same bytes)", zero)):
        med, mn = timed(fn, 3 * args.iters)
        print(f"[attn maps] {name:24s} B={B} H={H} {L}x{L}: {med:7.3f} ms (min {mn:.3f}), {nbytes / 1e9:.2f} GB written, "
              f"{nbytes / med / 1e9:.2f} TB/s", flush=True)
    d.dropout_p, d.dropout_seed = 0.1, 99
    med, mn = timed(probs, 3 * args.iters)
    print(f"[attn maps] {'m3ae_attn_probs p=0.1':24s} B={B} H={H} {L}x{L}: {med:7.3f} ms (min {mn:.3f}), "
          f"{nbytes / med / 1e9:.2f} TB/s", flush=True)
    del out, q, k, lse
    torch.cuda.empty_cache()

    # m3ae_xattn_probs_export of a fusion layer's fused cross-attention at B = 256 (bf16 read + fp32 write per element)
    layer = m.multi_modal_vision_layers[0].crossattention
    P = layer.block_params()
    x = torch.randn(B * L, 768, device="cuda", generator=g).to(torch.bfloat16)
    t = torch.randn(B * 32, 768, device="cuda", generator=g).to(torch.bfloat16)
    for name, (h2, Lq, o2, Lk) in (("dir 1 (image queries)", (x, L, t, 32)), ("dir 0 (text queries)", (t, 32, x, L))):
        with torch.no_grad():
            _, saved = ops.xattn_fwd(h2, B, Lq, o2, Lk, None, P, need_bwd=False, want_probs=True)
        n = B * 12 * Lq * Lk
        med, mn = timed(lambda: ops.xattn_probs(saved), 3 * args.iters)
        print(f"[attn maps] m3ae_xattn_probs_export {name} B={B} {Lq}x{Lk}: {med:7.3f} ms (min {mn:.3f}), "
              f"{n * 6 / med / 1e9:.2f} TB/s (2 B read + 4 B written per element)", flush=True)
        del saved


if __name__ == "__main__":
    main()
