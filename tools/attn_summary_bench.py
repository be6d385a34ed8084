"""What the attention summaries cost next to the attention maps (infer(output_attention_summary=True) / output_attentions=True).

    python tools/attn_summary_bench.py [--batches 16,32,256] [--iters 3] [--rounds 3] [--log profiles/r18_attn_summary.log]

1. forward-only infer of configs[1] (bf16, eval mode, no_grad) at each batch: plain, with the maps, with the summaries; the three
   alternate window by window in ONE process, best window of each, and the ratios summary / plain and summary / maps;
2. one image-layer self-attention (B = 256, 12 heads, 577 x 577): m3ae_attn_colmean against m3ae_attn_probs on the same q, k and
   log-sum-exp table, with the bytes each moves to and from memory (the map: B H Lq Lk fp32 written; the summary: the partial
   rows written and read back, B Lk fp32 out; both read q, k and the table once).

Times are device events on the launch stream.  A run without a GPU fails; nothing here falls back."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
import torch  # noqa: E402
from m3ae_amd import ops, synth  # noqa: E402
from m3ae_amd.config import finetune_vqa_rad_config  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402

_log = None


def say(msg):
    print(msg, flush=True)
    if _log is not None:
        _log.write(msg + "\n")
        _log.flush()


def window(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, iters, rounds):
    """fns: key -> callable; best window of each, the keys alternating."""
    best = {k: float("inf") for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            best[k] = min(best[k], window(fn, iters))
    return best


def to_cuda(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and v and
                isinstance(v[0], torch.Tensor) else v) for k, v in batch.items()}


def infer_windows(batches, iters, rounds):
    cfg = finetune_vqa_rad_config(compute_dtype="bf16")
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    m.eval()
    for B in batches:
        batch = to_cuda(synth.synthetic_batch(B, text_len=cfg["max_text_len"], image_size=cfg["image_size"], rank=0))

        def run(**kw):
            def f():
                with torch.no_grad():
                    m.infer(batch, **kw)
            return f
        best = alternate({"plain": run(), "maps": run(output_attentions=True), "summary": run(output_attention_summary=True)},
                         iters, rounds)
        p, a, s = best["plain"], best["maps"], best["summary"]
        say(f"[infer] configs[1] bf16 forward-only B {B:4d}: plain {p:8.2f} ms  maps {a:8.2f} ms ({(a / p - 1) * 100:+5.1f} %)  summary "
            f"{s:8.2f} ms ({(s / p - 1) * 100:+5.1f} %)   summary / plain {s / p:.3f}   summary / maps {s / a:.3f}")
        del batch
        torch.cuda.empty_cache()


def kernels(B, H, L, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v = (torch.randn(B, L, 64 * H, device="cuda", generator=g).to(torch.bfloat16) for _ in range(3))
    with torch.no_grad():
        _, lse = ops.attn_forward(q, k, v, H)
    fns = {"probs": lambda: ops.attn_probs(q, k, lse, H), "colmean": lambda: ops.attn_colmean(q, k, lse, H)}
    best = alternate(fns, 5, rounds)
    nqb = (L + 127) // 128
    reads = 2 * B * L * H * 64 * 2 + B * H * L * 4      # q and k once each (the per-block re-reads of k are served by L2), the lse rows
    moved = {"probs": reads + B * H * L * L * 4, "colmean": reads + 2 * B * H * nqb * L * 4 + B * L * 4}
    for name in fns:
        us = best[name] * 1e3
        say(f"[kernel] image self-attention B {B} H {H} {L} x {L}: m3ae_attn_{name:8s} {us:9.1f} us   {moved[name] / 2 ** 20:9.1f} MiB to and from "
            f"memory   {moved[name] / us / 1e6:5.2f} TB/s")
    say(f"[kernel] m3ae_attn_colmean / m3ae_attn_probs: time {best['colmean'] / best['probs']:.3f}, bytes "
        f"{moved['colmean'] / moved['probs']:.4f}")


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,32,256", help="batches of the infer windows ('' skips them)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-batch", type=int, default=256, help="batch of the kernel comparison (0 skips it)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r18_attn_summary.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/attn_summary_bench.py measures on the GPU; none is visible")
    _log = open(args.log, "w")
    ops.use_launch_stream()
    say(f"[attn_summary_bench] {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if args.kernel_batch:
        kernels(args.kernel_batch, 12, 577, args.rounds)
    if args.batches:
        infer_windows([int(b) for b in args.batches.split(",")], args.iters, args.rounds)


if __name__ == "__main__":
    main()
