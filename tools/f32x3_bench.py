"""fp32x3 mode throughput: the generic fp32 GEMM, the fp32x3 GEMM (csrc/gemm_f32x3.hip) and the bf16 kernels on the step's
shapes, and one-GPU pairs/s of the configs[1] training step (forward, backward, AdamW; train mode) in fp32, fp32x3 and bf16.

    python tools/f32x3_bench.py gemm [--batches 32,64]
    python tools/f32x3_bench.py step --mode fp32x3 --batch 32 [--steps 5 --warmup 2]

One part per process (the caller puts each under its own time limit).  GEMM timings: HIP events around `iters` back-to-back
launches after one warm-up launch, random normal operands; TFLOP/s counts 2 M N K (times the batch) per call."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
import torch  # noqa: E402
from m3ae_amd import ops  # noqa: E402


def time_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def gemm_shapes(B):
    M, T = B * 577, B * 32
    return [  # (class, M, N, K, layout, batch)
        ("NT qkv", M, 2304, 768, "NT", 1), ("NT out-proj", M, 768, 768, "NT", 1), ("NT fc1", M, 3072, 768, "NT", 1),
        ("NT fc2", M, 768, 3072, "NT", 1),
        ("NN dgrad fc1", M, 768, 3072, "NN", 1), ("NN dgrad fc2", M, 3072, 768, "NN", 1),
        ("TN wgrad fc1", 3072, 768, M, "TN", 1), ("TN wgrad qkv", 2304, 768, M, "TN", 1), ("TN wgrad text", 768, 768, T, "TN", 1),
        ("attn S=QK^T", 577, 577, 64, "NT", B * 12), ("attn O=PV", 577, 64, 577, "NN", B * 12),
        ("attn dV=P^T dO", 577, 64, 577, "TN", B * 12)]


def gemm_call(layout, M, N, K, nb, dtype):
    dev = "cuda"
    if layout == "NT":
        a, b = torch.randn(nb, M, K, device=dev), torch.randn(nb, N, K, device=dev) * K ** -0.5
        strides = (K, 1, 1, K)
    elif layout == "NN":
        a, b = torch.randn(nb, M, K, device=dev), torch.randn(nb, K, N, device=dev) * K ** -0.5
        strides = (K, 1, N, 1)
    else:
        a, b = torch.randn(nb, K, M, device=dev), torch.randn(nb, K, N, device=dev) * K ** -0.5
        strides = (1, M, N, 1)
    a, b = a.to(dtype), b.to(dtype)
    c = torch.zeros(nb, M, N, device=dev, dtype=torch.float32 if layout == "TN" else dtype)
    kw = dict(batch=(1, nb), a_sb=(0, a[0].numel()), b_sb=(0, b[0].numel()), c_sb=(0, M * N)) if nb > 1 else {}
    sm, sk, bk, bn = strides
    return lambda **extra: ops.gemm(a, sm, sk, b, bk, bn, c, N, M, N, K, accumulate=layout == "TN", **kw, **extra)


def run_gemm(batches, iters):
    print("GEMM TFLOP/s: generic fp32 FMA | fp32x3 split-bf16 MFMA | bf16 operands as dispatched (kernel)")
    for B in batches:
        print(f"B = {B}")
        for name, M, N, K, layout, nb in gemm_shapes(B):
            flops = 2.0 * M * N * K * nb
            f32 = gemm_call(layout, M, N, K, nb, torch.float32)
            t_gen = time_ms(lambda: f32(force_generic=True), max(2, iters // 4))
            with ops.f32x3_mode(True):
                t_x3 = time_ms(f32, iters)
                assert ops.last_gemm_path() == "f32x3"
            del f32
            bf = gemm_call(layout, M, N, K, nb, torch.bfloat16)
            t_bf = time_ms(bf, iters)
            path_bf = ops.last_gemm_path()
            del bf
            torch.cuda.empty_cache()
            tf = lambda t: flops / t / 1e9
            print(f"  {name:15s} {M:6d} x {N:5d} x {K:6d} x {nb:4d}: generic {tf(t_gen):7.1f}  f32x3 {tf(t_x3):7.1f}  "
                  f"bf16 {tf(t_bf):7.1f} ({path_bf})   f32x3 vs generic {t_gen / t_x3:5.2f}x", flush=True)


def run_step(mode, B, steps, warmup):
    from m3ae_amd import synth
    from m3ae_amd.config import finetune_vqa_rad_config
    from m3ae_amd.modules import M3AETransformerSS
    from m3ae_amd.modules.objectives import build_vqa_targets
    dev = "cuda"
    cfg = finetune_vqa_rad_config(compute_dtype=mode)
    model = M3AETransformerSS(cfg)
    synth.fill_deterministic(model)
    model.finalize(dev, mode)
    model.train(True)
    store = model.store
    batch = synth.synthetic_batch(B, text_len=cfg["max_text_len"], image_size=cfg["image_size"], rank=0)
    batch = {k: (v.to(dev) if isinstance(v, torch.Tensor) else ([t.to(dev) for t in v] if isinstance(v, list) and v and
                 isinstance(v[0], torch.Tensor) else v)) for k, v in batch.items()}
    batch["vqa_targets"] = build_vqa_targets(batch, cfg["vqa_label_size"], dev)

    def step():
        store.zero_grad()
        loss = model.training_step(batch)
        loss.backward()
        store.adamw_step(max_steps=1000)
        return loss

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    print(f"step {mode:6s} B = {B:3d}: {dt * 1e3:9.1f} ms/step  {B / dt:8.1f} pairs/s  loss {loss.item():.5f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["gemm", "step"])
    ap.add_argument("--batches", default="32,64")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--mode", choices=["fp32", "fp32x3", "bf16"], default="fp32x3")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"device {torch.cuda.get_device_name(0)}")
    if a.part == "gemm":
        run_gemm([int(b) for b in a.batches.split(",")], a.iters)
    else:
        run_step(a.mode, a.batch, a.steps, a.warmup)


if __name__ == "__main__":
    main()
