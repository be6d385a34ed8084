"""What deterministic mode costs (ops.set_deterministic / config key `deterministic`).

    python tools/deterministic_bench.py [--batches 32,64,256] [--step-batches 32,256] [--steps 6] [--rounds 3]

1. the step's four wgrad shapes at per-GPU batch B (reduction = B * 577 image-token rows and B * 32 text-token rows): the split-K fp32-atomic form against the ordered form (partial tiles + fold in split order), with the fused bias
   gradient, interleaved A B A B ... as tools/tn_ab.py does, best of `rounds` windows of 10 launches each;
2. the configs[1] training step (bench.py's step: zero_grad, forward, backward, AdamW; bf16, train-mode dropout) in both modes,
   the modes alternating window by window in ONE process, median step of each window.

Times are device events on the launch stream.  A run without a GPU fails; nothing here falls back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
import torch  # noqa: E402
from m3ae_amd import _lib, ops, synth  # noqa: E402

SHAPES = ((3072, 768), (768, 3072), (2304, 768), (768, 768))


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


def splits_of(n, k, rows):
    import ctypes as C
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.batch1, d.batch2 = n, k, rows, 1, 1
    d.a_sm, d.a_sk, d.b_sk, d.b_sn, d.c_sm, d.c_sn = 1, n, k, 1, k, 1
    d.dtype_a, d.dtype_b, d.dtype_c, d.alpha, d.accumulate = _lib.BF16, _lib.BF16, _lib.F32, 1.0, 1
    nbytes = _lib.lib().m3ae_gemm_det_workspace_bytes(C.byref(d))
    return nbytes // (4 * (n * k + n)), nbytes


def wgrad_shapes(batches, rounds):
    for B in batches:
        for rows in (B * 577, B * 32):
            for (n, k) in SHAPES:
                dy = torch.randn(rows, n, device="cuda").to(torch.bfloat16)
                x = torch.randn(rows, k, device="cuda").to(torch.bfloat16)
                g, gb = torch.zeros(n, k, device="cuda"), torch.zeros(n, device="cuda")
                fn = lambda: ops.gemm(dy, 1, n, x, k, 1, g, k, n, k, rows, accumulate=True, a_rowsum=gb)
                best = {False: float("inf"), True: float("inf")}
                for _ in range(rounds):
                    for det in (False, True):
                        with ops.deterministic_mode(det):
                            best[det] = min(best[det], window(fn, 10))
                sp, nbytes = splits_of(n, k, rows)
                a, o = best[False] * 1e3, best[True] * 1e3
                print(f"[wgrad] B {B:3d} rows {rows:6d} {n:4d}x{k:<4d}: atomic {a:7.1f} us  ordered {o:7.1f} us  ({(o / a - 1) * 100:+6.1f} %)"
                      f"  splits {sp:2d}  workspace {nbytes / 2 ** 20:5.1f} MiB  ordered {2.0 * rows * n * k / o / 1e6:5.0f} TF/s", flush=True)
                del dy, x, g, gb


def step_times(batches, steps, rounds):
    from m3ae_amd.config import finetune_vqa_rad_config
    from m3ae_amd.modules import M3AETransformerSS
    from m3ae_amd.modules.objectives import build_vqa_targets
    cfg = finetune_vqa_rad_config(compute_dtype="bf16")
    model = M3AETransformerSS(cfg)
    synth.fill_deterministic(model)
    model.finalize("cuda", torch.bfloat16)
    model.train()
    store = model.store
    for B in batches:
        batch = {}
        for kk, v in synth.synthetic_batch(B, text_len=cfg["max_text_len"], image_size=cfg["image_size"], rank=0).items():
            batch[kk] = v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if isinstance(v, list) and v and
                                                                      isinstance(v[0], torch.Tensor) else v)
        batch["vqa_targets"] = build_vqa_targets(batch, cfg["vqa_label_size"], torch.device("cuda"))

        def step():
            store.zero_grad()
            loss = model.training_step(batch)
            loss.backward()
            store.adamw_step(max_steps=10000, grad_scale=1.0)

        med = {False: [], True: []}
        for det in (False, True):          # warm both paths (first launches load code objects, the allocator grows its pools)
            with ops.deterministic_mode(det):
                for _ in range(2):
                    step()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for det in (False, True):
                with ops.deterministic_mode(det):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
                    for i in range(steps):
                        ev[i].record()
                        step()
                    ev[steps].record()
                    torch.cuda.synchronize()
                    med[det].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(steps)))
        a, o = min(med[False]), min(med[True])
        print(f"[step] configs[1] bf16 per-GPU batch {B}: default {a:8.2f} ms/step ({B / a * 1e3:7.1f} samples/s)  deterministic {o:8.2f} ms/step "
              f"({B / o * 1e3:7.1f} samples/s)  ({(o / a - 1) * 100:+5.1f} %)   windows default {[round(t, 2) for t in med[False]]} "
              f"deterministic {[round(t, 2) for t in med[True]]}", flush=True)
        del batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,64,256", help="per-GPU batches of the wgrad shape table ('' skips it)")
    ap.add_argument("--step-batches", default="32,256", help="per-GPU batches of the step timing ('' skips it)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/deterministic_bench.py measures on the GPU; none is visible")
    ops.use_launch_stream()
    print(f"[deterministic_bench] {torch.cuda.get_device_name(0)}, torch {torch.__version__}", flush=True)
    if args.batches:
        wgrad_shapes([int(b) for b in args.batches.split(",")], args.rounds)
    if args.step_batches:
        step_times([int(b) for b in args.step_batches.split(",")], args.steps, args.rounds)


if __name__ == "__main__":
    main()
