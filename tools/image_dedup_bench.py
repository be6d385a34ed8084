"""What running the image tower once per distinct image saves (batch["image_index"], config key `image_dedup`).

    python tools/image_dedup_bench.py [--batches 256,32] [--steps 6] [--rounds 3] [--log profiles/r11_image_dedup.log]

1. the two kernels alone (m3ae_expand_samples, m3ae_segment_sum_rows) at the step's shape -- rows of 577 x 768 bf16 -- against the
   bytes they move, next to the zero-fill rate (m3ae_zero) of the same number of bytes measured in the same run;
2. the configs[1] training step with the classification head (bench.py's step: zero_grad, forward, backward, AdamW; bf16,
   train-mode dropout) at per-GPU batch B with U distinct images: the key absent, the identity index (U = B), the distinct
   share of a uniform draw of B samples from 315 images, B / 4 and B / 11.  The variants alternate window by window in ONE
   process, median step of each window, best window of each variant.  Against each: the predicted saving, the image tower's
   share of the step's FLOPs (101.8 of 183.8 GFLOP per sample) times (1 - U / B).

Times are device events on the launch stream.  A run without a GPU fails; nothing here falls back.  The key-absent variant runs the
launches of a batch without the feature (infer() reads one dict key more); compare its step with bench.py's of the parent commit."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
import torch  # noqa: E402
from m3ae_amd import _lib, ops, synth  # noqa: E402

TOWER_SHARE = 101.8 / 183.8
TOKENS, WIDTH, POOL = 577, 768, 315
_LOG = None


def say(msg):
    print(msg, flush=True)
    if _LOG is not None:
        _LOG.write(msg + "\n")
        _LOG.flush()


def distinct_counts(B):
    """[(label, U)]: the distinct share of a uniform draw from POOL images, a quarter, an eleventh."""
    uniform = round(POOL * (1.0 - (1.0 - 1.0 / POOL) ** B))
    return [("uniform draw from 315", min(uniform, B)), ("1/4", max(B // 4, 1)), ("1/11", max(round(B / 11), 1))]


def make_index(B, U, seed=0):
    """B samples over U images, every image used, members scattered (a fixed permutation)."""
    g = torch.Generator().manual_seed(seed + 1000 * B + U)
    idx = torch.cat([torch.arange(U), torch.randint(0, U, (B - U,), generator=g)])
    return idx[torch.randperm(B, generator=g)].contiguous()


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


def kernels(batches, rounds):
    L = _lib.lib()
    R = TOKENS * WIDTH
    for B in batches:
        for label, U in distinct_counts(B):
            g = ops.image_groups(make_index(B, U)).to("cuda")
            x = torch.randn(U, R, device="cuda").to(torch.bfloat16)
            y = torch.empty(B, R, dtype=torch.bfloat16, device="cuda")
            dx = torch.empty_like(x)
            s = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
            p = lambda t: C.c_void_p(t.data_ptr())
            fns = {
                "expand": lambda: L.m3ae_expand_samples(p(x), p(g.index), p(y), B, U, R, _lib.BF16, s()),
                "segment_sum": lambda: L.m3ae_segment_sum_rows(p(y), p(g.offsets), p(g.members), p(dx), U, B, R, _lib.BF16, s()),
                "zero_fill": lambda: L.m3ae_zero(p(y), y.numel() * 2, s()),
            }
            # bytes through the memory system: the expansion reads U rows (repeats are served on-die) and writes B; the sum reads
            # B rows and writes U; the fill writes B rows
            nbytes = {"expand": (U + B) * R * 2, "segment_sum": (B + U) * R * 2, "zero_fill": B * R * 2}
            best = {k: float("inf") for k in fns}
            for _ in range(rounds):
                for k, fn in fns.items():
                    best[k] = min(best[k], window(fn, 10))
            largest = int(torch.bincount(g.index).max())
            say(f"[kernels] B {B:3d} U {U:3d} ({label}; largest group {largest:2d}), rows of {R * 2 / 1e3:.0f} kB bf16: " + "  ".join(
                f"{k} {best[k] * 1e3:7.1f} us = {nbytes[k] / best[k] / 1e9:5.2f} TB/s" for k in fns))
            del x, y, dx


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
        base = {}
        for kk, v in synth.synthetic_batch(B, text_len=cfg["max_text_len"], image_size=cfg["image_size"], rank=0).items():
            base[kk] = v.cuda() if isinstance(v, torch.Tensor) else ([t.cuda() for t in v] if isinstance(v, list) and v and
                                                                     isinstance(v[0], torch.Tensor) else v)
        base["vqa_targets"] = build_vqa_targets(base, cfg["vqa_label_size"], torch.device("cuda"))
        variants = [("key absent", B, base)]
        ident = ops.image_groups(torch.arange(B)).to("cuda")
        variants.append(("identity index", B, dict(base, image_index=ident.index, image_groups=ident)))
        for label, U in distinct_counts(B):
            g = ops.image_groups(make_index(B, U)).to("cuda")
            variants.append((label, U, dict(base, image=[base["image"][0][:U].contiguous()], image_index=g.index, image_groups=g)))

        def step(batch):
            store.zero_grad()
            loss = model.training_step(batch)
            loss.backward()
            store.adamw_step(max_steps=10000, grad_scale=1.0)

        for _, _, b in variants:            # warm every path (code objects, allocator pools)
            for _ in range(2):
                step(b)
        torch.cuda.synchronize()
        med = {label: [] for label, _, _ in variants}
        for _ in range(rounds):
            for label, _, b in variants:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
                for i in range(steps):
                    ev[i].record()
                    step(b)
                ev[steps].record()
                torch.cuda.synchronize()
                med[label].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(steps)))
        t0 = min(med["key absent"])
        for label, U, _ in variants:
            t = min(med[label])
            predicted = (1.0 - U / B) * TOWER_SHARE
            say(f"[step] configs[1] bf16 per-GPU batch {B:3d}, U {U:3d} ({label}): {t:8.2f} ms/step ({B / t * 1e3:7.1f} samples/s)  "
                f"measured saving {(1 - t / t0) * 100:+5.1f} %  predicted {(predicted) * 100:4.1f} % (tower share x (1 - U/B), less the "
                f"two kernels)   windows {[round(v, 2) for v in med[label]]}")
        del variants, base


def main():
    global _LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,32", help="per-GPU batches of the step timing and the kernel table")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r11_image_dedup.log"), help="'' writes no file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/image_dedup_bench.py measures on the GPU; none is visible")
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        _LOG = open(args.log, "w")
    ops.use_launch_stream()
    say(f"[image_dedup_bench] {torch.cuda.get_device_name(0)}, torch {torch.__version__}; tower share of the step taken as "
        f"{TOWER_SHARE * 100:.1f} % (BASELINE.md section 3)")
    batches = [int(b) for b in args.batches.split(",")]
    kernels(batches, args.rounds)
    if not args.skip_steps:
        step_times(batches, args.steps, args.rounds)


if __name__ == "__main__":
    main()
