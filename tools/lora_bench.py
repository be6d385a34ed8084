"""What LoRA in merged form (`lora_rank`) costs over the full-size flat buffers, against bytes moved and against the step.

    python tools/lora_bench.py [--rank 8] [--rounds 3] [--iters 30] [--step-iters 6] [--batches 256 32] [--log profiles/r22_lora.log]

Two measurements over the configs[1] model in bf16 mode, each in windows that alternate with windows of its baseline in one
process, so every ratio is taken inside one thermal / clock state; the best window of either side counts, and the spread of the
windows (worst / best) is printed next to it:

  1. the optimizer phase with adapters -- m3ae_lora_grad, the rule over the two adapter ranges and the head segments, m3ae_lora_merge
     (LoraAdapters.step without the transposed / tiled copies, which both sides launch alike) -- against the six m3ae_adamw launches
     of the full fine-tune on the same buffers, and the projection and the merge alone.  Bytes per target element: the projection
     reads dW = 4 B, the merge reads W0 and writes W and the bf16 shadow = 10 B, together 14 B (+ the planes: r / 64 of a read and
     a write); AdamW reads p, g, m, v and writes p, m, v and the shadow = 30 B.  The prediction this run can falsify: the phase is
     shorter with the key on;
  2. the training step (forward, backward, optimizer_step) with the adapters detached against attached, at each per-GPU batch of
     --batches: the delta is read against the spread of the step's own windows.

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
from m3ae_amd.modules.objectives import build_vqa_targets  # noqa: E402

MERGE_BYTES, PROJ_BYTES, ADAMW_BYTES = 10, 4, 30
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


def alternate(fns, rounds, iters):
    """[[windows of fns[0]], [windows of fns[1]], ...] in ms per call, the windows alternating."""
    out = [[] for _ in fns]
    for _ in range(rounds):
        for o, fn in zip(out, fns):
            o.append(window(fn, iters))
    return out


def to_dev(batch):
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to("cuda")
        elif isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            out[k] = [t.to("cuda") for t in v]
        else:
            out[k] = v
    return out


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--step-iters", type=int, default=6)
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 32])
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r22_lora.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lora_bench.py measures on the GPU; none is visible")
    _log = open(args.log, "w")
    ops.use_launch_stream()
    say(f"[lora_bench] {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    cfg = finetune_vqa_rad_config(compute_dtype="bf16", lora_rank=args.rank)
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    m.train()
    st = m.store
    ad = m.attach_lora()
    assert st.optim == "adamw" and st.lora is ad
    # learning rate 0 and no decay: the parameters stay where they are across repeats while every load, operation and store runs
    still = dict(max_steps=10000, group_lrs=[0.0] * 6, group_wds=[0.0] * 6)
    hyper = st.begin_update(**still)            # (allocates the store's moments)
    ad._alloc_state()
    st.grad.normal_(0.0, 1e-3)
    for i in range(len(ad.records)):            # B != 0: the merge's arithmetic sees ordinary values
        ad.views(i)[1].normal_(0.0, 1e-3)
    torch.cuda.synchronize()
    n = st.trainable_end
    target = sum(N * K for _, N, K, _, _, _ in ad.records)
    say(f"[lora_bench] configs[1] bf16: {n} trainable elements with padding; {ad.describe()}, {target} target elements "
        f"({100.0 * target / n:.1f} % of the trainable range), workspace {ad.table.ws_bytes / 2 ** 20:.1f} MiB; {args.rounds} rounds of "
        f"alternating windows of {args.iters} repeats ({args.step_iters} for the step), best window; spread = worst / best window")

    def adamw_six():
        for gi in range(6):
            a, b = st.segments[gi]
            st.update_range(a, min(b, n), gi, hyper)

    def lora_phase():                # LoraAdapters.step without sync_shadows(cast=False), which the full fine-tune launches too
        ad.project()
        bufs = (ad.lora, ad.lora_grad, ad.exp_avg, ad.exp_avg_sq, None)
        st.update_range(0, ad.split, 0, hyper, bufs=bufs, lr_mult=ad.lr_multiplier)
        st.update_range(ad.split, ad.total, 4, hyper, bufs=bufs, lr_mult=ad.lr_multiplier)
        for gi in (2, 3):
            a, b = st.segments[gi]
            st.update_range(a, min(b, n), gi, hyper)
        ad.merge()

    base, mine, proj, mrg = alternate([adamw_six, lora_phase, ad.project, ad.merge], args.rounds, args.iters)
    tb, tm, tp, tg = min(base), min(mine), min(proj), min(mrg)
    say(f"[lora] optimizer phase, key on  {tm * 1e3:8.1f} us (spread {max(mine) / tm:.3f})   m3ae_adamw x 6 in the same windows "
        f"{tb * 1e3:8.1f} us  {ADAMW_BYTES * n / tb / 1e9:6.2f} TB/s of {ADAMW_BYTES} B / element (spread {max(base) / tb:.3f})   "
        f"time ratio {tm / tb:.3f}")
    say(f"[lora] m3ae_lora_grad  {tp * 1e3:8.1f} us  {PROJ_BYTES * target / tp / 1e9:6.2f} TB/s of {PROJ_BYTES} B / target element "
        f"(spread {max(proj) / tp:.3f})   m3ae_lora_merge  {tg * 1e3:8.1f} us  {MERGE_BYTES * target / tg / 1e9:6.2f} TB/s of "
        f"{MERGE_BYTES} B / target element (spread {max(mrg) / tg:.3f})")

    for B in args.batches:
        batch = to_dev(synth.synthetic_batch(B, text_len=cfg["max_text_len"], image_size=cfg["image_size"], rank=0))
        batch["vqa_targets"] = build_vqa_targets(batch, cfg["vqa_label_size"], torch.device("cuda", torch.cuda.current_device()))

        def step(adapters):
            def run():
                st.lora = adapters            # update_apply reads it: None makes the step's calls what they are without the key
                st.zero_grad()
                out = m.training_step(batch)
                (out["loss"] if isinstance(out, dict) else out).backward()
                st.optimizer_step(**still)
            return run
        try:
            base, mine = alternate([step(None), step(ad)], args.rounds, args.step_iters)
        finally:
            st.lora = ad
        tb, tm = min(base), min(mine)
        say(f"[lora] step at per-GPU batch {B:4d}: key off {tb:8.3f} ms (spread {max(base) / tb:.3f})   lora_rank={args.rank} {tm:8.3f} ms "
            f"(spread {max(mine) / tm:.3f})   delta {(tm - tb) * 1e3:+8.1f} us = {100 * (tm - tb) / tb:+.2f} % of the step; "
            f"windows off {[round(x, 3) for x in base]} on {[round(x, 3) for x in mine]}")
        del batch


if __name__ == "__main__":
    main()
