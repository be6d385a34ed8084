"""What gradient clipping by global norm (config key gradient_clip_val) costs on the full-size model, and whether summing the squares
in double costs anything beside the bytes read.

    python tools/grad_clip_bench.py [--step-batches 256,32] [--steps 6] [--rounds 3] [--log profiles/r15_grad_clip.log]

1. the configs[1] training step (bench.py's step: zero_grad, forward, backward, AdamW; bf16, train-mode dropout) with the key off
   and on (a bound the norm exceeds, so the factor is a real one), alternating window by window on ONE model in one process, as
   tools/deterministic_bench.py does; median step of each window;
2. the chain alone on that model's gradient buffer: m3ae_sumsq_segments (piece kernel + per-segment fold) + m3ae_clip_finalize,
   against the 4 bytes per element of every segment it reads, and the six m3ae_adamw launches of the same buffer against the
   30 bytes per element they move in bf16 mode (p, g, m, v read; p, m, v and the bf16 shadow written).

The prediction this run can falsify: from bytes the pass reads 4 of the optimizer's 30 bytes per element (about 1 / 7), so it
should cost a few tenths of a millisecond of a step, and one v_fma_f64 per element should cost nothing beside the load: the
chain's achieved bytes/s no worse than the AdamW kernel's.

Times are device events on the launch stream.  A run without a GPU fails; nothing here falls back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
import torch  # noqa: E402
from m3ae_amd import gradnorm, ops, synth  # noqa: E402
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


def to_cuda(batch):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and v and
                isinstance(v[0], torch.Tensor) else v) for k, v in batch.items()}


def steps(m, cfg, batches, nsteps, rounds):
    from m3ae_amd.modules.objectives import build_vqa_targets
    st = m.store
    for B in batches:
        batch = to_cuda(synth.synthetic_batch(B, text_len=cfg["max_text_len"], image_size=cfg["image_size"], rank=0))
        batch["vqa_targets"] = build_vqa_targets(batch, cfg["vqa_label_size"], torch.device("cuda"))

        def step():
            st.zero_grad()
            m.training_step(batch).backward()
            st.adamw_step(max_steps=10000, grad_scale=1.0)
        st.cfg["gradient_clip_val"] = 0.0
        for _ in range(2):
            step()
        st.zero_grad()
        m.training_step(batch).backward()
        norm = st.grad_norm()
        keys = {"off": 0.0, "on": norm / 2}
        med = {k: [] for k in keys}
        for k, v in keys.items():      # warm both paths
            st.cfg["gradient_clip_val"] = v
            step()
        for _ in range(rounds):
            for k, v in keys.items():
                st.cfg["gradient_clip_val"] = v
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(nsteps + 1)]
                for i in range(nsteps):
                    ev[i].record()
                    step()
                ev[nsteps].record()
                torch.cuda.synchronize()
                med[k].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(nsteps)))
        a, o = min(med["off"]), min(med["on"])
        s = st.grad_stats()
        say(f"[step] configs[1] bf16 per-GPU batch {B}: key off {a:8.2f} ms/step  gradient_clip_val={norm / 2:.4g} {o:8.2f} ms/step  "
            f"({(o / a - 1) * 100:+5.2f} %, {o - a:+.3f} ms)   windows off {[round(t, 2) for t in med['off']]} on "
            f"{[round(t, 2) for t in med['on']]}   last step: norm {s['norm']:.4g} coef {s['coef']:.4f}, {s['steps']} steps "
            f"{s['clipped_steps']} clipped {s['skipped_steps']} skipped")
        st.cfg["gradient_clip_val"] = 0.0
        del batch


def chain(m, rounds):
    st = m.store
    sums = st._segment_sums()
    rec = st._clip_buffers()
    elements = sum(n for _, n, _ in st.grad_segments)
    stream = ops._stream

    def run_chain():
        gradnorm.clip_finalize(sums.run(st.grad, stream()), 1.0, 1.0, rec, stream())

    def run_sumsq():
        sums.run(st.grad, stream())
    hyper = st.begin_update(max_steps=10000, group_lrs=[0.0] * 6, group_wds=[0.0] * 6)     # p stays where it is across repeats

    def run_adamw():
        for gi in range(6):
            a, b = st.segments[gi]
            st.adamw_range(a, min(b, st.trainable_end), gi, hyper)
    best = {k: float("inf") for k in ("sumsq", "chain", "adamw")}
    for _ in range(rounds):
        for k, fn in (("sumsq", run_sumsq), ("chain", run_chain), ("adamw", run_adamw)):
            best[k] = min(best[k], window(fn, 50))
    n_adamw = min(st.segments[5][1], st.trainable_end)
    sq_bytes, ad_bytes = 4 * elements, 30 * n_adamw
    say(f"[chain] {sums.nseg} segments, {sums.npieces} pieces of <= {gradnorm.PIECE} elements, {elements} elements "
        f"({sq_bytes / 1e9:.3f} GB read; buffer {st.grad.numel()} elements with padding)")
    say(f"[chain] m3ae_sumsq_segments (2 launches)              {best['sumsq'] * 1e3:8.1f} us  {sq_bytes / best['sumsq'] / 1e9:6.2f} TB/s of 4 B / element")
    say(f"[chain] + m3ae_clip_finalize (3 launches)             {best['chain'] * 1e3:8.1f} us  {sq_bytes / best['chain'] / 1e9:6.2f} TB/s")
    say(f"[chain] m3ae_adamw x 6 over the same buffer (bf16)    {best['adamw'] * 1e3:8.1f} us  {ad_bytes / best['adamw'] / 1e9:6.2f} TB/s of 30 B / element")
    r = (sq_bytes / best['sumsq']) / (ad_bytes / best['adamw'])
    say(f"[chain] double accumulation: sumsq bytes/s = {r:.2f} x the AdamW kernel's "
        f"({'stands' if r >= 1.0 else 'worse by ' + format((1 - r) * 100, '.0f') + ' %: kept, the accuracy contract outranks it'});  "
        f"chain / AdamW time = {best['chain'] / best['adamw']:.3f} (bytes alone predict {sq_bytes / ad_bytes:.3f})")


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-batches", default="256,32", help="per-GPU batches of the step timing ('' skips it)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r15_grad_clip.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/grad_clip_bench.py measures on the GPU; none is visible")
    _log = open(args.log, "w")
    ops.use_launch_stream()
    say(f"[grad_clip_bench] {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    cfg = finetune_vqa_rad_config(compute_dtype="bf16")
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    m.train(True)
    if args.step_batches:
        steps(m, cfg, [int(b) for b in args.step_batches.split(",")], args.steps, args.rounds)
    else:
        m.store.begin_update(max_steps=10000)      # allocates the moments
    chain(m, args.rounds)


if __name__ == "__main__":
    main()
