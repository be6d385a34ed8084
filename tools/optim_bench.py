"""What the three optimizer rules of `optim_type` cost over the full-size flat buffers, against bytes moved.

    python tools/optim_bench.py [--rounds 3] [--iters 50] [--log profiles/r16_optim.log]

The six per-group launches of m3ae_adamw, m3ae_adam and m3ae_sgd, each in its plain and its _clip form (the record holds coef 1, no
skip: the launch reads it and does the whole update), over the configs[1] model's buffers in bf16 mode.  Every variant is timed in
windows that alternate with windows of plain m3ae_adamw on the same buffers in one process, so each ratio is taken inside one
thermal / clock state; the best window of either side counts.

Bytes per element: AdamW and Adam read p, g, m, v and write p, m, v (fp32) and the bf16 shadow = 30 B; SGD reads p, g, buf and writes
p, buf and the shadow = 22 B.  The prediction this run can falsify: all three are HBM-streaming kernels with a handful of fp32
operations per element, so SGD / AdamW time should be 22 / 30 = 0.73, Adam / AdamW 1.0 (one more division per element), and the
_clip forms cost nothing beside their plain forms (two scalar loads per wave).

Times are device events on the launch stream.  A run without a GPU fails; nothing here falls back."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
import torch  # noqa: E402
from m3ae_amd import _lib, ops, synth  # noqa: E402
from m3ae_amd.config import finetune_vqa_rad_config  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402

BYTES = {"adamw": 30, "adam": 30, "sgd": 22}
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


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r16_optim.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_bench.py measures on the GPU; none is visible")
    _log = open(args.log, "w")
    ops.use_launch_stream()
    say(f"[optim_bench] {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    m = M3AETransformerSS(finetune_vqa_rad_config(compute_dtype="bf16"))
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    st = m.store
    assert st.optim == "adamw"
    # learning rate 0 and no decay: the parameters stay where they are across repeats while every load, operation and store runs
    hyper = st.begin_update(max_steps=10000, group_lrs=[0.0] * 6, group_wds=[0.0] * 6)       # (allocates both moments)
    st.grad.normal_(0.0, 1e-3)
    rec = st._clip_buffers()
    rec[_lib.CLIP_COEF] = 1.0
    torch.cuda.synchronize()
    n = min(st.segments[5][1], st.trainable_end)
    say(f"[optim_bench] configs[1] bf16: {n} trainable elements in 6 group segments, {st.grad.numel()} with padding; "
        f"{args.rounds} rounds of alternating windows of {args.iters} repeats, best window")

    def runner(rule, clip):
        def run():
            st.optim = rule           # the store dispatches on it; the buffers are the same
            for gi in range(6):
                a, b = st.segments[gi]
                st.update_range(a, min(b, st.trainable_end), gi, hyper, rec if clip else None)
        return run
    base_run = runner("adamw", False)
    try:
        for rule in ("adamw", "adam", "sgd"):
            for clip in (False, True):
                run = runner(rule, clip)
                base, best = float("inf"), float("inf")
                for _ in range(args.rounds):
                    base = min(base, window(base_run, args.iters))
                    best = min(best, window(run, args.iters))
                name = f"m3ae_{rule}{'_clip' if clip else ''}"
                say(f"[optim] {name:16s} x 6  {best * 1e3:8.1f} us  {BYTES[rule] * n / best / 1e9:6.2f} TB/s of {BYTES[rule]} B / element   "
                    f"m3ae_adamw in the same windows {base * 1e3:8.1f} us  {30 * n / base / 1e9:6.2f} TB/s   time ratio {best / base:.3f} "
                    f"(bytes alone predict {BYTES[rule] / 30:.3f})")
    finally:
        st.optim = "adamw"


if __name__ == "__main__":
    main()
