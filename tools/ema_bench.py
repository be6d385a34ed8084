"""What the EMA of the weights (`ema_decay`) costs over the full-size flat buffers, against bytes moved and against the step.

    python tools/ema_bench.py [--rounds 3] [--iters 50] [--step-iters 6] [--batches 256 32] [--log profiles/r20_ema.log]

Three measurements over the configs[1] model in bf16 mode, each in windows that alternate with windows of its baseline in one
process, so every ratio is taken inside one thermal / clock state; the best window of either side counts, and the spread of the
windows (worst / best) is printed next to it:

  1. the six per-group launches of m3ae_ema_update against the six of m3ae_adamw on the same buffers.  Bytes per element: the EMA
     reads p and ema and writes ema = 12 B; AdamW reads p, g, m, v and writes p, m, v and the bf16 shadow = 30 B.  The prediction
     this run can falsify: both are HBM-streaming kernels, so the time ratio should be 12 / 30 = 0.40;
  2. ParamStore.ema_weights()'s entry (= its exit): m3ae_ema_swap over the trainable range + sync_shadows(cast=False);
  3. the training step (forward, backward, optimizer_step) with the key off against on, at each per-GPU batch of --batches: the
     delta is read against the spread of the step's own windows.

Times are device events on the launch stream.  A run without a GPU fails; nothing here falls back."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
import torch  # noqa: E402
from m3ae_amd import ops, synth  # noqa: E402
from m3ae_amd.config import ema_weight, finetune_vqa_rad_config  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from m3ae_amd.modules.objectives import build_vqa_targets  # noqa: E402

EMA_BYTES, ADAMW_BYTES = 12, 30
DECAY = 0.999
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


def alternate(base_fn, fn, rounds, iters):
    """([base windows], [windows]) in ms per call, windows of the two alternating."""
    base, mine = [], []
    for _ in range(rounds):
        base.append(window(base_fn, iters))
        mine.append(window(fn, iters))
    return base, mine


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-iters", type=int, default=6)
    ap.add_argument("--batches", type=int, nargs="*", default=[256, 32])
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r20_ema.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_bench.py measures on the GPU; none is visible")
    _log = open(args.log, "w")
    ops.use_launch_stream()
    say(f"[ema_bench] {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    cfg = finetune_vqa_rad_config(compute_dtype="bf16", ema_decay=DECAY)
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    m.train()
    st = m.store
    assert st.optim == "adamw" and st.ema_decay == DECAY
    # learning rate 0 and no decay: the parameters stay where they are across repeats while every load, operation and store runs
    still = dict(max_steps=10000, group_lrs=[0.0] * 6, group_wds=[0.0] * 6)
    hyper = st.begin_update(**still)            # (allocates both moments and the average)
    st.grad.normal_(0.0, 1e-3)
    st.ema.add_(torch.randn_like(st.ema) * 1e-3)                    # p != ema: the kernel's arithmetic sees ordinary values
    torch.cuda.synchronize()
    n = st.trainable_end
    say(f"[ema_bench] configs[1] bf16: {n} trainable elements with padding in 6 group segments; {args.rounds} rounds of alternating "
        f"windows of {args.iters} repeats ({args.step_iters} for the step), best window; spread = worst / best window")
    es, stream = 4, ops._stream
    import ctypes as C
    from m3ae_amd import _lib
    L = _lib.lib()
    w = ema_weight(DECAY, 1000, True)

    plain = {k: v for k, v in hyper.items() if k != "ema_w"}

    def adamw_six():
        for gi in range(6):
            a, b = st.segments[gi]
            st.update_range(a, min(b, n), gi, plain)

    def ema_six():
        for gi in range(6):
            a, b = st.segments[gi]
            b = min(b, n)
            if b > a:
                _lib.check(L.m3ae_ema_update(C.c_void_p(st.flat.data_ptr() + a * es), C.c_void_p(st.ema.data_ptr() + a * es), b - a, w,
                                             None, stream()), "m3ae_ema_update")

    base, mine = alternate(adamw_six, ema_six, args.rounds, args.iters)
    tb, tm = min(base), min(mine)
    say(f"[ema] m3ae_ema_update x 6  {tm * 1e3:8.1f} us  {EMA_BYTES * n / tm / 1e9:6.2f} TB/s of {EMA_BYTES} B / element (spread {max(mine) / tm:.3f})   "
        f"m3ae_adamw x 6 in the same windows {tb * 1e3:8.1f} us  {ADAMW_BYTES * n / tb / 1e9:6.2f} TB/s (spread {max(base) / tb:.3f})   "
        f"time ratio {tm / tb:.3f} (bytes alone predict {EMA_BYTES / ADAMW_BYTES:.3f})")

    def sync_twice():
        st.sync_shadows(cast=False)
        st.sync_shadows(cast=False)

    def enter_and_leave():           # (what `with st.ema_weights(): pass` launches; an even count of swaps leaves the weights in place)
        st._ema_swap()
        st._ema_swap()
    base, mine = alternate(sync_twice, enter_and_leave, args.rounds, args.iters)
    base, mine = [x / 2 for x in base], [x / 2 for x in mine]
    tb, tm = min(base), min(mine)
    say(f"[ema] ema_weights() entry = m3ae_ema_swap + sync_shadows(cast=False)  {tm * 1e3:8.1f} us (spread {max(mine) / tm:.3f})   "
        f"sync_shadows(cast=False) alone in the same windows {tb * 1e3:8.1f} us (spread {max(base) / tb:.3f})   "
        f"the swap: {(tm - tb) * 1e3:8.1f} us, {18 * n / max(tm - tb, 1e-9) / 1e9:6.2f} TB/s of 18 B / element")

    for B in args.batches:
        batch = to_dev(synth.synthetic_batch(B, text_len=cfg["max_text_len"], image_size=cfg["image_size"], rank=0))
        batch["vqa_targets"] = build_vqa_targets(batch, cfg["vqa_label_size"], torch.device("cuda", torch.cuda.current_device()))

        def step(decay):
            def run():
                st.ema_decay = decay          # begin_update reads it: 0.0 makes the step's calls what they are without the key
                st.zero_grad()
                out = m.training_step(batch)
                (out["loss"] if isinstance(out, dict) else out).backward()
                st.optimizer_step(**still)
            return run
        try:
            base, mine = alternate(step(0.0), step(DECAY), args.rounds, args.step_iters)
        finally:
            st.ema_decay = DECAY
        tb, tm = min(base), min(mine)
        say(f"[ema] step at per-GPU batch {B:4d}: key off {tb:8.3f} ms (spread {max(base) / tb:.3f})   ema_decay={DECAY} {tm:8.3f} ms "
            f"(spread {max(mine) / tm:.3f})   delta {(tm - tb) * 1e3:+8.1f} us = {100 * (tm - tb) / tb:+.2f} % of the step; "
            f"windows off {[round(x, 3) for x in base]} on {[round(x, 3) for x in mine]}")
        del batch
    if st._ema_open:
        raise SystemExit("the weights were left exchanged with their average")


if __name__ == "__main__":
    main()
