"""What the fp32 residual stream of the image tower costs and buys in bf16 mode (config key clip_residual_dtype).

    python tools/clip_residual_bench.py [--step-batches 256,32] [--steps 6] [--rounds 3] [--log profiles/r12_clip_residual.log]

The two settings ("bf16": the default, "fp32") alternate window by window in ONE process, as tools/deterministic_bench.py does:
1. the configs[1] training step (bench.py's step: zero_grad, forward, backward, AdamW; bf16, train-mode dropout), median step of
   each window, and the allocator's peak bytes of a step;
2. the image tower alone at the same batch: forward, and forward + backward;
3. the two mixed LayerNorm kernels at 147712 x 768 against the bytes they move (forward 4 + 2 B per element, backward 2 + 4 + 4
   read and 4 + 2 written with dx_add and dx_lo) and against the bf16 and fp32 LayerNorm kernels of the same shape;
4. the NT GEMMs of the block's two joins at 147712 rows (out-proj 768 x 768, fc2 768 x 3072, bias + residual) with an fp32 C and
   residual against their bf16-C siblings;
5. m3ae_amd/parity.py's full-size figures (configs[1] dimensions, B = 2, eval mode, tests/golden/full_vqa.npz) for both settings.

Times are device events on the launch stream.  A run without a GPU fails; nothing here falls back."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from m3ae_amd import _lib, ops, synth  # noqa: E402
from m3ae_amd.config import finetune_vqa_rad_config  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402

KEYS = ("bf16", "fp32")
BF, F32 = torch.bfloat16, torch.float32
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


def build(key, train):
    cfg = finetune_vqa_rad_config(compute_dtype="bf16", clip_residual_dtype=key)
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", BF)
    m.train(train)
    return cfg, m


def step_and_tower(batches, steps, rounds):
    from m3ae_amd.modules.objectives import build_vqa_targets
    models = {k: build(k, True) for k in KEYS}
    cfg = models["bf16"][0]
    for B in batches:
        batch = to_cuda(synth.synthetic_batch(B, text_len=cfg["max_text_len"], image_size=cfg["image_size"], rank=0))
        batch["vqa_targets"] = build_vqa_targets(batch, cfg["vqa_label_size"], torch.device("cuda"))

        def make_step(m):
            def step():
                m.store.zero_grad()
                loss = m.training_step(batch)
                loss.backward()
                m.store.adamw_step(max_steps=10000, grad_scale=1.0)
            return step
        step = {k: make_step(m) for k, (_, m) in models.items()}
        peak = {}
        for k in KEYS:          # warm both paths (code objects, allocator pools), and take the peak of one more step
            for _ in range(2):
                step[k]()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step[k]()
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated()
        med = {k: [] for k in KEYS}
        for _ in range(rounds):
            for k in KEYS:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
                for i in range(steps):
                    ev[i].record()
                    step[k]()
                ev[steps].record()
                torch.cuda.synchronize()
                med[k].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(steps)))
        a, o = min(med["bf16"]), min(med["fp32"])
        say(f"[step] configs[1] bf16 per-GPU batch {B}: bf16 stream {a:8.2f} ms/step ({B / a * 1e3:7.1f} samples/s)  fp32 stream {o:8.2f} ms/step "
            f"({B / o * 1e3:7.1f} samples/s)  ({(o / a - 1) * 100:+5.1f} %)   windows bf16 {[round(t, 2) for t in med['bf16']]} "
            f"fp32 {[round(t, 2) for t in med['fp32']]}   peak allocated {peak['bf16'] / 2 ** 30:.2f} / {peak['fp32'] / 2 ** 30:.2f} GiB "
            f"({(peak['fp32'] - peak['bf16']) / 2 ** 30:+.2f})")
        img = batch["image"][0]

        def make_tower(m, backward):
            def run():
                if backward:
                    m.store.zero_grad()
                    m.vision_encoder(img, BF).float().sum().backward()
                else:
                    with torch.no_grad():
                        m.vision_encoder(img, BF)
            return run
        for backward in (False, True):
            best = alternate({k: make_tower(m, backward) for k, (_, m) in models.items()}, 3, rounds)
            say(f"[tower] B {B} {'forward + backward' if backward else 'forward'}: bf16 stream {best['bf16']:8.2f} ms  fp32 stream "
                f"{best['fp32']:8.2f} ms  ({(best['fp32'] / best['bf16'] - 1) * 100:+5.1f} %)")
        del batch, img


def layernorm_kernels(M, D, rounds):
    import ctypes as C
    L = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = ops._stream
    x32, dy32, add32 = (torch.randn(M, D, device="cuda") for _ in range(3))
    xb, dyb, addb = x32.to(BF), dy32.to(BF), add32.to(BF)
    g, b = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    y32, yb, dx32, dxb, lo = torch.empty_like(x32), torch.empty_like(xb), torch.empty_like(x32), torch.empty_like(xb), torch.empty_like(xb)
    dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    ws = torch.empty(2 * L.m3ae_layernorm_bwd_blocks(M) * D, device="cuda")
    fwd = {
        "bf16 -> bf16": (lambda: L.m3ae_layernorm_fwd(p(xb), p(g), p(b), p(yb), p(mean), p(rstd), M, D, 1e-5, _lib.BF16, 0, 0, s()), 4),
        "fp32 -> fp32": (lambda: L.m3ae_layernorm_fwd(p(x32), p(g), p(b), p(y32), p(mean), p(rstd), M, D, 1e-5, _lib.F32, 0, 0, s()), 8),
        "fp32 -> bf16 (mixed)": (lambda: L.m3ae_layernorm_fwd_mixed(p(x32), p(g), p(b), p(yb), p(mean), p(rstd), M, D, 1e-5, s()), 6),
    }
    bwd = {
        "bf16, dx_add": (lambda: L.m3ae_layernorm_bwd(p(dyb), p(xb), p(g), None, p(mean), p(rstd), p(dxb), p(addb), p(dg), p(db), p(ws),
                                                      M, D, _lib.BF16, 0, 0, s()), 8),
        "fp32, dx_add": (lambda: L.m3ae_layernorm_bwd(p(dy32), p(x32), p(g), None, p(mean), p(rstd), p(dx32), p(add32), p(dg), p(db),
                                                      p(ws), M, D, _lib.F32, 0, 0, s()), 16),
        "mixed, dx_add": (lambda: L.m3ae_layernorm_bwd_mixed(p(dyb), p(x32), p(g), p(mean), p(rstd), p(dx32), p(add32), None, p(dg),
                                                             p(db), p(ws), M, D, s()), 14),
        "mixed, dx_add + dx_lo": (lambda: L.m3ae_layernorm_bwd_mixed(p(dyb), p(x32), p(g), p(mean), p(rstd), p(dx32), p(add32), p(lo),
                                                                     p(dg), p(db), p(ws), M, D, s()), 16),
        "mixed ordered, dx_add + dx_lo": (lambda: L.m3ae_layernorm_bwd_mixed_det(p(dyb), p(x32), p(g), p(mean), p(rstd), p(dx32),
                                                                                 p(add32), p(lo), p(dg), p(db), p(ws), M, D, s()), 16),
    }
    fwd["fp32 -> fp32"][0]()   # statistics for the backward forms
    for name, table in (("forward", fwd), ("backward", bwd)):
        best = alternate({k: f for k, (f, _) in table.items()}, 10, rounds)
        for k, (_, bytes_per_el) in table.items():
            us = best[k] * 1e3
            say(f"[layernorm {name}] {M} x {D} {k:32s} {us:7.1f} us  {bytes_per_el} B / element  {M * D * bytes_per_el / us / 1e6:5.2f} TB/s")


def join_gemms(M, rounds):
    for name, N, K in (("out-proj", 768, 768), ("fc2", 768, 3072)):
        a = (torch.randn(M, K, device="cuda") * 0.5).to(BF)
        w = (torch.randn(N, K, device="cuda") * K ** -0.5).to(BF)
        bias = torch.zeros(N, device="cuda")
        res32 = torch.randn(M, N, device="cuda")
        resb = res32.to(BF)
        cb, c32 = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, N, dtype=F32, device="cuda")
        fns = {"bf16 C": lambda: ops.gemm(a, K, 1, w, 1, K, cb, N, M, N, K, bias=bias, residual=resb),
               "fp32 C": lambda: ops.gemm(a, K, 1, w, 1, K, c32, N, M, N, K, bias=bias, residual=res32)}
        best = alternate(fns, 10, rounds)
        paths = {}
        for k, f in fns.items():
            f()
            paths[k] = ops.last_gemm_path()
        say(f"[join gemm] {name} {M} x {N} x {K} bias + residual: bf16 C {best['bf16 C'] * 1e3:7.1f} us ({paths['bf16 C']}, "
            f"{2.0 * M * N * K / best['bf16 C'] / 1e9:5.0f} TFLOP/s)  fp32 C {best['fp32 C'] * 1e3:7.1f} us ({paths['fp32 C']}, "
            f"{2.0 * M * N * K / best['fp32 C'] / 1e9:5.0f} TFLOP/s)  ({(best['fp32 C'] / best['bf16 C'] - 1) * 100:+5.1f} %, "
            f"{(best['fp32 C'] - best['bf16 C']) * 1e3:+6.1f} us)")
        del a, w, res32, resb, cb, c32


def parity():
    from m3ae_amd.parity import parity_report
    gpath = os.path.join(ROOT, "tests", "golden", "full_vqa.npz")
    golden = np.load(gpath, allow_pickle=False)
    batch = to_cuda(synth.synthetic_batch(2, text_len=32, image_size=384, vocab_size=50265, rank=0))
    for k in KEYS:
        _, m = build(k, False)
        r = parity_report(m, golden, batch)
        say(f"[parity] full size, B = 2, stream {k}: max |dlogits| {r['max_abs_dlogits']:.3e} (|logits| <= {r['max_abs_logits_ref']:.2f})  rms dlogits "
            f"{r['rms_dlogits']:.3e}  loss rel {r['loss_rel_err']:.3e}  global grad norm rel {r['global_grad_norm_rel_err']:.3e}  worst large "
            f"per-parameter grad norm rel {r['max_rel_err_large_param_grad_norms']:.3e} ({r['worst_large_param']})  median "
            f"{r['median_rel_err_param_grad_norms']:.3e}")
        del m


def main():
    global _log
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-batches", default="256,32", help="per-GPU batches of the step and tower timing ('' skips them)")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, default=147712, help="rows of the LayerNorm and join-GEMM tables (0 skips them)")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r12_clip_residual.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_residual_bench.py measures on the GPU; none is visible")
    _log = open(args.log, "w")
    ops.use_launch_stream()
    say(f"[clip_residual_bench] {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    if args.rows:
        layernorm_kernels(args.rows, 768, args.rounds)
        join_gemms(args.rows, args.rounds)
    if not args.no_parity:
        parity()
    if args.step_batches:
        step_and_tower([int(b) for b in args.step_batches.split(",")], args.steps, args.rounds)


if __name__ == "__main__":
    main()
