"""Pre-training metrics, ATen form against device form (m3ae_amd/metrics.py: TokenAccuracy; csrc/token_eval.hip; m3ae_amd/trainer.py:
Trainer.validate with pretrain_metrics="host" / "device").

    python tools/token_eval_bench.py [--windows 3] [--reps 20] [--val-batches 2] [--batch 64] [--chunks 0] [--skip-pass]
                                     [--out profiles/r21_token_eval.log]

  * the metric alone on MLM logits as the head leaves them -- bf16 [R, V], a view of a buffer padded to a multiple of 128 -- with
    15 % of the rows labelled, at R = 256 x 64, V = 30522 (task_pretrain_m3ae: BERT vocabulary, 64 tokens) and R = 256 x 40,
    V = 50265 (the RoBERTa vocabulary, 40 tokens).  "aten": logits.float().argmax(-1), a boolean index of predictions and labels,
    the count of hits, and F.cross_entropy(logits.float(), labels, ignore_index=-100) -- what a user would write.  "device k=0" /
    "device k=5": ops.token_eval with a record.  The forms alternate window by window in one process after a warm-up of each; a window
    is `reps` calls between two device events (the second one synchronised).  The bytes of the labelled rows over the device time
    is printed as GB/s: the kernel reads those rows once and no others.  `--chunks 0,4096,...` times the device forms at each
    of these values of `chunk` (0: the default);
  * one validation pass of the pre-training model (task_pretrain_m3ae, ViT-B/16, bf16, per-GPU batch `--batch`, `--val-batches`
    batches) with the key off ("host") and on ("device"), alternating windows likewise.
The device form reports accuracy, accuracy within the top 5, nll and perplexity; the ATen form here computes accuracy and the mean
loss.  Needs a GPU: there is no fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, out


def aten_form(logits, labels):
    x = logits.float()
    keep = labels != -100
    hits = (x.argmax(-1)[keep] == labels[keep]).sum()
    return hits, keep.sum(), F.cross_entropy(x, labels, ignore_index=-100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--val-batches", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--chunks", default="0")
    ap.add_argument("--skip-pass", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_token_eval.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("token_eval_bench needs a GPU")
    from m3ae_amd import config, ops, trainer
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    say(f"# token metrics, bf16 logits, 15 % of the rows labelled; {a.windows} alternating windows of {a.reps} calls; device events; "
        f"{torch.cuda.get_device_name(0)}")
    for R, V in ((256 * 64, 30522), (256 * 40, 50265)):
        g = torch.Generator(device=dev).manual_seed(R + V)
        ld = (V + 127) // 128 * 128
        buf = torch.empty((R, ld), dtype=torch.bfloat16, device=dev)
        buf.normal_(0.0, 2.0, generator=g)
        logits = buf[:, :V]
        labels = torch.randint(0, V, (R,), device=dev, generator=g)
        labels = torch.where(torch.rand(R, device=dev, generator=g) < 0.15, labels, torch.full_like(labels, -100))
        n = int((labels != -100).sum())
        rec = ops.token_record(dev)
        forms = {"aten": lambda: aten_form(logits, labels),
                 "device k=0": lambda: ops.token_eval(logits, labels, None, rec, k=0),
                 "device k=5": lambda: ops.token_eval(logits, labels, None, rec, k=5)}
        for c in [int(c) for c in a.chunks.split(",") if int(c)]:
            forms[f"device k=0 chunk={c}"] = lambda c=c: ops.token_eval(logits, labels, None, rec, k=0, chunk=c)
            forms[f"device k=5 chunk={c}"] = lambda c=c: ops.token_eval(logits, labels, None, rec, k=5, chunk=c)
        for f in forms.values():
            f()
        hits, total, ce = aten_form(logits, labels)
        rec.zero_()
        ops.token_eval(logits, labels, None, rec, k=5)
        r = rec.cpu().tolist()
        us = {k: [] for k in forms}
        for _ in range(a.windows):
            for k, f in forms.items():
                us[k].append(window(f, a.reps)[0] * 1e3)
        mb = n * V * 2 / 1e6
        say(f"R={R} V={V} labelled {n} ({mb:.0f} MB)  us/call  " +
            "  ".join(f"{k} {min(v):9.1f} (windows {' '.join(f'{x:.1f}' for x in v)})" for k, v in us.items()) +
            f"  device k=0 {mb / min(us['device k=0']) * 1e3:.0f} GB/s of labelled rows  "
            f"hits aten {int(hits)}/{int(total)} device {int(r[1])}/{int(r[0])} @5 {int(r[2])}  nll aten {float(ce):.6f} device {r[3] / max(r[0], 1):.6f}")
        del buf, logits, labels, forms
        torch.cuda.empty_cache()
    if not a.skip_pass:
        B = a.batch
        cfg = config.compose("task_pretrain_m3ae", "clip16", compute_dtype="bf16", per_gpu_batchsize=B, batch_size=B, max_steps=1,
                             eval_topk=5, log_dir=os.path.join(ROOT, "result"))
        model = trainer.build_model(cfg, "cls", dev)
        dm = trainer.SyntheticDataModule(cfg, 0, 1, dev, pool=1, train_samples=B, val_samples=a.val_batches * B)
        for b in dm.val_pool:       # fixed ITM pairs: without them every pass draws its own, and the monitored values differ
            b["itm_labels"] = (torch.arange(B) % 2).float()
        tr = trainer.Trainer(cfg, model, dm, 0, 1, dev)

        def run(form):
            tr.pretrain_metrics = form
            return tr.validate()
        vals = {f: run(f) for f in ("host", "device")}          # warm-up of both forms
        ms = {f: [] for f in vals}
        for _ in range(a.windows):
            for f in ms:
                ms[f].append(window(lambda: run(f), 1)[0])
        say(f"task_pretrain_m3ae ViT-B/16 bf16 B={B}, validation pass of {a.val_batches} batches, ms  "
            f"host {min(ms['host']):9.2f} (windows {' '.join(f'{x:.2f}' for x in ms['host'])})  "
            f"device {min(ms['device']):9.2f} (windows {' '.join(f'{x:.2f}' for x in ms['device'])})  "
            f"monitored host {vals['host']:.6f} device {vals['device']:.6f} {tr.pretrain_text().strip()}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
