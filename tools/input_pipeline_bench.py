"""Host image transform against the device image transform (config key `image_transform`), on JPEG arrow tables.

    python tools/input_pipeline_bench.py [--batch 256] [--workers 16] [--batches 2] [--windows 3] [--size 384]
                                         [--sources 512,1024] [--out profiles/r07_input_pipeline.log]

Writes seeded JPEG tables in the prepro/make_arrow.py schema (PIL + pyarrow, nothing read from outside the tree) into a
temporary directory, one per source size, then per table:

1. producer throughput: `ArrowDataModule._stream` at `per_gpu_batchsize=batch`, `num_workers=workers`, with a consumer that
   only synchronises -- images/s of the host path and of the device path, the two alternating window by window in ONE process
   (the first window of each warms the table cache and the pinned allocator and is reported apart);
2. where the host time goes: per-image decode, decode + host transform, decode + device-path preparation on one core, and the
   packing of one batch;
3. device time of one batch from HIP events: the H2D copy of the packed sources, and the two passes of
   `m3ae_image_resample_u8` (median of `--iters`), with the bytes the passes must move (source rows read once, the uint8
   intermediate written and read, the fp32 output written) against the HBM rate of MI355X_MICROARCH.md.

4. the same for the train transform `clip_resizedcrop` (a random crop box per image and epoch, so a table set per image):
   producer images/s of the host and the device transform, every window a new epoch, and the device time of one batch split into
   `m3ae_image_resample_tables` (the coefficient tables built on the GPU) and the two passes, next to the `clip` figures above;
   nothing is asserted about these.

5. the same for `randaug=True` (RandAugment(2, 9) in front of the `clip` tail, two operations per image and epoch): producer
   images/s of the host path (Pillow runs the operations on the loader threads) and of the device path (csrc/randaug.hip), and
   the device time of the two stages of one batch (`m3ae_image_randaug_u8`, every timed call on a fresh copy of the sources)
   against the bytes they move (per stage every augmented image read and written once, and read once more where the stage takes
   a histogram).  This leg is also written to `--randaug-out` (profiles/r14_randaug.log); nothing is asserted about it.

A run without a GPU fails; nothing here falls back."""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from m3ae_amd import data, randaug, resample  # noqa: E402
from m3ae_amd.config import compose  # noqa: E402

HBM_ACHIEVABLE = 6.3e12   # MI355X_MICROARCH.md: 8.0 TB/s spec, about 6.3 TB/s measured with a float4 copy
DISTINCT = 16             # distinct images per table; the rows cycle through them


def vqa_rad_config(**over):
    """The fine-tuning config of run_scripts/finetune_m3ae.sh (config.finetune_vqa_rad_config) at the image size asked for."""
    return compose("task_finetune_vqa_vqa_rad", "clip16", "text_roberta", **over)


def jpeg(side, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:side, 0:side].astype(np.float32)
    a = np.stack([127.5 + 100 * np.sin(x / (11 + 3 * c + seed % 5)) * np.cos(y / (13 + 2 * c)) for c in range(3)], -1)
    a = np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)    # structure + grain: a radiograph-sized JPEG
    buf = io.BytesIO()
    Image.fromarray(a, "RGB").save(buf, format="JPEG", quality=90)
    return buf.getvalue()


def write_table(root, side, rows):
    import pyarrow as pa
    imgs = [jpeg(side, s) for s in range(DISTINCT)]
    cols = {"image": [imgs[i % DISTINCT] for i in range(rows)], "questions": [[f"what does image {i} show ?"] for i in range(rows)],
            "answers": [[["yes"]] for _ in range(rows)], "answer_labels": [[[i % 498]] for i in range(rows)],
            "answer_scores": [[[1.0]] for _ in range(rows)], "image_id": [f"img{i}" for i in range(rows)],
            "question_id": [[i] for i in range(rows)], "answer_type": [[i % 2] for i in range(rows)], "split": ["train"] * rows}
    table = pa.table(cols)
    os.makedirs(root, exist_ok=True)
    with pa.OSFile(os.path.join(root, "vqa_vqa_rad_train.arrow"), "wb") as sink:
        with pa.RecordBatchFileWriter(sink, table.schema) as writer:
            writer.write_table(table)
    return sum(len(b) for b in imgs) / len(imgs)


def producer_window(dm, epoch=None):
    idx = dm._indices(dm.train_set, 0, True)
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    for b in dm._stream(dm.train_set, idx, drop_last=True, epoch=epoch):
        torch.cuda.synchronize()
        n += b["image"][0].shape[0]
    return n / (time.perf_counter() - t0)


def per_image_host_times(table, size, n=16):
    from PIL import Image
    raws = [table["image"][i].as_py() for i in range(n)]
    t = {}
    t0 = time.perf_counter()
    for r in raws:
        Image.open(io.BytesIO(r)).load()
    t["decode"] = (time.perf_counter() - t0) / n
    t0 = time.perf_counter()
    for r in raws:
        data.load_image_u8(r, size, "host")
    t["decode + host transform"] = (time.perf_counter() - t0) / n
    t0 = time.perf_counter()
    srcs = [data.load_image_u8(r, size, "device") for r in raws]
    t["decode + device-path preparation"] = (time.perf_counter() - t0) / n
    return t, srcs


def event_ms(fn, iters):
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--batches", type=int, default=2, help="batches per window")
    ap.add_argument("--windows", type=int, default=3, help="windows per path, after one warm-up window each")
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--sources", default="512,1024")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_input_pipeline.log"))
    ap.add_argument("--randaug-out", default=os.path.join(ROOT, "profiles", "r14_randaug.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "input_pipeline_bench.py needs the GPU"
    from arrow_util import HashTokenizer
    lines, failed, aug_lines = [], [], []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/input_pipeline_bench.py  batch {a.batch}  workers {a.workers}  target {a.size}  {a.batches} batches/window  "
        f"{a.windows} windows/path  torch threads {torch.get_num_threads()}  {torch.cuda.get_device_name(0)}")
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        for side in [int(s) for s in a.sources.split(",")]:
            root = os.path.join(tmp, f"jpeg{side}")
            mean_bytes = write_table(root, side, a.batch * a.batches)
            say(f"\n## JPEG {side}x{side} sources -> {a.size} ({DISTINCT} distinct images, mean {mean_bytes / 1024:.0f} KiB, {a.batch * a.batches} rows)")
            dms = {}
            for mode in ("host", "device"):
                cfg = vqa_rad_config(data_root=root, per_gpu_batchsize=a.batch, num_workers=a.workers, image_size=a.size,
                                              image_transform=mode)
                dms[mode] = data.ArrowDataModule(cfg, 0, 1, dev, tokenizer=HashTokenizer())
            rates = {"host": [], "device": []}
            for w in range(a.windows + 1):
                for mode in ("host", "device"):
                    r = producer_window(dms[mode])
                    if w == 0:
                        say(f"producer warm-up window   {mode:6s} {r:9.1f} images/s")
                    else:
                        rates[mode].append(r)
                        say(f"producer window {w}          {mode:6s} {r:9.1f} images/s")
            mh, md = statistics.median(rates["host"]), statistics.median(rates["device"])
            say(f"producer throughput (median of {a.windows} windows): host {mh:.1f} images/s, device {md:.1f} images/s, "
                f"device / host = {md / mh:.2f}x;  routes of the device path: {dict(dms['device'].transform_stats)}")

            t, srcs = per_image_host_times(dms["host"].train_set.table, a.size)
            for k, v in t.items():
                say(f"one core, per image: {k:34s} {v * 1e3:8.2f} ms")
            srcs = [srcs[i % len(srcs)] for i in range(a.batch)]
            t0 = time.perf_counter()
            pack = resample.pack_batch(srcs, a.size, pin=True)
            t_pack = time.perf_counter() - t0
            t0 = time.perf_counter()
            pack = resample.pack_batch(srcs, a.size, pin=True)
            say(f"packing one batch of {a.batch} into pinned memory: first {t_pack * 1e3:.1f} ms, again {(time.perf_counter() - t0) * 1e3:.1f} ms "
                f"({pack['src'].numel() / 1e6:.1f} MB; one thread, per batch)")

            dst = torch.empty_like(pack["src"], device=dev)
            h2d_med, h2d_min = event_ms(lambda: dst.copy_(pack["src"], non_blocking=True), a.iters)
            dpack = resample.upload(pack, dev)
            torch.cuda.synchronize()
            resample.resample_on_device(dpack)   # warm the allocator: the timed calls launch the two kernels only
            k_med, k_min = event_ms(lambda: resample.resample_on_device(dpack), a.iters)
            plan = pack["plan"].numpy()
            src_b = int((plan[:, resample.PLAN_NROWS] * plan[:, resample.PLAN_W] * 3).sum())
            inter_b = resample.workspace_bytes(pack["rows"], a.size)
            out_b = a.batch * 3 * a.size * a.size * 4
            moved = src_b + 2 * inter_b + out_b
            say(f"H2D copy of the batch's sources ({pack['src'].numel() / 1e6:.1f} MB): median {h2d_med:.3f} ms, min {h2d_min:.3f} ms "
                f"({pack['src'].numel() / h2d_med / 1e6:.1f} GB/s)")
            say(f"m3ae_image_resample_u8, both passes, {a.batch} images: median {k_med:.3f} ms, min {k_min:.3f} ms "
                f"= {k_med / h2d_med:.3f} of the H2D copy")
            say(f"bytes the passes must move: sources {src_b / 1e6:.1f} MB + intermediate 2 x {inter_b / 1e6:.1f} MB + fp32 output "
                f"{out_b / 1e6:.1f} MB = {moved / 1e6:.1f} MB -> {moved / HBM_ACHIEVABLE * 1e3:.3f} ms at {HBM_ACHIEVABLE / 1e12:.1f} TB/s; "
                f"achieved {moved / k_med / 1e9:.2f} TB/s = {moved / k_med / 1e9 / (HBM_ACHIEVABLE / 1e12) * 100:.1f} % of the HBM rate")
            if not k_med < h2d_med:
                failed.append(f"{side}: the transform is slower than the upload of its input")
            if not md > mh:
                failed.append(f"{side}: the device path's producer is not faster than the host path's")

            # ---- train transform clip_resizedcrop: a box, and so a table set, per image and epoch
            crop = {}
            for mode in ("host", "device"):
                cfg = vqa_rad_config(data_root=root, per_gpu_batchsize=a.batch, num_workers=a.workers, image_size=a.size,
                                              image_transform=mode, train_transform_keys=["clip_resizedcrop"])
                crop[mode] = data.ArrowDataModule(cfg, 0, 1, dev, tokenizer=HashTokenizer())
            rates = {"host": [], "device": []}
            for w in range(a.windows + 1):
                for mode in ("host", "device"):
                    r = producer_window(crop[mode], epoch=w)
                    if w > 0:
                        rates[mode].append(r)
                    say(f"clip_resizedcrop producer {'warm-up window' if w == 0 else f'window {w}      '} {mode:6s} {r:9.1f} images/s")
            ch, cd = statistics.median(rates["host"]), statistics.median(rates["device"])
            say(f"clip_resizedcrop producer throughput (median of {a.windows} windows): host {ch:.1f} images/s, device {cd:.1f} "
                f"images/s, device / host = {cd / ch:.2f}x;  against clip: host {ch / mh:.2f}x, device {cd / md:.2f}x")
            boxes = [resample.random_resized_crop_box(s.shape[1], s.shape[0], resample.box_rng(0, 0, i, 0)) for i, s in enumerate(srcs)]
            t0 = time.perf_counter()
            bpack = resample.pack_batch(srcs, a.size, pin=True, boxes=boxes)
            t_pack = time.perf_counter() - t0
            n_sets = int(bpack["plan"][:, resample.PLAN_BUILD].sum())
            say(f"clip_resizedcrop: packing one batch of {a.batch} with boxes {t_pack * 1e3:.1f} ms; {n_sets} table sets, "
                f"{bpack['tab_ints'] * 4 / 1e6:.2f} MB of tables built on the device (none uploaded)")
            dbpack = resample.upload(bpack, dev)
            tab = torch.zeros(bpack["tab_ints"], dtype=torch.int32, device=dev)
            resample.build_tables_on_device(dbpack["plan"], a.size, tab)
            torch.cuda.synchronize()
            with_tab = {**dbpack, "tab": tab}
            resample.resample_on_device(with_tab)
            resample.resample_on_device(dbpack)
            t_med, t_min = event_ms(lambda: resample.build_tables_on_device(dbpack["plan"], a.size, tab), a.iters)
            p_med, p_min = event_ms(lambda: resample.resample_on_device(with_tab), a.iters)
            b_med, b_min = event_ms(lambda: resample.resample_on_device(dbpack), a.iters)
            say(f"clip_resizedcrop, {a.batch} images: m3ae_image_resample_tables median {t_med:.3f} ms, min {t_min:.3f} ms; the two "
                f"passes on built tables median {p_med:.3f} ms, min {p_min:.3f} ms (clip: {k_med:.3f} ms); tables + memset + passes as "
                f"resample_on_device runs them median {b_med:.3f} ms, min {b_min:.3f} ms")

            # ---- randaug: two operations per image and epoch in front of the clip tail
            first_aug_line = len(lines)
            aug = {}
            for mode in ("host", "device"):
                cfg = vqa_rad_config(data_root=root, per_gpu_batchsize=a.batch, num_workers=a.workers, image_size=a.size,
                                              image_transform=mode, randaug=True)
                aug[mode] = data.ArrowDataModule(cfg, 0, 1, dev, tokenizer=HashTokenizer())
            rates = {"host": [], "device": []}
            for w in range(a.windows + 1):
                for mode in ("host", "device"):
                    r = producer_window(aug[mode], epoch=w)
                    if w > 0:
                        rates[mode].append(r)
                    say(f"randaug producer {'warm-up window' if w == 0 else f'window {w}      '} {mode:6s} {r:9.1f} images/s")
            ah, ad = statistics.median(rates["host"]), statistics.median(rates["device"])
            say(f"randaug producer throughput, JPEG {side} (median of {a.windows} windows): host {ah:.1f} images/s, device {ad:.1f} "
                f"images/s, device / host = {ad / ah:.2f}x;  against clip (host {mh:.1f}, device {md:.1f} images/s): host {ah / mh:.2f}x, "
                f"device {ad / md:.2f}x;  routes of the device path: {dict(aug['device'].transform_stats)}")
            draws = [randaug.draw(randaug.aug_rng(0, 0, i, 0)) for i in range(a.batch)]
            t0 = time.perf_counter()
            apack = resample.pack_batch(srcs, a.size, pin=True, augs=draws)
            say(f"randaug: packing one batch of {a.batch} with its augment plan {(time.perf_counter() - t0) * 1e3:.1f} ms "
                f"(clip_resizedcrop, with boxes: {t_pack * 1e3:.1f} ms)")
            aplan = apack["aug"].numpy()
            npix = aplan[:, randaug.AUG_W] * aplan[:, randaug.AUG_H]
            moved, users = 0, []
            for st in range(2):
                ops = aplan[:, randaug.AUG_STAGE0 + randaug.AUG_STAGE_FIELDS * st]
                moved += int((3 * npix * (2 + np.isin(ops, randaug.HIST_OPS))).sum())
                users.append(int(np.isin(ops, randaug.HIST_OPS).sum()))
            dapack = resample.upload(apack, dev)
            pristine = dapack["src"].clone()
            scratch = torch.empty_like(pristine)
            randaug.augment_on_device(dapack["src"], dapack["aug"], dapack["aug_flags"], scratch=scratch)   # warm the allocator
            times = []
            for _ in range(a.iters):
                dapack["src"].copy_(pristine)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                randaug.augment_on_device(dapack["src"], dapack["aug"], dapack["aug_flags"], scratch=scratch)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            s_med, s_min = statistics.median(times), min(times)
            say(f"m3ae_image_randaug_u8, both stages, {a.batch} images of {side}x{side} (stage flags {apack['aug_flags']:#x}; histogram "
                f"users per stage {users}): median {s_med:.3f} ms, min {s_min:.3f} ms = {s_med / k_med:.2f} of the two resample passes "
                f"({k_med:.3f} ms), {s_med / h2d_med:.3f} of the H2D copy")
            say(f"bytes the stages must move: {moved / 1e6:.1f} MB -> {moved / HBM_ACHIEVABLE * 1e3:.3f} ms at "
                f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s; achieved {moved / s_med / 1e9:.2f} TB/s = "
                f"{moved / s_med / 1e9 / (HBM_ACHIEVABLE / 1e12) * 100:.1f} % of the HBM rate")
            aug_lines += [f"\n## JPEG {side}x{side} sources -> {a.size}", f"clip producer throughput (median of {a.windows} windows): host "
                          f"{mh:.1f} images/s, device {md:.1f} images/s; m3ae_image_resample_u8 median {k_med:.3f} ms"] + lines[first_aug_line:]
            del dms, dst, dpack, crop, dbpack, with_tab, tab, aug, dapack, pristine, scratch
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(a.randaug_out, "w") as f:
        f.write(lines[0] + "\n" + "\n".join(aug_lines) + "\n")
    if failed:
        raise SystemExit("FAILED: " + "; ".join(failed))


if __name__ == "__main__":
    main()
