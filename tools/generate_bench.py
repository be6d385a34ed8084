"""T5 generate, host against device beam search (m3ae_amd/modules/t5.py: generate(beam_search=...) / generate_async).

    python tools/generate_bench.py [--batches 8,64,256] [--dtypes bf16,fp32] [--windows 3] [--calls 4] [--out profiles/r10_generate.log]

T5-small dimensions, vocabulary 32128, 512 encoder tokens, 4 beams, max_length 12.  Per (dtype, B): the two forms alternate window
by window in one process after a warm-up of both; a window is `calls` generate calls ended by a device synchronise, timed with the
host clock (what a caller of generate waits for).  Then the device form for lookahead 1, 2 and None (ms per call, steps enqueued),
and m3ae_beam_topk alone on a [B * 4, 32128] logits buffer for every vocabulary split, timed with device events around `reps`
calls, against the bytes it reads (two passes over the logits).  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))

import torch  # noqa: E402

NB, MAXLEN, V, LS = 4, 12, 32128, 512


def build(dtype):
    from m3ae_amd import synth
    from m3ae_amd.config import tiny_config
    from m3ae_amd.modules.t5 import T5ForConditionalGeneration
    from m3ae_amd.param_store import ParamStore, group_hparams_decoder, param_group_of_decoder
    m = T5ForConditionalGeneration("t5-small", V)
    sd = {"t5." + k: v for k, v in m.state_dict().items()}
    synth.fill_deterministic(sd)
    for k in sd:   # weights large enough for peaked next-token distributions (the recipe of the generate fixture)
        if any(t in k for t in (".q.weight", ".k.weight", ".v.weight", ".o.weight", ".wi.weight", ".wo.weight")):
            sd[k].mul_(8.0)
    sd["t5.shared.weight"].copy_(synth.det_normal("t5.shared.weight", sd["t5.shared.weight"].shape, std=0.3))
    m.load_state_dict({k[3:]: v for k, v in sd.items()})
    mode = "bf16" if dtype == torch.bfloat16 else "fp32"
    ParamStore(m, tiny_config(compute_dtype=mode), "cuda", dtype, m.weight_units, group_fn=param_group_of_decoder,
               hparams_fn=group_hparams_decoder)
    return m.eval()


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,64,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_generate.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generate_bench needs a GPU")
    from m3ae_amd import ops
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# T5-small, V={V}, {LS} encoder tokens, {NB} beams, max_length={MAXLEN}; {a.windows} alternating windows of {a.calls} calls; "
        f"{torch.cuda.get_device_name(0)}")
    for dname in a.dtypes.split(","):
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        m = build(dtype)
        for B in (int(b) for b in a.batches.split(",")):
            enc = (torch.randn(B, LS, 512, generator=torch.Generator().manual_seed(B)) * 0.5).to("cuda", dtype)
            forms = {"host": lambda: m.generate(enc, NB, MAXLEN, beam_search="host"),
                     "device": lambda: m.generate(enc, NB, MAXLEN, beam_search="device")}
            outs = {k: f() for k, f in forms.items()}     # warm-up of both forms, every shape
            same = outs["host"].shape == outs["device"].shape and bool((outs["host"] == outs["device"]).all())
            ms = {k: [] for k in forms}
            for _ in range(a.windows):
                for k, f in forms.items():
                    ms[k].append(window(f, a.calls)[0])
            steps = m.generate_async(enc, NB, MAXLEN).steps
            say(f"{dname} B={B:<3d} generate ms/call  host {min(ms['host']):8.2f} (windows {' '.join(f'{x:.2f}' for x in ms['host'])})  "
                f"device {min(ms['device']):8.2f} (windows {' '.join(f'{x:.2f}' for x in ms['device'])})  "
                f"host/device {min(ms['host']) / min(ms['device']):.2f}x  device steps {steps} of {MAXLEN - 1}  same tokens {same}")
            for la in (1, 2, None):
                f = lambda: m.generate_async(enc, NB, MAXLEN, lookahead=la)   # noqa: E731
                f()
                t = min(window(f, a.calls)[0] for _ in range(a.windows))
                say(f"{dname} B={B:<3d}   generate_async lookahead={la!s:<4s} {t:8.2f} ms/call, {f().steps} steps")
            if dname == a.dtypes.split(",")[0]:     # the top-k reads fp32 logits in either mode: once per B
                R = B * NB
                logits = torch.randn(R, V, device="cuda") * 2.0
                scores = torch.rand(R, device="cuda") * -30.0
                for chunk in (1024, 2048, 4096):
                    ws = ops.beam_topk_workspace(B, NB, V, "cuda", chunk)
                    ops.beam_topk(logits, scores, B, NB, chunk, ws)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        ops.beam_topk(logits, scores, B, NB, chunk, ws)
                    e1.record()
                    e1.synchronize()
                    us = e0.elapsed_time(e1) * 1e3 / a.reps
                    gb = 2 * R * V * 4 / 1e9
                    say(f"     B={B:<3d}   m3ae_beam_topk chunk={chunk:<4d} grid {R * -(-V // chunk):6d} workgroups  {us:8.1f} us/step  "
                        f"{gb * 1e3:7.1f} MB read (2 passes)  {gb / (us * 1e-6):7.0f} GB/s")
                t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0[0].record()
                for _ in range(a.reps):
                    torch.topk((torch.log_softmax(logits, dim=-1) + scores[:, None]).view(B, NB * V), 2 * NB, dim=1)
                t0[1].record()
                t0[1].synchronize()
                say(f"     B={B:<3d}   ATen log_softmax + add + topk (the host form's three ops) {t0[0].elapsed_time(t0[1]) * 1e3 / a.reps:8.1f} us/step")
            del enc
        del m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
