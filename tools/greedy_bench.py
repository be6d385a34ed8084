"""Decoder head greedy search, host against device form (m3ae_amd/modules/m3ae_decoder.py: Decoder.search_path(search=...) /
search_path_async).

    python tools/greedy_bench.py [--batches 8,64,256] [--dtypes bf16,fp32] [--windows 3] [--calls 2] [--out profiles/r17_greedy.log]

The decoder head at its product dimensions (width 768, 8 heads, vocabulary 30522, max_len 128) on 2 encoder-side tokens (the CLS
features).  Two weight sets: "open" (no row ever emits [SEP]: all 128 steps, the case the host form pays a blocking round trip
per token for) and "early" (the [SEP] bias raised until every row has finished within the first steps).  Per (dtype, weights, B):
the two forms alternate window by window in one process after a warm-up of both; a window is `calls` search_path calls between
two device events (the second one synchronised), so the figure is what a caller waits for.  Then the device form for lookahead 1,
2 and None (ms per call, steps enqueued), and m3ae_greedy_argmax alone on [B, 30522] bf16 and fp32 logits (a view of a buffer 30592
wide, as the vocabulary GEMM leaves them) for a few vocabulary splits, `reps` calls between two events, against the bytes it reads,
next to ATen argmax on the same view.  Needs a GPU: there is no fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))

import torch  # noqa: E402

V, LD, MAXLEN, LE, D, SEP = 30522, 30592, 128, 2, 768, 102


def build(dtype):
    """The decoder head alone (DecoderModel's constructor arguments), deterministic weights, its own parameter store."""
    from m3ae_amd import synth
    from m3ae_amd.config import tiny_config
    from m3ae_amd.modules.m3ae_decoder import Decoder
    from m3ae_amd.param_store import ParamStore, group_hparams_decoder, param_group_of_decoder
    m = Decoder(num_layers=6, d_model=D, num_heads=8, d_ff=4 * D, dropout=0.1, max_len=MAXLEN, target_vocab_size=V)
    synth.fill_deterministic(m)
    m.head_dtype = dtype
    mode = "bf16" if dtype == torch.bfloat16 else "fp32"
    ParamStore(m, tiny_config(compute_dtype=mode), "cuda", dtype, m.weight_units, group_fn=param_group_of_decoder,
               hparams_fn=group_hparams_decoder)
    for _, b in list(m.named_buffers()):
        b.data = b.data.to("cuda")
    return m.eval()


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,64,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_greedy.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("greedy_bench needs a GPU")
    from m3ae_amd import ops
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# decoder head, width {D}, V={V}, {LE} encoder tokens, max_len={MAXLEN}; {a.windows} alternating windows of {a.calls} calls, "
        f"device events; {torch.cuda.get_device_name(0)}")
    batches = [int(b) for b in a.batches.split(",")]
    for dname in a.dtypes.split(","):
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        m = build(dtype)
        bias = m.final_linear.bias
        open_bias = bias.data[SEP].clone()
        for weights in ("open", "early"):
            for B in batches:
                enc = (torch.randn(B, LE, D, generator=torch.Generator().manual_seed(B)) * 0.5).to("cuda", dtype)
                bias.data[SEP] = open_bias
                if weights == "early":      # raise the [SEP] bias until every row has finished within the first 16 steps
                    for delta in (0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0):
                        bias.data[SEP] = open_bias + delta
                        oc = m.search_path_async(enc, lookahead=None).state.open_count.cpu().tolist()
                        if 0 in oc[:16]:
                            break
                forms = {"host": lambda: m.search_path(enc), "device": lambda: m.search_path(enc, search="device")}
                outs = {k: f() for k, f in forms.items()}     # warm-up of both forms, every shape
                same = bool((outs["host"] == outs["device"]).all())
                ms = {k: [] for k in forms}
                for _ in range(a.windows):
                    for k, f in forms.items():
                        ms[k].append(window(f, a.calls)[0])
                full = m.search_path_async(enc, lookahead=None)
                oc = full.state.open_count.cpu().tolist()
                closed = next((t + 1 for t in range(MAXLEN) if oc[t] == 0), None)
                say(f"{dname} {weights:<5s} B={B:<3d} search_path ms/call  host {min(ms['host']):8.2f} (windows {' '.join(f'{x:.2f}' for x in ms['host'])})  "
                    f"device {min(ms['device']):8.2f} (windows {' '.join(f'{x:.2f}' for x in ms['device'])})  "
                    f"host/device {min(ms['host']) / min(ms['device']):.2f}x  all rows finished after step {closed}  same tokens {same}")
                for la in (1, 2, None):
                    f = lambda: m.search_path_async(enc, lookahead=la)   # noqa: E731
                    f()
                    t = min(window(f, a.calls)[0] for _ in range(a.windows))
                    say(f"{dname} {weights:<5s} B={B:<3d}   search_path_async lookahead={la!s:<4s} {t:8.2f} ms/call, {f().steps} steps of {MAXLEN}")
                del enc
        bias.data[SEP] = open_bias
        del m
        torch.cuda.empty_cache()
    for B in batches:
        for dname in a.dtypes.split(","):
            dtype = torch.bfloat16 if dname == "bf16" else torch.float32
            logits = (torch.randn(B, LD, device="cuda") * 2.0).to(dtype)[:, :V]
            mb = B * V * logits.element_size() / 1e6
            for chunk in (512, 1024, 2048, 4096, 8192):
                ws = ops.greedy_workspace(B, V, "cuda", chunk)
                ops.greedy_argmax(logits, chunk, ws)
                us = window(lambda: ops.greedy_argmax(logits, chunk, ws), a.reps)[0] * 1e3
                say(f"     B={B:<3d} {dname}  m3ae_greedy_argmax chunk={chunk:<4d} grid {B * -(-V // chunk):6d} workgroups  {us:7.1f} us/call  "
                    f"{mb:6.2f} MB read  {mb / us * 1e3:7.0f} GB/s")
            torch.argmax(logits, dim=-1)
            us = window(lambda: torch.argmax(logits, dim=-1), a.reps)[0] * 1e3
            say(f"     B={B:<3d} {dname}  ATen argmax on the same view {us:45.1f} us/call")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
