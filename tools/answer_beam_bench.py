"""Constrained beam search on the answer list against the greedy list search (decoder head) and against the free beam search (T5):
Decoder.answer_beam_async / answer_path_async, T5ForConditionalGeneration.constrained_beam_async / generate_async.

    python tools/answer_beam_bench.py [--batches 8,64,256] [--dtypes bf16,fp32] [--beams 4] [--windows 3] [--calls 2]
                                      [--out profiles/r24_trie_beam.log]

The set-up of tools/answer_bench.py: the decoder head at its product dimensions (width 768, 8 heads, vocabulary 30522) on 2
encoder-side tokens, and its synthetic answer list (498 answers of 1 to 8 tokens, ending in [SEP]).  Per (dtype, B) the greedy list
search and the beam search alternate window by window in one process after a warm-up of both; a window is `calls` searches between
two device events (the second one synchronised).  Both run without early exit (lookahead=None), which gives a per-step figure for
each; then the beam search with lookahead 2.  Then the two new kernels alone on [B * beams, 30522] logits (a view of a buffer 30592
wide), every beam live at the root (the widest node): m3ae_trie_scan + m3ae_triebeam_select + m3ae_triebeam_step, next to
m3ae_trie_scan + m3ae_trie_step on [B, 30522].  Then t5-small: constrained_beam_async against the free generate_async at the same
number of beams (tools/generate_bench.py's model, 512 encoder tokens, max_length 12, answers ending in </s>).
Needs a GPU: there is no fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import generate_bench as GB  # noqa: E402
from answer_bench import MAX_TOKENS, synthetic_answers  # noqa: E402
from greedy_bench import D, LD, LE, MAXLEN, SEP, V, build, window  # noqa: E402


def t5_answers(seed=0, n=498, alphabet=300, eos=1):
    rng = np.random.default_rng(seed)
    toks = [int(t) for t in rng.permutation(GB.V)[:alphabet + 2] if int(t) not in (0, eos)][:alphabet]
    seen = set()
    while len(seen) < n:
        seen.add(tuple(int(rng.choice(toks)) for _ in range(int(rng.integers(1, MAX_TOKENS + 1)))))
    return [list(s) for s in sorted(seen)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,64,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_trie_beam.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("answer_beam_bench needs a GPU")
    from m3ae_amd import ops
    from m3ae_amd.answer_trie import AnswerTrie
    lines, nb = [], a.beams

    def say(s):
        print(s, flush=True)
        lines.append(s)

    trie = AnswerTrie.from_answers(synthetic_answers(), SEP)
    say(f"# decoder head, width {D}, V={V}, {LE} encoder tokens; {trie.num_answers} answers of 1..{MAX_TOKENS} tokens (+ [SEP]): "
        f"{trie.num_nodes} nodes, {trie.num_edges} edges, depth {trie.depth}, {len(trie.children(0)[0])} children at the root; {nb} beams, "
        f"length_penalty 0; {a.windows} alternating windows of {a.calls} calls, device events; {torch.cuda.get_device_name(0)}")
    batches = [int(b) for b in a.batches.split(",")]
    for dname in a.dtypes.split(","):
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        m = build(dtype)
        for B in batches:
            enc = (torch.randn(B, LE, D, generator=torch.Generator().manual_seed(B)) * 0.5).to("cuda", dtype)
            forms = {"greedy": lambda: m.answer_path_async(enc, trie, lookahead=None),
                     "beam": lambda: m.answer_beam_async(enc, trie, nb, 0.0, lookahead=None)}
            outs = {k: f() for k, f in forms.items()}     # warm-up of both forms, every shape
            assert int(outs["greedy"].err.cpu()) == 0 and int(outs["beam"].err.cpu()) == 0 and int(outs["beam"].n_hyp.cpu().min()) >= 1
            ms = {k: [] for k in forms}
            for _ in range(a.windows):
                for k, f in forms.items():
                    ms[k].append(window(f, a.calls)[0])
            gs, bs = outs["greedy"].steps, outs["beam"].steps
            gain = float((outs["beam"].score - outs["greedy"].score).mean().cpu())
            better = int((outs["beam"].score > outs["greedy"].score + 1e-4).sum().cpu())
            say(f"{dname} B={B:<3d} ms/search  greedy {min(ms['greedy']):8.2f} ({gs} steps, {min(ms['greedy']) / gs * 1e3:6.1f} us/step; windows "
                f"{' '.join(f'{x:.2f}' for x in ms['greedy'])})  beam {min(ms['beam']):8.2f} ({bs} steps at {B * nb} rows, "
                f"{min(ms['beam']) / bs * 1e3:6.1f} us/step; windows {' '.join(f'{x:.2f}' for x in ms['beam'])})  beam/greedy "
                f"{min(ms['beam']) / min(ms['greedy']):.2f}x  a more probable entry in {better} of {B} rows, mean log-probability gain {gain:.3f}")
            f = lambda: m.answer_beam_async(enc, trie, nb, 0.0, lookahead=2)   # noqa: E731
            f()
            t = min(window(f, a.calls)[0] for _ in range(a.windows))
            say(f"{dname} B={B:<3d}   answer_beam_async lookahead=2    {t:8.2f} ms/search, {f().steps} steps of {trie.depth}")
            del enc
        del m
        torch.cuda.empty_cache()
    for B in batches:
        for dname in a.dtypes.split(","):
            dtype = torch.bfloat16 if dname == "bf16" else torch.float32
            R = B * nb
            logits = (torch.randn(R, LD, device="cuda") * 2.0).to(dtype)[:, :V]
            tab = trie.to_device("cuda", V, MAXLEN, pad_id=0)
            st = ops.TrieBeamState(B, nb, MAXLEN, "cuda", 101, 0)
            ws = ops.trie_workspace(R, V, "cuda", 0)
            gst = ops.TrieState(B, MAXLEN, "cuda", 101, 0)
            gws = ops.trie_workspace(B, V, "cuda", 0)

            def reset():
                st.node.zero_()                  # every beam live at the root: the widest node, nb * 2 nb candidates kept per thread pass
                st.finished.zero_()
                st.done.zero_()
                st.n_hyp.zero_()

            def triple():
                reset()
                ops.trie_scan(logits, tab, st, 0, ws)
                ops.trie_beam_select(logits, tab, st, ws, 0)
                ops.trie_beam_step(tab, st, V, 0, 0.0)

            def select_only():
                ops.trie_beam_select(logits, tab, st, ws, 0)

            def pair():
                gst.finished.zero_()
                gst.node.zero_()
                ops.trie_scan(logits[:B], tab, gst, 0, gws)
                ops.trie_step(logits[:B], tab, gst, gws, 0, 0, 0)
            triple()
            pair()
            t3 = window(triple, a.reps)[0] * 1e3
            reset()
            ops.trie_scan(logits, tab, st, 0, ws)
            tsel = window(select_only, a.reps)[0] * 1e3
            t2 = window(pair, a.reps)[0] * 1e3
            say(f"     B={B:<3d} {dname}  scan + m3ae_triebeam_select + m3ae_triebeam_step on {R} rows {t3:7.1f} us (with four 1-launch resets); "
                f"m3ae_triebeam_select alone {tsel:6.1f} us;  scan + m3ae_trie_step on {B} rows {t2:7.1f} us "
                f"(with two resets)")
    t5trie = AnswerTrie.from_answers(t5_answers(), 1)
    say(f"# t5-small, V={GB.V}, {GB.LS} encoder tokens, max_length {GB.MAXLEN}; {t5trie.num_answers} answers (+ </s>), depth {t5trie.depth}; "
        f"free generate_async at {nb} beams (length_penalty 1) against constrained_beam_async at {nb} beams (length_penalty 0)")
    for dname in a.dtypes.split(","):
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        m = GB.build(dtype)
        for B in batches:
            enc = (torch.randn(B, GB.LS, 512, generator=torch.Generator().manual_seed(B)) * 0.5).to("cuda", dtype)
            forms = {"free": lambda: m.generate_async(enc, num_beams=nb, max_length=GB.MAXLEN, lookahead=None),
                     "list": lambda: m.constrained_beam_async(enc, t5trie, nb, GB.MAXLEN, 0.0, lookahead=None),
                     "greedy": lambda: m.constrained_greedy_async(enc, t5trie, max_length=GB.MAXLEN, lookahead=None)}
            outs = {k: f() for k, f in forms.items()}
            assert int(outs["list"].err.cpu()) == 0
            ms = {k: [] for k in forms}
            for _ in range(a.windows):
                for k, f in forms.items():
                    ms[k].append(window(f, a.calls)[0])
            say(f"t5 {dname} B={B:<3d} ms/search  free beam {min(ms['free']):8.2f} ({outs['free'].steps} steps)  list beam {min(ms['list']):8.2f} "
                f"({outs['list'].steps} steps, {min(ms['list']) / outs['list'].steps * 1e3:6.1f} us/step)  list greedy {min(ms['greedy']):8.2f} "
                f"({outs['greedy'].steps} steps)  free/list beam {min(ms['free']) / min(ms['list']):.2f}x  list beam/greedy "
                f"{min(ms['list']) / min(ms['greedy']):.2f}x")
            del enc
        del m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
