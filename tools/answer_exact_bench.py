"""Exhaustive scoring of the answer list against the constrained beam search (decoder head): Decoder.answer_scores_async against
Decoder.answer_beam_async at 4 and 8 beams.  The two sides compute different things (every entry's log-probability, the arg-max and a
distribution over the list, against a search result): the figures are reported, no speed is promised.

    python tools/answer_exact_bench.py [--batches 8,64,256] [--dtypes bf16,fp32] [--windows 3] [--calls 2] [--reps 50]
                                       [--out profiles/r27_answer_exact.log]

The set-up of tools/answer_bench.py: the decoder head at its product dimensions (width 768, 8 heads, vocabulary 30522) on 2
encoder-side tokens, and its synthetic answer list (498 answers of 1 to 8 tokens, ending in [SEP]); Ni, the trie nodes with children
(the decoder rows a sample costs), is printed.  Per (dtype, B) the three forms alternate window by window in one process after a
warm-up of all; a window is `calls` calls between two device events (the second one synchronised); the beam searches run without
early exit.  Then `max_rows` at three values: the default (the rows whose logits fill 2 GiB), a quarter of it and four samples a
group.  Then the three new kernels alone on [G * Ni, 30522] logits (a view of a buffer 30592 wide) at the group size the default
cap gives, and m3ae_tree_attn on the [Ni, 768] rows of the self-attention half.
Needs a GPU: there is no fallback."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from answer_bench import MAX_TOKENS, synthetic_answers  # noqa: E402
from greedy_bench import D, LD, LE, MAXLEN, SEP, V, build, window  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,64,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_answer_exact.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("answer_exact_bench needs a GPU")
    from m3ae_amd import ops
    from m3ae_amd.answer_trie import AnswerTrie
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    trie = AnswerTrie.from_answers(synthetic_answers(), SEP)
    Ni = len(trie.score_tables()["internal"])
    say(f"# decoder head, width {D}, V={V}, {LE} encoder tokens; {trie.num_answers} answers of 1..{MAX_TOKENS} tokens (+ [SEP]): "
        f"{trie.num_nodes} nodes, Ni = {Ni} with children, depth {trie.depth}, {len(trie.children(0)[0])} children at the root; "
        f"length_penalty 0, k = 5; {a.windows} alternating windows of {a.calls} calls, device events; {torch.cuda.get_device_name(0)}")
    batches = [int(b) for b in a.batches.split(",")]
    for dname in a.dtypes.split(","):
        dtype = torch.bfloat16 if dname == "bf16" else torch.float32
        m = build(dtype)
        cap = m.default_score_rows()
        for B in batches:
            enc = (torch.randn(B, LE, D, generator=torch.Generator().manual_seed(B)) * 0.5).to("cuda", dtype)
            forms = {"exact": lambda: m.answer_scores_async(enc, trie, 5, 0.0),
                     "beam4": lambda: m.answer_beam_async(enc, trie, 4, 0.0, lookahead=None),
                     "beam8": lambda: m.answer_beam_async(enc, trie, 8, 0.0, lookahead=None)}
            outs = {k: f() for k, f in forms.items()}     # warm-up of every form, every shape
            assert all(int(o.err.cpu()) == 0 for o in outs.values())
            ms = {k: [] for k in forms}
            for _ in range(a.windows):
                for k, f in forms.items():
                    ms[k].append(window(f, a.calls)[0])
            ex = outs["exact"]
            found = {k: int((outs[k].label == ex.label).sum().cpu()) for k in ("beam4", "beam8")}
            say(f"{dname} B={B:<3d} ms/call  exact {min(ms['exact']):8.2f} ({B * Ni} rows in {ex.groups} group(s); windows "
                f"{' '.join(f'{x:.2f}' for x in ms['exact'])})  beam4 {min(ms['beam4']):8.2f} ({outs['beam4'].steps} steps at {4 * B} rows)  "
                f"beam8 {min(ms['beam8']):8.2f} ({outs['beam8'].steps} steps at {8 * B} rows)  exact/beam4 "
                f"{min(ms['exact']) / min(ms['beam4']):.2f}x  exact/beam8 {min(ms['exact']) / min(ms['beam8']):.2f}x  the arg-max found by beam4 in "
                f"{found['beam4']} and by beam8 in {found['beam8']} of {B} rows; mean exp(log_mass) {float(torch.exp(ex.log_mass).mean().cpu()):.3g}")
            caps = {"default": cap, "quarter": max(cap // 4, Ni), "4 samples": 4 * Ni}
            cms = {k: [] for k in caps}
            for k, c in caps.items():
                m.answer_scores_async(enc, trie, 5, 0.0, max_rows=c)
            for _ in range(a.windows):
                for k, c in caps.items():
                    cms[k].append(window(lambda: m.answer_scores_async(enc, trie, 5, 0.0, max_rows=c), a.calls)[0])   # noqa: B023
            say(f"{dname} B={B:<3d}   max_rows  " + "  ".join(f"{k} ({c} rows, {-(-B // max(1, min(B, c // Ni)))} group(s)) {min(cms[k]):8.2f} ms"
                                                            for k, c in caps.items()))
            del enc
        # the kernels alone, at the group the default cap gives
        G = max(1, min(max(batches), cap // Ni))
        R = G * Ni
        logits = (torch.randn(R, LD, device="cuda") * 2.0).to(dtype)[:, :V]
        dt = trie.score_to_device("cuda", V, MAXLEN, 0)
        st = ops.ListScoreState(G, 5, MAXLEN, dt, "cuda", 0)
        ws = ops.listscore_workspace(R, V, "cuda", 0)
        qkv = (torch.randn(Ni, 3 * D, device="cuda") * 0.5).to(dtype)
        steps = {"m3ae_listscore_lse": lambda: ops.listscore_lse(logits, 0, ws),
                 "m3ae_listscore_edges": lambda: ops.listscore_edges(logits, dt, st, ws, 0, 0),
                 "m3ae_listscore_fold (+ the seq gather)": lambda: ops.listscore_fold(dt, st, 0.0),
                 "m3ae_tree_attn": lambda: ops.tree_attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], dt.anc, m.num_heads, err=st.err)}
        for f in steps.values():
            f()
        say(f"     {dname} kernels alone, G={G} samples, {R} rows:  "
            + "  ".join(f"{k} {window(f, a.reps)[0] * 1e3:8.1f} us" for k, f in steps.items()))
        del m, logits
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
