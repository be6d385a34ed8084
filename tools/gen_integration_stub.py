"""Regenerates the ctypes descriptor stubs of INTEGRATION.md from m3ae_amd/_lib.py (the binding the tests exercise), so the
documented struct layouts cannot drift from the library:   python tools/gen_integration_stub.py [--write]
tests/test_host_logic.py::test_descriptor_layouts_match_header_binding_and_integration_stub compares the committed block with this output."""
import collections
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mm-vqa-healthcare_amd"))
BEGIN, END = "<!-- BEGIN GENERATED (tools/gen_integration_stub.py) -->", "<!-- END GENERATED -->"
_NAMES = {C.c_double: "C.c_double", C.c_int64: "C.c_int64", C.c_int32: "C.c_int32", C.c_float: "C.c_float", C.c_void_p: "C.c_void_p",
          C.c_uint64: "C.c_uint64"}


def struct_stub(cls, c_name):
    lines, cur = [], " " * 16
    for n, t in cls._fields_:
        item = f'("{n}", {_NAMES[t]}), '
        if len(cur) + len(item) > 118:
            lines.append(cur.rstrip())
            cur = " " * 16
        cur += item
    lines.append(cur.rstrip().rstrip(","))
    body = "\n".join(lines)
    return f"class {cls.__name__}(C.Structure):      # mirrors {c_name} (include/m3ae_hip.h), {C.sizeof(cls)} bytes\n" \
           f"    _fields_ = [\n{body}]\n"


# The block after the descriptor classes, in order.  A section is a heading comment, constant lines -- (names of m3ae_amd/_lib.py,
# the text after their values) -- and the entry points whose restype / argtypes lines follow.
Section = collections.namedtuple("Section", "heading consts entries")
SECTIONS = {
    "LAUNCH_FLAGS": Section(
        "# launch_flags bits (fp32x3 mode, ABI 4: additive)",
        (("GEMM_NO_PERSISTENT, GEMM_F32_X3", "     # m3ae_gemm_desc.launch_flags"),
         ("ATTN_LEGACY_KERNELS, ATTN_F32_X3", "    # m3ae_attn_desc.launch_flags")),
        ()),
    "MAP_ENTRIES": Section(
        "# attention maps (ABI 4): fp32 [B, H, Lq, Lk] out of an m3ae_attn_fwd / m3ae_xattn_fwd call", (),
        ("m3ae_attn_probs", "m3ae_xattn_probs_export")),
    "DET_ENTRIES": Section(
        "# deterministic mode (ABI 4, additive): ordered reductions, caller-owned workspaces",
        (("GEMM_DETERMINISTIC", "     # m3ae_gemm_desc.launch_flags, accepted by m3ae_gemm_det only"),
         ("DET_COLSUM, DET_EMBED_BWD, DET_BCE, DET_XENT, DET_MIM", "     # m3ae_det_workspace_bytes(op, rows, cols)")),
        ("m3ae_gemm_det_workspace_bytes", "m3ae_gemm_det", "m3ae_det_workspace_bytes", "m3ae_colsum_det", "m3ae_layernorm_bwd_det",
         "m3ae_layernorm_bwd_drop_det", "m3ae_roberta_embed_bwd_det", "m3ae_bce_logits_det", "m3ae_xent_det", "m3ae_mim_loss_fwd_det")),
    "IMAGE_ENTRIES": Section(
        "# device image transform (ABI 4, additive): Pillow-exact bicubic resize + centre crop + normalize from the source bytes", (),
        ("m3ae_image_resample_workspace_bytes", "m3ae_image_resample_u8", "m3ae_image_resample_tables")),
    "RANDAUG_ENTRIES": Section(
        "# RandAugment(2, 9) on the source bytes of the device image transform (ABI 4, additive): Pillow-exact, two stages", (),
        ("m3ae_image_randaug_workspace_bytes", "m3ae_image_randaug_u8")),
    "ROWS_ENTRIES": Section(
        "# dropout row map (ABI 4, additive): mask row = row_base + row * row_step, (row_base, row_step) before the stream", (),
        ("m3ae_gemm_rows", "m3ae_attn_fwd_rows", "m3ae_attn_bwd_rows", "m3ae_layernorm_bwd_drop_rows", "m3ae_dropout_rows")),
    "SAMPLES_ENTRIES": Section(
        "# de-duplicated image batches (ABI 4, additive): out[b] = in[src[b]] over whole rows, and the ordered per-image sum back", (),
        ("m3ae_expand_samples", "m3ae_segment_sum_rows")),
    "MIXED_LN_ENTRIES": Section(
        "# fp32 residual stream of a bf16 model (ABI 4, additive): LayerNorm from fp32 rows to bf16 rows and its backward", (),
        ("m3ae_layernorm_fwd_mixed", "m3ae_layernorm_bwd_mixed", "m3ae_layernorm_bwd_mixed_det")),
    "TILED_ENTRIES": Section(
        "# tiled weight operand of the NT GEMMs (ABI 4, additive): B = the tiled copy of W[N][K] (csrc/tiled_b.h), same results",
        (("GEMM_B_TILED", "     # m3ae_gemm_desc.launch_flags; b_sk = 1, b_sn = K, B 16-byte aligned, K % 32 == 0"),),
        ("m3ae_tile_bf16_batched",)),
    "CLIP_ENTRIES": Section(
        "# gradient clipping by global norm + non-finite step guard (ABI 4, additive): double sums of squares, device-side factor",
        (("CLIP_NORM, CLIP_COEF, CLIP_SKIP, CLIP_STEPS, CLIP_CLIPPED_STEPS, CLIP_SKIPPED_STEPS, CLIP_RECORD_WORDS",
          "     # 32-bit words of the record"),),
        ("m3ae_sumsq_workspace_bytes", "m3ae_sumsq_segments", "m3ae_clip_finalize", "m3ae_adamw_clip")),
    "OPTIM_ENTRIES": Section(
        "# optim_type adam / sgd (ABI 4, additive): torch.optim.Adam and SGD with momentum over a flat segment; _clip = + the record", (),
        ("m3ae_adam", "m3ae_adam_clip", "m3ae_sgd", "m3ae_sgd_clip")),
    "EMA_ENTRIES": Section(
        "# EMA of the weights (ABI 4, additive): ema = fmaf(w, p - ema, ema) over a flat segment; exact p <-> ema swap + bf16 shadow", (),
        ("m3ae_ema_update", "m3ae_ema_swap")),
    "GREEDY_ENTRIES": Section(
        "# device-resident greedy search for the decoder head (ABI 4, additive): order keys per vocabulary chunk, then the step", (),
        ("m3ae_greedy_workspace_bytes", "m3ae_greedy_argmax", "m3ae_greedy_step")),
    "SUMMARY_ENTRIES": Section(
        "# attention summaries (ABI 4, additive): fp32 [B, Lk] head-and-query mean of a map without the map; heatmap upsample", (),
        ("m3ae_attn_colmean_workspace_bytes", "m3ae_attn_colmean", "m3ae_xattn_probs_colmean", "m3ae_heatmap_upsample")),
    "VQA_EVAL_ENTRIES": Section(
        "# device-side VQA evaluation (ABI 4, additive): prediction, top-k answers, the closed / open / overall record; token exact match",
        (("ANS_CLOSED, ANS_OPEN, VQA_REC_DOUBLES",
          "     # types values; double rec[10] = {n, sum_top1, sum_topk} x (all, closed, open), calls"),),
        ("m3ae_vqa_eval_workspace_bytes", "m3ae_vqa_eval", "m3ae_seq_match")),
    "TOKEN_EVAL_ENTRIES": Section(
        "# device-side token evaluation (ABI 4, additive): argmax, label rank, nll and top-k over vocabulary-wide rows; a loss mean",
        (("TOKEN_REC_DOUBLES, TOKEN_MAX_K, TOKEN_IGNORE",
          "     # double rec[5] = {n, hit1, hitk, sum_nll, calls}; the bound on k; the label that means no label"),),
        ("m3ae_token_eval_workspace_bytes", "m3ae_token_eval", "m3ae_record_add")),
    "LORA_ENTRIES": Section(
        "# LoRA, merged form (ABI 4, additive): W = W0 + s B A into master and shadow; dA, dB from the full dW; one table of targets",
        (("LORA_MAX_RANK, LORA_MAX_TARGETS, LORA_PANEL_ROWS", "     # bounds on r and ntargets; rows of one row panel of the projection"),),
        ("m3ae_lora_merge", "m3ae_lora_grad_workspace_bytes", "m3ae_lora_grad")),
    "ANSWER_TRIE_ENTRIES": Section(
        "# answer-list decoding (ABI 4, additive): greedy on a prefix trie of the candidate answers + the path's log-probability; label scoring",
        (),
        ("m3ae_trie_workspace_bytes", "m3ae_trie_scan", "m3ae_trie_step", "m3ae_vqa_label_eval")),
    "TRIE_BEAM_ENTRIES": Section(
        "# constrained beam search on the answer list (ABI 4, additive): best 2 nb children across beams, the scorer step, n-best label scoring",
        (),
        ("m3ae_triebeam_select", "m3ae_triebeam_step", "m3ae_vqa_labels_eval")),
    "LIST_SCORE_ENTRIES": Section(
        "# exhaustive answer-list scoring (ABI 4, additive): attention over trie ancestors; every entry's log-probability, k best, list mass",
        (),
        ("m3ae_tree_attn", "m3ae_listscore_workspace_bytes", "m3ae_listscore_lse", "m3ae_listscore_edges",
         "m3ae_listscore_fold_workspace_bytes", "m3ae_listscore_fold")),
}
globals().update({key: s.entries for key, s in SECTIONS.items() if s.entries})   # MAP_ENTRIES, DET_ENTRIES, ...: views of the table


def _ctype_name(t):
    if t in _NAMES:
        return _NAMES[t]
    if t is C.c_int:
        return "C.c_int"
    return f"C.POINTER({t._type_.__name__})"


def block():
    from m3ae_amd import _lib
    out = ["```python", "import ctypes as C", f"ABI_VERSION = {_lib.ABI_VERSION}        # == lib.m3ae_abi_version()", ""]
    out.append(struct_stub(_lib.GemmDesc, "m3ae_gemm_desc"))
    out.append(struct_stub(_lib.XattnDesc, "m3ae_xattn_desc"))
    out.append(struct_stub(_lib.AttnDesc, "m3ae_attn_desc"))
    for i, section in enumerate(SECTIONS.values()):
        out += [""] * (i > 0) + [section.heading]
        for names, tail in section.consts:
            out.append(f"{names} = {', '.join(str(getattr(_lib, n)) for n in names.split(', '))}{tail}")
        for name in section.entries:
            res, args = _lib._SIGS[name]
            out.append(f"lib.{name}.restype, lib.{name}.argtypes = {_ctype_name(res)}, [{', '.join(_ctype_name(a) for a in args)}]")
    out.append("```")
    return "\n".join(out)


if __name__ == "__main__":
    path = os.path.join(ROOT, "INTEGRATION.md")
    text = open(path).read()
    new = text[:text.index(BEGIN) + len(BEGIN)] + "\n" + block() + "\n" + text[text.index(END):]
    if "--write" in sys.argv:
        open(path, "w").write(new)
    else:
        print(block())
