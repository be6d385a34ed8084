/*
 * m3ae_hip.h -- C ABI of libm3ae_hip.so: the MI355X (gfx950) kernels behind the M3AE Med-VQA hot path.
 *
 * The reference (better62/MM-VQA-Healthcare) is 100 % Python: it has no FFI / plugin interface for this path.
 * Its boundary is the nn.Module tree of M3AETransformerSS (m3ae/modules/m3ae_module.py:16) whose blocks call
 * PyTorch ATen ops.  Each entry point below replaces the ATen call chain of one reference code site (cited per
 * function); the Python modules in mm-vqa-healthcare_amd/m3ae_amd/modules/ keep the reference's module / parameter
 * names and call these entry points through ctypes (m3ae_amd/_lib.py).  See INTEGRATION.md for the binding stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  All pointers are DEVICE pointers unless noted.
 *   - Every function is stream-ordered on `stream` (a hipStream_t passed as void*), never synchronises the host,
 *     allocates nothing and keeps no mutable global state; the caller owns every buffer incl. workspaces.
 *   - Return value: 0 = ok; M3AE_ERR_* (negative) = rejected before launch; positive = hipError_t of the launch.
 *   - dtype: activations are M3AE_BF16 ("perf mode") or M3AE_F32 ("parity mode"); parameters that are vectors
 *     (biases, LayerNorm scale/shift), embedding tables, masks, statistics and gradients of parameters are fp32.
 */
#ifndef M3AE_HIP_H
#define M3AE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: m3ae_gemm_desc grew `preact_grad` and `launch_flags` (round 2), m3ae_xattn_desc grew `launch_flags` and dir 1 takes
 *    probs == NULL (forward-only calls); m3ae_desc_sizes() lets a binding check its struct layouts at load time. */
/* 3: dropout salt (round 4).  m3ae_gemm_desc / m3ae_attn_desc / m3ae_xattn_desc grew `dropout_salt`, m3ae_layernorm_bwd_drop and
 *    m3ae_dropout take it as an argument: an optional DEVICE pointer to a 32-bit value the kernels fold into the mask key, so a
 *    step captured in a hipGraph (kernel arguments frozen, seeds included) draws new masks at every replay once the caller bumps
 *    that value; m3ae_adamw takes `hyper_dev` (device {lr, step size} of the step) for the same reason. */
/* 4 (additive): deterministic mode.  M3AE_GEMM_DETERMINISTIC + m3ae_gemm_det / m3ae_gemm_det_workspace_bytes (ordered split-K of the
 *    wgrad kernels) and the *_det forms of the small reductions, all taking a caller-owned workspace; no descriptor changed. */
/* 4: attention maps.  m3ae_attn_probs (the probabilities of an m3ae_attn_fwd call, recomputed from its log-sum-exp table) and
 *    m3ae_xattn_probs_export (the probabilities a fused cross-attention call left in `probs` / `probs_drop`), both as fp32
 *    [B][H][Lq][Lk]; no descriptor changed. */
/* 4 (additive): device image transform.  m3ae_image_resample_u8 / m3ae_image_resample_workspace_bytes (Pillow-exact bicubic resize +
 *    centre crop + ToTensor / Normalize from the decoded source bytes); no descriptor changed. */
/* 4 (additive): m3ae_image_resample_tables builds the tables of m3ae_image_resample_u8 on the device (random resized crop: a
 *    resample of its own per image); plan field 13 marks the records it writes; no descriptor changed. */
/* 4 (additive): dropout row map.  m3ae_gemm_rows, m3ae_attn_fwd_rows / m3ae_attn_bwd_rows, m3ae_layernorm_bwd_drop_rows and
 *    m3ae_dropout_rows: the entry points they are named after with (row_base, row_step), so that a call on a subset of a tensor's
 *    rows draws the dropout masks of the full tensor (see m3ae_dropout); no descriptor changed. */
/* 4 (additive): device-resident beam search.  m3ae_beam_topk (+ m3ae_beam_topk_workspace_bytes), m3ae_beam_step and
 *    m3ae_beam_finalize (csrc/beam.hip); no descriptor changed. */
/* 4 (additive): tiled weight operand of the NT GEMMs.  M3AE_GEMM_B_TILED in m3ae_gemm_desc.launch_flags and m3ae_tile_bf16_batched,
 *    which writes the tiled copies (layout: csrc/tiled_b.h); no descriptor changed. */
/* 4 (additive): gradient clipping by global norm with a non-finite step guard.  m3ae_sumsq_segments (+ m3ae_sumsq_workspace_bytes),
 *    m3ae_clip_finalize and m3ae_adamw_clip (csrc/gradnorm.hip, csrc/misc.hip); the device record is plain 32-bit words
 *    (M3AE_CLIP_*), no descriptor changed and m3ae_adamw keeps its signature. */
/* 4 (additive): the optim_type rules next to AdamW.  m3ae_adam, m3ae_sgd and their _clip forms (csrc/misc.hip); no descriptor
 *    changed. */
/* 4 (additive): device-resident greedy search for the decoder head.  m3ae_greedy_argmax (+ m3ae_greedy_workspace_bytes) and
 *    m3ae_greedy_step (csrc/greedy.hip); no descriptor changed. */
/* 4 (additive): attention summaries.  m3ae_attn_colmean (+ m3ae_attn_colmean_workspace_bytes) and m3ae_xattn_probs_colmean: the mean
 *    of an attention map over heads and queries, fp32 [B][Lk], without the map; m3ae_heatmap_upsample (csrc/heatmap.hip): bilinear
 *    upsample of a patch grid; no descriptor changed. */
/* 4 (additive): device-side VQA evaluation.  m3ae_vqa_eval (+ m3ae_vqa_eval_workspace_bytes) and m3ae_seq_match
 *    (csrc/vqa_eval.hip): prediction, top-k answers and the closed / open / overall score record; no descriptor changed. */
/* 4 (additive): exponential moving average of the weights.  m3ae_ema_update and m3ae_ema_swap (csrc/misc.hip); no descriptor
 *    changed. */
/* 4 (additive): device-side token evaluation for rows of vocabulary width.  m3ae_token_eval (+ m3ae_token_eval_workspace_bytes) and
 *    m3ae_record_add (csrc/token_eval.hip): argmax, label rank, negative log-likelihood, top-k tokens with softmax probabilities and
 *    the {n, hit1, hitk, sum_nll, calls} record of the labelled rows; no descriptor changed. */
/* 4 (additive): LoRA in merged form on the flat buffers.  m3ae_lora_merge, m3ae_lora_grad and m3ae_lora_grad_workspace_bytes
 *    (csrc/lora.hip): W = W0 + s B A written into the master and shadow buffers, and dA / dB projected out of the full weight
 *    gradient, each as one grouped launch chain over a device table of targets; no descriptor changed. */
/* 4 (additive): answer-list decoding for the generator heads.  m3ae_trie_scan (+ m3ae_trie_workspace_bytes) and m3ae_trie_step
 *    (csrc/answer_trie.hip): greedy search constrained to a prefix trie of the candidate answers, with the log-probability of the
 *    chosen path; m3ae_vqa_label_eval (csrc/vqa_eval.hip): the score record from labels instead of logits; no descriptor changed. */
/* 4 (additive): constrained beam search on the answer list.  m3ae_triebeam_select and m3ae_triebeam_step (csrc/trie_beam.hip): the
 *    BeamSearchScorer of m3ae_beam_step with the trie as the prefix constraint and an n-best list of labels with scores as the
 *    result; m3ae_vqa_labels_eval (csrc/vqa_eval.hip): the score record from n-best labels; no descriptor changed. */
/* 4 (additive): exhaustive answer-list scoring.  m3ae_tree_attn (csrc/tree_attn.hip): attention whose keys are a row's trie
 *    ancestors; m3ae_listscore_lse (+ m3ae_listscore_workspace_bytes), m3ae_listscore_edges and m3ae_listscore_fold (+
 *    m3ae_listscore_fold_workspace_bytes) (csrc/list_score.hip): every list entry's log-probability from one pass over the trie's
 *    internal nodes, the k best entries, probabilities over the list and the list's mass; no descriptor changed. */
#define M3AE_ABI_VERSION 4

enum { M3AE_F32 = 0, M3AE_BF16 = 1 };
enum { M3AE_ACT_NONE = 0, M3AE_ACT_GELU = 1, M3AE_ACT_QUICKGELU = 2, M3AE_ACT_TANH = 3, M3AE_ACT_RELU = 4,
       M3AE_ACT_MULAUX = 5 /* dact only: dact_aux already holds act'(pre) (written by a forward with preact_grad) */ };
enum { M3AE_ERR_ARG = -1, M3AE_ERR_UNSUPPORTED = -2, M3AE_ERR_ALIGN = -3, M3AE_ERR_WORKSPACE = -4 };

int m3ae_abi_version(void);
/* sizeof(m3ae_gemm_desc), sizeof(m3ae_attn_desc), sizeof(m3ae_xattn_desc) as this library was compiled: a binding compares
 * them with its own struct definitions before the first call (a descriptor that is too short is read past its end). */
void m3ae_desc_sizes(int64_t out3[3]);
/* name of the kernel family the last m3ae_gemm call on this thread dispatched to ("mfma_nt", "mfma_tn", "generic", "f32x3") */
const char* m3ae_last_gemm_path(void);

/* ------------------------------------------------------------------------------------------------------------
 * GEMM with fused epilogue.  Replaces nn.Linear / torch.matmul / F.conv2d(k=s=patch) call sites:
 *   clip_model.py:44,47-49,58,94 (packed in-proj, out-proj, c_fc, c_proj, patch-embed conv as GEMM);
 *   bert_model.py:224-226,263,276-277,356,361,419,426,434,439 (Q/K/V, attention output, intermediate, output);
 *   m3ae_module.py:70-73,120-125,235,252 (modality projections, vqa_head); prediction_heads.py:12,17 (Pooler);
 *   and their autograd backward (dgrad / wgrad).
 *
 *   C[b1][b2][m][n] = epi( alpha * sum_k A[b1][b2][m][k] * B[b1][b2][k][n] )
 *   epi(x): x += bias[n]; if (preact) preact[m][n] = preact_grad ? act'(x) : x; x = act(x);
 *           if (residual) x += residual[m][n];
 *           if (dact_aux) x *= act'(dact_aux[m][n]) (derivative of `dact` at the saved pre-activation);
 *           if (accumulate) C += x else C = x.
 * Strides are in ELEMENTS.  preact / residual / dact_aux share C's strides and dtype.
 * a_rowsum (single-batch only: M3AE_ERR_UNSUPPORTED, before any launch, with batch1 * batch2 != 1 -- the vector has no batch
 * stride): additionally accumulates the row sums of op(A) over the reduction -- for wgrad
 * (A = dY^T) that is the bias gradient, so no separate column-sum pass over dY is needed.
 * Dispatch: bf16 A,B with K-contiguous operands (a_sk == b_sk == 1) -> MFMA "NT" kernel;
 *           bf16 A,B with reduction-strided operands (a_sm == b_sn == 1), fp32 C, accumulate -> MFMA "TN" (wgrad)
 *           kernel, split over the reduction: the splits are added into C with fp32 atomics (m3ae_gemm: the order of arrival
 *           decides the rounding), or written as partial tiles to a workspace and folded in ascending split order
 *           (m3ae_gemm_det, deterministic mode); anything else (fp32 operands, odd shapes, batched) -> generic kernel;
 *           fp32 A, B, C with launch_flags & M3AE_GEMM_F32_X3 (and not force_generic) -> fp32x3 kernel, any layout.
 */
typedef struct {
    int64_t M, N, K;
    int64_t batch1, batch2;
    const void* A; int64_t a_sm, a_sk, a_sb1, a_sb2;
    const void* B; int64_t b_sk, b_sn, b_sb1, b_sb2;
    void* C;       int64_t c_sm, c_sn, c_sb1, c_sb2;
    int32_t dtype_a, dtype_b, dtype_c;
    float alpha;
    int32_t accumulate;
    const float* bias;
    int32_t act;
    void* preact;
    const void* residual;
    const void* dact_aux;
    int32_t dact;
    int32_t force_generic; /* tests: bypass the MFMA kernels */
    float* a_rowsum;       /* optional fp32 [M]: a_rowsum[m] += sum_k A[m][k] (bias gradient fused into wgrad) */
    float dropout_p;       /* > 0: x = dropout(x) after bias/activation, BEFORE the residual add (nn.Dropout of */
    uint64_t dropout_seed; /*      bert_model.py:362,440); keep-mask = m3ae counter hash of (seed, m * N + n)     */
    int32_t preact_grad;   /* forward: store act'(pre-activation) in `preact` instead of the pre-activation: the erf / exp
                            * terms are already in registers there, and the backward GEMM (dact = M3AE_ACT_MULAUX) then
                            * multiplies by the saved derivative instead of re-evaluating it (its epilogue was VALU-bound) */
    int32_t launch_flags;  /* M3AE_GEMM_NO_PERSISTENT: never take the persistent (one workgroup per CU, static tile lists)
                            * form of the NT kernel -- for callers that run collectives next to the GEMMs (RCCL kernels
                            * hold CUs; a persistent workgroup that finds none starts after another has walked its list) */
    const void* dropout_salt; /* NULL, or device uint32: folded into the dropout mask key at kernel entry (ABI 3, above) */
} m3ae_gemm_desc;
enum { M3AE_GEMM_NO_PERSISTENT = 1,
       M3AE_GEMM_F32_X3 = 2,  /* fp32x3 mode (ABI 4, additive): fp32 A, B and C run csrc/gemm_f32x3.hip, which splits every operand
                               * element into bf16 hi + lo and forms a_hi b_hi + a_hi b_lo + a_lo b_hi on the bf16 MFMA with fp32
                               * accumulation: |C - C_exact| <= 3 (2^-16 + K 2^-23) (|A||B|)_mn before the epilogue, which is
                               * gemm_generic's.  The whole descriptor contract holds (strides, batches, every epilogue, dropout
                               * masks, a_rowsum over the fp32 A values); m3ae_last_gemm_path() = "f32x3".  force_generic wins;
                               * with bf16 operands or output the call returns M3AE_ERR_UNSUPPORTED. */
       M3AE_GEMM_DETERMINISTIC = 4, /* deterministic mode (ABI 4, additive): no fp32 atomics.  Only m3ae_gemm_det accepts it (it needs a
                               * workspace); m3ae_gemm returns M3AE_ERR_UNSUPPORTED rather than run the atomic kernels. */
       M3AE_GEMM_B_TILED = 8   /* tiled weight operand (ABI 4, additive): B points at the tiled copy of a K-contiguous bf16 weight
                               * W[N][K] (csrc/tiled_b.h; built by m3ae_tile_bf16_batched: N padded to a multiple of 256, times K elements); b_sk
                               * must be 1 and b_sn = K as for the row-major weight.  The NT kernels then stage B from contiguous
                               * 1-KiB pieces; results are bit for bit those of the row-major call.  M3AE_ERR_UNSUPPORTED, before
                               * any launch, for a B that is not bf16, reduction-strided (b_sk != 1) or batched, for K % 32 != 0,
                               * b_sn != K, a B that is not 16-byte aligned, and together with M3AE_GEMM_F32_X3. */ };
/* Diagnostic selectors in launch_flags (0 in the product path = kernel chosen by shape): tests pin the kernel variants
 * per call to compare them bit for bit, tools time them against each other.  The library keeps no tuning state.
 *   NT variant v: 0 = 128x128 tile, 4 = 256x256 2-stage, 7 = 256x256 ping-pong (8, once its persistent form, is unassigned:
 *   like every unassigned value it runs the 128x128 kernel);
 *   TN (wgrad) variant v: 0 / 2 = 128x128 tile with 64- / 32-row steps, 5 = 256x256 ping-pong;
 *   column-tile group width g (1..12) of the ping-pong kernels' tile order;
 *   bits 20-21: cache policy of the NT epilogue's streams (1 plain, 2 output stores nt, 3 + residual / aux loads nt; 0 = by size).
 *   NT variants 9 / 10 (round 4): the second-generation ping-pong kernel, one workgroup per tile / persistent. */
#define M3AE_GEMM_NT_VARIANT(v) ((((v) + 1) & 0xf) << 8)
#define M3AE_GEMM_TN_VARIANT(v) ((((v) + 1) & 0xf) << 12)
#define M3AE_GEMM_COL_GROUP(g) (((g) & 0xf) << 16)
int m3ae_gemm(const m3ae_gemm_desc* d, void* stream);
/* m3ae_gemm with a dropout row map: row m of the call is row row_base + m * row_step of the dropout mask (every other index of
 * the call is unchanged).  A call on rows r0, r0 + s, ... of a larger product (A addressed through a_sm, the outputs compact)
 * then applies the mask the full product applies to those rows.  (0, 1) is m3ae_gemm.  M3AE_ERR_ARG before any launch for
 * row_step < 1, row_base < 0 or a mapped index (row_base + (M - 1) row_step + 1) * ld(N) beyond 2^63 - 1; M3AE_ERR_UNSUPPORTED
 * for a wgrad (TN) descriptor that asks for dropout under a map.  ABI 4, additive. */
int m3ae_gemm_rows(const m3ae_gemm_desc* d, int64_t row_base, int64_t row_step, void* stream);
/* Deterministic mode of the TN (wgrad) family: the same kernels, tiles, split-K fan-out and accumulation order inside a split
 * (M3AE_GEMM_TN_VARIANT pins them as before), but every (tile, split) workgroup stores its fp32 accumulators -- and its partial
 * a_rowsum rows -- to `workspace` with 16-byte stores, and a streaming kernel behind it performs, with one writer per element,
 *     C (+)= alpha * (((p_0 + p_1) + p_2) + ...)        a_rowsum += ((r_0 + r_1) + ...)          in ascending split index.
 * Two calls with the same descriptor contents therefore give the same bits, whatever else runs on the device.
 * m3ae_gemm_det_workspace_bytes: bytes m3ae_gemm_det needs for this descriptor (splits * (M * N + M) fp32); 0 if the descriptor
 *   does not dispatch to the TN family (every other family has one writer per output element: call m3ae_gemm with the flag clear).
 *   Reads shapes, strides, dtypes, flags and the alignment of the pointers that are set; touches no device.
 * m3ae_gemm_det: launch_flags must carry M3AE_GEMM_DETERMINISTIC; M3AE_ERR_UNSUPPORTED for a descriptor whose size query is 0,
 *   M3AE_ERR_WORKSPACE for a missing, misaligned (16 B) or short workspace.  m3ae_last_gemm_path() = "mfma_tn". */
int64_t m3ae_gemm_det_workspace_bytes(const m3ae_gemm_desc* d);
int m3ae_gemm_det(const m3ae_gemm_desc* d, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Scaled-dot-product attention, forward and backward (flash-style in bf16, materialised in fp32).
 * Replaces bert_model.py:301-340 (QK^T / sqrt(dh) + additive mask, softmax, PV) for self- and cross-attention in
 * BertCrossLayer / RobertaLayer, and torch-1.9 F.multi_head_attention_forward's bmm-softmax-bmm in
 * clip_model.py:58; with pos_bias also HF T5Attention (called from m3ae_t5_mm_encoder_input.py:202,244).
 *   q [B, Lq, H*Dh], k / v [B, Lk, H*Dh] with explicit batch and token strides (head h at element offset h*Dh, Dh
 *   contiguous), so packed QKV buffers are addressed in place.  o like q.
 *   key_mask: additive fp32 [B, Lk] (the reference's (1-mask)*-10000.0 extended mask, m3ae_module.py:232) or NULL.
 *             Contract: the values are ADDED to the scaled scores.  They are finite, with one exception: -inf on SOME keys of a
 *             row (those probabilities are exactly 0), never on all keys of a row (the row maximum would be -inf and the row
 *             NaN); +inf and NaN are not allowed.  -10000 on every key of a row is fine: the row maximum is subtracted before
 *             the exponential, and the row comes out as the softmax of its unmasked scores, at the 2^-11 resolution fp32 has
 *             beside 10000.  (Pinned on the fp32 path by tests/test_gpu_parity_accuracy.py, tier B1.)
 *   pos_bias: additive fp32 [H, Lq, Lk] or NULL.  lse: fp32 [B, H, lse_stride] (lse_stride >= Lq, multiple of 32).
 *   Dh must be 64 for the bf16 kernels.  workspace: see m3ae_attn_workspace_bytes (fp32 path only).
 */
typedef struct {
    int64_t B, H, Lq, Lk, Dh;
    const void* q; int64_t q_sb, q_sl;
    const void* k; int64_t k_sb, k_sl;
    const void* v; int64_t v_sb, v_sl;
    void* o;       int64_t o_sb, o_sl;
    const float* key_mask;
    const float* pos_bias;
    float scale;
    int32_t causal;
    float* lse; int64_t lse_stride;
    int32_t dtype;
    void* workspace; int64_t workspace_bytes;
    /* backward only */
    const void* d_o;               /* layout of o */
    void* dq; void* dk; void* dv;  /* layouts of q, k, v */
    float* delta;                  /* fp32 [B, H, lse_stride] scratch: rowsum(dO * O) */
    float* d_pos_bias;             /* fp32 [H, Lq, Lk], accumulated; or NULL */
    /* attention-probability dropout (bert_model.py:334), bf16 kernels only: P is dropped (and rescaled by 1/(1-p))
     * after the softmax normaliser is taken; mask = counter hash of (seed, ((b*H+h)*Lq+q)*Lk+k), regenerated in bwd */
    float dropout_p;
    uint64_t dropout_seed;
    const void* dropout_salt; /* as m3ae_gemm_desc.dropout_salt */
    int32_t launch_flags;     /* M3AE_ATTN_LEGACY_KERNELS: the round-3 bf16 kernels (tests compare the two generations); ABI 3 */
} m3ae_attn_desc;
enum { M3AE_ATTN_LEGACY_KERNELS = 1,
       M3AE_ATTN_F32_X3 = 2   /* fp32 path: every product inside m3ae_attn_fwd (scores, P V), m3ae_attn_bwd (dP, dV, dQ, dK) and
                               * m3ae_attn_probs (the scores recompute) takes the fp32x3 GEMM (M3AE_GEMM_F32_X3); the softmax,
                               * softmax backward, dropout and pos-bias gradient kernels are unchanged.  Ignored by the bf16
                               * kernels.  ABI 4, additive. */ };
int64_t m3ae_attn_workspace_bytes(const m3ae_attn_desc* d, int backward);
int m3ae_attn_fwd(const m3ae_attn_desc* d, void* stream);
int m3ae_attn_bwd(const m3ae_attn_desc* d, void* stream);
/* The same with a row map of the probability-dropout mask: mask row row_base + ((b*H + h)*Lq + q) * row_step.  A call on query 0
 * alone (Lq = 1, q_sb = the batch stride of the full tensor) with row_step = Lq_full draws the masks query 0 has in the call on
 * all Lq_full queries.  Argument checks as m3ae_gemm_rows (rows = B*H*Lq, cols = Lk).  ABI 4, additive. */
int m3ae_attn_fwd_rows(const m3ae_attn_desc* d, int64_t row_base, int64_t row_step, void* stream);
int m3ae_attn_bwd_rows(const m3ae_attn_desc* d, int64_t row_base, int64_t row_step, void* stream);
/* The attention probabilities of the m3ae_attn_fwd call made with the same descriptor (the visualisation maps of
 * bert_model.py:346): probs[b * p_sb + h * p_sh + q * p_sq + k] (fp32, strides in elements, p_sq >= Lk) for q < Lq, k < Lk,
 *   = softmax_k(q.k / sqrt(dh) + key_mask[b][k])                    with dropout_p == 0,
 *   = the same times the forward's keep mask / (1 - dropout_p)      with dropout_p > 0 (the drop(P) that multiplied V: the
 *     same seed, salt and mask index ((b*H + h)*Lq + q) * ld(Lk) + k).
 * Padding keys (additive -10000 mask) come out as 0 (exp underflow); padding query rows are computed like any other.
 * bf16: read q, k, key_mask and the `lse` table the forward wrote (v, o, workspace unused), Dh = 64.  fp32: the forward's
 * scores GEMM, row softmax and dropout run again with `probs` as their buffer, which must then be dense (p_sq = Lk,
 * p_sh = Lq*Lk, p_sb = H*Lq*Lk).
 * No pos_bias, no causal mask (M3AE_ERR_UNSUPPORTED).  ABI 4. */
int m3ae_attn_probs(const m3ae_attn_desc* d, float* probs, int64_t p_sb, int64_t p_sh, int64_t p_sq, void* stream);
/* The received attention of the same call: the mean of the map m3ae_attn_probs defines over heads and queries,
 *   out[b * out_sb + k] = 1 / (H Lq) * sum_h sum_q probs[b][h][q][k]      (fp32, k < Lk, out_sb >= Lk),
 * over all Lq query rows, without the map ever reaching memory.  Descriptor contract, dtype dispatch and refusals as
 * m3ae_attn_probs (q, k, lse, key mask, dropout fields; the identity row map; pos_bias / causal: M3AE_ERR_UNSUPPORTED).
 * bf16 (Dh = 64): every entry is formed by the expression of m3ae_attn_probs, so each summed entry has the bits that call writes; a
 *   workgroup sums its 128 query rows on chip and writes one partial row per (b, h, query block) to the workspace, and a second
 *   kernel adds the partial rows in ascending (h, query block) order and multiplies by the rounded 1 / (H Lq).  No atomics: the
 *   result is a function of the inputs alone.  Workspace: B * H * ceil(Lq / 128) * Lk floats.
 * fp32 (and M3AE_ATTN_F32_X3): the scores GEMM, row softmax and dropout of m3ae_attn_probs run over M3AE_ATTN_COLMEAN_F32_CHUNK
 *   samples at a time into the workspace, whose columns the same fold adds (queries, then heads).  Workspace:
 *   min(B, chunk) * H * (Lq + 1) * Lk floats -- a function of the chunk, not of B.
 * The workspace is caller-owned and 16-byte aligned; missing, misaligned or shorter than m3ae_attn_colmean_workspace_bytes(d):
 * M3AE_ERR_WORKSPACE before any launch.  ABI 4, additive. */
#define M3AE_ATTN_COLMEAN_F32_CHUNK 4
int64_t m3ae_attn_colmean_workspace_bytes(const m3ae_attn_desc* d);
int m3ae_attn_colmean(const m3ae_attn_desc* d, float* out, int64_t out_sb, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused cross-attention sub-block of BertCrossLayer (north_star's kernel), bf16: BertAttention as `crossattention`
 * (bert_model.py:480-488) = BertSelfAttention.forward cross branch (:253-350, :275-278) + BertSelfOutput (:353-364):
 *     out = LayerNorm(x + dropout(dense(softmax(QK^T / sqrt(dh) + mask) V)))     Q from x, K / V from y.
 * The projection of the LONG side (the 577 image tokens) is absorbed into the short side (32 text tokens); see
 * csrc/xattn.hip.  dir 0: text queries over image keys (Lq = 32); dir 1: image queries over text keys (Lk = 32).
 * Results equal the unfused composition (m3ae_gemm + m3ae_attn_fwd + m3ae_gemm + m3ae_layernorm_fwd) up to bf16
 * rounding of the intermediates; the dropout masks are THE SAME masks (same seeds, same index convention), so the
 * two can be compared under dropout.  All buffers are caller-owned; the intermediates are what the backward reads.
 *   weights (bf16): wq [D, D], wq_t = wq^T, wkv [2D, D] (key rows, then value rows), wkv_t = wkv^T [D, 2D], wo [D, D],
 *                   wo_t = wo^T; biases and LayerNorm parameters fp32.
 *   key_mask: additive fp32 [B, Lk] or NULL.
 *   proj:  dir 0: q [B*Lq, D];          dir 1: k | v [B*Lk, 2D]
 *   prime: dir 0: Q' [B, Lq*H, D];      dir 1: K' then V', each [B, H*Lk, D]
 *   colbias (dir 1): fp32 [B, H*Lk].    probs / probs_drop: dir 0 [B, Lq*H, 640]; dir 1 [B, Lq, H*Lk]
 *   (probs_drop, rowsum [B, Lq*H] fp32 (dir 0): only with dropout_p > 0).   zctx (dir 0): [B, Lq*H, D]; ctx (dir 0): [B*Lq, D]
 *   s: pre-LayerNorm sum [B*Lq, D]; out [B*Lq, D]; mean / rstd fp32 [B*Lq].
 */
typedef struct {
    int32_t dir;
    int64_t B, Lq, Lk, D, H;
    const void* x;
    const void* y;
    const float* key_mask;
    const void *wq, *wq_t, *wkv, *wkv_t, *wo, *wo_t;
    const float *bq, *bkv, *bo, *ln_g, *ln_b;
    float ln_eps;
    float dropout_p;
    uint64_t seed_attn, seed_hidden;
    void* proj;
    void* prime;
    float* colbias;
    void* probs;
    void* probs_drop;
    float* rowsum;
    void* zctx;
    void* ctx;
    void* s;
    void* out;
    float *mean, *rstd;
    /* ---- backward only (m3ae_xattn_bwd): the forward's fields above hold what the forward wrote ---- */
    const void* d_out;            /* [B*Lq, D] gradient of `out` */
    void* dx;                     /* [B*Lq, D] gradient of x (residual branch included) */
    void* dy;                     /* [B*Lk, D] gradient of y */
    /* parameter gradients, fp32, ACCUMULATED: weights [D, D] / [2D, D] like the parameters, biases [D] / [2D] */
    float *g_wq, *g_wkv, *g_wo, *g_bq, *g_bkv, *g_bo, *g_ln_g, *g_ln_b;
    /* caller-owned scratch */
    void* ws_ds;                  /* [B*Lq, D]                       gradient of s */
    void* ws_dsd;                 /* [B*Lq, D]   (dropout_p > 0)     gradient of the dense output before the hidden dropout */
    void* ws_dscores;             /* like `probs`                    gradient of the scores */
    void* ws_dprime;              /* like `prime`                    gradient of Q' (dir 0) / K', V' (dir 1) */
    void* ws_dproj;               /* like `proj`                     gradient of q (dir 0) / k | v (dir 1) */
    void* ws_dz;                  /* dir 0: [B, Lq*H, D]             gradient of zctx */
    void* ws_dctx;                /* dir 0: [B*Lq, D]                gradient of ctx */
    float* ws_vec;                /* fp32 [3 * B * H * T], T = min(Lq, Lk) text tokens */
    float* ws_ln;                 /* fp32 [2 * m3ae_layernorm_bwd_blocks(B*Lq) * D] */
    int32_t launch_flags;         /* M3AE_XATTN_*: per-call launch policy (the library keeps no state) */
    const void* dropout_salt;     /* as m3ae_gemm_desc.dropout_salt: both dropout sites of the sub-block */
} m3ae_xattn_desc;
enum { M3AE_XATTN_NO_PERSISTENT = 1,  /* the internal m3ae_gemm calls never take the persistent NT kernel (callers that run
                                       * collectives next to the step: see m3ae_gemm_desc.launch_flags) */
       M3AE_XATTN_LEGACY_CHAIN = 2    /* dir 1 forward: the round-2 chain (score GEMM + softmax epilogue, P through HBM, P V'
                                       * GEMM) instead of the one-launch kernel of csrc/xflash.hip -- A/B measurements only */ };
/* dir 1 (image queries): Lk = 32 or 64 text keys, any Lq; probs / probs_drop may be NULL in a forward-only call (the scores and
 * probabilities then never leave the chip).  dir 0 (text queries): Lq = 32 or 64, Lk <= 640.  Both: head width D / H a multiple of 32
 * up to 256, D <= 4096 (the backward: D <= 2048, the LayerNorm backward's widest row); DESIGN.md 2c tabulates the envelope.  The
 * backward never touches the key-bias half of g_bkv: that gradient is exactly zero. */
int m3ae_xattn_supported(const m3ae_xattn_desc* d);   /* 1 if the fused forward covers these shapes */
int m3ae_xattn_bwd_supported(const m3ae_xattn_desc* d);   /* 1 if m3ae_xattn_bwd does too */
int64_t m3ae_xattn_probs_ld(const m3ae_xattn_desc* d);
int m3ae_xattn_fwd(const m3ae_xattn_desc* d, void* stream);
/* Backward of m3ae_xattn_fwd in the same absorbed form: two more per-sample products per direction (the gradient of the
 * scores with the softmax backward in its epilogue, the gradients of the absorbed operands), the other stream's gradient,
 * and the per-head weight gradients as split-K fp32 atomics.  d(b_k) is exactly zero (b_k drops out of the softmax) and is
 * not touched.  Dropout masks are regenerated from the forward's seeds. */
int m3ae_xattn_bwd(const m3ae_xattn_desc* d, void* stream);
/* The attention probabilities a m3ae_xattn_fwd call wrote (dir 0 always; dir 1 when `probs` was passed), as fp32
 * out[b * o_sb + h * o_sh + q * o_sq + k] for q < Lq, k < Lk: `probs` (dropped == 0) or `probs_drop` (dropped != 0, the dropped
 * and rescaled P of a call with dropout_p > 0), with dir 0's key padding (640 columns) sliced off.  Reads d->dir, B, Lq, Lk, H and
 * the chosen buffer only.  ABI 4. */
int m3ae_xattn_probs_export(const m3ae_xattn_desc* d, int dropped, float* out, int64_t o_sb, int64_t o_sh, int64_t o_sq,
                            void* stream);
/* The received attention of the same buffer: out[b * out_sb + k] = 1 / (H Lq) * sum_h sum_q P[b][h][q][k] for k < Lk (fp32,
 * out_sb >= Lk), P as m3ae_xattn_probs_export reads it (layout, padding columns, leading dimension m3ae_xattn_probs_ld); the stored
 * bf16 values widen exactly.  One streaming pass with 16-byte loads; every output element has one owner (no atomics, fixed
 * order).  Reads d->dir, B, Lq, Lk, H and the chosen buffer only.  M3AE_ERR_ALIGN for a buffer off 16 bytes; M3AE_ERR_UNSUPPORTED for
 * dir 0 with Lk > 640, dir 1 with Lk % 8 != 0, B > 65535.  ABI 4, additive. */
int m3ae_xattn_probs_colmean(const m3ae_xattn_desc* d, int dropped, float* out, int64_t out_sb, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Bilinear upsample of a patch grid (csrc/heatmap.hip): in [B][g][g] fp32 (sample stride in_sb elements, rows dense) ->
 * out [B][S][S] fp32, dense, torch.nn.functional.interpolate(mode="bilinear", align_corners=False) semantics.  `in` may point at
 * token 1 of a [B][1 + g*g] row of received attention with in_sb = 1 + g*g: the class token is skipped without a copy.
 * Per axis and destination index d, in fp32 with no contraction:
 *   scale = (float)g / (float)S;  src = max(scale * ((float)d + 0.5f) - 0.5f, 0);  i0 = min((int)src, g - 1);
 *   i1 = min(i0 + 1, g - 1);  l1 = src - (float)i0;  l0 = 1 - l1;
 * and out = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d) with a, b = in[i0y][i0x], in[i0y][i1x]; c, d the same of row
 * i1y: rows first, then columns, every product and sum rounded once.
 * M3AE_ERR_ARG for a null pointer, B < 1, g < 1, S < 1 or in_sb < g*g; M3AE_ERR_UNSUPPORTED for B > 65535, g or S > 16384.
 * ABI 4, additive. */
int m3ae_heatmap_upsample(const float* in, int64_t in_sb, int64_t g, float* out, int64_t B, int64_t S, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * LayerNorm (biased variance, eps inside the sqrt, fp32 statistics), optional fused activation on the output.
 * Replaces nn.LayerNorm at bert_model.py:357,363,435,441 (eps 1e-12 / 1e-5), clip_model.py:27-33 (fp32 upcast),
 * m3ae_module.py:122 (+ nn.GELU :123 via `act`).  mean / rstd: fp32 [M] saved for backward.
 * bwd: dx = LN'(dy) (+ dx_add: the residual branch's gradient of a pre-LN block, fused); dgamma / dbeta are
 * ACCUMULATED (+=) in fp32 (dgamma may be NULL for frozen parameters).  workspace: fp32 [2 * nblk * D] with
 * nblk = m3ae_layernorm_bwd_blocks(M).  rms != 0 selects T5 RMSNorm (no mean subtraction, no beta).
 *
 * The family: m3ae_layernorm_fwd / _bwd; _bwd_drop and _bwd_drop_rows (a second output under a dropout mask); _fwd_mixed / _bwd_mixed
 * (fp32 rows next to bf16 rows); and, declared with the deterministic mode below, _bwd_det / _bwd_drop_det / _bwd_mixed_det (the
 * same calls with the dgamma / dbeta fold in a fixed order).  Every one of them checks in this order, before any launch:
 *   1. M3AE_ERR_ARG: a required pointer is NULL, M <= 0 (the forwards: D <= 0), or a bad row map.  Required: x, gamma, y of a
 *      forward; dy, x, gamma, rstd, dx, workspace of a backward, plus dx_drop of the dropout forms and mean of the mixed forms.
 *   2. M3AE_ERR_UNSUPPORTED: D % 4 != 0, D > 4096 (m3ae_layernorm_fwd) or D > 2048 (every other call), an unknown dtype.
 *   3. M3AE_ERR_ALIGN: every array is aligned to 4 of its own elements -- fp32 rows, gamma and beta to 16 bytes, bf16 rows to 8 bytes
 *      (a NULL optional array counts as aligned).
 */
int m3ae_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                       int64_t M, int64_t D, float eps, int dtype, int act, int rms, void* stream);
int64_t m3ae_layernorm_bwd_blocks(int64_t M);
int m3ae_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean,
                       const float* rstd, void* dx, const void* dx_add, float* dgamma, float* dbeta, float* workspace,
                       int64_t M, int64_t D, int dtype, int act, int rms, void* stream);
/* same, plus a second output dx_drop = dropout_mask(seed, p) * LN'(dy) / (1 - p): the gradient entering the dense layer
 * whose output was dropped before the residual add (post-LN BERT blocks), produced without an extra pass over dx. */
int m3ae_layernorm_bwd_drop(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean,
                            const float* rstd, void* dx, void* dx_drop, float dropout_p, uint64_t dropout_seed,
                            const void* dropout_salt, float* dgamma, float* dbeta, float* workspace, int64_t M, int64_t D,
                            int dtype, void* stream);
/* the same on rows row_base + m * row_step of the mask (m3ae_gemm_rows); ABI 4, additive */
int m3ae_layernorm_bwd_drop_rows(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean,
                                 const float* rstd, void* dx, void* dx_drop, float dropout_p, uint64_t dropout_seed,
                                 const void* dropout_salt, float* dgamma, float* dbeta, float* workspace, int64_t M, int64_t D,
                                 int dtype, int64_t row_base, int64_t row_step, void* stream);
/* fp32 residual stream of a bf16 model (ABI 4, additive): the LayerNorm between fp32 rows and bf16 GEMM operands, plain LayerNorm
 * only (no activation, no RMS mode); x / dx / dx_add are the fp32 rows, y / dy / dx_lo the bf16 rows of the checks above.
 * fwd_mixed: x fp32 [M][D] -> y bf16 [M][D] = rne_bf16 of what m3ae_layernorm_fwd (M3AE_F32) writes for x, from the same fp32
 *   arithmetic in the same order; mean / rstd are that call's, bit for bit.
 * bwd_mixed: dy bf16 (what a dgrad GEMM wrote), x fp32 (the saved stream), dx_add fp32 (the stream's gradient, may be NULL) ->
 *   dx fp32 = what m3ae_layernorm_bwd (M3AE_F32) writes for the widened dy, and, when dx_lo is not NULL, dx_lo bf16 =
 *   rne_bf16(dx) in the same pass (the operand of the GEMMs below).  dgamma / dbeta / workspace as for m3ae_layernorm_bwd;
 *   _det folds them in the fixed order of m3ae_layernorm_bwd_det. */
int m3ae_layernorm_fwd_mixed(const float* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                             int64_t M, int64_t D, float eps, void* stream);
int m3ae_layernorm_bwd_mixed(const void* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                             float* dx, const float* dx_add, void* dx_lo, float* dgamma, float* dbeta, float* workspace,
                             int64_t M, int64_t D, void* stream);
int m3ae_layernorm_bwd_mixed_det(const void* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                                 float* dx, const float* dx_add, void* dx_lo, float* dgamma, float* dbeta, float* workspace,
                                 int64_t M, int64_t D, void* stream);
/* out = dropout(x) on a dense [rows][cols] array with the library's counter-hash mask (forward and backward are
 * the same map).  Every dropout site of the library -- this call, the GEMM epilogue (rows = M, cols = N), the
 * LayerNorm backward second output, and attention probabilities (rows = (b*H + h)*Lq + q, cols = Lk) -- uses the mask
 * index row * ld + col with ld = cols rounded up to a multiple of 4, so a mask exported here (keep_mask, uint8
 * [rows][cols], optional) is the mask those kernels apply for the same (p, seed). */
int m3ae_dropout(const void* x, void* out, uint8_t* keep_mask, int64_t rows, int64_t cols, float p, uint64_t seed,
                 const void* salt, int dtype, void* stream);
/* Row map (ABI 4, additive): the *_rows entry points take (row_base, row_step) and use mask row row_base + row * row_step in that
 * index, so a call on every row_step-th row of a site draws the masks of the call on all rows; (0, 1) is the plain entry point.
 * Checked on the host before any launch: row_step >= 1, row_base >= 0, last mapped index < 2^63 (else M3AE_ERR_ARG). */
int m3ae_dropout_rows(const void* x, void* out, uint8_t* keep_mask, int64_t rows, int64_t cols, float p, uint64_t seed,
                      const void* salt, int dtype, int64_t row_base, int64_t row_step, void* stream);

/* out[n] (+)= sum_m x[m][n]  (bias gradients; x has row stride ldx elements). */
int m3ae_colsum(const void* x, float* out, int64_t M, int64_t N, int64_t ldx, int dtype, int accumulate,
                void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * RoBERTa embeddings (HF RobertaEmbeddings called at m3ae_module.py:230): position ids =
 * cumsum(ids != pad) * (ids != pad) + pad; out = word[ids] + type[0] + pos[position id]  (LayerNorm is a separate
 * call).  Tables are the fp32 master parameters.  bwd scatter-adds d_out into the fp32 table gradients.
 */
int m3ae_roberta_embed_fwd(const int64_t* ids, const float* word, const float* pos, const float* type, void* out,
                           int64_t B, int64_t S, int64_t D, int64_t pad_id, int dtype, void* stream);
int m3ae_roberta_embed_bwd(const int64_t* ids, const void* d_out, float* d_word, float* d_pos, float* d_type,
                           int64_t B, int64_t S, int64_t D, int64_t pad_id, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * ViT token assembly (clip_model.py:94-99): im2col of non-overlapping patches (column order c, ph, pw = the
 * row-major flattening of conv1.weight[width, 3, P, P]) and [cls | patches] + positional_embedding.
 * Pointers need the alignment of their element type only.  m3ae_patchify (bf16 output, P % 8 == 0) and m3ae_vit_tokens_fwd
 * (bf16, D % 8 == 0) move 16 bytes per lane when every pointer they would access that way -- img and out; patch, cls, pos and
 * out -- is 16-byte aligned, and take the element-wise kernel otherwise: same bits either way.
 */
int m3ae_patchify(const float* img, void* out, int64_t B, int64_t R, int64_t P, int dtype, void* stream);
/* Input pipeline tail (transforms/transform.py:60-67 ToTensor + Normalize, after the host-side PIL resize / centre crop):
 * uint8 [B, H, W, 3] (RGB, as uploaded from pinned host memory: a quarter of the fp32 PCIe bytes) ->
 * fp32 [B, 3, H, W] with out = (u / 255 - mean[c]) / std[c], the same two IEEE divisions torch performs. */
int m3ae_image_normalize_u8(const uint8_t* in, float* out, int64_t B, int64_t H, int64_t W, const float* mean3,
                            const float* std3, void* stream);
/* Device image transform (csrc/image.hip): transforms/transform.py:60-67 whole -- Resize(size, BICUBIC) on the 8-bit image,
 * CenterCrop(size), ToTensor, Normalize -- for a batch of B decoded, OPAQUE sources of any sizes, in two launches.  The resize is
 * Pillow's fixed-point arithmetic (libImaging/Resample.c, 8 bits per channel): per pass and channel
 *     out = clamp((2^21 + sum_t pixel[xmin + t] * k[t]) >> 22, 0, 255)      (int32, arithmetic shift),
 * horizontal pass first into a uint8 intermediate (its rounding is part of the result), then the vertical pass; the bounds
 * (xmin, taps) and the 22-bit coefficients k of every output column / row come from the caller (m3ae_amd/resample.py builds them
 * in float64 in Pillow's operation order; |k| < 2^23), with the centre crop folded in: `size` outputs per axis.  The result is
 * the bytes PIL produces, and `out` is bit-equal to m3ae_image_normalize_u8 of them.
 *   src   bytes of the B sources, RGB interleaved, each starting at a 16-byte aligned offset
 *   plan  int64 [B][16] per image: 0 byte offset in src, 1 w, 2 h, 3 row pitch in bytes, 4 row0, 5 nrows (the source rows the
 *         surviving output rows read: the horizontal pass runs on these alone), 6 ksize_x, 7 ksize_y (row lengths of the two
 *         coefficient tables), 8..11 offsets (in int32) into tab of: x bounds [size][2], x coefficients [size][ksize_x], y bounds
 *         [size][2] (absolute source rows), y coefficients [size][ksize_y], 12 first intermediate row of this image (running sum
 *         of nrows), 13 read by m3ae_image_resample_tables alone, 14..15 zero.  w <= 8192.
 *   tab   int32 tables as addressed by plan
 *   workspace  uint8 intermediates [sum nrows][size * 3 rounded up to 4]; m3ae_image_resample_workspace_bytes(sum nrows, size)
 *   out   fp32 [B][3][size][size] = (u / 255 - mean[c]) / std[c];  out_u8: NULL, or uint8 [B][size][size][3] (the crop itself)
 *   mean3 / std3: HOST arrays, as for m3ae_image_normalize_u8.
 * src_bytes / tab_ints / workspace_bytes are the sizes of src (bytes), tab (int32) and workspace (bytes): the kernels check every
 * plan record and table bound against them and leave an image whose record points outside unwritten. */
int64_t m3ae_image_resample_workspace_bytes(int64_t total_rows, int64_t size);
int m3ae_image_resample_u8(const uint8_t* src, int64_t src_bytes, const int64_t* plan, const int32_t* tab, int64_t tab_ints, int64_t B,
                           int64_t size, uint8_t* workspace, int64_t workspace_bytes, float* out, uint8_t* out_u8,
                           const float* mean3, const float* std3, void* stream);
/* Coefficient tables of m3ae_image_resample_u8 built on the device (csrc/image.hip), for plans whose every image has a resample of
 * its own: transforms/transform.py:70-77, RandomResizedCrop(size, scale=(0.9, 1.0), BICUBIC) -- image b is the box (plan w x h at
 * plan offset, the full image's pitch) resized to size x size, row0 = 0, nrows = h.  For every plan record with field 13 != 0 the
 * kernel writes the four tables at the record's offsets 8..11: bounds [size][2] and coefficients [size][ksize] (zero-filled past
 * the taps) of the resamples w -> size and h -> size, outputs 0 .. size - 1, in float64 in Pillow's operation order without
 * contraction: bit-equal to m3ae_amd/resample.py's axis_table.  Records that share tables mark one owner.  A record whose
 * extents do not lie inside tab, or whose ksize_x / ksize_y is smaller than Pillow's ksize of its axis, is left unwritten whole.
 * Call it in front of m3ae_image_resample_u8 on the same stream.  Returns as m3ae_image_resample_u8: M3AE_ERR_ARG for a null
 * pointer or a non-positive B / size / tab_ints, M3AE_ERR_UNSUPPORTED for B > 65535 or size > 4096. */
int m3ae_image_resample_tables(const int64_t* plan, int64_t B, int64_t size, int32_t* tab, int64_t tab_ints, void* stream);
/* RandAugment(2, 9) on the source bytes of a device image transform batch (csrc/randaug.hip; transforms/randaug.py:164-272 of the
 * reference in front of the CLIP transform, transforms/transform.py:80-91): two operations per image out of 14, Pillow's
 * arithmetic restated so that the bytes are Pillow's (m3ae_amd/randaug.py holds the numpy model).  Call it in front of
 * m3ae_image_resample_tables / m3ae_image_resample_u8 on the same stream.
 *   src      the pack's source bytes (every image RGB interleaved, rows packed, at a 16-byte aligned offset); augmented in place
 *   scratch  a second buffer of buf_bytes bytes: stage 0 reads src and writes scratch, stage 1 reads scratch and writes src
 *   plan     int64 [B][24] per image: 0 byte offset, 1 w (<= 8192), 2 h (<= 16384), 3 zero, then per stage s at 4 + 10 s:
 *            operation (0 identity, 1 AutoContrast, 2 Equalize, 3 Rotate, 4 Posterize, 5 Solarize, 6 SolarizeAdd, 7 Color,
 *            8 Contrast, 9 Brightness, 10 Sharpness, 11 ShearX, 12 ShearY, 13 TranslateXabs, 14 TranslateYabs), the sign of a geometric
 *            operation's value (+1 / -1), a0 .. a5 = the 16.16 fixed-point coefficients of Pillow's affine_fixed for a geometric
 *            operation (source pixel of output (x, y) = ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16); |a| < 2^40), two zeros.
 *            A record with both operations 0 is passed over; a record that does not lie inside buf_bytes, or names an unknown
 *            operation, is left unwritten whole.
 *   workspace  m3ae_image_randaug_workspace_bytes(B) bytes, 4-byte aligned: uint32 histograms [2][B][4][256] (R, G, B, L of the
 *            input of each stage, for the images whose operation reads one), then the uint8 tables [B][3][256] of the point operations
 *   flags    bit s: stage s has an operation that reads a histogram (1, 2, 8); bit 2 + s: stage s has a point operation
 *            (1, 2, 4, 5, 6, 8, 9).  A stage whose bit is clear skips that launch.
 * Returns M3AE_ERR_ARG (null pointer, src == scratch, non-positive B / buf_bytes, unknown flag bits), M3AE_ERR_UNSUPPORTED
 * (B > 65535), M3AE_ERR_ALIGN, M3AE_ERR_WORKSPACE. */
int64_t m3ae_image_randaug_workspace_bytes(int64_t B);
int m3ae_image_randaug_u8(uint8_t* src, uint8_t* scratch, int64_t buf_bytes, const int64_t* plan, int64_t B, void* workspace,
                          int64_t workspace_bytes, int flags, void* stream);
int m3ae_vit_tokens_fwd(const void* patch, const float* cls, const float* pos, void* out, int64_t B, int64_t G,
                        int64_t D, int dtype, void* stream);
int m3ae_vit_tokens_bwd(const void* d_out, void* d_patch, float* d_cls, float* d_pos, int64_t B, int64_t G,
                        int64_t D, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Losses.  bce: objectives.py:201  loss = mean(BCEWithLogits(x, z)) * C.  Writes loss[0] (fp32, overwritten) and
 * d_logits = d(loss)/dx * grad_scale.  xent: F.cross_entropy(ignore_index=-100, mean) (objectives.py:19-23,101).
 */
int m3ae_bce_logits(const void* logits, const float* targets, float* loss, void* d_logits, int64_t B, int64_t C,
                    float grad_scale, int dtype, void* stream);
int m3ae_xent(const void* logits, const int64_t* labels, float* loss, void* d_logits, float* workspace,
              int64_t rows, int64_t C, int64_t ld, float grad_scale, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * AdamW as transformers==4.6.0 implements it (m3ae_utils.py:206): bias-corrected Adam update, then decoupled
 * decay p -= lr * wd * p.  One call per contiguous fp32 segment (a parameter group of the flat buffer).
 * g is multiplied by grad_scale first (1 / world_size for DDP averaging).  If shadow != NULL also writes the bf16
 * copy used by the forward pass.
 */
int m3ae_adamw(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, float beta1,
               float beta2, float eps, float wd, int64_t step, float grad_scale, const float* hyper_dev, void* stream);
/* hyper_dev (ABI 3): NULL, or a device pointer to {lr, lr * sqrt(1 - beta2^step) / (1 - beta1^step)} of THIS step: the kernel then
 * takes both from there instead of from `lr` / `step` (a hipGraph-captured step replays with frozen arguments; the caller
 * uploads the two floats per group before every replay). */

/* ------------------------------------------------------------------------------------------------------------
 * Gradient clipping by global norm with a non-finite step guard (ABI 4, additive; csrc/gradnorm.hip).  No atomics, no host
 * round trip: sums of squares in double -> one-workgroup finalize -> m3ae_adamw_clip reads the factor from device memory.
 *
 * m3ae_sumsq_segments: out[s] = sum of x[i]^2 over segment s, as double, accumulated in double from the first add (the square
 *   of an fp32 value is exact in double, only the adds round: |out - exact| <= (len - 1) * 2^-53 * exact in any order; no finite
 *   input overflows or underflows).  The segments [begin, end) of x[n] -- sorted, non-overlapping, any alignment, empty ones and
 *   gaps allowed -- are given cut into pieces by the caller:
 *     pieces_dev  [npieces][2] int64 {begin, end} in elements, every piece inside one segment, a segment's pieces adjacent and
 *                 ascending (the binding cuts at most 32768 elements per piece; any length works);
 *     seg_ptr_dev [nseg + 1] int64, CSR: segment s owns pieces seg_ptr[s] .. seg_ptr[s + 1] - 1 (none: out[s] = 0).
 *   One workgroup per piece writes one double to `workspace` (fixed lane positions, fixed tree); one wave per segment then adds
 *   that segment's pieces in ascending order.  The result is a function of (x, tables) alone: two calls give the same bits, and
 *   deterministic mode takes this same entry point.  Elements outside every piece are never read; piece bounds are clamped to
 *   [0, n].  x 16-byte aligned.  m3ae_sumsq_workspace_bytes(npieces): bytes of `workspace` (touches no device).
 * m3ae_clip_finalize (one workgroup): total = seg_sumsq[0] + ... + seg_sumsq[nseg - 1] in ascending index, in double, then the
 *   record (M3AE_CLIP_RECORD_WORDS 32-bit words on the device, zeroed once by the caller; indices below):
 *     norm (float)  = sqrt(total) * |grad_scale|                          -- the norm of the averaged gradient under DDP
 *     coef (float)  = min(1, max_norm / (norm + 1e-6)), formed in double  -- torch.nn.utils.clip_grad_norm_'s rule; exactly 1.0f
 *                     whenever the norm is inside the bound; max_norm = +inf: guard only
 *     skip (uint32) = 1 and coef = 0 when total is inf or nan, else 0
 *     steps / clipped_steps / skipped_steps (uint32): running counters, incremented by this call.
 *   max_norm in (0, +inf], grad_scale finite, else M3AE_ERR_ARG.
 * m3ae_adamw_clip: m3ae_adamw with `clip_dev`, the record: skip != 0 -> returns before touching p, m, v or the shadow; otherwise
 *   grad_scale * coef, formed once in fp32, takes the place of grad_scale (coef == 1.0f: the bits of m3ae_adamw).
 */
enum { M3AE_CLIP_NORM = 0, M3AE_CLIP_COEF = 1, M3AE_CLIP_SKIP = 2, M3AE_CLIP_STEPS = 4, M3AE_CLIP_CLIPPED_STEPS = 5,
       M3AE_CLIP_SKIPPED_STEPS = 6, M3AE_CLIP_RECORD_WORDS = 8 };
int64_t m3ae_sumsq_workspace_bytes(int64_t npieces);
int m3ae_sumsq_segments(const float* x, int64_t n, const int64_t* pieces_dev, int64_t npieces, const int64_t* seg_ptr_dev,
                        int64_t nseg, double* out, void* workspace, int64_t workspace_bytes, void* stream);
int m3ae_clip_finalize(const double* seg_sumsq, int64_t nseg, float grad_scale, float max_norm, float* record, void* stream);
int m3ae_adamw_clip(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, float beta1,
                    float beta2, float eps, float wd, int64_t step, float grad_scale, const float* hyper_dev,
                    const float* clip_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The other two rules of the reference's `optim_type` (m3ae_utils.py:203-210), ABI 4, additive (csrc/misc.hip).  Same contract as
 * m3ae_adamw: one call per contiguous fp32 segment, n % 4 == 0, fp32 pointers 16-byte aligned, g multiplied by grad_scale first,
 * the bf16 shadow written in the same pass when given; fp32 arithmetic, one operation per line below.  Neither takes hyper_dev
 * (a hipGraph-captured step is offered for AdamW only).
 *
 * m3ae_adam: single-tensor torch.optim.Adam, no amsgrad, coupled L2 decay; step >= 1:
 *     g' = g * grad_scale;  if (wd > 0) g' = g' + wd * p
 *     m  = m * beta1 + g' * (1 - beta1)
 *     v  = v * beta2 + g' * g' * (1 - beta2)
 *     denom = sqrtf(v) / bc2_sqrt + eps
 *     p  = p - step_size * (m / denom)
 *   with step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step), (1 - beta1) and (1 - beta2) each formed in double on
 *   the host and rounded to fp32 once (the bias correction of v sits inside the denominator, not in the step size as in
 *   m3ae_adamw).  beta1 / beta2 are doubles, as torch holds them: at torch's default 0.999 the fp32 value is 1.3e-8 off, but its
 *   complement 1.0f - 0.999f is 1.3e-5 off 0.001, which v would carry whole (m3ae_adamw's 0.98 is four times closer to its fp32
 *   value and its complement forty times larger).
 * m3ae_sgd: torch.optim.SGD with momentum, dampening 0, no Nesterov:
 *     g'  = g * grad_scale;  if (wd > 0) g' = g' + wd * p
 *     buf = buf * momentum + g'
 *     p   = p - lr * buf
 *   torch's first step sets buf = g'; a zero-initialised buf gives the same bits, so there is no step argument.
 * The _clip forms take the record of m3ae_clip_finalize exactly as m3ae_adamw_clip does: skip != 0 -> returns before touching
 *   anything; otherwise grad_scale * coef, formed once in fp32, takes the place of grad_scale (coef == 1.0f: the plain form's bits).
 */
int m3ae_adam(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, double beta1, double beta2,
              float eps, float wd, int64_t step, float grad_scale, void* stream);
int m3ae_adam_clip(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, float lr, double beta1,
                   double beta2, float eps, float wd, int64_t step, float grad_scale, const float* clip_dev, void* stream);
int m3ae_sgd(float* p, const float* g, float* buf, void* shadow_bf16, int64_t n, float lr, float momentum, float wd,
             float grad_scale, void* stream);
int m3ae_sgd_clip(float* p, const float* g, float* buf, void* shadow_bf16, int64_t n, float lr, float momentum, float wd,
                  float grad_scale, const float* clip_dev, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Exponential moving average of the weights (ABI 4, additive; csrc/misc.hip).  Same contract as m3ae_adamw: one call per contiguous
 * fp32 segment, n % 4 == 0, p and ema 16-byte aligned, clip_dev 4-byte aligned; M3AE_ERR_ARG / M3AE_ERR_ALIGN before any launch.
 *
 * m3ae_ema_update: per element, two fp32 roundings:
 *     d   = p - ema
 *     ema = fmaf(w, d, ema)
 *   with w = 1 - decay of THIS update, formed in double by the caller and rounded to fp32 once (1.0f - 0.9999f is 3e-4 relative off
 *   1e-4).  p == ema or w == 0 leaves every bit of a finite ema (but its sign where it is a zero: -0 + 0 = +0).  clip_dev: NULL, or the record of m3ae_clip_finalize: skip != 0 -> returns
 *   before touching ema (the step the guard skipped changed no weight); coef is not read.
 * m3ae_ema_swap: exchanges p[i] and ema[i] exactly; shadow_bf16 (NULL, or 8-byte aligned) receives the bf16 rounding of the new p[i]
 *   as the optimizer kernels round it.  Two calls are the identity on all three buffers.
 */
int m3ae_ema_update(const float* p, float* ema, int64_t n, float w, const float* clip_dev, void* stream);
int m3ae_ema_swap(float* p, float* ema, void* shadow_bf16, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * LoRA, merged form (ABI 4, additive; csrc/lora.hip).  The reference has no counterpart.  A table is `ntargets` records of six
 * int64 {elem_offset, N, K, a_off, b_off, base_off}:  W[N][K] at elem_offset of the flat fp32 master `flat` (and of the bf16 shadow),
 * A[r][K] at a_off and B[N][r] at b_off of the adapter buffer `lora` (in m3ae_lora_grad: dA / dB at the same offsets of `lora_grad`),
 * W0[N][K] at base_off of `base`.  One rank r in 1..M3AE_LORA_MAX_RANK for the table, 1 <= ntargets <= M3AE_LORA_MAX_TARGETS
 * (M3AE_ERR_UNSUPPORTED above either), N, K >= 1, every offset a multiple of 4 elements (ParamStore: 64).  The table is in DEVICE
 * memory and is not checked against the buffers: the caller validates it (m3ae_amd/lora.py: LoraTable).  No atomics; every result is
 * a function of the inputs alone.
 *
 * m3ae_lora_merge: per element, r + 1 fused multiply-adds in this order
 *     acc = 0;  for j = 0 .. r-1: acc = fmaf(B[n][j], A[j][k], acc);     W[n][k] = fmaf(s, acc, W0[n][k])
 *   written to `flat` and, where shadow_bf16 is not NULL, as its round-to-nearest-even bf16 to the shadow.  B = 0 gives W0 bit for
 *   bit (a W0 of -0 becomes +0).  mode 1: W = W0 and its shadow; A, B and s are not read (lora may be NULL).  Only the N * K elements
 *   of each target are written.  base, lora, flat 16-byte aligned, shadow 8-byte.
 * m3ae_lora_grad: dB[n][j] = s * acc, acc = 0; for k = 0 .. K-1: acc = fmaf(dW[n][k], A[j][k], acc);
 *   dA[j][k] = s * (((P_0 + P_1) + P_2) + ...), P_p = the chain acc = fmaf(B[n][j], dW[n][k], acc) over the rows n of row panel p
 *   (M3AE_LORA_PANEL_ROWS rows each, ascending).  dW = grad_flat at elem_offset, read once; the outputs are overwritten; the planes
 *   P_p live in `workspace` (4-byte aligned, m3ae_lora_grad_workspace_bytes of a HOST copy of the same table; NULL: M3AE_ERR_WORKSPACE).
 */
enum { M3AE_LORA_MAX_RANK = 64, M3AE_LORA_MAX_TARGETS = 512, M3AE_LORA_PANEL_ROWS = 64 };
int m3ae_lora_merge(const int64_t* table_dev, int64_t ntargets, int64_t r, float s, const float* base, const float* lora, float* flat,
                    void* shadow_bf16, int mode, void* stream);
int64_t m3ae_lora_grad_workspace_bytes(const int64_t* table_host, int64_t ntargets, int64_t r);
int m3ae_lora_grad(const int64_t* table_dev, int64_t ntargets, int64_t r, float s, const float* lora, const float* grad_flat,
                   float* lora_grad, void* workspace, void* stream);

/* bf16 [R, C] <- fp32 [R, C] cast; and the transposed bf16 copy out_t [C, R] (dgrad operand). either may be NULL */
int m3ae_cast_transpose(const float* in, void* out, void* out_t, int64_t R, int64_t C, void* stream);
/* every weight unit in one launch: jobs_dev = device array of {const float* in; bf16* out_t; int64 R, C, first_tile}
 * (first_tile = running sum of ceil(R/32)*ceil(C/32)), total_tiles = the final running sum. */
int m3ae_cast_transpose_batched(const void* jobs_dev, int njobs, int64_t total_tiles, void* stream);
/* the same from bf16 sources (the weight shadows the optimizer kernel has just written): jobs_dev = device array of
 * {const bf16* in; bf16* out_t; int64 R, C, first_tile} with first_tile = running sum of ceil(R/64)*ceil(C/64).
 * (the reference has no counterpart: weights are used transposed-on-the-fly by torch.nn.functional.linear's backward,
 * /root/reference/m3ae/modules/language_encoders/bert_model.py:419-441) */
int m3ae_transpose_bf16_batched(const void* jobs_dev, int njobs, int64_t total_tiles, void* stream);
/* The tiled copies the NT GEMMs read under M3AE_GEMM_B_TILED (layout: csrc/tiled_b.h), in one pass over the bf16 sources.
 * jobs_dev = device array of {const bf16* in; bf16* out_tiled; bf16* out_t; bf16* out_t_tiled; int64 R, C, first_tile}: per unit
 * in[R][C], any of
 *   out_tiled   -- tiled copy of in   (forward operand: N = R, K = C; needs C % 32 == 0; pad256(R) * C elements),
 *   out_t       -- row-major in^T [C][R], what m3ae_transpose_bf16_batched writes,
 *   out_t_tiled -- tiled copy of in^T (dgrad operand: N = C, K = R; needs R % 32 == 0; pad256(C) * R elements);
 * NULL = not wanted.  Padding rows of the tiled copies are written as zeros.  R % 8 == 0, C % 8 == 0 and 16-byte aligned pointers
 * are preconditions of every unit.  first_tile = running sum of ceil(Rp / 64) * ceil(Cp / 64) with Rp = pad256(R) if out_tiled else
 * R and Cp = pad256(C) if out_t_tiled else C; total_tiles = the final sum.  ABI 4, additive. */
int m3ae_tile_bf16_batched(const void* jobs_dev, int njobs, int64_t total_tiles, void* stream);
/* elementwise: out = cast(in) (dtype_in -> dtype_out), n elements */
int m3ae_cast(const void* in, void* out, int64_t n, int dtype_in, int dtype_out, void* stream);
/* out = a + b (same dtype) */
/* stream-ordered zero fill of `bytes` bytes (the flat gradient buffer before a step; hipMemsetAsync) */
int m3ae_zero(void* p, int64_t bytes, void* stream);
int m3ae_add(const void* a, const void* b, void* out, int64_t n, int dtype, void* stream);
/* dx = dy * act'(x_pre) ; y = act(x) standalone forms */
int m3ae_act_fwd(const void* x, void* y, int64_t n, int act, int dtype, void* stream);
int m3ae_act_bwd(const void* dy, const void* x_pre, void* dx, int64_t n, int act, int dtype, void* stream);
/* rows gather / scatter-add along dim 0 of a [R, D] matrix: out[i] = in[idx[i]] ; d_in[idx[i]] += d_out[i]
 * (MIM masking, m3ae_module.py:170; prediction_heads.py:68).  idx may repeat rows in m3ae_gather_rows; m3ae_scatter_add_rows is
 * a plain read-modify-write and requires the entries of idx to be DISTINCT (a permutation slice): with a repeated entry
 * contributions are lost. */
int m3ae_gather_rows(const void* in, const int64_t* idx, void* out, int64_t n_out, int64_t D, int dtype,
                     void* stream);
int m3ae_scatter_add_rows(const void* d_out, const int64_t* idx, void* d_in, int64_t n_out, int64_t D, int dtype,
                          void* stream);

/* Masked-image-modelling bookkeeping of pre-training.
 * m3ae_mask_ranks: M3AETransformerSS.random_masking's index work (m3ae_module.py:153-183) for a given noise [B, L]
 *   (fp32): ids_restore[b][j] = rank of patch j (= argsort(argsort(noise)), ties by index); mask[b][j] = 1 for removed
 *   patches (rank >= len_keep); keep_rows [B, len_keep + 1]: flat row ids into the [B * (L + 1)] token rows, class row
 *   first, then the kept patches in rank order (the gather of :176-180).
 * m3ae_mim_targets: patchify (m3ae_module.py:185-192) of img [B, C, H, W] fp32 into out [B, (H/P)(W/P), P*P*C] fp32,
 *   element order (p, q, c); norm_pix != 0 standardises every patch with the unbiased variance + 1e-6
 *   (objectives.py:52-56).
 * m3ae_mim_loss_fwd / _bwd: objectives.py:58-62 on the decoder output x [B, L + 1, D] (class row skipped,
 *   prediction_heads.py:86), target [B, L, D] fp32, mask [B, L] fp32: loss[0] = sum_n mask mean_d (x - t)^2 / sum mask.
 *   acc: fp32[2] scratch owned by the caller, written by fwd (masked error sum, mask sum) and read by bwd;
 *   gout: fp32[1] device scalar (upstream gradient); dx [B, L + 1, D] (class rows zero). */
int m3ae_mask_ranks(const float* noise, int64_t* ids_restore, int64_t* keep_rows, float* mask, int64_t B, int64_t L,
                    int64_t len_keep, void* stream);
int m3ae_mim_targets(const float* img, float* out, int64_t B, int64_t C, int64_t H, int64_t W, int64_t P, int norm_pix,
                     void* stream);
int m3ae_mim_loss_fwd(const void* x, const float* target, const float* mask, float* acc, float* loss, int64_t B, int64_t L,
                      int64_t D, int dtype, void* stream);
int m3ae_mim_loss_bwd(const void* x, const float* target, const float* mask, const float* acc, const float* gout, void* dx,
                      int64_t B, int64_t L, int64_t D, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Deterministic mode: ordered forms of the reductions that more than one workgroup feeds.  Same arguments and results as the
 * entry points they are named after (which keep their kernels and their fp32 atomics), plus a caller-owned workspace where
 * noted: every workgroup stores its partial to a workspace row of its own and a second kernel adds the rows in an order
 * that depends on the shapes alone.  m3ae_det_workspace_bytes(op, rows, cols) gives the size (touches no device):
 *   M3AE_DET_COLSUM (M, N); M3AE_DET_EMBED_BWD (B * S, D); M3AE_DET_BCE (B, C); M3AE_DET_XENT (rows, C) -- this workspace
 *   replaces m3ae_xent's float[1]; M3AE_DET_MIM (B * L, D).
 * m3ae_layernorm_bwd_det / _drop_det (and _bwd_mixed_det above): the dgamma / dbeta fold walks all partial rows of `workspace`
 *   (sized as for m3ae_layernorm_bwd) in one workgroup per 32 columns; arguments and checks: the LayerNorm section.
 * m3ae_roberta_embed_bwd_det: the first token that carries a word id (position id) owns that table row and adds the rows of
 *   all tokens with the same id in ascending token order, then adds the sum into the table: no atomics, any duplicates.
 *   D <= 2048.
 */
enum { M3AE_DET_COLSUM = 0, M3AE_DET_EMBED_BWD = 1, M3AE_DET_BCE = 2, M3AE_DET_XENT = 3, M3AE_DET_MIM = 4 };
int64_t m3ae_det_workspace_bytes(int op, int64_t rows, int64_t cols);
int m3ae_colsum_det(const void* x, float* out, int64_t M, int64_t N, int64_t ldx, int dtype, int accumulate, void* workspace,
                    int64_t workspace_bytes, void* stream);
int m3ae_layernorm_bwd_det(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean,
                           const float* rstd, void* dx, const void* dx_add, float* dgamma, float* dbeta, float* workspace,
                           int64_t M, int64_t D, int dtype, int act, int rms, void* stream);
int m3ae_layernorm_bwd_drop_det(const void* dy, const void* x, const float* gamma, const float* beta, const float* mean,
                                const float* rstd, void* dx, void* dx_drop, float dropout_p, uint64_t dropout_seed,
                                const void* dropout_salt, float* dgamma, float* dbeta, float* workspace, int64_t M, int64_t D,
                                int dtype, void* stream);
int m3ae_roberta_embed_bwd_det(const int64_t* ids, const void* d_out, float* d_word, float* d_pos, float* d_type, int64_t B,
                               int64_t S, int64_t D, int64_t pad_id, int dtype, void* workspace, int64_t workspace_bytes,
                               void* stream);
int m3ae_bce_logits_det(const void* logits, const float* targets, float* loss, void* d_logits, int64_t B, int64_t C,
                        float grad_scale, int dtype, void* workspace, int64_t workspace_bytes, void* stream);
int m3ae_xent_det(const void* logits, const int64_t* labels, float* loss, void* d_logits, int64_t rows, int64_t C, int64_t ld,
                  float grad_scale, int dtype, void* workspace, int64_t workspace_bytes, void* stream);
int m3ae_mim_loss_fwd_det(const void* x, const float* target, const float* mask, float* acc, float* loss, int64_t B, int64_t L,
                          int64_t D, int dtype, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-resident beam search (csrc/beam.hip; ABI 4, additive): transformers-4.6.0 `beam_search` + `BeamSearchScorer` as
 * T5ForConditionalGeneration.generate restates them (the reference runs HF `generate` at m3ae_t5_mm_encoder_input.py:209-218,
 * 252-261), with the per-step bookkeeping on device state.  R = B * nb beam rows, nb <= 8; no atomics anywhere: two calls on the
 * same inputs give the same bits.
 *
 * m3ae_beam_topk: logits fp32 [R][V] with row stride ld >= V, beam_scores fp32 [R].  Per row m = max x, lse = log sum exp(x - m)
 *   (fp32, summation order fixed by V and chunk), score = fl(fl(fl(x - m) - lse) + beam_score); per sample the best 2 nb of its
 *   nb * V candidates into top_s fp32 [B][2 nb] / top_i int32 [B][2 nb], ordered by (rounded score descending, flat index
 *   beam * V + token ascending).  top_i entries are distinct and in [0, nb * V) whatever the logits hold (NaN ranks somewhere).
 *   Rows are split over vocabulary chunks of `chunk` elements (0 = 2048; at most 4096), one workgroup per (row, chunk), partial
 *   lists merged by a second stage.  workspace: m3ae_beam_topk_workspace_bytes(B, nb, V, chunk) bytes, 8-byte aligned.
 *   M3AE_ERR_UNSUPPORTED unless 1 <= nb <= 8, V >= 2 nb + 1, nb * V < 2^31 and chunk <= 4096.
 * m3ae_beam_step: one scorer step at prefix length cur_len (1 <= cur_len < max_length) from the candidates of m3ae_beam_topk.
 *   Per sample, in rank order: an EOS candidate at rank >= nb is skipped; at rank < nb it pushes (score / div, source prefix) into
 *   the sample's hypothesis list -- double arithmetic, div = cur_len ** length_penalty computed by the caller; the list stays
 *   sorted descending with a new entry AFTER equal scores and is cut to nb; other candidates fill the next nb beams.  A sample is
 *   done once it holds nb hypotheses; a done sample gets source row b * nb, pad tokens and score 0 for all its beams.
 *   ids_in / ids_out int64 [R][max_length] (different buffers: a row may feed several rows), last_tok int64 [R] (the new column),
 *   beam_scores fp32 [R], order int64 [R] (source rows, for m3ae_gather_rows of the key / value caches), done / n_hyp int32 [B],
 *   hyp_score double [B][nb], hyp_len int32 [B][nb], hyp_tok int64 [B][nb][max_length]; open_count int32 [1] receives the number
 *   of samples not done after the step; err int64 [1] is set to 1 when a top_i entry is outside [0, nb * V) (the entry is
 *   skipped, never turned into an address).
 * m3ae_beam_finalize: samples not done push their nb open beams (ids [R][max_length], prefix length cur_len) with
 *   beam_score / div, div = (cur_len - len_offset) ** length_penalty; then seq int64 [B][max_length] = the best hypothesis, EOS
 *   appended when shorter than max_length, pad after it, and len int64 [B] = its length. */
int64_t m3ae_beam_topk_workspace_bytes(int64_t B, int64_t nb, int64_t V, int64_t chunk);
int m3ae_beam_topk(const float* logits, int64_t ld, const float* beam_scores, int64_t B, int64_t nb, int64_t V, int64_t chunk,
                   void* workspace, int64_t workspace_bytes, float* top_s, int32_t* top_i, void* stream);
int m3ae_beam_step(const float* top_s, const int32_t* top_i, const int64_t* ids_in, int64_t* ids_out, int64_t* last_tok,
                   float* beam_scores, int64_t* order, int32_t* done, int32_t* n_hyp, double* hyp_score, int32_t* hyp_len,
                   int64_t* hyp_tok, int32_t* open_count, int64_t* err, int64_t B, int64_t nb, int64_t V, int64_t max_length,
                   int64_t cur_len, int64_t eos, int64_t pad, double div, void* stream);
int m3ae_beam_finalize(const int64_t* ids, const float* beam_scores, const int32_t* done, int32_t* n_hyp, double* hyp_score,
                       int32_t* hyp_len, int64_t* hyp_tok, int64_t* seq, int64_t* len, int64_t B, int64_t nb, int64_t max_length,
                       int64_t cur_len, int64_t eos, int64_t pad, double div, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-resident greedy search (csrc/greedy.hip; ABI 4, additive): the per-token work of the decoder head's `search_path`
 * (reference m3ae_decoder.py:141-182) -- argmax over the vocabulary, [SEP] / EOS detection, the growing sequence and the count
 * of unfinished rows -- on device state.  Integer compares only, no atomics: two calls on the same inputs give the same bits.
 *
 * m3ae_greedy_argmax: logits [R][V], dtype M3AE_F32 or M3AE_BF16, row stride ld >= V in elements (columns [V, ld) are never
 *   read); the base pointer is element-aligned, nothing else is asked of ld.  Rows are split over vocabulary chunks of `chunk`
 *   elements (0 = 2048; 64 <= chunk <= 65536), one workgroup per (row, chunk); each writes the maximum of its chunk's order keys,
 *   (monotone image of the fp32 value) << 32 | (2^32 - 1 - column), to workspace[row][chunk] (uint64; the key of beam.hip).  The
 *   maximum of a row's keys is torch.argmax's choice: the greatest value, the lowest column among equal values (+0 == -0), and
 *   any NaN (either sign) above every number, the first NaN winning.  workspace: m3ae_greedy_workspace_bytes(R, V, chunk) bytes
 *   (0 for shapes the call rejects), 8-byte aligned.  tokens: optional int64 [R], receives the decoded column of every row.
 *   M3AE_ERR_UNSUPPORTED for another dtype, chunk outside its bounds, V >= 2^31 or R * chunks >= 2^31.
 * m3ae_greedy_step: one search step at position pos (0 <= pos < max_len) from the keys of m3ae_greedy_argmax (nch chunks per row).
 *   For row r with tok its argmax: last_tok[r] = tok always (the host loop feeds the raw token back after a row has finished,
 *   too); a finished row gets seq[r][pos] = pad; an open row gets seq[r][pos] = tok and, when tok == sep or (eos >= 0 and
 *   tok == eos), finished[r] = 1 and len[r] = pos + 1.  open_count[pos] = rows not finished after the step.  seq int64
 *   [B][max_len], len / last_tok int64 [B], finished int32 [B], open_count int32 [max_len]; err int64 [1] is set to 1 when a
 *   decoded column is outside [0, V) (the row then continues with token 0: never an address). */
int64_t m3ae_greedy_workspace_bytes(int64_t R, int64_t V, int64_t chunk);
int m3ae_greedy_argmax(const void* logits, int64_t ld, int64_t R, int64_t V, int64_t chunk, int dtype, void* workspace,
                       int64_t workspace_bytes, int64_t* tokens, void* stream);
int m3ae_greedy_step(const void* keys, int64_t nch, int64_t* seq, int64_t* len, int64_t* last_tok, int32_t* finished,
                     int32_t* open_count, int64_t* err, int64_t B, int64_t V, int64_t max_len, int64_t pos, int64_t sep, int64_t eos,
                     int64_t pad, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sample expansion of a de-duplicated image batch (csrc/samples.hip; ABI 4, additive): the image tower runs once per distinct
 * image of a batch and its [n_in][R] output (R = tokens * width elements per image, fp32 or bf16) is expanded to the batch's
 * samples.  Row bases are 64-bit element offsets; rows move in 16-byte units when R * sizeof(element) is a multiple of 16 and
 * both base pointers are 16-byte aligned, element by element otherwise.
 *
 * m3ae_expand_samples: out[b] = in[src[b]], b < n_out; src int64 [n_out] with values in [0, n_in) (a value outside is never
 *   dereferenced: that output row is left untouched).
 * m3ae_segment_sum_rows: its backward, d_in[u] = sum of d_out[members[j]] for offsets[u] <= j < offsets[u + 1]; offsets int64
 *   [n_in + 1], members int64 [n_out] (a CSR of the samples of every image, each list in ascending sample order).  One lane owns
 *   an output element: it adds the members in list order in an fp32 register, starting from the first member, and rounds once to
 *   the storage dtype (bf16: round-to-nearest-even).  No atomics: the same bits on every run, a group of one is a copy. */
int m3ae_expand_samples(const void* in, const int64_t* src, void* out, int64_t n_out, int64_t n_in, int64_t R, int dtype,
                        void* stream);
int m3ae_segment_sum_rows(const void* d_out, const int64_t* offsets, const int64_t* members, void* d_in, int64_t n_in,
                          int64_t n_out, int64_t R, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-side VQA evaluation (csrc/vqa_eval.hip; ABI 4, additive): the prediction, the top-k answers and the closed / open / overall
 * score sums of a validation pass, with no host involvement.
 *
 * The record: double rec[M3AE_VQA_REC_DOUBLES] in device memory, zeroed by the caller (m3ae_zero) before the first update.  For
 *   group g of (all, closed, open): rec[3 g + 0] = n_g rows seen, rec[3 g + 1] = sum of hit1, rec[3 g + 2] = sum of hitk;
 *   rec[9] = number of update calls.  A row's group is types[r]: M3AE_ANS_CLOSED or M3AE_ANS_OPEN (the reference's values,
 *   my_metrics.py:180-181); any other value, and every row when types is NULL, counts in "all" only.
 *
 * m3ae_vqa_eval: one workgroup per row.  logits [B][C], dtype M3AE_F32 or M3AE_BF16, row stride ld >= C in elements; the base
 *   pointer is element-aligned, nothing else is asked of ld, and columns [C, ld) are never read (as m3ae_greedy_argmax).  targets
 *   fp32 [B][C] with row stride ldt >= C, or NULL; types int32 [B] or NULL.
 *   Ranking: by the order key of m3ae_greedy_argmax -- value descending, the lowest column among equal values (+0 == -0), every
 *   NaN of either sign above every number, the first NaN first.  Rank 0 is torch.max(logits, 1)[1], the reference's prediction
 *   (my_metrics.py:68); ranks 0 .. k - 1 are the top-k, 0 <= k <= 16.  The row is read once; keys of distinct columns are distinct,
 *   so the result depends on no order.
 *   Per row: hit1 = targets[r][rank 0]; hitk = the maximum of targets[r][col] over the top-k (k = 0: 0).
 *   Outputs, each may be NULL: pred int64 [B] (rank 0); topk_idx int32 [B][k]; topk_prob fp32 [B][k] = 1 / (1 + expf(-x)) of the
 *   fp32-widened logit (a NaN logit gives NaN); hit1 fp32 [B] (written only with targets).  NULL targets skip the hits and the
 *   record; NULL rec skips the record.
 *   The fold (targets and rec given): one launch of one workgroup adds the rows' hit1 / hitk and the counts onto rec, in double,
 *   in an order that depends on B alone; no atomics, so deterministic mode needs no second form.  With scores in {0} u [2^-20, 1]
 *   and at most 1024 rows accumulated every sum is exact, whatever the order.  workspace: m3ae_vqa_eval_workspace_bytes(B, k)
 *   bytes (the rows' {hit1, hitk}; 0 for a B or k the call rejects), 8-byte aligned, needed only when the fold runs.
 *   M3AE_ERR_ARG: NULL logits, B < 1, C < 1, k < 0.  M3AE_ERR_UNSUPPORTED, before any launch: k > 16, k > C, C >= 2^31, B >= 2^31,
 *   a dtype other than fp32 / bf16, ld < C (ldt < C), a missing or short workspace.  M3AE_ERR_ALIGN: a pointer off its element size.
 *
 * m3ae_seq_match: TOKEN exact match for the generator heads.  gen int64 [B][Lg] (row stride ldg), ref int64 [B][Lr] (row stride
 *   ldr), skip int64 [ns], 0 <= ns <= 8 (device memory; pad / start / end ids).  Row r matches iff the subsequence of gen[r] with
 *   ids outside skip equals the same subsequence of ref[r]; hit1 = hitk = 1.0 or 0.0 go onto rec through the same fold (types,
 *   rec and workspace as above; rec is required).  match: optional int32 [B].  One thread per row, one workgroup per 256 rows.
 *   Equal ids imply equal decoded strings, so this is a LOWER BOUND of the reference's string VQAExactMatch (my_metrics.py:80-96:
 *   two id sequences may decode to the same text); it is not that metric.
 *   M3AE_ERR_UNSUPPORTED: ns > 8, B >= 2^31, ldg < Lg, ldr < Lr, a missing or short workspace. */
enum { M3AE_ANS_CLOSED = 0, M3AE_ANS_OPEN = 1 };
enum { M3AE_VQA_REC_DOUBLES = 10, M3AE_VQA_MAX_K = 16 /* the bound on k above */, M3AE_SEQ_MAX_SKIP = 8 /* the bound on ns */ };
int64_t m3ae_vqa_eval_workspace_bytes(int64_t B, int64_t k);
int m3ae_vqa_eval(const void* logits, int64_t ld, const float* targets, int64_t ldt, const int32_t* types, int64_t B, int64_t C,
                  int64_t k, int dtype, int64_t* pred, int32_t* topk_idx, float* topk_prob, float* hit1, double* rec,
                  void* workspace, int64_t workspace_bytes, void* stream);
int m3ae_seq_match(const int64_t* gen, int64_t ldg, int64_t Lg, const int64_t* ref, int64_t ldr, int64_t Lr, const int64_t* skip,
                   int64_t ns, const int32_t* types, int64_t B, int32_t* match, double* rec, void* workspace,
                   int64_t workspace_bytes, void* stream);
/* m3ae_vqa_label_eval: the same record from LABELS (answer-list decoding, below: a generator head's output is a list entry).
 *   labels int64 [B]; targets fp32 [B][C] with row stride ldt >= C (required); per row hit1 = hitk = targets[r][labels[r]], added
 *   onto rec through the same fold (types, rec, workspace as m3ae_vqa_eval; rec is required).  A label outside [0, C) scores 0 and
 *   sets err[0] = 1 (int64, required): a label is turned into an address only after that check.  hit1: optional fp32 [B].
 *   M3AE_ERR_ARG: NULL labels / targets / rec / err, B < 1, C < 1.  M3AE_ERR_UNSUPPORTED: C >= 2^31, B >= 2^31, ldt < C, a missing or
 *   short workspace.  M3AE_ERR_ALIGN: a pointer off its element size. */
int m3ae_vqa_label_eval(const int64_t* labels, const float* targets, int64_t ldt, const int32_t* types, int64_t B, int64_t C,
                        float* hit1, double* rec, int64_t* err, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Answer-list decoding (csrc/answer_trie.hip; ABI 4, additive): greedy search of a generator head constrained to a prefix trie of
 * candidate answers, so that every output is a list entry (a label) and arrives with its log-probability.  No atomics, every
 * reduction in a fixed order: two calls on the same inputs give the same bits, the score included.
 *
 * The trie, in device memory, int32: child_off [N + 1], child_tok [E] (ascending within a node), child_node [E], leaf_label [N]
 *   (the label at the node behind an end token, -1 elsewhere); node 0 is the root; the children of node n are entries
 *   child_off[n] .. child_off[n + 1] - 1.  The caller checks the table (tokens < V, every non-leaf node has a child); the kernels
 *   turn no table value into an address without a range check and report a row they cannot advance through err.
 *
 * m3ae_trie_scan: logits [R][V], dtype M3AE_F32 or M3AE_BF16, row stride ld >= V in elements, element-aligned base, columns
 *   [V, ld) never read (as m3ae_greedy_argmax).  node int32 [R]: the row's trie node; finished int32 [R]: nothing of a row with
 *   a nonzero word is read or written.  chunk: columns per workgroup, 0 = 8192, 64 <= chunk <= 65536.  Per row, chunks + 1
 *   workgroups: one per vocabulary chunk writes the chunk's (m, s) = (maximum, sum of e(x, m)) in fp32 (the arithmetic of
 *   m3ae_token_eval) to workspace; one gathers the logits at the child tokens of the row's node, however many, and writes the
 *   greatest order key (monotone image of the value) << 32 | (2^32 - 1 - child position): the greatest value, the lowest token
 *   among equal values (+0 == -0), any NaN above every number -- torch.argmax's rule restricted to the allowed columns.
 *   workspace: m3ae_trie_workspace_bytes(R, V, chunk) bytes (0 for shapes the call rejects), 8-byte aligned.
 *   M3AE_ERR_ARG: a NULL pointer, R < 1, V < 1, ld < V, chunk < 0, N < 1, E < 1.  M3AE_ERR_UNSUPPORTED: another dtype, chunk outside
 *   its bounds, V, N or E >= 2^31, R * (chunks + 1) >= 2^31.  M3AE_ERR_ALIGN: a pointer off its element size.  M3AE_ERR_WORKSPACE:
 *   a missing, misaligned or short workspace.
 * m3ae_trie_step: one search step at position pos (0 <= pos < max_len) from the workspace of m3ae_trie_scan on the same logits
 *   (nch = chunks per row).  For an open row: lse = m + logf(s) of the row's pairs folded in ascending chunk order; tok and the
 *   next node come from the child position the key decodes to; score[r] += (double)(x[tok] - lse) with the difference in fp32;
 *   seq[r][pos] = last_tok[r] = tok; node[r] = the next node; if leaf_label[node] >= 0 then label[r] = it, len[r] = pos + 1 and
 *   finished[r] = 1.  A finished row gets seq[r][pos] = pad and keeps node, score, label and last_tok.  open_count[pos] = rows
 *   not finished after the step.  A non-finite row gives what torch.log_softmax gives, by the same arithmetic.  seq int64
 *   [B][max_len]; len / label / last_tok int64 [B]; score double [B]; node / finished int32 [B]; open_count int32 [max_len]; err
 *   int64 [1] is set to 1 when a node, a decoded child position, a token or a next node is outside its range (the row then
 *   writes token 0, keeps node and score and stays open: never an address).
 *   M3AE_ERR_ARG: a NULL pointer or a count outside its range.  M3AE_ERR_UNSUPPORTED / _ALIGN / _WORKSPACE as above. */
int64_t m3ae_trie_workspace_bytes(int64_t R, int64_t V, int64_t chunk);
int m3ae_trie_scan(const void* logits, int64_t ld, int64_t R, int64_t V, int64_t chunk, int dtype, const int32_t* child_off,
                   const int32_t* child_tok, int64_t N, int64_t E, const int32_t* node, const int32_t* finished, void* workspace,
                   int64_t workspace_bytes, void* stream);
int m3ae_trie_step(const void* logits, int64_t ld, int dtype, const void* workspace, int64_t workspace_bytes, int64_t nch,
                   const int32_t* child_off, const int32_t* child_tok, const int32_t* child_node, const int32_t* leaf_label, int64_t N,
                   int64_t E, int64_t* seq, int64_t* len, int64_t* label, double* score, int64_t* last_tok, int32_t* node,
                   int32_t* finished, int32_t* open_count, int64_t* err, int64_t B, int64_t V, int64_t max_len, int64_t pos,
                   int64_t pad, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Constrained beam search on the answer list (csrc/trie_beam.hip; ABI 4, additive): transformers-4.6.0 `beam_search` +
 * `BeamSearchScorer` (as m3ae_beam_step) with the trie above as the prefix constraint; the result of a sample is an n-best list of
 * labels with scores.  Log-probabilities come from the UNCONSTRAINED softmax; a token the trie does not allow is not a candidate.
 * No atomics: two calls on the same inputs give the same bits.
 *
 * Rows and state.  R = B * nb beam rows, 1 <= nb <= 8, row b * nb + k is slot k of sample b.  Per row: node int32 (-1 = a DEAD
 *   slot), beam_score fp32, last_tok int64.  At the start slot 0 of every sample is at the root (node 0) with score 0 and slots 1..
 *   are dead; a dead slot contributes no candidate (there is no -1e9 trick).  m3ae_trie_scan runs unchanged over the R rows with
 *   the dead flags (int32 [R], written by the step) as its `finished` argument: nothing of a dead row is read.
 * Candidates of a sample: the children of its live beams' nodes.  lse of a row = m + logf(s) of its (m, s) pairs folded in
 *   ascending chunk order (as m3ae_trie_step); score = fl(fl(x[tok] - lse) + beam_score) in fp32.  The best min(2 nb, candidates)
 *   are kept, by rounded score descending, then (beam, entry) ascending -- which is (beam, token) ascending, tokens ascend within a
 *   node; +0 == -0, any NaN ranks above every number.
 * m3ae_triebeam_select: logits [R][V] as m3ae_trie_scan (fp32 or bf16, row stride ld >= V, element-aligned base), workspace = the
 *   one m3ae_trie_scan filled from the same logits with the same chunk (m3ae_trie_workspace_bytes(R, V, chunk) bytes).  One
 *   workgroup of 256 threads per sample.  Outputs: top_s fp32 [B][2 nb], top_beam int32 [B][2 nb] (the slot, 0 .. nb - 1), top_edge
 *   int32 [B][2 nb] (the entry of child_tok / child_node), n_cand int32 [B] (the number kept); unused slots carry score 0, beam -1
 *   and entry -1.  err int64 [1] is set to 1 by a live node outside [0, N) or without a child range and by a token outside [0, V):
 *   such a candidate is skipped and never turned into an address.
 *   M3AE_ERR_ARG: a NULL pointer, B < 1, V < 1, ld < V, chunk < 0, N < 1, E < 1.  M3AE_ERR_UNSUPPORTED: another dtype, nb outside
 *   [1, 8], nb * E >= 2^31, N >= 2^31, or (B * nb, V, chunk) not a shape m3ae_trie_scan takes.  M3AE_ERR_ALIGN: a pointer off its
 *   element size.  M3AE_ERR_WORKSPACE: a missing, misaligned or short workspace.
 * m3ae_triebeam_step: one step at position pos (0 <= pos < max_len); div = (pos + 1) ** length_penalty > 0 (HF's cur_len
 *   divisor, computed by the caller).  One thread per sample walks the candidates in rank order.  A candidate whose next node is a
 *   leaf (leaf_label >= 0) is skipped at rank >= nb; at rank < nb it pushes (score / div in double, score, label, pos + 1) into the
 *   sample's hypothesis list (scores descending, a new entry after equal scores, cut to nb).  Other candidates fill the next beam
 *   slots (beam_score, last_tok, order = the source row, node = the next node) until nb are filled; the remaining slots become dead:
 *   node -1, beam_score 0, last_tok = pad, order = b * nb (always a valid row and a valid embedding index).  A sample is done once
 *   it holds nb hypotheses or has no live beam; all slots of a done sample are dead.  open_count[pos] = samples not done.  Every
 *   path ends within the trie's depth, so after that many steps no beam is live, every sample holds at least one hypothesis and
 *   no finalize pass is needed.
 *   The hypothesis lists are the result: labels int64 [B][nb] (the caller fills them with -1), scores double [B][nb] (normalised),
 *   logprob double [B][nb] (the raw fp32 sums), hyp_len int64 [B][nb], n_hyp int64 [B] (the caller zeroes it); best int64 [B] =
 *   max(labels[b][0], 0) and len int64 [B] = hyp_len[b][0] once the sample holds a hypothesis.  order int64 [R] is the index of
 *   m3ae_gather_rows for the key / value caches; dead int32 [R]; done int32 [B].  err int64 [1] is set to 1 when a slot, an entry
 *   (also one that is not a child of the slot's node), a token, a next node or a label (A = the number of answers) is outside
 *   its range: the candidate is skipped.
 *   M3AE_ERR_ARG: a NULL pointer, a count outside its range, div <= 0.  M3AE_ERR_UNSUPPORTED: nb outside [1, 8], nb * E >= 2^31,
 *   B * nb >= 2^31.  M3AE_ERR_ALIGN: a pointer off its element size. */
int m3ae_triebeam_select(const void* logits, int64_t ld, int64_t B, int64_t nb, int64_t V, int64_t chunk, int dtype,
                          const int32_t* child_off, const int32_t* child_tok, int64_t N, int64_t E, const int32_t* node,
                          const float* beam_score, const void* workspace, int64_t workspace_bytes, float* top_s, int32_t* top_beam,
                          int32_t* top_edge, int32_t* n_cand, int64_t* err, void* stream);
int m3ae_triebeam_step(const float* top_s, const int32_t* top_beam, const int32_t* top_edge, const int32_t* child_off,
                        const int32_t* child_tok, const int32_t* child_node, const int32_t* leaf_label, int64_t N, int64_t E,
                        int32_t* node, float* beam_score, int64_t* last_tok, int64_t* order, int32_t* dead, int32_t* done,
                        int64_t* n_hyp, int64_t* labels, double* scores, double* logprob, int64_t* hyp_len, int64_t* best, int64_t* len,
                        int32_t* open_count, int64_t* err, int64_t B, int64_t nb, int64_t V, int64_t A, int64_t max_len, int64_t pos,
                        int64_t pad, double div, void* stream);
/* m3ae_vqa_labels_eval: the n-best form of m3ae_vqa_label_eval.  labels int64 [B][k] with row stride ldl >= k, 1 <= k <= 16;
 *   hit1 = targets[r][labels[r][0]], hitk = the maximum of targets[r][l] over the row's entries l >= 0.  An entry of -1 in columns
 *   1.. is an empty slot and is skipped; any other value outside [0, C), or an empty column 0, scores 0 and sets err[0] = 1.  The
 *   fold, record and workspace are m3ae_vqa_label_eval's.  M3AE_ERR_ARG: NULL labels / targets / rec / err, B < 1, C < 1, k < 1.
 *   M3AE_ERR_UNSUPPORTED: k > 16, ldl < k, C >= 2^31, B >= 2^31, ldt < C, a missing or short workspace.  M3AE_ERR_ALIGN as above. */
int m3ae_vqa_labels_eval(const int64_t* labels, int64_t ldl, int64_t k, const float* targets, int64_t ldt, const int32_t* types,
                         int64_t B, int64_t C, float* hit1, double* rec, int64_t* err, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Exhaustive answer-list scoring (csrc/tree_attn.hip, csrc/list_score.hip; ABI 4, additive): the log-probability of EVERY entry of
 * the answer list from one decoder pass over the internal nodes of the answer trie (the nodes that have children: a decoder row
 * computed for a node serves every answer through it), the list's arg-max, its k best entries with probabilities over the list and
 * the mass the head puts on the list.  No atomics, every reduction in a fixed order: two calls on the same inputs give the same bits.
 *
 * Tables, int32, device memory, beside the trie above: internal [Ni] (the nodes with children, ascending), anc [Ni][Dmax] (for
 *   internal row i the internal rows from the root, first, to i itself, last, then -1), parent [N] (-1 at the root), depth [N],
 *   level_off [Dmax + 2] (the nodes of depth d are level_off[d] .. level_off[d + 1] - 1), leaf_node [A] (the leaf of each label).
 *   Nodes are numbered breadth-first in the order their edges are made: the edge into node n is entry n - 1 of child_tok, E = N - 1,
 *   a parent precedes its children.  The caller checks the tables; the kernels turn no table value into an address without a range
 *   check and report through err int64 [1].
 *
 * m3ae_tree_attn: attention whose keys are a row's trie ancestors, forward only, no dropout.  q, k, v [G][Ni][H * Dh] with row
 *   strides ldq / ldk / ldv >= H * Dh in elements (row g * Ni + i starts at row * ld: the thirds of a packed qkv buffer qualify),
 *   out [G][Ni][H * Dh] with row stride ldo, all of dtype M3AE_F32 or M3AE_BF16; Dh 64 or 96; 1 <= Dmax <= 32.  rel_bias fp32
 *   [H][Dmax] or NULL: rel_bias[h][depth(query) - depth(key)] is added to a score.  One wave per (group, row, head); arithmetic in
 *   fp32 in the order csrc/tree_attn.hip documents: dot product (a lane's one or two products, then a 6-stage butterfly), s =
 *   fmaf(dot, scale, bias), softmax with the maximum subtracted over the row's 1 .. 32 keys, the weighted sum by ascending key,
 *   one division, one rounding to the output dtype.  A row with one key gives v exactly.  A row whose anc holds no leading entry
 *   >= 0 or an entry >= Ni sets err[0] = 1 and is written as zeros.
 *   M3AE_ERR_ARG: a NULL pointer (rel_bias aside), a count < 1, a stride < H * Dh.  M3AE_ERR_UNSUPPORTED: another dtype, Dh not 64 /
 *   96, Dmax > 32, G * Ni >= 2^31.  M3AE_ERR_ALIGN: a pointer off its element size.
 * m3ae_listscore_lse: logits [R][V] as m3ae_trie_scan takes them (fp32 or bf16, row stride ld >= V, element-aligned base, columns
 *   [V, ld) never read), R = G * Ni; chunk as there (0 = 8192).  One workgroup per (chunk, row) writes the chunk's (m, s) in fp32,
 *   by the arithmetic of m3ae_trie_scan's chunk items, to workspace fp32 [R][chunks][2]: m3ae_listscore_workspace_bytes(R, V, chunk)
 *   bytes (0 for shapes the call rejects), 8-byte aligned.  Status codes as m3ae_trie_scan.
 * m3ae_listscore_edges: from the same logits and that workspace (nch = chunks per row), one workgroup per row g * Ni + i: lse = m +
 *   logf(s) of the row's pairs folded in ascending chunk order (as m3ae_trie_step); edge_lp[g][e] = x[child_tok[e]] - lse in fp32
 *   for every child entry e of node internal[i], any number of them; edge_lp fp32 [G][E].  A node outside [0, N) or without a child
 *   range sets err[0] = 1 and writes nothing; a token outside [0, V) sets err[0] = 1 and its edge is NaN.
 *   M3AE_ERR_ARG: a NULL pointer, a count < 1, ld < V.  M3AE_ERR_UNSUPPORTED: another dtype, V, N, E or G * Ni >= 2^31, Ni > N.
 *   M3AE_ERR_ALIGN; M3AE_ERR_WORKSPACE: a missing, misaligned or short (m, s) workspace.
 * m3ae_listscore_fold: one workgroup per sample b of edge_lp fp32 [B][N - 1].  node_lp[0] = 0 and level by level node_lp[n] =
 *   node_lp[parent[n]] + (double)edge_lp[b][n - 1] -- fp32 terms added in double in path order, m3ae_trie_step's rule, so that on
 *   the same logits an entry's log-probability has the bits that search accumulates along its path.  all_logprob double [B][A] =
 *   node_lp at the labels' leaves; score = logprob / pen[len], pen double [Dmax + 1] = len ** length_penalty from the caller, len =
 *   depth[leaf]; log_mass double [B] = M + log(sum_i exp(logprob_i - M)) over the finite entries, M their maximum, summed in label
 *   order; the 1 <= k <= 16 best entries by (score descending, label ascending) into labels int64 / scores / logprob / probs double
 *   [B][k], probs = exp(logprob - log_mass); ranks >= A hold label -1 and zeros; n_hyp int64 [B] = min(k, A); best int64 [B] =
 *   labels[b][0], len int64 [B] = its token count.  Non-finite values: an entry whose logprob is not finite has probability 0 and adds
 *   nothing to the mass; with no finite entry log_mass = -inf and every probability is 0; a NaN score ranks after every number,
 *   label ascending among NaNs; +0 == -0.  A parent that is not in an earlier level, a level outside [1, N], a leaf outside [1, N) or a depth outside
 *   [1, Dmax] sets err[0] = 1 and yields NaN, never an address.  workspace: m3ae_listscore_fold_workspace_bytes(B, N) bytes (0 while
 *   node_lp fits the workgroup's LDS, N <= 4096; -1 for counts the call rejects), 8-byte aligned.
 *   M3AE_ERR_ARG: a NULL pointer, B < 1, N < 2, A < 1, Dmax < 1, k < 1.  M3AE_ERR_UNSUPPORTED: k > 16, Dmax > 32, A >= N, N or B >=
 *   2^31.  M3AE_ERR_ALIGN: a pointer off its element size.  M3AE_ERR_WORKSPACE: a missing, misaligned or short workspace. */
int m3ae_tree_attn(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out, int64_t ldo,
                   const int32_t* anc, int64_t Dmax, const float* rel_bias, float scale, int64_t G, int64_t Ni, int64_t H, int64_t Dh,
                   int dtype, int64_t* err, void* stream);
int64_t m3ae_listscore_workspace_bytes(int64_t R, int64_t V, int64_t chunk);
int m3ae_listscore_lse(const void* logits, int64_t ld, int64_t R, int64_t V, int64_t chunk, int dtype, void* workspace,
                       int64_t workspace_bytes, void* stream);
int m3ae_listscore_edges(const void* logits, int64_t ld, int64_t G, int64_t Ni, int64_t V, int dtype, const void* workspace,
                         int64_t workspace_bytes, int64_t nch, const int32_t* internal, const int32_t* child_off, const int32_t* child_tok,
                         int64_t N, int64_t E, float* edge_lp, int64_t* err, void* stream);
int64_t m3ae_listscore_fold_workspace_bytes(int64_t B, int64_t N);
int m3ae_listscore_fold(const float* edge_lp, const int32_t* parent, const int32_t* depth, const int32_t* level_off,
                        const int32_t* leaf_node, const double* pen, int64_t B, int64_t N, int64_t A, int64_t Dmax, int64_t k,
                        void* workspace, int64_t workspace_bytes, double* all_logprob, int64_t* labels, double* scores, double* logprob,
                        double* probs, double* log_mass, int64_t* n_hyp, int64_t* best, int64_t* len, int64_t* err, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-side token evaluation (csrc/token_eval.hip; ABI 4, additive): what the reference's `Accuracy` metric computes for the MLM
 * and ITM objectives (my_metrics.py: preds = logits.argmax(-1) over the rows whose target is not -100), plus the label's rank, the
 * negative log-likelihood and the top-k tokens with their softmax probabilities, for rows of vocabulary width, on the device.
 *
 * The record: double rec[M3AE_TOKEN_REC_DOUBLES] in device memory, zeroed by the caller before the first update: rec[0] = n, the
 *   evaluated rows that carry a label; rec[1] = hit1, those with rank == 0; rec[2] = hitk, those with rank < k; rec[3] = the sum of
 *   their nll; rec[4] = number of update calls.
 *
 * m3ae_token_eval.  logits [R][V], dtype M3AE_F32 or M3AE_BF16, row stride ld >= V in elements; the base pointer is
 *   element-aligned, nothing else is asked of ld, and columns [V, ld) are never read (as m3ae_greedy_argmax: scalar head up to the
 *   first 16-byte boundary, 16-byte loads, scalar tail).  labels int64 [R] or NULL; select uint8 [R] or NULL.  chunk: columns per
 *   workgroup, 0 = 8192, 64 <= chunk <= 65536.  0 <= k <= M3AE_TOKEN_MAX_K and k <= V.
 *   Which rows are evaluated: with select, the rows with select[r] != 0; else, with labels, the rows with labels[r] !=
 *   M3AE_TOKEN_IGNORE (-100); else every row.  An evaluated row whose label is neither -100 nor in [0, V) sets err[0] = 1 (int64,
 *   required with labels) and is skipped: a label is turned into an address only after that check.  No logit of a row that is not
 *   evaluated is read.
 *   Ranking: the order key of m3ae_greedy_argmax -- value descending, the lowest column among equal values (+0 == -0), every NaN of
 *   either sign above every number, the first NaN first.  pred is rank 0, torch.argmax's choice.  rank = the number of columns whose
 *   key is strictly greater than the label's: 0 iff pred == label, so a label that ties the maximum from a higher column is no hit.
 *   lse: per chunk (m, s) = (maximum, sum of e(x, m)) in fp32 with e(x, m) = x == m ? 1 : expf(x - m); pairs merge as
 *   m' = fmaxf(m1, m2), s' = s1 e(m1, m') + s2 e(m2, m'); lse = m + logf(s).  Non-finite rows get what torch.logsumexp gives, by the
 *   same arithmetic and no special case: a NaN anywhere gives lse = NaN; a +inf gives lse = +inf (nll = +inf, or NaN when the label
 *   is that column); a row of -inf alone gives lse = -inf and nll = -inf - -inf = NaN.  Such an nll goes into rec[3] as it is.
 *   Outputs, each may be NULL: pred int64 [R]; rank int32 [R] (-1 for an evaluated row without a label); nll fp32 [R] = lse -
 *   x[label] (the lse itself for an evaluated row without a label); topk_idx int32 [R][k]; topk_prob fp32 [R][k] = expf(x_j - lse).
 *   A row that is not evaluated gets pred -1, rank -1, nll 0, topk_idx -1, topk_prob 0.
 *   The fold (rec given): one launch of one workgroup adds the labelled rows onto rec in double, in an order that depends on R
 *   alone; no atomics, so two calls on the same inputs give the same bits and deterministic mode needs no second form.
 *   workspace: m3ae_token_eval_workspace_bytes(R, V, chunk, k) bytes (0 for shapes the call rejects), 8-byte aligned, always needed.
 *   M3AE_ERR_ARG: NULL logits or workspace, R < 1, V < 1, ld < V, chunk < 0, k < 0, labels without err.  M3AE_ERR_UNSUPPORTED, before
 *   any launch: k > 16, k > V, chunk outside its bounds, V >= 2^31, R >= 2^31, R * chunks >= 2^31, a dtype other than fp32 / bf16, a
 *   short workspace.  M3AE_ERR_ALIGN: a pointer off its element size.
 * m3ae_record_add: rec[0] += value[0] (a device fp32 scalar, widened), rec[1] += 1, in double: the running sum and count of a
 *   per-batch loss (the reference's `Scalar` metric) without a host round trip. */
enum { M3AE_TOKEN_REC_DOUBLES = 5, M3AE_TOKEN_MAX_K = 16 /* the bound on k above */, M3AE_TOKEN_IGNORE = -100 };
int64_t m3ae_token_eval_workspace_bytes(int64_t R, int64_t V, int64_t chunk, int64_t k);
int m3ae_token_eval(const void* logits, int64_t ld, const int64_t* labels, const uint8_t* select, int64_t R, int64_t V, int64_t chunk,
                    int64_t k, int dtype, int64_t* pred, int32_t* rank, float* nll, int32_t* topk_idx, float* topk_prob, double* rec,
                    int64_t* err, void* workspace, int64_t workspace_bytes, void* stream);
int m3ae_record_add(const float* value, double* rec, void* stream);

/* self-test of hardware idioms the kernels rely on (MFMA fragment maps, ds_read_b64_tr_b16, accumulator-as-
 * operand k-order).  out: int32[8 + 256] device buffer (tail = scratch), out[0] = number of mismatches. */
int m3ae_selftest(int32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* M3AE_HIP_H */
