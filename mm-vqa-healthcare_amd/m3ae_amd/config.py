"""Config dict for the hot path: the reference's sacred defaults and named configs as plain dicts.

Mirrors reference m3ae/config.py:18-119 (defaults) and :121-282 (named configs); the model only
ever reads a plain dict (SURVEY.md 5 "Config / flags"), so sacred itself is not needed.  Named configs
compose left to right exactly like on the reference CLI (`... task_finetune_vqa_vqa_rad clip16
text_roberta image_size=384`, run_scripts/finetune_m3ae.sh:18-21); see `compose()` / `parse_cli()`.

Architecture widths that the reference derives from downloaded checkpoints (clip_model.py:277-290,
RobertaModel.from_pretrained) are looked up from the `vit` / `tokenizer` names here (`_ARCH`), and can be
overridden with explicit `vit_width/vit_layers/text_hidden/...` keys (used by the tiny test config).
"""
import ast
import copy


def _loss_names(d):
    ret = {"mlm": 0, "mim": 0, "itm": 0, "vqa": 0, "cls": 0, "irtr": 0}
    ret.update(d)
    return ret


DEFAULTS = dict(
    exp_name="meter", seed=0, datasets=["medicat", "roco"], loss_names=_loss_names({"itm": 1, "mlm": 1}),
    batch_size=4096,
    image_size=224, patch_size=32, draw_false_image=1, image_only=False,
    vqa_label_size=3129, mlc_label_size=14, max_text_len=40, tokenizer="bert-base-uncased", vocab_size=30522,
    whole_word_masking=True, mlm_prob=0.15, draw_false_text=0,
    num_top_layer=6, input_image_embed_size=768, input_text_embed_size=768, vit="ViT-B/32", hidden_size=768,
    num_heads=12, num_layers=6, mlp_ratio=4, drop_rate=0.1,
    mim_prob=0.75, mim_decoder_hidden_size=384, mim_decoder_num_layers=4, mim_decoder_num_heads=6,
    norm_pix_loss=True, mim_layer=-1,
    # the optimizer rule (m3ae_utils.py:203-210): "adamw" | "adam" | "sgd" -- each one fused launch per parameter group over the
    # flat buffers (csrc/misc.hip); config.optim_type validates, ParamStore dispatches.  graph.GraphedStep covers "adamw" only.
    optim_type="adamw", learning_rate=1e-5, weight_decay=0.01, decay_power=1, max_epoch=100, max_steps=-1,
    warmup_steps=10000, end_lr=0, lr_multiplier_head=5, lr_multiplier_multi_modal=5,
    mm_encoder_inputs_include_cls_feats=True, mm_encoder_inputs_include_imagetext_feats=False,
    mm_encoder_inputs_mm_feats_width=0,
    t5_model_name="t5-small", t5_max_length=25, t5_generation=True,
    unfreeze_num_encoder_layers=2, unfreeze_num_decoder_layers=2,
    get_recall_metric=False, resume_from=None, fast_dev_run=False, val_check_interval=1.0, test_only=False,
    default_root_dir="checkpoints", data_root="", log_dir="result", per_gpu_batchsize=0, use_ddp=False,
    num_gpus=1, num_nodes=1, load_path="", decoder_load_path="", load_path_t5="", num_workers=8, precision=32,
    gpu_device_number=0, label_column_name="",
    # build extensions (not in the reference): compute mode of the HIP path
    compute_dtype="bf16",  # "bf16" (perf mode) | "fp32" (parity mode) | "fp32x3" (parity mode's storage, GEMMs on the split-bf16 MFMA)
    # bit-reproducible training steps (ops.set_deterministic): every gradient and loss reduction in a fixed order instead of fp32
    # atomics.  The reference's trainer runs with deterministic=True (main.py:64); here the default is False -- the one deliberate
    # difference from that flag -- because the ordered split-K weight gradients cost step time.
    deterministic=False,
    # where the CLIP transform's bicubic resize + centre crop run for arrow data (m3ae_amd/data.py): "host" (PIL, on the loader's
    # threads) | "device" (csrc/image.hip from the decoded source bytes; bit-identical batches)
    image_transform="host",
    # where the beam-search bookkeeping of the T5 head's generate runs (m3ae_amd/modules/t5.py): "host" (one small copy and a Python
    # loop per step) | "device" (csrc/beam.hip, no host round trip per step; same tokens)
    t5_beam_search="host",
    # where the greedy-search bookkeeping of the decoder head runs (m3ae_amd/modules/m3ae_decoder.py: Decoder.search_path): "host"
    # (ATen argmax / compares / cat and one blocking `finished.all()` per token) | "device" (csrc/greedy.hip, no host round trip per
    # token; same tokens)
    decoder_search="host",
    # how test() scores the generator heads with vqa_metrics="device" (m3ae_amd/trainer.py): "free" (token exact match of the free
    # search alone, as before) | "list" (also answer-list decoding, csrc/answer_trie.hip: greedy search restricted to the answers
    # of Trainer.set_answer_list, scored as labels with the closed / open VQA score).  "free" calls no new entry point.
    answer_decoding="free",
    # answer_decoding="list" only: the beams of the list search (csrc/trie_beam.hip).  1 = the greedy search with the launches it
    # always made; 2 .. 8 = constrained beam search, which also yields the n-best answers test() scores `@k`.
    # answer_length_penalty: hypotheses rank by log-probability / length ** penalty.  0.0 ranks a closed list by the entries'
    # log-probability (with answer_beams >= the list's size the search is exhaustive and the result is the maximum-likelihood
    # entry); 1.0 is HF generate's length-normalised ranking.
    answer_beams=1,
    answer_length_penalty=0.0,
    # answer_decoding="list" only: "search" (the list search above, the launches it always made) | "exhaustive" (every list entry
    # scored in one tree-shaped decoder pass, csrc/tree_attn.hip + csrc/list_score.hip: the list's arg-max, the min(eval_topk, 16)
    # best answers for `@k`, and the mean mass the head puts on the list; answer_beams is then ignored).
    answer_scoring="search",
    # where validation / test compute their metric (m3ae_amd/trainer.py, m3ae_amd/metrics.py): "host" (ATen float / argmax /
    # gather / sum: the overall VQA score alone) | "device" (csrc/vqa_eval.hip: overall, closed and open scores, the score within
    # the top `eval_topk` answers, and token exact match for the generator heads in test()).  eval_topk is honoured only with "device".
    vqa_metrics="host",
    eval_topk=5,
    # what a validation pass of the pre-training objectives reports (m3ae_amd/trainer.py, m3ae_amd/metrics.py): "host" (the monitored
    # negative summed loss alone, as before) | "device" (csrc/token_eval.hip: MLM accuracy, accuracy within the top `eval_topk` tokens
    # and perplexity, ITM accuracy and the mean loss per objective, accumulated on the GPU and read with one copy; the monitored
    # quantity stays what it is).  eval_topk is shared with vqa_metrics and checked with either "device".
    pretrain_metrics="host",
    # arrow VQA batches collated per distinct image (m3ae_amd/data.py: collate_dedup): every distinct image of a batch is decoded,
    # uploaded and run through the image tower once, and ops.expand_samples hands its tokens to the samples that ask about it
    # (batch["image_index"]).  Same samples, same arithmetic per sample; not available with the mim / itm objectives.
    image_dedup=False,
    # dtype of the image tower's residual stream in bf16 mode (m3ae_amd/modules/clip_model.py): "bf16" (the stream is rounded at
    # every join, 2 roundings per block) | "fp32" (stream and its gradient in fp32 from the token assembly to the input of
    # ln_post, as under the reference's autocast, config.py:146 precision=16; every GEMM and attention operand stays bf16).  No
    # effect under compute_dtype "fp32" / "fp32x3", whose stream is fp32 already.  Not available with graph.GraphedStep.
    clip_residual_dtype="bf16",
    # image transform per split (reference config.py:41-42; m3ae_amd/data.py).  Train: "clip" | "clip_resizedcrop"
    # (RandomResizedCrop(size, scale=(0.9, 1.0), BICUBIC) in front of the CLIP tail, transform.py:70-77: one crop box per image
    # and epoch, resample.random_resized_crop_box).  Every other split runs "clip" (base_dataset.py:39-41 strips the suffix).
    train_transform_keys=["clip"], val_transform_keys=["clip"],
    # RandAugment(2, 9) (reference transforms/randaug.py) on every image a train split loads, in front of whichever tail
    # train_transform_keys names; with "clip" it is the reference's `clip_randaug` (transform.py:80-91).  Under image_transform
    # "host" Pillow runs the operations on the loader threads, under "device" csrc/randaug.hip does, on the uploaded source bytes:
    # equal batches (m3ae_amd/randaug.py).  Val / test never augment.  Not available with graph.GraphedStep.
    randaug=False,
    # gradient clipping by global norm (Lightning's Trainer flag, PL 1.3.2 norm clipping; torch.nn.utils.clip_grad_norm_'s rule) with a
    # non-finite step guard: 0.0 = off (the step's launches are what they are without the key) | a bound > 0 | float("inf") = guard
    # only.  The norm is summed in double on the device (csrc/gradnorm.hip) and the factor reaches the AdamW launches through device
    # memory: no host round trip.  A step whose gradient holds an inf or a nan updates nothing and is counted
    # (ParamStore.grad_stats).  Not available with graph.GraphedStep or FlatGradReducer(update_in_backward=True).
    gradient_clip_val=0.0,
    # exponential moving average of the trainable weights (not in the reference; m3ae_amd/param_store.py): ema_decay 0.0 = off (the
    # step's launches are what they are without the key, nothing is allocated) | a float in (0, 1).  One more flat fp32 buffer and
    # one streaming launch per optimizer range (csrc/misc.hip: m3ae_ema_update).  ema_warmup: decay_t = min(ema_decay, (1 + t) /
    # (10 + t)) at the t-th update (1-based), so that a short run is not dominated by its starting point.  ema_eval: validation and
    # test -- and with them the choice of best.ckpt -- run on the averaged weights (ParamStore.ema_weights).  load_ema: `load_path`
    # takes a checkpoint's `ema_state_dict` over its `state_dict`.  Not available with graph.GraphedStep.
    ema_decay=0.0, ema_warmup=True, ema_eval=True, load_ema=False,
    # LoRA fine-tuning in merged form (not in the reference; m3ae_amd/lora.py, csrc/lora.hip): lora_rank 0 = off (a step makes the
    # calls it makes without the key) | 1..64.  The effective weight W0 + (lora_alpha / lora_rank) B A lives in the ordinary weight
    # buffers, so the forward, the backward and every state_dict are what they are; only the adapters and the heads are updated.
    # lora_targets: "all-linear" (every GEMM weight of optimizer groups 0 and 4) | "attention" (the attention projections among
    # them).  lora_lr_multiplier scales the learning rate of the target's group for the adapters; its default follows the usual
    # practice of running adapters an order of magnitude above the full fine-tuning rate -- nobody has tuned it on VQA-RAD here.
    # lora_path: an adapter file (LoraAdapters.state_dict) to load after `load_path`.  Not available with graph.GraphedStep,
    # FlatGradReducer(update_in_backward=True), ema_decay > 0, gradient_clip_val > 0 or the T5 / decoder wrappers.
    lora_rank=0, lora_alpha=16.0, lora_targets="all-linear", lora_lr_multiplier=10.0, lora_path="",
)

NAMED = {
    "task_pretrain_m3ae": dict(
        exp_name="task_pretrain_m3ae", datasets=["medicat", "roco"],
        loss_names=_loss_names({"itm": 1, "mlm": 1, "mim": 1}), batch_size=256, max_epoch=10, max_steps=100000,
        warmup_steps=0.1, whole_word_masking=True, vocab_size=30522, max_text_len=64, image_size=224,
        tokenizer="bert-base-uncased", learning_rate=1e-5, val_check_interval=1.0, lr_multiplier_head=5,
        lr_multiplier_multi_modal=5, num_top_layer=6, hidden_size=768, num_heads=12, precision=16, mim_layer=3),
    "task_finetune_vqa_vqa_rad": dict(
        exp_name="task_finetune_vqa_vqa_rad", datasets=["vqa_vqa_rad"], loss_names=_loss_names({"vqa": 1}),
        batch_size=64, max_epoch=20, max_steps=1000, warmup_steps=0.1, draw_false_image=0, learning_rate=1e-5,
        val_check_interval=1.0, lr_multiplier_head=100, lr_multiplier_multi_modal=5,
        tokenizer="bert-base-uncased", input_text_embed_size=768, vit="ViT-B/32", input_image_embed_size=768,
        image_size=576, vqa_label_size=498, max_text_len=32),
    "task_finetune_vqa_ehr_xqa": dict(
        exp_name="task_finetune_vqa_ehr_xqa", datasets=["vqa_ehr_xqa"], loss_names=_loss_names({"vqa": 1}),
        batch_size=64, max_epoch=50, max_steps=1000, warmup_steps=0.1, draw_false_image=0, learning_rate=5e-6,
        val_check_interval=1.0, lr_multiplier_head=100, lr_multiplier_multi_modal=5,
        tokenizer="bert-base-uncased", input_text_embed_size=768, vit="ViT-B/32", input_image_embed_size=768,
        image_size=576, vqa_label_size=498, max_text_len=32),
    "clip32": dict(vit="ViT-B/32", image_size=224, patch_size=32, input_image_embed_size=768),
    "clip16": dict(vit="ViT-B/16", image_size=224, patch_size=16, input_image_embed_size=768),
    "clip16_large": dict(vit="ViT-L/16", image_size=224, patch_size=16, input_image_embed_size=1024),  # extension
    "text_roberta": dict(tokenizer="roberta-base", vocab_size=50265, input_text_embed_size=768),
    "text_roberta_large": dict(tokenizer="roberta-large", vocab_size=50265, input_text_embed_size=1024),
    "clip_resizedcrop": dict(train_transform_keys=["clip_resizedcrop"]),   # config.py:280-282
}

# widths the reference reads out of downloaded checkpoints
_ARCH_VIT = {
    "ViT-B/32": dict(vit_width=768, vit_layers=12),
    "ViT-B/16": dict(vit_width=768, vit_layers=12),
    "ViT-L/14": dict(vit_width=1024, vit_layers=24),
    "ViT-L/16": dict(vit_width=1024, vit_layers=24),
}
_ARCH_TEXT = {
    "base": dict(text_hidden=768, text_layers=12, text_heads=12, text_inter=3072),
    "large": dict(text_hidden=1024, text_layers=24, text_heads=16, text_inter=4096),
}


CLIP_RESIDUAL_DTYPES = ("bf16", "fp32")


def clip_residual_dtype(cfg):
    """The validated clip_residual_dtype of a config dict (default "bf16")."""
    v = cfg.get("clip_residual_dtype", "bf16")
    if v not in CLIP_RESIDUAL_DTYPES:
        raise ValueError(f"clip_residual_dtype must be one of {CLIP_RESIDUAL_DTYPES}, got {v!r}")
    return v


TRAIN_TRANSFORM_KEYS = ("clip", "clip_resizedcrop")
VAL_TRANSFORM_KEYS = ("clip",)


def transform_keys(cfg):
    """The validated (train, val) transform names of a config dict (defaults "clip").  Each key is a list of one name, as on the
    reference's command line; a split other than train drops the "_resizedcrop" suffix first (base_dataset.py:39-41).  The
    reference's other names are not available: "clip_randaug" is `randaug=True` next to "clip" here, the "imagenet*" keys stay out
    of scope."""
    out = []
    for name, allowed, strip in (("train_transform_keys", TRAIN_TRANSFORM_KEYS, False), ("val_transform_keys", VAL_TRANSFORM_KEYS, True)):
        v = cfg.get(name, ["clip"])
        ok = isinstance(v, (list, tuple)) and len(v) == 1 and isinstance(v[0], str)
        key = v[0].replace("_resizedcrop", "") if ok and strip else (v[0] if ok else None)
        if key not in allowed:
            raise ValueError(f"{name} must be a list of one of {allowed}, got {v!r}")
        out.append(key)
    return tuple(out)


def randaug_enabled(cfg):
    """The validated `randaug` of a config dict (default False).  (n, m) is the reference's (2, 9); no other value is offered."""
    v = cfg.get("randaug", False)
    if not isinstance(v, bool):
        raise ValueError(f"randaug must be True or False, got {v!r}")
    return v


def gradient_clip_val(cfg):
    """The validated `gradient_clip_val` of a config dict (default 0.0 = off) as a float: a number >= 0, or float("inf") -- on the
    command line `gradient_clip_val=inf` -- for the non-finite guard without a bound."""
    v = cfg.get("gradient_clip_val", 0.0)
    if v == "inf":   # the command-line grammar has no literal for it
        v = float("inf")
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v < 0:
        raise ValueError(f'gradient_clip_val must be a number >= 0 (0: off) or float("inf") (guard only), got {v!r}')
    return float(v)


def ema_decay(cfg):
    """The validated `ema_decay` of a config dict (default 0.0 = off) as a float in [0, 1); `ema_warmup`, `ema_eval` and `load_ema`
    next to it must be bools."""
    v = cfg.get("ema_decay", 0.0)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v < 1:
        raise ValueError(f"ema_decay must be a number in [0, 1) (0: off), got {v!r}")
    for key, default in (("ema_warmup", True), ("ema_eval", True), ("load_ema", False)):
        if not isinstance(cfg.get(key, default), bool):
            raise ValueError(f"{key} must be True or False, got {cfg[key]!r}")
    return float(v)


def ema_decay_at(decay, t, warmup=True):
    """decay_t of the t-th EMA update (t = 1, 2, ...): min(decay, (1 + t) / (10 + t)) under `ema_warmup`, else `decay`."""
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def ema_weight(decay, t, warmup=True):
    """w = 1 - decay_t as the float m3ae_ema_update takes: formed in double, rounded to fp32 once (struct round trip).  In fp32
    arithmetic 1.0f - 0.9999f is 3e-4 relative off 1e-4, and the average would carry that."""
    import struct
    return struct.unpack("f", struct.pack("f", 1.0 - ema_decay_at(decay, t, warmup)))[0]


LORA_TARGETS = ("all-linear", "attention")
LORA_MAX_RANK = 64


def lora_rank(cfg):
    """The validated `lora_rank` of a config dict (default 0 = off): an int in [0, 64].  The keys next to it are checked with it:
    `lora_alpha` and `lora_lr_multiplier` finite numbers > 0, `lora_targets` one of LORA_TARGETS, `lora_path` a string."""
    v = cfg.get("lora_rank", 0)
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= LORA_MAX_RANK:
        raise ValueError(f"lora_rank must be an integer in [0, {LORA_MAX_RANK}] (0: off), got {v!r}")
    for key, default in (("lora_alpha", 16.0), ("lora_lr_multiplier", 10.0)):
        x = cfg.get(key, default)
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0 < x < float("inf"):
            raise ValueError(f"{key} must be a finite number > 0, got {x!r}")
    tg = cfg.get("lora_targets", "all-linear")
    if not isinstance(tg, str) or tg not in LORA_TARGETS:
        raise ValueError(f"lora_targets must be one of {LORA_TARGETS}, got {tg!r}")
    if not isinstance(cfg.get("lora_path", ""), str):
        raise ValueError(f"lora_path must be a string, got {cfg['lora_path']!r}")
    return v


DECODER_SEARCHES = ("host", "device")


def decoder_search(cfg):
    """The validated `decoder_search` of a config dict (default "host")."""
    v = cfg.get("decoder_search", "host")
    if not isinstance(v, str) or v not in DECODER_SEARCHES:
        raise ValueError(f"decoder_search must be one of {DECODER_SEARCHES}, got {v!r}")
    return v


ANSWER_DECODINGS = ("free", "list")


def answer_decoding(cfg):
    """The validated `answer_decoding` of a config dict (default "free")."""
    v = cfg.get("answer_decoding", "free")
    if not isinstance(v, str) or v not in ANSWER_DECODINGS:
        raise ValueError(f"answer_decoding must be one of {ANSWER_DECODINGS}, got {v!r}")
    return v


ANSWER_MAX_BEAMS = 8


def answer_beams(cfg):
    """The validated (`answer_beams`, `answer_length_penalty`) of a config dict (defaults 1 and 0.0): an int in [1, 8] and a finite
    number.  Read under answer_decoding="list" only, checked always."""
    nb = cfg.get("answer_beams", 1)
    if isinstance(nb, bool) or not isinstance(nb, int) or not 1 <= nb <= ANSWER_MAX_BEAMS:
        raise ValueError(f"answer_beams must be an integer in [1, {ANSWER_MAX_BEAMS}], got {nb!r}")
    lp = cfg.get("answer_length_penalty", 0.0)
    if isinstance(lp, bool) or not isinstance(lp, (int, float)) or lp != lp or lp in (float("inf"), float("-inf")):
        raise ValueError(f"answer_length_penalty must be a finite number, got {lp!r}")
    return nb, float(lp)


ANSWER_SCORINGS = ("search", "exhaustive")


def answer_scoring(cfg):
    """The validated `answer_scoring` of a config dict (default "search": the list search of `answer_beams`).  "exhaustive" scores
    every list entry in one tree-shaped decoder pass instead (csrc/list_score.hip).  Read under answer_decoding="list" only,
    checked always."""
    v = cfg.get("answer_scoring", "search")
    if not isinstance(v, str) or v not in ANSWER_SCORINGS:
        raise ValueError(f"answer_scoring must be one of {ANSWER_SCORINGS}, got {v!r}")
    return v


VQA_METRICS = ("host", "device")


def vqa_metrics(cfg):
    """The validated `vqa_metrics` of a config dict (default "host"); with "device", `eval_topk` must be an int in [0, 16]."""
    v = cfg.get("vqa_metrics", "host")
    if not isinstance(v, str) or v not in VQA_METRICS:
        raise ValueError(f"vqa_metrics must be one of {VQA_METRICS}, got {v!r}")
    k = cfg.get("eval_topk", 5)
    if v == "device" and (isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 16):
        raise ValueError(f"eval_topk must be an integer in [0, 16] with vqa_metrics='device', got {k!r}")
    return v


PRETRAIN_METRICS = ("host", "device")


def pretrain_metrics(cfg):
    """The validated `pretrain_metrics` of a config dict (default "host"); with "device", `eval_topk` must be an int in [0, 16]."""
    v = cfg.get("pretrain_metrics", "host")
    if not isinstance(v, str) or v not in PRETRAIN_METRICS:
        raise ValueError(f"pretrain_metrics must be one of {PRETRAIN_METRICS}, got {v!r}")
    k = cfg.get("eval_topk", 5)
    if v == "device" and (isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 16):
        raise ValueError(f"eval_topk must be an integer in [0, 16] with pretrain_metrics='device', got {k!r}")
    return v


OPTIM_TYPES = ("adamw", "adam", "sgd")


def optim_type(cfg):
    """The validated `optim_type` of a config dict (default "adamw"): the optimizer rule, as the reference's set_schedule builds it
    (m3ae_utils.py:203-210) -- "adamw" = HF AdamW(betas=(0.9, 0.98), eps=1e-8), "adam" = torch.optim.Adam, "sgd" =
    torch.optim.SGD(momentum=0.9).  The names are case-sensitive there too; anything else is a ValueError."""
    v = cfg.get("optim_type", "adamw")
    if not isinstance(v, str) or v not in OPTIM_TYPES:
        raise ValueError(f"optim_type must be one of {OPTIM_TYPES}, got {v!r}")
    return v


def resolve_arch(cfg):
    """Fill vit_width/vit_layers/text_* from the `vit` / `tokenizer` names unless given explicitly."""
    cfg = dict(cfg)
    optim_type(cfg)
    decoder_search(cfg)
    answer_decoding(cfg)
    answer_beams(cfg)
    answer_scoring(cfg)
    vqa_metrics(cfg)
    pretrain_metrics(cfg)
    if "gradient_clip_val" in cfg:
        cfg["gradient_clip_val"] = gradient_clip_val(cfg)
    if "ema_decay" in cfg:
        cfg["ema_decay"] = ema_decay(cfg)
    else:
        ema_decay(cfg)
    lora_rank(cfg)
    for key in ("lora_alpha", "lora_lr_multiplier"):
        if key in cfg:
            cfg[key] = float(cfg[key])
    clip_residual_dtype(cfg)
    transform_keys(cfg)
    randaug_enabled(cfg)
    vit = _ARCH_VIT.get(cfg["vit"], _ARCH_VIT["ViT-B/16"])
    for k, v in vit.items():
        cfg.setdefault(k, v)
    text = _ARCH_TEXT["large" if "large" in cfg["tokenizer"] else "base"]
    for k, v in text.items():
        cfg.setdefault(k, v)
    cfg.setdefault("text_max_pos", 514 if "roberta" in cfg["tokenizer"] else 512)
    return cfg


def compose(*parts, **overrides):
    """compose("task_finetune_vqa_vqa_rad", "clip16", "text_roberta", image_size=384)."""
    cfg = copy.deepcopy(DEFAULTS)
    for p in parts:
        cfg.update(copy.deepcopy(NAMED[p]) if isinstance(p, str) else p)
    cfg.update(overrides)
    return resolve_arch(cfg)


def parse_cli(argv):
    """Parse the sacred grammar of run_scripts/*.sh: `with k=v ... named_config ... k=v`.  As in sacred, named configs
    apply first (left to right) and explicit `k=v` updates win over them wherever they stand on the command line
    (finetune_m3ae.sh passes `max_epoch=70` BEFORE `task_finetune_vqa_vqa_rad`, whose own max_epoch is 20)."""
    args = [a for a in argv if a != "with"]
    cfg = copy.deepcopy(DEFAULTS)
    for a in args:
        if "=" not in a:
            if a not in NAMED:
                raise KeyError(f"unknown named config {a!r}")
            cfg.update(copy.deepcopy(NAMED[a]))
    for a in args:
        if "=" in a:
            k, v = a.split("=", 1)
            try:
                v = ast.literal_eval(v)
            except (ValueError, SyntaxError):
                pass
            cfg[k] = v
    return resolve_arch(cfg)


def finetune_vqa_rad_config(**over):
    """The effective config of run_scripts/test_m3ae.sh / finetune_m3ae.sh (BASELINE configs[0..2])."""
    return compose("task_finetune_vqa_vqa_rad", "clip16", "text_roberta", image_size=384, **over)


def tiny_config(**over):
    """Reduced-size model of the same architecture used by the golden fixtures (oracle/make_golden.py TINY)."""
    base = dict(image_size=64, hidden_size=128, num_heads=2, num_top_layer=2, input_image_embed_size=128,
                input_text_embed_size=128, vocab_size=1000, vit_width=128, vit_layers=3, text_hidden=128,
                text_layers=2, text_heads=2, text_inter=512)
    base.update(over)
    return compose("task_finetune_vqa_vqa_rad", "clip16", "text_roberta", **base)
