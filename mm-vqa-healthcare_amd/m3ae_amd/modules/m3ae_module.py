"""M3AETransformerSS on MI355X -- the drop-in boundary of the hot path.

Same constructor (`M3AETransformerSS(config: dict)`), same `infer()` / `forward()` / `training_step()` contract,
same module tree and state_dict key names / shapes as the reference's m3ae/modules/m3ae_module.py:16-373, so
`load_state_dict(ckpt["state_dict"], strict=False)` of an upstream M3AE checkpoint works and the generator wrappers
(`self.m3ae.infer(batch)`, m3ae_t5_mm_encoder_input.py:102) are served unchanged.  Below the modules every FLOP
runs in hand-written gfx950 kernels (libm3ae_hip.so) -- there is no PyTorch-op fallback.

Differences that are deliberate: weights are never downloaded (architecture comes from the config);
`finalize(device)` moves the parameters into the flat MI355X layout (ParamStore) and must be called before the
first forward; attention probabilities are not materialised unless `infer(..., output_attentions=True)` asks for the
fusion layers' maps (fp32 [B, H, Lq, Lk], detached: the reference's gradient hook on them is disabled); dropout
(`module.training`, RoBERTa p = 0.1, fusion layers p = `drop_rate`) uses the library's counter-hash masks fused into
the kernels (seeded by `ops.set_dropout_seed`), not torch's Philox stream.
"""
import math
import os

import torch
import torch.nn as nn

from .. import ops
from ..config import clip_residual_dtype, resolve_arch
from ..param_store import ParamStore
from . import objectives, prediction_heads
from .bert_model import BertCrossLayer, RobertaModel
from .clip_model import adapt_position_encoding, build_model

class _JoinAtEndFn(ops.Function):
    """Identity.  Its backward (among the first nodes of a backward pass) queues `main.wait_stream(side)` to run when the pass ends."""

    @staticmethod
    def forward(ctx, x, main, side):
        ctx.streams = (main, side)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        main, side = ctx.streams

        def join():
            # the in-place weight gradients are invisible to autograd's own end-of-backward synchronisation: whoever reads
            # store.grad next does so on the stream that is current NOW (normally `main`; it may differ from the forward's)
            main.wait_stream(side)
            cur = torch.cuda.current_stream()
            if cur != main:
                cur.wait_stream(main)
                cur.wait_stream(side)

        torch.autograd.Variable._execution_engine.queue_callback(join)
        return g, None, None


try:  # drop-in for pl.Trainer when Lightning is installed on the user's side
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    pl = None
    _Base = nn.Module


class _HParams(dict):
    __getattr__ = dict.__getitem__


def init_weights(module):
    """m3ae_utils.py:101-109."""
    if isinstance(module, (nn.Linear, nn.Embedding)):
        module.weight.data.normal_(mean=0.0, std=0.02)
    elif isinstance(module, nn.LayerNorm):
        module.bias.data.zero_()
        module.weight.data.fill_(1.0)
    if isinstance(module, nn.Linear) and module.bias is not None:
        module.bias.data.zero_()


def answers_of(labels, probs, label2ans):
    """Rows of label ids and probabilities -> rows of (answer, probability) through label2ans[str(label)]."""
    out = []
    for ls, ps in zip(labels, probs):
        row = []
        for l, p in zip(ls, ps):
            key = str(int(l))
            if key not in label2ans:
                raise KeyError(f"label {key} is not in label2ans ({len(label2ans)} answers)")
            row.append((label2ans[key], float(p)))
        out.append(row)
    return out


class M3AETransformerSS(_Base):
    def __init__(self, config):
        super().__init__()
        config = resolve_arch(config)
        if pl is None:
            self.hparams = _HParams(config=config)
        else:
            self.save_hyperparameters()
        cfg = config
        hs = cfg["hidden_size"]
        self.is_clip = "swin" not in cfg["vit"]
        if not self.is_clip:
            raise NotImplementedError("swin backbones are unreachable in the reference (SURVEY 2 #14)")
        # == 1. Build Models (m3ae_module.py:21-89) ==
        self.vision_encoder = build_model(cfg["vit"], resolution_after=cfg["image_size"], vision_width=cfg["vit_width"],
                                          vision_layers=cfg["vit_layers"], patch_size=cfg["patch_size"],
                                          residual_dtype=clip_residual_dtype(cfg))
        self.language_encoder = RobertaModel(cfg["vocab_size"], cfg["text_hidden"], cfg["text_layers"],
                                             cfg["text_heads"], cfg["text_inter"], cfg["text_max_pos"])
        self.multi_modal_language_proj = nn.Linear(cfg["input_text_embed_size"], hs)
        self.multi_modal_vision_proj = nn.Linear(cfg["input_image_embed_size"], hs)
        self.modality_type_embeddings = nn.Embedding(2, hs)
        inter = hs * cfg["mlp_ratio"]
        self.multi_modal_vision_layers = nn.ModuleList(
            [BertCrossLayer(hs, cfg["num_heads"], inter, drop_rate=cfg["drop_rate"]) for _ in range(cfg["num_top_layer"])])
        self.multi_modal_language_layers = nn.ModuleList(
            [BertCrossLayer(hs, cfg["num_heads"], inter, drop_rate=cfg["drop_rate"]) for _ in range(cfg["num_top_layer"])])
        self.multi_modal_vision_pooler = prediction_heads.Pooler(hs)
        self.multi_modal_language_pooler = prediction_heads.Pooler(hs)
        for m in (self.multi_modal_language_proj, self.multi_modal_vision_proj, self.modality_type_embeddings,
                  self.multi_modal_vision_layers, self.multi_modal_language_layers, self.multi_modal_vision_pooler,
                  self.multi_modal_language_pooler):
            m.apply(init_weights)
        # == 2. Pre-training heads (m3ae_module.py:91-101) ==
        if cfg["loss_names"]["mlm"] > 0:
            self.mlm_head = prediction_heads.MLMHead(hs, cfg["vocab_size"])
            self.mlm_head.apply(init_weights)
        if cfg["loss_names"]["mim"] > 0:
            self.mim_head = prediction_heads.MIMHead(cfg)
            self.mim_head.apply(init_weights)
        if cfg["loss_names"]["itm"] > 0 or cfg["loss_names"]["irtr"] > 0:
            self.itm_head = prediction_heads.ITMHead(hs * 2)
            self.itm_head.apply(init_weights)
        # == 3. Load (m3ae_module.py:103-114) ==
        if cfg["load_path"] != "" and not cfg["test_only"]:
            self._load(cfg["load_path"])
        # == 4. Downstream heads (m3ae_module.py:116-126) ==
        if cfg["loss_names"]["vqa"] > 0:
            vs = cfg["vqa_label_size"]
            self.vqa_head = nn.Sequential(nn.Linear(hs * 2, hs * 2), nn.LayerNorm(hs * 2), nn.GELU(),
                                          nn.Linear(hs * 2, vs))
            self.vqa_head.apply(init_weights)
        self.current_tasks = list()
        # == 5. Load for testing (m3ae_module.py:132-142) ==
        if cfg["load_path"] != "" and cfg["test_only"]:
            self._load(cfg["load_path"])
        self.store = None
        self.lora = None      # lora.LoraAdapters once attach_lora() has run (cfg["lora_rank"] > 0), else None
        self._dtype = torch.bfloat16 if cfg.get("compute_dtype", "bf16") == "bf16" else torch.float32
        self._x3 = cfg.get("compute_dtype") == "fp32x3"   # fp32x3 mode: fp32 storage, fp32 GEMMs on the split-bf16 MFMA kernel
        # deterministic=True (the reference trainer's flag, main.py:64): ordered reductions in every backward from here on.  The
        # switch is process-wide (ops.set_deterministic), as the reference's is; ops.set_deterministic(False) takes it back.
        if cfg.get("deterministic", False):
            ops.set_deterministic(True)

    @property
    def f32x3(self):
        """True in fp32x3 mode (compute_dtype="fp32x3"): parity mode's storage, every GEMM and attention product on the
        fp32-accurate MFMA kernel (ops.f32x3_mode)."""
        return self._x3 and self._dtype == torch.float32

    def set_compute_dtype(self, compute_dtype):
        """"bf16" | "fp32" | "fp32x3", or a torch dtype (which keeps the configured fp32x3 choice for float32)."""
        if isinstance(compute_dtype, str):
            self._x3 = compute_dtype == "fp32x3"
            compute_dtype = torch.bfloat16 if compute_dtype == "bf16" else torch.float32
        self._dtype = compute_dtype

    # ------------------------------------------------------------------------------------------------------
    def _load(self, path):
        # upstream checkpoints are Lightning pickles (callbacks / hyper_parameters hold class globals): the weights-only
        # unpickler of torch >= 2.6 rejects them, as it would for the reference's own torch.load (m3ae_module.py:105)
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        weights = ckpt["state_dict"]
        if self.hparams.config.get("load_ema", False):
            # config key `load_ema`: the averaged weights of a run with ema_decay > 0 (trainer.Trainer.save) over the raw ones; the
            # average has the trainable parameters only, everything else (frozen weights, buffers) comes from state_dict
            if ckpt.get("ema_state_dict") is None:
                raise ValueError(f"load_ema=True, but {path} has no ema_state_dict (it was not written by a run with ema_decay > 0)")
            weights = dict(weights, **ckpt["ema_state_dict"])
        sd = adapt_position_encoding(weights, after=self.hparams.config["image_size"],
                                     patch_size=self.hparams.config["patch_size"])
        self.load_state_dict(sd, strict=False)
        if getattr(self, "store", None) is not None:   # also reachable from __init__ (load_path), before finalize()
            self.store.sync_shadows()

    def weight_units(self):
        u = self.vision_encoder.weight_units() + self.language_encoder.weight_units()
        u += [self.multi_modal_language_proj.weight, self.multi_modal_vision_proj.weight]
        for l in list(self.multi_modal_vision_layers) + list(self.multi_modal_language_layers):
            u += l.weight_units()
        u += self.multi_modal_vision_pooler.weight_units() + self.multi_modal_language_pooler.weight_units()
        for name in ("mlm_head", "mim_head", "itm_head"):
            if hasattr(self, name):
                u += getattr(self, name).weight_units()
        if hasattr(self, "vqa_head"):
            u += [self.vqa_head[0].weight, self.vqa_head[3].weight]
        return u

    def finalize(self, device="cuda", compute_dtype=None, frozen=()):
        """Move parameters into the flat MI355X layout (ParamStore).  Call once, after loading weights."""
        if compute_dtype is not None:
            self.set_compute_dtype(compute_dtype)
        for b_name, b in list(self.named_buffers()):
            b.data = b.data.to(device)
        self.store = ParamStore(self, self.hparams.config, device, self._dtype, self.weight_units, frozen=frozen)
        return self

    def attach_lora(self, path=""):
        """Attach LoRA adapters per the config (lora_rank > 0), after finalize() and after the base weights are loaded: the weights
        as they stand become the base.  `path`: an adapter file (LoraAdapters.state_dict) to load onto it.  Returns the adapters."""
        from ..lora import LoraAdapters
        if self.store is None:
            raise RuntimeError("attach_lora() needs the flat layout: call finalize() first")
        self.lora = LoraAdapters(self.store, self, self.hparams.config)
        if path:
            self.lora.load_state_dict(torch.load(path, map_location="cpu", weights_only=False))
        else:
            self.lora.merge()
        return self.lora

    # ------------------------------------------------------------------------------------------------------
    two_streams = os.environ.get("M3AE_TWO_STREAMS", "1") == "1"   # M3AE_TWO_STREAMS=0: everything on the caller's stream
    _side_stream = None

    def _side(self):
        if self._side_stream is None:
            # default priority (a high-priority side stream measured the same in round 3; M3AE_SIDE_STREAM_PRIORITY: A/B runs only)
            prio = os.environ.get("M3AE_SIDE_STREAM_PRIORITY")
            self._side_stream = torch.cuda.Stream() if prio is None else torch.cuda.Stream(priority=int(prio))
            # gradients of directly-used leaves (e.g. the modality type embeddings) arrive from nodes of either stream: intended
            warn_off = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
            if warn_off is not None:
                warn_off(False)
        return self._side_stream

    @staticmethod
    def _collect_attention(out, attns, summ, side_key):
        """Splits a fusion layer's result (output, [self map, cross map], [self recv, cross recv]) and files the extras."""
        if attns is None and summ is None:
            return out
        out, *extra = out
        if attns is not None:
            attns[f"{side_key}_attns"].append(tuple(extra[:2]))
            extra = extra[2:]
        if summ is not None:
            summ[side_key].append(tuple(extra))
        return out

    def _fusion_two_streams(self, text_tower, v, mt, mv, mask_image, ret, main, side, ev_inputs, attns=None, live=False,
                            summ=None):
        """The text tower and the text half of every fusion layer on a second HIP stream.  The towers are independent until the
        fusion layers and a fusion layer's two halves read only the PREVIOUS layer's outputs, so the short text-side kernels
        (B*32 rows: half-empty grids) fill the tail rounds of the image-side launches instead of running alone.  Events order
        the hand-overs; `record_stream` keeps the caching allocator from recycling a tensor while the other stream still reads
        it.  autograd runs every node's backward on the stream of its forward and inserts the same hand-overs in reverse."""
        side.wait_event(ev_inputs)
        mt.record_stream(side)
        self.store.streams.update((main, side))
        with torch.cuda.stream(side):
            x = text_tower()
            ev_x = side.record_event()
        y = v
        ev_y = main.record_event()
        for layer_idx, (text_layer, image_layer) in enumerate(zip(self.multi_modal_language_layers,
                                                                  self.multi_modal_vision_layers)):
            if mask_image and self.hparams.config["mim_layer"] == layer_idx:
                ret[f"multi_modal_text_feats_{layer_idx}"], ret[f"multi_modal_image_feats_{layer_idx}"] = x, y
            # x and y each feed both layers of the pair: forked on the stream that produced them, so the two gradients are joined
            # there by the library's add (ops.Fork2Fn)
            with torch.cuda.stream(side):
                xa, xb = ops.fork2(x)
            ya, yb = ops.fork2(y)
            side.wait_event(ev_y)
            y.record_stream(side)
            last = live and layer_idx == len(self.multi_modal_language_layers) - 1   # (live: token 0 of the last pair only)
            with torch.cuda.stream(side):
                x1 = text_layer(xa, yb, mt, mv, output_attentions=attns is not None, cls_only=last,
                                output_attention_summary=summ is not None)
                ev_x1 = side.record_event()
            main.wait_event(ev_x)
            x.record_stream(main)
            y1 = image_layer(ya, xb, mv, mt, output_attentions=attns is not None, cls_only=last,
                             output_attention_summary=summ is not None)
            # (the layers' reference-shaped tuples: output, self-attention map, cross-attention map; then the two summaries)
            x1 = self._collect_attention(x1, attns, summ, "text2image")
            y1 = self._collect_attention(y1, attns, summ, "image2text")
            ev_y = main.record_event()
            x, y, ev_x = x1, y1, ev_x1
        main.wait_event(ev_x)
        x.record_stream(main)
        # the text maps and summaries were written on the side stream: ordered before ev_x, handed to the caller's stream
        for pairs in ((attns["text2image_attns"] if attns is not None else ()), (summ["text2image"] if summ is not None else ())):
            for p in pairs:
                for t in p:
                    t.record_stream(main)
        if torch.is_grad_enabled():
            # whichever of the two runs in backward queues the end-of-backward join: when loss.backward() returns, the caller's
            # stream has waited for the side stream (the weight gradients land in the flat buffer as side effects of the nodes,
            # not as autograd outputs, so the engine's own end-of-backward synchronisation does not cover them)
            x, y = _JoinAtEndFn.apply(x, main, side), _JoinAtEndFn.apply(y, main, side)
        return x, y

    def random_masking(self, x, mask_ratio, noise=None):
        """m3ae_module.py:153-183.  The argsort / argsort-of-argsort / gather-of-ones bookkeeping is one kernel
        (`m3ae_mask_ranks`: ranks by counting); the row gather and its gradient run in the library too."""
        B, Lp1, D = x.shape
        L = Lp1 - 1
        len_keep = int(L * (1 - mask_ratio))
        if noise is None:
            noise = torch.rand(B, L, device=x.device)
        ids_restore, keep_rows, mask = ops.mask_ranks(noise, len_keep)
        pos = self.vision_encoder.visual.positional_embedding
        xp = x + pos.to(x.dtype)  # x + pos, cls row included (m3ae_module.py:169,180); pretrain-only glue
        # keep_rows: per sample the class row and len_keep patches of distinct rank, a slice of a permutation of the token rows
        x_masked = ops.gather_rows(xp, keep_rows, unique=True).view(B, len_keep + 1, D)
        return x_masked, mask, ids_restore

    def patchify(self, imgs):
        """m3ae_module.py:185-192 (`m3ae_mim_targets` without the standardisation)."""
        return ops.mim_targets(imgs, self.hparams.config["patch_size"], False)

    @staticmethod
    def _image_groups(batch, img, n_samples):
        """The index tables of a batch with `image_index` (ops.ImageGroups on the image's device).  A datamodule batch brings them
        in `batch["image_groups"]`, uploaded from pinned memory with the batch: no host call here.  A hand-built batch without
        them pays ONE blocking copy of a device `image_index` to the host, where the tables are built (ops.image_groups)."""
        groups = batch.get("image_groups")
        if groups is None:
            groups = ops.image_groups(batch["image_index"].cpu(), n_images=img.shape[0])
        if groups.index.device != img.device:
            groups = groups.to(img.device)
        if groups.n_images != img.shape[0]:
            raise ValueError(f'batch["image_groups"] is for {groups.n_images} images, batch["image"][0] has {img.shape[0]} rows')
        if groups.n_samples != n_samples:
            raise ValueError(f'batch["image_index"] has {groups.n_samples} entries for {n_samples} samples')
        return groups

    @ops.model_mode
    def infer(self, batch, mask_text=False, mask_image=False, image_token_type_idx=1, img=None,
              output_attentions=False, unimodal=False, cls_only=False, output_attention_summary=False):
        """m3ae_module.py:203-312.  With `batch["image_index"]` (int64 [B]) the image tensor holds one row per DISTINCT image
        ([U, 3, H, W], U <= B, every row used): the tower runs on the U images and `ops.expand_samples` hands sample b the tokens
        of image image_index[b] before the fusion layers; image_index == arange(B) is the path without the key.  cls_only: the caller reads `multi_modal_cls_feats` alone (the VQA and ITM heads): the last fusion
        pair then computes only its token-0 rows (ops.CLS_ONLY) and the two full-sequence feature entries are left out of the
        result.  Attention maps (output_attentions) and deterministic mode keep the full computation.
        output_attention_summary: ret["attention_summary"] = {"text2image": [(self_recv, cross_recv) per fusion layer],
        "image2text": [...]}, the received attention of every map of ret["attentions"] -- its mean over heads and queries, fp32
        [B, Lk], contiguous, detached, per sample (after the expansion of a de-duplicated batch) -- formed without the maps
        (ops.attn_colmean, ops.xattn_colmean).  Like the maps it keeps the full computation; both flags may be set."""
        if self.store is None:
            raise RuntimeError("call finalize(device) before the first forward")
        ret = dict()
        dedup = batch.get("image_index") is not None
        if dedup and (mask_image or img is not None):
            raise ValueError('batch["image_index"] (one image row per DISTINCT image) cannot be combined with '
                             f'{"mask_image=True" if mask_image else "an explicit img= argument"}: that path reads the image '
                             'pixels per sample; pass the expanded [B, 3, H, W] images without the key')
        if img is None:
            img_key = f"image_{image_token_type_idx - 1}" if f"image_{image_token_type_idx - 1}" in batch else "image"
            img = batch[img_key][0]
        do_mlm = "_mlm" if mask_text else ""
        text_ids = batch[f"text_ids{do_mlm}"]
        groups = self._image_groups(batch, img, text_ids.shape[0]) if dedup else None
        text_labels = batch[f"text_labels{do_mlm}"]
        text_masks = batch["text_masks"]
        dt = self._dtype
        H = self.hparams.config["num_heads"]
        type_emb = self.modality_type_embeddings.weight
        mt = self.language_encoder.get_extended_attention_mask(text_masks).contiguous()
        ev_inputs = None
        if self.two_streams and img.is_cuda:   # the text tower (side stream) may start as soon as the inputs are there
            ev_inputs = torch.cuda.current_stream().record_event()
        # == Image Encoding (m3ae_module.py:238-256) ==
        if mask_image:
            v = self.vision_encoder.forward_patch_embed(img, dt)
            v, mim_masks, mim_ids_restore = self.random_masking(v, self.hparams.config["mim_prob"],
                                                                batch.get("mim_noise"))
            v = self.vision_encoder.forward_trans(v, dt)
            ret["mim_masks"], ret["mim_ids_restore"] = mim_masks, mim_ids_restore
        else:
            v = self.vision_encoder(img, dt)
        v = ops.linear(v, self.multi_modal_vision_proj.weight, self.multi_modal_vision_proj.bias,
                       extra_bias=type_emb[image_token_type_idx])
        if groups is not None and not groups.identity:
            # the tower and the projection ran on the U distinct images: [U, L, D] -> [B, L, D] on this (the image-side) stream,
            # before the fusion layers; one autograd node, whose backward adds the samples' gradients per image in a fixed order
            v = ops.expand_samples(v, groups)
        # == Text Encoding (m3ae_module.py:229-236) ==
        # The two towers are independent until the fusion layers.  The reference runs the text tower first; here it runs SECOND, so
        # that autograd (latest-created nodes first) runs its short backward FIRST: the 154-MB word-embedding gradient is then
        # complete ~5 % into backward and its all-reduce overlaps the image tower's backward, and the last gradients of the step
        # are the image tower's first parameters -- the small tail bucket of ddp.FlatGradReducer.  Same values either way (only the
        # order in which the dropout sites draw their seeds changes).
        side = self._side() if (self.two_streams and img.is_cuda) else None
        main = torch.cuda.current_stream() if side is not None else None
        mv = None  # all-ones image mask -> additive zeros (m3ae_module.py:253-256)

        def text_tower():
            if side is not None:
                text_ids.record_stream(side)
            t = self.language_encoder.embeddings(text_ids, dt)
            for layer in self.language_encoder.encoder.layer:
                t = layer(t, mt)
            # projection + modality type embedding (m3ae_module.py:235,260-263): the type row rides in the GEMM bias
            return ops.linear(t, self.multi_modal_language_proj.weight, self.multi_modal_language_proj.bias,
                              extra_bias=type_emb[0])

        # m3ae_module.py:266,280-283: per fusion layer the (self, cross) attention maps of each direction
        attns = {"text2image_attns": [], "image2text_attns": []} if output_attentions else None
        summ = {"text2image": [], "image2text": []} if output_attention_summary else None
        live = (bool(cls_only) and ops.CLS_ONLY and not output_attentions and not output_attention_summary
                and not ops.deterministic())
        n_fusion = len(self.multi_modal_language_layers)
        if side is None:
            t = text_tower()
            # == Multi-Modal Fusion (m3ae_module.py:266-285): both streams read the PRE-update x, y ==
            x, y = t, v
            for layer_idx, (text_layer, image_layer) in enumerate(zip(self.multi_modal_language_layers,
                                                                      self.multi_modal_vision_layers)):
                if mask_image and self.hparams.config["mim_layer"] == layer_idx:
                    ret[f"multi_modal_text_feats_{layer_idx}"], ret[f"multi_modal_image_feats_{layer_idx}"] = x, y
                (xa, xb), (ya, yb) = ops.fork2(x), ops.fork2(y)
                last = live and layer_idx == n_fusion - 1
                x1 = text_layer(xa, yb, mt, mv, output_attentions=output_attentions, cls_only=last,
                                output_attention_summary=output_attention_summary)
                y1 = image_layer(ya, xb, mv, mt, output_attentions=output_attentions, cls_only=last,
                                 output_attention_summary=output_attention_summary)
                x = self._collect_attention(x1, attns, summ, "text2image")
                y = self._collect_attention(y1, attns, summ, "image2text")
        else:
            x, y = self._fusion_two_streams(text_tower, v, mt, mv, mask_image, ret, main, side, ev_inputs, attns, live, summ)
        # == Output (m3ae_module.py:287-297) ==
        cls_t = self.multi_modal_language_pooler(x)
        cls_v = self.multi_modal_vision_pooler(y)
        cls = torch.cat([cls_t, cls_v], dim=-1)
        ret.update({
            "images": img,
            "text_labels": text_labels,
            "text_ids": text_ids,
            "text_masks": text_masks,
            "extended_image_masks": mv,
            "extended_text_masks": mt,
            "multi_modal_cls_feats": cls,
        })
        if dedup:   # ("images" stays the [U, 3, H, W] tensor that was passed in)
            ret["image_index"] = batch["image_index"]
        if not live:   # (live: x and y are the token-0 rows alone; a consumer that needs the sequences fails on the missing key)
            ret["multi_modal_text_feats"], ret["multi_modal_image_feats"] = x, y
        if mask_image:  # only MIM needs it (the reference recomputes it on every call, m3ae_module.py:301)
            ret["patched_images"] = self.patchify(img)
        ret["attentions"] = attns
        if summ is not None:
            ret["attention_summary"] = summ
        return ret

    HEATMAP_SOURCES = {"image_self": ("image2text", 0), "text2image": ("text2image", 1)}

    @staticmethod
    def heatmap_images(batch):
        """The images attention_heatmaps(batch) lies over: infer's ret["images"] for image_token_type_idx = 1."""
        return batch["image_0" if "image_0" in batch else "image"][0]

    def attention_heatmaps(self, batch, layer=-1, which="image_self", size=None):
        """Per-sample attention heatmaps over the image, fp32 [B, size, size] on the device (size: config["image_size"] by
        default): the received attention of the image patches in fusion layer `layer`, class token dropped, as the g x g patch
        grid, upsampled bilinearly (align_corners=False) -- what the reference's DecoderModel.visualize_attention_heatmap
        (m3ae_decoder.py:225-290) computes from a full attention map before it plots.
        which = "image_self": the reference's choice, the image layer's self-attention (image2text[layer][0]) -- how much attention
        each patch receives from the image tokens; "text2image": the text layer's cross-attention (text2image[layer][1]) -- how
        much the question's tokens attend to each patch.  One infer under no_grad with output_attention_summary; no map is formed."""
        if which not in self.HEATMAP_SOURCES:
            raise ValueError(f"which={which!r}: expected one of {sorted(self.HEATMAP_SOURCES)}")
        cfg = self.hparams.config
        img = self.heatmap_images(batch)
        # I - 1: the image tokens without the class token, known before anything runs
        tokens = (img.shape[-2] // cfg["patch_size"]) * (img.shape[-1] // cfg["patch_size"])
        g = math.isqrt(tokens)
        if g * g != tokens:
            raise ValueError(f"{tokens} image patches (I - 1) are not a square grid: no heatmap")
        size = cfg["image_size"] if size is None else int(size)
        if size < 1:
            raise ValueError(f"size={size}")
        with torch.no_grad():
            ret = self.infer(batch, output_attention_summary=True)
        side, idx = self.HEATMAP_SOURCES[which]
        recv = ret["attention_summary"][side][layer][idx]
        if recv.shape[1] != tokens + 1:
            raise ValueError(f"the summary has {recv.shape[1]} image tokens, expected 1 + {tokens}")
        return ops.heatmap_upsample(recv[:, 1:], size)

    def vqa_head_forward(self, cls):
        """m3ae_module.py:120-125: Linear -> LayerNorm -> GELU (fused into the LN kernel) -> Linear."""
        h = ops.linear(cls, self.vqa_head[0].weight, self.vqa_head[0].bias)
        ln = self.vqa_head[1]
        h = ops.layer_norm(h, ln.weight, ln.bias, ln.eps, act=ops.ACT_GELU)
        # 498 answers: N % 4 != 0 / K % 64 != 0 would send forward, dgrad and wgrad to the fp32-FMA generic kernel in perf mode
        # (6 launches per step at 3 TFLOP/s); the zero-padded operand copies of ops.vocab_linear keep them on the MFMA kernels
        return ops.vocab_linear(h, self.vqa_head[3].weight, self.vqa_head[3].bias)

    @ops.model_mode
    def predict(self, batch, k=5):
        """The k most probable answers of every sample: {"labels": int64 [B, k] (answer label ids, best first: labels[:, 0] is
        torch.max(logits, 1)[1], the reference's prediction), "probs": fp32 [B, k] (sigmoid of their logits), "logits": the head's
        logits [B, vqa_label_size]}, all on the device.  Runs under no_grad in eval mode (the training flag is restored), with the
        CLS-only last fusion layer; ranking and probabilities come from ops.vqa_eval on the logits as the head left them."""
        if not hasattr(self, "vqa_head"):
            raise RuntimeError('predict needs the VQA head (loss_names["vqa"] > 0)')
        k = int(k)
        if not 1 <= k <= 16:
            raise ValueError(f"k={k} outside [1, 16]")
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                infer = self.infer(batch, mask_text=False, mask_image=False, cls_only=True)
                logits = self.vqa_head_forward(infer["multi_modal_cls_feats"])
                rows = ops.vqa_eval(logits, None, None, None, k=k, want_rows=True)
        finally:
            self.train(was_training)
        return {"labels": rows.topk_idx.long(), "probs": rows.topk_prob, "logits": logits}

    def answers(self, batch, label2ans, k=1):
        """The k best answers of every sample as text: a list of B lists of (answer, probability), best first.  label2ans: the
        reference's mapping with STRING keys (label2ans[str(label)], objectives.py:183-185).  A label it does not hold is a
        KeyError that names it.  One blocking copy of the k labels and probabilities."""
        out = self.predict(batch, k=k)
        return answers_of(out["labels"].cpu().tolist(), out["probs"].cpu().tolist(), label2ans)

    def default_mask_token_id(self):
        """The id fill_mask looks for when it is given none: `self.tokenizer.mask_token_id` when a tokenizer has been attached
        to the module, else config["mask_token_id"], else the id of the vocabulary config["tokenizer"] names -- 50264 (`<mask>`)
        for the RoBERTa vocabularies, 103 (`[MASK]`) for the BERT ones."""
        tok = getattr(self, "tokenizer", None)
        cfg = self.hparams.config
        if tok is not None and getattr(tok, "mask_token_id", None) is not None:
            return int(tok.mask_token_id)
        if cfg.get("mask_token_id") is not None:
            return int(cfg["mask_token_id"])
        return 50264 if "roberta" in str(cfg["tokenizer"]) else 103

    @ops.model_mode
    def fill_mask(self, batch, k=5, mask_token_id=None):
        """The k most probable tokens at every masked position of batch["text_ids"]: {"tokens": int64 [B, S, k] (best first),
        "probs": fp32 [B, S, k] (softmax probabilities over the vocabulary), "mask": bool [B, S] (text_ids == mask_token_id)}, all
        dense and on the device -- a position that is not masked holds -1 / 0, and nothing is copied to the host to count the
        masked ones.  Runs under no_grad in eval mode (the training flag is restored): infer(mask_text=False), the MLM head, and
        ops.token_eval on the logits as the head left them, which reads the masked rows alone.  mask_token_id: None = the id
        default_mask_token_id() finds."""
        if not hasattr(self, "mlm_head"):
            raise RuntimeError('fill_mask needs the MLM head (loss_names["mlm"] > 0)')
        k = int(k)
        if not 1 <= k <= 16:
            raise ValueError(f"k={k} outside [1, 16]")
        V = self.hparams.config["vocab_size"]
        mid = self.default_mask_token_id() if mask_token_id is None else int(mask_token_id)
        if not 0 <= mid < V:
            raise ValueError(f"mask_token_id={mid} outside the vocabulary [0, {V}): pass mask_token_id=")
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                infer = self.infer(batch, mask_text=False, mask_image=False)
                logits = self.mlm_head(infer["multi_modal_text_feats"])
                B, S = logits.shape[0], logits.shape[1]
                mask = infer["text_ids"] == mid                 # built on the device
                rows = ops.token_eval(logits.view(B * S, logits.shape[-1]), None, mask.reshape(-1).contiguous(), None, k=k, want_topk=True)
        finally:
            self.train(was_training)
        return {"tokens": rows.topk_idx.long().view(B, S, k), "probs": rows.topk_prob.view(B, S, k), "mask": mask}

    @ops.model_mode
    def forward(self, batch, test=False):
        """m3ae_module.py:314-345."""
        ret = dict()
        if len(self.current_tasks) == 0:
            ret.update(self.infer(batch))
            return ret
        if "mlm" in self.current_tasks:
            ret.update(objectives.compute_mlm(self, batch))
        if "mim" in self.current_tasks:
            ret.update(objectives.compute_mim(self, batch))
        if "itm" in self.current_tasks:
            ret.update(objectives.compute_itm(self, batch, batch.get("itm_labels")))
        if "vqa" in self.current_tasks:
            ret.update(objectives.compute_vqa_m3ae(self, batch, test=test))
        return ret

    def set_task(self):
        """m3ae_utils.py:95-97."""
        self.current_tasks = [k for k, v in self.hparams.config["loss_names"].items() if v > 0]

    def training_step(self, batch, batch_idx=0):
        """m3ae_module.py:347-353."""
        self.set_task()
        output = self(batch)
        return sum([v * self.hparams.config["loss_names"][k.replace("_loss", "")]
                    for k, v in output.items() if k.endswith("_loss")])

    def configure_optimizers(self):
        """m3ae_module.py:372-373 -> m3ae_utils.set_schedule (:112-242): `([optimizer], [{"scheduler", "interval": "step"}])`.
        The optimizer is a torch.optim.Optimizer (six param groups) whose step() is the fused AdamW over the flat buffers;
        the scheduler is a LambdaLR with the reference's polynomial (or cosine) decay with warm-up.  max_steps comes from
        the attached trainer when there is one (m3ae_utils.py:212-219), else from the config."""
        max_steps = None
        tr = getattr(self, "_trainer", None) or getattr(self, "trainer_ref", None)
        if tr is not None and getattr(tr, "max_steps", None) not in (None, -1):
            max_steps = tr.max_steps
        return self.store.make_optimizer(max_steps)


def state_dict_spec(config):
    """{name: shape} of the module's state_dict (== the reference's key names / shapes)."""
    with torch.device("meta"):
        m = M3AETransformerSS(dict(config, load_path=""))
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}
