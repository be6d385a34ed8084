"""Flat parameter / gradient / optimizer-state storage laid out for MI355X (288 GB HBM3E: everything resident).

All trainable parameters live in ONE fp32 buffer ordered by optimizer group (m3ae_utils.py:135-204's six groups),
each tensor 64-element aligned, with `param.data` and `param.grad` re-pointed to views of the flat buffers:
  * AdamW is one fused kernel launch per group segment (6 launches instead of ~670 per-tensor updates);
    cfg["optim_type"] picks the rule -- AdamW, torch's Adam or SGD with momentum -- and with it the kernel (update_range);
  * the gradient all-reduce operates on contiguous byte ranges of the flat gradient buffer (m3ae_amd/ddp.py);
  * query/key/value weights of one attention block are adjacent, so the packed [3D, D] (or [2D, D]) projection the
    kernels want is a zero-copy view (PackedParam) while state_dict names stay the reference's;
  * in bf16 mode the AdamW kernel also writes the bf16 shadow the forward GEMMs read (same offsets), and each GEMM
    weight unit gets a transposed bf16 copy [K, N] so dgrad is the same K-contiguous "NT" MFMA kernel.
Parameters that never receive a gradient (CLIP text-tower leftovers, RoBERTa pooler) keep their names and
values but are left out of the gradient / optimizer / all-reduce buffers.
"""
import contextlib
import ctypes as C
import math

import torch

from . import _lib

ALIGN = 64
# default betas per rule: the reference's AdamW(betas=(0.9, 0.98)) (m3ae_utils.py:204) and torch.optim.Adam's own.  begin_update's
# `betas` default IS the first object: left alone under optim_type "adam" it stands for the second.
ADAMW_BETAS, ADAM_BETAS = (0.9, 0.98), (0.9, 0.999)

NO_DECAY = ["bias", "LayerNorm.bias", "LayerNorm.weight", "norm.bias", "norm.weight", "norm1.bias", "norm1.weight",
            "norm2.bias", "norm2.weight"]
HEAD_NAMES = ["mlm_head", "mim_head", "itm_head", "vqa_head", "cls_head", "irtr_head"]
NEVER_USED = ("vision_encoder.positional_embedding", "vision_encoder.token_embedding.weight",
              "vision_encoder.ln_final.weight", "vision_encoder.ln_final.bias",
              "language_encoder.pooler.dense.weight", "language_encoder.pooler.dense.bias")


def param_group_of(name):
    """Index 0..5 of the reference's six AdamW groups (m3ae_utils.py:135-204), by substring match on the name."""
    nd = any(k in name for k in NO_DECAY)
    hd = any(k in name for k in HEAD_NAMES)
    mm = "multi_modal" in name
    if not hd and not mm:
        return 1 if nd else 0
    if hd and not mm:
        return 3 if nd else 2
    if mm and not hd:
        return 5 if nd else 4
    return -1


def group_hparams(cfg):
    lr, wd = cfg["learning_rate"], cfg["weight_decay"]
    lh, lm = cfg["lr_multiplier_head"], cfg["lr_multiplier_multi_modal"]
    return [(lr, wd), (lr, 0.0), (lr * lh, wd), (lr * lh, 0.0), (lr * lm, wd), (lr * lm, 0.0)]


class PackedParam:
    """Zero-copy [sum(N_i), K] view over adjacent parameters (q|k|v weights or biases) of the flat buffers."""

    def __init__(self, members):
        self.members = list(members)
        m0 = self.members[0]
        rows = sum(m.shape[0] for m in self.members)
        self.shape = (rows,) + tuple(m0.shape[1:])
        self.m3ae_t = None
        self.m3ae_tb = self.m3ae_tt = None   # tiled copies of the packed weight and of its transpose (ParamStore, tiled_b.py)
        self._check_adjacent()

    def _check_adjacent(self):
        off = 0
        m0 = self.members[0]
        for m in self.members:
            if m.data_ptr() != m0.data_ptr() + off * m0.element_size():
                raise _lib.M3AEHipError("PackedParam members are not adjacent: apply ParamStore before forward")
            off += m.numel()

    def _view(self, t0):
        stride = (self.shape[1], 1) if len(self.shape) == 2 else (1,)
        return t0.as_strided(self.shape, stride)

    @property
    def data(self):
        return self._view(self.members[0].data)

    @property
    def m3ae_c(self):
        m0 = self.members[0]
        v = self._view(getattr(m0, "m3ae_c", m0.data))
        if self.m3ae_tb is not None:
            v.m3ae_tb = self.m3ae_tb
        return v

    @property
    def requires_grad(self):
        return all(m.requires_grad for m in self.members)

    @property
    def grad(self):
        g0 = self.members[0].grad
        return None if g0 is None else self._view(g0)


def param_group_of_decoder(name):
    """The two groups of m3ae_t5_utils.set_schedule_decoder (:308-333): no-decay by substring, one learning rate."""
    nd = ["bias", "LayerNorm.bias", "LayerNorm.weight", "norm.bias", "norm.weight"]
    return 1 if any(k in name for k in nd) else 0


def group_hparams_decoder(cfg):
    lr, wd = cfg["learning_rate"], cfg["weight_decay"]
    return [(lr, wd), (lr, 0.0)] + [(lr, 0.0)] * 4


class ParamStore:
    def __init__(self, module, cfg, device, compute_dtype=torch.bfloat16, weight_units=None, frozen=(),
                 group_fn=param_group_of, hparams_fn=group_hparams):
        self.module, self.cfg, self.device, self.compute_dtype = module, cfg, device, compute_dtype
        # the HIP streams that carry this module's backward work when there is more than one (M3AETransformerSS runs its text
        # half on a second stream): consumers of the flat gradient buffer that run INSIDE a backward pass (ddp.FlatGradReducer)
        # make their own stream wait for the others
        self.streams = set()
        self.hparams_fn = hparams_fn
        from .config import optim_type
        self.optim = optim_type(cfg)      # "adamw" | "adam" | "sgd": which fused kernel update_range launches
        self.momentum = 0.9               # sgd (m3ae_utils.py:208); FlatSGD.step writes its param group's value here
        named = [(n, p) for n, p in module.named_parameters()]
        self.names = {id(p): n for n, p in named}
        # 0..5 optimizer groups; 6..11 = the same classes for parameters without gradient (frozen / never used), kept
        # apart so that weights stay adjacent to weights and biases to biases (PackedParam views) there too
        groups = [[] for _ in range(12)]
        for n, p in named:
            gi = group_fn(n)
            unused = any(n == u or n.endswith("." + u) for u in NEVER_USED) or any(n.startswith(f) for f in frozen)
            if unused or gi < 0 or not p.requires_grad:
                groups[6 + max(gi, 0)].append((n, p))
            else:
                groups[gi].append((n, p))
        self.groups = groups
        # offsets
        self.offset, self.segments = {}, []
        off = 0
        for gi, g in enumerate(groups):
            start = off
            for n, p in g:
                self.offset[id(p)] = off
                off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
            self.segments.append((start, off))
        self.total = off
        self.trainable_end = self.segments[5][1]
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=device)
        self.grad = torch.zeros(self.trainable_end, dtype=torch.float32, device=device)
        self.exp_avg = None
        self.exp_avg_sq = None
        self.shadow = torch.zeros(self.total, dtype=torch.bfloat16, device=device) \
            if compute_dtype == torch.bfloat16 else None
        for gi, g in enumerate(groups):
            for n, p in g:
                o = self.offset[id(p)]
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data.to(device=device, dtype=torch.float32))
                p.data = view
                if gi < 6:
                    p.grad = self.grad[o:o + p.numel()].view(p.shape)
                else:
                    p.requires_grad_(False)
                    p.grad = None
                if self.shadow is not None:
                    p.m3ae_c = self.shadow[o:o + p.numel()].view(p.shape)
        self.step_count = 0
        # EMA of the trainable weights (cfg["ema_decay"] > 0): allocated by the first begin_update, see there
        from .config import ema_decay
        self.ema_decay = ema_decay(cfg)
        self.ema, self.ema_updates, self._ema_open = None, 0, False
        # LoRA (cfg["lora_rank"] > 0): the lora.LoraAdapters attached to this store, whose step() update_apply then takes; None = off
        self.lora = None
        # per-parameter segments (offset, numel) of the trainable range, in buffer order, for the gradient norm (gradnorm.py): the
        # ALIGN padding between parameters is in no segment.  Host list; tables and workspace are uploaded on first use.
        self.grad_segments = sorted((self.offset[id(p)], p.numel(), n) for g in groups[:6] for n, p in g)
        self._sums = self._clip_record = None
        # weight units: GEMM weights that need a transposed bf16 copy for dgrad
        self.units = list(weight_units() if callable(weight_units) else (weight_units or []))
        self._t_bufs = []
        if self.shadow is not None:
            for u in self.units:
                shp = u.shape
                rows, cols = shp[0], int(math.prod(shp[1:]))
                t = torch.empty((cols, rows), dtype=torch.bfloat16, device=device)
                u.m3ae_t = t
                self._t_bufs.append((u, rows, cols, t))
            # Tiled copies (tiled_b.py, ops.TILED_B): the NT GEMMs stage their weight operand from 1-KiB blocks instead of strided
            # 64-B row pieces.  A unit that qualifies gets the tiled copy of its shadow (forward operand) and of its transpose (dgrad
            # operand); one kernel then writes them AND the row-major transpose (other readers: the fused cross-attention kernels,
            # sliced projections) from one read of the shadow.  Every other unit stays with the one-launch transposer.
            from . import ops as _ops, tiled_b as _tb
            self._tile_jobs, tiled, plain = None, [], []
            for (u, rows, cols, t) in self._t_bufs:
                off = (u.data.data_ptr() - self.flat.data_ptr()) // 4
                assert 0 <= off < self.total
                ok = _ops.TILED_B and len(u.shape) == 2 and rows % 8 == 0 and cols % 8 == 0 and (rows % 32 == 0 or cols % 32 == 0)
                if not ok:
                    plain.append((u, rows, cols, t))
                    continue
                src = self.shadow[off:off + rows * cols].view(rows, cols)
                fwd = torch.empty(_tb.tiled_rows(rows) * cols, dtype=torch.bfloat16, device=device) if cols % 32 == 0 else None
                tt = torch.empty(_tb.tiled_rows(cols) * rows, dtype=torch.bfloat16, device=device) if rows % 32 == 0 else None
                tiled.append((src, fwd, t, tt))
                u.m3ae_tt = tt
                if isinstance(u, PackedParam):
                    u.m3ae_tb = fwd
                elif fwd is not None:
                    u.m3ae_c.m3ae_tb = fwd
            if tiled:
                self._tile_jobs = _tb.job_table(tiled, device)
            # job table for the one-launch transposer
            import numpy as np
            tab = np.zeros((len(plain), 5), dtype=np.int64)
            first = 0
            for i, (u, rows, cols, t) in enumerate(plain):
                # source = the unit's bf16 shadow (same element offset as its fp32 master in the flat buffer)
                off = (u.data.data_ptr() - self.flat.data_ptr()) // 4
                assert 0 <= off < self.total
                tab[i] = (self.shadow.data_ptr() + 2 * off, t.data_ptr(), rows, cols, first)
                first += ((rows + 63) // 64) * ((cols + 63) // 64)
            self._t_tiles, self._t_njobs = first, len(plain)
            self._t_jobs = torch.from_numpy(tab).to(device) if plain else None
        self.sync_shadows()

    # ---- shadows -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def sync_shadows(self, cast=True):
        """Refresh bf16 shadows from the fp32 masters (after load_state_dict / manual edits), and the transposed
        copies of every GEMM weight unit.  After an optimizer step only the transposes are needed (cast=False)."""
        if self.shadow is None:
            return
        L = _lib.lib()
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if cast:
            _lib.check(L.m3ae_cast(C.c_void_p(self.flat.data_ptr()), C.c_void_p(self.shadow.data_ptr()), self.total,
                                   _lib.F32, _lib.BF16, s), "m3ae_cast")
        if self._t_bufs and self._t_jobs is not None:
            _lib.check(L.m3ae_transpose_bf16_batched(C.c_void_p(self._t_jobs.data_ptr()), self._t_njobs,
                                                     self._t_tiles, s), "m3ae_transpose_bf16_batched")
        if self._t_bufs and self._tile_jobs is not None:   # tiled copies + the row-major transposes of their units, one pass
            from . import tiled_b as _tb
            _tb.run(*self._tile_jobs, stream=s)

    # ---- optimizer -----------------------------------------------------------------------------------------
    def zero_grad(self):
        from . import ops as _ops
        _lib.check(_lib.lib().m3ae_zero(C.c_void_p(self.grad.data_ptr()), self.grad.numel() * 4, _ops._stream()), "m3ae_zero")

    def lr_factor(self, step, max_steps):
        """transformers get_polynomial_decay_schedule_with_warmup (m3ae_utils.py:232-238), lr_init-relative."""
        cfg = self.cfg
        warm = cfg["warmup_steps"]
        if isinstance(warm, float):
            warm = int(max_steps * warm)
        lr_init, lr_end, power = cfg["learning_rate"], cfg["end_lr"], cfg["decay_power"]
        if step < warm:
            return float(step) / float(max(1, warm))
        if power == "cosine":  # transformers get_cosine_schedule_with_warmup (m3ae_utils.py:225-230), half a cosine
            progress = float(step - warm) / float(max(1, max_steps - warm))
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))
        if step > max_steps:
            return lr_end / lr_init
        pct = 1 - (step - warm) / (max_steps - warm)
        return ((lr_init - lr_end) * pct ** power + lr_end) / lr_init

    def _alloc_state(self):
        """The optimizer state of the rule, zero-filled on first use: two moments for adamw / adam; under sgd the momentum buffer
        lives in `exp_avg` and `exp_avg_sq` is never allocated (one trainable-sized fp32 buffer less)."""
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(self.grad)
        if self.exp_avg_sq is None and self.optim != "sgd":
            self.exp_avg_sq = torch.zeros_like(self.grad)

    def begin_update(self, max_steps=None, grad_scale=1.0, lr_factor=None, group_lrs=None, betas=ADAMW_BETAS, eps=1e-8,
                     group_wds=None):
        """The host part of an optimizer step: per-group learning rates (built-in schedule unless given), step count.  Returns
        the hyper-parameter record `update_range` takes; `optimizer_step` = begin_update + update_range over the six segments, and
        ddp.FlatGradReducer(update_in_backward=True) applies the same record bucket by bucket while backward still runs.
        `betas` left at its default means the rule's own: (0.9, 0.98) for adamw (the reference's), torch's (0.9, 0.999) for adam;
        sgd reads neither betas nor eps and takes its momentum from `self.momentum`.
        With gradient_clip_val set, a step the non-finite guard skips on the device still consumes its step number here and its
        scheduler tick at the caller (as Lightning's scheduler ticks through a GradScaler skip): the count lives on the host,
        which is what keeps the step free of host syncs; grad_stats()["skipped_steps"] counts them.
        With ema_decay > 0 the record carries `ema_w` = 1 - decay_t of this update (config.ema_weight: double, rounded once), and the
        first call allocates `self.ema` as a copy of the trainable weights as they stand before that step.  The count `ema_updates`
        is the host's too: a step the guard skips leaves the average where it is (m3ae_ema_update reads the same record) but still
        consumes its warmup tick, as it consumes its step number."""
        self._no_ema_open("begin_update")
        self._alloc_state()
        if betas is ADAMW_BETAS and self.optim == "adam":
            betas = ADAM_BETAS
        hp = self.hparams_fn(self.cfg)
        if group_lrs is None:
            if lr_factor is None:
                max_steps = max_steps or self.cfg["max_steps"]
                lr_factor = self.lr_factor(self.step_count, max_steps)
            group_lrs = [lr * lr_factor for lr, _ in hp]
        if group_wds is None:
            group_wds = [wd for _, wd in hp]
        self.step_count += 1
        hyper = dict(lrs=[float(x) for x in group_lrs], wds=[float(x) for x in group_wds], b1=float(betas[0]), b2=float(betas[1]),
                     eps=float(eps), step=self.step_count, grad_scale=grad_scale, momentum=float(self.momentum))
        if self.ema_decay > 0:
            from .config import ema_weight
            self._alloc_ema()
            self.ema_updates += 1
            hyper["ema_w"] = ema_weight(self.ema_decay, self.ema_updates, self.cfg.get("ema_warmup", True))
        return hyper

    # ---- EMA of the trainable weights (cfg["ema_decay"]; csrc/misc.hip: m3ae_ema_update / m3ae_ema_swap) ------------------------
    def _alloc_ema(self):
        """`self.ema`: fp32 [trainable_end], on first use a copy of the trainable weights as they stand.  Frozen and never-used
        parameters (flat[trainable_end:]) do not change and are not averaged."""
        if self.ema is None:
            with torch.no_grad():
                self.ema = self.flat[:self.trainable_end].clone()

    def _no_ema_open(self, what):
        if self._ema_open:
            raise RuntimeError(f"ParamStore.{what} inside ema_weights(): the weights are exchanged with their average; leave the "
                               "context before stepping the optimizer")
        if self.lora is not None and self.lora._disabled:
            raise RuntimeError(f"ParamStore.{what} inside lora.disabled(): the weights are the base model's; leave the context "
                               "before stepping the optimizer")

    def _ema_swap(self):
        if self.trainable_end == 0:
            return
        sh = C.c_void_p(self.shadow.data_ptr()) if self.shadow is not None else None
        _lib.check(_lib.lib().m3ae_ema_swap(C.c_void_p(self.flat.data_ptr()), C.c_void_p(self.ema.data_ptr()), sh, self.trainable_end,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "m3ae_ema_swap")
        self.sync_shadows(cast=False)

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate with the averaged weights: on entry one exact exchange of flat[:trainable_end] with `ema` that also writes the bf16
        shadow (m3ae_ema_swap), then the transposed and tiled copies (sync_shadows(cast=False)), on the current stream; on exit, in a
        `finally`, the same again -- which restores every buffer bit for bit.  Runs under no_grad, is not re-entrant, and the
        optimizer entry points raise RuntimeError while it is open.  fp32 / fp32x3: no shadow, the exchange alone."""
        if self.ema is None:
            raise RuntimeError("ema_weights(): no average yet (ema_decay is 0, or no optimizer step has run and none was loaded)")
        if self._ema_open:
            raise RuntimeError("ema_weights() is not re-entrant")
        with torch.no_grad():
            self._ema_swap()
            self._ema_open = True
            try:
                yield self
            finally:
                self._ema_open = False
                self._ema_swap()

    def ema_state_dict(self):
        """{name: CPU fp32 tensor} of the averaged weights, one entry per trainable parameter under its state_dict name."""
        if self.ema is None:
            raise RuntimeError("ema_state_dict(): no average yet (ema_decay is 0, or no optimizer step has run and none was loaded)")
        if self._ema_open:
            raise RuntimeError("ema_state_dict() inside ema_weights(): `ema` holds the raw weights there")
        host = self.ema.cpu()
        return {n: host[self.offset[id(p)]:self.offset[id(p)] + p.numel()].view(p.shape).clone() for g in self.groups[:6] for n, p in g}

    @torch.no_grad()
    def load_ema_state_dict(self, sd, updates):
        """Restore the average and its update count (a checkpoint's `ema_state_dict` / `ema_updates`); a ValueError names a trainable
        parameter that is missing or has another shape, and nothing is written then."""
        self._no_ema_open("load_ema_state_dict")
        named = [(n, p) for g in self.groups[:6] for n, p in g]
        for n, p in named:
            if n not in sd:
                raise ValueError(f"ema_state_dict has no entry for the trainable parameter {n!r}")
            if tuple(sd[n].shape) != tuple(p.shape):
                raise ValueError(f"ema_state_dict[{n!r}] has shape {tuple(sd[n].shape)}, the parameter {tuple(p.shape)}")
        self._alloc_ema()
        for n, p in named:
            o = self.offset[id(p)]
            self.ema[o:o + p.numel()].view(p.shape).copy_(sd[n].to(dtype=torch.float32))
        self.ema_updates = int(updates)

    # A hipGraph-captured step replays with frozen kernel arguments: graph.GraphedStep makes the AdamW launches read this step's
    # learning rate and bias-corrected step size per group from `hyper_dev` ([6][2] fp32 on the device, uploaded before a replay).
    hyper_dev = None

    def _hyper_dev_ptr(self, gi):
        return None if self.hyper_dev is None else C.c_void_p(self.hyper_dev.data_ptr() + 8 * gi)

    @staticmethod
    def hyper_values(hyper):
        """[6][2] host floats {lr, lr * sqrt(1 - b2^t) / (1 - b1^t)} of a begin_update() record: what m3ae_adamw computes from
        (lr, step) on the host when hyper_dev is NULL."""
        t = hyper["step"]
        bc1, bc2 = 1.0 - hyper["b1"] ** t, 1.0 - hyper["b2"] ** t
        return [[lr, lr * math.sqrt(bc2) / bc1] for lr in hyper["lrs"]]

    # ---- the three rules of cfg["optim_type"]: generic names dispatch, the adamw_* names are AdamW and nothing else -----------
    def _adamw_only(self, name):
        if self.optim != "adamw":
            raise ValueError(f'ParamStore.{name} is the AdamW rule, but this store was built with optim_type="{self.optim}": call '
                             f"{dict(adamw_range='update_range', adamw_apply='update_apply', adamw_step='optimizer_step')[name]}")

    @torch.no_grad()
    def update_range(self, a, b, gi, hyper, clip=None, bufs=None, lr_mult=None):
        """The rule's fused kernel (m3ae_adamw / m3ae_adam / m3ae_sgd) over elements [a, b) of the flat buffers (inside optimizer
        group `gi`), on the current stream.  `clip`: the device record of m3ae_clip_finalize; the launch is then the rule's _clip
        form (skip / grad_scale * coef on the device).  With ema_decay > 0, m3ae_ema_update follows right behind over the same
        [a, b) with the same record (a skipped step moves neither): one rule for update_apply and ddp.FlatGradReducer alike.
        `bufs` = (param, grad, exp_avg, exp_avg_sq, shadow) tensors: the same launch over [a, b) of THOSE buffers with group gi's
        hyper-parameters, its learning rate times `lr_mult` (lora.LoraAdapters.step: the adapters have buffers of their own)."""
        self._no_ema_open("update_range")
        if b <= a:
            return
        from . import ops as _ops
        es = 4
        flat, grad, exp_avg, exp_avg_sq, shadow = (self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.shadow) if bufs is None else bufs
        lr = hyper["lrs"][gi] if lr_mult is None else hyper["lrs"][gi] * lr_mult
        sh = C.c_void_p(shadow.data_ptr() + a * 2) if shadow is not None else None
        p, g, m = (C.c_void_p(t.data_ptr() + a * es) for t in (flat, grad, exp_avg))
        if self.optim == "sgd":
            name = "m3ae_sgd"
            args = (p, g, m, sh, b - a, lr, hyper["momentum"], hyper["wds"][gi], hyper["grad_scale"])
        else:
            name = "m3ae_" + self.optim
            args = (p, g, m, C.c_void_p(exp_avg_sq.data_ptr() + a * es), sh, b - a, lr, hyper["b1"], hyper["b2"],
                    hyper["eps"], hyper["wds"][gi], hyper["step"], hyper["grad_scale"])
            if self.optim == "adamw":
                args += (self._hyper_dev_ptr(gi) if bufs is None else None,)
        if clip is not None:
            name, args = name + "_clip", args + (C.c_void_p(clip.data_ptr()),)
        _lib.check(getattr(_lib.lib(), name)(*args, _ops._stream()), name)
        if "ema_w" in hyper and bufs is None:
            _lib.check(_lib.lib().m3ae_ema_update(p, C.c_void_p(self.ema.data_ptr() + a * es), b - a, hyper["ema_w"],
                                                  None if clip is None else C.c_void_p(clip.data_ptr()), _ops._stream()),
                       "m3ae_ema_update")

    @torch.no_grad()
    def optimizer_step(self, max_steps=None, grad_scale=1.0, lr_factor=None, group_lrs=None, betas=ADAMW_BETAS, eps=1e-8,
                       group_wds=None):
        """One optimizer step of the rule over the six group segments + the polynomial-decay schedule, stepped per optimizer step.
        `group_lrs` (one learning rate per group, e.g. an Optimizer's param_groups after its scheduler stepped) overrides the
        built-in schedule.  Arguments as begin_update's."""
        self.update_apply(self.begin_update(max_steps, grad_scale, lr_factor, group_lrs, betas, eps, group_wds))

    @torch.no_grad()
    def update_apply(self, hyper):
        """The device part of an optimizer step for a begin_update() record: six fused launches + the transposed weight copies.
        With cfg["gradient_clip_val"] > 0: the sum of squares of the gradient buffer per parameter (double), the one-workgroup
        finalize with this step's grad_scale, then the six launches in their _clip form -- all on the current stream, the factor and
        the skip flag never leave the device.  With the key at 0 this is the six plain launches and nothing is allocated.
        With adapters attached (cfg["lora_rank"] > 0, self.lora) the device part is lora.LoraAdapters.step: projection, adapter
        update, head segments, merge."""
        self._no_ema_open("update_apply")
        if self.lora is not None:
            return self.lora.step(hyper)
        clip = None
        max_norm = self.clip_val()
        if max_norm > 0:
            from . import gradnorm as _gn, ops as _ops
            clip = self._clip_buffers()
            _gn.clip_finalize(self._sums.run(self.grad, _ops._stream()), hyper["grad_scale"], max_norm, clip, _ops._stream())
        for gi in range(6):
            a, b = self.segments[gi]
            self.update_range(a, min(b, self.trainable_end), gi, hyper, clip)
        self.sync_shadows(cast=False)

    def adamw_range(self, a, b, gi, hyper, clip=None):
        """update_range under optim_type "adamw" (m3ae_adamw / m3ae_adamw_clip); a ValueError under any other rule."""
        self._adamw_only("adamw_range")
        self.update_range(a, b, gi, hyper, clip)

    def adamw_step(self, max_steps=None, grad_scale=1.0, lr_factor=None, group_lrs=None, betas=ADAMW_BETAS, eps=1e-8,
                   group_wds=None):
        """One AdamW step over the six group segments (m3ae_utils.py:206; transformers-4.6.0 AdamW semantics,
        betas (0.9, 0.98), eps 1e-8) + the polynomial-decay schedule, stepped per optimizer step: optimizer_step under optim_type
        "adamw"; a ValueError under any other rule."""
        self._adamw_only("adamw_step")
        self.optimizer_step(max_steps, grad_scale, lr_factor, group_lrs, betas, eps, group_wds)

    def adamw_apply(self, hyper):
        """update_apply under optim_type "adamw"; a ValueError under any other rule."""
        self._adamw_only("adamw_apply")
        self.update_apply(hyper)

    # ---- gradient norm, clipping, non-finite guard (csrc/gradnorm.hip) ---------------------------------------
    def clip_val(self):
        """The validated cfg["gradient_clip_val"]: 0.0 (off), a bound > 0, or inf (guard only)."""
        from .config import gradient_clip_val
        return gradient_clip_val(self.cfg)

    def _segment_sums(self):
        if self._sums is None:
            from . import gradnorm as _gn
            self._sums = _gn.SegmentSums([(o, o + n) for o, n, _ in self.grad_segments], self.grad.numel(), self.grad.device)
        return self._sums

    def _clip_buffers(self):
        self._segment_sums()
        if self._clip_record is None:
            self._clip_record = torch.zeros(_lib.CLIP_RECORD_WORDS, dtype=torch.float32, device=self.grad.device)
        return self._clip_record

    def grad_stats(self):
        """{norm, coef, skipped, steps, clipped_steps, skipped_steps} of the last clipped / guarded step (gradient_clip_val set):
        the norm of the averaged gradient, the factor applied, whether the step was skipped for a non-finite gradient, and the
        running counters.  One small device-to-host copy that blocks: call it where the caller syncs anyway (the log line)."""
        if self._clip_record is None:
            raise RuntimeError("grad_stats(): no step has run with gradient_clip_val set")
        rec = self._clip_record.cpu()
        cnt = rec.view(torch.int32)
        return dict(norm=float(rec[_lib.CLIP_NORM]), coef=float(rec[_lib.CLIP_COEF]), skipped=bool(cnt[_lib.CLIP_SKIP]),
                    steps=int(cnt[_lib.CLIP_STEPS]), clipped_steps=int(cnt[_lib.CLIP_CLIPPED_STEPS]),
                    skipped_steps=int(cnt[_lib.CLIP_SKIPPED_STEPS]))

    @torch.no_grad()
    def grad_norms(self):
        """{name: L2 norm} of every trainable parameter's gradient as the buffer stands (double sums on the device, one launch
        chain, one copy back); no clipping, no scaling."""
        from . import ops as _ops
        out = self._segment_sums().run(self.grad, _ops._stream()).cpu().sqrt()
        return {n: float(v) for (_, _, n), v in zip(self.grad_segments, out)}

    @torch.no_grad()
    def grad_norm(self):
        """Global L2 norm of the gradient buffer as it stands (from the per-parameter double sums)."""
        from . import ops as _ops
        out = self._segment_sums().run(self.grad, _ops._stream()).cpu()
        return math.sqrt(math.fsum(out.tolist()))

    def make_optimizer(self, max_steps=None):
        """([optimizer], [{"scheduler", "interval": "step"}]) in the shape m3ae_utils.set_schedule returns (:240-242); the
        optimizer is the Flat* class of cfg["optim_type"] (m3ae_utils.py:203-210)."""
        max_steps = max_steps or self.cfg["max_steps"]
        opt = {"adamw": FlatAdamW, "adam": FlatAdam, "sgd": FlatSGD}[self.optim](self)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda step: self.lr_factor(step, max_steps))
        return [opt], [{"scheduler": sched, "interval": "step"}]

    def group_names(self):
        return [[n for n, _ in g] for g in self.groups[:6]]


def state_dict_rule(state_dict):
    """Which rule wrote an optimizer state dict: "sgd" (torch.optim.SGD, FlatSGD: a `momentum` group key or momentum buffers),
    "adam" (torch.optim.Adam, FlatAdam: torch's `amsgrad` group key, decay not decoupled) or "adamw" (FlatAdamW, HF AdamW: betas
    without `amsgrad`).  Adam's and AdamW's per-parameter state look alike; the group keys tell them apart."""
    groups = state_dict["param_groups"]
    first = next(iter(state_dict["state"].values()), {})
    if any("momentum" in g for g in groups) or "momentum_buffer" in first:
        return "sgd"
    if any("amsgrad" in g and not g.get("decoupled_weight_decay", False) for g in groups):
        return "adam"
    return "adamw"


class _FlatOptimizer(torch.optim.Optimizer):
    """What the three Optimizer faces of ParamStore share: six param groups -- {base, head x lr_multiplier_head, multi_modal x
    lr_multiplier_multi_modal} x {weight decay, no decay} -- with the reference's lr / weight_decay per group, a `step()` that is
    one fused launch per group with the learning rates read from `param_groups[i]["lr"]` (whatever a scheduler wrote there), and
    `state_dict()` / `load_state_dict()` in torch's per-parameter layout over views of the flat state buffers."""
    RULE = None
    STATE = ()            # (torch's state key, ParamStore attribute) per flat state buffer
    HAS_STEP = True       # torch's per-parameter `step`
    GROUP_KEYS = ("lr", "weight_decay", "initial_lr")

    def __init__(self, store, defaults, grad_scale=1.0):
        if store.optim != self.RULE:
            raise ValueError(f'{type(self).__name__} needs a store built with optim_type="{self.RULE}", got "{store.optim}"')
        self.store = store
        self.grad_scale = grad_scale
        groups = []
        for gi, (lr, wd) in enumerate(store.hparams_fn(store.cfg)):
            params = [p for _, p in store.groups[gi]]
            if not params:   # torch rejects empty groups: keep the slot with a placeholder so that indices stay group ids
                params = [torch.nn.Parameter(torch.zeros(0, device=store.device), requires_grad=False)]
            groups.append(dict(params=params, lr=lr, weight_decay=wd, m3ae_group=gi))
        super().__init__(groups, defaults)

    def _bind_state(self):
        st = self.store
        st._alloc_state()
        for gi in range(6):
            for _, p in st.groups[gi]:
                o = st.offset[id(p)]
                d = dict(step=torch.tensor(float(st.step_count))) if self.HAS_STEP else {}
                for key, attr in self.STATE:
                    d[key] = getattr(st, attr)[o:o + p.numel()].view(p.shape)
                self.state[p] = d

    def _hyper(self, g):
        """Keyword arguments of ParamStore.optimizer_step from the param groups (by m3ae_group)."""
        return dict(group_lrs=[g[i]["lr"] for i in range(6)], group_wds=[g[i]["weight_decay"] for i in range(6)],
                    grad_scale=self.grad_scale)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.store.optimizer_step(**self._hyper({pg["m3ae_group"]: pg for pg in self.param_groups}))
        return loss

    def zero_grad(self, set_to_none=False):
        self.store.zero_grad()   # gradients are views of the flat buffer: never set to None

    def state_dict(self):
        self._bind_state()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        st = self.store
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        mine = [p for g in self.param_groups for p in g["params"]]
        if len(ids) != len(mine):
            raise ValueError("optimizer state_dict does not match this model's parameter groups")
        self._check_rule(state_dict, state_dict_rule(state_dict))     # state of another rule: ValueError
        st._alloc_state()
        step = None
        for i, p in zip(ids, mine):
            s = state_dict["state"].get(i)
            if s is None or id(p) not in st.offset or p.numel() == 0:
                continue
            o = st.offset[id(p)]
            for key, attr in self.STATE:
                getattr(st, attr)[o:o + p.numel()].view(p.shape).copy_(s[key])
            if self.HAS_STEP:
                step = int(s["step"]) if step is None else step
        if step is not None:
            st.step_count = step
        for pg, sg in zip(self.param_groups, state_dict["param_groups"]):
            for k in self.GROUP_KEYS:
                if k in sg:
                    pg[k] = sg[k]
        self._bind_state()

    def _check_rule(self, state_dict, rule):
        if rule != self.RULE:
            raise ValueError(f'optimizer state_dict was written by the "{rule}" rule, this optimizer is optim_type="{self.RULE}"')


class FlatAdamW(_FlatOptimizer):
    """torch.optim.Optimizer face of ParamStore's fused AdamW (the object m3ae_utils.set_schedule returns as
    `optimizer`, m3ae_utils.py:135-206): six param groups -- {base, head x lr_multiplier_head, multi_modal x
    lr_multiplier_multi_modal} x {weight decay, no decay} -- with the reference's lr / weight_decay / betas / eps per group,
    so a Lightning-style loop (`optimizer.step(); scheduler.step(); optimizer.zero_grad()`) and LambdaLR schedulers work.
    `step()` is one fused kernel launch per group over the flat buffers; the learning rates are read from
    `param_groups[i]["lr"]` (whatever a scheduler wrote there).  `state_dict()` / `load_state_dict()` round-trip the
    moments (per parameter, torch's layout) and the step count.
    With `gradient_clip_val` in the store's config, `step()` clips by global norm and skips a non-finite step on the device
    (ParamStore.update_apply); a skipped step still advances the step count, and the caller's scheduler ticks as usual."""
    RULE = "adamw"
    STATE = (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq"))
    GROUP_KEYS = ("lr", "weight_decay", "betas", "eps", "initial_lr")

    def __init__(self, store, grad_scale=1.0):
        super().__init__(store, dict(lr=store.cfg["learning_rate"], betas=ADAMW_BETAS, eps=1e-8, weight_decay=0.0), grad_scale)

    def _hyper(self, g):
        return dict(super()._hyper(g), betas=g[0]["betas"], eps=g[0]["eps"])

    def _check_rule(self, state_dict, rule):
        # (a torch.optim.AdamW dict carries `amsgrad` like Adam's: only a dict FlatAdam wrote is known to be the other rule)
        if rule == "sgd" or any(g.get("m3ae_rule", "adamw") != "adamw" for g in state_dict["param_groups"]):
            raise ValueError(f'optimizer state_dict was written by the "{rule}" rule, this optimizer is optim_type="adamw"')


class FlatAdam(FlatAdamW):
    """The same face over the fused torch.optim.Adam rule (optim_type "adam", m3ae_utils.py:205-206): torch's defaults, betas
    (0.9, 0.999), eps 1e-8, coupled weight decay, no amsgrad.  param_groups carry every key of torch.optim.Adam's defaults, the
    state is torch's (`step`, `exp_avg`, `exp_avg_sq`): a torch.optim.Adam state dict over the same groups loads here and this
    one's loads there.  The moments of FlatAdamW mean something else (decoupled decay, another bias correction): its state dicts
    are refused."""
    RULE = "adam"

    def __init__(self, store, grad_scale=1.0):
        d = dict(torch.optim.Adam([torch.zeros(1)], lr=store.cfg["learning_rate"]).defaults)   # torch's keys, whatever its version
        d.update(betas=ADAM_BETAS, eps=1e-8, weight_decay=0.0, amsgrad=False, m3ae_rule="adam")
        _FlatOptimizer.__init__(self, store, d, grad_scale)

    def _check_rule(self, state_dict, rule):
        groups = state_dict["param_groups"]
        if rule != "adam" or any(g.get("m3ae_rule", "adam") != "adam" for g in groups):
            raise ValueError('optimizer state_dict was written by an AdamW rule (decoupled decay), this optimizer is optim_type="adam"')
        if any(g.get("amsgrad") for g in groups):
            raise ValueError("optim_type adam has no amsgrad variant")


class FlatSGD(_FlatOptimizer):
    """The same face over the fused torch.optim.SGD rule (optim_type "sgd", m3ae_utils.py:207-208): momentum 0.9, dampening 0, no
    Nesterov, coupled weight decay.  param_groups carry every key of torch.optim.SGD's defaults, the state is torch's
    (`momentum_buffer`, no step): a torch.optim.SGD state dict over the same groups loads here and this one's loads there.  The
    buffer is the store's `exp_avg`; `exp_avg_sq` is never allocated."""
    RULE = "sgd"
    STATE = (("momentum_buffer", "exp_avg"),)
    HAS_STEP = False
    GROUP_KEYS = ("lr", "weight_decay", "momentum", "initial_lr")

    def __init__(self, store, grad_scale=1.0):
        d = dict(torch.optim.SGD([torch.zeros(1)], lr=store.cfg["learning_rate"], momentum=store.momentum).defaults)
        d.update(momentum=store.momentum, dampening=0, nesterov=False, weight_decay=0.0, m3ae_rule="sgd")
        super().__init__(store, d, grad_scale)

    def step(self, closure=None):
        g0 = self.param_groups[0]
        if any(pg["momentum"] != g0["momentum"] or pg["dampening"] != 0 or pg["nesterov"] for pg in self.param_groups):
            raise ValueError("optim_type sgd: one momentum for all groups, dampening 0, no Nesterov")
        self.store.momentum = float(g0["momentum"])
        return super().step(closure)
