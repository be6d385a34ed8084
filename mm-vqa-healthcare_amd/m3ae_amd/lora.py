"""LoRA fine-tuning in merged form on the flat buffers (config keys lora_rank / lora_alpha / lora_targets / lora_lr_multiplier /
lora_path; csrc/lora.hip).

The effective weight W = W0 + s B A (s = lora_alpha / lora_rank) of every target lives in the ordinary fp32 master and bf16
shadow of the ParamStore, so every forward, dgrad and wgrad kernel runs as it does without adapters, the ordinary state_dict always
holds the merged weights (it loads upstream and in a lora_rank=0 model; merge-and-unload is free) and inference pays nothing.  The
adapter gradients come out of the full weight gradient the step computes anyway: dA = s B^T dW, dB = s dW A^T, exact by the chain
rule because y = x W^T.  Per optimizer step (LoraAdapters.step, called by ParamStore.update_apply):

    m3ae_lora_grad  ->  the store's optimizer rule over the adapter buffer (two ranges)  ->  the rule over the head segments
    ->  m3ae_lora_merge  ->  sync_shadows(cast=False)

Nothing else in the trainable range moves: norms, biases and embeddings stay at their base values.

Buffers: `base`, a compact fp32 copy of every target's W0 taken at attach time; `lora`, the adapters' flat fp32 buffer laid out
[group-0 targets: A, B, A, B, ... | group-4 targets: A, B, ...] (every matrix 64-element aligned, as ParamStore aligns parameters);
`lora_grad` of the same layout; the adapters' optimizer moments; the workspace of the projection.
"""
import contextlib
import ctypes as C
import hashlib
import math

import numpy as np
import torch

from . import _lib
from .param_store import ALIGN, NEVER_USED, PackedParam, group_hparams, param_group_of

FIELDS = ("elem_offset", "N", "K", "a_off", "b_off", "base_off")
TARGET_GROUPS = (0, 4)     # optimizer groups whose GEMM weights are adapted: towers / projections (0), fusion layers / poolers (4)


def _align(n):
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


def adapter_key(weight_name):
    """state_dict prefix of a target's adapters: the weight's name without ".weight"; CLIP's fused `...attn.in_proj_weight` gives
    `...attn.in_proj` (keys `<prefix>.lora_A` / `<prefix>.lora_B`)."""
    if weight_name.endswith(".weight"):
        return weight_name[:-len(".weight")]
    if weight_name.endswith("_weight"):
        return weight_name[:-len("_weight")]
    return weight_name


def is_attention(name):
    """Whether a target's name is an attention projection (CLIP `attn.`, BERT `attention.` / `crossattention.`)."""
    return ".attn." in name or "attention." in name


def target_names(module, targets="all-linear", frozen=(), group_fn=param_group_of):
    """Names of the parameters LoRA adapts, in named_parameters order: the 2-D weight of every nn.Linear and CLIP's fused
    `in_proj_weight` [3D, D] -- the GEMM weights -- that train and sit in optimizer group 0 or 4.  The query / key / value Linears of
    a packed unit are three targets under their own names; heads (groups 2 / 3), embeddings, the 4-D patch convolution, biases and
    norms are not selected.  Works before finalize() and on a module built on the meta device: only names, types and shapes are
    read (LoraAdapters checks the selection against the store's weight units when it attaches)."""
    from .config import LORA_TARGETS
    if not isinstance(targets, str) or targets not in LORA_TARGETS:
        raise ValueError(f"lora_targets must be one of {LORA_TARGETS}, got {targets!r}")
    gemm = {id(m.weight) for m in module.modules() if isinstance(m, torch.nn.Linear)}
    out = []
    for n, p in module.named_parameters():
        if not (id(p) in gemm or n.endswith("in_proj_weight")) or p.dim() != 2 or not p.requires_grad or group_fn(n) not in TARGET_GROUPS:
            continue
        if any(n == u or n.endswith("." + u) for u in NEVER_USED) or any(n.startswith(f) for f in frozen):
            continue
        if targets == "attention" and not is_attention(n):
            continue
        out.append(n)
    return out


def adapter_layout(shapes, r):
    """([(a_off, b_off)], total) of the adapters of `shapes` = [(N, K), ...] at rank r: A[r, K] then B[N, r] per target, each
    64-element aligned."""
    offs, off = [], 0
    for N, K in shapes:
        a = off
        off += _align(r * K)
        b = off
        off += _align(N * r)
        offs.append((a, b))
    return offs, off


class LoraTable:
    """The device table of m3ae_lora_merge / m3ae_lora_grad and the projection's workspace.  `records`: one
    (elem_offset, N, K, a_off, b_off, base_off) per target; `sizes`: the element counts of the buffers the offsets point into
    (flat, lora, base).  The kernels follow the table without checking it, so everything is checked here: shapes >= 1, offsets
    aligned and inside their buffer, no two targets overlapping in any buffer."""

    def __init__(self, records, r, sizes, device):
        tab = np.asarray(records, dtype=np.int64).reshape(-1, 6)
        self.r, self.n = int(r), len(tab)
        if not 1 <= self.r <= _lib.LORA_MAX_RANK:
            raise ValueError(f"LoRA rank must be in [1, {_lib.LORA_MAX_RANK}], got {r}")
        if not 1 <= self.n <= _lib.LORA_MAX_TARGETS:
            raise ValueError(f"a LoRA table holds 1..{_lib.LORA_MAX_TARGETS} targets, got {self.n}")
        spans = {"flat": [], "lora": [], "base": []}
        for i, (off, N, K, a, b, bo) in enumerate(tab.tolist()):
            if N < 1 or K < 1:
                raise ValueError(f"target {i}: N and K must be >= 1, got {(N, K)}")
            for what, o, n in (("flat", off, N * K), ("lora", a, self.r * K), ("lora", b, N * self.r), ("base", bo, N * K)):
                if o < 0 or o % 4 or o + n > sizes[what]:
                    raise ValueError(f"target {i}: [{o}, {o + n}) is misaligned or outside the {what} buffer ({sizes[what]} elements)")
                spans[what].append((o, o + n))
        for what, sp in spans.items():
            sp.sort()
            for (_, e0), (b1, _) in zip(sp, sp[1:]):
                if b1 < e0:
                    raise ValueError(f"two targets overlap in the {what} buffer at element {b1}")
        self.sizes = dict(sizes)
        self.host = np.ascontiguousarray(tab)
        self.dev = torch.from_numpy(self.host).to(device)
        self.ws_bytes = int(_lib.lib().m3ae_lora_grad_workspace_bytes(self.host.ctypes.data_as(C.c_void_p), self.n, self.r))
        if self.ws_bytes < 0:
            _lib.check(self.ws_bytes, "m3ae_lora_grad_workspace_bytes")
        self.workspace = torch.empty(max(self.ws_bytes // 4, 1), dtype=torch.float32, device=device)

    def _check(self, **bufs):
        for what, (t, key) in bufs.items():
            if t is not None and t.numel() < self.sizes[key]:
                raise ValueError(f"{what} has {t.numel()} elements, the table was built for {self.sizes[key]}")

    def merge(self, s, base, lora, flat, shadow, mode, stream):
        """W = W0 + s B A (mode 0) or W = W0 (mode 1) into `flat` and, where given, the bf16 `shadow`."""
        self._check(base=(base, "base"), lora=(lora, "lora"), flat=(flat, "flat"), shadow=(shadow, "flat"))
        _lib.check(_lib.lib().m3ae_lora_merge(C.c_void_p(self.dev.data_ptr()), self.n, self.r, float(s), C.c_void_p(base.data_ptr()),
                                              None if lora is None else C.c_void_p(lora.data_ptr()), C.c_void_p(flat.data_ptr()),
                                              None if shadow is None else C.c_void_p(shadow.data_ptr()), int(mode), stream),
                   "m3ae_lora_merge")

    def grad(self, s, lora, grad_flat, lora_grad, stream, workspace=None):
        """dA = s B^T dW, dB = s dW A^T for every target, overwriting `lora_grad`."""
        ws = self.workspace if workspace is None else workspace
        if ws.numel() * 4 < self.ws_bytes:
            raise ValueError(f"workspace has {ws.numel() * 4} bytes, the projection needs {self.ws_bytes}")
        self._check(lora=(lora, "lora"), grad_flat=(grad_flat, "flat"), lora_grad=(lora_grad, "lora"))
        _lib.check(_lib.lib().m3ae_lora_grad(C.c_void_p(self.dev.data_ptr()), self.n, self.r, float(s), C.c_void_p(lora.data_ptr()),
                                             C.c_void_p(grad_flat.data_ptr()), C.c_void_p(lora_grad.data_ptr()),
                                             C.c_void_p(ws.data_ptr()), stream), "m3ae_lora_grad")


def init_A(name, r, K, seed):
    """A ~ U(-1 / sqrt(K), 1 / sqrt(K)) [r, K] from a CPU generator seeded by (seed, parameter name): the same on every process."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int.from_bytes(hashlib.sha256(f"{int(seed)}:{name}".encode()).digest()[:8], "little") & (2 ** 63 - 1))
    return (torch.rand(r, K, generator=g, dtype=torch.float32) * 2.0 - 1.0) / math.sqrt(K)


def fingerprint_mismatch(name, mine, theirs, numel):
    """None, or why the (sum, sum of squares) fingerprints of two base weights differ.  The sums are float64 reductions whose order
    may differ between devices: they are compared to 1e-9 of their scale (sum of squares: itself; sum: sqrt(numel * sum of
    squares), the Cauchy-Schwarz bound on sum |x|), far below what a different weight moves them by."""
    (s0, q0), (s1, q1) = mine, theirs
    if abs(q0 - q1) > 1e-9 * max(q0, q1) or abs(s0 - s1) > 1e-9 * math.sqrt(numel * max(q0, q1)):
        return f"the base weight {name!r} differs from the one the adapters were trained on (sum {s1!r} / sum of squares {q1!r} there, {s0!r} / {q0!r} here)"
    return None


class LoraAdapters:
    """The adapters of one ParamStore.  LoraAdapters(store, module) attaches: it selects the targets, copies their weights as they
    stand into `base`, draws A, zeroes B, and sets store.lora so that ParamStore.update_apply takes step().  With B = 0 the merged
    weights are the base weights, so attaching changes no bit of the model."""

    def __init__(self, store, module, cfg=None):
        from . import config as config_mod
        cfg = store.cfg if cfg is None else cfg
        self.rank = config_mod.lora_rank(cfg)
        if self.rank < 1:
            raise ValueError("LoraAdapters needs lora_rank >= 1")
        if config_mod.ema_decay(cfg) > 0 or config_mod.ema_decay(store.cfg) > 0:
            raise ValueError("lora_rank > 0 cannot be combined with ema_decay: the average covers the full weight buffer, whose "
                             "targets are a function of the adapters; averaging the adapters is not built")
        if config_mod.gradient_clip_val(cfg) > 0 or store.clip_val() > 0:
            raise ValueError("lora_rank > 0 cannot be combined with gradient_clip_val: the norm that clips would be the full "
                             "gradient's, not the adapters'; clipping over the projected gradients is not built")
        if getattr(store, "lora", None) is not None:
            raise ValueError("this ParamStore already has adapters attached")
        if store.hparams_fn is not group_hparams:
            raise ValueError("lora_rank > 0 is not available under the T5 / decoder wrappers: their M3AE is frozen and produces no "
                             "weight gradient to project")
        self.store, self.alpha, self.targets_mode = store, float(cfg.get("lora_alpha", 16.0)), cfg.get("lora_targets", "all-linear")
        self.lr_multiplier = float(cfg.get("lora_lr_multiplier", 10.0))
        self.scale = self.alpha / self.rank
        self._disabled = False
        dev, r = store.device, self.rank
        params = dict(module.named_parameters())
        in_group = {gi: {id(p) for _, p in store.groups[gi]} for gi in TARGET_GROUPS}
        names = [n for n in target_names(module, self.targets_mode) if any(id(params[n]) in in_group[gi] for gi in TARGET_GROUPS)]
        if not names:
            raise ValueError(f"lora_targets={self.targets_mode!r} selects no trainable GEMM weight of this model")
        units = {id(m) for u in store.units for m in (u.members if isinstance(u, PackedParam) else [u])}
        stray = [n for n in names if id(params[n]) not in units]
        if stray:   # the transposed / tiled copies follow the weight units: a target outside them would train without its copies
            raise ValueError(f"LoRA target {stray[0]!r} is no GEMM weight unit of this store")
        order = sorted(names, key=lambda n: store.offset[id(params[n])])      # buffer order: group 0 first, then group 4
        self.names = order
        self.params = [params[n] for n in order]
        shapes = [tuple(p.shape) for p in self.params]
        offs, self.total = adapter_layout(shapes, r)
        n0 = sum(1 for p in self.params if id(p) in in_group[0])
        self.split = offs[n0][0] if n0 < len(offs) else self.total               # [0, split): group-0 adapters, [split, total): group-4
        records, boff = [], 0
        for p, (N, K), (a, b) in zip(self.params, shapes, offs):
            records.append((store.offset[id(p)], N, K, a, b, boff))
            boff += _align(N * K)
        self.base_total = boff
        self.table = LoraTable(records, r, dict(flat=store.trainable_end, lora=self.total, base=boff), dev)
        self.records = records
        with torch.no_grad():
            self.base = torch.zeros(boff, dtype=torch.float32, device=dev)
            self.lora = torch.zeros(self.total, dtype=torch.float32, device=dev)
            self.lora_grad = torch.zeros(self.total, dtype=torch.float32, device=dev)
            for n, p, rec in zip(order, self.params, records):
                _, N, K, a, _, bo = rec
                self.base[bo:bo + N * K].copy_(p.data.reshape(-1))
                self.lora[a:a + r * K].copy_(init_A(n, r, K, cfg.get("seed", 0)).reshape(-1))
        self.exp_avg = self.exp_avg_sq = None
        self.fingerprint = self._fingerprint()
        self.elements = sum(r * K + N * r for N, K in shapes)
        store.lora = self

    # ---- description ---------------------------------------------------------------------------------------------------------
    def describe(self):
        return f"lora r={self.rank} ({len(self.names)} targets, {self.elements} adapter elements)"

    def config(self):
        return dict(rank=self.rank, alpha=self.alpha, targets=self.targets_mode)

    @torch.no_grad()
    def _fingerprint(self):
        """float64 (sum, sum of squares) of every target's W0, [ntargets, 2] on the host."""
        out = torch.zeros(len(self.records), 2, dtype=torch.float64, device=self.base.device)
        for i, (_, N, K, _, _, bo) in enumerate(self.records):
            w = self.base[bo:bo + N * K].double()
            out[i, 0], out[i, 1] = w.sum(), (w * w).sum()
        return out.cpu()

    def views(self, i, buf=None):
        """(A [r, K], B [N, r]) views of target i in `buf` (default: the adapter buffer)."""
        buf = self.lora if buf is None else buf
        _, N, K, a, b, _ = self.records[i]
        return buf[a:a + self.rank * K].view(self.rank, K), buf[b:b + N * self.rank].view(N, self.rank)

    # ---- the step --------------------------------------------------------------------------------------------------------------
    def _stream(self):
        from . import ops as _ops
        return _ops._stream()

    def _alloc_state(self):
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(self.lora)
        if self.exp_avg_sq is None and self.store.optim != "sgd":
            self.exp_avg_sq = torch.zeros_like(self.lora)

    def _open(self, what):
        if self._disabled:
            raise RuntimeError(f"{what} inside lora.disabled(): the weights are the base model's; leave the context first")

    @torch.no_grad()
    def merge(self, mode=0):
        """Write W = W0 + s B A (mode 1: W0) of every target into the store's master and shadow, on the current stream."""
        st = self.store
        self.table.merge(self.scale, self.base, self.lora, st.flat, st.shadow, mode, self._stream())

    @torch.no_grad()
    def project(self):
        """lora_grad = the adapter gradients of the store's gradient buffer as it stands (overwritten)."""
        self.table.grad(self.scale, self.lora, self.store.grad, self.lora_grad, self._stream())

    @torch.no_grad()
    def step(self, hyper):
        """The device part of an optimizer step with adapters (ParamStore.update_apply hands its begin_update() record over):
        projection, the store's rule over the two adapter ranges with the learning rate and weight decay of groups 0 and 4 (rate x
        lora_lr_multiplier), the rule over the head segments (groups 2 and 3) as without adapters, merge, transposed / tiled copies."""
        self._open("LoraAdapters.step")
        st = self.store
        self._alloc_state()
        self.project()
        bufs = (self.lora, self.lora_grad, self.exp_avg, self.exp_avg_sq, None)
        st.update_range(0, self.split, TARGET_GROUPS[0], hyper, bufs=bufs, lr_mult=self.lr_multiplier)
        st.update_range(self.split, self.total, TARGET_GROUPS[1], hyper, bufs=bufs, lr_mult=self.lr_multiplier)
        for gi in (2, 3):
            a, b = st.segments[gi]
            st.update_range(a, min(b, st.trainable_end), gi, hyper)
        self.merge()
        st.sync_shadows(cast=False)

    @contextlib.contextmanager
    def disabled(self):
        """The base model: on entry W = W0 on every target (m3ae_lora_merge mode 1) and the transposed / tiled copies; on exit, in a
        `finally`, the normal merge and the copies again, which restores every bit (the merge is a function of base and adapters
        alone).  Runs under no_grad, is not re-entrant, and the optimizer entry points raise RuntimeError while it is open."""
        self._open("lora.disabled()")
        with torch.no_grad():
            self.merge(mode=1)
            self.store.sync_shadows(cast=False)
            self._disabled = True
            try:
                yield self
            finally:
                self._disabled = False
                self.merge()
                self.store.sync_shadows(cast=False)

    # ---- adapter files ---------------------------------------------------------------------------------------------------------
    def head_items(self):
        return [(n, p) for gi in (2, 3) for n, p in self.store.groups[gi]]

    @torch.no_grad()
    def state_dict(self):
        """{`<prefix>.lora_A`, `<prefix>.lora_B` per target (adapter_key), every head parameter under its state_dict name,
        "lora_config": {rank, alpha, targets}, "base_fingerprint": {weight name: (sum, sum of squares) of W0 in float64}} on the
        host: the base checkpoint plus this dict is the whole fine-tuned model."""
        self._open("LoraAdapters.state_dict")
        host = self.lora.cpu()
        sd = {}
        for i, n in enumerate(self.names):
            A, B = self.views(i, host)
            sd[adapter_key(n) + ".lora_A"], sd[adapter_key(n) + ".lora_B"] = A.clone(), B.clone()
        for n, p in self.head_items():
            sd[n] = p.detach().to("cpu", copy=True)
        sd["lora_config"] = self.config()
        sd["base_fingerprint"] = {n: (float(self.fingerprint[i, 0]), float(self.fingerprint[i, 1])) for i, n in enumerate(self.names)}
        return sd

    def check_state_dict(self, sd):
        """Raise the ValueError that names the first way `sd` does not fit these adapters and this base; writes nothing."""
        cfg = sd.get("lora_config")
        if not isinstance(cfg, dict):
            raise ValueError("not an adapter state dict: no lora_config entry")
        for key, mine in self.config().items():
            if key != "alpha" and cfg.get(key) != mine:
                raise ValueError(f"adapter file has lora {key} {cfg.get(key)!r}, this model {mine!r}")
        fp = sd.get("base_fingerprint") or {}
        theirs = [k for k in fp if k not in set(self.names)]
        if theirs:
            raise ValueError(f"adapter file has the target {theirs[0]!r}, which this model does not adapt")
        for i, (n, (_, N, K, _, _, _)) in enumerate(zip(self.names, self.records)):
            if n not in fp:
                raise ValueError(f"adapter file has no target {n!r}")
            for suffix, shape in ((".lora_A", (self.rank, K)), (".lora_B", (N, self.rank))):
                t = sd.get(adapter_key(n) + suffix)
                if t is None or tuple(t.shape) != shape:
                    raise ValueError(f"adapter file: {adapter_key(n) + suffix} is {None if t is None else tuple(t.shape)}, expected {shape}")
            why = fingerprint_mismatch(n, (float(self.fingerprint[i, 0]), float(self.fingerprint[i, 1])), fp[n], N * K)
            if why:
                raise ValueError(why)
        for n, p in self.head_items():
            if n not in sd or tuple(sd[n].shape) != tuple(p.shape):
                raise ValueError(f"adapter file: head parameter {n!r} is missing or has another shape")

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Restore adapters, alpha and head parameters from state_dict()'s dict and merge.  Another base (fingerprint), rank or
        target set is a ValueError that names the first mismatch; nothing is written then."""
        self._open("LoraAdapters.load_state_dict")
        self.check_state_dict(sd)
        self.alpha = float(sd["lora_config"]["alpha"])
        self.scale = self.alpha / self.rank
        for i, n in enumerate(self.names):
            A, B = self.views(i)
            A.copy_(sd[adapter_key(n) + ".lora_A"].to(dtype=torch.float32))
            B.copy_(sd[adapter_key(n) + ".lora_B"].to(dtype=torch.float32))
        for n, p in self.head_items():
            p.data.copy_(sd[n].to(dtype=torch.float32))
        self.merge()
        self.store.sync_shadows()

    def optimizer_state(self):
        """The adapters' moments on the host (None before the first step)."""
        return None if self.exp_avg is None else dict(exp_avg=self.exp_avg.cpu(), exp_avg_sq=None if self.exp_avg_sq is None else self.exp_avg_sq.cpu())

    @torch.no_grad()
    def load_optimizer_state(self, state):
        if state is None:
            return
        if tuple(state["exp_avg"].shape) != (self.total,) or (state.get("exp_avg_sq") is None) != (self.store.optim == "sgd"):
            raise ValueError("the adapters' optimizer state was written for another adapter layout or optimizer rule")
        self._alloc_state()
        self.exp_avg.copy_(state["exp_avg"])
        if self.exp_avg_sq is not None:
            self.exp_avg_sq.copy_(state["exp_avg_sq"])


def refuse_wrapper(cfg, what):
    """The T5 and decoder wrappers call this from finalize(): their M3AE is frozen and produces no weight gradient."""
    from .config import lora_rank
    if lora_rank(cfg) > 0:
        raise ValueError(f"lora_rank > 0 is not available under {what}: its M3AE is frozen and produces no weight gradient to project")
