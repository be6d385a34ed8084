"""Autograd operators of the hot path, each a thin host wrapper over the C ABI (include/m3ae_hip.h).

PyTorch supplies device memory, the stream and the autograd tape; every FLOP on the path runs in libm3ae_hip.so.
Parameter gradients are ACCUMULATED IN PLACE into `param.grad` (fp32, normally a view of ParamStore's flat
gradient buffer) by the wgrad / reduction kernels themselves, and the Functions return None for them: no autograd
accumulation kernels, and the data-parallel reducer (m3ae_amd/ddp.py) is told the moment a gradient is complete
through `grad_ready_hook`.
"""
import contextlib
import ctypes as C
import functools
import math
import os
import threading
from types import SimpleNamespace as _NS
from typing import NamedTuple

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_MULAUX, ACT_NONE, ACT_QUICKGELU, ACT_RELU, ACT_TANH, BF16, F32, AttnDesc, GemmDesc, XattnDesc,
                   check)

grad_ready_hook = None  # callable(param) set by the DDP reducer
# forward activation GEMMs save act'(pre-activation) for their backward GEMM (A/B knob: M3AE_SAVE_DACT=0 saves the
# pre-activation and re-evaluates the derivative in the backward epilogue, the first scheme of this repo)
SAVE_DACT = os.environ.get("M3AE_SAVE_DACT", "1") != "0"
# host-side launch policy, set by ddp.FlatGradReducer while collectives run next to backward (per-call flag in the GEMM
# descriptor: the library itself keeps no state)
NT_NO_PERSISTENT = os.environ.get("M3AE_NT_NO_PERSISTENT", "0") == "1"   # (set by ddp.FlatGradReducer.attach; the env default is for A/B runs)
# diagnostic per-call kernel selectors (m3ae_gemm_desc.launch_flags; -1 / 0 = by shape): tests compare kernel variants bit for
# bit, tools time them; the product path never sets them
GEMM_NT_VARIANT, GEMM_TN_VARIANT, GEMM_COL_GROUP = int(os.environ.get("M3AE_GEMM_NT_VARIANT", -1)), int(os.environ.get("M3AE_GEMM_TN_VARIANT", -1)), int(os.environ.get("M3AE_GEMM_COL_GROUP", 0))   # (env: A/B runs of tools)


ATTN_LEGACY = os.environ.get("M3AE_ATTN_LEGACY", "0") == "1"   # round-3 attention kernels (tests / tools compare the generations)
GEMM_ST_POLICY = int(os.environ.get("M3AE_GEMM_ST_POLICY", 0))   # output-store cache policy selector (0: the kernel's default)
# Weight operand of the NT GEMMs from the tiled copies ParamStore keeps beside the shadows (m3ae_amd/tiled_b.py, M3AE_GEMM_B_TILED):
# bit-identical results.  Read when a ParamStore is built (it allocates the copies) and at every mm_nt / mm_dgrad call.
# On by default: -1.2 % on the step at per-GPU batch 256 (three alternating runs each against the parent commit, DESIGN.md 6e,
# profiles/r09_nt_tiled_weights_ab.log).  M3AE_TILED_B=0 turns it off (A/B runs): no copies are kept, every GEMM reads the shadows.
TILED_B = os.environ.get("M3AE_TILED_B", "1") != "0"


def _gemm_flags():
    return ((1 if NT_NO_PERSISTENT else 0) | (((GEMM_NT_VARIANT + 1) & 0xF) << 8) | (((GEMM_TN_VARIANT + 1) & 0xF) << 12)
            | ((GEMM_COL_GROUP & 0xF) << 16) | ((GEMM_ST_POLICY & 0x3) << 20))
PROFILE = None  # when a list: every GEMM / attention launch is bracketed by HIP events on the launch stream


# fp32x3 mode (compute_dtype="fp32x3"): parity mode's fp32 storage and kernels, with every fp32 GEMM -- the attention products
# included -- on the split-bf16 MFMA kernel (M3AE_GEMM_F32_X3 / M3AE_ATTN_F32_X3, csrc/gemm_f32x3.hip).  The mode is per thread:
# a model's entry points run inside `f32x3_mode(model.f32x3)` (`model_mode`), and every autograd node (`Function`) records the
# mode of its forward and restores it around its backward, which autograd runs on a thread of its own.  A parity-mode model in
# the same process never sees the bits.
class _Mode(threading.local):
    x3 = False


_MODE = _Mode()


@contextlib.contextmanager
def f32x3_mode(on):
    prev, _MODE.x3 = _MODE.x3, bool(on)
    try:
        yield
    finally:
        _MODE.x3 = prev


def f32x3_active():
    return _MODE.x3


def model_mode(fn):
    """Decorator of a model method: run it in the model's GEMM mode (`self.f32x3`)."""
    @functools.wraps(fn)
    def run(self, *args, **kwargs):
        with f32x3_mode(getattr(self, "f32x3", False)):
            return fn(self, *args, **kwargs)
    return run


# Deterministic mode (config key `deterministic`): every reduction of a training step that more than one workgroup feeds -- the
# split-K weight gradients, bias / LayerNorm / embedding gradients, the loss scalars -- takes its ordered form (m3ae_gemm_det and
# the *_det entry points: partials in a workspace, folded in a fixed order) instead of fp32 atomics, so two runs of a step from
# the same state, seeds and masks give the same bits.  The switch is process-wide, like torch.use_deterministic_algorithms
# (autograd runs backward on a thread of its own, and the mode must hold there too), and is read at every call: off (the
# default), no helper below makes one call more than before.  An op that has no ordered form raises DeterministicError when
# its backward is asked with the mode on; it never runs the atomic kernel quietly.
class DeterministicError(_lib.M3AEHipError):
    pass


_DETERMINISTIC = False


def set_deterministic(on):
    global _DETERMINISTIC
    _DETERMINISTIC = bool(on)


def deterministic():
    return _DETERMINISTIC


@contextlib.contextmanager
def deterministic_mode(on=True):
    prev = deterministic()
    set_deterministic(on)
    try:
        yield
    finally:
        set_deterministic(prev)


def _no_ordered_form(op):
    if _DETERMINISTIC:
        raise DeterministicError(f"{op} has no deterministic form (it adds with fp32 atomics) and ops.deterministic() is on: "
                                 f"switch the mode off for this op with ops.set_deterministic(False)")


def _det_ws(nbytes, device):
    """Workspace of a deterministic call: allocated on the caller's stream like every other temporary of the step."""
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _small_ws(op, rows, cols, device):
    n = _lib.lib().m3ae_det_workspace_bytes(op, rows, cols)
    if n < 0:
        check(int(n), "m3ae_det_workspace_bytes")
    return _det_ws(n, device), n


class Function(torch.autograd.Function):
    """torch.autograd.Function whose backward runs in the fp32x3 mode its forward ran in (saved on ctx)."""

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        fwd, bwd = cls.__dict__.get("forward"), cls.__dict__.get("backward")
        if fwd is not None:
            f = fwd.__func__ if isinstance(fwd, staticmethod) else fwd

            def forward(ctx, *args):
                ctx.m3ae_x3 = _MODE.x3
                return f(ctx, *args)
            cls.forward = staticmethod(functools.wraps(f)(forward))
        if bwd is not None:
            b = bwd.__func__ if isinstance(bwd, staticmethod) else bwd

            def backward(ctx, *grads):
                prev, _MODE.x3 = _MODE.x3, getattr(ctx, "m3ae_x3", False)
                try:
                    return b(ctx, *grads)
                finally:
                    _MODE.x3 = prev
            cls.backward = staticmethod(functools.wraps(b)(backward))


def _prof_begin():
    if PROFILE is None:
        return None
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record()
    return e0


def _prof_end(e0, kind, dims):
    if e0 is None:
        return
    e1 = torch.cuda.Event(enable_timing=True)
    e1.record()
    PROFILE.append((kind, dims, e0, e1))


# dropout seeds: every dropout site of every forward call draws a fresh 64-bit seed from this counter stream; the
# site stores it for its backward.  `set_dropout_seed` makes a run reproducible.
_drop_base, _drop_ctr = 0x5EED, 0


def set_dropout_seed(seed):
    global _drop_base, _drop_ctr
    _drop_base, _drop_ctr = int(seed) & 0xFFFFFFFF, 0


# Dropout salt (ABI 3): a device uint32 every dropout kernel folds into its mask key.  None in eager runs (the host draws a fresh
# seed per site and step); graph.GraphedStep points it at its per-replay counter while it captures, so the frozen seeds of the
# captured launches still give new masks at every replay.
DROPOUT_SALT = None


def _salt():
    return None if DROPOUT_SALT is None else C.c_void_p(DROPOUT_SALT.data_ptr())


def next_dropout_seed():
    global _drop_ctr
    _drop_ctr += 1
    return ((_drop_base << 32) | (_drop_ctr & 0xFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF


def dropout_pair(p):
    """(p, fresh seed) of one dropout site; None when the site is inactive (p <= 0)."""
    return (p, next_dropout_seed()) if p > 0 else None


def _set_dropout(d, dropout):
    """dropout = (p, seed) or None into a GEMM / attention descriptor, with the salt of the moment."""
    if dropout is not None and dropout[0] > 0:
        d.dropout_p, d.dropout_seed = dropout
        d.dropout_salt = _salt()


def _dt(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_dev_index = None


def _stream():
    """The caller's current HIP stream as a raw handle.  (torch.cuda.current_stream() builds a Stream object through three
    layers of device-index helpers: 8 us a call, 14 % of the host time of a step at ~1600 calls -- tools/host_profile.py.)"""
    global _dev_index
    if _raw_stream is None:
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if _dev_index is None:
        _dev_index = torch.cuda.current_device()   # one process drives one GPU (bench.py / trainer: torch.cuda.set_device first)
    return C.c_void_p(_raw_stream(_dev_index))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need_cuda(t):
    if not t.is_cuda:
        raise _lib.M3AEHipError("m3ae_amd ops run on the GPU only (no CPU fallback); got a CPU tensor")
    # _stream() hands out the raw current stream of ONE device (the first one an op ran on: one process drives one GPU): a
    # tensor of another device would be launched on that device's stream handle
    if _dev_index is not None and t.device.index != _dev_index:
        raise _lib.M3AEHipError(f"m3ae_amd ops were first used on cuda:{_dev_index}; got a tensor on {t.device} "
                                f"(one process drives one GPU: call torch.cuda.set_device before the first op)")


def compute_weight(w):
    """The tensor a GEMM reads for parameter `w`: its bf16 shadow in perf mode, itself in fp32 mode."""
    return getattr(w, "m3ae_c", w)


# ----------------------------------------------------------------------------------------------------------
# raw GEMM
# ----------------------------------------------------------------------------------------------------------
def gemm(a, a_sm, a_sk, b, b_sk, b_sn, c, c_sm, M, N, K, *, alpha=1.0, accumulate=False, bias=None, act=ACT_NONE,
         preact=None, residual=None, dact_aux=None, dact=ACT_NONE, force_generic=False, batch=(1, 1),
         a_sb=(0, 0), b_sb=(0, 0), c_sb=(0, 0), a_rowsum=None, dropout=None, preact_grad=False, rows=None, b_tiled=False):
    """rows = (row_base, row_step): the dropout mask row of output row m is row_base + m * row_step (m3ae_gemm_rows).
    b_tiled: `b` is the tiled copy (tiled_b.py) of the K-contiguous bf16 weight [N, K]; b_sk = 1 and b_sn = K as for the weight."""
    _need_cuda(c)
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.batch1, d.batch2 = batch
    d.A, d.a_sm, d.a_sk, d.a_sb1, d.a_sb2 = a.data_ptr(), a_sm, a_sk, a_sb[0], a_sb[1]
    d.B, d.b_sk, d.b_sn, d.b_sb1, d.b_sb2 = b.data_ptr(), b_sk, b_sn, b_sb[0], b_sb[1]
    d.C, d.c_sm, d.c_sn, d.c_sb1, d.c_sb2 = c.data_ptr(), c_sm, 1, c_sb[0], c_sb[1]
    d.dtype_a, d.dtype_b, d.dtype_c = _dt(a), _dt(b), _dt(c)
    d.alpha = alpha
    d.accumulate = int(accumulate)
    if bias is not None:
        assert bias.dtype == torch.float32
        d.bias = bias.data_ptr()
    d.act = act
    for name, t in (("preact", preact), ("residual", residual), ("dact_aux", dact_aux)):
        if t is not None:
            assert t.dtype == c.dtype and t.stride(-1) == 1 and t.stride(-2) == c_sm, name
            setattr(d, name, t.data_ptr())
    d.dact = dact
    d.preact_grad = int(preact_grad)
    d.launch_flags = _gemm_flags() | (_lib.GEMM_B_TILED if b_tiled else 0)
    if _MODE.x3 and d.dtype_a == F32 and d.dtype_b == F32 and d.dtype_c == F32:
        d.launch_flags |= _lib.GEMM_F32_X3
    d.force_generic = int(force_generic)
    if a_rowsum is not None:
        assert a_rowsum.dtype == torch.float32 and a_rowsum.numel() >= M and batch == (1, 1)
        d.a_rowsum = a_rowsum.data_ptr()
    _set_dropout(d, dropout)
    e0 = _prof_begin()
    # deterministic mode: a descriptor of the split-K wgrad family (the only GEMM family that adds with atomics) takes the
    # ordered form; the size query is 0 for every other descriptor
    nws = _lib.lib().m3ae_gemm_det_workspace_bytes(C.byref(d)) if _DETERMINISTIC else 0
    if nws > 0:
        d.launch_flags |= _lib.GEMM_DETERMINISTIC
        ws = _det_ws(nws, c.device)
        check(_lib.lib().m3ae_gemm_det(C.byref(d), _p(ws), nws, _stream()), "m3ae_gemm_det")
        del ws
    elif rows is not None:
        check(_lib.lib().m3ae_gemm_rows(C.byref(d), rows[0], rows[1], _stream()), "m3ae_gemm_rows")
    else:
        check(_lib.lib().m3ae_gemm(C.byref(d), _stream()), "m3ae_gemm")
    if e0 is not None:
        _prof_end(e0, "gemm:" + last_gemm_path(), (M, N, K, batch[0] * batch[1]))


def last_gemm_path():
    return _lib.lib().m3ae_last_gemm_path().decode()


def _rows(x):
    """View x [..., K] as 2-D rows (M, K) without copying; returns (tensor2d, M, K, row_stride)."""
    K = x.shape[-1]
    if x.dim() == 2:
        assert x.stride(1) == 1
        return x, x.shape[0], K, x.stride(0)
    if not x.is_contiguous():
        x = x.contiguous()
    x2 = x.view(-1, K)
    return x2, x2.shape[0], K, K


_LAUNCH_STREAM = None


def launch_stream():
    """The process-wide HIGH-priority HIP stream the step is issued on (bench.py, trainer.py).  The model's text half runs on a second,
    normal-priority stream beside the image half (modules/m3ae_module.py); with the caller's stream at high priority the hardware
    dispatches the image kernels' workgroups first and the text kernels fill what they leave -- measured +0.75 / +1.4 % on the step at
    per-GPU batch 256, same box, alternating runs (profiles/r04_launch_stream_priority_ab.log; a high-priority SIDE stream: nothing)."""
    global _LAUNCH_STREAM
    if _LAUNCH_STREAM is None:
        _LAUNCH_STREAM = torch.cuda.Stream(priority=-1)
    return _LAUNCH_STREAM


def use_launch_stream():
    """Make launch_stream() this thread's current stream, ordered behind everything already queued on the device; returns the stream
    that was current (torch.cuda.set_stream(prev) restores it).  M3AE_LAUNCH_PRIORITY=normal keeps the caller's stream (A/B runs)."""
    prev = torch.cuda.current_stream()
    if os.environ.get("M3AE_LAUNCH_PRIORITY", "high") != "high":
        return prev
    torch.cuda.synchronize()
    torch.cuda.set_stream(launch_stream())
    return prev


def mm_nt(x2, ldx, M, w, bias=None, act=ACT_NONE, residual=None, want_preact=False, out_dtype=None, dact_aux=None,
          dact=ACT_NONE, force_generic=False, alpha=1.0, dropout=None, preact_grad=False, rows=None, sl=None):
    """y[M,N] = epi(alpha * x2[M,K] . w[N,K]^T).  want_preact + preact_grad: the second output is act'(pre-activation)
    (consumed by a backward GEMM with dact=ACT_MULAUX) instead of the pre-activation itself.  sl: a slice of the rows of w
    and of bias (the Q or the K | V part of a packed projection): read in place with the weight's strides, never from the
    tiled copy -- also when the slice is the whole range."""
    if sl is not None:
        w, bias = w[sl], None if bias is None else bias[sl]
    N, K = w.shape
    y = torch.empty((M, N), dtype=out_dtype or x2.dtype, device=x2.device)
    pre = torch.empty_like(y) if want_preact else None
    tb = getattr(w, "m3ae_tb", None) if TILED_B and sl is None and x2.dtype == torch.bfloat16 and w.stride(0) == K else None
    gemm(x2, ldx, 1, w if tb is None else tb, 1, w.stride(0), y, N, M, N, K, bias=bias, act=act, preact=pre, residual=residual,
         dact_aux=dact_aux, dact=dact, force_generic=force_generic, alpha=alpha, dropout=dropout,
         preact_grad=preact_grad and want_preact, rows=rows, b_tiled=tb is not None)
    return y, pre


def mm_dgrad(dy, w_param, dact_aux=None, dact=ACT_NONE, residual=None, alpha=1.0, dropout=None, out=None, ld_out=None, rows=None,
             sl=None):
    """dx[M,K] = dy[M,N] . W[N,K]  (bf16: NT against the transposed shadow; fp32: strided generic).  out / ld_out: write
    the rows into this preallocated tensor at this row stride instead of a fresh [M, K].  sl: W = rows `sl` of the parameter
    (columns of its transposed shadow), as in mm_nt."""
    M, N = dy.shape
    wt = getattr(w_param, "m3ae_t", None)
    wtt = getattr(w_param, "m3ae_tt", None) if TILED_B and sl is None and wt is not None and dy.dtype == torch.bfloat16 else None
    if wtt is not None:   # the tiled copy of the transposed shadow [K, N]: row length N
        b, b_sk, b_sn, K = wtt, 1, N, wt.shape[0]
    elif wt is not None:
        b, b_sk, b_sn, K = (wt if sl is None else wt[:, sl]), 1, wt.stride(0), wt.shape[0]
    else:
        b = compute_weight(w_param) if sl is None else compute_weight(w_param)[sl]
        b_sk, b_sn, K = b.stride(0), 1, b.shape[1]
    if out is None:
        out, ld_out = torch.empty((M, K), dtype=dy.dtype, device=dy.device), K
    gemm(dy, dy.stride(0), 1, b, b_sk, b_sn, out, ld_out, M, K, N, dact_aux=dact_aux, dact=dact, residual=residual,
         alpha=alpha, dropout=dropout, rows=rows, b_tiled=wtt is not None)
    return out


def mm_wgrad(dy, x2, ldx, w_param, b_param=None, alpha=1.0, sl=None):
    """w.grad[N,K] += dy[M,N]^T . x2[M,K]  (fp32 accumulate in place); with b_param also b.grad[N] += colsum(dy),
    fused into the same kernel (row sums of the A operand dy^T).  sl: into rows `sl` of both gradients; the parameters are
    then NOT reported done: the caller does that (_done) once all slices of a parameter are in."""
    want_b = b_param is not None and b_param.requires_grad
    gb = None if not want_b else _grad_buf(b_param) if sl is None else _grad_buf(b_param)[sl]
    if not w_param.requires_grad:
        if want_b:
            colsum(dy, gb, True)
    else:
        g = _grad_buf(w_param) if sl is None else _grad_buf(w_param)[sl]
        M, N = dy.shape
        gemm(dy, 1, dy.stride(0), x2, ldx, 1, g, g.stride(0), N, g.shape[1], M, accumulate=True, alpha=alpha, a_rowsum=gb)
    if sl is None:
        if w_param.requires_grad:
            _done(w_param)
        if want_b:
            _done(b_param)


def colsum(x, out, accumulate):
    """out[n] (+)= sum_m x[m][n]; the ordered form in deterministic mode."""
    M, N = x.shape
    if _DETERMINISTIC:
        ws, n = _small_ws(_lib.DET_COLSUM, M, N, x.device)
        check(_lib.lib().m3ae_colsum_det(_p(x), _p(out), M, N, x.stride(0), _dt(x), int(accumulate), _p(ws), n, _stream()),
              "m3ae_colsum_det")
        return
    check(_lib.lib().m3ae_colsum(_p(x), _p(out), M, N, x.stride(0), _dt(x), int(accumulate), _stream()), "m3ae_colsum")


def act_bwd(dy, pre, act):
    dx = torch.empty_like(dy)
    check(_lib.lib().m3ae_act_bwd(_p(dy), _p(pre), _p(dx), dy.numel(), act, _dt(dy), _stream()), "m3ae_act_bwd")
    return dx


# ----------------------------------------------------------------------------------------------------------
# Linear / MLP
# ----------------------------------------------------------------------------------------------------------
def _members(p):
    return getattr(p, "members", None) or ([p] if p is not None else [])


def _done(p):
    if grad_ready_hook is not None and p is not None:
        for m in _members(p):
            grad_ready_hook(m)


def _grad_buf(p):
    if getattr(p, "members", None) is not None:  # PackedParam: members' grads are adjacent views of the flat buffer
        g = p.grad
        if g is None:
            raise _lib.M3AEHipError("packed parameters need ParamStore-managed gradients")
        return g
    if p.grad is None:
        p.grad = torch.zeros_like(p, dtype=torch.float32)
    return p.grad


def add(a, b, out=None):
    """out = a + b on the library's streaming add (same shape / dtype, contiguous)."""
    _need_cuda(a)
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty_like(a) if out is None else out
    check(_lib.lib().m3ae_add(_p(a), _p(b), _p(out), a.numel(), _dt(a), _stream()), "m3ae_add")
    return out


def cast(x, dtype):
    """x in `dtype` on the library's streaming cast (fp32 -> bf16 rounds to nearest even); x itself when it already is."""
    if x.dtype == dtype:
        return x
    _need_cuda(x)
    x = x.contiguous()
    out = torch.empty_like(x, dtype=dtype)
    check(_lib.lib().m3ae_cast(_p(x), _p(out), x.numel(), _dt(x), _dt(out), _stream()), "m3ae_cast")
    return out


class Fork2Fn(Function):
    """Identity with two outputs for a tensor that feeds two consumers (a fusion layer's x / y feed the text layer AND the image
    layer of the pair, m3ae_module.py:269-278): the two gradients meet here and are summed by the library's add instead of by
    autograd's accumulation (12 ATen adds per step in round 3).  Runs on the stream of its forward, i.e. the producer's."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None:
            return gb
        if gb is None:
            return ga
        return add(ga, gb)


def fork2(x):
    return Fork2Fn.apply(x) if (x.requires_grad and torch.is_grad_enabled()) else (x, x)


class LinearFn(Function):
    """y = act(x W^T + b + extra_bias) (+ residual).  nn.Linear sites of clip_model.py / bert_model.py /
    m3ae_module.py.  `weight` / `bias` are Parameters or PackedParams; `anchors` are the underlying Parameters of a
    PackedParam (graph recording only)."""

    @staticmethod
    def forward(ctx, x, residual, extra_bias, weight, bias, act, alpha, *anchors):
        x2, M, K, ldx = _rows(x)
        w = compute_weight(weight)
        b = None if bias is None else (bias.data if hasattr(bias, "members") else bias.detach())
        if extra_bias is not None:  # e.g. + modality_type_embeddings row (m3ae_module.py:260-263)
            b = extra_bias.detach().float() if b is None else b + extra_bias.detach().float()
        res2 = None
        if residual is not None:
            res2 = residual.contiguous().view(M, -1)
        # a residual of another dtype than x (the fp32 stream of a bf16 CLIP tower) sets the output's dtype: the join stays in it
        y, pre = mm_nt(x2, ldx, M, w, bias=b, act=act, residual=res2, want_preact=(act != ACT_NONE), alpha=alpha,
                       out_dtype=None if res2 is None else res2.dtype)
        ctx.save_for_backward(x2, pre)
        ctx.weight, ctx.bias, ctx.act, ctx.ldx, ctx.alpha = weight, bias, act, ldx, alpha
        ctx.x_shape, ctx.has_res = x.shape, residual is not None
        ctx.x_needs = x.requires_grad
        ctx.extra_needs = extra_bias is not None and extra_bias.requires_grad
        ctx.n_anchor = len(anchors)
        return y.view(*x.shape[:-1], y.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        x2, pre = ctx.saved_tensors
        N = dy.shape[-1]
        dy2 = cast(dy.contiguous().view(-1, N), x2.dtype)   # (a cast only below an fp32 residual join of bf16 operands)
        dres = dy if ctx.has_res else None
        dz = act_bwd(dy2, pre, ctx.act) if ctx.act != ACT_NONE else dy2
        dextra = None
        dx = None
        if ctx.x_needs:   # before the weight gradient reports the parameter: an optimizer-in-backward update of this weight's
            dx = mm_dgrad(dz, ctx.weight, alpha=ctx.alpha).view(ctx.x_shape)   # bucket is then ordered behind this read of it
        if ctx.extra_needs:
            mm_wgrad(dz, x2, ctx.ldx, ctx.weight, alpha=ctx.alpha)
            dextra = torch.empty(N, dtype=torch.float32, device=dz.device)
            colsum(dz, dextra, False)
            if ctx.bias is not None and ctx.bias.requires_grad:
                _grad_buf(ctx.bias).add_(dextra)
                _done(ctx.bias)
        else:
            mm_wgrad(dz, x2, ctx.ldx, ctx.weight, ctx.bias, alpha=ctx.alpha)
        return (dx, dres, dextra, None, None, None, None) + (None,) * ctx.n_anchor


class GatherLinearFn(Function):
    """y = act(x[:, 0] W^T + b): Pooler (prediction_heads.py:15-18).  The token-0 rows are addressed in place
    through the GEMM's row stride; the backward scatters into a zeroed [B, L, D] gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        B, L, D = x.shape
        xc = x.contiguous()
        w = compute_weight(weight)
        y, pre = mm_nt(xc, L * D, B, w, bias=bias, act=act, want_preact=(act != ACT_NONE))
        ctx.save_for_backward(xc, pre)
        ctx.weight, ctx.bias, ctx.act = weight, bias, act
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, pre = ctx.saved_tensors
        B, L, D = xc.shape
        dy2 = dy.contiguous()
        dz = act_bwd(dy2, pre, ctx.act) if ctx.act != ACT_NONE else dy2
        mm_wgrad(dz, xc, L * D, ctx.weight, ctx.bias)
        dx = mm_dgrad(dz, ctx.weight, out=torch.zeros_like(xc), ld_out=L * D)
        return dx, None, None, None


class MLPFn(Function):
    """y = act(x W1^T + b1) W2^T + b2 (+ residual).  BertIntermediate + BertOutput.dense (bert_model.py:416-440)
    and the CLIP mlp (clip_model.py:46-50).  The activation derivative is fused into the dgrad GEMM's epilogue."""

    @staticmethod
    def forward(ctx, x, residual, w1, b1, w2, b2, act):
        x2, M, K, ldx = _rows(x)
        g, u = mm_nt(x2, ldx, M, compute_weight(w1), bias=b1, act=act, want_preact=True, preact_grad=SAVE_DACT)
        res2 = residual.contiguous().view(M, -1) if residual is not None else None
        y, _ = mm_nt(g, g.stride(0), M, compute_weight(w2), bias=b2, residual=res2, out_dtype=None if res2 is None else res2.dtype)
        ctx.save_for_backward(x2, u, g)
        ctx.p = (w1, b1, w2, b2)
        ctx.act, ctx.ldx, ctx.x_shape, ctx.has_res = act, ldx, x.shape, residual is not None
        return y.view(*x.shape[:-1], y.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        x2, u, g = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.p
        dy2 = cast(dy.contiguous().view(-1, dy.shape[-1]), g.dtype)
        dres = dy if ctx.has_res else None
        mm_wgrad(dy2, g, g.stride(0), w2, b2)
        du = mm_dgrad(dy2, w2, dact_aux=u, dact=ACT_MULAUX if SAVE_DACT else ctx.act)  # dU = (dY W2) * act'(U), act'(U) saved by the forward
        mm_wgrad(du, x2, ctx.ldx, w1, b1)
        dx = mm_dgrad(du, w1).view(ctx.x_shape)
        return dx, dres, None, None, None, None, None


def linear(x, weight, bias=None, act=ACT_NONE, residual=None, extra_bias=None, alpha=1.0):
    anchors = tuple(_members(weight)) if hasattr(weight, "members") else ()
    if hasattr(bias, "members"):
        anchors = anchors + tuple(bias.members)
    return LinearFn.apply(x, residual, extra_bias, weight, bias, act, alpha, *anchors)


def mlp(x, w1, b1, w2, b2, act, residual=None):
    return MLPFn.apply(x, residual, w1, b1, w2, b2, act)


# ----------------------------------------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------------------------------------
class LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, act, rms, out_dtype=None):
        xc = x.contiguous()
        ln = (gamma, beta, eps)
        y, mean, rstd = ln_fwd_raw(xc.view(-1, xc.shape[-1]), ln, act, rms, out_dtype, rms_mean=True)
        ctx.save_for_backward(xc, mean, rstd)
        ctx.ln, ctx.act, ctx.rms = ln, act, rms
        return y.view(xc.shape)

    @staticmethod
    def backward(ctx, dy):
        xc, mean, rstd = ctx.saved_tensors
        D = xc.shape[-1]
        # (train=True: the op accumulates into the gamma / beta it was given, whatever their requires_grad)
        dx = ln_bwd_raw(dy.contiguous().view(-1, D), xc.view(-1, D), ctx.ln, mean, rstd, act=ctx.act, rms=ctx.rms, train=True)
        return dx.view(xc.shape), None, None, None, None, None, None


def layer_norm(x, gamma, beta, eps, act=ACT_NONE, rms=False, out_dtype=None):
    """out_dtype=torch.bfloat16 on fp32 rows: the LayerNorm between an fp32 residual stream and bf16 GEMM operands (the fp32
    kernel's arithmetic, rounded once; its backward takes the bf16 gradient and returns the fp32 one)."""
    return LayerNormFn.apply(x, gamma, beta, eps, act, rms, out_dtype)


def _ln_mixed_ok(x, y, act, rms):
    if not (x.dtype == torch.float32 and y.dtype == torch.bfloat16 and act == ACT_NONE and not rms):
        raise _lib.M3AEHipError(f"LayerNorm from {x.dtype} rows to {y.dtype} rows: only plain LayerNorm from float32 to bfloat16 "
                                "has a kernel")


# ----------------------------------------------------------------------------------------------------------
# raw LayerNorm helpers (no autograd): the fused block functions and LayerNormFn.  The ONE place that picks a LayerNorm entry
# point of the library.  `ln`: a LayerNorm module (weight, bias, eps) or the triple (gamma, beta, eps) itself.
# ----------------------------------------------------------------------------------------------------------
def _ln_params(ln):
    return ln if isinstance(ln, tuple) else (ln.weight, ln.bias, ln.eps)


def ln_fwd_raw(x2, ln, act=ACT_NONE, rms=False, out_dtype=None, rms_mean=False):
    """(y, mean, rstd) of rows x2 [M, D].  rms: no mean is kept (None), unless rms_mean (LayerNormFn hands the kernel a buffer
    all the same)."""
    M, D = x2.shape
    gamma, beta, eps = _ln_params(ln)
    y = torch.empty_like(x2, dtype=out_dtype or x2.dtype)
    mean = None if rms and not rms_mean else torch.empty(M, dtype=torch.float32, device=x2.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x2.device)
    head = (_p(x2), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), M, D, eps)
    if y.dtype != x2.dtype:   # fp32 rows -> bf16 rows (the fp32 residual stream of a bf16 CLIP tower)
        _ln_mixed_ok(x2, y, act, rms)
        check(_lib.lib().m3ae_layernorm_fwd_mixed(*head, _stream()), "LayerNorm forward (mixed form)")
    else:
        check(_lib.lib().m3ae_layernorm_fwd(*head, _dt(x2), act, int(rms), _stream()), "LayerNorm forward")
    return y, mean, rstd


# The backward's choice.  form: (atomic entry, ordered entry -- None: there is none --, the call's label in an error, the entry's
# arguments between (dy, x, gamma) and the stream, by the names ln_bwd_raw gives them).
_LN_DROP_ARGS = "beta mean rstd dx second p seed salt dgamma dbeta ws M D dtype".split()
_LN_BWD = {
    "plain": ("m3ae_layernorm_bwd", "m3ae_layernorm_bwd_det", "LayerNorm backward",
              "beta mean rstd dx dx_add dgamma dbeta ws M D dtype act rms".split()),
    "drop": ("m3ae_layernorm_bwd_drop", "m3ae_layernorm_bwd_drop_det", "LayerNorm backward (dropout form)", _LN_DROP_ARGS),
    "rows": ("m3ae_layernorm_bwd_drop_rows", None, "LayerNorm backward (dropout form)", _LN_DROP_ARGS + ["row_base", "row_step"]),
    "mixed": ("m3ae_layernorm_bwd_mixed", "m3ae_layernorm_bwd_mixed_det", "LayerNorm backward (mixed form)",
              "mean rstd dx dx_add second dgamma dbeta ws M D".split()),
}


def ln_bwd_raw(dy, x2, ln, mean, rstd, dx_add=None, act=ACT_NONE, rms=False, drop=None, rows=None, want_lo=False, train=None):
    """dx = LN'(dy) (+ dx_add); gamma.grad / beta.grad accumulate in place (train: whether they do; default gamma.requires_grad).
    With drop = (p, seed) returns (dx, dx_drop): dx_drop is dx under the dropout mask of the dense layer that fed this LayerNorm,
    rows = (row_base, row_step) the row map of that mask.  bf16 dy on fp32 x2 (the fp32 residual stream of a bf16 CLIP tower): dx
    and dx_add are fp32, and want_lo returns (dx, dx rounded to bf16).
    The entry point is the atomic or the ordered one (deterministic mode) of the form's row in _LN_BWD; a row map in deterministic
    mode has none and raises DeterministicError."""
    M, D = x2.shape
    gamma, beta, eps = _ln_params(ln)
    drop = drop if drop is not None and drop[0] > 0 else None
    mixed = dy.dtype != x2.dtype
    # (only the dropout mask has rows to map)
    form = ("drop" if rows is None else "rows") if drop is not None else "mixed" if mixed else "plain"
    atomic, ordered, label, names = _LN_BWD[form]
    if ordered is None:
        _no_ordered_form("the LayerNorm backward under a dropout row map (the live-row form)")
    if form in ("drop", "rows"):
        assert dx_add is None and act == ACT_NONE and not rms and not mixed and not want_lo
    elif form == "mixed":
        _ln_mixed_ok(x2, dy, act, rms)
        assert dx_add is None or dx_add.dtype == torch.float32
    else:
        assert not want_lo
    L = _lib.lib()
    fn = getattr(L, ordered if _DETERMINISTIC else atomic)
    dx = torch.empty_like(x2)
    ws = torch.empty(2 * L.m3ae_layernorm_bwd_blocks(M) * D, dtype=torch.float32, device=x2.device)
    train = gamma.requires_grad if train is None else train
    gg = _grad_buf(gamma) if train else None
    gb = _grad_buf(beta) if (train and beta is not None) else None
    # the second output: dx under the dropout mask, or dx rounded to bf16
    second = torch.empty_like(x2) if drop is not None else torch.empty_like(dy) if want_lo else None
    p, seed = drop or (None, None)
    row_base, row_step = rows or (None, None)
    a = dict(beta=_p(beta), mean=_p(mean), rstd=_p(rstd), dx=_p(dx), dx_add=_p(dx_add), second=_p(second), p=p, seed=seed, salt=_salt(),
             dgamma=_p(gg), dbeta=_p(gb), ws=_p(ws), M=M, D=D, dtype=_dt(x2), act=act, rms=int(rms), row_base=row_base, row_step=row_step)
    check(fn(_p(dy), _p(x2), _p(gamma), *(a[n] for n in names), _stream()), label)
    if train:
        _done(gamma)
        _done(beta)
    return (dx, second) if (drop is not None or want_lo) else dx


# ----------------------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------------------
def _attn_desc(B, H, Lq, Lk, Dh, q, k, v, o, key_mask, pos_bias, scale, causal, lse, lse_stride, dtype):
    d = AttnDesc()
    d.B, d.H, d.Lq, d.Lk, d.Dh = B, H, Lq, Lk, Dh
    d.q, d.q_sb, d.q_sl = q.data_ptr(), q.stride(0), q.stride(1)
    d.k, d.k_sb, d.k_sl = k.data_ptr(), k.stride(0), k.stride(1)
    d.v, d.v_sb, d.v_sl = v.data_ptr(), v.stride(0), v.stride(1)
    d.o, d.o_sb, d.o_sl = o.data_ptr(), o.stride(0), o.stride(1)
    d.key_mask = key_mask.data_ptr() if key_mask is not None else None
    d.pos_bias = pos_bias.data_ptr() if pos_bias is not None else None
    d.scale, d.causal = scale, int(causal)
    d.lse = lse.data_ptr() if lse is not None else None
    d.lse_stride = lse_stride
    d.dtype = dtype
    d.launch_flags = _lib.ATTN_LEGACY_KERNELS if ATTN_LEGACY else 0
    if _MODE.x3 and dtype == F32:
        d.launch_flags |= _lib.ATTN_F32_X3
    return d


def _attn_ws(d, backward, device):
    n = _lib.lib().m3ae_attn_workspace_bytes(C.byref(d), int(backward))
    if n <= 0:
        return None
    ws = torch.empty(n, dtype=torch.uint8, device=device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), n
    return ws


def attn_forward(q, k, v, heads, key_mask=None, pos_bias=None, scale=None, causal=False, dropout=None, rows=None):
    """q [B,Lq,D] / k,v [B,Lk,D] (last dim contiguous, any batch/token strides) -> o [B,Lq,D], lse.
    rows = (row_base, row_step): row map of the probability-dropout mask (m3ae_attn_fwd_rows)."""
    _need_cuda(q)
    B, Lq, D = q.shape
    Lk = k.shape[1]
    Dh = D // heads
    if q.dtype == torch.bfloat16 and Dh != 64:
        # the MFMA attention kernels are specialised for 64-wide heads; other widths (the decoder head's 96) take the fp32
        # materialised-softmax kernels on fp32 copies of the projections: short sequences, a few % of that head's work
        o32, lse = attn_forward(q.float(), k.float(), v.float(), heads, key_mask, pos_bias, scale, causal, dropout, rows)
        return o32.to(torch.bfloat16), lse
    scale = (1.0 / math.sqrt(Dh)) if scale is None else scale
    o = torch.empty((B, Lq, D), dtype=q.dtype, device=q.device)
    lse_stride = (Lq + 31) // 32 * 32
    # bf16 kernels write every row of the table, padding rows (>= Lq) included; the fp32 path leaves it untouched
    lse = (torch.empty if q.dtype == torch.bfloat16 else torch.zeros)((B, heads, lse_stride), dtype=torch.float32, device=q.device)
    d = _attn_desc(B, heads, Lq, Lk, Dh, q, k, v, o, key_mask, pos_bias, scale, causal, lse, lse_stride, _dt(q))
    _set_dropout(d, dropout)
    ws = _attn_ws(d, False, q.device)
    e0 = _prof_begin()
    if rows is not None:
        check(_lib.lib().m3ae_attn_fwd_rows(C.byref(d), rows[0], rows[1], _stream()), "m3ae_attn_fwd_rows")
    else:
        check(_lib.lib().m3ae_attn_fwd(C.byref(d), _stream()), "m3ae_attn_fwd")
    _prof_end(e0, "attn_fwd", (B, heads, Lq, Lk, Dh))
    del ws
    return o, lse


def attn_backward(q, k, v, o, lse, do, dq, dk, dv, heads, key_mask=None, pos_bias=None, scale=None, causal=False,
                  d_pos_bias=None, dropout=None, rows=None):
    if d_pos_bias is not None:
        _no_ordered_form("the relative-position-bias gradient of m3ae_attn_bwd (d_pos_bias, T5 attention)")
    B, Lq, D = q.shape
    Lk = k.shape[1]
    Dh = D // heads
    if q.dtype == torch.bfloat16 and Dh != 64:   # fp32 detour, as in attn_forward
        f = [t.float() for t in (q, k, v, o, do)]
        g = [torch.empty_like(t) for t in f[:3]]
        attn_backward(f[0], f[1], f[2], f[3].contiguous(), lse, f[4].contiguous(), g[0], g[1], g[2], heads, key_mask,
                      pos_bias, scale, causal, d_pos_bias, dropout, rows)
        for dst, src in zip((dq, dk, dv), g):
            dst.copy_(src)
        return
    scale = (1.0 / math.sqrt(Dh)) if scale is None else scale
    assert do.stride() == o.stride() and dq.stride() == q.stride() and dk.stride() == k.stride() and dv.stride() == v.stride()
    d = _attn_desc(B, heads, Lq, Lk, Dh, q, k, v, o, key_mask, pos_bias, scale, causal, lse, lse.shape[-1], _dt(q))
    # rows Lq .. lse_stride-1 are padding and must stay finite (0 * NaN in the dK/dV tile): the dQ kernel writes them as 0
    delta = torch.empty_like(lse) if q.dtype == torch.bfloat16 else torch.zeros_like(lse)
    d.d_o, d.dq, d.dk, d.dv, d.delta = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
    d.d_pos_bias = d_pos_bias.data_ptr() if d_pos_bias is not None else None
    _set_dropout(d, dropout)
    ws = _attn_ws(d, True, q.device)
    e0 = _prof_begin()
    if rows is not None:
        check(_lib.lib().m3ae_attn_bwd_rows(C.byref(d), rows[0], rows[1], _stream()), "m3ae_attn_bwd_rows")
    else:
        check(_lib.lib().m3ae_attn_bwd(C.byref(d), _stream()), "m3ae_attn_bwd")
    _prof_end(e0, "attn_bwd", (B, heads, Lq, Lk, Dh))
    del ws, delta


def attn_probs(q, k, lse, heads, key_mask=None, scale=None, dropout=None):
    """The attention probabilities of the attn_forward call that returned `lse` for these q / k (same heads, mask, scale and
    dropout = (p, seed)): fp32 [B, H, Lq, Lk], contiguous (m3ae_attn_probs).  Under dropout: the dropped and rescaled P that
    multiplied V (bert_model.py:334).  A fresh tensor outside autograd (the reference's hook on the maps is disabled, :328)."""
    _need_cuda(q)
    B, Lq, D = q.shape
    Lk = k.shape[1]
    Dh = D // heads
    if q.dtype == torch.bfloat16 and Dh != 64:   # attn_forward's fp32 detour: its softmax is recomputed in fp32
        return attn_probs(q.float(), k.float(), None, heads, key_mask, scale, dropout)
    scale = (1.0 / math.sqrt(Dh)) if scale is None else scale
    out = torch.empty((B, heads, Lq, Lk), dtype=torch.float32, device=q.device)
    lse_stride = lse.shape[-1] if lse is not None else 0
    d = _attn_desc(B, heads, Lq, Lk, Dh, q, k, k, q, key_mask, None, scale, False, lse, lse_stride, _dt(q))
    _set_dropout(d, dropout)
    e0 = _prof_begin()
    check(_lib.lib().m3ae_attn_probs(C.byref(d), C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1), out.stride(2),
                                     _stream()), "m3ae_attn_probs")
    _prof_end(e0, "attn_probs", (B, heads, Lq, Lk, Dh))
    return out


def attn_colmean(q, k, lse, heads, key_mask=None, scale=None, dropout=None):
    """The received attention of the attn_forward call that returned `lse` for these q / k: the mean over heads and queries of the
    map attn_probs returns for the same arguments, fp32 [B, Lk], formed without the map (m3ae_attn_colmean).  A fresh tensor
    outside autograd."""
    _need_cuda(q)
    B, Lq, D = q.shape
    Lk = k.shape[1]
    Dh = D // heads
    if q.dtype == torch.bfloat16 and Dh != 64:   # attn_probs' fp32 detour
        return attn_colmean(q.float(), k.float(), None, heads, key_mask, scale, dropout)
    scale = (1.0 / math.sqrt(Dh)) if scale is None else scale
    out = torch.empty((B, Lk), dtype=torch.float32, device=q.device)
    lse_stride = lse.shape[-1] if lse is not None else 0
    d = _attn_desc(B, heads, Lq, Lk, Dh, q, k, k, q, key_mask, None, scale, False, lse, lse_stride, _dt(q))
    _set_dropout(d, dropout)
    L = _lib.lib()
    n = L.m3ae_attn_colmean_workspace_bytes(C.byref(d))
    ws = torch.empty(n, dtype=torch.uint8, device=q.device)
    e0 = _prof_begin()
    check(L.m3ae_attn_colmean(C.byref(d), C.c_void_p(out.data_ptr()), out.stride(0), C.c_void_p(ws.data_ptr()), n, _stream()),
          "m3ae_attn_colmean")
    _prof_end(e0, "attn_colmean", (B, heads, Lq, Lk, Dh))
    del ws
    return out


def heatmap_upsample(recv, size):
    """Bilinear upsample (align_corners=False) of patch grids to [B, size, size] fp32 (m3ae_heatmap_upsample).  recv: fp32
    [B, g, g], or a [B, g * g] view with unit stride along the tokens -- such as recv[:, 1:] of a [B, 1 + g * g] summary, whose
    class token is then skipped without a copy."""
    _need_cuda(recv)
    if recv.dtype != torch.float32:
        raise ValueError(f"heatmap_upsample takes fp32 grids, got {recv.dtype}")
    if recv.dim() == 3:
        if recv.shape[1] != recv.shape[2]:
            raise ValueError(f"heatmap_upsample takes square grids, got {tuple(recv.shape)}")
        recv = recv.reshape(recv.shape[0], -1)
    B, n = recv.shape
    g = math.isqrt(n)
    if g * g != n or g < 1:
        raise ValueError(f"heatmap_upsample: {n} tokens are not a square grid")
    size = int(size)
    if size < 1:
        raise ValueError(f"heatmap_upsample: size {size}")
    if recv.stride(1) != 1 or (B > 1 and recv.stride(0) < n):
        recv = recv.contiguous()
    out = torch.empty((B, size, size), dtype=torch.float32, device=recv.device)
    check(_lib.lib().m3ae_heatmap_upsample(C.c_void_p(recv.data_ptr()), max(recv.stride(0), n), g, C.c_void_p(out.data_ptr()), B, size,
                                           _stream()), "m3ae_heatmap_upsample")
    return out


class SelfAttnFn(Function):
    """softmax(QK^T / sqrt(dh) + mask) V on a packed [B, L, 3D] projection (rows Q | K | V)."""

    @staticmethod
    def forward(ctx, qkv, key_mask, heads, dropout=None, causal=False):
        D = qkv.shape[-1] // 3
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        o, lse = attn_forward(q, k, v, heads, key_mask, dropout=dropout, causal=causal)
        ctx.save_for_backward(qkv, o, lse, key_mask)
        ctx.heads, ctx.dropout, ctx.causal = heads, dropout, causal
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, key_mask = ctx.saved_tensors
        D = qkv.shape[-1] // 3
        dqkv = torch.empty_like(qkv)
        attn_backward(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], o, lse, do.contiguous(), dqkv[..., :D],
                      dqkv[..., D:2 * D], dqkv[..., 2 * D:], ctx.heads, key_mask, dropout=ctx.dropout, causal=ctx.causal)
        return dqkv, None, None, None, None


class CrossAttnFn(Function):
    """Q from this stream [B, Lq, D]; packed K | V [B, Lk, 2D] from the other stream (bert_model.py:275-278)."""

    @staticmethod
    def forward(ctx, q, kv, key_mask, heads, dropout=None):
        D = q.shape[-1]
        o, lse = attn_forward(q, kv[..., :D], kv[..., D:], heads, key_mask, dropout=dropout)
        ctx.save_for_backward(q, kv, o, lse, key_mask)
        ctx.heads, ctx.dropout = heads, dropout
        return o

    @staticmethod
    def backward(ctx, do):
        q, kv, o, lse, key_mask = ctx.saved_tensors
        D = q.shape[-1]
        # same strides as the (possibly sliced) inputs: the kernels address dq / dk / dv with the q / k / v strides
        dq = torch.empty_strided(q.shape, q.stride(), dtype=q.dtype, device=q.device)
        dkv = torch.empty_strided(kv.shape, kv.stride(), dtype=kv.dtype, device=kv.device)
        attn_backward(q, kv[..., :D], kv[..., D:], o, lse, do.contiguous(), dq, dkv[..., :D], dkv[..., D:], ctx.heads,
                      key_mask, dropout=ctx.dropout)
        return dq, dkv, None, None, None


def self_attention(qkv, key_mask, heads, dropout=None, causal=False):
    """dropout = (p, seed): attention-probability dropout (mask rows (b*H + h)*Lq + q, columns k)."""
    return SelfAttnFn.apply(qkv, key_mask, heads, dropout, causal)


def cross_attention(q, kv, key_mask, heads, dropout=None):
    return CrossAttnFn.apply(q, kv, key_mask, heads, dropout)


# ----------------------------------------------------------------------------------------------------------
# fused transformer blocks: ONE autograd node per block, hand-written backward, every gradient join of the block
# (residual branches) folded into a dgrad-GEMM or LayerNorm-backward epilogue -- no autograd add / copy kernels.
# `P` is a plain namespace of parameter references built by the module (m3ae_amd/modules/*); `anchors` are the same
# parameters as tensors so that autograd records the node.
# ----------------------------------------------------------------------------------------------------------
def _bdata(b):
    return None if b is None else (b.data if hasattr(b, "members") else b.detach())


# the fused cross-attention sub-block (csrc/xattn.hip, csrc/xflash.hip): "auto" = whenever the shapes are covered AND absorbing
# the long side's projection saves work (heads x text tokens < hidden width: 32 text tokens; at 64 the absorbed products are as
# large as the projections they replace and the fused path measures SLOWER than the composition -- forward 459 vs 331 us,
# training +25 %, profiles/r03_xattn_T64_fused_vs_composition.log); "always" = whenever covered (tests, tools); "off" = always the
# composition q / kv GEMM + flash attention + output GEMM + LayerNorm
XATTN = os.environ.get("M3AE_XATTN", "auto")
# training (a backward will be asked): "auto" = fused forward + fused backward, "off" = the composition
XATTN_TRAIN = os.environ.get("M3AE_XATTN_TRAIN", "auto")
# ... from this per-call batch on: measured on one MI355X (profiles/r02_xattn_batch_rule.log), fused forward + backward
# against the composition per sub-block: B = 32 +25..30 % slower, B = 64 +9..13 % slower, B = 128 8..12 % faster, B = 256
# 11..12 % faster -- the per-sample products of the absorbed form need the batch to fill the chip
XATTN_TRAIN_MIN_BATCH = int(os.environ.get("M3AE_XATTN_TRAIN_MIN_BATCH", 96))
# A/B measurements (tools/, tests): the round-2 dir-1 forward chain (P through HBM) instead of the one-launch kernel
XATTN_LEGACY_CHAIN = False
# CLS-head steps (VQA, ITM) read token 0 of the last fusion pair's outputs only: with the switch on, infer(cls_only=True) runs that
# pair on its live rows (BertCrossLayerFn's live-row form below); M3AE_CLS_ONLY=0 restores the full computation (tests, A/B runs)
CLS_ONLY = os.environ.get("M3AE_CLS_ONLY", "1") != "0"


def _xattn_desc(h2, B, L, other2, Lo, mask, P, pdrop, seeds):
    D = h2.shape[1]
    d = XattnDesc()
    d.dir = 0 if L <= Lo else 1
    d.B, d.Lq, d.Lk, d.D, d.H = B, L, Lo, D, P.heads
    d.x, d.y = h2.data_ptr(), other2.data_ptr()
    d.key_mask = mask.data_ptr() if mask is not None else None
    wq, wkv, wo = P.w_q, P.w_kv, P.w_o
    d.wq, d.wkv, d.wo = compute_weight(wq).data_ptr(), compute_weight(wkv).data_ptr(), compute_weight(wo).data_ptr()
    d.wq_t, d.wkv_t, d.wo_t = wq.m3ae_t.data_ptr(), wkv.m3ae_t.data_ptr(), wo.m3ae_t.data_ptr()
    d.bq, d.bkv, d.bo = _bdata(P.b_q).data_ptr(), _bdata(P.b_kv).data_ptr(), _bdata(P.b_o).data_ptr()
    d.ln_g, d.ln_b, d.ln_eps = P.ln.weight.data_ptr(), P.ln.bias.data_ptr(), P.ln.eps
    if pdrop > 0:
        d.dropout_p, d.seed_attn, d.seed_hidden = pdrop, seeds[0], seeds[1]
        d.dropout_salt = _salt()
    d.launch_flags = (_lib.XATTN_NO_PERSISTENT if NT_NO_PERSISTENT else 0) | (_lib.XATTN_LEGACY_CHAIN if XATTN_LEGACY_CHAIN else 0)
    return d


def xattn_supported(h2, L, other2, Lo, mask, P, backward=False):
    """The fused sub-block covers these shapes (forward); backward=True: and m3ae_xattn_bwd does, and every projection
    parameter is trainable (the fused backward accumulates all six gradients in place; a layer with frozen projections
    whose input still needs a gradient takes the composition)."""
    if XATTN == "off" or h2.dtype != torch.bfloat16 or other2.shape[1] != h2.shape[1]:
        return False
    if XATTN != "always" and P.heads * min(L, Lo) >= h2.shape[1]:
        return False                      # covered, but not profitable (see XATTN above)
    if getattr(P.w_q, "m3ae_t", None) is None or getattr(P.w_kv, "m3ae_t", None) is None or getattr(P.w_o, "m3ae_t", None) is None:
        return False
    d = XattnDesc()
    d.dir = 0 if L <= Lo else 1
    d.B, d.Lq, d.Lk, d.D, d.H = 1, L, Lo, h2.shape[1], P.heads
    d.launch_flags = _lib.XATTN_LEGACY_CHAIN if XATTN_LEGACY_CHAIN else 0
    if not backward:
        return bool(_lib.lib().m3ae_xattn_supported(C.byref(d)))
    if not all(p.requires_grad for p in (P.w_q, P.w_kv, P.w_o, P.b_q, P.b_kv, P.b_o)):
        return False
    if _DETERMINISTIC:   # m3ae_xattn_bwd sums its weight and bias gradients over the samples with fp32 atomics: training calls
        return False     # take the composition, whose wgrads and reductions have ordered forms
    return bool(_lib.lib().m3ae_xattn_bwd_supported(C.byref(d)))


def _xattn_alloc(dev):
    """The default allocator of the fused cross-attention buffers: alloc(name, shape, dtype) -> an uninitialised contiguous tensor.
    xattn_fwd / xattn_bwd take another one through `alloc` (tests: every buffer the descriptor names as a view of a fenced one)."""
    return lambda name, shape, dt=torch.bfloat16: torch.empty(shape, dtype=dt, device=dev)


def xattn_fwd(h2, B, L, other2, Lo, mask, P, pdrop=0.0, need_bwd=True, want_probs=False, alloc=None):
    """BertAttention as crossattention (bert_model.py:480-488) through the fused kernels.  Returns (out, saved).
    need_bwd=False (forward-only call): the image-query direction keeps scores and probabilities on chip, unless want_probs
    (attention maps asked for: the same launch copies them out of LDS, xattn_probs reads them)."""
    _need_cuda(h2)
    dev, D, H = h2.device, h2.shape[1], P.heads
    seeds = (next_dropout_seed(), next_dropout_seed()) if pdrop > 0 else None
    d = _xattn_desc(h2, B, L, other2, Lo, mask, P, pdrop, seeds)
    f32 = torch.float32
    T, R = min(L, Lo), H * min(L, Lo)
    e = alloc or _xattn_alloc(dev)
    t = {}
    if d.dir == 0:
        t["proj"] = e("proj", (B * L, D))
        t["prime"] = e("prime", (B, R, D))
        t["probs"] = e("probs", (B, R, 640))
        t["zctx"] = e("zctx", (B, R, D))
        t["ctx"] = e("ctx", (B * L, D))
        if pdrop > 0:
            t["probs_drop"] = e("probs_drop", (B, R, 640))
            t["rowsum"] = e("rowsum", (B, R), f32)
    else:
        t["proj"] = e("proj", (B * Lo, 2 * D))
        t["prime"] = e("prime", (2, B, R, D))
        t["colbias"] = e("colbias", (B, R), f32)
        if need_bwd or XATTN_LEGACY_CHAIN or want_probs:
            t["probs"] = e("probs", (B, L, R))
            if pdrop > 0:
                t["probs_drop"] = e("probs_drop", (B, L, R))
    t["s"] = e("s", (B * L, D))
    t["out"] = e("out", (B * L, D))
    t["mean"] = e("mean", (B * L,), f32)
    t["rstd"] = e("rstd", (B * L,), f32)
    for k, v in t.items():
        setattr(d, k, v.data_ptr())
    e0 = _prof_begin()
    check(_lib.lib().m3ae_xattn_fwd(C.byref(d), _stream()), "m3ae_xattn_fwd")
    _prof_end(e0, "xattn_fwd", (B, H, L, Lo, D // H))
    return t["out"], ("xattn", h2, other2, mask, t, seeds, pdrop)


def _xattn_probs_desc(saved, what):
    """The descriptor fields m3ae_xattn_probs_export / m3ae_xattn_probs_colmean read, from what an xattn_fwd call saved:
    (descriptor, dropped, B, Lq, Lk)."""
    _, h2, other2, mask, t, seeds, pdrop = saved
    if "probs" not in t:
        raise _lib.M3AEHipError(f"this fused cross-attention call kept its probabilities on chip ({what} needs xattn_fwd(want_probs=True))")
    d = XattnDesc()
    prime = t["prime"]
    dir1 = prime.dim() == 4                  # dir 1 keeps K' and V' ([2, B, R, D]), dir 0 Q' ([B, R, D])
    B = prime.shape[1] if dir1 else prime.shape[0]
    L, Lo = h2.shape[0] // B, other2.shape[0] // B
    d.dir = 1 if dir1 else 0
    d.B, d.Lq, d.Lk, d.D = B, L, Lo, h2.shape[1]
    d.H = prime.shape[-2] // min(L, Lo)
    d.probs = t["probs"].data_ptr()
    dropped = pdrop > 0
    if dropped:
        d.probs_drop = t["probs_drop"].data_ptr()
    return d, dropped, B, L, Lo


def xattn_probs(saved):
    """The attention probabilities of an xattn_fwd call from its saved buffers: fp32 [B, H, Lq, Lk], contiguous
    (m3ae_xattn_probs_export: padding keys sliced off; under dropout the dropped and rescaled P the call used)."""
    d, dropped, B, L, Lo = _xattn_probs_desc(saved, "xattn_probs")
    out = torch.empty((B, d.H, L, Lo), dtype=torch.float32, device=saved[1].device)
    check(_lib.lib().m3ae_xattn_probs_export(C.byref(d), int(dropped), C.c_void_p(out.data_ptr()), out.stride(0), out.stride(1),
                                             out.stride(2), _stream()), "m3ae_xattn_probs_export")
    return out


def xattn_colmean(saved):
    """The received attention of an xattn_fwd call from its saved buffers: the mean of xattn_probs(saved) over heads and queries,
    fp32 [B, Lk] (m3ae_xattn_probs_colmean: one pass over the stored bf16 P)."""
    d, dropped, B, L, Lo = _xattn_probs_desc(saved, "xattn_colmean")
    out = torch.empty((B, Lo), dtype=torch.float32, device=saved[1].device)
    check(_lib.lib().m3ae_xattn_probs_colmean(C.byref(d), int(dropped), C.c_void_p(out.data_ptr()), out.stride(0), _stream()),
          "m3ae_xattn_probs_colmean")
    return out


def xattn_bwd(dy, saved, B, L, Lo, P, need_dother=True, alloc=None):
    """Backward of xattn_fwd (m3ae_xattn_bwd): returns (dx, dother); parameter gradients accumulate in place."""
    _no_ordered_form("the fused cross-attention backward (m3ae_xattn_bwd; its forward ran before the mode was switched on)")
    _, h2, other2, mask, t, seeds, pdrop = saved
    dev, D, H = h2.device, h2.shape[1], P.heads
    d = _xattn_desc(h2, B, L, other2, Lo, mask, P, pdrop, seeds)
    for k, v in t.items():
        setattr(d, k, v.data_ptr())
    f32 = torch.float32
    e = alloc or _xattn_alloc(dev)
    dyc = dy.contiguous()
    dx = e("dx", (B * L, D))
    dother = e("dy", (B * Lo, D)) if need_dother else None
    L_ = _lib.lib()
    w = {"ws_ds": e("ws_ds", (B * L, D)), "ws_dscores": e("ws_dscores", tuple(t["probs"].shape)),
         "ws_dprime": e("ws_dprime", tuple(t["prime"].shape)), "ws_dproj": e("ws_dproj", tuple(t["proj"].shape)),
         "ws_vec": e("ws_vec", (3 * B * H * min(L, Lo),), f32),
         "ws_ln": e("ws_ln", (2 * L_.m3ae_layernorm_bwd_blocks(B * L) * D,), f32)}
    if pdrop > 0:
        w["ws_dsd"] = e("ws_dsd", (B * L, D))
    if d.dir == 0:
        w["ws_dz"] = e("ws_dz", tuple(t["zctx"].shape))
        w["ws_dctx"] = e("ws_dctx", (B * L, D))
    for k, v in w.items():
        setattr(d, k, v.data_ptr())
    d.d_out, d.dx = dyc.data_ptr(), dx.data_ptr()
    d.dy = dother.data_ptr() if dother is not None else None
    train = P.ln.weight.requires_grad
    grads = {"g_wq": P.w_q, "g_wkv": P.w_kv, "g_wo": P.w_o, "g_bq": P.b_q, "g_bkv": P.b_kv, "g_bo": P.b_o}
    for k, prm in grads.items():
        if not prm.requires_grad:
            raise _lib.M3AEHipError("the fused cross-attention backward needs trainable projection parameters")
        setattr(d, k, _grad_buf(prm).data_ptr())
    if train:
        d.g_ln_g, d.g_ln_b = _grad_buf(P.ln.weight).data_ptr(), _grad_buf(P.ln.bias).data_ptr()
    e0 = _prof_begin()
    check(L_.m3ae_xattn_bwd(C.byref(d), _stream()), "m3ae_xattn_bwd")
    _prof_end(e0, "xattn_bwd", (B, H, L, Lo, D // H))
    for prm in (P.w_o, P.b_o, P.w_kv, P.b_kv, P.w_q, P.b_q) + ((P.ln.weight, P.ln.bias) if train else ()):
        _done(prm)
    return dx, dother


def _qkv_views(bufs, B):
    """(q, k, v) as [B, L, inner] views of packed projection buffers -- (qkv [B L, 3 inner],) or (q [B L, inner], kv [B Ls,
    2 inner]) -- and, with the same call, of their gradient buffers."""
    if len(bufs) == 1:
        p3 = bufs[0].view(B, -1, bufs[0].shape[1])
        n = p3.shape[2] // 3
        return p3[..., :n], p3[..., n:2 * n], p3[..., 2 * n:]
    q, kv = bufs
    n = q.shape[1]
    kv3 = kv.view(B, -1, 2 * n)
    return q.view(B, -1, n), kv3[..., :n], kv3[..., n:]


class _ProjRows(NamedTuple):
    """One projection of an attention parameter set: weight, bias (or None) and the slice of their rows it takes (None: all
    of them, through mm_nt / mm_dgrad / mm_wgrad without `sl`)."""
    w: object
    b: object
    sl: object = None


def _attn_proj(P, live=False):
    """(Q, K | V) projections of an attention parameter set: the two slices of the packed Q | K | V weight, or the separate Q
    and K | V weights (cross-attention; live-row form: as whole-range slices, which keeps its B-row GEMMs on the shadows)."""
    if hasattr(P, "w_qkv"):
        n = P.w_qkv.shape[0] // 3
        return _ProjRows(P.w_qkv, P.b_qkv, slice(0, n)), _ProjRows(P.w_qkv, P.b_qkv, slice(n, 3 * n))
    sl = slice(None) if live else None
    return _ProjRows(P.w_q, P.b_q, sl), _ProjRows(P.w_kv, P.b_kv, sl)


def _attn_core_fwd(xq, xkv, B, P, kv=None, mask=None, pos_bias=None, scale=None, causal=False, dropout=None, rows=None):
    """Projections + attention product of every block family.  xq [B Lq, D]: the rows the queries come from; xkv [B Ls, Ds]: the
    rows the keys / values come from.  xkv is xq: packed self-attention, Q | K | V in one GEMM (P.w_qkv).  Other rows: two GEMMs,
    P.w_q and P.w_kv (cross-attention), or the Q and the K | V slice of P.w_qkv (live-row self-attention: xq = token 0 of the
    samples of xkv).  kv [B Ls, 2 inner]: ready-made keys / values (xkv is then None).  dropout = (p, seed) of the attention
    probabilities, rows their row map (live-row form).  Returns (o [B, Lq, inner], lse, proj), proj = (qkv,) or (q, kv)."""
    M, D = xq.shape
    if xkv is xq:
        proj = (mm_nt(xq, D, M, compute_weight(P.w_qkv), bias=_bdata(P.b_qkv))[0],)
    else:
        pq, pkv = _attn_proj(P, live=rows is not None)
        q, _ = mm_nt(xq, D, M, compute_weight(pq.w), bias=_bdata(pq.b), sl=pq.sl)
        if kv is None:
            kv, _ = mm_nt(xkv, xkv.shape[1], xkv.shape[0], compute_weight(pkv.w), bias=_bdata(pkv.b), sl=pkv.sl)
        proj = (q, kv)
    q3, k3, v3 = _qkv_views(proj, B)
    o, lse = attn_forward(q3, k3, v3, P.heads, mask, pos_bias, scale, causal, dropout, rows)
    return o, lse, proj


def _attn_core_bwd(dctx, xq, xkv, proj, o, lse, B, P, mask=None, pos_bias=None, scale=None, causal=False, dropout=None,
                   d_pos_bias=None, residual=None, need_dx=True, need_dsrc=True, rows=None):
    """Backward of _attn_core_fwd from dctx = d(o) [B Lq, inner]: attention backward into a packed gradient buffer, the weight
    gradients, then the input gradients.  Returns (dx, dsrc); `residual` is added to dx in the dgrad epilogue.  Packed or not is
    read off `proj`, i.e. off what the forward did.  Live-row self-attention: (dx [B Ls, D], None), the gradient of ALL rows of
    the stream (xkv), token 0's with its query part and `residual` in."""
    dproj = tuple(torch.empty_like(t) for t in proj)
    attn_backward(*_qkv_views(proj, B), o, lse, dctx.view(o.shape), *_qkv_views(dproj, B), P.heads, mask, pos_bias, scale,
                  causal, d_pos_bias, dropout, rows)
    D = xq.shape[1]
    if len(proj) == 1:
        mm_wgrad(dproj[0], xq, D, P.w_qkv, P.b_qkv)
        return (mm_dgrad(dproj[0], P.w_qkv, residual=residual) if need_dx else None), None
    assert xkv is not None, "the forward was given ready-made kv (inference only): there is no source to differentiate"
    pq, pkv = _attn_proj(P, live=rows is not None)
    dq, dkv = dproj
    mm_wgrad(dq, xq, D, pq.w, pq.b, sl=pq.sl)
    mm_wgrad(dkv, xkv, xkv.shape[1], pkv.w, pkv.b, sl=pkv.sl)
    if pq.sl is not None:   # sliced weight gradients report nothing: every distinct parameter once, now that its slices are in
        for prm in {id(p): p for p in (pq.w, pq.b, pkv.w, pkv.b) if p is not None}.values():
            if prm.requires_grad:
                _done(prm)
    if pq.w is pkv.w:
        # LIVE-ROW SELF-ATTENTION: token 0 is query and key.  Its gradient is the full layer's product for that row, d(q | k | v)
        # . W_qkv + residual in ONE accumulation and one rounding (the same bits as the full call's row, so the layers below see
        # the same gradient): B packed rows, written over row 0 of the key / value rows' gradient
        dx = mm_dgrad(dkv, pkv.w, sl=pkv.sl)
        dqkv0 = torch.cat([dq, dkv.view(B, -1, dkv.shape[1])[:, 0]], dim=1)
        dx.view(B, -1, D)[:, 0] = mm_dgrad(dqkv0, pq.w, residual=residual)
        return dx, None
    dx = mm_dgrad(dq, pq.w, residual=residual, sl=pq.sl) if need_dx else None
    return dx, (mm_dgrad(dkv, pkv.w, sl=pkv.sl) if need_dsrc else None)


def _ffn_core_fwd(x2, P, act, residual, mid_drop=None, out_drop=None, rows=None):
    """y = dropout_out(dropout_mid(act(x2 W1^T + b1)) W2^T + b2) + residual.  Returns (y, u, g): g the (dropped) activation,
    u what the backward GEMM needs of the pre-activation (its act' when SAVE_DACT, else itself)."""
    M, D = x2.shape
    g, u = mm_nt(x2, D, M, compute_weight(P.w1), bias=_bdata(P.b1), act=act, want_preact=True, preact_grad=SAVE_DACT,
                 dropout=mid_drop, rows=rows)
    y, _ = mm_nt(g, g.shape[1], M, compute_weight(P.w2), bias=_bdata(P.b2), residual=residual, dropout=out_drop, rows=rows,
                 out_dtype=None if residual is None else residual.dtype)   # (an fp32 residual stream stays fp32 through the join)
    return y, u, g


def _ffn_core_bwd(dy, x2, u, g, P, act, mid_drop=None, residual=None, rows=None):
    """Backward of _ffn_core_fwd from dy = d(W2 output, before the residual join): returns dx (+ residual, in the epilogue)."""
    mm_wgrad(dy, g, g.shape[1], P.w2, P.b2)
    du = mm_dgrad(dy, P.w2, dact_aux=u, dact=ACT_MULAUX if SAVE_DACT else act, dropout=mid_drop, rows=rows)   # dU = (dY W2) * act'(U)
    mm_wgrad(du, x2, x2.shape[1], P.w1, P.b1)
    return mm_dgrad(du, P.w1, residual=residual)


def _attn_sub_fwd(h2, B, L, other2, Lo, mask, P, pdrop=0.0, fused_cross=False, need_bwd=True, want_probs=False, live=False):
    """BertAttention (bert_model.py:367-413) on 2-D token-major activations. Returns (y, saved).
    pdrop > 0 (training): attention-probability dropout (:334) and hidden dropout on the output dense (:362).
    fused_cross: take the fused cross-attention sub-block where it covers the shapes (need_bwd: and its backward does).
    want_probs: the attention map will be asked of `saved` (_attn_sub_probs): a forward-only fused call copies it out.
    live: the live-row form.  h2 [B, D] is token 0 of each sample (compact) and the only row computed; other2 [B Lo, Ds] the rows
    of the keys / values -- the other stream's, or for self-attention all rows of the samples themselves.  L stays the query rows
    per sample of the full call, whose dropout masks (rows b L of the dense sites, (b H + h) L of the probabilities) this call
    draws, with seeds taken in the same order."""
    if other2 is not None and fused_cross and not live and xattn_supported(h2, L, other2, Lo, mask, P, backward=need_bwd):
        return xattn_fwd(h2, B, L, other2, Lo, mask, P, pdrop, need_bwd=need_bwd, want_probs=want_probs)
    da, dh = dropout_pair(pdrop), dropout_pair(pdrop)
    rows = (0, L) if live else None
    xkv = h2 if other2 is None else other2
    o, lse, proj = _attn_core_fwd(h2, xkv, B, P, mask=mask, dropout=da, rows=rows)
    M, n = h2.shape[0], o.shape[2]
    s, _ = mm_nt(o.view(M, n), n, M, compute_weight(P.w_o), bias=_bdata(P.b_o), residual=h2, dropout=dh, rows=rows)
    y, mean, rstd = ln_fwd_raw(s, P.ln)
    return y, (h2, xkv, proj, o, lse, s, mean, rstd, mask, da, dh, rows)


def _attn_sub_probs(saved, B, L, Lo, P):
    """The attention map of an _attn_sub_fwd call (fp32 [B, H, L, Lo]) from what it saved: the fused cross-attention's buffers,
    or the composition's projections and log-sum-exp table."""
    if isinstance(saved[0], str):
        return xattn_probs(saved)
    q3, k3, _ = _qkv_views(saved[2], B)
    lse, mask, da = saved[4], saved[8], saved[9]
    return attn_probs(q3, k3, lse, P.heads, mask, dropout=da)


def _attn_sub_colmean(saved, B, L, Lo, P):
    """The received attention of an _attn_sub_fwd call (fp32 [B, Lo]: the mean of _attn_sub_probs over heads and queries) from what
    it saved, with the same dispatch; the map itself is not formed."""
    if isinstance(saved[0], str):
        return xattn_colmean(saved)
    q3, k3, _ = _qkv_views(saved[2], B)
    lse, mask, da = saved[4], saved[8], saved[9]
    return attn_colmean(q3, k3, lse, P.heads, mask, dropout=da)


def _post_ln_bwd(dy, s, ln, mean, rstd, dh, rows=None):
    """Backward of the post-LayerNorm of a BERT sub-block whose dense output was dropped with dh = (p, seed) or None:
    (ds, dsd) = the gradient of the LayerNorm input (residual branch) and of the dense output before its dropout."""
    if dh is not None:
        return ln_bwd_raw(dy, s, ln, mean, rstd, drop=dh, rows=rows)
    ds = ln_bwd_raw(dy, s, ln, mean, rstd)
    return ds, ds


def _attn_sub_bwd(dy, saved, B, L, Lo, P, need_dother=True):
    """Backward of _attn_sub_fwd: (dh, dother).  Live-row form: dh is the gradient of the token-0 rows [B, D]; of self-attention,
    whose key / value rows are the stream itself, the gradient of all its rows [B L, D]."""
    if isinstance(saved[0], str):   # ("xattn", ...): the fused sub-block
        return xattn_bwd(dy, saved, B, L, Lo, P, need_dother)
    h2, xkv, proj, o, lse, s, mean, rstd, mask, da, dh, rows = saved
    M, n = h2.shape[0], o.shape[2]
    ds, dsd = _post_ln_bwd(dy, s, P.ln, mean, rstd, dh, rows)
    mm_wgrad(dsd, o.view(M, n), n, P.w_o, P.b_o)
    dctx = mm_dgrad(dsd, P.w_o)
    # ds: the residual-branch gradient, joined in the last dgrad's epilogue
    return _attn_core_bwd(dctx, h2, xkv, proj, o, lse, B, P, mask=mask, dropout=da, residual=ds, need_dsrc=need_dother, rows=rows)


def _ffn_sub_fwd(h2, P, pdrop=0.0, rows=None):
    """BertIntermediate + BertOutput (bert_model.py:416-442, 500-503); pdrop: hidden dropout on the output dense (:440).
    rows: h2 holds the rows row_base + m * row_step of the full activation (live-row form): their dropout masks are drawn."""
    dh = dropout_pair(pdrop)
    s, u, g = _ffn_core_fwd(h2, P, ACT_GELU, h2, out_drop=dh, rows=rows)
    y, mean, rstd = ln_fwd_raw(s, P.ln)
    return y, (h2, u, g, s, mean, rstd, dh, rows)


def _ffn_sub_bwd(dy, saved, P):
    h2, u, g, s, mean, rstd, dh, rows = saved
    ds, dsd = _post_ln_bwd(dy, s, P.ln, mean, rstd, dh, rows)
    return _ffn_core_bwd(dsd, h2, u, g, P, ACT_GELU, residual=ds, rows=rows)


class BlockOpts(NamedTuple):
    """The per-call options of the fused block functions, built by the module at every call and passed beside `P` (which holds
    parameters only).  pdrop: dropout probability of this call (0 in eval mode).  cls_only: BertCrossLayerFn's live-row form.
    fused_cross / need_bwd / want_probs: see _attn_sub_fwd.  want_summary: BertCrossLayerFn also returns the received attention of
    its two attentions (_attn_sub_colmean); like want_probs it needs the full layer and a fused call's P in memory."""
    pdrop: float = 0.0
    cls_only: bool = False
    fused_cross: bool = False
    want_probs: bool = False
    need_bwd: bool = True
    want_summary: bool = False


class BertCrossLayerFn(Function):
    """BertCrossLayer.forward (bert_model.py:457-498): self-attn -> cross-attn -> FFN as one node.
    opts.cls_only, the live-row form: only token 0 of the output is read (CLS heads).  K | V of both attentions for all rows,
    every other product on the B token-0 rows; the dropout sites draw the full call's seeds and masks.  Returns [B, 1, D]."""

    @staticmethod
    def forward(ctx, h, other, mask_self, mask_other, P, opts, *anchors):
        B, L, D = h.shape
        Lo = other.shape[1]
        h2 = h.contiguous().view(B * L, D)
        other2 = other.contiguous().view(B * Lo, other.shape[2])
        pd, live = opts.pdrop, opts.cls_only
        q2, kv2 = (h2.view(B, L, D)[:, 0].contiguous(), h2) if live else (h2, None)
        a, s1 = _attn_sub_fwd(q2, B, L, kv2, L, mask_self, P.attn, pd, live=live)
        # the fused cross-attention sub-block (csrc/xattn.hip) where the shapes are covered: forward-only calls always,
        # training with its fused backward (ops.XATTN_TRAIN)
        c, s2 = _attn_sub_fwd(a, B, L, other2, Lo, mask_other, P.cross, pd, fused_cross=opts.fused_cross, need_bwd=opts.need_bwd,
                              want_probs=opts.want_probs or opts.want_summary, live=live)
        y, s3 = _ffn_sub_fwd(c, P.ffn, pd, rows=(0, L) if live else None)
        ctx.saved = (s1, s2, s3)
        ctx.P, ctx.dims, ctx.n_anchor = P, (B, L, Lo, D), len(anchors)
        ctx.need_other = other.requires_grad
        extra = ()
        if opts.want_probs:
            # the two attention maps (bert_model.py:346 of the self- and the cross-attention), read-only outputs
            extra += (_attn_sub_probs(s1, B, L, L, P.attn), _attn_sub_probs(s2, B, L, Lo, P.cross))
        if opts.want_summary:
            # their means over heads and queries, [B, L] and [B, Lo], after the maps when both are asked for
            assert not live, "attention summaries are full-layer outputs"
            extra += (_attn_sub_colmean(s1, B, L, L, P.attn), _attn_sub_colmean(s2, B, L, Lo, P.cross))
        if extra:
            ctx.mark_non_differentiable(*extra)
            return (y.view(B, L, D),) + extra
        return y.view(B, -1, D)

    @staticmethod
    def backward(ctx, dy, *_maps):   # (the maps and summaries, when returned, carry no gradient)
        B, L, Lo, D = ctx.dims
        s1, s2, s3 = ctx.saved
        ctx.saved = None
        P = ctx.P
        dc = _ffn_sub_bwd(dy.contiguous().view(-1, D), s3, P.ffn)
        da, dother = _attn_sub_bwd(dc, s2, B, L, Lo, P.cross, need_dother=ctx.need_other)
        dh, _ = _attn_sub_bwd(da, s1, B, L, L, P.attn)   # (live-row form too: all rows of the stream)
        return (dh.view(B, L, D), None if dother is None else dother.view(B, Lo, -1), None, None, None, None) + \
               (None,) * ctx.n_anchor


class BertSelfLayerFn(Function):
    """BertSelfLayer == HF RobertaLayer (bert_model.py:506-546; m3ae_module.py:233-234)."""

    @staticmethod
    def forward(ctx, h, mask, P, opts, *anchors):
        B, L, D = h.shape
        h2 = h.contiguous().view(B * L, D)
        a, s1 = _attn_sub_fwd(h2, B, L, None, L, mask, P.attn, opts.pdrop)
        y, s3 = _ffn_sub_fwd(a, P.ffn, opts.pdrop)
        ctx.saved = (s1, s3)
        ctx.P, ctx.dims, ctx.n_anchor = P, (B, L, D), len(anchors)
        return y.view(B, L, D)

    @staticmethod
    def backward(ctx, dy):
        B, L, D = ctx.dims
        s1, s3 = ctx.saved
        ctx.saved = None
        da = _ffn_sub_bwd(dy.contiguous().view(B * L, D), s3, ctx.P.ffn)
        dh, _ = _attn_sub_bwd(da, s1, B, L, L, ctx.P.attn)
        return (dh.view(B, L, D), None, None, None) + (None,) * ctx.n_anchor


class ClipBlockFn(Function):
    """ResidualAttentionBlock.forward (clip_model.py:60-63), pre-LN: x += MHA(LN1(x)); x += MLP(LN2(x)).

    fp32 residual stream (clip_residual_dtype="fp32" in bf16 mode): x arrives in fp32 while the weights' compute copies are bf16.
    The two LayerNorms then read fp32 rows and write the bf16 GEMM operands, the two joins (out-proj and fc2 epilogues) add the
    fp32 stream and write fp32, and the backward carries the stream's gradient in fp32: one cast of the incoming dy for the fc2
    wgrad / dgrad, and LN2's backward hands the out-proj GEMMs their bf16 operand from the same pass.  Every GEMM and attention
    operand is bf16 as in the bf16 stream; x in the weights' dtype is the path of before, launch for launch."""

    @staticmethod
    def forward(ctx, x, P, *anchors):
        B, L, D = x.shape
        M = B * L
        x2 = x.contiguous().view(M, D)
        lo = compute_weight(P.w_qkv).dtype   # the GEMM operands' dtype; x2.dtype is the stream's
        h1, m1, r1 = ln_fwd_raw(x2, P.ln1, out_dtype=lo)
        o, lse, proj = _attn_core_fwd(h1, h1, B, P)
        xa, _ = mm_nt(o.view(M, D), D, M, compute_weight(P.w_o), bias=_bdata(P.b_o), residual=x2, out_dtype=x2.dtype)
        h2, m2, r2 = ln_fwd_raw(xa, P.ln2, out_dtype=lo)
        y, u, g = _ffn_core_fwd(h2, P, ACT_QUICKGELU, xa)
        ctx.saved = (x2, m1, r1, h1, proj, o, lse, xa, m2, r2, h2, u, g)
        ctx.P, ctx.dims, ctx.n_anchor = P, (B, L, D), len(anchors)
        return y.view(B, L, D)

    @staticmethod
    def backward(ctx, dy):
        B, L, D = ctx.dims
        M = B * L
        x2, m1, r1, h1, proj, o, lse, xa, m2, r2, h2, u, g = ctx.saved
        ctx.saved = None
        P = ctx.P
        dy2 = dy.contiguous().view(M, D)
        mixed = h2.dtype != xa.dtype   # fp32 stream, bf16 operands
        dh2 = _ffn_core_bwd(cast(dy2, h2.dtype), h2, u, g, P, ACT_QUICKGELU)
        if mixed:
            dxa_s, dxa = ln_bwd_raw(dh2, xa, P.ln2, m2, r2, dx_add=dy2, want_lo=True)   # the stream's gradient and its bf16 rounding
        else:
            dxa_s = dxa = ln_bwd_raw(dh2, xa, P.ln2, m2, r2, dx_add=dy2)  # + residual branch, fused into LN backward
        mm_wgrad(dxa, o.view(M, D), D, P.w_o, P.b_o)
        dctx = mm_dgrad(dxa, P.w_o)
        dh1, _ = _attn_core_bwd(dctx, h1, h1, proj, o, lse, B, P)
        dx = ln_bwd_raw(dh1, x2, P.ln1, m1, r1, dx_add=dxa_s)
        return (dx.view(B, L, D), None) + (None,) * ctx.n_anchor


# ----------------------------------------------------------------------------------------------------------
# T5 pre-norm blocks (HF T5Block restated; m3ae_t5_mm_encoder_input.py:202,244): RMSNorm, no linear biases, no
# 1/sqrt(d) scaling, additive relative-position bias, ReLU FFN.  One autograd node per block.
# ----------------------------------------------------------------------------------------------------------
def _drop_raw(x2, drop):
    """dropout of a 2-D activation with an explicit (p, seed): the gradient entering a dropped sub-layer output."""
    if drop is None:
        return x2
    x2 = x2.contiguous()
    out = torch.empty_like(x2)
    check(_lib.lib().m3ae_dropout(_p(x2), _p(out), None, x2.shape[0], x2.shape[1], drop[0], drop[1], _salt(), _dt(x2), _stream()),
          "m3ae_dropout")
    return out


def t5_attn_fwd(h2, B, P, bias, causal, pdrop=0.0, src2=None, kv=None):
    """HF T5LayerSelfAttention / T5LayerCrossAttention (third party, transformers 4.6.0) on rows h2 [B L, D]: attention-weight
    dropout inside T5Attention and `hidden + dropout(attn)`.  src2 [B Ls, D]: the rows the cross-attention reads; kv: their
    projected keys / values computed earlier ([B Ls, 2 inner]; generation re-uses them every step).  Returns (y, saved)."""
    da, dh = dropout_pair(pdrop), dropout_pair(pdrop)
    n, _, rstd = ln_fwd_raw(h2, P.ln, rms=True)
    xkv = n if (src2 is None and kv is None) else src2   # self-attention reads its own normalised rows
    o, lse, proj = _attn_core_fwd(n, xkv, B, P, kv=kv, pos_bias=bias, scale=1.0, causal=causal, dropout=da)
    M, inner = h2.shape[0], o.shape[2]
    y, _ = mm_nt(o.view(M, inner), inner, M, compute_weight(P.w_o), residual=h2, dropout=dh)
    return y, (h2, rstd, n, proj, o, lse, xkv, da, dh)


def t5_self_attn_step(h2, B, P, bias_row, cache, t, pdrop=0.0):
    """Generation: the T5 self-attention sub-layer for ONE new position t of every sequence.  h2 [B, D]; `cache` [B, Tmax,
    2 inner] holds the keys | values of positions < t and receives row t; bias_row [H, 1, t + 1] is the relative-position
    bias of the new query.  Same kernels, same order as t5_attn_fwd on the whole prefix (whose last row this equals)."""
    da, dh = dropout_pair(pdrop), dropout_pair(pdrop)
    n, _, _ = ln_fwd_raw(h2, P.ln, rms=True)
    D = n.shape[1]
    inner = P.w_o.shape[1]
    qkv, _ = mm_nt(n, D, B, compute_weight(P.w_qkv))
    cache[:, t].copy_(qkv[:, inner:])
    q = qkv[:, :inner].unsqueeze(1)                        # [B, 1, inner], batch stride 3 inner
    o, _ = attn_forward(q, cache[:, :t + 1, :inner], cache[:, :t + 1, inner:], P.heads, None, bias_row, scale=1.0,
                        causal=False, dropout=da)
    y, _ = mm_nt(o.view(B, inner), inner, B, compute_weight(P.w_o), residual=h2, dropout=dh)
    return y


def t5_self_attn_tree(h2, G, Ni, P, rel_bias, anc, err):
    """Exhaustive list scoring: the T5 self-attention sub-layer over the rows of the answer trie's internal nodes, h2 [G Ni, D]
    (sample g at internal row i in row g Ni + i).  As t5_self_attn_step, but a row's keys are its trie ancestors (tree_attention,
    scale 1) and rel_bias fp32 [H, Dmax] holds the relative-position bias by depth difference.  Inference only: no dropout."""
    n, _, _ = ln_fwd_raw(h2, P.ln, rms=True)
    D, inner, M = n.shape[1], P.w_o.shape[1], G * Ni
    qkv, _ = mm_nt(n, D, M, compute_weight(P.w_qkv))
    q3 = qkv.view(G, Ni, 3 * inner)
    o = tree_attention(q3[..., :inner], q3[..., inner:2 * inner], q3[..., 2 * inner:], anc, P.heads, 1.0, rel_bias, err)
    y, _ = mm_nt(o.view(M, inner), inner, M, compute_weight(P.w_o), residual=h2)
    return y


def _t5_attn_bwd(dy, saved, B, P, bias, causal, dbias, need_dh=True, need_dsrc=True):
    h2, rstd, n, proj, o, lse, xkv, da, dh_drop = saved
    need_dh = need_dh or P.ln.weight.requires_grad  # the RMSNorm scale gradient comes out of the same kernel
    M, inner = h2.shape[0], o.shape[2]
    dyd = _drop_raw(dy, dh_drop)  # gradient of the (dropped) sub-layer output; the residual branch keeps dy itself
    mm_wgrad(dyd, o.view(M, inner), inner, P.w_o)
    dctx = mm_dgrad(dyd, P.w_o)
    dn, dsrc = _attn_core_bwd(dctx, n, xkv, proj, o, lse, B, P, pos_bias=bias, scale=1.0, causal=causal, dropout=da,
                              d_pos_bias=dbias, need_dx=need_dh, need_dsrc=need_dsrc)
    dh = ln_bwd_raw(dn, h2, P.ln, None, rstd, dx_add=dy, rms=True) if need_dh else None
    return dh, dsrc


def t5_ff_fwd(h2, P, pdrop=0.0):
    # HF T5DenseReluDense: wo(dropout(relu(wi(x)))); T5LayerFF: hidden + dropout(ff)
    d1, d2 = dropout_pair(pdrop), dropout_pair(pdrop)
    n, _, rstd = ln_fwd_raw(h2, P.ln, rms=True)
    y, u, g = _ffn_core_fwd(n, P, ACT_RELU, h2, mid_drop=d1, out_drop=d2)
    return y, (h2, rstd, n, u, g, d1, d2)


def _t5_ff_bwd(dy, saved, P):
    h2, rstd, n, u, g, d1, d2 = saved
    dn = _ffn_core_bwd(_drop_raw(dy, d2), n, u, g, P, ACT_RELU, mid_drop=d1)   # g: the dropped activation W2 multiplied
    return ln_bwd_raw(dn, h2, P.ln, None, rstd, dx_add=dy, rms=True)


class T5EncBlockFn(Function):
    @staticmethod
    def forward(ctx, h, pos_bias, P, opts, *anchors):
        B, L, D = h.shape
        h2 = h.contiguous().view(B * L, D)
        bias = pos_bias.detach() if pos_bias is not None else None
        pd = opts.pdrop
        a, s1 = t5_attn_fwd(h2, B, P.attn, bias, False, pd)
        y, s2 = t5_ff_fwd(a, P.ffn, pd)
        ctx.saved = (s1, s2, bias)
        ctx.P, ctx.dims, ctx.n_anchor = P, (B, L, D), len(anchors)
        ctx.need_h = h.requires_grad
        ctx.need_bias = pos_bias is not None and pos_bias.requires_grad
        return y.view(B, L, D)

    @staticmethod
    def backward(ctx, dy):
        B, L, D = ctx.dims
        s1, s2, bias = ctx.saved
        ctx.saved = None
        dbias = torch.zeros_like(bias) if ctx.need_bias else None
        da = _t5_ff_bwd(dy.contiguous().view(B * L, D), s2, ctx.P.ffn)
        dh, _ = _t5_attn_bwd(da, s1, B, ctx.P.attn, bias, False, dbias, need_dh=ctx.need_h)
        return (None if dh is None else dh.view(B, L, D), dbias, None, None) + (None,) * ctx.n_anchor


class T5DecBlockFn(Function):
    @staticmethod
    def forward(ctx, h, enc, pos_bias, P, opts, *anchors):
        B, T, D = h.shape
        Ls = enc.shape[1]
        h2 = h.contiguous().view(B * T, D)
        enc2 = enc.contiguous().view(B * Ls, enc.shape[2])
        bias = pos_bias.detach() if pos_bias is not None else None
        pd = opts.pdrop
        a, s1 = t5_attn_fwd(h2, B, P.attn, bias, True, pd)
        c, s2 = t5_attn_fwd(a, B, P.cross, None, False, pd, src2=enc2)
        y, s3 = t5_ff_fwd(c, P.ffn, pd)
        ctx.saved = (s1, s2, s3, bias)
        ctx.P, ctx.dims, ctx.n_anchor = P, (B, T, Ls, D), len(anchors)
        ctx.need_h, ctx.need_enc = h.requires_grad, enc.requires_grad
        ctx.need_bias = pos_bias is not None and pos_bias.requires_grad
        return y.view(B, T, D)

    @staticmethod
    def backward(ctx, dy):
        B, T, Ls, D = ctx.dims
        s1, s2, s3, bias = ctx.saved
        ctx.saved = None
        P = ctx.P
        dbias = torch.zeros_like(bias) if ctx.need_bias else None
        dc = _t5_ff_bwd(dy.contiguous().view(B * T, D), s3, P.ffn)
        da, denc = _t5_attn_bwd(dc, s2, B, P.cross, None, False, None, need_dsrc=ctx.need_enc)
        dh, _ = _t5_attn_bwd(da, s1, B, P.attn, bias, True, dbias, need_dh=ctx.need_h)
        return (None if dh is None else dh.view(B, T, D), None if denc is None else denc.view(B, Ls, -1), dbias,
                None, None) + (None,) * ctx.n_anchor


class EmbedRowsFn(Function):
    """rows = table[ids] (T5 `shared` lookup for the teacher-forced decoder input).  `table` is the compute-dtype
    view of `weight`; the gradient (only when the embedding is trainable) is scatter-added into weight.grad."""

    @staticmethod
    def forward(ctx, ids, weight, table):
        ids = ids.contiguous()   # the kernel walks ids linearly: a strided view (e.g. prefix[:, -1:]) would read its neighbours
        out = torch.empty((ids.numel(), table.shape[1]), dtype=table.dtype, device=table.device)
        check(_lib.lib().m3ae_gather_rows(_p(table), _p(ids), _p(out), ids.numel(), table.shape[1], _dt(table),
                                          _stream()), "m3ae_gather_rows")
        ctx.save_for_backward(ids)
        ctx.weight = weight
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        if ctx.weight.requires_grad:  # rare path: the embedding is frozen in the reference's recipe
            _no_ordered_form("the gradient of a trainable embedding lookup (EmbedRowsFn: torch index_add_)")
            _grad_buf(ctx.weight).index_add_(0, ids, dout.float())
            _done(ctx.weight)
        return None, None, None


# ----------------------------------------------------------------------------------------------------------
# embeddings / tokens
# ----------------------------------------------------------------------------------------------------------
class RobertaEmbedFn(Function):
    @staticmethod
    def forward(ctx, ids, word, pos, typ, pad_id, dtype):
        _need_cuda(ids)
        B, S = ids.shape
        D = word.shape[1]
        out = torch.empty((B, S, D), dtype=dtype, device=ids.device)
        check(_lib.lib().m3ae_roberta_embed_fwd(_p(ids), _p(word), _p(pos), _p(typ), _p(out), B, S, D, pad_id, _dt(out),
                                                _stream()), "m3ae_roberta_embed_fwd")
        ctx.save_for_backward(ids)
        ctx.p, ctx.pad_id = (word, pos, typ), pad_id
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        word, pos, typ = ctx.p
        B, S = ids.shape
        D = word.shape[1]
        d = dout.contiguous()
        if _DETERMINISTIC:
            ws, n = _small_ws(_lib.DET_EMBED_BWD, B * S, D, d.device)
            check(_lib.lib().m3ae_roberta_embed_bwd_det(_p(ids), _p(d), _p(_grad_buf(word)), _p(_grad_buf(pos)),
                                                        _p(_grad_buf(typ)), B, S, D, ctx.pad_id, _dt(d), _p(ws), n, _stream()),
                  "m3ae_roberta_embed_bwd_det")
        else:
            check(_lib.lib().m3ae_roberta_embed_bwd(_p(ids), _p(d), _p(_grad_buf(word)), _p(_grad_buf(pos)),
                                                    _p(_grad_buf(typ)), B, S, D, ctx.pad_id, _dt(d), _stream()),
                  "m3ae_roberta_embed_bwd")
        for p in (word, pos, typ):
            _done(p)
        return None, None, None, None, None, None


def roberta_embed(ids, word, pos, typ, pad_id, dtype):
    return RobertaEmbedFn.apply(ids, word, pos, typ, pad_id, dtype)


class VitTokensFn(Function):
    """conv1 (k = s = patch, no bias) as im2col + GEMM, prepend class_embedding, optional + positional_embedding
    (clip_model.py:94-99 / :110-116)."""

    @staticmethod
    def forward(ctx, img, conv_w, cls, pos, dtype, add_pos, out_dtype=None):
        _need_cuda(img)
        L = _lib.lib()
        B, _, R, _ = img.shape
        width, _, P, _ = conv_w.shape
        g = R // P
        G = g * g
        imgc = img.contiguous().float()
        patches = torch.empty((B * G, 3 * P * P), dtype=dtype, device=img.device)
        check(L.m3ae_patchify(_p(imgc), _p(patches), B, R, P, _dt(patches), _stream()), "m3ae_patchify")
        w2 = compute_weight(conv_w).view(width, -1)
        out_dtype = out_dtype or dtype   # float32 with dtype bfloat16: the fp32 residual stream starts here (bf16 operands, fp32 C)
        pe, _ = mm_nt(patches, patches.stride(0), B * G, w2, out_dtype=out_dtype)
        out = torch.empty((B, G + 1, width), dtype=out_dtype, device=img.device)
        posz = pos if add_pos else torch.zeros_like(pos)
        check(L.m3ae_vit_tokens_fwd(_p(pe), _p(cls), _p(posz), _p(out), B, G, width, _dt(out), _stream()),
              "m3ae_vit_tokens_fwd")
        ctx.save_for_backward(patches)
        ctx.p, ctx.dims, ctx.add_pos = (conv_w, cls, pos), (B, G, width), add_pos
        return out

    @staticmethod
    def backward(ctx, dout):
        (patches,) = ctx.saved_tensors
        conv_w, cls, pos = ctx.p
        B, G, width = ctx.dims
        d = dout.contiguous()
        dpe = torch.empty((B * G, width), dtype=d.dtype, device=d.device)
        gpos = _grad_buf(pos) if ctx.add_pos else torch.zeros_like(pos)
        check(_lib.lib().m3ae_vit_tokens_bwd(_p(d), _p(dpe), _p(_grad_buf(cls)), _p(gpos), B, G, width, _dt(d),
                                             _stream()), "m3ae_vit_tokens_bwd")
        _done(cls)
        if ctx.add_pos:
            _done(pos)
        if conv_w.requires_grad:
            g = _grad_buf(conv_w).view(width, -1)
            dpe = cast(dpe, patches.dtype)   # (fp32 stream: one cast for the conv wgrad's bf16 operand)
            gemm(dpe, 1, dpe.stride(0), patches, patches.stride(0), 1, g, g.stride(0), width, g.shape[1], B * G,
                 accumulate=True)
            _done(conv_w)
        return None, None, None, None, None, None, None


def vit_tokens(img, conv_w, cls, pos, dtype, add_pos=True, out_dtype=None):
    """dtype: the GEMM operands' (patches, conv weight copy); out_dtype: the tokens' (default dtype)."""
    return VitTokensFn.apply(img, conv_w, cls, pos, dtype, add_pos, out_dtype)


# ----------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------
class BCELossFn(Function):
    """F.binary_cross_entropy_with_logits(x, z) * z.shape[1]  (objectives.py:201)."""

    @staticmethod
    def forward(ctx, logits, targets):
        x = logits.contiguous()
        B, Cc = x.shape
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        if _DETERMINISTIC:
            ws, n = _small_ws(_lib.DET_BCE, B, Cc, x.device)
            check(_lib.lib().m3ae_bce_logits_det(_p(x), _p(targets), _p(loss), _p(dx), B, Cc, 1.0, _dt(x), _p(ws), n, _stream()),
                  "m3ae_bce_logits_det")
        else:
            check(_lib.lib().m3ae_bce_logits(_p(x), _p(targets), _p(loss), _p(dx), B, Cc, 1.0, _dt(x), _stream()),
                  "m3ae_bce_logits")
        ctx.save_for_backward(dx)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g.to(dx.dtype), None


def bce_with_logits_loss(logits, targets):
    return BCELossFn.apply(logits, targets)


class XentFn(Function):
    """F.cross_entropy(logits, labels, ignore_index=-100) (objectives.py:19-23, :101)."""

    @staticmethod
    def forward(ctx, logits, labels):
        # rows may be strided (a [..., :V] view of vocabulary-padded logits, see VocabProjFn): no compaction copy
        x = logits
        Cc = x.shape[-1]
        uniform = x.dim() >= 2 and x.stride(-1) == 1 and all(
            x.stride(i) == x.stride(i + 1) * x.shape[i + 1] for i in range(x.dim() - 2))
        if not uniform:
            x = x.contiguous()
        ld = x.stride(-2) if x.dim() >= 2 else Cc
        rows = x.numel() // Cc
        lab = labels.contiguous().view(-1)
        loss = torch.zeros(1, dtype=torch.float32, device=x.device)
        ws = torch.empty(4, dtype=torch.float32, device=x.device)
        dx = (torch.zeros if ld != Cc else torch.empty)((rows, ld), dtype=x.dtype, device=x.device)
        if _DETERMINISTIC:
            ws, n = _small_ws(_lib.DET_XENT, rows, Cc, x.device)
            check(_lib.lib().m3ae_xent_det(_p(x), _p(lab), _p(loss), _p(dx), rows, Cc, ld, 1.0, _dt(x), _p(ws), n, _stream()),
                  "m3ae_xent_det")
        else:
            check(_lib.lib().m3ae_xent(_p(x), _p(lab), _p(loss), _p(dx), _p(ws), rows, Cc, ld, 1.0, _dt(x), _stream()),
                  "m3ae_xent")
        ctx.save_for_backward(dx)
        ctx.shape, ctx.cols = logits.shape, Cc
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        d = dx * g.to(dx.dtype)
        return d.view(*ctx.shape[:-1], dx.shape[-1])[..., :ctx.cols], None


def cross_entropy(logits, labels):
    return XentFn.apply(logits, labels)


class VocabProjFn(Function):
    """logits = x . W^T + b for a vocabulary that is not a multiple of 128 (RoBERTa: 50265), perf mode.  The MFMA
    kernels need N % 4 == 0 (forward), K % 64 == 0 (dgrad) and N1 % 128 == 0 (wgrad); the odd size would send all three
    to the generic kernel (14 % of a pre-training step).  Zero-padded bf16 operand copies [Vp, K] / [K, Vp] (Vp = V rounded
    up to 128, refreshed from the weight's bf16 shadows on every call: two 77-MB copies) keep them on the MFMA path.
    Returns PADDED logits [..., Vp] (pad columns = 0); callers slice [..., :V] (ops.vocab_linear)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x2, M, K, ldx = _rows(x)
        V = weight.shape[0]
        Vp = (V + 127) // 128 * 128
        st = getattr(weight, "_vocab_pad", None)
        if st is None:
            dev = x.device
            st = (torch.zeros((Vp, K), dtype=torch.bfloat16, device=dev), torch.zeros((K, Vp), dtype=torch.bfloat16, device=dev),
                  torch.zeros(Vp, dtype=torch.float32, device=dev))
            weight._vocab_pad = st
        Wp, WpT, bp = st
        Wp[:V].copy_(compute_weight(weight))
        WpT[:, :V].copy_(weight.m3ae_t)
        if bias is not None:
            bp[:V].copy_(bias.detach())
        y, _ = mm_nt(x2, ldx, M, Wp, bias=bp)
        ctx.save_for_backward(x2)
        ctx.meta = (weight, bias, M, K, V, Vp, ldx, x.shape)
        return y.view(*x.shape[:-1], Vp)

    @staticmethod
    def backward(ctx, dy):
        (x2,) = ctx.saved_tensors
        weight, bias, M, K, V, Vp, ldx, xshape = ctx.meta
        _, WpT, _ = weight._vocab_pad
        dy2 = dy.contiguous().view(M, Vp)
        dx = torch.empty((M, K), dtype=dy2.dtype, device=dy2.device)
        gemm(dy2, Vp, 1, WpT, 1, Vp, dx, K, M, K, Vp)                       # dX = dY . W   (K-contiguous transposed copy)
        if weight.requires_grad:
            dWp = torch.zeros((Vp, K), dtype=torch.float32, device=dy2.device)
            dbp = torch.zeros(Vp, dtype=torch.float32, device=dy2.device)
            gemm(dy2, 1, Vp, x2, ldx, 1, dWp, K, Vp, K, M, accumulate=True, a_rowsum=dbp)   # dW = dY^T . X  (+ column sums)
            _grad_buf(weight).add_(dWp[:V])
            _done(weight)
            if bias is not None and bias.requires_grad:
                _grad_buf(bias).add_(dbp[:V])
                _done(bias)
        return dx.view(xshape), None, None


def vocab_linear(x, weight, bias):
    """Vocabulary projection (MLM head, prediction_heads.py:33): MFMA path for any vocabulary size in perf mode."""
    V = weight.shape[0]
    if x.dtype == torch.bfloat16 and V % 128 != 0 and getattr(weight, "m3ae_t", None) is not None:
        return VocabProjFn.apply(x, weight, bias)[..., :V]
    return linear(x, weight, bias)


# ----------------------------------------------------------------------------------------------------------
# row gather (MIM masking) -- differentiable in the source
# ----------------------------------------------------------------------------------------------------------
class GatherRowsFn(Function):
    """out[i] = src[idx[i]].  unique: the caller guarantees that idx holds no row twice (a permutation slice); the backward is then
    m3ae_scatter_add_rows, a plain read-modify-write per row.  Otherwise rows may repeat and the backward is torch's index_add_ in
    fp32, cast back to the gradient's dtype (fp32 atomics: no ordered form)."""

    @staticmethod
    def forward(ctx, src, idx, unique):
        idx = idx.contiguous()
        s2 = src.contiguous().view(-1, src.shape[-1])
        out = torch.empty((idx.numel(), s2.shape[1]), dtype=src.dtype, device=src.device)
        check(_lib.lib().m3ae_gather_rows(_p(s2), _p(idx), _p(out), idx.numel(), s2.shape[1], _dt(s2), _stream()),
              "m3ae_gather_rows")
        ctx.save_for_backward(idx)
        ctx.shape = src.shape
        ctx.unique = bool(unique)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        d = dout.contiguous()
        if not ctx.unique:
            _no_ordered_form("the gradient of ops.gather_rows with rows that may repeat (torch index_add_; unique=True for a permutation)")
            dsrc = torch.zeros((math.prod(ctx.shape[:-1]), ctx.shape[-1]), dtype=torch.float32, device=d.device)
            dsrc.index_add_(0, idx.view(-1), d.float())
            return dsrc.to(d.dtype).view(ctx.shape), None, None
        dsrc = torch.zeros(ctx.shape, dtype=d.dtype, device=d.device)
        check(_lib.lib().m3ae_scatter_add_rows(_p(d), _p(idx), _p(dsrc), idx.numel(), d.shape[1], _dt(d), _stream()),
              "m3ae_scatter_add_rows")
        return dsrc, None, None


def gather_rows(src, flat_idx, unique=False):
    return GatherRowsFn.apply(src, flat_idx, unique)


# ----------------------------------------------------------------------------------------------------------
# de-duplicated image batches (batch["image_index"]): one image-tower pass per distinct image, expanded to the samples
# ----------------------------------------------------------------------------------------------------------
class ImageGroups:
    """The index tables of a de-duplicated image batch, as the two kernels read them: `index` int64 [B] (sample b uses image
    index[b]) and the samples of every image as a CSR -- `offsets` int64 [U + 1], `members` int64 [B], each image's samples in
    ascending order.  `identity`: index == arange(B) with U == B (nothing to expand).  Built on the host by `image_groups`;
    `to(device)` uploads the three tables without blocking when they are pinned."""

    __slots__ = ("index", "offsets", "members", "n_images", "identity")

    def __init__(self, index, offsets, members, n_images, identity):
        self.index, self.offsets, self.members, self.n_images, self.identity = index, offsets, members, n_images, identity

    @property
    def n_samples(self):
        return self.index.numel()

    def tensors(self):
        return self.index, self.offsets, self.members

    def to(self, device):
        return ImageGroups(*(t.to(device, non_blocking=True) for t in self.tensors()), self.n_images, self.identity)


def image_groups(image_index, n_images=None, pin=True):
    """Host tables for `batch["image_groups"]` from a CPU `image_index` (any int sequence / tensor, [B]); pinned when a GPU is
    there so that `.to(device)` does not block.  n_images: rows of the image tensor (default: the largest index + 1).  Raises
    ValueError for an index outside [0, n_images) and for an image row that no sample uses."""
    import numpy as np
    if isinstance(image_index, torch.Tensor):
        if image_index.is_cuda:
            raise ValueError("image_groups builds its tables on the host: pass image_index.cpu()")
        image_index = image_index.numpy()
    idx = np.asarray(image_index)
    if idx.ndim != 1 or idx.size == 0 or idx.dtype.kind not in "iu":
        raise ValueError(f"image_index must be a non-empty 1-D integer array, got shape {idx.shape} dtype {idx.dtype}")
    idx = idx.astype(np.int64)
    U = int(idx.max()) + 1 if n_images is None else int(n_images)
    if idx.min() < 0 or idx.max() >= U:
        raise ValueError(f"image_index has values outside [0, {U}): min {idx.min()}, max {idx.max()}")
    counts = np.bincount(idx, minlength=U)
    if (counts == 0).any():
        raise ValueError(f"image rows {np.flatnonzero(counts == 0).tolist()} are used by no sample (image_index must cover "
                         f"every row of the [{U}, ...] image tensor)")
    offsets = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    members = np.argsort(idx, kind="stable").astype(np.int64)   # per image, its samples in ascending order
    identity = U == idx.size and bool((idx == np.arange(U)).all())
    ts = [torch.from_numpy(a) for a in (idx, offsets, members)]
    if pin and torch.cuda.is_available():
        ts = [t.pin_memory() for t in ts]
    return ImageGroups(*ts, U, identity)


class ExpandSamplesFn(Function):
    """out[b] = x[index[b]] over whole [L, D] blocks (m3ae_expand_samples); backward: the ordered per-image sum of the samples'
    gradients (m3ae_segment_sum_rows: fp32 adds in ascending sample order, one rounding; no atomics, so deterministic mode takes
    the same kernel)."""

    @staticmethod
    def forward(ctx, x, groups):
        xc = x.contiguous()
        U, B = xc.shape[0], groups.n_samples
        R = xc.numel() // U
        out = torch.empty((B, *xc.shape[1:]), dtype=xc.dtype, device=xc.device)
        check(_lib.lib().m3ae_expand_samples(_p(xc), _p(groups.index), _p(out), B, U, R, _dt(xc), _stream()),
              "m3ae_expand_samples")
        ctx.groups, ctx.in_shape = groups, xc.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        g, d = ctx.groups, dout.contiguous()
        U = ctx.in_shape[0]
        dx = torch.empty(ctx.in_shape, dtype=d.dtype, device=d.device)
        check(_lib.lib().m3ae_segment_sum_rows(_p(d), _p(g.offsets), _p(g.members), _p(dx), U, g.n_samples, dx.numel() // U,
                                               _dt(d), _stream()), "m3ae_segment_sum_rows")
        return dx, None


def expand_samples(x, groups):
    """x [U, ...] -> [B, ...] by `groups` (an ImageGroups on x's device): sample b gets x[groups.index[b]].  One autograd node."""
    _need_cuda(x)
    if x.shape[0] != groups.n_images:
        raise ValueError(f"expand_samples: {x.shape[0]} rows for tables of {groups.n_images} images")
    for t in groups.tensors():
        if t.device != x.device or t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError("expand_samples: the group tables must be contiguous int64 tensors on the input's device "
                             "(ops.image_groups(...).to(device))")
    if groups.offsets.numel() != groups.n_images + 1 or groups.members.numel() != groups.n_samples:
        raise ValueError("expand_samples: inconsistent group tables")
    return ExpandSamplesFn.apply(x, groups)


class DropoutFn(Function):
    """nn.Dropout as a standalone op (RoBERTa embeddings, HF RobertaEmbeddings.dropout; m3ae_module.py:230)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        xc = x.contiguous()
        y = torch.empty_like(xc)
        cols = xc.shape[-1]
        check(_lib.lib().m3ae_dropout(_p(xc), _p(y), None, xc.numel() // cols, cols, p, seed, _salt(), _dt(xc), _stream()),
              "m3ae_dropout")
        ctx.p, ctx.seed = p, seed
        return y

    @staticmethod
    def backward(ctx, dy):
        d = dy.contiguous()
        dx = torch.empty_like(d)
        cols = d.shape[-1]
        check(_lib.lib().m3ae_dropout(_p(d), _p(dx), None, d.numel() // cols, cols, ctx.p, ctx.seed, _salt(), _dt(d), _stream()),
              "m3ae_dropout")
        return dx, None, None


def dropout(x, p, training=True):
    if not training or p <= 0:
        return x
    return DropoutFn.apply(x, p, next_dropout_seed())


def dropout_keep_mask(rows, cols, p, seed, device="cuda"):
    """uint8 [rows, cols] keep-mask of the library's counter hash: the mask every dropout site applies for (p, seed)
    on a [rows, cols] array -- GEMM epilogue (M, N), LayerNorm backward (M, D), attention ((b*H + h)*Lq + q, Lk)."""
    m = torch.empty((rows, cols), dtype=torch.uint8, device=device)
    check(_lib.lib().m3ae_dropout(None, None, _p(m), rows, cols, p, seed, _salt(), F32, _stream()), "m3ae_dropout")
    return m


def selftest():
    out = torch.zeros(8 + 256, dtype=torch.int32, device="cuda")
    check(_lib.lib().m3ae_selftest(_p(out), _stream()), "m3ae_selftest")
    return out[:6].cpu().tolist()


# ------------------------------------------------------------------------------------------------------------
# device-resident beam search (csrc/beam.hip): T5ForConditionalGeneration.generate_async
# ------------------------------------------------------------------------------------------------------------
BEAM_TOPK_CHUNK = 2048   # vocabulary elements per workgroup of m3ae_beam_topk when the caller passes chunk=0


def beam_topk_workspace(B, nb, V, device, chunk=0):
    n = _lib.lib().m3ae_beam_topk_workspace_bytes(B, nb, V, chunk)
    return torch.empty(max(n, 8) // 8, dtype=torch.int64, device=device)


def beam_topk(logits, beam_scores, B, nb, chunk=0, ws=None, out=None):
    """logits fp32 [B * nb, V] (row stride >= V), beam_scores fp32 [B * nb] -> top_s fp32 [B, 2 nb], top_i int32 [B, 2 nb]: the best
    2 nb of every sample's nb * V values of fl(log_softmax(x) + beam_score), by (score descending, beam * V + token ascending)."""
    _need_cuda(logits)
    _need_cuda(beam_scores)
    if logits.dtype != torch.float32 or beam_scores.dtype != torch.float32:
        raise TypeError("beam_topk takes fp32 logits and beam scores")
    R, V = logits.shape
    if R != B * nb or beam_scores.numel() != R or logits.stride(1) != 1 or not beam_scores.is_contiguous():
        raise ValueError(f"beam_topk: logits {tuple(logits.shape)} / beam_scores {tuple(beam_scores.shape)} for B={B}, nb={nb}")
    if ws is None:
        ws = beam_topk_workspace(B, nb, V, logits.device, chunk)
    top_s, top_i = out if out is not None else (torch.empty((B, 2 * nb), dtype=torch.float32, device=logits.device),
                                                torch.empty((B, 2 * nb), dtype=torch.int32, device=logits.device))
    check(_lib.lib().m3ae_beam_topk(_p(logits), logits.stride(0), _p(beam_scores), B, nb, V, chunk, _p(ws), ws.numel() * 8,
                                    _p(top_s), _p(top_i), _stream()), "m3ae_beam_topk")
    return top_s, top_i


class _SearchState:
    """What the four search states share: every result field and the error word `err` live in ONE int64 buffer `out`, so one copy
    brings a whole result to the host.  `layout` ({field: shape} in buffer order, then err; `scores` and `logprob` hold the bits of
    float64, as do `probs` and `log_mass` of the list-score state) is the only description of that buffer: views() applies it to the device buffer (alloc_out) and to a host copy (host).
    The answer-list states hold `labels` / `scores` [B, nb] for search.answer_result; k_text is its word on a k outside [1, nb]."""

    def views(self, out):
        parts = out.split([math.prod(shape) for shape in self.layout.values()] + [1])
        return _NS(err=parts[-1], **{n: (p.view(torch.float64) if n in ("scores", "logprob", "probs", "log_mass") else p).view(shape)
                                     for (n, shape), p in zip(self.layout.items(), parts)})

    def alloc_out(self, device, **layout):
        self.layout = layout
        self.out = torch.zeros((sum(map(math.prod, layout.values())) + 1,), dtype=torch.int64, device=device)
        vars(self).update(vars(self.views(self.out)))

    def host(self):
        """One device-to-host copy of `out` -> the namespace of its fields on the host; raises if the error word is set."""
        h = self.views(self.out.cpu())
        if int(h.err) != 0:
            raise _lib.M3AEHipError(self.err_text)
        return h


class BeamState(_SearchState):
    """The device state of one beam search (include/m3ae_hip.h, m3ae_beam_step): allocated once per generate call."""
    err_text = "device beam search: a candidate index left [0, num_beams * vocab_size)"

    def __init__(self, B, nb, max_length, device, start_id=0, pad_id=0):
        R = B * nb
        z = functools.partial(torch.zeros, device=device)
        self.B, self.nb, self.max_length = B, nb, max_length
        self.ids = torch.full((2, R, max_length), pad_id, dtype=torch.int64, device=device)   # ping-pong: a row may feed several rows
        self.ids[0, :, 0] = start_id
        self.cur = 0                                   # which half of `ids` holds the prefixes
        self.last_tok = torch.full((R,), start_id, dtype=torch.int64, device=device)
        self.beam_scores = z((B, nb), dtype=torch.float32)
        self.beam_scores[:, 1:] = -1e9
        self.beam_scores = self.beam_scores.view(-1)
        self.order = z((R,), dtype=torch.int64)
        self.done, self.n_hyp = z((B,), dtype=torch.int32), z((B,), dtype=torch.int32)
        self.hyp_score = z((B, nb), dtype=torch.float64)
        self.hyp_len = z((B, nb), dtype=torch.int32)
        self.hyp_tok = z((B, nb, max_length), dtype=torch.int64)
        self.open_count = z((max_length,), dtype=torch.int32)
        self.alloc_out(device, seq=(B, max_length), len=(B,))


def beam_step(st, top_s, top_i, V, cur_len, eos_id, pad_id, length_penalty=1.0):
    """One BeamSearchScorer step on `st` at prefix length cur_len; st.open_count[cur_len] = samples still open afterwards."""
    for t in (top_s, top_i, st.ids):
        _need_cuda(t)
    if top_s.dtype != torch.float32 or top_i.dtype != torch.int32 or tuple(top_s.shape) != (st.B, 2 * st.nb) \
            or top_i.shape != top_s.shape or not top_s.is_contiguous() or not top_i.is_contiguous():
        raise ValueError("beam_step: top_s fp32 / top_i int32 [B, 2 nb], contiguous")
    if not 1 <= cur_len < st.max_length:
        raise ValueError(f"beam_step: cur_len {cur_len} outside [1, {st.max_length})")
    check(_lib.lib().m3ae_beam_step(_p(top_s), _p(top_i), _p(st.ids[st.cur]), _p(st.ids[1 - st.cur]), _p(st.last_tok), _p(st.beam_scores),
                                    _p(st.order), _p(st.done), _p(st.n_hyp), _p(st.hyp_score), _p(st.hyp_len), _p(st.hyp_tok),
                                    _p(st.open_count[cur_len:]), _p(st.err), st.B, st.nb, V, st.max_length, cur_len, eos_id, pad_id,
                                    float(cur_len) ** length_penalty, _stream()), "m3ae_beam_step")
    st.cur = 1 - st.cur


def beam_finalize(st, cur_len, eos_id, pad_id, length_penalty=1.0, len_offset=0):
    """Open beams of the samples not done join their hypothesis lists; st.seq / st.len = the best hypothesis per sample."""
    _need_cuda(st.ids)
    if not 1 <= cur_len <= st.max_length or cur_len - len_offset < 1:
        raise ValueError(f"beam_finalize: cur_len {cur_len}, len_offset {len_offset}")
    check(_lib.lib().m3ae_beam_finalize(_p(st.ids[st.cur]), _p(st.beam_scores), _p(st.done), _p(st.n_hyp), _p(st.hyp_score),
                                        _p(st.hyp_len), _p(st.hyp_tok), _p(st.seq), _p(st.len), st.B, st.nb, st.max_length, cur_len,
                                        eos_id, pad_id, float(cur_len - len_offset) ** length_penalty, _stream()),
          "m3ae_beam_finalize")
    return st.seq, st.len


class OpenCountWatch:
    """The early exit of the device-resident search loop (search.run, the one loop of all six searches).  Steps after every row is
    done change no token, so leaving the loop is an optimisation only.  The count of open rows after each step is copied to pinned
    host memory behind the step, with an event; the host runs at most `lookahead` steps past the newest step whose event has
    completed (it waits on the event of the step `lookahead` back, so the device always has work queued) and stops enqueuing once a
    completed step reports zero.  Steps are numbered from `first`; lookahead=None never stops (and copies nothing)."""

    def __init__(self, n_steps, lookahead, first=0):
        if lookahead is not None and lookahead < 1:
            raise ValueError("lookahead must be >= 1 or None")
        self.lookahead, self.first = lookahead, first
        self.seen = first - 1                # newest step whose event is known to have completed
        if lookahead is not None:
            self.host = torch.empty(n_steps, dtype=torch.int32, pin_memory=True)
            self.np = self.host.numpy()      # read through numpy: plain host memory, filled by the copies below
            self.events = {}

    def enqueued(self, open_count, t):
        """Call after step t has been enqueued (open_count int32 [n_steps] on the device, slot t written by it).  True: stop."""
        if self.lookahead is None:
            return False
        self.host[t:t + 1].copy_(open_count[t:t + 1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[t] = ev
        back = t + 1 - self.lookahead
        if back >= self.first:               # step t + 1 may be enqueued once step t + 1 - lookahead is through
            self.events[back].synchronize()
            self.seen = max(self.seen, back)
        while self.seen < t and self.events[self.seen + 1].query():
            self.seen += 1
        return any(self.np[s] == 0 for s in range(self.first, self.seen + 1))


# ------------------------------------------------------------------------------------------------------------
# device-resident greedy search (csrc/greedy.hip): Decoder.search_path_async
# ------------------------------------------------------------------------------------------------------------
GREEDY_CHUNK = 2048   # vocabulary elements per workgroup of m3ae_greedy_argmax when the caller passes chunk=0


def _logits_rows(what, logits, rows=None):
    """The check of every entry point that reads rows of logits the way csrc/row_scan.h does: fp32 or bf16 [R, V], unit column
    stride, row stride >= V (R == rows where given).  Returns (R, V)."""
    _need_cuda(logits)
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{what} takes fp32 or bf16 logits")
    shape = logits.shape           # read once: these checks run per decoding step, where the host's enqueue is the bound
    if (len(shape) != 2 or shape[0] < 1 or shape[1] < 1 or (rows is not None and shape[0] != rows) or logits.stride(1) != 1
            or logits.stride(0) < shape[1]):
        raise ValueError(f"{what}: logits {tuple(shape)} with strides {tuple(logits.stride())}"
                         + ("" if rows is None else f" for {rows} rows"))
    return shape


def _chunk_arg(what, chunk):
    """chunk as an int: 0 (the kernel's default) or within the bounds of csrc/row_scan.h."""
    chunk = int(chunk)
    if chunk != 0 and not 64 <= chunk <= 65536:
        raise ValueError(f"{what}: chunk={chunk} is neither 0 nor in [64, 65536]")
    return chunk


def _chunk_workspace(what, nbytes, entry, R, V, device, chunk):
    """int64 [R, words of a row]: the workspace of `entry`, whose size in bytes nbytes(R, V, chunk) gives."""
    n = nbytes(R, V, chunk)
    if n <= 0:
        raise ValueError(f"{what}: R={R}, V={V}, chunk={chunk} is not a shape {entry} takes")
    return torch.empty((R, n // (8 * R)), dtype=torch.int64, device=device)


def greedy_workspace(R, V, device, chunk=0):
    """The keys buffer of greedy_argmax: int64 [R, chunks of a row] (the bits of the kernels' uint64 order keys)."""
    return _chunk_workspace("greedy_workspace", _lib.lib().m3ae_greedy_workspace_bytes, "m3ae_greedy_argmax", R, V, device, chunk)


def greedy_argmax(logits, chunk=0, ws=None, out=None):
    """logits fp32 or bf16 [R, V] (row stride >= V, unit column stride) -> the keys buffer `ws` int64 [R, chunks]: per vocabulary
    chunk the greatest order key (value, then lowest column), for greedy_step.  With `out` (int64 [R], for direct testing) the
    decoded tokens are written there and returned instead: torch.argmax's choice, ties and NaN included."""
    R, V = _logits_rows("greedy_argmax", logits)
    if ws is None:
        ws = greedy_workspace(R, V, logits.device, chunk)
    if ws.dtype != torch.int64 or not ws.is_contiguous() or not ws.is_cuda:
        raise ValueError("greedy_argmax: ws is the int64 buffer of greedy_workspace")
    if out is not None and (out.dtype != torch.int64 or tuple(out.shape) != (R,) or not out.is_contiguous() or not out.is_cuda):
        raise ValueError("greedy_argmax: out int64 [R], contiguous")
    check(_lib.lib().m3ae_greedy_argmax(_p(logits), logits.stride(0), R, V, chunk, _dt(logits), _p(ws), ws.numel() * 8, _p(out),
                                        _stream()), "m3ae_greedy_argmax")
    return ws if out is None else out


class GreedyState(_SearchState):
    """The device state of one greedy search (include/m3ae_hip.h, m3ae_greedy_step): allocated once per search_path call."""
    err_text = "device greedy search: a decoded token left [0, vocab_size)"

    def __init__(self, B, max_len, device, cls_id=101, pad_id=0, **more):
        self.B, self.max_len = B, max_len
        self.alloc_out(device, seq=(B, max_len), len=(B,), **more)
        self.seq.fill_(pad_id)
        self.len.fill_(max_len)
        self.last_tok = torch.full((B,), cls_id, dtype=torch.int64, device=device)
        self.finished = torch.zeros((B,), dtype=torch.int32, device=device)
        self.open_count = torch.zeros((max_len,), dtype=torch.int32, device=device)


def greedy_step(st, keys, V, pos, sep_id, eos_id, pad_id):
    """One step of the search on `st` at position pos from the keys of greedy_argmax (eos_id None or < 0: no second end token);
    st.open_count[pos] = rows still unfinished afterwards."""
    _need_cuda(keys)
    _need_cuda(st.out)
    if keys.dtype != torch.int64 or keys.dim() != 2 or keys.shape[0] != st.B or not keys.is_contiguous():
        raise ValueError("greedy_step: keys int64 [B, chunks], contiguous (the buffer greedy_argmax returns)")
    if not 0 <= pos < st.max_len:
        raise ValueError(f"greedy_step: pos {pos} outside [0, {st.max_len})")
    check(_lib.lib().m3ae_greedy_step(_p(keys), keys.shape[1], _p(st.seq), _p(st.len), _p(st.last_tok), _p(st.finished), _p(st.open_count),
                                      _p(st.err), st.B, V, st.max_len, pos, sep_id, -1 if eos_id is None else eos_id, pad_id, _stream()),
          "m3ae_greedy_step")


# ------------------------------------------------------------------------------------------------------------
# answer-list decoding (csrc/answer_trie.hip): Decoder.answer_path_async, T5.constrained_greedy_async
# ------------------------------------------------------------------------------------------------------------
TRIE_CHUNK = 8192   # vocabulary elements per workgroup of m3ae_trie_scan when the caller passes chunk=0


def trie_workspace(R, V, device, chunk=0):
    """The workspace of trie_scan / trie_step: int64 [R, 1 + chunks of a row] words (the child keys, then the (m, s) pairs)."""
    return _chunk_workspace("trie_workspace", _lib.lib().m3ae_trie_workspace_bytes, "m3ae_trie_scan", R, V, device, chunk)


class TrieState(GreedyState):
    """The device state of one answer-list search (include/m3ae_hip.h, m3ae_trie_step): allocated once per call.  The greedy
    search's state plus each row's trie node, label and score (in `out` as the beam state's n-best list with nb = 1)."""
    err_text = "answer-list decoding: the answer table led a row out of its range"
    k_text, nb = "answer_result: k={k} needs a beam search (num_beams >= k); the greedy search returns one entry", 1

    def __init__(self, B, max_len, device, start_id=101, pad_id=0):
        super().__init__(B, max_len, device, start_id, pad_id, labels=(B, 1), scores=(B, 1))
        self.label, self.score = self.labels[:, 0], self.scores[:, 0]
        self.label.fill_(-1)
        self.node = torch.zeros((B,), dtype=torch.int32, device=device)


def _trie_ws(what, ws, B, V, chunk):
    need = _lib.lib().m3ae_trie_workspace_bytes(B, V, chunk)
    if need <= 0:
        raise ValueError(f"{what}: B={B}, V={V}, chunk={chunk} is not a shape m3ae_trie_scan takes")
    if ws.dtype != torch.int64 or not ws.is_contiguous() or not ws.is_cuda or ws.numel() * 8 < need:
        raise ValueError(f"{what}: ws is the int64 buffer of trie_workspace")
    return need // (8 * B) - 1


def trie_scan(logits, trie, st, chunk=0, ws=None):
    """logits fp32 or bf16 [B, V] (row stride >= V, unit column stride), read once: per open row of `st` the (m, s) pair of every
    vocabulary chunk and the greatest order key among the children of the row's trie node, into `ws`.  Returns ws."""
    _need_cuda(st.out)
    B, V = _logits_rows("trie_scan", logits, st.B)
    chunk = _chunk_arg("trie_scan", chunk)
    if ws is None:
        ws = trie_workspace(B, V, logits.device, chunk)
    _trie_ws("trie_scan", ws, B, V, chunk)
    check(_lib.lib().m3ae_trie_scan(_p(logits), logits.stride(0), B, V, chunk, _dt(logits), _p(trie.child_off), _p(trie.child_tok), trie.N,
                                    trie.E, _p(st.node), _p(st.finished), _p(ws), ws.numel() * 8, _stream()), "m3ae_trie_scan")
    return ws


def trie_step(logits, trie, st, ws, pos, pad_id, chunk=0):
    """One step of the search on `st` at position pos from the workspace trie_scan filled from the same logits (same chunk):
    token, next node, score += log-probability, label / len / finished at a leaf; st.open_count[pos] = rows still open."""
    _need_cuda(st.out)
    B, V = _logits_rows("trie_step", logits, st.B)
    nch = _trie_ws("trie_step", ws, B, V, int(chunk))
    if not 0 <= pos < st.max_len:
        raise ValueError(f"trie_step: pos {pos} outside [0, {st.max_len})")
    check(_lib.lib().m3ae_trie_step(_p(logits), logits.stride(0), _dt(logits), _p(ws), ws.numel() * 8, nch, _p(trie.child_off),
                                    _p(trie.child_tok), _p(trie.child_node), _p(trie.leaf_label), trie.N, trie.E, _p(st.seq), _p(st.len),
                                    _p(st.label), _p(st.score), _p(st.last_tok), _p(st.node), _p(st.finished), _p(st.open_count), _p(st.err),
                                    B, V, st.max_len, pos, pad_id, _stream()), "m3ae_trie_step")


# ------------------------------------------------------------------------------------------------------------
# constrained beam search on the answer list (csrc/trie_beam.hip): Decoder.answer_beam_async, T5.constrained_beam_async
# ------------------------------------------------------------------------------------------------------------
TRIE_MAX_BEAMS = 8


class TrieBeamState(_SearchState):
    """The device state of one constrained beam search (include/m3ae_hip.h, m3ae_triebeam_step): allocated once per call.
    R = B * nb beam rows; `B` is the row count trie_scan sees (it runs over the beam rows with `finished` = the dead flags), `Bs`
    the number of samples.  The result is the hypothesis list of every sample, in `out`."""
    err_text, k_text = TrieState.err_text, "answer_result: k={k} outside [1, num_beams={nb}]"

    def __init__(self, Bs, nb, max_len, device, start_id=101, pad_id=0):
        if not 1 <= nb <= TRIE_MAX_BEAMS:
            raise ValueError(f"TrieBeamState: num_beams={nb} outside [1, {TRIE_MAX_BEAMS}]")
        R = Bs * nb
        self.Bs, self.nb, self.B, self.max_len, self.pad_id = Bs, nb, R, max_len, pad_id
        self.alloc_out(device, seq=(Bs, max_len), len=(Bs,), labels=(Bs, nb), scores=(Bs, nb), logprob=(Bs, nb), n_hyp=(Bs,))
        self.seq.fill_(pad_id)
        self.labels.fill_(-1)
        self.label, self.score = self.labels[:, 0], self.scores[:, 0]
        z = functools.partial(torch.zeros, device=device)
        self.hyp_len, self.best = z((Bs, nb), dtype=torch.int64), z((Bs,), dtype=torch.int64)
        self.node = z((Bs, nb), dtype=torch.int32)
        self.node[:, 1:] = -1
        self.node = self.node.view(-1)
        self.finished = (self.node < 0).to(torch.int32)          # the dead flags: trie_scan's `finished`
        self.beam_score = z((R,), dtype=torch.float32)
        self.last_tok = torch.full((Bs, nb), pad_id, dtype=torch.int64, device=device)
        self.last_tok[:, 0] = start_id
        self.last_tok = self.last_tok.view(-1)
        self.order = torch.arange(Bs, device=device, dtype=torch.int64).repeat_interleave(nb) * nb
        self.done = z((Bs,), dtype=torch.int32)
        self.open_count = z((max_len,), dtype=torch.int32)
        self.top_s = z((Bs, 2 * nb), dtype=torch.float32)
        self.top_beam, self.top_edge = z((Bs, 2 * nb), dtype=torch.int32), z((Bs, 2 * nb), dtype=torch.int32)
        self.n_cand = z((Bs,), dtype=torch.int32)


def trie_beam_select(logits, trie, st, ws, chunk=0):
    """The candidate selection of one step: logits fp32 or bf16 [B * nb, V] as trie_scan took them, `ws` the workspace trie_scan
    filled from them (same chunk).  Per sample the best min(2 nb, candidates) children of its live beams' nodes by
    fl(fl(x[tok] - lse) + beam_score), into st.top_s / st.top_beam / st.top_edge / st.n_cand."""
    _need_cuda(st.out)
    R, V = _logits_rows("trie_beam_select", logits, st.B)
    _trie_ws("trie_beam_select", ws, R, V, int(chunk))
    check(_lib.lib().m3ae_triebeam_select(_p(logits), logits.stride(0), st.Bs, st.nb, V, int(chunk), _dt(logits), _p(trie.child_off),
                                           _p(trie.child_tok), trie.N, trie.E, _p(st.node), _p(st.beam_score), _p(ws), ws.numel() * 8,
                                           _p(st.top_s), _p(st.top_beam), _p(st.top_edge), _p(st.n_cand), _p(st.err), _stream()),
          "m3ae_triebeam_select")
    return st.top_s, st.top_beam, st.top_edge, st.n_cand


def trie_beam_step(trie, st, V, pos, length_penalty=0.0):
    """One BeamSearchScorer step on `st` at position pos from the candidates trie_beam_select left in it: hypotheses, the next
    beams (st.node / beam_score / last_tok), st.order (the gather index of the caches), the dead flags (st.finished) and
    st.open_count[pos] = samples not done."""
    _need_cuda(st.out)
    if not 0 <= pos < st.max_len:
        raise ValueError(f"trie_beam_step: pos {pos} outside [0, {st.max_len})")
    check(_lib.lib().m3ae_triebeam_step(_p(st.top_s), _p(st.top_beam), _p(st.top_edge), _p(trie.child_off), _p(trie.child_tok),
                                         _p(trie.child_node), _p(trie.leaf_label), trie.N, trie.E, _p(st.node), _p(st.beam_score),
                                         _p(st.last_tok), _p(st.order), _p(st.finished), _p(st.done), _p(st.n_hyp), _p(st.labels),
                                         _p(st.scores), _p(st.logprob), _p(st.hyp_len), _p(st.best), _p(st.len), _p(st.open_count),
                                         _p(st.err), st.Bs, st.nb, V, trie.A, st.max_len, pos, st.pad_id, float(pos + 1) ** length_penalty,
                                         _stream()), "m3ae_triebeam_step")


def trie_beam_result(trie, st):
    """st.seq = the token rows of the best hypotheses, gathered on the device from the pad-filled answers table of `trie`
    (AnswerTrie.to_device(..., pad_id=...)): int64 rows moved as pairs of fp32 words by m3ae_gather_rows.  The kernel is called
    directly, not through `gather_rows`: that wrapper is an autograd node over fp32 / bf16 tensors which allocates its output, and
    here an int64 table is copied bit for bit INTO st.out, so that one copy still brings the whole result to the host.  st.best is
    written by m3ae_triebeam_step alone, which takes only labels in [0, A) (A = the rows of the table, checked below)."""
    tab = trie.answers
    if tab.shape[0] != trie.A or st.best.dtype != torch.int64 or tuple(st.best.shape) != (st.Bs,) or not tab.is_cuda:
        raise ValueError(f"trie_beam_result: the answers table has {tab.shape[0]} rows for {trie.A} answers, or the state is not this search's")
    if tab.dtype != torch.int64 or tuple(tab.shape) != (tab.shape[0], st.max_len) or not tab.is_contiguous():
        raise ValueError(f"trie_beam_result: the answers table int64 [A, {st.max_len}]")
    check(_lib.lib().m3ae_gather_rows(_p(tab), _p(st.best), _p(st.seq), st.Bs, 2 * st.max_len, F32, _stream()), "m3ae_gather_rows")
    return st.seq


# ------------------------------------------------------------------------------------------------------------
# exhaustive answer-list scoring (csrc/tree_attn.hip, csrc/list_score.hip): Decoder.answer_scores_async
# ------------------------------------------------------------------------------------------------------------
LIST_MAX_K, LIST_MAX_DEPTH = 16, 32


def tree_attention(q, k, v, anc, heads, scale=None, rel_bias=None, err=None):
    """Attention whose keys are a row's trie ancestors (m3ae_tree_attn): q, k, v [G, Ni, D] or [Ni, D] (fp32 or bf16, unit last
    stride, rows of a group one row stride apart: thirds of a packed qkv buffer qualify), anc int32 [Ni, Dmax <= 32] contiguous
    (AnswerTrie.score_tables), rel_bias fp32 [heads, Dmax] or None, err int64 [1] (allocated when None).  D / heads is 64 or 96.
    Returns out [.., Ni, D] in the input dtype, contiguous; err is set by a table value out of range (that row is zeros)."""
    for t in (q, k, v, anc):
        _need_cuda(t)
    shape = q.shape
    if q.dim() == 2:
        q, k, v = q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0)
    if q.dim() != 3 or k.shape != q.shape or v.shape != q.shape or k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"tree_attention: q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)} {k.dtype}, v {tuple(v.shape)} {v.dtype}")
    G, Ni, D = q.shape
    if G < 1 or Ni < 1 or D % heads:
        raise ValueError(f"tree_attention: shape {tuple(q.shape)} for {heads} heads")
    for t in (q, k, v):
        if t.stride(2) != 1 or t.stride(1) < D or (G > 1 and t.stride(0) != Ni * t.stride(1)):
            raise ValueError(f"tree_attention: strides {tuple(t.stride())} (unit last stride, groups a whole number of rows apart)")
    if anc.dtype != torch.int32 or anc.dim() != 2 or anc.shape[0] != Ni or not 1 <= anc.shape[1] <= LIST_MAX_DEPTH or not anc.is_contiguous():
        raise ValueError(f"tree_attention: anc int32 [{Ni}, 1 .. {LIST_MAX_DEPTH}], contiguous")
    Dmax = anc.shape[1]
    if rel_bias is not None and (rel_bias.dtype != torch.float32 or tuple(rel_bias.shape) != (heads, Dmax) or not rel_bias.is_contiguous()
                                 or not rel_bias.is_cuda):
        raise ValueError(f"tree_attention: rel_bias fp32 [{heads}, {Dmax}], contiguous")
    if err is None:
        err = torch.zeros((1,), dtype=torch.int64, device=q.device)
    elif err.dtype != torch.int64 or err.numel() != 1 or not err.is_cuda:
        raise ValueError("tree_attention: err int64 [1]")
    Dh = D // heads
    out = torch.empty((G, Ni, D), dtype=q.dtype, device=q.device)
    check(_lib.lib().m3ae_tree_attn(_p(q), q.stride(1), _p(k), k.stride(1), _p(v), v.stride(1), _p(out), D, _p(anc), Dmax, _p(rel_bias),
                                    (1.0 / math.sqrt(Dh)) if scale is None else float(scale), G, Ni, heads, Dh, _dt(q), _p(err), _stream()),
          "m3ae_tree_attn")
    return out.view(*shape[:-1], D)


def listscore_workspace(R, V, device, chunk=0):
    """The workspace of listscore_lse / listscore_edges: int64 [R, chunks of a row] words (the bits of the fp32 (m, s) pairs)."""
    return _chunk_workspace("listscore_workspace", _lib.lib().m3ae_listscore_workspace_bytes, "m3ae_listscore_lse", R, V, device, chunk)


class ListScoreState(_SearchState):
    """The device state of one exhaustive scoring of the answer list (include/m3ae_hip.h, m3ae_listscore_fold): allocated once per
    call.  `trie` is what AnswerTrie.score_to_device returned.  The k best entries of every sample with scores, log-probabilities and
    probabilities over the list, the list's log-mass and the token row of the best entry live in `out`; all_logprob double [B, A]
    has a buffer of its own, as have the scratch arrays (edge_lp fp32 [B, E], best int64 [B], the fold's workspace)."""
    err_text, k_text = TrieState.err_text, "answer_result: k={k} outside [1, the k={nb} the list was scored with]"

    def __init__(self, B, k, max_len, trie, device, pad_id=0):
        k = int(k)
        if not 1 <= k <= LIST_MAX_K:
            raise ValueError(f"ListScoreState: k={k} outside [1, {LIST_MAX_K}]")
        if trie.depth > max_len or trie.depth > LIST_MAX_DEPTH:
            raise ValueError(f"ListScoreState: the longest answer has {trie.depth} tokens, there is room for {min(max_len, LIST_MAX_DEPTH)}")
        self.B, self.nb, self.max_len, self.pad_id = B, k, max_len, pad_id
        self.alloc_out(device, seq=(B, max_len), len=(B,), labels=(B, k), scores=(B, k), logprob=(B, k), probs=(B, k), log_mass=(B,),
                       n_hyp=(B,))
        self.label, self.score = self.labels[:, 0], self.scores[:, 0]
        self.all_logprob = torch.zeros((B, trie.A), dtype=torch.float64, device=device)
        self.edge_lp = torch.zeros((B, trie.E), dtype=torch.float32, device=device)
        self.best = torch.zeros((B,), dtype=torch.int64, device=device)
        need = _lib.lib().m3ae_listscore_fold_workspace_bytes(B, trie.N)
        if need < 0:
            raise ValueError(f"ListScoreState: B={B}, N={trie.N} is not a shape m3ae_listscore_fold takes")
        self.fold_ws = torch.empty((need // 8,), dtype=torch.float64, device=device) if need else None


def _listscore_ws(what, ws, R, V, chunk):
    need = _lib.lib().m3ae_listscore_workspace_bytes(R, V, chunk)
    if need <= 0:
        raise ValueError(f"{what}: R={R}, V={V}, chunk={chunk} is not a shape m3ae_listscore_lse takes")
    if ws.dtype != torch.int64 or not ws.is_contiguous() or not ws.is_cuda or ws.numel() * 8 < need:
        raise ValueError(f"{what}: ws is the int64 buffer of listscore_workspace")
    return need // (8 * R)


def listscore_lse(logits, chunk=0, ws=None):
    """logits fp32 or bf16 [R, V] (row stride >= V, unit column stride), read once: the (m, s) pair of every vocabulary chunk of
    every row, into `ws` (listscore_workspace).  Returns ws."""
    R, V = _logits_rows("listscore_lse", logits)
    chunk = _chunk_arg("listscore_lse", chunk)
    if ws is None:
        ws = listscore_workspace(R, V, logits.device, chunk)
    _listscore_ws("listscore_lse", ws, R, V, chunk)
    check(_lib.lib().m3ae_listscore_lse(_p(logits), logits.stride(0), R, V, chunk, _dt(logits), _p(ws), ws.numel() * 8, _stream()),
          "m3ae_listscore_lse")
    return ws


def listscore_edges(logits, trie, st, ws, first=0, chunk=0):
    """logits [G * Ni, V] of samples first .. first + G - 1 (row g * Ni + i: sample first + g at node trie.internal[i]) and the
    workspace listscore_lse filled from them (same chunk): st.edge_lp[first + g, e] = x[tok_e] - lse for every edge of the trie."""
    _need_cuda(st.out)
    R, V = _logits_rows("listscore_edges", logits)
    G, Ni = R // trie.Ni, trie.Ni
    if G * Ni != R or first < 0 or first + G > st.B or tuple(st.edge_lp.shape) != (st.B, trie.E):
        raise ValueError(f"listscore_edges: {R} rows for {Ni} internal nodes, samples {first} .. {first + G - 1} of {st.B}")
    nch = _listscore_ws("listscore_edges", ws, R, V, _chunk_arg("listscore_edges", chunk))
    check(_lib.lib().m3ae_listscore_edges(_p(logits), logits.stride(0), G, Ni, V, _dt(logits), _p(ws), ws.numel() * 8, nch, _p(trie.internal),
                                           _p(trie.child_off), _p(trie.child_tok), trie.N, trie.E, _p(st.edge_lp[first:]), _p(st.err), _stream()),
          "m3ae_listscore_edges")


def listscore_fold(trie, st, length_penalty=0.0):
    """Every entry's log-probability from st.edge_lp, the list's log-mass and the k best entries of every sample (m3ae_listscore_fold),
    then st.seq = the token rows of the best entries, gathered on the device from the answers table (as trie_beam_result)."""
    _need_cuda(st.out)
    tab = trie.answers
    if (tab.dtype != torch.int64 or tuple(tab.shape) != (trie.A, st.max_len) or not tab.is_contiguous() or not tab.is_cuda
            or tuple(st.all_logprob.shape) != (st.B, trie.A) or tuple(st.edge_lp.shape) != (st.B, trie.E) or trie.E != trie.N - 1):
        raise ValueError(f"listscore_fold: the answers table int64 [{trie.A}, {st.max_len}] and a state built for this list")
    pen = trie.pen.get(float(length_penalty))
    if pen is None:      # len ** length_penalty per depth, uploaded once per value: pos + 1 is per leaf here
        host = torch.tensor([1.0] + [float(d) ** float(length_penalty) for d in range(1, trie.depth + 1)], dtype=torch.float64)
        pen = trie.pen[float(length_penalty)] = host.pin_memory().to(tab.device, non_blocking=True)
    ws = st.fold_ws
    check(_lib.lib().m3ae_listscore_fold(_p(st.edge_lp), _p(trie.parent), _p(trie.node_depth), _p(trie.level_off), _p(trie.leaf_node), _p(pen),
                                          st.B, trie.N, trie.A, trie.depth, st.nb, _p(ws), 0 if ws is None else ws.numel() * 8,
                                          _p(st.all_logprob), _p(st.labels), _p(st.scores), _p(st.logprob), _p(st.probs), _p(st.log_mass),
                                          _p(st.n_hyp), _p(st.best), _p(st.len), _p(st.err), _stream()), "m3ae_listscore_fold")
    check(_lib.lib().m3ae_gather_rows(_p(tab), _p(st.best), _p(st.seq), st.B, 2 * st.max_len, F32, _stream()), "m3ae_gather_rows")
    return st


# ------------------------------------------------------------------------------------------------------------
# device-side VQA evaluation (csrc/vqa_eval.hip): m3ae_amd/metrics.py, M3AETransformerSS.predict
# ------------------------------------------------------------------------------------------------------------
class VqaRows(NamedTuple):
    """The per-row outputs of vqa_eval(want_rows=True); topk_* are None for k = 0, hit1 without targets."""
    pred: torch.Tensor                 # int64 [B]: torch.max(logits, 1)[1]
    topk_idx: torch.Tensor | None      # int32 [B, k]
    topk_prob: torch.Tensor | None     # fp32 [B, k]
    hit1: torch.Tensor | None          # fp32 [B]


def vqa_record(device):
    """A zeroed record of vqa_eval / seq_match: float64 [10] (include/m3ae_hip.h)."""
    return torch.zeros((_lib.VQA_REC_DOUBLES,), dtype=torch.float64, device=device)


def _eval_common(what, B, types, rec, device):
    if types is not None:
        _need_cuda(types)
        if types.dtype != torch.int32 or tuple(types.shape) != (B,) or not types.is_contiguous():
            raise ValueError(f"{what}: types int32 [B], contiguous")
    if rec is not None:
        _need_cuda(rec)
        if rec.dtype != torch.float64 or tuple(rec.shape) != (_lib.VQA_REC_DOUBLES,) or not rec.is_contiguous():
            raise ValueError(f"{what}: rec float64 [{_lib.VQA_REC_DOUBLES}], contiguous (ops.vqa_record)")
        return torch.empty((B, 2), dtype=torch.float32, device=device)
    return None


def vqa_eval(logits, targets, types, rec, k=0, want_rows=False):
    """One update of the VQA score record from a batch, enqueued on the current stream (no host sync).
    logits fp32 or bf16 [B, C] (row stride >= C, unit column stride: the [..., :498] view of vocab_linear's padded buffer is
    taken as it is); targets fp32 [B, C] or None; types int32 [B] (_lib.ANS_CLOSED / ANS_OPEN, anything else: "all" only) or
    None; rec float64 [10] (ops.vqa_record) or None.  Adds {n, hit1, hitk} of the rows onto rec, where hit1 is the target of
    torch.max(logits, 1)[1] and hitk the best target among the top-k (0 <= k <= 16).  want_rows: returns VqaRows."""
    B, Cc = _logits_rows("vqa_eval", logits)
    k = int(k)
    if not 0 <= k <= min(_lib.VQA_MAX_K, Cc):
        raise ValueError(f"vqa_eval: k={k} outside [0, min({_lib.VQA_MAX_K}, C={Cc})]")
    if targets is not None:
        _need_cuda(targets)
        if targets.dtype != torch.float32 or tuple(targets.shape) != (B, Cc) or targets.stride(1) != 1 or targets.stride(0) < Cc:
            raise ValueError(f"vqa_eval: targets fp32 {(B, Cc)}, unit column stride; got {targets.dtype} {tuple(targets.shape)}")
    ws = _eval_common("vqa_eval", B, types, rec if targets is not None else None, logits.device)
    if rec is not None and targets is None:
        raise ValueError("vqa_eval: a record needs targets")
    dev = logits.device
    pred = idx = prob = hit1 = None
    if want_rows:
        pred = torch.empty((B,), dtype=torch.int64, device=dev)
        if k:
            idx = torch.empty((B, k), dtype=torch.int32, device=dev)
            prob = torch.empty((B, k), dtype=torch.float32, device=dev)
        if targets is not None:
            hit1 = torch.empty((B,), dtype=torch.float32, device=dev)
    check(_lib.lib().m3ae_vqa_eval(_p(logits), logits.stride(0), _p(targets), 0 if targets is None else targets.stride(0), _p(types), B,
                                   Cc, k, _dt(logits), _p(pred), _p(idx), _p(prob), _p(hit1), _p(rec), _p(ws),
                                   0 if ws is None else ws.numel() * 4, _stream()), "m3ae_vqa_eval")
    return VqaRows(pred, idx, prob, hit1) if want_rows else None


def seq_match(gen, ref, skip, types, rec, want_rows=False):
    """Token exact match of generated ids against reference ids, enqueued on the current stream (no host sync): gen int64
    [B, Lg], ref int64 [B, Lr] (unit column stride), skip int64 [ns <= 8] on the device (ids dropped from both sides before the
    compare: pad / start / end), types and rec as vqa_eval.  Adds {n, match, match} of the rows onto rec.  want_rows: the
    per-row int32 [B] (1 = match).  Equal ids imply equal strings: a lower bound of the reference's string exact match."""
    _need_cuda(gen)
    _need_cuda(ref)
    _need_cuda(skip)
    for name, t in (("gen", gen), ("ref", ref)):
        if t.dtype != torch.int64 or t.dim() != 2 or t.shape[0] != gen.shape[0] or t.shape[0] < 1 or \
                (t.shape[1] > 0 and (t.stride(1) != 1 or t.stride(0) < t.shape[1])):
            raise ValueError(f"seq_match: {name} int64 [B, L], unit column stride; got {t.dtype} {tuple(t.shape)} {tuple(t.stride())}")
    if skip.dtype != torch.int64 or skip.dim() != 1 or skip.shape[0] > _lib.SEQ_MAX_SKIP or not skip.is_contiguous():
        raise ValueError(f"seq_match: skip int64 [ns], ns <= {_lib.SEQ_MAX_SKIP}")
    if rec is None:
        raise ValueError("seq_match: rec is required (ops.vqa_record)")
    B = gen.shape[0]
    ws = _eval_common("seq_match", B, types, rec, gen.device)
    match = torch.empty((B,), dtype=torch.int32, device=gen.device) if want_rows else None
    check(_lib.lib().m3ae_seq_match(_p(gen), gen.stride(0), gen.shape[1], _p(ref), ref.stride(0), ref.shape[1],
                                    _p(skip) if skip.shape[0] else None, skip.shape[0], _p(types), B, _p(match), _p(rec), _p(ws),
                                    ws.numel() * 4, _stream()), "m3ae_seq_match")
    return match


class LabelRows(NamedTuple):
    """The per-row outputs of vqa_label_eval(want_rows=True)."""
    hit1: torch.Tensor                 # fp32 [B]: targets[r, labels[r]] (0 for a label outside [0, C))
    err: torch.Tensor                  # int64 [1]: 1 after a label outside [0, C)


def vqa_label_eval(labels, targets, types, rec, err=None, want_rows=False):
    """One update of the VQA score record from LABELS (answer-list decoding: a generator head's output is a list entry), enqueued
    on the current stream (no host sync).  labels int64 [B]; targets fp32 [B, C] (unit column stride); types and rec as vqa_eval
    (rec is required).  Adds {n, t, t} with t = targets[r, labels[r]] onto rec.  err: an int64 [1] device word that is set to 1
    by a label outside [0, C) (such a row scores 0); a fresh one is made when None.  Returns err, or LabelRows with want_rows."""
    _need_cuda(labels)
    _need_cuda(targets)
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] < 1 or not labels.is_contiguous():
        raise ValueError(f"vqa_label_eval: labels int64 [B], contiguous; got {labels.dtype} {tuple(labels.shape)}")
    B = labels.shape[0]
    if targets.dtype != torch.float32 or targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] < 1 or targets.stride(1) != 1 \
            or targets.stride(0) < targets.shape[1]:
        raise ValueError(f"vqa_label_eval: targets fp32 [{B}, C], unit column stride; got {targets.dtype} {tuple(targets.shape)}")
    if rec is None:
        raise ValueError("vqa_label_eval: rec is required (ops.vqa_record)")
    ws = _eval_common("vqa_label_eval", B, types, rec, labels.device)
    if err is None:
        err = torch.zeros((1,), dtype=torch.int64, device=labels.device)
    elif err.dtype != torch.int64 or err.numel() != 1 or not err.is_cuda:
        raise ValueError("vqa_label_eval: err int64 [1] on the device")
    hit1 = torch.empty((B,), dtype=torch.float32, device=labels.device) if want_rows else None
    check(_lib.lib().m3ae_vqa_label_eval(_p(labels), _p(targets), targets.stride(0), _p(types), B, targets.shape[1], _p(hit1), _p(rec),
                                         _p(err), _p(ws), ws.numel() * 4, _stream()), "m3ae_vqa_label_eval")
    return LabelRows(hit1, err) if want_rows else err


def _labels_shape(what, labels, B=None):
    """The shape rule of n-best labels (needs no device): int64 [B, k], 1 <= k <= 16, unit column stride, row stride >= k."""
    if labels.dtype != torch.int64 or labels.dim() != 2 or labels.shape[0] < 1 or (B is not None and labels.shape[0] != B) or \
            not 1 <= labels.shape[1] <= _lib.VQA_MAX_K or labels.stride(1) != 1 or labels.stride(0) < labels.shape[1]:
        raise ValueError(f"{what}: labels int64 [B, k] with 1 <= k <= {_lib.VQA_MAX_K}, unit column stride; got {labels.dtype} "
                         f"{tuple(labels.shape)} {tuple(labels.stride())}")
    return labels.shape


def vqa_labels_eval(labels, targets, types, rec, err=None, want_rows=False):
    """The n-best form of vqa_label_eval (a constrained beam search's `labels`): labels int64 [B, k] (a view with a row stride is
    taken as it is), -1 in columns 1.. = an empty slot.  Adds {n, targets[r, labels[r, 0]], max over the row's entries of
    targets[r, l]} onto rec.  Any other value outside [0, C), or an empty column 0, scores 0 and sets err.  Returns err, or
    LabelRows with want_rows."""
    B, k = _labels_shape("vqa_labels_eval", labels)
    _need_cuda(labels)
    _need_cuda(targets)
    if targets.dtype != torch.float32 or targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] < 1 or targets.stride(1) != 1 \
            or targets.stride(0) < targets.shape[1]:
        raise ValueError(f"vqa_labels_eval: targets fp32 [{B}, C], unit column stride; got {targets.dtype} {tuple(targets.shape)}")
    if rec is None:
        raise ValueError("vqa_labels_eval: rec is required (ops.vqa_record)")
    ws = _eval_common("vqa_labels_eval", B, types, rec, labels.device)
    if err is None:
        err = torch.zeros((1,), dtype=torch.int64, device=labels.device)
    elif err.dtype != torch.int64 or err.numel() != 1 or not err.is_cuda:
        raise ValueError("vqa_labels_eval: err int64 [1] on the device")
    hit1 = torch.empty((B,), dtype=torch.float32, device=labels.device) if want_rows else None
    check(_lib.lib().m3ae_vqa_labels_eval(_p(labels), labels.stride(0), k, _p(targets), targets.stride(0), _p(types), B, targets.shape[1],
                                          _p(hit1), _p(rec), _p(err), _p(ws), ws.numel() * 4, _stream()), "m3ae_vqa_labels_eval")
    return LabelRows(hit1, err) if want_rows else err


# ------------------------------------------------------------------------------------------------------------
# device-side token evaluation for rows of vocabulary width (csrc/token_eval.hip): m3ae_amd/metrics.py (TokenAccuracy, LossMean),
# M3AETransformerSS.fill_mask
# ------------------------------------------------------------------------------------------------------------
class TokenRows(NamedTuple):
    """The per-row outputs of token_eval(want_rows=True / want_topk=True); a group that was not asked for is None.  A row that was
    not evaluated holds pred -1, rank -1, nll 0, topk_idx -1, topk_prob 0."""
    pred: torch.Tensor | None          # int64 [R]: torch.argmax(logits, -1)
    rank: torch.Tensor | None          # int32 [R]: columns ranked above the label (0: a hit); -1 without a label
    nll: torch.Tensor | None           # fp32 [R]: logsumexp(row) - row[label]
    topk_idx: torch.Tensor | None      # int32 [R, k]
    topk_prob: torch.Tensor | None     # fp32 [R, k]: softmax probabilities
    err: torch.Tensor | None           # int64 [1]: 1 after a label that is neither -100 nor in [0, V) (with labels)


def token_record(device):
    """A zeroed record of token_eval: float64 [5] = {n, hit1, hitk, sum_nll, calls} (include/m3ae_hip.h)."""
    return torch.zeros((_lib.TOKEN_REC_DOUBLES,), dtype=torch.float64, device=device)


def token_eval(logits, labels=None, select=None, rec=None, k=0, chunk=0, want_rows=False, want_topk=False):
    """One update of the token record from the rows of `logits`, enqueued on the current stream (no host sync).
    logits fp32 or bf16 [R, V] (row stride >= V, unit column stride: the [..., :V] view of vocab_linear's padded buffer is taken as
    it is); labels int64 [R] or None (-100: no label); select uint8 / bool [R] or None; rec float64 [5] (ops.token_record) or None.
    Evaluated rows: select != 0 if given, else labels != -100 if given, else all; the logits of the other rows are not read.
    Adds {n, rank == 0, rank < k, nll} of the labelled evaluated rows onto rec.  0 <= k <= min(16, V); chunk: columns per workgroup
    (0: 8192).  want_rows: pred / rank / nll, want_topk: topk_idx / topk_prob (k > 0), returned as TokenRows."""
    R, V = _logits_rows("token_eval", logits)
    k = int(k)
    if not 0 <= k <= min(_lib.TOKEN_MAX_K, V):
        raise ValueError(f"token_eval: k={k} outside [0, min({_lib.TOKEN_MAX_K}, V={V})]")
    chunk = _chunk_arg("token_eval", chunk)
    if want_topk and k == 0:
        raise ValueError("token_eval: want_topk needs k > 0")
    dev = logits.device
    if labels is not None:
        _need_cuda(labels)
        if labels.dtype != torch.int64 or tuple(labels.shape) != (R,) or not labels.is_contiguous():
            raise ValueError(f"token_eval: labels int64 [{R}], contiguous; got {labels.dtype} {tuple(labels.shape)}")
    if select is not None:
        _need_cuda(select)
        if select.dtype not in (torch.uint8, torch.bool) or tuple(select.shape) != (R,) or not select.is_contiguous():
            raise ValueError(f"token_eval: select uint8 / bool [{R}], contiguous; got {select.dtype} {tuple(select.shape)}")
    if rec is not None:
        _need_cuda(rec)
        if rec.dtype != torch.float64 or tuple(rec.shape) != (_lib.TOKEN_REC_DOUBLES,) or not rec.is_contiguous():
            raise ValueError(f"token_eval: rec float64 [{_lib.TOKEN_REC_DOUBLES}], contiguous (ops.token_record)")
    L = _lib.lib()
    need = L.m3ae_token_eval_workspace_bytes(R, V, chunk, k)
    if need <= 0:
        raise ValueError(f"token_eval: unsupported shape R={R}, V={V}, chunk={chunk}, k={k}")
    ws = torch.empty((need // 8,), dtype=torch.int64, device=dev)
    err = torch.zeros((1,), dtype=torch.int64, device=dev) if labels is not None else None
    pred = rank = nll = idx = prob = None
    if want_rows:
        pred = torch.empty((R,), dtype=torch.int64, device=dev)
        rank = torch.empty((R,), dtype=torch.int32, device=dev)
        nll = torch.empty((R,), dtype=torch.float32, device=dev)
    if want_topk:
        idx = torch.empty((R, k), dtype=torch.int32, device=dev)
        prob = torch.empty((R, k), dtype=torch.float32, device=dev)
    check(L.m3ae_token_eval(_p(logits), logits.stride(0), _p(labels), _p(select), R, V, chunk, k, _dt(logits), _p(pred), _p(rank),
                            _p(nll), _p(idx), _p(prob), _p(rec), _p(err), _p(ws), need, _stream()), "m3ae_token_eval")
    return TokenRows(pred, rank, nll, idx, prob, err) if (want_rows or want_topk) else None


def record_add(value, rec):
    """rec[0] += value, rec[1] += 1 in double on the device (metrics.LossMean): value a device fp32 scalar (0-d or [1]), rec a
    float64 [2] device tensor.  Enqueued on the current stream; no ATen arithmetic, no host sync."""
    _need_cuda(value)
    _need_cuda(rec)
    if value.dtype != torch.float32 or value.numel() != 1:
        raise ValueError(f"record_add: value is one fp32 number on the device; got {value.dtype} {tuple(value.shape)}")
    if rec.dtype != torch.float64 or tuple(rec.shape) != (2,) or not rec.is_contiguous():
        raise ValueError("record_add: rec float64 [2], contiguous")
    check(_lib.lib().m3ae_record_add(_p(value), _p(rec), _stream()), "m3ae_record_add")


# ------------------------------------------------------------------------------------------------------------
# masked-image-modelling bookkeeping (pre-training)
# ------------------------------------------------------------------------------------------------------------
def mask_ranks(noise, len_keep):
    """random_masking's index work (m3ae_module.py:153-183) -> ids_restore [B, L] int64, keep_rows [B * (len_keep + 1)]
    int64 (flat token-row ids, class row first), mask [B, L] fp32 (1 = removed)."""
    _need_cuda(noise)
    B, L = noise.shape
    n = noise.contiguous().float()
    ids_restore = torch.empty((B, L), dtype=torch.long, device=noise.device)
    keep_rows = torch.empty((B, len_keep + 1), dtype=torch.long, device=noise.device)
    mask = torch.empty((B, L), dtype=torch.float32, device=noise.device)
    check(_lib.lib().m3ae_mask_ranks(_p(n), _p(ids_restore), _p(keep_rows), _p(mask), B, L, len_keep, _stream()),
          "m3ae_mask_ranks")
    return ids_restore, keep_rows.view(-1), mask


def mim_targets(img, patch, norm_pix):
    """patchify (m3ae_module.py:185-192) [+ per-patch standardisation, objectives.py:52-56]: [B, C, H, W] -> [B, L, P*P*C]."""
    _need_cuda(img)
    B, Cc, H, W = img.shape
    x = img.contiguous().float()
    out = torch.empty((B, (H // patch) * (W // patch), patch * patch * Cc), dtype=torch.float32, device=img.device)
    check(_lib.lib().m3ae_mim_targets(_p(x), _p(out), B, Cc, H, W, patch, int(bool(norm_pix)), _stream()), "m3ae_mim_targets")
    return out


class MimLossFn(Function):
    """objectives.py:58-62 on the decoder output WITH its class row (x [B, L + 1, D]): masked per-patch MSE."""

    @staticmethod
    def forward(ctx, x, target, mask):
        _need_cuda(x)
        xc = x.contiguous()
        B, L1, D = xc.shape
        t, m = target.contiguous().float(), mask.contiguous().float()
        acc = torch.empty(2, dtype=torch.float32, device=x.device)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        if _DETERMINISTIC:
            ws, n = _small_ws(_lib.DET_MIM, B * (L1 - 1), D, x.device)
            check(_lib.lib().m3ae_mim_loss_fwd_det(_p(xc), _p(t), _p(m), _p(acc), _p(loss), B, L1 - 1, D, _dt(xc), _p(ws), n,
                                                   _stream()), "m3ae_mim_loss_fwd_det")
        else:
            check(_lib.lib().m3ae_mim_loss_fwd(_p(xc), _p(t), _p(m), _p(acc), _p(loss), B, L1 - 1, D, _dt(xc), _stream()),
                  "m3ae_mim_loss_fwd")
        ctx.save_for_backward(xc, t, m, acc)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        xc, t, m, acc = ctx.saved_tensors
        B, L1, D = xc.shape
        dx = torch.empty_like(xc)
        go = g.detach().reshape(1).float().contiguous()
        check(_lib.lib().m3ae_mim_loss_bwd(_p(xc), _p(t), _p(m), _p(acc), _p(go), _p(dx), B, L1 - 1, D, _dt(xc), _stream()),
              "m3ae_mim_loss_bwd")
        return dx, None, None


def mim_loss(x_with_cls, target, mask):
    return MimLossFn.apply(x_with_cls, target, mask)
