"""Validation metrics that live on the device (csrc/vqa_eval.hip): `VQARADScore` -- overall / closed / open VQA score and the
score within the top-k answers -- and `TokenExactMatch` for the generator heads.

`update` enqueues kernels on the current stream and returns; nothing is copied to the host until `compute` / `result`, which
make ONE small blocking copy (the 10 doubles of the record) and, when a process group exists, one SUM all-reduce of them first.

What closed / open mean here.  The method names are the reference's `VQARADScore` (m3ae/gadgets/my_metrics.py:165-199), the
closed / open ARITHMETIC is not, because the reference's has no defined value to be equal to:
  * my_metrics.py:180-181 multiplies the type mask by `self.score`, the RUNNING sum over all batches so far (a scalar), not by
    this batch's per-row scores: every closed row of batch n is credited the total of batches 1 .. n;
  * the counts (:184, :186) add `numel()` of that product, which has one entry per row of the batch whatever its type: both
    groups count every row.
The intended quantity is defined instead: closed = (sum of the top-1 scores of the rows whose answer type is CLOSED) / (number of
such rows), the same for open, and score = the same over all rows -- which IS the reference's overall VQAScore
(my_metrics.py:57-79).  A group with no rows reports 0.0, as the reference's `!= 0` guard does.
"""
import torch
import torch.distributed as dist

from . import _lib, ops

REC_N, REC_TOP1, REC_TOPK = 0, 1, 2      # offsets inside a group of the record
GROUPS = ("all", "closed", "open")       # record groups, in order (include/m3ae_hip.h)


def reduce_record(rec, group=None):
    """SUM all-reduce of a record over the process group (the default group when `group` is None), in place; a no-op without an
    initialised group or with a world of 1.  Takes device tensors (RCCL) and CPU tensors (gloo) alike."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(rec, op=dist.ReduceOp.SUM, group=group)
    return rec


def record_result(rec):
    """The `result()` dict of a record given as 10 host numbers."""
    r = [float(v) for v in rec]

    def ratio(num, den):
        return num / den if den != 0 else 0.0
    n, nc, no = r[0], r[3], r[6]
    return {"score": ratio(r[0 + REC_TOP1], n), "closed": ratio(r[3 + REC_TOP1], nc), "open": ratio(r[6 + REC_TOP1], no),
            "score_at_k": ratio(r[0 + REC_TOPK], n), "n": int(n), "n_closed": int(nc), "n_open": int(no)}


def types_tensor(types, device):
    """batch["answer_types"] (a host list of ints, or a tensor) as the int32 device tensor the kernels read; None stays None."""
    if types is None:
        return None
    if not isinstance(types, torch.Tensor):
        types = torch.tensor([int(t) for t in types], dtype=torch.int32)
    return types.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()


class _DeviceRecordMetric:
    """State and read-out shared by the two metrics: the device record, the best-so-far figures, compute / result / reset."""

    def __init__(self, device="cuda", group=None):
        self.device, self.group = torch.device(device), group
        self.rec = ops.vqa_record(self.device)
        self.best_score = self.best_close_score = self.best_open_score = 0.0

    def reset(self):
        self.rec.zero_()

    def result(self):
        """{"score", "closed", "open", "score_at_k", "n", "n_closed", "n_open"} over every update since reset(), all ranks
        included: one all-reduce (when a group exists) and one blocking copy of 10 doubles."""
        rec = self.rec.clone() if self.group is not None or (dist.is_available() and dist.is_initialized()) else self.rec
        out = record_result(reduce_record(rec, self.group).cpu().tolist())
        self.best_score = max(self.best_score, out["score"])
        self.best_close_score = max(self.best_close_score, out["closed"])
        self.best_open_score = max(self.best_open_score, out["open"])
        return out

    def compute(self):
        """The overall score (the reference's return value)."""
        return self.result()["score"]

    def get_best_score(self):
        return self.best_score

    def get_best_close_score(self):
        return self.best_close_score

    def get_best_open_score(self):
        return self.best_open_score


class VQARADScore(_DeviceRecordMetric):
    """Overall / closed / open VQA score on the device, with the reference's method names (see the module docstring for what
    closed / open mean and why that is not the reference's arithmetic).  k > 0 also keeps `score_at_k`: the best soft score among
    the k highest logits of a row."""

    def __init__(self, device="cuda", k=0, group=None):
        super().__init__(device, group)
        if not 0 <= int(k) <= _lib.VQA_MAX_K:
            raise ValueError(f"k={k} outside [0, {_lib.VQA_MAX_K}]")
        self.k = int(k)

    def update(self, logits, target, types=None, want_rows=False):
        """logits fp32 / bf16 [B, C] (the padded view of the head is taken as it is), target fp32 [B, C], types: None, a list
        of ints or an int tensor [B] (0 = closed, 1 = open).  Enqueues only."""
        if target.dtype != torch.float32:
            target = target.float()
        return ops.vqa_eval(logits.detach(), target.detach(), types_tensor(types, logits.device), self.rec,
                            k=min(self.k, logits.shape[1]), want_rows=want_rows)


class TokenExactMatch(_DeviceRecordMetric):
    """Exact match of generated token ids against reference token ids with the ids of `skip` (pad / start / end) dropped from both
    sides, overall / closed / open.  TOKEN exact match: equal ids imply equal decoded strings, so this is a lower bound of the
    reference's string VQAExactMatch (my_metrics.py:80-96), not that metric."""

    def __init__(self, skip, device="cuda", group=None):
        super().__init__(device, group)
        skip = sorted({int(s) for s in skip if s is not None})
        if len(skip) > _lib.SEQ_MAX_SKIP:
            raise ValueError(f"at most {_lib.SEQ_MAX_SKIP} skip ids, got {len(skip)}")
        self.skip = torch.tensor(skip, dtype=torch.int64).to(self.device)

    def update(self, gen, ref, types=None, want_rows=False):
        """gen int64 [B, Lg], ref int64 [B, Lr] on the device.  Enqueues only."""
        return ops.seq_match(gen, ref, self.skip, types_tensor(types, gen.device), self.rec, want_rows=want_rows)
