"""Validation metrics that live on the device (csrc/vqa_eval.hip): `VQARADScore` -- overall / closed / open VQA score and the
score within the top-k answers -- and `TokenExactMatch` for the generator heads; and the pre-training metrics (csrc/token_eval.hip):
`TokenAccuracy` -- the reference's `Accuracy` for the MLM / ITM objectives with accuracy within the top-k, mean negative
log-likelihood and perplexity -- and `LossMean`, the reference's `Scalar`; `PretrainMetrics` keeps them in one buffer.

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
import math

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

    def __init__(self, device="cuda", group=None, rec=None):
        self.device, self.group = torch.device(device), group
        self.rec = self.new_record(self.device) if rec is None else rec    # rec: a view of a buffer several metrics share
        self.best_score = self.best_close_score = self.best_open_score = 0.0

    @staticmethod
    def new_record(device):
        return ops.vqa_record(device)

    def reset(self):
        self.rec.zero_()

    def read(self):
        """The record over every update since reset(), all ranks included, as host numbers: one all-reduce (when a group exists)
        and one blocking copy."""
        rec = self.rec.clone() if self.group is not None or (dist.is_available() and dist.is_initialized()) else self.rec
        return reduce_record(rec, self.group).cpu().tolist()

    def result(self):
        """{"score", "closed", "open", "score_at_k", "n", "n_closed", "n_open"} over every update since reset(), all ranks
        included: one all-reduce (when a group exists) and one blocking copy of 10 doubles."""
        out = record_result(self.read())
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

    def update_labels(self, labels, target, types=None, want_rows=False):
        """The same update from LABELS (answer-list decoding of a generator head, ops.vqa_label_eval): labels int64 [B] on the
        device, target fp32 [B, C]; a row adds target[r, labels[r]] as its score and its score within the top-k alike.  A label
        outside [0, C) scores 0 and sets `self.label_err` (int64 [1] on the device).  labels int64 [B, k], 1 <= k <= 16 (the
        n-best list of a constrained beam search, -1 = an empty slot in columns 1..): the score is column 0's and the score
        within the top-k the best target among the row's entries.  Enqueues only."""
        if labels.dim() == 2:   # n-best labels [B, k] of a constrained beam search (ops.vqa_labels_eval): -1 = an empty slot in
            ops._labels_shape("update_labels", labels, target.shape[0])   # columns 1..; score_at_k is the best target among them
        elif labels.dim() != 1:
            raise ValueError(f"update_labels: labels int64 [B] or [B, k], got {tuple(labels.shape)}")
        if target.dtype != torch.float32:
            target = target.float()
        if getattr(self, "label_err", None) is None:
            self.label_err = torch.zeros((1,), dtype=torch.int64, device=labels.device)
        if labels.dim() == 2:
            return ops.vqa_labels_eval(labels.detach(), target.detach(), types_tensor(types, labels.device), self.rec,
                                       err=self.label_err, want_rows=want_rows)
        return ops.vqa_label_eval(labels.detach().contiguous(), target.detach(), types_tensor(types, labels.device), self.rec,
                                  err=self.label_err, want_rows=want_rows)


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


def token_result(rec):
    """The `TokenAccuracy.result()` dict of a token record given as 5 host numbers {n, hit1, hitk, sum_nll, calls}.  With no
    labelled row everything is 0.0, never a NaN; perplexity = exp(nll), inf where that overflows a double."""
    n, hit1, hitk, snll = (float(v) for v in rec[:4])
    if n == 0:
        return {"accuracy": 0.0, "accuracy_at_k": 0.0, "n": 0, "nll": 0.0, "perplexity": 0.0}
    nll = snll / n
    try:
        ppl = math.exp(nll)
    except OverflowError:
        ppl = float("inf")
    return {"accuracy": hit1 / n, "accuracy_at_k": hitk / n, "n": int(n), "nll": nll, "perplexity": ppl}


class TokenAccuracy(_DeviceRecordMetric):
    """The reference's `Accuracy` (my_metrics.py: preds = logits.argmax(-1), rows with target -100 dropped, correct / total) on
    the device, for logits of any width up to a vocabulary's: `update` enqueues ops.token_eval and returns.  k > 0 also keeps
    `accuracy_at_k` (the label among the k highest logits); `nll` is the mean of logsumexp(row) - row[label] over the labelled rows
    (F.cross_entropy's mean) and `perplexity` its exponential."""

    def __init__(self, device="cuda", k=0, group=None, rec=None):
        super().__init__(device, group, rec)
        if not 0 <= int(k) <= _lib.TOKEN_MAX_K:
            raise ValueError(f"k={k} outside [0, {_lib.TOKEN_MAX_K}]")
        self.k = int(k)

    @staticmethod
    def new_record(device):
        return ops.token_record(device)

    def update(self, logits, target, want_rows=False):
        """logits fp32 / bf16 [..., V] (the padded view of the head is taken as it is; the leading dimensions must flatten without
        a copy), target [...] of the same leading shape, int64 or any dtype that casts to it (-100: no label).  Enqueues only."""
        V = logits.shape[-1]
        if tuple(target.shape) != tuple(logits.shape[:-1]):
            raise ValueError(f"target {tuple(target.shape)} does not match the rows of logits {tuple(logits.shape)}")
        try:
            rows = logits.detach().view(-1, V)
        except RuntimeError:
            raise ValueError(f"logits {tuple(logits.shape)} with strides {tuple(logits.stride())} do not flatten to rows without a copy")
        labels = target.detach().reshape(-1)
        if labels.dtype != torch.int64:
            labels = labels.long()
        return ops.token_eval(rows, labels.contiguous(), None, self.rec, k=min(self.k, V), want_rows=want_rows)

    def result(self):
        """{"accuracy", "accuracy_at_k", "n", "nll", "perplexity"} over every update since reset(), all ranks included: one
        all-reduce (when a group exists) and one blocking copy of 5 doubles."""
        out = token_result(self.read())
        self.best_score = max(self.best_score, out["accuracy"])
        return out

    def compute(self):
        """The accuracy (the reference's return value)."""
        return self.result()["accuracy"]


def loss_result(rec):
    """{"mean", "n"} of a LossMean record given as 2 host numbers {sum, count}; 0.0 with no update."""
    total, n = float(rec[0]), float(rec[1])
    return {"mean": total / n if n != 0 else 0.0, "n": int(n)}


class LossMean(_DeviceRecordMetric):
    """The reference's `Scalar` (my_metrics.py): the sum of the per-batch values over the number of batches.  `update` takes the
    loss as the device scalar the step produced and adds it onto the record with one tiny launch (ops.record_add)."""

    @staticmethod
    def new_record(device):
        return torch.zeros((2,), dtype=torch.float64, device=device)

    def update(self, value):
        value = value.detach()
        if value.dtype != torch.float32:
            value = value.float()
        ops.record_add(value.reshape(1), self.rec)

    def result(self):
        return loss_result(self.read())

    def compute(self):
        return self.result()["mean"]


class PretrainMetrics:
    """The metrics of a pre-training validation pass in ONE device buffer, read with one all-reduce and one blocking copy:
    `mlm` (TokenAccuracy with k), `itm` (TokenAccuracy, two classes) and a LossMean per objective in `loss`."""
    OBJECTIVES = ("mlm", "itm", "mim")

    def __init__(self, device="cuda", k=0, group=None):
        self.device, self.group, self.k = torch.device(device), group, int(k)
        T = _lib.TOKEN_REC_DOUBLES
        self.flat = torch.zeros((2 * T + 2 * len(self.OBJECTIVES),), dtype=torch.float64, device=self.device)
        self.mlm = TokenAccuracy(self.device, k=self.k, group=group, rec=self.flat[:T])
        self.itm = TokenAccuracy(self.device, k=0, group=group, rec=self.flat[T:2 * T])
        self.loss = {name: LossMean(self.device, group=group, rec=self.flat[2 * T + 2 * i:2 * T + 2 * i + 2])
                     for i, name in enumerate(self.OBJECTIVES)}

    def update(self, ret):
        """From the `ret` of a pre-training forward: whatever of mlm_logits / itm_logits / {mlm, itm, mim}_loss it holds."""
        if "mlm_logits" in ret:
            self.mlm.update(ret["mlm_logits"], ret["mlm_labels"])
        if "itm_logits" in ret:
            self.itm.update(ret["itm_logits"], ret["itm_labels"])
        for name, m in self.loss.items():
            if f"{name}_loss" in ret:
                m.update(ret[f"{name}_loss"])

    def result(self):
        """{"mlm": TokenAccuracy result, "itm": ..., "mlm_loss" / "itm_loss" / "mim_loss": means} of what was fed (a metric with no
        update is left out)."""
        T = _lib.TOKEN_REC_DOUBLES
        rec = self.flat.clone() if self.group is not None or (dist.is_available() and dist.is_initialized()) else self.flat
        r = reduce_record(rec, self.group).cpu().tolist()
        out = {}
        if r[T - 1] > 0:
            out["mlm"] = token_result(r[:T])
        if r[2 * T - 1] > 0:
            out["itm"] = token_result(r[T:2 * T])
        for i, name in enumerate(self.OBJECTIVES):
            pair = r[2 * T + 2 * i:2 * T + 2 * i + 2]
            if pair[1] > 0:
                out[f"{name}_loss"] = loss_result(pair)["mean"]
        return out
