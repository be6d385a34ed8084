"""CPU: the contract of csrc/token_eval.hip as tests/token_eval_model.py states it, against torch on CPU (argmax, topk,
F.cross_entropy, the reference's Accuracy metric, torch.logsumexp on non-finite rows); the model's fold; config validation of
`pretrain_metrics`; TokenAccuracy / LossMean / PretrainMetrics with the two ops stubbed; the binding of the new entry points."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_eval_model as M
from vqa_eval_model import special_rows
from m3ae_amd import _lib, config, metrics, ops
from m3ae_amd.modules.m3ae_module import M3AETransformerSS


def test_the_new_entry_points_are_bound():
    for name in ("m3ae_token_eval_workspace_bytes", "m3ae_token_eval", "m3ae_record_add"):
        assert name in _lib.EXPORTS
    assert (_lib.TOKEN_REC_DOUBLES, _lib.TOKEN_MAX_K, _lib.TOKEN_IGNORE) == (M.REC, 16, M.IGNORE) == (5, 16, -100)
    assert hasattr(M3AETransformerSS, "fill_mask") and hasattr(ops, "token_eval") and hasattr(ops, "token_record")


def reference_accuracy(logits, target):
    """my_metrics.Accuracy.update / compute transcribed: detach, argmax over the last dimension, drop target == -100, count."""
    logits, target = logits.detach(), target.detach()
    preds = logits.argmax(dim=-1)
    preds = preds[target != -100]
    target = target[target != -100]
    if target.numel() == 0:
        return 0, 0
    assert preds.shape == target.shape
    return int(torch.sum(preds == target)), int(target.numel())


def tie_free(R, V, seed):
    """fp32 rows with pairwise distinct values (asserted): a permutation of V equally spaced numbers, scaled to a softmax's range."""
    rng = np.random.default_rng(seed)
    x = np.stack([(rng.permutation(V).astype(np.float32) - np.float32(V / 3)) * np.float32(12.0 / V) for _ in range(R)])
    assert all(len(np.unique(row)) == V for row in x)
    return x


@pytest.mark.parametrize("V,k", [(1, 1), (7, 7), (65, 5), (1000, 16), (30522, 5)])
def test_model_equals_cpu_torch_on_tie_free_rows(V, k):
    R = 12
    x = tie_free(R, V, V + k)
    rng = np.random.default_rng(V)
    labels = rng.integers(0, V, size=R).astype(np.int64)
    labels[::3] = M.IGNORE
    labels[1] = int(np.argmax(x[1]))                                      # a hit
    got = M.evaluate(x, labels, None, k)
    xt, lt = torch.from_numpy(x), torch.from_numpy(labels)
    ev = labels != M.IGNORE
    assert np.array_equal(got["ev"], ev) and got["err"] == 0
    assert np.array_equal(got["pred"][ev], torch.argmax(xt, dim=1).numpy()[ev]) and (got["pred"][~ev] == -1).all()
    top = torch.topk(xt, k, dim=1)
    assert np.array_equal(got["topk"][ev], top.indices.numpy()[ev])
    assert np.allclose(got["prob"][ev], torch.softmax(xt.double(), 1).gather(1, top.indices).numpy()[ev], rtol=1e-12, atol=0)
    # the record against the reference metric and F.cross_entropy in float64
    rank32, nll32 = got["rank"], got["nll"].astype(np.float32)
    rec = M.fold(rank32, nll32, k)
    correct, total = reference_accuracy(xt.view(3, 4, V), lt.view(3, 4))
    assert (rec[0], rec[1], rec[4]) == (total, correct, 1.0) and rec[2] >= rec[1]
    assert rec[2] == sum(int(labels[r]) in got["topk"][r] for r in np.nonzero(ev)[0])
    ce = F.cross_entropy(xt.double(), lt, ignore_index=-100, reduction="sum").item()
    assert abs(got["nll"][ev].sum() - ce) <= 1e-12 * max(abs(ce), 1.0)
    assert M.result(rec)["accuracy"] == correct / total and M.result(rec)["n"] == total


@pytest.mark.parametrize("V", [1, 7, 65])
def test_model_follows_torch_on_tied_and_non_finite_rows(V):
    """argmax: the lowest column among equals, the first NaN above everything; lse: torch.logsumexp's value; rank 0 iff preds ==
    target, so a label that ties the maximum from a higher column is no hit."""
    rng = np.random.default_rng(V)
    x = special_rows(V, rng)
    xt = torch.from_numpy(x)
    labels = np.array([min(i % 5, V - 1) for i in range(x.shape[0])], dtype=np.int64)
    got = M.evaluate(x, labels, None, min(3, V))
    want = torch.argmax(xt, dim=1)
    assert np.array_equal(got["pred"], want.numpy())
    assert np.array_equal(got["rank"] == 0, (want == torch.from_numpy(labels)).numpy())
    lse = torch.logsumexp(xt.double(), dim=1).numpy()
    assert np.array_equal(np.isnan(got["lse"]), np.isnan(lse))
    fin = np.isfinite(lse)
    assert np.array_equal(got["lse"][~fin & ~np.isnan(lse)], lse[~fin & ~np.isnan(lse)])      # +-inf as torch gives them
    assert np.allclose(got["lse"][fin], lse[fin], rtol=1e-14, atol=0)
    if V >= 7:
        r = np.full(V, np.float32(-2.0))
        r[1] = r[4] = np.float32(3.0)                                                         # the maximum twice
        for label, rank in ((1, 0), (4, 1), (0, 2), (6, 6)):
            assert M.evaluate(r[None], np.array([label]), None, 0)["rank"][0] == rank, label


def test_row_selection_and_label_errors():
    x = tie_free(6, 9, 3)
    labels = np.array([0, M.IGNORE, 9, -1, -101, 8], dtype=np.int64)
    got = M.evaluate(x, labels, None, 2)
    assert got["err"] == 1 and got["ev"].tolist() == [True, False, False, False, False, True]
    assert got["rank"][1:5].tolist() == [-1] * 4 and (got["topk"][1:5] == -1).all() and (got["nll"][1:5] == 0).all()
    sel = np.array([0, 1, 0, 0, 0, 1], dtype=np.uint8)                       # select overrides labels: row 1 runs without a label
    got = M.evaluate(x, labels, sel, 2)
    assert got["err"] == 0 and got["ev"].tolist() == [False, True, False, False, False, True]
    assert got["rank"][1] == -1 and got["nll"][1] == got["lse"][1] and got["rank"][5] >= 0
    got = M.evaluate(x, None, None, 0)
    assert got["ev"].all() and (got["rank"] == -1).all() and M.fold(got["rank"], got["nll"], 0).tolist() == [0, 0, 0, 0, 1]


def test_fold_is_a_plain_sum_in_a_fixed_order():
    rng = np.random.default_rng(1)
    R = 700
    rank = rng.integers(-2, 9, size=R).astype(np.int32)
    nll = rng.random(R).astype(np.float32) * 11
    rec = M.fold(rank, nll, 5)
    lab = rank >= 0
    assert rec[0] == lab.sum() and rec[1] == (rank == 0).sum() and rec[2] == (lab & (rank < 5)).sum()
    assert abs(rec[3] - nll[lab].astype(np.float64).sum()) <= 1e-12 * rec[3]
    rec2 = M.fold(rank, nll, 5, rec)
    assert rec2[4] == 2.0 and rec2[0] == 2 * rec[0] and abs(rec2[3] - 2 * rec[3]) <= 1e-12 * rec2[3]
    assert M.result(np.zeros(5)) == {"accuracy": 0.0, "accuracy_at_k": 0.0, "n": 0, "nll": 0.0, "perplexity": 0.0}


def test_the_bound_is_a_few_hundred_units_and_grows_with_the_chunk():
    assert M.path_units(1000, 0, 4) == 2 + (4 * 1 + 2) + 3 * 3 + 72 + 4
    assert M.path_units(50265, 0, 2) == 2 + (8 * 4 + 2) + 3 * 6 + 72 + 4
    assert M.path_units(50265, 65536, 4) > M.path_units(50265, 0, 4)
    x = tie_free(1, 1000, 0)[0]
    nll, b = M.nll_bound(x, 3, 0, 4)
    assert 0 < b < 2.0 ** -24 * (M.path_units(1000, 0, 4) + 40 + 2 * abs(nll))


def test_pretrain_metrics_config_key():
    assert config.DEFAULTS["pretrain_metrics"] == "host" and config.pretrain_metrics({}) == "host"
    assert config.compose("task_pretrain_m3ae", pretrain_metrics="device")["pretrain_metrics"] == "device"
    assert config.parse_cli(["task_pretrain_m3ae", "pretrain_metrics=device", "eval_topk=3"])["eval_topk"] == 3
    for bad in ("gpu", "", None, 1, True):
        with pytest.raises(ValueError, match="pretrain_metrics"):
            config.compose("task_pretrain_m3ae", pretrain_metrics=bad)
    for bad in (17, -1, 2.0, True, "5"):
        with pytest.raises(ValueError, match="eval_topk"):
            config.compose("task_pretrain_m3ae", pretrain_metrics="device", eval_topk=bad)
    assert config.compose("task_pretrain_m3ae", eval_topk=17)["eval_topk"] == 17          # not looked at with "host"


class Calls:
    """Stand-ins for ops.token_eval / ops.record_add that note their arguments and add a known increment onto the record."""

    def __init__(self, monkeypatch):
        self.token, self.add = [], []
        monkeypatch.setattr(ops, "token_eval", self.token_eval)
        monkeypatch.setattr(ops, "record_add", self.record_add)

    def token_eval(self, logits, labels=None, select=None, rec=None, k=0, chunk=0, want_rows=False, want_topk=False):
        self.token.append(dict(logits=logits, labels=labels, select=select, k=k, chunk=chunk, want_rows=want_rows))
        lab = labels != -100
        rec += torch.tensor([float(lab.sum()), float((lab & (labels == 0)).sum()), float(lab.sum()), 2.0 * float(lab.sum()), 1.0], dtype=torch.float64)

    def record_add(self, value, rec):
        self.add.append(value)
        rec += torch.tensor([float(value), 1.0], dtype=torch.float64)


def test_token_accuracy_call_shapes_empty_case_and_result_keys(monkeypatch):
    calls = Calls(monkeypatch)
    met = metrics.TokenAccuracy("cpu", k=5)
    assert isinstance(met, metrics._DeviceRecordMetric) and tuple(met.rec.shape) == (5,) and met.rec.dtype == torch.float64
    empty = met.result()
    assert empty == {"accuracy": 0.0, "accuracy_at_k": 0.0, "n": 0, "nll": 0.0, "perplexity": 0.0} and met.compute() == 0.0
    padded = torch.zeros(2, 3, 16)
    logits = padded[..., :10]                                       # the head's [..., :V] view: flattened without a copy
    target = torch.tensor([[0.0, -100.0, 3.0], [-100.0, -100.0, 0.0]])        # float targets, as the ITM labels are
    assert met.update(logits, target) is None
    c = calls.token[0]
    assert tuple(c["logits"].shape) == (6, 10) and c["logits"].stride() == (16, 1) and c["logits"].data_ptr() == padded.data_ptr()
    assert c["labels"].dtype == torch.int64 and c["labels"].tolist() == [0, -100, 3, -100, -100, 0] and c["select"] is None and c["k"] == 5
    met.update(torch.zeros(4, 2), torch.tensor([1, 0, -100, 0]))    # two classes: k is clipped to the width
    assert calls.token[1]["k"] == 2 and calls.token[1]["labels"].tolist() == [1, 0, -100, 0]
    out = met.result()
    assert set(out) == {"accuracy", "accuracy_at_k", "n", "nll", "perplexity"}
    assert out["n"] == 6 and out["accuracy"] == 4 / 6 and out["accuracy_at_k"] == 1.0 and out["nll"] == 2.0
    assert out["perplexity"] == pytest.approx(np.exp(2.0), rel=1e-15) and met.compute() == 4 / 6
    met.update(torch.zeros(2, 2), torch.tensor([-100, -100]))       # nothing labelled: only `calls` moves
    assert met.result()["n"] == 6 and met.rec[4].item() == 3.0
    met.reset()
    assert met.result() == empty
    with pytest.raises(ValueError):
        met.update(torch.zeros(2, 3, 4), torch.zeros(2, 4))
    with pytest.raises(ValueError):
        met.update(torch.zeros(3, 2, 8).transpose(0, 1), torch.zeros(2, 3))       # rows that do not flatten without a copy
    with pytest.raises(ValueError):
        metrics.TokenAccuracy("cpu", k=17)
    assert metrics.token_result([1.0, 0.0, 0.0, 1e6, 1.0])["perplexity"] == float("inf")


def test_loss_mean_is_the_reference_scalar(monkeypatch):
    calls = Calls(monkeypatch)
    met = metrics.LossMean("cpu")
    assert met.result() == {"mean": 0.0, "n": 0} and met.compute() == 0.0
    for v in (0.5, 1.5, 4.0):
        met.update(torch.tensor(v))
    assert all(a.dtype == torch.float32 and tuple(a.shape) == (1,) for a in calls.add)
    assert met.result() == {"mean": 2.0, "n": 3} and met.compute() == 2.0            # sum of per-batch values / batches
    met.update(torch.tensor(1.0, dtype=torch.bfloat16))
    assert calls.add[-1].dtype == torch.float32 and met.result()["n"] == 4


def test_pretrain_metrics_share_one_buffer_and_report_what_was_fed(monkeypatch):
    Calls(monkeypatch)
    pm = metrics.PretrainMetrics("cpu", k=3)
    assert tuple(pm.flat.shape) == (16,) and pm.mlm.rec.data_ptr() == pm.flat.data_ptr() and pm.itm.k == 0
    assert pm.result() == {}
    pm.update({"mlm_logits": torch.zeros(2, 3, 10), "mlm_labels": torch.tensor([[0, -100, 2], [-100, -100, -100]]), "mlm_loss": torch.tensor(3.0),
               "mim_loss": torch.tensor(0.25)})
    out = pm.result()
    assert set(out) == {"mlm", "mlm_loss", "mim_loss"} and out["mlm"]["n"] == 2 and out["mlm_loss"] == 3.0 and out["mim_loss"] == 0.25
    pm.update({"itm_logits": torch.zeros(4, 2), "itm_labels": torch.tensor([1.0, 0.0, 0.0, 1.0]), "itm_loss": torch.tensor(1.0)})
    out = pm.result()
    assert out["itm"]["n"] == 4 and out["itm"]["accuracy"] == 0.5 and out["itm_loss"] == 1.0 and out["mlm"]["n"] == 2


def test_default_mask_token_id_lookup():
    class Stub:
        default_mask_token_id = M3AETransformerSS.default_mask_token_id

        def __init__(self, cfg, tok=None):
            self.hparams = type("H", (), {"config": cfg})()
            if tok is not None:
                self.tokenizer = tok
    assert Stub({"tokenizer": "roberta-base"}).default_mask_token_id() == 50264
    assert Stub({"tokenizer": "downloaded/roberta-base"}).default_mask_token_id() == 50264
    assert Stub({"tokenizer": "bert-base-uncased"}).default_mask_token_id() == 103
    assert Stub({"tokenizer": "roberta-base", "mask_token_id": 7}).default_mask_token_id() == 7
    assert Stub({"tokenizer": "roberta-base", "mask_token_id": 7}, type("T", (), {"mask_token_id": 4})()).default_mask_token_id() == 4
