"""CPU: the rule of csrc/vqa_eval.hip as tests/vqa_eval_model.py states it, against torch on CPU; the exactness of the record's sums
(what lets tests/test_gpu_vqa_eval.py demand bit equality); config validation; the record reduction over gloo; answers()."""
import os
import socket
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import vqa_eval_model as model
from m3ae_amd import _lib, config, metrics
from m3ae_amd.modules.m3ae_module import M3AETransformerSS, answers_of


def test_the_new_entry_points_are_bound():
    for name in ("m3ae_vqa_eval_workspace_bytes", "m3ae_vqa_eval", "m3ae_seq_match"):
        assert name in _lib.EXPORTS
    assert (_lib.ANS_CLOSED, _lib.ANS_OPEN, _lib.VQA_REC_DOUBLES) == (model.ANS_CLOSED, model.ANS_OPEN, model.REC) == (0, 1, 10)
    assert hasattr(M3AETransformerSS, "predict") and hasattr(M3AETransformerSS, "answers")


@pytest.mark.parametrize("C", [1, 7, 498])
def test_rank0_is_torch_max_on_cpu_and_sum_top1_is_the_reference_expression(C):
    """Rows with ties, a tie with the maximum, all-equal rows, +-0, +-inf, one and several NaNs: rank 0 of the model equals
    torch.max(x, 1)[1] and torch.argmax (first index on ties, the first NaN wins, -0 == +0), and sum_top1 equals the reference's
    one-hot scatter times target, summed (my_metrics.py:63-74)."""
    rng = np.random.default_rng(C)
    x = np.concatenate([model.special_rows(C, rng), rng.standard_normal((5, C)).astype(np.float32)])
    t = rng.choice(np.array([0.0, 0.3, 0.6, 0.9, 1.0], dtype=np.float32), size=x.shape)
    xt, tt = torch.from_numpy(x), torch.from_numpy(t)
    got = model.evaluate(x, t, None, 1)
    want = torch.max(xt, 1)[1]
    assert torch.equal(torch.from_numpy(got["pred"]), want) and torch.equal(want, torch.argmax(xt, dim=1))
    one_hots = torch.zeros_like(tt)
    one_hots.scatter_(1, want.view(-1, 1), 1)
    scores = one_hots * tt
    assert got["rec"][1] == float(scores.double().sum()) and got["rec"][0] == x.shape[0]
    assert np.array_equal(got["hit1"], scores.sum(1).numpy())


def test_the_cpu_conventions_the_rule_restates():
    assert int(torch.argmax(torch.tensor([1.0, 3.0, 3.0, 2.0]))) == 1                                  # first index on ties
    assert int(torch.argmax(torch.tensor([1.0, float("nan"), float("inf"), float("nan")]))) == 1       # the first NaN wins
    assert int(torch.argmax(torch.tensor([-1.0, -0.0, 0.0]))) == 1 and int(torch.argmax(torch.tensor([-1.0, 0.0, -0.0]))) == 1
    assert model.rank_row(np.array([1.0, np.nan, np.inf, np.nan], dtype=np.float32), 4).tolist() == [1, 3, 2, 0]
    assert model.rank_row(np.array([-1.0, -0.0, 0.0, -np.inf], dtype=np.float32), 4).tolist() == [1, 2, 0, 3]


@pytest.mark.parametrize("C,k", [(7, 1), (7, 7), (498, 5), (498, 16), (4099, 16)])
def test_topk_is_torch_topk_on_tie_free_rows(C, k):
    rng = np.random.default_rng(C * 31 + k)
    x = np.stack([rng.permutation(C).astype(np.float32) - C / 3 for _ in range(6)])      # distinct values in every row
    want = torch.topk(torch.from_numpy(x), k, dim=1)
    got = model.evaluate(x, None, None, k)
    assert np.array_equal(got["topk"], want.indices.numpy())
    assert np.allclose(got["prob"], torch.sigmoid(want.values.double()).numpy(), rtol=1e-15, atol=0)


SCORES = [Fraction(3, 10), Fraction(6, 10), Fraction(9, 10), Fraction(1), Fraction(1, 10), Fraction(1, 3), Fraction(1, 2 ** 20), Fraction(0)]


def test_sums_of_up_to_1024_scores_are_exact_in_double_in_any_order():
    """Scores in {0} u [2^-20, 1] as fp32: every value is a multiple of 2^-43 (an fp32 of exponent >= -20 has its last bit at
    2^-43 or above) and a sum of at most 1024 of them is below 2^10, so it needs at most 53 bits: a double sum is exact in any
    order.  200 random draws, two orders, against fractions.Fraction."""
    vals = np.array([float(s) for s in SCORES], dtype=np.float32)
    assert all(v == 0 or 2.0 ** -20 <= v <= 1 for v in vals.tolist())
    assert all((Fraction(float(v)) * 2 ** 43).denominator == 1 for v in vals)
    rng = np.random.default_rng(7)
    for _ in range(200):
        n = int(rng.integers(1, 1025))
        draw = rng.choice(vals, size=n)
        exact = sum((Fraction(float(v)) for v in draw), Fraction(0))
        fwd = 0.0
        for v in draw:
            fwd += float(v)
        perm = 0.0
        for v in draw[rng.permutation(n)]:
            perm += float(v)
        assert Fraction(fwd) == exact and Fraction(perm) == exact
        assert Fraction(float(np.sum(draw.astype(np.float64)))) == exact           # numpy's pairwise order too


def test_record_groups_and_empty_groups():
    hit1 = np.array([1.0, 0.3, 0.0, 0.6, 0.9], dtype=np.float32)
    hitk = np.array([1.0, 0.6, 0.3, 0.6, 1.0], dtype=np.float32)
    rec = model.record(hit1, hitk, [0, 1, 2, 0, 1])
    r = metrics.record_result(rec)
    assert r == model.result(rec)
    assert (r["n"], r["n_closed"], r["n_open"]) == (5, 2, 2)
    f = lambda *v: float(sum(np.float64(np.float32(x)) for x in v))
    assert r["score"] == f(1.0, 0.3, 0.0, 0.6, 0.9) / 5 and r["closed"] == f(1.0, 0.6) / 2 and r["open"] == f(0.3, 0.9) / 2
    assert r["score_at_k"] == f(1.0, 0.6, 0.3, 0.6, 1.0) / 5
    only_open = metrics.record_result(model.record(hit1, hitk, [1] * 5))
    assert only_open["closed"] == 0.0 and only_open["n_closed"] == 0 and only_open["open"] == only_open["score"]
    untyped = metrics.record_result(model.record(hit1, hitk, None))
    assert untyped["closed"] == 0.0 and untyped["open"] == 0.0 and untyped["n"] == 5
    empty = metrics.record_result(np.zeros(10))
    assert empty == {"score": 0.0, "closed": 0.0, "open": 0.0, "score_at_k": 0.0, "n": 0, "n_closed": 0, "n_open": 0}


def test_seq_match_model():
    skip = (0, 101, 102)
    gen = [[7, 8, 102, 0, 0], [7, 8, 102, 0, 0], [0, 0, 0, 0, 0], [7, 0, 8, 102, 9]]
    ref = [[101, 7, 8, 102], [101, 7, 9, 102], [101, 102, 0, 0], [101, 7, 8, 9]]
    assert model.seq_match(gen, ref, skip).tolist() == [1, 0, 1, 1]
    assert model.seq_match(gen, ref, ()).tolist() == [0, 0, 0, 0]


def test_vqa_metrics_key_is_validated_at_compose_and_parse_time():
    assert config.DEFAULTS["vqa_metrics"] == "host" and config.DEFAULTS["eval_topk"] == 5 and config.VQA_METRICS == ("host", "device")
    assert config.tiny_config()["vqa_metrics"] == "host"
    assert config.tiny_config(vqa_metrics="device", eval_topk=0)["vqa_metrics"] == "device"
    assert config.parse_cli(["with", "task_finetune_vqa_vqa_rad", "vqa_metrics=device", "eval_topk=16"])["eval_topk"] == 16
    for bad in ("gpu", "Device", 1, None):
        with pytest.raises(ValueError, match="vqa_metrics"):
            config.tiny_config(vqa_metrics=bad)
    with pytest.raises(ValueError, match="vqa_metrics"):
        config.parse_cli(["with", "task_finetune_vqa_vqa_rad", "vqa_metrics=cuda"])
    for bad in (17, -1, 2.5, True, "5"):
        with pytest.raises(ValueError, match="eval_topk"):
            config.tiny_config(vqa_metrics="device", eval_topk=bad)
    assert config.tiny_config(eval_topk=99)["eval_topk"] == 99      # honoured, and checked, only with "device"


def test_answers_mapping_and_its_key_error():
    label2ans = {"0": "yes", "1": "no", "7": "left lung"}
    out = answers_of([[7, 0], [1, 7]], [[0.9, 0.25], [0.5, 0.125]], label2ans)
    assert out == [[("left lung", 0.9), ("yes", 0.25)], [("no", 0.5), ("left lung", 0.125)]]
    with pytest.raises(KeyError, match="label 3 "):
        answers_of([[0, 3]], [[0.5, 0.5]], label2ans)
    with pytest.raises(KeyError, match="label 0 "):
        answers_of([[0]], [[0.5]], {0: "an int key is not the reference's convention"})


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_record(rank):
    hit1 = np.array([1.0, 0.3, 0.0, 0.6][:3 + rank], dtype=np.float32)
    return model.record(hit1, np.maximum(hit1, np.float32(0.6)), [0, 1, 2, 1][:3 + rank])


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rec = torch.from_numpy(_rank_record(rank).copy())
        got = metrics.reduce_record(rec)
        assert got is rec
        out.put((rank, rec.tolist()))
    finally:
        dist.destroy_process_group()


def test_record_reduction_over_a_world_of_two_gloo():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    res = sorted(out.get(timeout=10) for _ in range(2))
    want = (_rank_record(0) + _rank_record(1)).tolist()
    assert res[0][1] == want and res[1][1] == want
    r = metrics.record_result(want)
    assert (r["n"], r["n_closed"], r["n_open"]) == (7, 2, 3) and want[9] == 2.0


def test_reduce_record_without_a_group_is_the_identity():
    rec = torch.arange(10, dtype=torch.float64)
    assert metrics.reduce_record(rec) is rec and rec.tolist() == list(range(10))
