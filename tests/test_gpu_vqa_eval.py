"""GPU: device-side VQA evaluation (csrc/vqa_eval.hip) -- m3ae_vqa_eval and m3ae_seq_match against the numpy model of
tests/vqa_eval_model.py, exactly (indices, hit1 and the record bit for bit: the sums are exact, tests/test_vqa_eval_host.py); the
probabilities against float64 within a derived bound; the rejections; predict / answers / Trainer.validate / Trainer.test."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vqa_eval_model as M  # noqa: E402
from m3ae_amd import _lib, metrics, ops, synth, trainer  # noqa: E402
from oracle_util import tiny_batch, tiny_config  # noqa: E402

DEV = "cuda"
SOFT = np.array([0.0, 0.0, 0.0, 0.3, 0.6, 0.9, 1.0, 0.1, 1.0 / 3.0, 2.0 ** -20], dtype=np.float32)   # {0} u [2^-20, 1]
LAYOUTS = ("f32", "f32_pad", "bf16_pad", "bf16_off1")


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def exact_in(x, layout):
    """fp32 array -> the fp32 array of the values the layout's dtype holds (bf16: round to nearest even; a NaN keeps its sign)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if layout.startswith("f32"):
        return x
    r = torch.from_numpy(x).to(torch.bfloat16).float().numpy().copy()
    nan = np.isnan(x)
    r.view(np.uint32)[nan] = x.view(np.uint32)[nan] & np.uint32(0xffff0000)
    assert np.isnan(r[nan]).all()
    return r


def on_device(x, layout):
    """x fp32 [B, Cc], exact in the layout's dtype -> the [B, Cc] view the kernel gets.  Every element of the buffer outside the
    view holds +inf or NaN: read as a column, either would outrank the row.
      f32        contiguous                                   f32_pad    ld = Cc + 3 (rows off 16 bytes)
      bf16_pad   [:, :Cc] of a Cc + 14 wide buffer ([:, :498] of 512: ops.vocab_linear)
      bf16_off1  [:, 1:Cc + 1] of it (a base pointer off 4 bytes: the scalar head and tail paths)"""
    B, Cc = x.shape
    dtype = torch.float32 if layout.startswith("f32") else torch.bfloat16
    ld = {"f32": Cc, "f32_pad": Cc + 3, "bf16_pad": Cc + 14, "bf16_off1": Cc + 14}[layout]
    off = 1 if layout == "bf16_off1" else 0
    buf = torch.full((B, ld), float("inf"), dtype=dtype, device=DEV)
    buf[:, 1::2] = float("nan")
    if dtype == torch.float32:
        body = torch.from_numpy(np.ascontiguousarray(x))
    else:
        hi = (np.ascontiguousarray(x).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
        body = torch.from_numpy(hi.copy()).view(torch.bfloat16)
        assert np.array_equal(body.float().numpy().view(np.uint32), x.view(np.uint32))
    buf[:, off:off + Cc] = body.to(DEV)
    v = buf[:, off:off + Cc]
    assert v.stride(0) == ld and v.data_ptr() == buf.data_ptr() + off * buf.element_size()
    return v


def make_batch(B, Cc, layout, rng, call):
    x = (rng.standard_normal((B, Cc)) * 2.0).astype(np.float32)
    sp = M.special_rows(Cc, rng)
    for i in range(min(B, len(sp))):
        x[i] = sp[(i + call * B) % len(sp)]
    x = exact_in(x, layout)
    t = rng.choice(SOFT, size=(B, Cc)).astype(np.float32)
    types = rng.integers(0, 3, size=B).astype(np.int32)     # 0 closed, 1 open, 2: "all" only
    return x, t, types


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. m3ae_vqa_eval against the model, exactly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Cc", [1, 7, 498, 4099])
@pytest.mark.parametrize("B", [1, 3, 37, 300])
def test_vqa_eval_matches_the_model_exactly(B, Cc, layout):
    """Three successive calls into one record per (k, types) combination (at most 900 rows: inside the exactness condition), k in
    {0, 1, 5, 16} clipped to C, types None and a 0 / 1 / 2 mix.  The special rows of the host test lead every batch; at C = 4099 the
    bf16 layouts hold many naturally equal values."""
    rng = np.random.default_rng(B * 100003 + Cc * 17 + LAYOUTS.index(layout))
    batches = []
    for call in range(3):
        x, t, types = make_batch(B, Cc, layout, rng, call)
        batches.append((x, t, types, M.topk(x, min(16, Cc)), on_device(x, layout), torch.from_numpy(t).to(DEV), torch.from_numpy(types).to(DEV)))
    if layout.startswith("bf16") and Cc == 4099:
        assert len(np.unique(batches[0][0][-1])) < Cc - 1000     # natural ties: bf16 has fewer values in range than the row has columns
    for k in sorted({min(k, Cc) for k in (0, 1, 5, 16)}):
        for typed in (False, True):
            rec = ops.vqa_record(DEV)
            want_rec = np.zeros(M.REC)
            for x, t, types, ranks, xd, td, tyd in batches:
                want = M.evaluate(x, t, types if typed else None, k, ranks=ranks)
                got = ops.vqa_eval(xd, td, tyd if typed else None, rec, k=k, want_rows=True)
                want_rec += want["rec"]
                assert np.array_equal(got.pred.cpu().numpy(), want["pred"])
                if k:
                    assert np.array_equal(got.topk_idx.cpu().numpy(), want["topk"])
                else:
                    assert got.topk_idx is None and got.topk_prob is None
                assert np.array_equal(got.hit1.cpu().numpy().view(np.uint32), want["hit1"].view(np.uint32))
            assert np.array_equal(rec.cpu().numpy().view(np.uint64), want_rec.view(np.uint64)), (k, typed, rec.cpu().numpy(), want_rec)
            assert want_rec[9] == 3.0 and want_rec[0] == 3 * B


def test_vqa_eval_without_targets_and_without_rows():
    rng = np.random.default_rng(5)
    x, t, types = make_batch(37, 498, "bf16_pad", rng, 0)
    xd, td = on_device(x, "bf16_pad"), torch.from_numpy(t).to(DEV)
    got = ops.vqa_eval(xd, None, None, None, k=5, want_rows=True)
    want = M.evaluate(x, None, None, 5)
    assert got.hit1 is None and np.array_equal(got.pred.cpu().numpy(), want["pred"]) and np.array_equal(got.topk_idx.cpu().numpy(), want["topk"])
    rec = ops.vqa_record(DEV)
    assert ops.vqa_eval(xd, td, None, rec, k=5) is None                       # the record alone
    assert np.array_equal(rec.cpu().numpy(), M.evaluate(x, t, None, 5)["rec"])
    with pytest.raises(_lib.M3AEHipError):
        ops.vqa_eval(xd.cpu(), None, None, None, k=1)
    with pytest.raises(ValueError):
        ops.vqa_eval(xd, None, None, None, k=17)
    with pytest.raises(ValueError):
        ops.vqa_eval(xd, None, None, rec, k=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the probabilities
# ---------------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
FLOOR = 2.0 ** -126


def prob_bound(ref):
    """|topk_prob - sigmoid in float64| for an fp32 logit x (the widening of a bf16 logit is exact), from the kernel's three fp32
    operations s = 1 / (1 + expf(-x)) -- the negation is exact:
      expf   1 ulp of the ROCm device library = 2 U relative on e = exp(-x), the figure tests/gemm_accuracy.py::_eval_act states for the
             exponential of this form ("v_exp2 2 U"); it moves s by e / (1 + e) = (1 - s) of that:   2 U (1 - s) relative
      add    one rounding of 1 + e:                                                                  U relative
      divide one rounding (correctly rounded fp32 division):                                         U relative
    so |got - s| <= (2 (1 - s) + 2) U s <= 4 U s while the result is a normal number.  Below the normal range -- s < 2^-126, which
    includes every x whose expf(-x) overflows to inf (x < -88.73, s < 2^-128, result 0) -- the result may lose bits or be flushed:
    an absolute 2^-126, the fp32 denormal floor, covers it.  Above, expf(-x) underflowing only makes 1 + e = 1 exactly as it
    rounds anyway.  Nothing here is a multiple of an observed error."""
    return 4 * U * ref + FLOOR


@pytest.mark.parametrize("layout", ["f32", "bf16_off1"])
def test_topk_prob_against_float64_sigmoid(layout):
    rng = np.random.default_rng(11)
    Cc = 16
    x = (rng.standard_normal((64, Cc)) * 8.0).astype(np.float32)
    x[0] = [-120, -100, -89, -88.5, -87.5, -30, 0.0, -0.0, 30, 88.5, 100, np.inf, -np.inf, 1e-30, -1e-30, 17.0]
    x[1, 3] = np.nan
    x = exact_in(x, layout)
    got = ops.vqa_eval(on_device(x, layout), None, None, None, k=Cc, want_rows=True)
    idx, prob = got.topk_idx.cpu().numpy().astype(np.int64), got.topk_prob.cpu().numpy().astype(np.float64)
    assert np.array_equal(idx, M.topk(x, Cc))
    ref = M.sigmoid64(np.take_along_axis(x, idx, 1))
    nan = np.isnan(ref)
    assert nan.sum() == 1 and np.array_equal(np.isnan(prob), nan)
    err, bound = np.abs(prob - ref)[~nan], prob_bound(ref)[~nan]
    print(f"topk_prob {layout}: max err / bound = {np.max(err / bound):.3f}, max rel err = {np.max(err[ref[~nan] > 1e-30] / ref[~nan][ref[~nan] > 1e-30]) / U:.2f} U")
    assert (err <= bound).all()
    assert ((prob[~nan] >= 0) & (prob[~nan] <= 1)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. rejections: the code, and nothing written
# ---------------------------------------------------------------------------------------------------------------------------------
def test_rejections_return_unsupported_and_leave_everything_untouched():
    L = _lib.lib()
    B, Cc, k = 4, 7, 3
    x = torch.randn(B, Cc, device=DEV)
    xb = x.to(torch.bfloat16)
    t = torch.rand(B, Cc, device=DEV)
    outs = dict(pred=torch.full((B,), -7, dtype=torch.int64, device=DEV), idx=torch.full((B, 16), -7, dtype=torch.int32, device=DEV),
                prob=torch.full((B, 16), -7.0, device=DEV), hit1=torch.full((B,), -7.0, device=DEV),
                rec=torch.full((10,), -7.0, dtype=torch.float64, device=DEV), ws=torch.full((B, 2), -7.0, device=DEV),
                match=torch.full((B,), -7, dtype=torch.int32, device=DEV))
    before = {n: v.clone() for n, v in outs.items()}
    need = L.m3ae_vqa_eval_workspace_bytes(B, k)
    assert need == B * 8 and L.m3ae_vqa_eval_workspace_bytes(B, 17) == 0 and L.m3ae_vqa_eval_workspace_bytes(0, 1) == 0

    def call(logits=x, ld=Cc, ldt=Cc, Cc_=Cc, k_=k, dtype=_lib.F32, ws_bytes=need):
        return L.m3ae_vqa_eval(vp(logits), ld, vp(t), ldt, None, B, Cc_, k_, dtype, vp(outs["pred"]), vp(outs["idx"]), vp(outs["prob"]),
                               vp(outs["hit1"]), vp(outs["rec"]), vp(outs["ws"]), ws_bytes, stream())
    UNSUPPORTED = -2
    assert call(k_=17) == UNSUPPORTED                      # k > 16
    assert call(k_=Cc + 1) == UNSUPPORTED                  # k > C
    assert call(Cc_=2 ** 31, ld=2 ** 31, ldt=2 ** 31) == UNSUPPORTED   # C >= 2^31 (refused on the host: nothing is launched)
    assert call(dtype=2) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(ld=Cc - 1) == UNSUPPORTED                  # ld < C
    assert call(logits=xb, dtype=_lib.BF16, ld=Cc - 1) == UNSUPPORTED
    assert call(ldt=Cc - 1) == UNSUPPORTED
    assert call(ws_bytes=need - 1) == UNSUPPORTED          # a short workspace
    assert call(ws_bytes=0) == UNSUPPORTED
    gen = torch.zeros((B, 5), dtype=torch.int64, device=DEV)
    skip = torch.zeros((9,), dtype=torch.int64, device=DEV)

    def match(ns=2, ldg=5, ws_bytes=need):
        return L.m3ae_seq_match(vp(gen), ldg, 5, vp(gen), 5, 5, vp(skip), ns, None, B, vp(outs["match"]), vp(outs["rec"]), vp(outs["ws"]),
                                ws_bytes, stream())
    assert match(ns=9) == UNSUPPORTED and match(ldg=4) == UNSUPPORTED and match(ws_bytes=need - 1) == UNSUPPORTED
    torch.cuda.synchronize()
    for n, v in outs.items():
        assert torch.equal(v, before[n]), n
    assert call() == 0 and match() == 0                     # the same calls with nothing wrong run
    torch.cuda.synchronize()
    assert outs["rec"][9].item() == -5.0 and (outs["pred"] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. m3ae_seq_match against the model
# ---------------------------------------------------------------------------------------------------------------------------------
def seq_case(B, Lg, Lr, skip, rng):
    """Rows of every kind: equal after skipping but different before (skip ids interleaved differently), a one-token difference
    at the last position, all skip ids on both sides / on one side, one side a prefix of the other, identical rows."""
    fill = list(skip) if len(skip) else [0]
    n_max = min(Lg, Lr)

    def spread(core, L, at_end=False):
        """core in order inside a row of length L, the other positions drawn from `fill`."""
        row = [int(rng.choice(fill)) for _ in range(L)]
        pos = list(range(L - len(core), L)) if at_end else sorted(rng.choice(L, size=len(core), replace=False).tolist())
        for p, tok in zip(pos, core):
            row[p] = tok
        return row
    gen, ref = [], []
    for r in range(B):
        kind = r % 7
        n = int(rng.integers(1, n_max + 1))
        core = rng.integers(1000, 1200, size=n).tolist()
        if kind == 0:
            g, f = spread(core, Lg), spread(core, Lr)
        elif kind == 1:
            other = core[:-1] + [core[-1] + 1]
            g, f = spread(core, Lg, at_end=True), spread(other, Lr, at_end=True)
        elif kind == 2:
            g, f = spread([], Lg), spread([], Lr)
        elif kind == 3:
            g, f = spread([], Lg), spread(core, Lr)
        elif kind == 4:
            g, f = spread(core, Lg), spread([], Lr)
        elif kind == 5:
            g, f = spread(core[:-1], Lg), spread(core, Lr)
        else:
            g = spread(core, Lg)
            f = (g + [fill[0]] * Lr)[:Lr] if Lr >= Lg else spread(core, Lr)
        gen.append(g)
        ref.append(f)
    return np.array(gen, dtype=np.int64), np.array(ref, dtype=np.int64)


@pytest.mark.parametrize("B,Lg,Lr,ns", [(1, 9, 6, 8), (300, 9, 6, 8), (300, 6, 9, 3), (300, 7, 7, 0), (300, 9, 6, 0), (1, 7, 7, 0)])
def test_seq_match_matches_the_model(B, Lg, Lr, ns):
    rng = np.random.default_rng(B + 10 * Lg + 100 * ns)
    skip = [0, 101, 102, 1, 2, 3, 50, 999][:ns]
    met = metrics.TokenExactMatch(skip, DEV)
    assert met.skip.tolist() == sorted(skip)
    want_rec = np.zeros(M.REC)
    for call in range(2):
        gen, ref = seq_case(B, Lg, Lr, skip, rng)
        types = rng.integers(0, 3, size=B).astype(np.int32)
        want = M.seq_match(gen, ref, skip)
        if B == 300 and (ns or Lg == Lr):
            assert 0 < want.sum() < B
        got = met.update(torch.from_numpy(gen).to(DEV), torch.from_numpy(ref).to(DEV), torch.from_numpy(types), want_rows=True)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
        want_rec += M.match_record(want, types)
    assert np.array_equal(met.rec.cpu().numpy().view(np.uint64), want_rec.view(np.uint64))
    assert met.result() == M.result(want_rec) and met.compute() == M.result(want_rec)["score"]
    met.reset()
    assert met.result()["n"] == 0 and met.get_best_score() == M.result(want_rec)["score"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the model and the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp32x3": torch.float32}


def to_dev(b):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and v
                and isinstance(v[0], torch.Tensor) else v) for k, v in b.items()}


def cls_model(mode, **over):
    from m3ae_amd.modules import M3AETransformerSS
    m = M3AETransformerSS(tiny_config(compute_dtype=mode, **over))
    synth.fill_deterministic(m)
    m.finalize(DEV, DTYPES[mode])
    return m


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_predict_labels_are_cpu_argmax_and_topk_of_the_returned_logits(mode):
    m = cls_model(mode)
    b = to_dev(tiny_batch())
    k = 5
    for training in (True, False):
        m.train(training)
        out = m.predict(b, k=k)
        assert m.training is training                          # the flag is as predict found it
    assert out["labels"].dtype == torch.int64 and out["probs"].dtype == torch.float32 and out["labels"].is_cuda
    logits = out["logits"].float().cpu()
    assert tuple(logits.shape) == (2, 498) and tuple(out["labels"].shape) == tuple(out["probs"].shape) == (2, k)
    labels = out["labels"].cpu()
    assert torch.equal(labels[:, 0], torch.argmax(logits, dim=1)) and torch.equal(labels[:, 0], torch.max(logits, 1)[1])
    assert np.array_equal(labels.numpy(), M.topk(logits.numpy(), k))
    top = torch.topk(logits, k + 1, dim=1)
    for r in range(2):
        if len(set(top.values[r].tolist())) == k + 1:           # tie-free among the leaders: torch.topk's order is defined
            assert torch.equal(labels[r], top.indices[r, :k])
    ref = M.sigmoid64(np.take_along_axis(logits.numpy(), labels.numpy(), 1))
    assert (np.abs(out["probs"].cpu().numpy().astype(np.float64) - ref) <= prob_bound(ref)).all()
    with pytest.raises(ValueError):
        m.predict(b, k=0)


def test_answers_maps_labels_and_takes_a_dedup_batch():
    m = cls_model("bf16")
    b = to_dev(tiny_batch())
    label2ans = {str(i): f"answer {i}" for i in range(498)}
    dedup = dict(b)
    dedup["image"] = [b["image"][0][:1].contiguous()]
    dedup["image_index"] = torch.zeros(2, dtype=torch.int64, device=DEV)     # both questions ask about image 0
    for batch in (b, dedup):
        out = m.predict(batch, k=3)
        ans = m.answers(batch, label2ans, k=3)
        assert len(ans) == 2 and all(len(row) == 3 for row in ans)
        for row, ls, ps in zip(ans, out["labels"].cpu().tolist(), out["probs"].cpu().tolist()):
            assert row == [(f"answer {l}", p) for l, p in zip(ls, ps)]
    first = m.predict(dedup, k=1)["labels"][0, 0].item()
    with pytest.raises(KeyError, match=f"label {first} "):
        m.answers(dedup, {k_: v for k_, v in label2ans.items() if k_ != str(first)}, k=1)


def cls_trainer(tmp_path, **over):
    cfg = tiny_config(compute_dtype="bf16", per_gpu_batchsize=4, batch_size=4, max_steps=1, log_dir=str(tmp_path), **over)
    dev = torch.device("cuda", torch.cuda.current_device())
    model = trainer.build_model(cfg, "cls", dev)
    dm = trainer.SyntheticDataModule(cfg, 0, 1, dev, pool=1, train_samples=8, val_samples=8)
    rng = np.random.default_rng(3)
    for b in dm.val_pool:                                      # dense soft targets, so that random weights still score
        b["vqa_targets"] = torch.from_numpy(rng.choice(SOFT, size=(4, cfg["vqa_label_size"])).astype(np.float32)).to(dev)
    return trainer.Trainer(cfg, model, dm, 0, 1, dev), model, dm


class Counting:
    """The library with the calls of the new entry points counted (as test_default_search_calls_no_greedy_entry_point)."""

    def __init__(self, L, counts):
        self.L, self.counts = L, counts

    def __getattr__(self, name):
        if name.startswith("m3ae_vqa_") or name.startswith("m3ae_seq_"):
            self.counts[name] = self.counts.get(name, 0) + 1
        return getattr(self.L, name)


def blocking_calls(monkeypatch, fn):
    """The blocking host calls of fn(): Tensor.cpu / item / tolist / __bool__ on device tensors and torch.cuda.synchronize."""
    calls = []
    for name in ("cpu", "item", "tolist", "__bool__"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _r=real, _n=name, **k: (calls.append(_n) if self.is_cuda else None, _r(self, *a, **k))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
    try:
        out = fn()
    finally:
        monkeypatch.undo()
    return out, calls


def test_validate_device_equals_host_and_reports_closed_and_open(tmp_path, monkeypatch):
    host, _, _ = cls_trainer(tmp_path / "host")
    devt, model, dm = cls_trainer(tmp_path / "dev", vqa_metrics="device", eval_topk=5)
    assert host.vqa_metrics == "host" and devt.vqa_metrics == "device"
    counts = {}
    monkeypatch.setattr(_lib, "_lib", Counting(_lib.lib(), counts))
    h = host.validate()
    assert counts == {} and host.metrics is None               # the default key calls no new entry point
    d = devt.validate()
    nb = len(list(dm.val_batches()))
    assert nb == 2 and counts == {"m3ae_vqa_eval": nb}, counts
    monkeypatch.undo()
    assert isinstance(d, float) and abs(h - d) <= 2.0 ** -24 * abs(d)      # host divides fp32 sums, device divides doubles
    # closed / open / @k from numpy over the per-row predictions
    want_rec = np.zeros(M.REC)
    model.eval()
    with torch.no_grad():
        for b in dm.val_batches():
            model.set_task()
            ret = model(b, test=True)
            want_rec += M.evaluate(ret["vqa_logits"].float().cpu().numpy(), ret["vqa_targets"].cpu().numpy(), b["answer_types"], 5)["rec"]
    model.train()
    want = M.result(want_rec)
    assert devt.metrics == want and d == want["score"] and want["n"] == 8 and want["n_closed"] + want["n_open"] == 8
    assert want["score"] > 0 and want["score_at_k"] >= want["score"]
    assert " closed " in devt.metrics_text() and host.metrics_text() == ""
    ck = torch.load(devt.save("m.ckpt", d), map_location="cpu", weights_only=False)
    assert ck["val/the_metric"] == d and ck["val/closed_score"] == want["closed"] and ck["val/open_score"] == want["open"]
    assert "val/closed_score" not in torch.load(host.save("m.ckpt", h), map_location="cpu", weights_only=False)
    # the device form blocks no more often than the host form: the forward passes as they are, then ONE copy of the record
    _, calls_host = blocking_calls(monkeypatch, host.validate)
    _, calls_dev = blocking_calls(monkeypatch, devt.validate)
    assert len(calls_dev) <= len(calls_host) and calls_dev[-1:] == ["cpu"] and calls_host[-1:] == ["item"], (calls_host, calls_dev)


def test_update_never_waits_for_the_device(monkeypatch):
    """Guard in use: torch.cuda.set_sync_debug_mode("error") where `.item()` under it raises on this torch / ROCm pair (checked
    first); otherwise blocking calls are counted (as test_search_path_async_never_waits_for_the_device)."""
    rng = np.random.default_rng(9)
    x, t, types = make_batch(37, 498, "bf16_pad", rng, 0)
    xd, td = on_device(x, "bf16_pad"), torch.from_numpy(t).to(DEV)
    met = metrics.VQARADScore(DEV, k=5)
    met.update(xd, td, types.tolist())                         # warm
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            live = False
        except RuntimeError:
            live = True
        if live:
            met.update(xd, td, types.tolist())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not live:
        _, calls = blocking_calls(monkeypatch, lambda: met.update(xd, td, types.tolist()))
        assert calls == [], calls
    print("sync guard:", "set_sync_debug_mode" if live else "call counting")
    one = M.evaluate(x, t, types, 5)["rec"]
    assert np.array_equal(met.rec.cpu().numpy(), 2 * one)
    assert met.result() == M.result(2 * one) and met.get_best_close_score() == M.result(one)["closed"]
    assert met.get_best_open_score() == M.result(one)["open"] and met.compute() == met.get_best_score()


class ListDM:
    train_samples = 8

    def __init__(self, batches):
        self.batches = batches

    def val_batches(self):
        return iter(self.batches)

    def train_batches(self, epoch):
        return iter(self.batches)


def test_trainer_test_reports_token_exact_match_for_the_decoder_head(tmp_path):
    from m3ae_amd.modules import DecoderModel
    cfg = tiny_config(compute_dtype="fp32", image_size=64, hidden_size=768, num_heads=12, num_top_layer=1, input_image_embed_size=128,
                      input_text_embed_size=128, vocab_size=1000, vit_width=128, vit_layers=2, text_hidden=128, text_layers=1,
                      text_heads=2, text_inter=512, mm_encoder_inputs_include_cls_feats=True, mm_encoder_inputs_include_imagetext_feats=False,
                      vqa_metrics="device", per_gpu_batchsize=2, batch_size=2, max_steps=1, log_dir=str(tmp_path))
    m = DecoderModel(cfg, vocab_size=1200)
    synth.fill_deterministic(m)
    m.finalize(DEV, torch.float32)
    m.eval()
    m.decoder.max_len = 8
    b = to_dev(tiny_batch())
    ids = m.generate_async(b).seq.cpu()
    # row 0's reference is what the model generates, row 1's is another answer
    ref = torch.zeros((2, 1 + ids.shape[1]), dtype=torch.int64)
    ref[:, 0] = m.cls_id
    ref[0, 1:] = ids[0]
    ref[1, 1:4] = torch.tensor([1000 if ids[1, 0].item() != 1000 else 1001, 1002, m.sep_id])
    b["decoder_tokens"] = ref.to(DEV)
    b["answer_types"] = [0, 1]
    tr = trainer.Trainer(cfg, m, ListDM([b, b]), 0, 1, torch.device("cuda", torch.cuda.current_device()))
    skip = (m.pad_id, m.cls_id, m.sep_id)
    want_rows = M.seq_match(ids.numpy(), ref.numpy(), skip)
    assert want_rows.tolist() == [1, 0]
    val = tr.validate()
    assert tr.exact_match is None                              # validate() keeps its meaning: the negative loss, no search
    got = tr.test()
    assert abs(got - val) <= 1e-5 * abs(val) and got < 0       # the same negative loss (its reduction is not ordered by default)
    want = M.result(2 * M.match_record(want_rows, [0, 1]))
    assert tr.exact_match == want and want["closed"] == 1.0 and want["open"] == 0.0 and want["n"] == 4


def test_trainer_test_reports_token_exact_match_for_the_t5_head(tmp_path):
    from m3ae_amd.modules import T5VQA_MMEncoderInput
    dims = dict(d_model=512, d_kv=64, d_ff=2048, num_layers=2, num_decoder_layers=2, num_heads=8)
    cfg = tiny_config(compute_dtype="fp32", t5_max_length=8, vqa_metrics="device", per_gpu_batchsize=2, batch_size=2, max_steps=1,
                      log_dir=str(tmp_path))
    m = T5VQA_MMEncoderInput(cfg, t5_vocab=1100, t5_dims=dims)
    m.unfreeze_top_layers(1, 1)
    synth.fill_deterministic(m)
    m.finalize(DEV, torch.float32)
    m.eval()
    b = to_dev(tiny_batch())
    ids = m.generate_async(b).seq.cpu()
    assert tuple(ids.shape) == (2, 8)
    lab = torch.zeros((2, 8), dtype=torch.int64)
    lab[0] = ids[0]
    lab[1, :3] = torch.tensor([5 if ids[1, 1].item() != 5 else 6, 7, 1])
    b["t5_labels"] = lab.to(DEV)
    b["answer_types"] = [1, 0]
    tr = trainer.Trainer(cfg, m, ListDM([b]), 0, 1, torch.device("cuda", torch.cuda.current_device()))
    c = m.t5.config
    want_rows = M.seq_match(ids.numpy(), lab.numpy(), (c.pad_token_id, c.decoder_start_token_id, c.eos_token_id))
    assert want_rows.tolist() == [1, 0]
    got = tr.test()
    want = M.result(M.match_record(want_rows, [1, 0]))
    assert got < 0 and tr.exact_match == want and want["open"] == 1.0 and want["closed"] == 0.0 and want["n"] == 2
