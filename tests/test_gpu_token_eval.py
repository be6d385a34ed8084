"""GPU: device-side token evaluation (csrc/token_eval.hip) -- m3ae_token_eval against the numpy model of tests/token_eval_model.py:
pred, rank, topk_idx, the counts of the record and err bit for bit; nll and topk_prob against float64 within the model's derived
bound; the fold against the model's replay of the kernel's own rows, bit for bit; the rejections; TokenAccuracy / LossMean;
Trainer.validate with pretrain_metrics="device"; fill_mask."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import token_eval_model as M  # noqa: E402
from vqa_eval_model import special_rows  # noqa: E402
from m3ae_amd import _lib, metrics, ops, trainer  # noqa: E402
from oracle_util import tiny_batch, tiny_config  # noqa: E402

DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device(x, dtype, off=0, ld=None):
    """fp32 array [R, V] -> (the values the dtype holds, as fp32 numpy; the [R, V] device view that starts `off` elements into a
    buffer with row stride ld).  Every element of the buffer outside the view holds +inf or NaN: read as a column, either would
    outrank the row and poison its lse."""
    R, V = x.shape
    ld = V if ld is None else ld
    body = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DT[dtype])
    buf = torch.full((R * ld + off + 8,), float("inf"), dtype=DT[dtype], device=DEV)
    buf[1::2] = float("nan")
    v = buf.as_strided((R, V), (ld, 1), off)
    v.copy_(body.to(DEV))
    assert v.stride(0) == ld and v.data_ptr() == buf.data_ptr() + off * buf.element_size()
    return body.float().numpy(), v


def rows_for(R, V, seed, scale=3.0):
    """Random rows led by the special rows of the ranking rule (ties, all-equal, +-0, +-inf, -inf alone, NaNs of both signs)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, V)) * scale).astype(np.float32)
    sp = special_rows(V, rng)
    n = min(R, len(sp))
    x[:n] = sp[:n]
    return x, rng


def labels_for(x, rng):
    """Labels of every kind the width allows: -100, column 0, V - 1, 63, 64 (clipped), the argmax, random columns."""
    R, V = x.shape
    lab = rng.integers(0, V, size=R).astype(np.int64)
    for r in range(R):
        kind = r % 7
        if kind == 0:
            lab[r] = M.IGNORE
        elif kind in (1, 2, 3, 4):
            lab[r] = min((0, V - 1, 63, 64)[kind - 1], V - 1)
        elif kind == 5:
            lab[r] = M.full_order(x[r])[0]
    return lab


def compare(x, xd, labels, select, k, chunk, itemsize, rec=None):
    """One call with every output; everything the issue holds to bit equality against the model, nll / topk_prob to the bound.
    Returns (rows, model)."""
    R, V = x.shape
    ld_ = None if labels is None else torch.from_numpy(labels).to(DEV)
    sd_ = None if select is None else torch.from_numpy(select).to(DEV)
    rec_before = None if rec is None else rec.cpu().numpy().copy()
    got = ops.token_eval(xd, ld_, sd_, rec, k=k, chunk=chunk, want_rows=True, want_topk=k > 0)
    want = M.evaluate(x, labels, select, k)
    pred, rank, nll = got.pred.cpu().numpy(), got.rank.cpu().numpy(), got.nll.cpu().numpy()
    assert np.array_equal(pred, want["pred"]), (pred, want["pred"])
    assert np.array_equal(rank, want["rank"]), (rank, want["rank"])
    assert rank.dtype == np.int32 and pred.dtype == np.int64 and nll.dtype == np.float32
    if labels is not None:
        assert got.err.item() == want["err"]
    else:
        assert got.err is None
    ev = want["ev"]
    assert (nll[~ev] == 0).all()
    if k:
        idx, prob = got.topk_idx.cpu().numpy(), got.topk_prob.cpu().numpy()
        assert np.array_equal(idx.astype(np.int64), want["topk"])
        assert (prob[~ev] == 0).all()
    worst = 0.0
    for r in np.nonzero(ev)[0]:
        ref = want["nll"][r]
        if not np.isfinite(want["lse"][r]):                      # non-finite rows: torch.logsumexp's value, exactly
            assert np.array_equal(np.float64(nll[r]), ref, equal_nan=True), (r, nll[r], ref)
            if k:
                assert np.array_equal(prob[r].astype(np.float64), want["prob"][r], equal_nan=True), (r, prob[r], want["prob"][r])
            continue
        if want["labelled"][r]:
            NLL, b = M.nll_bound(x[r], int(labels[r]), chunk, itemsize)
        else:
            NLL, b = M.lse_bound(x[r], V, chunk, itemsize)
            b *= M.SLACK
        if np.isfinite(NLL):
            assert abs(np.float64(nll[r]) - NLL) <= b, (r, nll[r], NLL, b)
            worst = max(worst, abs(np.float64(nll[r]) - NLL) / b)
        else:                                                    # the label sits on a -inf column
            assert np.float64(nll[r]) == NLL
        if k:
            P, pb = M.prob_bound(x[r], want["topk"][r], chunk, itemsize)
            assert (np.abs(prob[r].astype(np.float64) - P) <= pb).all(), (r, prob[r], P, pb)
    if rec is not None:
        new = rec.cpu().numpy()
        replay = M.fold(rank, nll, k, rec_before)
        num = ~np.isnan(replay)               # a NaN nll makes the sum a NaN (in both): its payload is not part of the contract
        assert np.array_equal(np.isnan(new), ~num) and np.array_equal(new[num].view(np.uint64), replay[num].view(np.uint64)), (new, replay)
        lab = want["labelled"]
        inc = new[:3] - rec_before[:3]
        assert inc.tolist() == [lab.sum(), (want["rank"][lab] == 0).sum(), (want["rank"][lab] < k).sum()]
        assert new[4] == rec_before[4] + 1
    print(f"V={V} chunk={chunk} k={k}: worst nll error / bound = {worst:.3f}")
    return got, want


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. shapes, layouts, k: everything against the model
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPES = [  # (R, V, chunk, dtype, off, ld)
    (12, 1, 64, "f32", 0, None), (12, 63, 64, "bf16", 0, None), (12, 64, 64, "f32", 0, None), (12, 65, 64, "bf16", 0, None),
    (12, 130, 64, "f32", 0, None), (12, 130, 64, "bf16", 0, 136),            # the last chunk of 130 holds 2 columns
    (12, 1000, 0, "f32", 0, None), (12, 1000, 0, "bf16", 0, 1024),            # a single chunk, the tiny model's width
    (2, 30522, 0, "f32", 0, None), (3, 50265, 0, "bf16", 0, 50304),
    (12, 301, 64, "bf16", 1, 333), (12, 301, 128, "bf16", 3, 333), (12, 301, 64, "f32", 1, 333),   # scalar head and tail paths
]


@pytest.mark.parametrize("R,V,chunk,dtype,off,ld", SHAPES)
def test_token_eval_matches_the_model(R, V, chunk, dtype, off, ld):
    x, rng = rows_for(R, V, R * 1009 + V + off)
    if V > 20000:
        x = (rng.standard_normal((R, V)) * 3.0).astype(np.float32)      # big rows: no special rows, the label kinds still
    x, xd = on_device(x, dtype, off, ld)
    if dtype == "bf16" and V == 50265:
        assert len(np.unique(x[-1])) < V - 1000     # duplicated values: the column tie-break decides the rank
    labels = labels_for(x, rng)
    if dtype == "bf16" and V == 50265:               # a label whose value another column holds too
        vals, inv, cnt = np.unique(x[-1], return_inverse=True, return_counts=True)
        labels[-1] = int(np.nonzero(cnt[inv] > 1)[0][-1])
        labels[0] = int(np.argmax(x[0]))
    itemsize = 4 if dtype == "f32" else 2
    for k in sorted({min(k, V) for k in (0, 1, 5, 16)}):
        rec = ops.token_record(DEV)
        compare(x, xd, labels, None, k, chunk, itemsize, rec)
    compare(x, xd, None, None, min(5, V), chunk, itemsize)                # no labels: every row, rank -1


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. labels and selection
# ---------------------------------------------------------------------------------------------------------------------------------
def test_labels_selection_ties_and_bad_labels():
    V, chunk = 130, 64
    x, rng = rows_for(16, V, 77)
    x[12] = -2.0
    x[12, 5] = x[12, 70] = 3.0                       # the maximum twice, in two chunks
    x[13] = x[12]
    x[14] = x[12]
    x, xd = on_device(x, "f32")
    # every row -100: the record is unchanged except `calls`, and no row output is touched beyond its "skipped" values
    rec = ops.token_record(DEV)
    rec[:4] = torch.tensor([3.0, 2.0, 1.0, 0.5], dtype=torch.float64)
    got, _ = compare(x, xd, np.full(16, M.IGNORE, np.int64), None, 5, chunk, 4, rec)
    assert rec.cpu().tolist() == [3.0, 2.0, 1.0, 0.5, 1.0] and (got.pred == -1).all() and (got.topk_idx == -1).all()
    # label == argmax; a tie with the maximum from the lower column (a hit) and from the higher column (rank 1, no hit)
    labels = labels_for(x, rng)
    labels[12], labels[13], labels[14] = 5, 70, 0
    got, want = compare(x, xd, labels, None, 5, chunk, 4, ops.token_record(DEV))
    assert got.rank[12].item() == 0 and got.rank[13].item() == 1 and got.pred[13].item() == 5 and got.rank[14].item() == 2
    for r in range(16):
        if r % 7 == 5:
            assert got.rank[r].item() == 0
    # labels V, -1 and -101: err, those rows skipped, the others as before
    bad = labels.copy()
    bad[1], bad[2], bad[3] = V, -1, -101
    got_bad, want_bad = compare(x, xd, bad, None, 5, chunk, 4, ops.token_record(DEV))
    assert got_bad.err.item() == 1 and got.err.item() == 0 and (got_bad.pred[1:4] == -1).all()
    keep = np.ones(16, bool)
    keep[1:4] = False
    for a, b in ((got.pred, got_bad.pred), (got.rank, got_bad.rank), (got.nll, got_bad.nll), (got.topk_idx, got_bad.topk_idx)):
        assert torch.equal(a[keep].view(torch.uint8), b[keep].view(torch.uint8))
    # select overrides labels: a selected -100 row runs without a label, an unselected labelled row does not run
    select = np.zeros(16, np.uint8)
    select[[0, 5, 12, 13]] = 1
    got_sel, _ = compare(x, xd, labels, select, 5, chunk, 4, ops.token_record(DEV))
    assert got_sel.pred[0].item() >= 0 and got_sel.rank[0].item() == -1 and got_sel.pred[1].item() == -1
    _, xdb = on_device(x, "f32")
    got_bool = ops.token_eval(xdb, None, torch.from_numpy(select.astype(bool)).to(DEV), None, k=5, want_rows=True)
    assert torch.equal(got_bool.pred, got_sel.pred) and (got_bool.rank == -1).all()


def test_non_finite_rows_give_what_logsumexp_gives():
    """special_rows row 5 holds +inf, row 6 is -inf alone, rows 7 .. 10 hold NaNs, row 0 gets -inf columns here: the nll is torch's
    logsumexp(row) - row[label] on the CPU, NaN for NaN and infinity for infinity."""
    V = 130
    x, rng = rows_for(12, V, 5)
    x[0, 10:40] = -np.inf
    for dtype in ("f32", "bf16"):
        xs, xd = on_device(x, dtype)
        labels = np.full(12, 9, dtype=np.int64)
        got, _ = compare(xs, xd, labels, None, 3, 64, 4 if dtype == "f32" else 2)
        xt = torch.from_numpy(xs).double()
        ref = (torch.logsumexp(xt, 1) - xt[:, 9]).numpy()
        nll = got.nll.cpu().numpy().astype(np.float64)
        bad = ~np.isfinite(ref)
        assert bad.sum() >= 6 and np.array_equal(nll[bad], ref[bad], equal_nan=True)
        assert np.isfinite(nll[0]) and np.isfinite(nll[~bad]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. rejections: the code, and nothing launched or written
# ---------------------------------------------------------------------------------------------------------------------------------
class Counting:
    """The library with the calls of the new entry points counted (as test_default_search_calls_no_greedy_entry_point)."""

    def __init__(self, L, counts):
        self.L, self.counts = L, counts

    def __getattr__(self, name):
        if name in ("m3ae_token_eval", "m3ae_record_add"):
            self.counts[name] = self.counts.get(name, 0) + 1
        return getattr(self.L, name)


def test_bad_k_is_a_value_error_with_no_launch(monkeypatch):
    x = torch.randn(4, 7, device=DEV)
    counts = {}
    monkeypatch.setattr(_lib, "_lib", Counting(_lib.lib(), counts))
    for k in (8, 17, -1):
        with pytest.raises(ValueError):
            ops.token_eval(x, None, None, None, k=k, want_rows=True)
    with pytest.raises(ValueError):
        ops.token_eval(x, None, None, None, k=1, chunk=32)
    with pytest.raises(ValueError):
        ops.token_eval(x, torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.token_eval(x[:, ::2])
    with pytest.raises(TypeError):
        ops.token_eval(x.half())
    with pytest.raises(_lib.M3AEHipError):
        ops.token_eval(x.cpu())
    assert counts == {}
    ops.token_eval(x, None, None, None, k=7)
    assert counts == {"m3ae_token_eval": 1}


def test_rejections_return_their_code_and_leave_everything_untouched():
    L = _lib.lib()
    R, V, k = 4, 70, 3
    x = torch.randn(R, V, device=DEV)
    labels = torch.zeros(R, dtype=torch.int64, device=DEV)
    need = L.m3ae_token_eval_workspace_bytes(R, V, 64, k)
    S = R * 2
    assert need == 8 * S * (2 + k) + 4 * S + 2 * 4 * R and need % 8 == 0
    assert L.m3ae_token_eval_workspace_bytes(R, V, 0, k) == 8 * R * (2 + k) + 8 * ((4 * R + 7) // 8) + 2 * 4 * R
    for bad in ((0, V, 64, k), (R, 0, 64, k), (R, V, 63, k), (R, V, 65537, k), (R, V, 64, 17), (R, V, 64, -1), (R, 2, 64, 3), (R, 2 ** 31, 64, 1)):
        assert L.m3ae_token_eval_workspace_bytes(*bad) == 0, bad
    outs = dict(pred=torch.full((R,), -7, dtype=torch.int64, device=DEV), rank=torch.full((R,), -7, dtype=torch.int32, device=DEV),
                nll=torch.full((R,), -7.0, device=DEV), idx=torch.full((R, 16), -7, dtype=torch.int32, device=DEV),
                prob=torch.full((R, 16), -7.0, device=DEV), rec=torch.full((5,), -7.0, dtype=torch.float64, device=DEV),
                err=torch.full((1,), -7, dtype=torch.int64, device=DEV), ws=torch.full((need // 8,), -7, dtype=torch.int64, device=DEV))
    before = {n: v.clone() for n, v in outs.items()}

    def call(logits=x, ld=V, lab=labels, V_=V, chunk=64, k_=k, dtype=_lib.F32, err=outs["err"], ws=outs["ws"], ws_bytes=need, R_=R):
        return L.m3ae_token_eval(vp(logits), ld, vp(lab), None, R_, V_, chunk, k_, dtype, vp(outs["pred"]), vp(outs["rank"]), vp(outs["nll"]),
                                 vp(outs["idx"]), vp(outs["prob"]), vp(outs["rec"]), vp(err), vp(ws), ws_bytes, stream())
    ARG, UNSUPPORTED = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
    assert call(logits=None) == ARG and call(ws=None) == ARG and call(err=None) == ARG       # labels without err
    assert call(ld=V - 1) == ARG and call(chunk=-1) == ARG and call(k_=-1) == ARG and call(R_=0) == ARG and call(V_=0, ld=0) == ARG
    assert call(k_=17) == UNSUPPORTED and call(V_=2, k_=3) == UNSUPPORTED
    assert call(chunk=63) == UNSUPPORTED and call(chunk=65537) == UNSUPPORTED
    assert call(dtype=2) == UNSUPPORTED and call(dtype=-1) == UNSUPPORTED
    assert call(V_=2 ** 31, ld=2 ** 31) == UNSUPPORTED
    assert call(ws_bytes=need - 1) == UNSUPPORTED and call(ws_bytes=0) == UNSUPPORTED
    assert L.m3ae_record_add(None, vp(outs["rec"]), stream()) == ARG and L.m3ae_record_add(vp(outs["nll"]), None, stream()) == ARG
    torch.cuda.synchronize()
    for n, v in outs.items():
        assert torch.equal(v, before[n]), n
    assert call() == 0                                       # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert outs["rec"][4].item() == -6.0 and (outs["pred"] >= 0).all() and outs["err"].item() == -7


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the fold and the metrics
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_updates_fold_in_the_fixed_order_and_two_runs_give_the_same_bits():
    R, V, k = 700, 130, 5                                    # more rows than the fold has threads
    x, rng = rows_for(R, V, 21, scale=2.0)
    x[:11] = rng.standard_normal((11, V)).astype(np.float32)        # finite rows only: a NaN nll would hide the sum
    x, xd = on_device(x, "bf16", 1, 141)
    labels = rng.integers(0, V, size=R).astype(np.int64)
    labels[rng.random(R) < 0.5] = M.IGNORE
    ld_ = torch.from_numpy(labels).to(DEV)
    runs = []
    for _ in range(2):
        rec = ops.token_record(DEV)
        a = ops.token_eval(xd, ld_, None, rec, k=k, chunk=64, want_rows=True, want_topk=True)
        b = ops.token_eval(xd, ld_, None, rec, k=k, chunk=64, want_rows=True, want_topk=True)
        runs.append([t.cpu().numpy() for t in (a.pred, a.rank, a.nll, a.topk_idx, a.topk_prob, b.nll, rec)])
    for u, v in zip(*runs):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    pred, rank, nll, _, _, nll_b, rec = runs[0]
    want = M.fold(rank, nll_b, k, M.fold(rank, nll, k))
    assert np.array_equal(rec.view(np.uint64), want.view(np.uint64)), (rec, want)
    assert rec[0] == 2 * (labels != M.IGNORE).sum() and rec[4] == 2.0 and np.isfinite(rec[3]) and rec[3] > 0


def test_token_accuracy_and_loss_mean_on_the_device():
    B, S, V = 3, 8, 1000
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((B * S, V)) * 2).astype(np.float32)
    xs, xd = on_device(x, "bf16", 0, 1024)
    labels = rng.integers(0, V, size=B * S).astype(np.int64)
    labels[rng.random(B * S) < 0.7] = M.IGNORE
    labels[1] = int(M.full_order(xs[1])[0])
    logits = xd.as_strided((B, S, V), (S * 1024, 1024, 1))            # the head's [B, S, :V] view
    met = metrics.TokenAccuracy(DEV, k=5)
    assert met.result() == M.result(np.zeros(5))                     # nothing fed: 0.0, never a NaN
    rows = met.update(logits, torch.from_numpy(labels).to(DEV).view(B, S), want_rows=True)
    met.update(logits, torch.from_numpy(labels).to(DEV).view(B, S).float())          # float targets
    rec = M.fold(rows.rank.cpu().numpy(), rows.nll.cpu().numpy(), 5)
    rec = M.fold(rows.rank.cpu().numpy(), rows.nll.cpu().numpy(), 5, rec)
    out = met.result()
    assert out == M.result(rec) and out["n"] == 2 * (labels != M.IGNORE).sum() and out["accuracy"] > 0 and met.compute() == out["accuracy"]
    lt = torch.from_numpy(labels)
    pred = torch.from_numpy(xs).argmax(-1)
    assert out["accuracy"] == float((pred == lt)[lt != -100].sum()) / float((lt != -100).sum())
    ce = torch.nn.functional.cross_entropy(torch.from_numpy(xs).double(), lt, ignore_index=-100).item()
    assert abs(out["nll"] - ce) <= 2.0 ** -24 * (M.path_units(V, 0, 2) + 60) * max(ce, 1.0)
    # LossMean: the fp32 values widened and added in double, in order
    vals = [np.float32(v) for v in (0.1, 2.5, 1e-3, 7.75)]
    lm = metrics.LossMean(DEV)
    for v in vals:
        lm.update(torch.tensor(v, device=DEV))
    lm.update(torch.tensor(3.0, device=DEV, dtype=torch.bfloat16))
    total = 0.0
    for v in vals + [np.float32(3.0)]:
        total += float(v)
    assert lm.rec.cpu().tolist() == [total, 5.0] and lm.result() == {"mean": total / 5.0, "n": 5}


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the trainer and fill_mask
# ---------------------------------------------------------------------------------------------------------------------------------
PRETRAIN = dict(loss_names={"mlm": 1, "mim": 1, "itm": 1, "vqa": 0, "cls": 0, "irtr": 0}, mim_layer=1, mim_decoder_hidden_size=128,
                mim_decoder_num_layers=2, mim_decoder_num_heads=2)


def pretrain_trainer(tmp_path, **over):
    cfg = tiny_config(compute_dtype="bf16", per_gpu_batchsize=4, batch_size=4, max_steps=1, log_dir=str(tmp_path), **PRETRAIN, **over)
    dev = torch.device("cuda", torch.cuda.current_device())
    model = trainer.build_model(cfg, "cls", dev)
    dm = trainer.SyntheticDataModule(cfg, 0, 1, dev, pool=1, train_samples=8, val_samples=8)
    for i, b in enumerate(dm.val_pool):
        b["itm_labels"] = torch.tensor([1.0, 0.0, 0.0, 1.0] if i == 0 else [0.0, 1.0, 1.0, 1.0])     # fixed: both runs see the same pairs
    return trainer.Trainer(cfg, model, dm, 0, 1, dev), model, dm


def test_validate_device_reports_torch_accuracies_and_keeps_the_monitored_value(tmp_path, monkeypatch):
    host, _, _ = pretrain_trainer(tmp_path / "host")
    devt, model, dm = pretrain_trainer(tmp_path / "dev", pretrain_metrics="device", eval_topk=5)
    assert host.pretrain_metrics == "host" and devt.pretrain_metrics == "device"
    counts = {}
    monkeypatch.setattr(_lib, "_lib", Counting(_lib.lib(), counts))
    with ops.deterministic_mode(True):                              # ordered loss reductions: two passes give the same bits
        h = host.validate()
        assert counts == {} and host.pretrain is None and host.metrics_text() == ""     # the default key calls no new entry point
        d = devt.validate()
    nb = len(list(dm.val_batches()))
    assert nb == 2 and counts == {"m3ae_token_eval": 2 * nb, "m3ae_record_add": 3 * nb}, counts
    monkeypatch.undo()
    assert d == h                                                   # the monitored quantity is computed as before
    want = {"mlm": [0, 0, 0], "itm": [0, 0, 0]}
    losses = {"mlm": [], "itm": [], "mim": []}
    weighted = 0.0
    model.eval()
    with torch.no_grad(), ops.deterministic_mode(True):
        for b in dm.val_batches():
            model.set_task()
            ret = model(b, test=True)
            for name in ("mlm", "itm"):
                logits, lab = ret[f"{name}_logits"].float(), ret[f"{name}_labels"].long()
                keep = lab != -100
                want[name][0] += int(keep.sum())
                want[name][1] += int((logits.argmax(-1) == lab)[keep].sum())
                if name == "mlm":
                    for row, l in zip(logits[keep].cpu().numpy(), lab[keep].cpu().tolist()):
                        want[name][2] += int(l in M.full_order(row)[:5])
                    weighted += int(keep.sum()) * ret["mlm_loss"].float().item()
            for name in losses:
                losses[name].append(ret[f"{name}_loss"].float().item())
    model.train()
    r = devt.pretrain
    assert set(r) == {"mlm", "itm", "mlm_loss", "itm_loss", "mim_loss"}
    for name in ("mlm", "itm"):
        n, hit = want[name][:2]
        assert n > 0 and r[name]["n"] == n and r[name]["accuracy"] == hit / n, (name, r[name], want[name])
    assert want["itm"][0] == 8 and r["itm"]["accuracy_at_k"] == 0.0                   # the ITM metric runs with k = 0
    assert r["mlm"]["accuracy_at_k"] == want["mlm"][2] / want["mlm"][0]
    # the mean nll is the MLM loss over the same rows: two fp32 evaluations of one quantity, each within (P + 60) u of it
    ce = weighted / want["mlm"][0]
    assert r["mlm"]["perplexity"] == float(np.exp(r["mlm"]["nll"])) and abs(r["mlm"]["nll"] - ce) <= 2 * 2.0 ** -24 * (M.path_units(1000, 0, 2) + 60) * max(ce, 1.0)
    for name, vals in losses.items():
        assert r[f"{name}_loss"] == sum(np.float64(np.float32(v)) for v in vals) / len(vals), name
    text = devt.metrics_text()
    assert " mlm acc " in text and " @5 " in text and " ppl " in text and " | itm acc " in text and " | mim loss " in text
    ck = torch.load(devt.save("m.ckpt", d), map_location="cpu", weights_only=False)
    assert ck["val/the_metric"] == d and ck["val/mlm_accuracy"] == r["mlm"]["accuracy"] and ck["val/itm_accuracy"] == r["itm"]["accuracy"]
    assert [ck[f"val/{n}_loss"] for n in ("mlm", "itm", "mim")] == [r[f"{n}_loss"] for n in ("mlm", "itm", "mim")]
    assert not any(key.startswith("val/mlm") for key in torch.load(host.save("m.ckpt", h), map_location="cpu", weights_only=False))


def test_fill_mask_returns_the_models_topk_at_the_masked_positions():
    from m3ae_amd.modules import M3AETransformerSS
    from m3ae_amd import synth
    m = M3AETransformerSS(tiny_config(compute_dtype="bf16", **PRETRAIN))
    synth.fill_deterministic(m)
    m.finalize(DEV, torch.bfloat16)
    b = {k_: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and v and isinstance(v[0], torch.Tensor)
              else v) for k_, v in tiny_batch(pretrain=True).items()}
    MASK, k = 999, 5
    ids = b["text_ids"].clone()
    ids[0, 2] = ids[1, 4] = MASK
    assert int((ids == MASK).sum()) == 2
    b["text_ids"] = ids
    for training in (True, False):
        m.train(training)
        out = m.fill_mask(b, k=k, mask_token_id=MASK)
        assert m.training is training                          # the flag is as fill_mask found it
    B, S = ids.shape
    assert out["tokens"].dtype == torch.int64 and tuple(out["tokens"].shape) == (B, S, k) and out["probs"].dtype == torch.float32
    assert out["mask"].dtype == torch.bool and torch.equal(out["mask"], ids == MASK) and out["tokens"].is_cuda
    assert (out["tokens"][~out["mask"]] == -1).all() and (out["probs"][~out["mask"]] == 0).all()
    m.eval()
    with torch.no_grad():
        logits = m.mlm_head(m.infer(b, mask_text=False)["multi_modal_text_feats"]).float().cpu().numpy()
    m.train()
    for (r, s) in ((0, 2), (1, 4)):
        row = logits[r, s]
        want = M.full_order(row)[:k]
        assert np.array_equal(out["tokens"][r, s].cpu().numpy(), want)
        P, pb = M.prob_bound(row, want, 0, 2)
        assert (np.abs(out["probs"][r, s].cpu().numpy().astype(np.float64) - P) <= pb).all()
    with pytest.raises(ValueError):
        m.fill_mask(b, k=0, mask_token_id=MASK)
    with pytest.raises(ValueError, match="mask_token_id"):
        m.fill_mask(b, k=1)                                    # roberta's 50264 is outside the tiny vocabulary
