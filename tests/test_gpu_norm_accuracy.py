"""GPU: the LayerNorm / RMSNorm kernels of csrc/norm.hip and the loss kernels of csrc/misc.hip against float64, with the references,
element-wise bounds, sequential-model yardsticks, exact tier and cases of tests/norm_accuracy.py (whose criteria
tests/test_norm_accuracy_host.py proves on the models and the mutants).  Zero violations, no element excluded, every output buffer
(y, dx, dx_drop, dx_lo, mean, rstd, dgamma, dbeta, d_logits, loss) fenced and every fence checked.

Calls go through the C ABI (_lib.lib().m3ae_layernorm_*, m3ae_xent*, m3ae_bce_logits*); test_ops_wrappers_choose_the_same_entry_points
goes through ops.ln_fwd_raw / ops.ln_bwd_raw / ops.layer_norm.  Instantiations reached: DISPATCH_CPL 1, 2, 3, 4, 6, 8 forward and
backward, 16 forward; the row-pair forward NP 2, 3, 4 (even and odd M, one and several sweeps); modes ACT, RMS, dropout, dropout
rows, ordered, mixed.  The worst err / bound and rms(kernel) / rms(sequential model) per kernel form are printed (pytest -s)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_accuracy as ga  # noqa: E402
import norm_accuracy as na  # noqa: E402
from m3ae_amd import _lib, ops  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
UNSUPPORTED, ALIGN = -2, -3
FIGURES = {}
CASE = {c["name"]: c for c in na.CASES}


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(t):
    return None if t is None else t.to(DEV)


def fenced_vec(n, zero=False):
    buf = torch.full((n + 8,), ga.FENCE, dtype=F32, device=DEV)
    if zero:
        buf[:n] = 0
    return buf, buf[:n]


def vec_fence_intact(buf, n, msg):
    assert bool((buf[n:] == ga.FENCE).all()), f"{msg}: written past element {n}"


def fenced_rows(M, D, dtype, offset=0):
    """(buffer, view [M, D]) with `offset` fence elements in front of the view and three fence rows behind it."""
    buf = torch.full((offset + (M + 3) * D,), ga.FENCE, dtype=dtype, device=DEV)
    return buf, buf[offset:offset + M * D].view(M, D)


def rows_fence_intact(buf, M, D, offset, msg):
    assert bool((buf[:offset] == ga.FENCE).all()) and bool((buf[offset + M * D:] == ga.FENCE).all()), f"{msg}: written outside the [{M}, {D}] rows"


def figures(form):
    return FIGURES.setdefault(form, {})


def report(form):
    f = FIGURES.get(form, {})
    print(f"NORM_ACCURACY {form}: " + ", ".join(f"worst {k} {v:.3f}" for k, v in sorted(f.items())))


def row_dtype(case):
    return BF if case["dtype"] == "bf16" else F32


def grad_dtype(case):
    return F32 if case["dtype"] == "f32" else BF


# ------------------------------------------------------------------------------------------------------------------------
# runners
# ------------------------------------------------------------------------------------------------------------------------
def run_fwd(case, inp, pair_off=None, offset=None):
    """dict(y, mean, rstd) of one forward call, every output fenced and the fences checked."""
    M, D = case["M"], case["D"]
    pair_off = case["pair_off"] if pair_off is None else pair_off
    offset = (4 if case["offset8"] else 0) if offset is None else offset   # 4 bf16 elements: 8 bytes
    L = _lib.lib()
    xbuf = torch.zeros(offset + M * D, dtype=row_dtype(case), device=DEV)
    x = xbuf[offset:].view(M, D)
    x.copy_(inp["x"])
    g, b = dev(inp["gamma"]), dev(inp["beta"])
    ybuf, y = fenced_rows(M, D, BF if na.fwd_bf16(case) else F32, offset)
    mbuf, mean = fenced_vec(M)
    rbuf, rstd = fenced_vec(M)
    want_mean = not case["rms"]
    if offset:
        assert x.data_ptr() % 16 == 8 and y.data_ptr() % 16 == 8
    if case["dtype"] == "mixed":
        rc = L.m3ae_layernorm_fwd_mixed(p(x), p(g), p(b), p(y), p(mean), p(rstd), M, D, case["eps"], stream())
    else:
        rc = L.m3ae_layernorm_fwd(p(x), p(g), p(b), p(y), p(mean) if want_mean else None, p(rstd), M, D, case["eps"],
                                  _lib.BF16 if case["dtype"] == "bf16" else _lib.F32, case["act"], int(case["rms"]) | (2 if pair_off else 0),
                                  stream())
    _lib.check(rc, f"LayerNorm forward {case['name']}")
    torch.cuda.synchronize()
    rows_fence_intact(ybuf, M, D, offset, f"{case['name']} y")
    vec_fence_intact(mbuf, M if want_mean else 0, f"{case['name']} mean")
    vec_fence_intact(rbuf, M, f"{case['name']} rstd")
    return dict(y=y, mean=mean, rstd=rstd)


def keep_mask(case, v):
    M, D = case["M"], case["D"]
    if v.get("drop") == "rows":
        base, step = na.DROP_ROWS
        return ops.dropout_keep_mask(base + (M - 1) * step + 1, D, na.DROP_P, na.DROP_SEED)[base::step].contiguous()
    return ops.dropout_keep_mask(M, D, na.DROP_P, na.DROP_SEED)


def run_bwd(case, inp, v, mean, rstd, det=None):
    """dict(dx, dgamma, dbeta[, dx_drop, dx_lo]) of one backward call, every output fenced and the fences checked."""
    M, D = case["M"], case["D"]
    L = _lib.lib()
    det = v.get("det", False) if det is None else det
    dt = _lib.BF16 if case["dtype"] == "bf16" else _lib.F32
    dy, x, g, b = dev(inp["dy"]), dev(inp["x"]), dev(inp["gamma"]), dev(inp["beta"])
    add = dev(inp["dx_add"]) if v.get("dx_add") else None
    tag = f"{case['name']} bwd {na.variant_tag(v)}"
    dxbuf, dx = fenced_rows(M, D, row_dtype(case))
    gbuf, dg = fenced_vec(D, zero=True)
    bbuf, db = fenced_vec(D, zero=True)
    want_db = v.get("dbeta", True)
    ws = torch.empty(2 * L.m3ae_layernorm_bwd_blocks(M) * D, dtype=F32, device=DEV)
    out = dict(dx=dx, dgamma=dg, dbeta=db)
    second = None
    if v.get("drop"):
        second = fenced_rows(M, D, row_dtype(case))
        out["dx_drop"] = second[1]
        args = (p(dy), p(x), p(g), p(b), p(mean), p(rstd), p(dx), p(second[1]), na.DROP_P, na.DROP_SEED, ops._salt(), p(dg),
                p(db) if want_db else None, p(ws), M, D, dt)
        if v["drop"] == "rows":
            rc = L.m3ae_layernorm_bwd_drop_rows(*args, *na.DROP_ROWS, stream())
        else:
            rc = (L.m3ae_layernorm_bwd_drop_det if det else L.m3ae_layernorm_bwd_drop)(*args, stream())
    elif case["dtype"] == "mixed":
        if v.get("lo"):
            second = fenced_rows(M, D, BF)
            out["dx_lo"] = second[1]
        fn = L.m3ae_layernorm_bwd_mixed_det if det else L.m3ae_layernorm_bwd_mixed
        rc = fn(p(dy), p(x), p(g), p(mean), p(rstd), p(dx), p(add), p(second[1]) if second else None, p(dg), p(db) if want_db else None,
                p(ws), M, D, stream())
    else:
        fn = L.m3ae_layernorm_bwd_det if det else L.m3ae_layernorm_bwd
        rc = fn(p(dy), p(x), p(g), p(b), None if case["rms"] else p(mean), p(rstd), p(dx), p(add), p(dg), p(db) if want_db else None, p(ws),
                M, D, dt, case["act"], int(case["rms"]), stream())
    _lib.check(rc, tag)
    torch.cuda.synchronize()
    rows_fence_intact(dxbuf, M, D, 0, tag + " dx")
    if second is not None:
        rows_fence_intact(second[0], M, D, 0, tag + " second output")
    vec_fence_intact(gbuf, D, tag + " dgamma")
    vec_fence_intact(bbuf, D, tag + " dbeta")   # (without dbeta the zeros in front stay zeros: asserted by the caller)
    return out


def form_of(case, part):
    if part == "fwd":
        kind = "pair" if case["route"] == "pair" else "mixed" if case["dtype"] == "mixed" else "row-" + case["dtype"]
        return "fwd " + kind + (" RMS" if case["rms"] else "") + (" ACT" if case["act"] else "")
    v = part
    mode = "dropout rows" if v.get("drop") == "rows" else "dropout" if v.get("drop") else "mixed" if case["dtype"] == "mixed" else case["dtype"]
    return "bwd " + mode + (" RMS" if case["rms"] else "") + (" ACT" if case["act"] else "") + (" ordered" if v.get("det") else "")


# ------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------
def test_the_large_shape_is_past_one_sweep_of_either_grid():
    assert na.BIG_M > 8 * 256 * 4 == na.SWEEP_FWD and na.BIG_M > 4096 == na.SWEEP_BWD and na.BIG_M % 2 == 1
    assert _lib.lib().m3ae_layernorm_bwd_blocks(na.BIG_M) * 4 == na.SWEEP_BWD
    assert torch.cuda.get_device_properties(0).multi_processor_count <= 256


@pytest.mark.parametrize("name", list(CASE), ids=str)
def test_case_against_float64(name):
    case = CASE[name]
    inp = na.case_inputs(case)
    exact = case["inputs"] in ("const", "ties")
    got = run_fwd(case, inp)
    fkw = dict(rms=case["rms"], act=case["act"], out_bf16=na.fwd_bf16(case))
    seq = None if exact else na.model_fwd(inp["x"], inp["gamma"], inp["beta"], case["eps"], order="seq", **fkw)
    form = form_of(case, "fwd")
    misses = na.fwd_misses(case, inp, got, seq, figures(form), DEV)
    assert misses == [], "\n".join(misses)
    if case["route"] is not None:   # which forward kernel ran: the one-row kernel is a fixed function of the row, the pair kernel sums in another order
        one_row = run_fwd(case, inp, pair_off=True, offset=0)
        same = all(torch.equal(got[k], one_row[k]) for k in ("y", "mean", "rstd"))
        assert same == (case["route"] == "row"), f"{name}: expected the {case['route']} kernel"
        assert na.fwd_misses(case, inp, one_row, seq, figures("fwd row-bf16"), DEV) == []
    if case["M"] % 2 == 1 and not exact:   # the last pair's single row, on its own
        last = {k: val[-1:] for k, val in got.items()}
        one = dict(case, M=1)
        inp1 = {k: (val[-1:] if val is not None and val.dim() == 2 else val) for k, val in inp.items()}
        assert na.fwd_misses(one, inp1, last, None, None, DEV) == [], f"{name}: last row"
    report(form)
    mean, rstd = got["mean"], got["rstd"]
    for v in case["bwd"]:
        keep = keep_mask(case, v) if v.get("drop") else None
        out = run_bwd(case, inp, v, mean, rstd)
        kw = dict(out_bf16=na.bwd_bf16(case), **na.bwd_kw(case, inp, v, None if keep is None else keep.cpu()))
        seq_b = na.model_bwd(inp["dy"], inp["x"], inp["gamma"], inp["beta"], mean.cpu(), rstd.cpu(), order="seq", **kw)
        form = form_of(case, v)
        misses = na.bwd_misses(case, inp, v, mean, rstd, out, seq_b, keep, figures(form), DEV)
        assert misses == [], "\n".join(misses)
        if v.get("drop"):
            plain = run_bwd(case, inp, {k: val for k, val in v.items() if k != "drop"}, mean, rstd)
            assert torch.equal(out["dx"], plain["dx"]), f"{name}: dx of the dropout form is not the undropped call's"
            want = out["dx"].double() * keep.double() / (1.0 - na.DROP_P)
            slack = 4 * na.U * want.abs()
            if na.bwd_bf16(case):
                slack = slack + na.hulp(want.abs() * (1 + 2.0 ** -8)) + na.hulp(out["dx"]) / (1.0 - na.DROP_P)
            assert bool(((out["dx_drop"].double() - want).abs() <= slack).all()), f"{name}: dx_drop is not dx keep / (1 - p) to one rounding"
            assert bool((out["dx_drop"][keep == 0] == 0).all())
        if v.get("lo"):
            assert torch.equal(out["dx_lo"], out["dx"].to(BF))
        if v.get("det"):
            again = run_bwd(case, inp, v, mean, rstd)
            for k in out:
                assert torch.equal(out[k], again[k]), f"{name}: ordered form, {k} differs between two runs"
        if not v.get("dbeta", True):
            assert bool((out["dbeta"] == 0).all())
        report(form)


OPS_CASES = ("sweep-f32-37x768", "sweep-bf16-37x768", "rms-f32-37x768", "rms-bf16-37x512", "gelu-f32-37x260", "gelu-bf16-37x1536",
             "drop-bf16-37x516", "drop-f32-37x516", f"mixed-{na.MID_M}x768", "pair-1025x768")


@pytest.mark.parametrize("name", OPS_CASES, ids=str)
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "ordered"])
def test_ops_wrappers_choose_the_same_entry_points(name, det):
    """ops.ln_fwd_raw / ops.ln_bwd_raw (the one place that picks an entry point) give the bits of the direct call, and their gradients
    meet the same criteria; ops.layer_norm's autograd path gives the same dx."""
    case = CASE[name]
    inp = na.case_inputs(case)
    x, dy = dev(inp["x"]), dev(inp["dy"])
    gamma = torch.nn.Parameter(dev(inp["gamma"]))
    beta = torch.nn.Parameter(dev(inp["beta"])) if inp["beta"] is not None else None
    ln = (gamma, beta, case["eps"])
    direct = run_fwd(case, inp)
    out_dtype = BF if case["dtype"] == "mixed" else None
    with ops.deterministic_mode(det):
        y, mean, rstd = ops.ln_fwd_raw(x, ln, case["act"], case["rms"], out_dtype)
        assert torch.equal(y, direct["y"]) and torch.equal(rstd, direct["rstd"]) and (case["rms"] or torch.equal(mean, direct["mean"]))
        for v in case["bwd"]:
            if v.get("drop") == "rows" and det:
                continue   # no ordered form of the row-map call (ops raises; tests/test_gpu_deterministic.py)
            for q in (gamma, beta):
                if q is not None:
                    q.grad = None
            keep = keep_mask(case, v) if v.get("drop") else None
            res = ops.ln_bwd_raw(dy, x, ln, mean, rstd, dx_add=dev(inp["dx_add"]) if v.get("dx_add") else None, act=case["act"], rms=case["rms"],
                                 drop=(na.DROP_P, na.DROP_SEED) if v.get("drop") else None, rows=na.DROP_ROWS if v.get("drop") == "rows" else None,
                                 want_lo=bool(v.get("lo")), train=True)
            dx, second = res if isinstance(res, tuple) else (res, None)
            got = dict(dx=dx, dgamma=gamma.grad, dbeta=beta.grad if beta is not None else None, dx_drop=second, dx_lo=second)
            vv = dict(v, dbeta=beta is not None and v.get("dbeta", True))
            want = run_bwd(case, inp, v, direct["mean"], direct["rstd"], det=det)
            assert torch.equal(dx, want["dx"])
            if second is not None:
                assert torch.equal(second, want["dx_drop" if v.get("drop") else "dx_lo"])
            assert na.bwd_misses(case, inp, vv, direct["mean"], direct["rstd"], got, None, keep, None, DEV) == []
    if not case["bwd"] or case["bwd"][0] != {}:
        return
    xx = x.clone().requires_grad_(True)
    ops.layer_norm(xx, gamma, beta, case["eps"], act=case["act"], rms=case["rms"]).backward(dy)
    assert torch.equal(xx.grad, run_bwd(case, inp, {}, direct["mean"], direct["rstd"])["dx"])


# ------------------------------------------------------------------------------------------------------------------------
# refusals: no launch, outputs untouched
# ------------------------------------------------------------------------------------------------------------------------
def _call_all(M, D, dt, x, y, g, b, dy, dx, add, second, mean, rstd, dg, db, ws, mixed=None, only=None):
    """Return codes of the LayerNorm entry points (only: those it names) for rows of dtype code dt (mixed: the fp32-stream forms'
    own arguments)."""
    L, s = _lib.lib(), stream()
    calls = {"fwd": lambda: L.m3ae_layernorm_fwd(p(x), p(g), p(b), p(y), p(mean), p(rstd), M, D, 1e-5, dt, 0, 0, s)}
    for n in ("m3ae_layernorm_bwd", "m3ae_layernorm_bwd_det"):
        calls[n] = lambda n=n: getattr(L, n)(p(dy), p(x), p(g), p(b), p(mean), p(rstd), p(dx), p(add), p(dg), p(db), p(ws), M, D, dt, 0, 0, s)
    for n in ("m3ae_layernorm_bwd_drop", "m3ae_layernorm_bwd_drop_det"):
        calls[n] = lambda n=n: getattr(L, n)(p(dy), p(x), p(g), p(b), p(mean), p(rstd), p(dx), p(second), 0.1, 7, None, p(dg), p(db), p(ws),
                                             M, D, dt, s)
    calls["rows"] = lambda: L.m3ae_layernorm_bwd_drop_rows(p(dy), p(x), p(g), p(b), p(mean), p(rstd), p(dx), p(second), 0.1, 7, None, p(dg),
                                                           p(db), p(ws), M, D, dt, 3, 2, s)
    if mixed is not None:
        xf, ybf, dybf, dxf, lo = mixed
        calls["fwd_mixed"] = lambda: L.m3ae_layernorm_fwd_mixed(p(xf), p(g), p(b), p(ybf), p(mean), p(rstd), M, D, 1e-5, s)
        for n in ("m3ae_layernorm_bwd_mixed", "m3ae_layernorm_bwd_mixed_det"):
            calls[n] = lambda n=n: getattr(L, n)(p(dybf), p(xf), p(g), p(mean), p(rstd), p(dxf), None, p(lo), p(dg), p(db), p(ws), M, D, s)
    rc = {k: fn() for k, fn in calls.items() if only is None or only(k)}
    torch.cuda.synchronize()
    return rc


def _buffers(M, D, dtype):
    fence = lambda n, dt=dtype: torch.full((n,), ga.FENCE, dtype=dt, device=DEV)
    return dict(x=fence(M * D + 16), y=fence(M * D + 16), dy=fence(M * D + 16), dx=fence(M * D + 16), add=fence(M * D + 16),
                second=fence(M * D + 16), g=fence(D + 16, F32), b=fence(D + 16, F32), mean=fence(M, F32), rstd=fence(M, F32),
                dg=fence(D, F32), db=fence(D, F32), ws=fence(2 * _lib.lib().m3ae_layernorm_bwd_blocks(M) * D, F32))


def _untouched(bufs):
    return all(bool((t == ga.FENCE).all()) for t in bufs.values())


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_unsupported_widths_are_refused_without_a_launch(dtype):
    dt = _lib.F32 if dtype == F32 else _lib.BF16
    M = 8
    for D in na.REFUSED_D + na.FWD_ONLY_D:
        bufs = _buffers(M, D, dtype)
        mixed = (bufs["x"].float(), bufs["y"].to(BF), bufs["dy"].to(BF), bufs["dx"].float(), bufs["second"].to(BF))
        rc = _call_all(M, D, dt, **{k: bufs[k] for k in ("x", "y", "g", "b", "dy", "dx", "add", "second", "mean", "rstd", "dg", "db", "ws")},
                       mixed=mixed)
        if D in na.FWD_ONLY_D:   # (the forward has a kernel for these; it ran, into y / mean / rstd)
            assert rc.pop("fwd") == 0
            bufs.pop("y"), bufs.pop("mean"), bufs.pop("rstd")
        assert all(r == UNSUPPORTED for r in rc.values()), (D, rc)
        assert _untouched(bufs) and all(bool((t == ga.FENCE).all()) for t in mixed[1:]), D


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_misaligned_pointers_are_refused_without_a_launch(dtype):
    """Rows are loaded 4 elements at a time (16 bytes of fp32, 8 bytes of bf16), gamma / beta 16 bytes at a time: every entry point
    returns M3AE_ERR_ALIGN for a pointer below that, before any launch.  (fp32 rows 8 bytes off are refused too.)"""
    dt = _lib.F32 if dtype == F32 else _lib.BF16
    M, D = 8, 128
    names = ("x", "y", "g", "b", "dy", "dx", "add", "second", "mean", "rstd", "dg", "db", "ws")
    users = {"x": None, "y": ("fwd",), "g": None, "b": None, "dy": "bwd", "dx": "bwd", "add": ("m3ae_layernorm_bwd", "m3ae_layernorm_bwd_det"),
             "second": ("m3ae_layernorm_bwd_drop", "m3ae_layernorm_bwd_drop_det", "rows")}
    shifts = (1, 2) if dtype == F32 else (2,)   # elements: 4 and 8 bytes off for fp32 rows, 4 bytes off for bf16 rows
    for which, used_by in users.items():
        for shift in ((1, 2) if which in ("g", "b") else shifts):
            bufs = _buffers(M, D, dtype)
            args = {k: bufs[k] for k in names}
            args[which] = bufs[which][shift:]
            assert args[which].data_ptr() % (16 if args[which].dtype == F32 else 8) != 0
            rc = _call_all(M, D, dt, **args, only=lambda k: used_by is None or (k != "fwd" if used_by == "bwd" else k in used_by))
            assert rc and all(r == ALIGN for r in rc.values()), (which, shift, rc)
            assert _untouched(bufs), (which, shift)


# ------------------------------------------------------------------------------------------------------------------------
# losses
# ------------------------------------------------------------------------------------------------------------------------
def run_xent(x, lab, ld, det, with_grad=True):
    """(loss, d_logits [rows, C]) of m3ae_xent / m3ae_xent_det on logits at row stride ld whose tail holds POISON; d_logits and loss
    fenced (the tail of d_logits included) and the fences checked."""
    rows, Cc = x.shape
    L = _lib.lib()
    xbuf = torch.full((rows, ld), na.POISON, dtype=x.dtype, device=DEV)
    xbuf[:, :Cc] = x.to(DEV)
    dbuf, d = ga.fenced((rows, Cc), ld, x.dtype, DEV)
    lbuf, loss = fenced_vec(1)
    labd = lab.to(DEV)
    dt = _lib.BF16 if x.dtype == BF else _lib.F32
    if det:
        ws, n = ops._small_ws(_lib.DET_XENT, rows, Cc, torch.device(DEV))
        rc = L.m3ae_xent_det(p(xbuf), p(labd), p(loss), p(dbuf) if with_grad else None, rows, Cc, ld, na.GRAD_SCALE, dt, p(ws), n, stream())
    else:
        ws = torch.empty(4, dtype=F32, device=DEV)
        rc = L.m3ae_xent(p(xbuf), p(labd), p(loss), p(dbuf) if with_grad else None, p(ws), rows, Cc, ld, na.GRAD_SCALE, dt, stream())
    _lib.check(rc, "m3ae_xent")
    torch.cuda.synchronize()
    ga.assert_fence_intact(dbuf, (rows, Cc) if with_grad else (0, 0), f"xent d_logits ({rows}, {Cc}), ld {ld}")
    vec_fence_intact(lbuf, 1, "xent loss")
    return loss[0].item(), d


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "ordered"])
def test_cross_entropy_against_float64(bf16, det):
    fig = figures(f"xent {'bf16' if bf16 else 'f32'}{' ordered' if det else ''}")
    for rows in na.XENT_ROWS:
        for Cc in na.XENT_C:
            for labelled in ("some", "one", "none"):
                x, lab = na.xent_inputs(rows, Cc, bf16, labelled)
                ref_loss, ref_grad, m = na.xent_reference(x, lab, na.GRAD_SCALE)
                e_loss, e_grad = na.xent_bound(ref_grad, m, bf16)
                for ld in (Cc, Cc + na.XENT_PAD):
                    loss, d = run_xent(x, lab, ld, det)
                    tag = f"rows {rows}, C {Cc}, ld {ld}, labelled {labelled}"
                    assert abs(loss - ref_loss.item()) <= e_loss.item(), (tag, loss, ref_loss.item(), e_loss.item())
                    if e_loss.item() > 0:
                        fig["loss err/bound"] = max(fig.get("loss err/bound", 0.0), abs(loss - ref_loss.item()) / e_loss.item())
                    miss = na.check_bound(d, ref_grad.to(DEV), e_grad.to(DEV), "d_logits", fig)
                    assert miss is None, (tag, miss)
                    if labelled == "none":   # what the library defines where torch gives NaN: loss 0, zero gradients, in both forms
                        assert loss == 0.0 and not bool(d.any())
    if det:   # without d_logits: the same loss, and nothing written
        x, lab = na.xent_inputs(48, 257, bf16)
        assert run_xent(x, lab, 257 + na.XENT_PAD, det, with_grad=False)[0] == run_xent(x, lab, 257 + na.XENT_PAD, det)[0]
    report(f"xent {'bf16' if bf16 else 'f32'}{' ordered' if det else ''}")


def test_cross_entropy_with_every_row_ignored_through_ops():
    for det in (False, True):
        with ops.deterministic_mode(det):
            x = torch.randn(6, 50, device=DEV, requires_grad=True)
            loss = ops.cross_entropy(x, torch.full((6,), na.IGNORE, device=DEV))
            loss.backward()
            assert loss.item() == 0.0 and not bool(x.grad.any())


def run_bce(x, z, det):
    B, Cc = x.shape
    L = _lib.lib()
    xd, zd = x.to(DEV), z.to(DEV)
    dbuf, d = ga.fenced((B, Cc), Cc, x.dtype, DEV)
    lbuf, loss = fenced_vec(1)
    dt = _lib.BF16 if x.dtype == BF else _lib.F32
    if det:
        ws, n = ops._small_ws(_lib.DET_BCE, B, Cc, torch.device(DEV))
        rc = L.m3ae_bce_logits_det(p(xd), p(zd), p(loss), p(d), B, Cc, na.GRAD_SCALE, dt, p(ws), n, stream())
    else:
        rc = L.m3ae_bce_logits(p(xd), p(zd), p(loss), p(d), B, Cc, na.GRAD_SCALE, dt, stream())
    _lib.check(rc, "m3ae_bce_logits")
    torch.cuda.synchronize()
    ga.assert_fence_intact(dbuf, (B, Cc), f"bce d_logits ({B}, {Cc})")
    vec_fence_intact(lbuf, 1, "bce loss")
    return loss[0].item(), d


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "ordered"])
def test_bce_with_logits_against_float64(bf16, det):
    form = f"bce {'bf16' if bf16 else 'f32'}{' ordered' if det else ''}"
    fig = figures(form)
    for B, Cc in na.BCE_SHAPES:
        x, z = na.bce_inputs(B, Cc, bf16)
        ref_loss, ref_grad, m = na.bce_reference(x, z, na.GRAD_SCALE)
        e_loss, e_grad = na.bce_bound(ref_loss, ref_grad, m, bf16)
        loss, d = run_bce(x, z, det)
        assert torch.isfinite(d.float()).all() and loss == loss and abs(loss) < float("inf")
        assert abs(loss - ref_loss.item()) <= e_loss.item(), (B, Cc, loss, ref_loss.item(), e_loss.item())
        fig["loss err/bound"] = max(fig.get("loss err/bound", 0.0), abs(loss - ref_loss.item()) / e_loss.item())
        miss = na.check_bound(d, ref_grad.to(DEV), e_grad.to(DEV), "d_logits", fig)
        assert miss is None, (B, Cc, miss)
        sat = (x.float().abs() >= 100.0).to(DEV)
        if bool(sat.any()):   # the saturated sigmoid is exactly 0 or 1: (0 or 1 - z) scale, within the arithmetic's 5 u (and the store)
            zz, xx = z.double().to(DEV), x.double().to(DEV)
            want = ((xx > 0).double() - zz) * m["scale"]
            err = (d.double() - want).abs()[sat]
            assert bool((err <= 5 * na.U * want.abs()[sat]).all()), (B, Cc, (err / want.abs()[sat].clamp_min(1e-300)).max().item() / na.U)
    report(form)
