"""GPU: the streaming kernels of csrc/misc.hip against the exact models and float64 references of tests/misc_accuracy.py (whose
criteria tests/test_misc_accuracy_host.py proves on fp32 models and mutants).  Calls go through the C ABI (_lib.lib().m3ae_*), the
last tests through ops.gather_rows.  Every output buffer is fenced in front and behind and every fence is checked; no element is
excluded from any comparison.  Exact tier: raw bits (a NaN matches a NaN).  Bounded tier: zero violations of the derived bound;
the worst err / bound per kernel form is printed as MISC_ACCURACY <form>: ... (pytest -s)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import misc_accuracy as ma  # noqa: E402
from m3ae_amd import _lib, ops  # noqa: E402

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
UNSUPPORTED = -2
FIGURES = {}
DTYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def code(dtype):
    return _lib.BF16 if dtype == BF else _lib.F32


def ok(rc, what):
    _lib.check(rc, what)
    torch.cuda.synchronize()


KEEP = []   # every device buffer of a test lives until the test ends: a pointer argument must not outlive its tensor


@pytest.fixture(autouse=True)
def _buffers_live_until_the_test_ends():
    yield
    KEEP.clear()


def dev(t):
    KEEP.append(t.to(DEV))
    return KEEP[-1]


def out_buf(shape, dtype, offset=0):
    """(buffer, fenced view of `shape`), the view `offset` elements past a 16-byte boundary."""
    buf, v = ma.fenced_flat(math.prod(shape), dtype, DEV, offset)
    KEEP.append(buf)
    assert v.data_ptr() % 16 == (offset * v.element_size()) % 16
    return buf, v.view(shape)


def filled(t, offset=0):
    """(buffer, fenced view) holding a copy of t: for buffers a kernel updates in place."""
    buf, v = out_buf(tuple(t.shape), t.dtype, offset)
    v.copy_(t)
    return buf, v


def src(t, offset=0):
    """A device copy of t that starts `offset` elements past a 16-byte boundary, FENCE around it."""
    return filled(t, offset)[1]


def intact(buf, view, msg):
    ma.flat_fence_intact(buf, view, msg)


def same(got, want, msg):
    n = ma.bits_differ(got, want.to(got.dtype))
    assert n == 0, f"{msg}: {n} of {got.numel()} elements differ in their bits"


def figures(form):
    return FIGURES.setdefault(form, {})


def report(form):
    print(f"MISC_ACCURACY {form}: " + ", ".join(f"worst {k} {v:.3e}" for k, v in sorted(FIGURES.get(form, {}).items())))


def name_of(dtype):
    return "bf16" if dtype == BF else "f32"


# ------------------------------------------------------------------------------------------------------------------------
# exact tier
# ------------------------------------------------------------------------------------------------------------------------
def test_the_large_sizes_are_past_one_sweep_of_the_capped_grid():
    sweep = 8192 * 256
    assert ma.CAST_SIZES[-1] > sweep and ma.ADD_SIZES[-1] // 8 > sweep and ma.DROP_BIG[0] * ma.DROP_BIG[1] > sweep
    assert ma.ADD_SIZES[0] % 8 == 0 and ma.ADD_SIZES[1] % 8 == 3


@pytest.mark.parametrize("n", ma.CAST_SIZES)
@pytest.mark.parametrize("pair", [(F32, BF), (BF, F32), (F32, F32), (BF, BF)], ids=lambda q: f"{name_of(q[0])}-to-{name_of(q[1])}")
def test_cast_bits(pair, n):
    di, do = pair
    v = ma.cast_values(n)
    x = src(v if di == F32 else v.to(BF))
    want = x.cpu() if do == di else ma.cast_model(x.cpu(), do == BF)
    buf, out = out_buf((n,), do)
    ok(_lib.lib().m3ae_cast(p(x), p(out), n, code(di), code(do), stream()), "m3ae_cast")
    intact(buf, out, f"cast {n}")
    same(out, want, f"cast {name_of(di)} -> {name_of(do)}, n = {n}")
    if do == BF and di == F32 and n >= len(ma.SPECIALS):
        head = out[:len(ma.SPECIALS)].float().cpu()
        assert head[:4].tolist() == [1.0, 1.015625, -1.0, -1.015625] and torch.isinf(head[12]) and torch.isnan(head[16])


@DTYPES
def test_add_bits(dtype):
    L, bf = _lib.lib(), dtype == BF

    def run(a, b, out, n):
        ok(L.m3ae_add(p(a), p(b), p(out), n, code(dtype), stream()), "m3ae_add")

    for n in ma.ADD_SIZES:
        a, b = ma.add_values(n, bf)
        want = ma.add_model(a, b, bf).to(dtype)
        offsets = ((0, 0, 0),) if n > 4096 else ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))
        for oa, ob, oo in offsets:   # one element off a 16-byte boundary: the scalar form by m3ae_add's own alignment test
            da, db = src(a, oa), src(b, ob)
            buf, out = out_buf((n,), dtype, oo)
            run(da, db, out, n)
            intact(buf, out, f"add n {n} offsets {(oa, ob, oo)}")
            same(out, want, f"add {name_of(dtype)} n {n} offsets {(oa, ob, oo)}")
        if n > 4096:
            continue
        buf, da = filled(a)   # out aliasing a (m3ae_decoder.py), then a aliasing b
        run(da, src(b), da, n)
        intact(buf, da, "add in place")
        same(da, want, f"add {name_of(dtype)} n {n}, out = a")
        da = src(a)
        buf, out = out_buf((n,), dtype)
        run(da, da, out, n)
        same(out, ma.add_model(a, a, bf), f"add {name_of(dtype)} n {n}, a = b")


@DTYPES
def test_gather_rows_bits(dtype):
    g = torch.Generator().manual_seed(11)
    for D, R, n_out in ((1, 40, 97), (7, 40, 97), (768, 40, 97), (768, 300, 2800)):
        assert D != 768 or n_out != 2800 or n_out * D > 2 ** 21
        table = torch.randn(R, D, generator=g).to(dtype)
        word = table.view(torch.int16 if dtype == BF else torch.int32)
        word[1, :] = 0x7FC1 if dtype == BF else 0x7FC00001        # NaN with a payload
        word[2, 0::2] = -0x8000 if dtype == BF else -0x80000000   # -0
        word[3, :] = 0x7FA5 if dtype == BF else 0x7FA00005
        idx = torch.randint(0, R, (n_out,), generator=g)
        idx[:8] = torch.tensor([1, 1, 2, 3, 2, 1, R - 1, 0])
        idx[8:8 + R] = torch.arange(R - 1, -1, -1)                # reversed
        buf, out = out_buf((n_out, D), dtype)
        ok(_lib.lib().m3ae_gather_rows(p(src(table)), p(dev(idx)), p(out), n_out, D, code(dtype), stream()), "m3ae_gather_rows")
        intact(buf, out, f"gather D {D}")
        iw = torch.int16 if dtype == BF else torch.int32
        assert torch.equal(out.view(iw).cpu(), word[idx]), f"gather {name_of(dtype)} D {D} n_out {n_out}: not a copy of the bits"


@DTYPES
def test_scatter_add_rows_with_distinct_indices(dtype):
    g = torch.Generator().manual_seed(12)
    for D, R, n_out in ((1, 40, 12), (7, 40, 40), (768, 300, 280)):
        d_in, d_out = torch.randn(R, D, generator=g).to(dtype), torch.randn(n_out, D, generator=g).to(dtype)
        idx = torch.randperm(R, generator=g)[:n_out]
        want = ma.store(d_in.float().index_add(0, idx, d_out.float()), dtype == BF)
        buf, acc = filled(d_in)
        ok(_lib.lib().m3ae_scatter_add_rows(p(src(d_out)), p(dev(idx)), p(acc), n_out, D, code(dtype), stream()), "m3ae_scatter_add_rows")
        intact(buf, acc, f"scatter D {D}")
        same(acc, want, f"scatter_add {name_of(dtype)} D {D}")


@DTYPES
@pytest.mark.parametrize("shape", ma.PATCHIFY_SHAPES, ids=lambda s: f"R{s[0]}-P{s[1]}")
def test_patchify_bits(dtype, shape):
    R, P = shape
    g = torch.Generator().manual_seed(13 + R)
    for B in (1, 3):
        img = torch.randn(B, 3, R, R, generator=g) + 2.0 ** -8 * torch.randint(-3, 4, (B, 3, R, R), generator=g)
        want = ma.store(ma.patchify_reference(img, P), dtype == BF)
        results = []
        for oi, oo in ((0, 0), (1, 0), (0, 1)):   # img / out one element off a 16-byte boundary: the scalar kernel, the same bits
            buf, out = out_buf(tuple(want.shape), dtype, oo)
            ok(_lib.lib().m3ae_patchify(p(src(img, oi)), p(out), B, R, P, code(dtype), stream()), "m3ae_patchify")
            intact(buf, out, f"patchify {shape} B {B} offsets {(oi, oo)}")
            same(out, want, f"patchify {name_of(dtype)} {shape} B {B} offsets {(oi, oo)}")
            results.append(out.clone())
        assert all(torch.equal(results[0], r) for r in results[1:])


@DTYPES
@pytest.mark.parametrize("D", [128, 132])
def test_vit_tokens_fwd_bits(dtype, D):
    g = torch.Generator().manual_seed(14 + D)
    grid = lambda *s: torch.randint(-512, 513, s, generator=g).float() * 2.0 ** -8   # noqa: E731  (sums on bf16 ties)
    for G in (1, 4):
        for B in (1, 3):
            patch, cls, pos = grid(B, G, D).to(dtype), grid(D), grid(G + 1, D)
            want = ma.vit_fwd_model(patch, cls, pos, dtype == BF)
            results = []
            for off in ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)):   # patch, cls, pos, out in turn off by one element
                buf, out = out_buf((B, G + 1, D), dtype, off[3])
                ok(_lib.lib().m3ae_vit_tokens_fwd(p(src(patch, off[0])), p(src(cls, off[1])), p(src(pos, off[2])), p(out), B, G, D, code(dtype),
                                                  stream()), "m3ae_vit_tokens_fwd")
                intact(buf, out, f"vit_tokens_fwd D {D} G {G} B {B} offsets {off}")
                same(out[:, 0], want[:, 0], f"vit_tokens_fwd class row, {name_of(dtype)} D {D} G {G} B {B} offsets {off}")
                same(out[:, 1:], want[:, 1:], f"vit_tokens_fwd patch rows, {name_of(dtype)} D {D} G {G} B {B} offsets {off}")
                results.append(out.clone())
            assert all(torch.equal(results[0], r) for r in results[1:])


@DTYPES
def test_vit_tokens_bwd_bits(dtype):
    g = torch.Generator().manual_seed(15)
    for D in (128, 132):
        for B in (1, 5):
            G = 4
            d_out = torch.randn(B, G + 1, D, generator=g).to(dtype)
            d_cls, d_pos = torch.randn(D, generator=g), torch.randn(G + 1, D, generator=g)
            want_patch, want_cls, want_pos = ma.vit_bwd_model(d_out, d_cls, d_pos)
            pbuf, d_patch = out_buf((B, G, D), dtype)
            cbuf, dc = filled(d_cls)
            qbuf, dp = filled(d_pos)
            ok(_lib.lib().m3ae_vit_tokens_bwd(p(src(d_out)), p(d_patch), p(dc), p(dp), B, G, D, code(dtype), stream()), "m3ae_vit_tokens_bwd")
            for b, v in ((pbuf, d_patch), (cbuf, dc), (qbuf, dp)):
                intact(b, v, f"vit_tokens_bwd D {D} B {B}")
            same(d_patch, want_patch, f"vit_tokens_bwd d_patch {name_of(dtype)} D {D} B {B}")
            same(dp, want_pos, f"vit_tokens_bwd d_pos {name_of(dtype)} D {D} B {B}")
            same(dc, want_cls, f"vit_tokens_bwd d_cls {name_of(dtype)} D {D} B {B}")


@DTYPES
@pytest.mark.parametrize("D", ma.EMBED_FWD_D)
def test_roberta_embed_fwd_bits(dtype, D):
    word, pos, typ = ma.embed_tables(D)
    dw, dp, dt = src(word), src(pos), src(typ)
    for name, (ids, pad) in ma.embed_fwd_cases().items():
        B, S = ids.shape
        want = ma.embed_fwd_model(ids, word, pos, typ, pad, dtype == BF)
        buf, out = out_buf((B, S, D), dtype)
        ok(_lib.lib().m3ae_roberta_embed_fwd(p(dev(ids)), p(dw), p(dp), p(dt), p(out), B, S, D, pad, code(dtype), stream()),
           "m3ae_roberta_embed_fwd")
        intact(buf, out, f"embed fwd {name}")
        same(out, want, f"embed fwd {name_of(dtype)} D {D} {name}")


@DTYPES
@pytest.mark.parametrize("D", ma.EMBED_BWD_D)
def test_roberta_embed_bwd_bits_on_integers(dtype, D):
    L = _lib.lib()
    for name, (ids, pad) in ma.embed_bwd_cases().items():
        B, S = ids.shape
        d_out = ma.small_ints((B, S, D), 50 + D, dtype)
        w0, p0, t0 = ma.small_ints((16, D), 51), ma.small_ints((ma.EMBED_POS_ROWS, D), 52), ma.small_ints((D,), 53)
        want = [t.float() for t in ma.embed_bwd_reference(ids, d_out, w0, p0, t0, pad)]
        dids, dd = ids.to(DEV), src(d_out)
        runs = []
        for det in (False, True, True):
            bufs = [filled(t) for t in (w0, p0, t0)]
            (_, w), (_, q), (_, t) = bufs
            if det:
                ws, n = ops._small_ws(_lib.DET_EMBED_BWD, B * S, D, torch.device(DEV))
                ok(L.m3ae_roberta_embed_bwd_det(p(dids), p(dd), p(w), p(q), p(t), B, S, D, pad, code(dtype), p(ws), n, stream()), "embed bwd det")
            else:
                ok(L.m3ae_roberta_embed_bwd(p(dids), p(dd), p(w), p(q), p(t), B, S, D, pad, code(dtype), stream()), "embed bwd")
            for (b, v), wnt, what in zip(bufs, want, ("d_word", "d_pos", "d_type")):
                intact(b, v, f"embed bwd {name} {what}")
                same(v, wnt, f"embed bwd {name_of(dtype)} D {D} {name} {'ordered' if det else 'atomic'} {what}")
            runs.append([v.clone() for _, v in bufs])
        assert all(torch.equal(a, b) for a, b in zip(runs[1], runs[2])), "ordered form: two calls differ"


@DTYPES
def test_roberta_embed_bwd_det_refuses_wide_rows_without_a_launch(dtype):
    D = ma.EMBED_BWD_REFUSED_D
    ids, pad = ma.embed_bwd_cases()["repeats"]
    B, S = ids.shape
    bufs = [filled(t) for t in (ma.small_ints((16, D), 51), ma.small_ints((ma.EMBED_POS_ROWS, D), 52), ma.small_ints((D,), 53))]
    before = [v.clone() for _, v in bufs]
    ws, n = ops._small_ws(_lib.DET_EMBED_BWD, B * S, D, torch.device(DEV))
    ws.fill_(0xA5)
    rc = _lib.lib().m3ae_roberta_embed_bwd_det(p(dev(ids)), p(src(ma.small_ints((B, S, D), 1, dtype))), p(bufs[0][1]), p(bufs[1][1]), p(bufs[2][1]),
                                               B, S, D, pad, code(dtype), p(ws), n, stream())
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED
    assert all(torch.equal(v, b) for (_, v), b in zip(bufs, before)) and bool((ws == 0xA5).all())


def run_colsum(x, M, N, ldx, dtype, old, det):
    """out [N] of m3ae_colsum / m3ae_colsum_det on x (a pointer to the first element, row stride ldx), fenced and checked."""
    L = _lib.lib()
    buf, out = filled(old) if old is not None else out_buf((N,), F32)
    if det:
        ws, n = ops._small_ws(_lib.DET_COLSUM, M, N, torch.device(DEV))
        ok(L.m3ae_colsum_det(p(x), p(out), M, N, ldx, code(dtype), int(old is not None), p(ws), n, stream()), "m3ae_colsum_det")
    else:
        ok(L.m3ae_colsum(p(x), p(out), M, N, ldx, code(dtype), int(old is not None), stream()), "m3ae_colsum")
    intact(buf, out, f"colsum {M}x{N} ld {ldx}")
    return out


def colsum_layouts(M, N, dtype):
    """name -> (leading dimension, first column inside a wider matrix, element offset of the buffer)."""
    lay = {"contiguous": (N, 0, 0), "column slice": (N + 24, 8, 0), "misaligned column slice": (N + 24, 1, 0)}
    if M >= 4096:   # the whole-row form wants ldx == N: a strided view falls back to the 256-column form
        lay = {"contiguous": (N, 0, 0), "strided view": (N + 8, 0, 0)}
    return lay


@DTYPES
@pytest.mark.parametrize("shape", ma.COLSUM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_colsum_exact_and_bounded(dtype, shape):
    M, N = shape
    bf = dtype == BF
    form = ("rows " if shape in ma.COLSUM_ROWS else "256-column ") + name_of(dtype)
    for kind in ("ints", "mean0", "mean64"):
        x, old = ma.colsum_inputs(M, N, kind, bf)
        seq = ma.colsum_model(x, None, "seq") if kind == "mean64" else None   # (the yardstick holds for terms of one sign)
        xd64 = x.to(DEV)
        for lname, (ld, c0, off) in colsum_layouts(M, N, dtype).items():
            wide = torch.full((M, ld), ma.FENCE, dtype=dtype)
            wide[:, c0:c0 + N] = x
            view = src(wide, off)[:, c0:c0 + N]
            for acc in (False, True):
                for det in (False, True):
                    got = run_colsum(view, M, N, ld, dtype, old if acc else None, det)
                    sq = None if seq is None else (seq if not acc else (ma.np32(old) + seq).astype(np.float32))
                    tag = f"colsum {name_of(dtype)} {M}x{N} {kind} {lname} accumulate {int(acc)} {'ordered' if det else 'atomic'}"
                    misses = ma.colsum_misses(got, xd64, old if acc else None, sq, figures(form + (" ordered" if det else "")), tag,
                                              exact=kind == "ints")
                    assert misses == [], "\n".join(misses)
    report(form)
    report(form + " ordered")


def job_table(jobs, tile):
    """Device int64 [njobs, 5]: {in, out_t, R, C, first_tile}, first_tile the running sum of the tiles of the jobs in front."""
    rows, first = [], 0
    for s, o in jobs:
        R, Cc = s.shape
        rows.append([s.data_ptr(), o.data_ptr(), R, Cc, first])
        first += -(-R // tile) * -(-Cc // tile)
    return torch.tensor(rows, dtype=torch.int64, device=DEV), first


@pytest.mark.parametrize("order", ["table order", "reversed"])
@pytest.mark.parametrize("kind", ["cast_transpose_batched", "transpose_bf16_batched"])
def test_batched_transposes_bits(kind, order):
    bf_src = kind == "transpose_bf16_batched"
    shapes = list(ma.TRANSPOSE_SHAPES) + [(64, 64)]   # the last one from a source one element off: the element-wise path
    if order == "reversed":
        shapes.reverse()
    jobs, bufs, wants = [], [], []
    for i, (R, Cc) in enumerate(shapes):
        s = ma.small_ints((R, Cc), 60 + i).float() * 0.25 + (0.0 if bf_src else 2.0 ** -8 * ma.small_ints((R, Cc), 90 + i, lo=-3, hi=3))
        off = 1 if (R, Cc) == (64, 64) and i in (0, len(shapes) - 1) else 0
        d = src(s.to(BF) if bf_src else s, off)
        buf, o = out_buf((Cc, R), BF)
        jobs.append((d, o)), bufs.append((buf, o)), wants.append(ma.transpose_model(s, 64 if bf_src else 32)[1])
    table, total = job_table(jobs, 64 if bf_src else 32)
    fn = getattr(_lib.lib(), "m3ae_" + kind)
    ok(fn(p(table), len(jobs), total, stream()), kind)
    for (buf, o), want, shape in zip(bufs, wants, shapes):
        intact(buf, o, f"{kind} {shape} {order}")
        same(o, want, f"{kind} {shape} {order}")


@pytest.mark.parametrize("outputs", ["both", "out only", "out_t only"])
def test_cast_transpose_bits(outputs):
    for i, (R, Cc) in enumerate(ma.TRANSPOSE_SHAPES):
        s = ma.small_ints((R, Cc), 60 + i).float() * 0.25 + 2.0 ** -8 * ma.small_ints((R, Cc), 90 + i, lo=-3, hi=3)
        want, want_t = ma.transpose_model(s, 32)
        b1, o = out_buf((R, Cc), BF)
        b2, ot = out_buf((Cc, R), BF)
        ok(_lib.lib().m3ae_cast_transpose(p(src(s)), p(o) if outputs != "out_t only" else None, p(ot) if outputs != "out only" else None, R, Cc,
                                          stream()), "m3ae_cast_transpose")
        intact(b1, o, f"cast_transpose out {(R, Cc)}"), intact(b2, ot, f"cast_transpose out_t {(R, Cc)}")
        same(o, want if outputs != "out_t only" else torch.full_like(want, ma.FENCE), f"cast_transpose out {(R, Cc)} {outputs}")
        same(ot, want_t if outputs != "out only" else torch.full_like(want_t, ma.FENCE), f"cast_transpose out_t {(R, Cc)} {outputs}")


@pytest.mark.parametrize("L", ma.RANK_L)
def test_mask_ranks_are_the_stable_double_argsort(L):
    noise = ma.rank_noise(L)
    B = noise.shape[0]
    dn = src(noise)
    for len_keep in sorted({0, L // 4, L}):
        want_r, want_m, want_k = ma.ranks_reference(noise, len_keep)
        rb, r = out_buf((B, L), torch.int64)
        kb, k = out_buf((B, len_keep + 1), torch.int64)
        mb, m = out_buf((B, L), F32)
        ok(_lib.lib().m3ae_mask_ranks(p(dn), p(r), p(k), p(m), B, L, len_keep, stream()), "m3ae_mask_ranks")
        for b, v, w, what in ((rb, r, want_r, "ranks"), (kb, k, want_k, "keep_rows"), (mb, m, want_m, "mask")):
            intact(b, v, f"mask_ranks L {L} keep {len_keep} {what}")
            same(v, w, f"mask_ranks L {L} keep {len_keep} {what}")


@pytest.mark.parametrize("shape", ma.MIM_TARGET_SHAPES, ids=str)
def test_mim_targets(shape):
    Cc, H, W, P = shape
    img = ma.mim_target_inputs(Cc, H, W, P)
    N, Lp, D = img.shape[0], (H // P) * (W // P), P * P * Cc
    di = src(img)
    buf, out = out_buf((N, Lp, D), F32)
    ok(_lib.lib().m3ae_mim_targets(p(di), p(out), N, Cc, H, W, P, 0, stream()), "m3ae_mim_targets")
    intact(buf, out, f"mim_targets {shape}")
    same(out, ma.mim_patches_reference(img, P), f"mim_targets {shape} without norm_pix")
    buf, out = out_buf((N, Lp, D), F32)
    ok(_lib.lib().m3ae_mim_targets(p(di), p(out), N, Cc, H, W, P, 1, stream()), "m3ae_mim_targets")
    intact(buf, out, f"mim_targets {shape} norm_pix")
    ref, bnd = ma.mim_target_reference(img, P)
    miss = ma.check_bound(out.cpu(), ref, bnd, f"mim_targets {shape} norm_pix", figures("mim_targets norm_pix"))
    assert miss is None, miss
    assert not bool(out[1, 0].any()), "a constant patch does not standardise to exact zeros"
    report("mim_targets norm_pix")


def run_dropout(x, rows, cols, pdrop, rmap, salt, dtype, want_out=True):
    L = _lib.lib()
    kb, keep = out_buf((rows, cols), torch.uint8)
    ob, out = out_buf((rows, cols), dtype) if want_out else (None, None)
    ds = None if salt is None else torch.tensor([salt], dtype=torch.int64, device=DEV).to(torch.int32)
    if rmap == (0, 1):
        rc = L.m3ae_dropout(p(x), p(out), p(keep), rows, cols, pdrop, ma.DROP_SEED, p(ds), code(dtype), stream())
    else:
        rc = L.m3ae_dropout_rows(p(x), p(out), p(keep), rows, cols, pdrop, ma.DROP_SEED, p(ds), code(dtype), rmap[0], rmap[1], stream())
    ok(rc, "m3ae_dropout")
    intact(kb, keep, f"dropout keep {rows}x{cols}")
    if want_out:
        intact(ob, out, f"dropout out {rows}x{cols}")
    return keep, out


@pytest.mark.parametrize("pdrop", ma.DROP_PS, ids=lambda q: f"p{q:.7f}")
def test_dropout_mask_is_the_hash_of_common_h(pdrop):
    rows = 37
    for cols in ma.DROP_COLS:
        for rmap in ma.DROP_ROW_MAPS:
            for salt in ma.DROP_SALTS:
                keep, _ = run_dropout(None, rows, cols, pdrop, rmap, salt, F32, want_out=False)
                want = torch.from_numpy(ma.keep_mask_model(rows, cols, pdrop, ma.DROP_SEED, rmap[0], rmap[1], salt))
                same(keep, want, f"keep mask p {pdrop} cols {cols} row map {rmap} salt {salt}")


@DTYPES
def test_dropout_outputs_and_the_large_mask(dtype):
    g = torch.Generator().manual_seed(16)
    cases = [(37, 577, q, (3, 5), 12345) for q in ma.DROP_PS] + [(*ma.DROP_BIG, 0.1, (0, 1), None), (37, 768, 0.5, (2 ** 40, 1), 0)]
    for rows, cols, pdrop, rmap, salt in cases:
        x = torch.randn(rows, cols, generator=g).to(dtype)
        keep, out = run_dropout(src(x), rows, cols, pdrop, rmap, salt, dtype)
        want = torch.from_numpy(ma.keep_mask_model(rows, cols, pdrop, ma.DROP_SEED, rmap[0], rmap[1], salt))
        same(keep, want, f"keep mask {rows}x{cols} p {pdrop}")
        same(out, ma.dropout_model(x, want, pdrop, dtype == BF), f"dropout output {name_of(dtype)} {rows}x{cols} p {pdrop}")
        assert not bool(torch.signbit(out[keep == 0].float()).any()), "a dropped element is not +0"
    x = torch.randn(37, 577, generator=g).to(dtype)
    keep, out = run_dropout(src(x), 37, 577, 0.0, (0, 1), None, dtype)
    assert bool(keep.all()), "p = 0 drops an element"
    same(out, x, "dropout p = 0")


# ------------------------------------------------------------------------------------------------------------------------
# bounded tier
# ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_act_fwd_and_bwd_against_float64(dtype):
    L, bf = _lib.lib(), dtype == BF
    x = ma.act_grid(bf)
    n = x.numel()
    dy = torch.linspace(-2, 2, n)
    dy = ma.rne_bf16(dy) if bf else dy
    dx_, ddy = src(x.to(dtype)), src(dy.to(dtype))
    for act in ma.ACTS:
        buf, y = out_buf((n,), dtype)
        ok(L.m3ae_act_fwd(p(dx_), p(y), n, act, code(dtype), stream()), "m3ae_act_fwd")
        intact(buf, y, f"act_fwd {act}")
        ref, bnd = ma.act_fwd_reference(x, act, bf)
        miss = ma.check_bound(y.cpu(), ref, bnd, f"act_fwd act {act} {name_of(dtype)}", figures(f"act_fwd {name_of(dtype)}"))
        assert miss is None, miss
        buf, g = out_buf((n,), dtype)
        ok(L.m3ae_act_bwd(p(ddy), p(dx_), p(g), n, act, code(dtype), stream()), "m3ae_act_bwd")
        intact(buf, g, f"act_bwd {act}")
        ref, bnd = ma.act_bwd_reference(dy, x, act, bf)
        miss = ma.check_bound(g.cpu(), ref, bnd, f"act_bwd act {act} {name_of(dtype)}", figures(f"act_bwd {name_of(dtype)}"))
        assert miss is None, miss
    report(f"act_fwd {name_of(dtype)}")
    report(f"act_bwd {name_of(dtype)}")


def test_image_normalize_u8_against_float64():
    u8 = ma.normalize_input()
    B, H, W = ma.NORMALIZE_SHAPE
    buf, out = out_buf((B, 3, H, W), F32)
    mean, std = (C.c_float * 3)(*ma.CLIP_MEAN), (C.c_float * 3)(*ma.CLIP_STD)
    ok(_lib.lib().m3ae_image_normalize_u8(p(src(u8)), p(out), B, H, W, mean, std, stream()), "m3ae_image_normalize_u8")
    intact(buf, out, "image_normalize_u8")
    ref, bnd = ma.normalize_reference(u8)
    miss = ma.check_bound(out.cpu(), ref, bnd, "image_normalize_u8", figures("image_normalize_u8"))
    assert miss is None, miss
    differ = ma.bits_differ(out.cpu(), torch.from_numpy(ma.normalize_model(u8)))
    print(f"MISC_ACCURACY image_normalize_u8: {differ} of {out.numel()} elements differ from the fp32 model")
    report("image_normalize_u8")


@DTYPES
@pytest.mark.parametrize("shape", ma.MIM_LOSS_SHAPES, ids=str)
def test_mim_loss_against_float64(dtype, shape):
    L, bf = _lib.lib(), dtype == BF
    B, Lp, D = shape
    form = f"mim_loss {name_of(dtype)}"
    for kind in ma.MIM_MASKS:
        x, t, mask = ma.mim_loss_inputs(B, Lp, D, kind, bf)
        loss, e_loss, dx, e_dx = ma.mim_loss_reference(x, t, mask, ma.MIM_GOUT)
        dx_, dt_, dm = src(x), src(t), src(mask)
        gout = torch.tensor([ma.MIM_GOUT], device=DEV)
        losses = []
        for det in (False, True, True):
            ab, acc = out_buf((2,), F32)
            lb, out = out_buf((1,), F32)
            if det:
                ws, n = ops._small_ws(_lib.DET_MIM, B * Lp, D, torch.device(DEV))
                ok(L.m3ae_mim_loss_fwd_det(p(dx_), p(dt_), p(dm), p(acc), p(out), B, Lp, D, code(dtype), p(ws), n, stream()), "mim_loss_fwd_det")
            else:
                ok(L.m3ae_mim_loss_fwd(p(dx_), p(dt_), p(dm), p(acc), p(out), B, Lp, D, code(dtype), stream()), "mim_loss_fwd")
            intact(ab, acc, "mim_loss acc"), intact(lb, out, "mim_loss loss")
            got = out.item()
            f = figures(form + (" ordered" if det else ""))
            f["loss err/bound"] = max(f.get("loss err/bound", 0.0), abs(got - loss.item()) / e_loss.item())
            assert math.isfinite(got) and abs(got - loss.item()) <= e_loss.item(), (shape, kind, det, got, loss.item(), e_loss.item())
            assert acc[1].item() == mask.sum().item()
            losses.append(got)
            gb, g = out_buf((B, Lp + 1, D), dtype)
            ok(L.m3ae_mim_loss_bwd(p(dx_), p(dt_), p(dm), p(acc), p(gout), p(g), B, Lp, D, code(dtype), stream()), "mim_loss_bwd")
            intact(gb, g, "mim_loss dx")
            miss = ma.check_bound(g.cpu(), dx, ma._store_bound(dx, e_dx, bf), f"mim_loss_bwd {shape} {kind}", figures(form + " bwd"))
            assert miss is None, miss
            assert not bool(g[:, 0].any()) and not bool(g[:, 1:][dm == 0].any()), "class rows / unmasked rows are not exact zeros"
        assert losses[1] == losses[2], "ordered form: two calls differ"
    for f in (form, form + " ordered", form + " bwd"):
        report(f)


# ------------------------------------------------------------------------------------------------------------------------
# through ops
# ------------------------------------------------------------------------------------------------------------------------
def _gather_case(dtype, repeated):
    g = torch.Generator().manual_seed(17)
    R, D = 50, 72
    if repeated:   # every row up to four times
        idx = torch.cat([torch.arange(R), torch.arange(0, R, 2), torch.arange(0, R, 4), torch.arange(0, R, 8)])[torch.randperm(95, generator=g)]
        assert idx.bincount().max() == 4
    else:
        idx = torch.randperm(R, generator=g)[:37]
    return torch.randn(R, D, generator=g).to(dtype), idx, torch.randn(idx.numel(), D, generator=g).to(dtype)


@DTYPES
def test_gather_rows_backward_with_repeated_indices(dtype):
    """d_src[r] = the sum of the dy rows gathered from r (at most 4): within 4 u sum|dy| of the float64 index_add_, and the store."""
    table, idx, dy = _gather_case(dtype, repeated=True)
    x = table.to(DEV).requires_grad_(True)
    ops.gather_rows(x, idx.to(DEV)).backward(dy.to(DEV))
    ref = torch.zeros(table.shape, dtype=F64).index_add_(0, idx, dy.double())
    bnd = ma._store_bound(ref, 4 * ma.U * torch.zeros(table.shape, dtype=F64).index_add_(0, idx, dy.double().abs()), dtype == BF)
    miss = ma.check_bound(x.grad.cpu(), ref, bnd, f"gather_rows backward {name_of(dtype)}", figures(f"gather_rows backward {name_of(dtype)}"))
    assert miss is None, miss
    report(f"gather_rows backward {name_of(dtype)}")


@DTYPES
def test_gather_rows_backward_of_a_permutation_is_the_kernel_path(dtype):
    table, idx, dy = _gather_case(dtype, repeated=False)
    want = torch.zeros(table.shape, dtype=dtype, device=DEV)
    ok(_lib.lib().m3ae_scatter_add_rows(p(dev(dy)), p(dev(idx)), p(want), idx.numel(), table.shape[1], code(dtype), stream()), "scatter")
    same(want, torch.zeros(table.shape).index_add_(0, idx, dy.float()), "scatter onto zeros")
    for unique in (False, True):
        x = table.to(DEV).requires_grad_(True)
        y = ops.gather_rows(x, idx.to(DEV), unique=unique)
        same(y, table[idx], "gather_rows forward")
        y.backward(dy.to(DEV))
        same(x.grad, want, f"gather_rows backward of a permutation, unique={unique}")
    with ops.deterministic_mode(True):
        x = table.to(DEV).requires_grad_(True)
        ops.gather_rows(x, idx.to(DEV), unique=True).backward(dy.to(DEV))
        same(x.grad, want, "gather_rows backward, unique=True in deterministic mode")
        x = table.to(DEV).requires_grad_(True)
        y = ops.gather_rows(x, idx.to(DEV))
        with pytest.raises(ops.DeterministicError):
            y.backward(dy.to(DEV))
