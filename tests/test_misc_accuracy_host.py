"""CPU: the yardsticks of tests/misc_accuracy.py checked on themselves, at the cases of tests/test_gpu_misc_accuracy.py.

  * the mirrors and references agree with independent torch (or plain integer) statements of the same operation: the keep mask
    with a scalar restatement of csrc/common.h in Python integers, the ranks with the stable argsort of the argsort, the patches with
    the einsum of the reference implementation, the embeddings with torch.nn.functional, the scatter with index_add_;
  * for every bounded case a sequential and a pairwise fp32 model stay within the bound (and the yardstick); the worst model / bound
    ratios are printed (pytest -s) and recorded in the docstring of tests/misc_accuracy.py;
  * every criterion fails on its mutants: each (case table, mutant) pair below must be rejected on at least one case of the table."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import misc_accuracy as ma

F32, BF, F64 = torch.float32, torch.bfloat16, torch.float64


# ------------------------------------------------------------------------------------------------------------------------
# the mirrors against independent statements
# ------------------------------------------------------------------------------------------------------------------------
def _keep_scalar(row, col, cols, p, seed, base, step, salt):
    """One element of the mask from the comment of csrc/common.h, in Python integers."""
    M = 0xFFFFFFFF
    idx = (base + row * step) * ((cols + 3) // 4 * 4) + col
    g = idx >> 2
    key_hi = (seed >> 32) & M
    if salt is not None:
        key_hi = (key_hi + salt * 0x85EBCA6B) & M
    x = (((g & M) ^ (seed & M)) + (g >> 32) * 0x9E3779B9 + key_hi) & M
    x ^= x >> 16
    x = x * 0x7feb352d & M
    x ^= x >> 15
    x = x * 0x846ca68b & M
    x ^= x >> 16
    r = 8 * (idx & 3)
    rot = ((x >> r) | (x << (32 - r))) & M
    return int(rot >= min(int(float(np.float32(p)) * 2.0 ** 32), M))


def test_keep_mask_model_is_the_hash_of_common_h():
    rng = np.random.default_rng(5)
    for p in ma.DROP_PS + (0.0,):
        for cols in ma.DROP_COLS:
            for base, step in ma.DROP_ROW_MAPS:
                for salt in ma.DROP_SALTS:
                    m = ma.keep_mask_model(9, cols, p, ma.DROP_SEED, base, step, salt)
                    for _ in range(24):
                        r, c = int(rng.integers(9)), int(rng.integers(cols))
                        assert m[r, c] == _keep_scalar(r, c, cols, p, ma.DROP_SEED, base, step, salt), (p, cols, base, step, salt, r, c)
    assert ma.keep_mask_model(64, 768, 0.0, 3).all()
    assert ma.drop_threshold(ma.P_BELOW_ONE) == 2 ** 32 - 256 and float(ma.inv_keep(ma.P_BELOW_ONE)) == 2.0 ** 24
    share = ma.keep_mask_model(512, 768, 0.1, 11).mean()
    assert abs(share - 0.9) < 4 * math.sqrt(0.09 / (512 * 768)), share
    assert ma.DROP_BIG[0] * ma.DROP_BIG[1] > 2 ** 21 and (2 ** 40 * 768) >> 34 > 0


def test_ranks_are_the_stable_double_argsort():
    for L in ma.RANK_L:
        noise = ma.rank_noise(L)
        for len_keep in (0, L // 4, L):
            got, want = ma.ranks_model(noise, len_keep), ma.ranks_reference(noise, len_keep)
            for g, w in zip(got, want):
                assert torch.equal(g, w), (L, len_keep)
    assert (ma.rank_noise(36)[2] == 0).sum() > 4 and torch.signbit(ma.rank_noise(36)[2][ma.rank_noise(36)[2] == 0]).any()


def test_patches_are_the_einsum_and_the_unfold():
    for C, H, W, P in ma.MIM_TARGET_SHAPES:
        img = ma.mim_target_inputs(C, H, W, P)
        h, w = H // P, W // P
        x = img.reshape(img.shape[0], C, h, P, w, P)
        want = torch.einsum("nchpwq->nhwpqc", x).reshape(img.shape[0], h * w, P * P * C)
        assert torch.equal(ma.mim_patches_reference(img, P), want)
    for R, P in ma.PATCHIFY_SHAPES:
        img = torch.randn(2, 3, R, R)
        g = R // P
        want = img.reshape(2, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(2, g * g, 3 * P * P)
        assert torch.equal(ma.patchify_reference(img, P), want)


def test_embedding_model_is_torch_functional():
    word, pos, typ = ma.embed_tables(130)
    for name, (ids, pad) in ma.embed_fwd_cases().items():
        mask = ids.ne(pad).int()
        pid = (torch.cumsum(mask, dim=1).type_as(mask) * mask).long() + pad   # transformers' create_position_ids_from_input_ids
        assert torch.equal(ma.position_ids(ids, pad), pid), name
        want = F.embedding(ids, word) + F.embedding(torch.zeros_like(ids), typ) + F.embedding(pid, pos)
        assert torch.equal(ma.embed_fwd_model(ids, word, pos, typ, pad, False), want), name
    assert ma.position_ids(*ma.embed_fwd_cases()["full-512-pad1"]).max() == 513 == ma.EMBED_POS_ROWS - 1


def test_scatter_and_embedding_backward_are_index_add():
    for bf16 in (False, True):
        d_in, d_out = ma.small_ints((40, 7), 1).float() / 4, ma.small_ints((12, 7), 2).float() / 64
        idx = torch.randperm(40, generator=torch.Generator().manual_seed(3))[:12]
        want = ma.store(d_in.clone().index_add_(0, idx, d_out), bf16)
        assert torch.equal(ma.scatter_add_model(d_out, idx, d_in, bf16), want)
    for name, (ids, pad) in ma.embed_bwd_cases().items():
        assert ids.numel() == 300
        D = 12
        d = ma.small_ints((3, 100, D), 9)
        w0, p0, t0 = ma.small_ints((16, D), 10), ma.small_ints((ma.EMBED_POS_ROWS, D), 11), ma.small_ints((D,), 12)
        w, p, t = ma.embed_bwd_reference(ids, d, w0, p0, t0, pad)
        pid = ma.position_ids(ids, pad).reshape(-1)
        assert torch.equal(w.float(), w0.clone().index_add_(0, ids.reshape(-1), d.reshape(-1, D))), name
        assert torch.equal(p.float(), p0.clone().index_add_(0, pid, d.reshape(-1, D))) and torch.equal(t.float(), t0 + d.sum((0, 1))), name
        assert w.abs().max() < 2 ** 24 / 8


# ------------------------------------------------------------------------------------------------------------------------
# bounded cases: the fp32 models stay inside, the ratios are printed
# ------------------------------------------------------------------------------------------------------------------------
def _colsum_cases():
    for M, N in ma.COLSUM_SHAPES:
        for bf16 in (False, True):
            for kind in ("mean0", "mean64"):
                for acc in (False, True):
                    yield M, N, bf16, kind, acc


def test_colsum_models_are_inside_the_bound_and_the_yardstick():
    worst = {"pair": {}, "seq": {}}
    for M, N, bf16, kind, acc in _colsum_cases():
        if bf16 and N == 4096:
            continue   # (the same arithmetic as the fp32 case of that shape: the models read fp32 values either way)
        x, old = ma.colsum_inputs(M, N, kind, bf16)
        old = old if acc else None
        seq = ma.colsum_model(x, old, "seq")
        for order in ("pair", "seq"):
            got = seq if order == "seq" else ma.colsum_model(x, old, "pair")
            yard = seq if kind == "mean64" else None   # the yardstick is for terms of one sign (tests/misc_accuracy.py)
            assert ma.colsum_misses(got, x, old, yard, worst[order], f"colsum {M}x{N} {kind}") == []
    for order in ("pair", "seq"):
        print(f"MISC_ACCURACY host, colsum {order} model: " + ", ".join(f"worst {k} {v:.3e}" for k, v in sorted(worst[order].items())))
        assert 0 < worst[order]["err/bound"] <= 1.0
    for M, N in ma.COLSUM_ROWS:
        P, R, per, nwg = ma.colsum_rows_geometry(M, N)
        assert M >= 4096 and N % 8 == 0 and P <= 512 and 1 <= R and P * R <= 512 and M % per != 0 and (M % per) % (4 * R) != 0, (M, N)
    assert {ma.colsum_rows_geometry(M, N)[1] for M, N in ma.COLSUM_ROWS} == {512, 7, 5, 1}


def test_elementwise_models_are_inside_the_bound():
    fig = {}
    u8 = ma.normalize_input()
    assert all(len(set(u8[..., c].reshape(-1).tolist())) == 256 for c in range(3))
    ref, bnd = ma.normalize_reference(u8)
    assert ma.check_bound(ma.normalize_model(u8), ref, bnd, "image_normalize", fig.setdefault("image_normalize", {})) is None
    for bf16 in (False, True):
        x = ma.act_grid(bf16)
        dy = torch.linspace(-2, 2, x.numel())
        dy = ma.rne_bf16(dy) if bf16 else dy
        for act in ma.ACTS:
            ref, bnd = ma.act_fwd_reference(x, act, bf16)
            assert ma.check_bound(ma.store(ma.act32(x, act), bf16), ref, bnd, f"act_fwd {act}", fig.setdefault("act_fwd", {})) is None
            ref, bnd = ma.act_bwd_reference(dy, x, act, bf16)
            got = ma.store(dy * ma.act32(x, act, grad=True), bf16)
            assert ma.check_bound(got, ref, bnd, f"act_bwd {act}", fig.setdefault("act_bwd", {})) is None
    for k, v in fig.items():
        print(f"MISC_ACCURACY host, {k} fp32 model: worst err/bound {v['err/bound']:.3f}")
        assert 0 < v["err/bound"] <= 1.0


def test_mim_models_are_inside_the_bound():
    fig = {o: {"target": {}, "loss": {}, "grad": {}} for o in ("pair", "seq")}
    for C, H, W, P in ma.MIM_TARGET_SHAPES:
        img = ma.mim_target_inputs(C, H, W, P)
        ref, bnd = ma.mim_target_reference(img, P)
        for order in ("pair", "seq"):
            got = ma.mim_target_model(img, P, order)
            assert ma.check_bound(got, ref, bnd, f"mim target {(C, H, W, P)}", fig[order]["target"]) is None
            assert not got[1, 0].any(), "a constant patch is exactly zero"
    for B, L, D in ma.MIM_LOSS_SHAPES:
        for kind in ma.MIM_MASKS:
            for bf16 in (False, True):
                x, t, mask = ma.mim_loss_inputs(B, L, D, kind, bf16)
                loss, e_loss, dx, e_dx = ma.mim_loss_reference(x, t, mask, ma.MIM_GOUT)
                for order in ("pair", "seq"):
                    got_loss, got_dx = ma.mim_loss_model(x, t, mask, ma.MIM_GOUT, bf16, order)
                    r = abs(float(got_loss) - loss.item()) / e_loss.item()
                    fig[order]["loss"]["err/bound"] = max(fig[order]["loss"].get("err/bound", 0.0), r)
                    assert r <= 1.0, (B, L, D, kind, bf16, order, r)
                    assert ma.check_bound(got_dx, dx, ma._store_bound(dx, e_dx, bf16), "mim dx", fig[order]["grad"]) is None
                    assert not got_dx[:, 0].any() and not got_dx[:, 1:][mask == 0].any()
    for order in ("pair", "seq"):
        print(f"MISC_ACCURACY host, MIM {order} model: " + ", ".join(f"{k} worst err/bound {v['err/bound']:.3f}" for k, v in fig[order].items()))
        assert all(0 < v["err/bound"] <= 1.0 for v in fig[order].values())
    assert ma.MIM_LOSS_SHAPES[-1][0] * ma.MIM_LOSS_SHAPES[-1][1] > 4096


# ------------------------------------------------------------------------------------------------------------------------
# mutants: per case table, rejected on at least one case
# ------------------------------------------------------------------------------------------------------------------------
def _colsum_exact(mutant):
    for M, N in ma.COLSUM_SHAPES:
        x, old = ma.colsum_inputs(M, N, "ints", True)
        yield bool(ma.colsum_misses(ma.colsum_model(x, old, "pair", mutant), x, old, exact=True)), bool(ma.colsum_misses(ma.colsum_model(x, old, "pair"), x, old, exact=True))


def _colsum_bounded(mutant):
    for M, N in ma.COLSUM_SHAPES:
        if N < ma.MIN_COLS or N == 4096:
            continue   # below MIN_COLS only the element-wise bound holds a case, and at mean 64 that bound exceeds one row
        x, _ = ma.colsum_inputs(M, N, "mean64", False)
        seq = ma.colsum_model(x, None, "seq")
        yield bool(ma.colsum_misses(ma.colsum_model(x, None, "pair", mutant), x, None, seq)), bool(ma.colsum_misses(ma.colsum_model(x, None, "pair"), x, None, seq))


def _cast(mutant):
    for n in ma.CAST_SIZES[:3]:
        v = ma.cast_values(n)
        yield ma.bits_differ(ma.cast_model(v, True, mutant), v.to(BF)) > 0, ma.bits_differ(ma.cast_model(v, True), v.to(BF)) > 0


def _add(mutant):
    for n in ma.ADD_SIZES[:2]:
        a, b = ma.add_values(n, True)
        want = (a.float() + b.float()).to(BF).float()
        yield ma.bits_differ(ma.add_model(a, b, True, mutant), want) > 0, ma.bits_differ(ma.add_model(a, b, True), want) > 0


def _embed(mutant):
    word, pos, typ = ma.embed_tables(130)
    for name, (ids, pad) in ma.embed_fwd_cases().items():
        want = (F.embedding(ids, word) + typ[0] + F.embedding(ma.position_ids(ids, pad), pos)).to(BF).float()
        yield ma.bits_differ(ma.embed_fwd_model(ids, word, pos, typ, pad, True, mutant), want) > 0, \
            ma.bits_differ(ma.embed_fwd_model(ids, word, pos, typ, pad, True), want) > 0


def _ranks(mutant):
    for L in ma.RANK_L:
        noise = ma.rank_noise(L)
        want = ma.ranks_reference(noise, L // 4)
        yield any(not torch.equal(g, w) for g, w in zip(ma.ranks_model(noise, L // 4, mutant), want)), \
            any(not torch.equal(g, w) for g, w in zip(ma.ranks_model(noise, L // 4), want))


def _mim_target(mutant):
    for C, H, W, P in ma.MIM_TARGET_SHAPES:
        img = ma.mim_target_inputs(C, H, W, P)
        ref, bnd = ma.mim_target_reference(img, P)
        yield ma.check_bound(ma.mim_target_model(img, P, "pair", mutant), ref, bnd, "t") is not None, \
            ma.check_bound(ma.mim_target_model(img, P, "pair"), ref, bnd, "t") is not None


def _transposes(mutant):
    for tile in (32, 64):
        for R, C in ma.TRANSPOSE_SHAPES:
            src = ma.small_ints((R, C), R + C).float() + 2.0 ** -8
            want = ma.rne_bf16(src).t().contiguous()
            yield ma.bits_differ(ma.transpose_model(src, tile, mutant)[1], want) > 0, ma.bits_differ(ma.transpose_model(src, tile)[1], want) > 0


def _mask(mutant):
    for cols in ma.DROP_COLS:
        for base, step in ma.DROP_ROW_MAPS:
            want = ma.keep_mask_model(33, cols, 0.5, ma.DROP_SEED, base, step, 12345)
            yield bool((ma.keep_mask_model(33, cols, 0.5, ma.DROP_SEED, base, step, 12345, mutant=mutant) != want).any()), False


TABLES = [("colsum exact", _colsum_exact, ma.COLSUM_MUTANTS), ("colsum bounded", _colsum_bounded, ma.COLSUM_MUTANTS),
          ("cast", _cast, ("store_truncates", "store_half_up")), ("add", _add, ("store_truncates", "store_half_up")),
          ("embed forward", _embed, ("store_truncates", "store_half_up", "pad_advances_position")), ("ranks", _ranks, ("unstable_tie_break",)),
          ("MIM target", _mim_target, ("biased_variance",)), ("transposes", _transposes, ("edge_tile_bounds_swapped",)),
          ("keep mask", _mask, ma.MASK_MUTANTS)]


@pytest.mark.parametrize("table,mutant", [(t[0], m) for t in TABLES for m in t[2]])
def test_mutant_is_rejected_by_its_case_table(table, mutant):
    run = {t[0]: t[1] for t in TABLES}[table]
    res = list(run(mutant))
    assert not any(clean for _, clean in res), f"{table}: the unmutated model misses its own criterion"
    n = sum(bad for bad, _ in res)
    print(f"MISC_ACCURACY host, {table}: mutant {mutant} rejected on {n} of {len(res)} cases")
    assert n > 0, f"{table}: mutant {mutant} survives every case"


def test_store_mutants_differ_only_where_they_should():
    v = torch.tensor(ma.SPECIALS[:4])
    assert ma.store(v, True).tolist() == [1.0, 1.015625, -1.0, -1.015625]
    assert ma.store(v, True, "store_half_up").tolist() == [1.0078125, 1.015625, -1.0078125, -1.015625]
    assert ma.store(v, True, "store_truncates").tolist() == [1.0, 1.0078125, -1.0, -1.0078125]
    a = np.array([[2.0 ** 24, 1.0, 1.0, 1.0, 1.0]], np.float32)
    assert ma.sum_seq(a)[0] == 2.0 ** 24 and ma.sum_pair(a)[0] == 2.0 ** 24 + 4
