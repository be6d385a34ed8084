"""GPU: the row reader of csrc/row_scan.h (walk_row, and token_chunk_kernel's own copy of its geometry) through the four entry points
that read rows with it -- m3ae_greedy_argmax, m3ae_trie_scan, m3ae_token_eval and m3ae_vqa_eval -- at every misalignment of a row's first element: every column is read exactly once, under its own number, and
nothing outside the view is read.

R = V rows, row r with its one maximum at column r, so a column that is skipped or numbered wrongly moves some row's argmax.  Every
other value is within 2.25 of the maximum, so a column read twice (or not at all) moves its chunk's s = sum exp(x - m) by at least
e^-2.25 / 64 > 1.6e-3 of s, far above the bound s is held to.  The rows lie in a buffer whose every other element is +inf or NaN: a
read outside the view takes the argmax and poisons (m, s).  The row stride V + 1 walks the rows' own alignment as well.

The (m, s) bound is tests/answer_trie_model.py's with the steps after the chunk's own fold left out: m is the chunk's maximum exactly,
and |s - S| / S <= u (sum t e^-t / S + P) + u^2 sum t^2 e^-t / S, P = P_trie - 4 chunks (thread + one 6 + 3 merge tree), times the
model's (1 + 2^-20).  The 4 chunks are the last term of answer_trie_model.path_units: the sequential merges of a row's chunk pairs in
m3ae_trie_step (4 units each), which the pairs m3ae_trie_scan leaves in the workspace have not been through."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import answer_trie_model as AM  # noqa: E402
import token_eval_model as TM  # noqa: E402
from m3ae_amd import ops  # noqa: E402

DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129)
CHUNK = 64


def rows_for(V):
    """float32 [V, V], exact in bf16: row r holds 1 at column r and multiples of -0.25 in [-1.25, -0.25] elsewhere."""
    r, c = np.meshgrid(np.arange(V), np.arange(V), indexing="ij")
    x = (-0.25 - 0.25 * ((7 * c + 3 * r) % 5)).astype(np.float32)
    x[np.arange(V), np.arange(V)] = 1.0
    return x


def on_device(x, dtype, off):
    """The [R, V] view that starts `off` elements into a buffer with row stride V + 1; every element outside it is +inf or NaN."""
    R, V = x.shape
    ld = V + 1
    buf = torch.full((R * ld + off + 8,), float("inf"), dtype=dtype, device=DEV)
    buf[1::2] = float("nan")
    v = buf.as_strided((R, V), (ld, 1), off)
    v.copy_(torch.from_numpy(x).to(dtype).to(DEV))
    assert v.data_ptr() == buf.data_ptr() + off * buf.element_size() and torch.equal(v.float().cpu(), torch.from_numpy(x))
    return v


def one_child_table():
    """A trie table whose root has the one child token 0: all m3ae_trie_scan needs to run its chunk items."""
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    return NS(child_off=i32([0, 1, 1]), child_tok=i32([0]), child_node=i32([1]), leaf_label=i32([-1, 0]), N=2, E=1, depth=1)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_every_column_once_at_every_misalignment(dname):
    dtype = DTYPES[dname]
    itemsize = 4 if dname == "fp32" else 2
    tab = one_child_table()
    for V in SIZES:
        x = rows_for(V)
        want = np.arange(V)
        nch = -(-V // CHUNK)
        units = AM.path_units(V, CHUNK, itemsize) - 4 * nch
        for off in range(16 // itemsize):
            where = (V, off)
            xd = on_device(x, dtype, off)
            for chunk in (0, CHUNK):
                got = ops.greedy_argmax(xd, chunk, out=torch.empty(V, dtype=torch.int64, device=DEV))
                assert np.array_equal(got.cpu().numpy(), want), (where, chunk)
                assert np.array_equal(ops.token_eval(xd, chunk=chunk, want_rows=True).pred.cpu().numpy(), want), (where, chunk)
            assert np.array_equal(ops.vqa_eval(xd, None, None, None, want_rows=True).pred.cpu().numpy(), want), where

            st = ops.TrieState(V, 1, DEV)
            ws = ops.trie_scan(xd, tab, st, CHUNK)
            ms = ws.view(-1)[V:].view(torch.float32).view(V, nch, 2).cpu().numpy().astype(np.float64)
            for r in range(V):
                for c in range(nch):
                    part = x[r, c * CHUNK:(c + 1) * CHUNK]
                    _, S, M, tsum, t2sum = TM.lse64(part)
                    rel = (TM.U * (tsum / S + units) + TM.U * TM.U * t2sum / S) * TM.SLACK
                    assert ms[r, c, 0] == M and abs(ms[r, c, 1] - S) <= rel * S, (where, r, c, ms[r, c], M, S, rel)
