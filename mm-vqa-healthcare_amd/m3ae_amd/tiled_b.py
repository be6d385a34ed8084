"""The tiled layout of a K-contiguous bf16 weight W[N][K] (csrc/tiled_b.h), mirrored in Python, and the job table of the kernel
that writes it (m3ae_tile_bf16_batched).

block = 16 rows x 32 k (1 KiB); the 16 blocks of rows [256 T, 256 T + 256) x k [32 c, 32 c + 32) are consecutive (a chunk, 16 KiB);
a tile's K / 32 chunks follow each other along k; N is padded to a multiple of 256 with zero rows.  Inside a block the 16-byte
unit u (8 k) of row r sits at unit position u ^ swz(r), swz(r) = (4 - ((r >> 2) & 3)) & 3: the source-side swizzle of the NT
kernels' LDS image is part of the layout.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

ROWS, CK, BLOCK_ELEMS, CHUNK_ELEMS = 256, 32, 512, 8192


def tiled_rows(N):
    """Rows of the padded copy; it holds tiled_rows(N) * K elements."""
    return (N + ROWS - 1) // ROWS * ROWS


def tiled_index(n, k, K):
    """Element index of W[n][k] in the tiled copy (m3ae_tiled_b_index); n, k: ints, numpy arrays or integer tensors."""
    T, c = n >> 8, k >> 5
    p, r, u = (n >> 4) & 15, n & 15, (k >> 3) & 3
    swz = (4 - ((r >> 2) & 3)) & 3
    return (T * (K >> 5) + c) * CHUNK_ELEMS + p * BLOCK_ELEMS + r * 32 + ((u ^ swz) << 3) + (k & 7)


def tile_reference(w):
    """The tiled copy of w [N, K] (K % 32 == 0) as the flat tensor the kernel writes, built with the index function alone."""
    N, K = w.shape
    assert K % CK == 0
    out = torch.zeros(tiled_rows(N) * K, dtype=w.dtype, device=w.device)
    n = torch.arange(N, device=w.device, dtype=torch.int64)[:, None]
    k = torch.arange(K, device=w.device, dtype=torch.int64)[None, :]
    out[tiled_index(n, k, K).reshape(-1)] = w.reshape(-1)
    return out


def job_tiles(R, C_, fwd, t_tiled):
    """64 x 64 tiles the kernel walks for a unit in[R][C]: the padding rows of the tiled copies have tiles of their own."""
    Rp = tiled_rows(R) if fwd else R
    Cp = tiled_rows(C_) if t_tiled else C_
    return ((Rp + 63) // 64) * ((Cp + 63) // 64)


def job_table(entries, device):
    """entries: (src, out_tiled, out_t, out_t_tiled) per unit; src a contiguous bf16 [R, C] tensor, the outputs bf16 tensors or
    None.  Returns (device int64 table, number of jobs, total tiles) for run()."""
    tab = np.zeros((len(entries), 7), dtype=np.int64)
    first = 0
    for i, (src, out_tiled, out_t, out_t_tiled) in enumerate(entries):
        R, C_ = src.shape
        assert src.dtype == torch.bfloat16 and src.is_contiguous() and R % 8 == 0 and C_ % 8 == 0
        for t, need in ((src, R * C_), (out_tiled, tiled_rows(R) * C_), (out_t, R * C_), (out_t_tiled, tiled_rows(C_) * R)):
            assert t is None or (t.dtype == torch.bfloat16 and t.is_contiguous() and t.numel() >= need and t.data_ptr() % 16 == 0)
        assert out_tiled is None or C_ % CK == 0
        assert out_t_tiled is None or R % CK == 0
        ptr = lambda t: 0 if t is None else t.data_ptr()
        tab[i] = (src.data_ptr(), ptr(out_tiled), ptr(out_t), ptr(out_t_tiled), R, C_, first)
        first += job_tiles(R, C_, out_tiled is not None, out_t_tiled is not None)
    return torch.from_numpy(tab).to(device), len(entries), first


def run(jobs, njobs, tiles, stream=None):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    _lib.check(_lib.lib().m3ae_tile_bf16_batched(C.c_void_p(jobs.data_ptr()), njobs, tiles, s), "m3ae_tile_bf16_batched")


def attach(w_param, device=None):
    """Give one weight parameter (with bf16 copies m3ae_c / m3ae_t) its tiled copies and fill them: what ParamStore does for every
    weight unit.  For callers that manage their own parameters (tests, tools)."""
    w = w_param.m3ae_c
    N, K = w.shape
    fwd = torch.empty(tiled_rows(N) * K, dtype=torch.bfloat16, device=w.device) if K % CK == 0 else None
    tt = torch.empty(tiled_rows(K) * N, dtype=torch.bfloat16, device=w.device) if N % CK == 0 else None
    jobs, n, tiles = job_table([(w, fwd, None, tt)], w.device)
    run(jobs, n, tiles)
    if fwd is not None:
        w.m3ae_tb = fwd
    w_param.m3ae_tt = tt
    return fwd, tt
