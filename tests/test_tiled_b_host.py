"""Host: the tiled weight layout (csrc/tiled_b.h) through its Python mirror m3ae_amd/tiled_b.py -- the properties the NT kernels
rely on, checked on index arithmetic alone (no GPU, no library)."""
import numpy as np
import pytest
import torch

from m3ae_amd import tiled_b as tb


def swz32(r):
    return (4 - ((r >> 2) & 3)) & 3          # mfma_tiles.h: nt_swz<32>


def swz64(r):
    return (r >> 1) & 7                      # mfma_tiles.h: nt_swz<64>


@pytest.mark.parametrize("N,K", [(16, 32), (128, 64), (200, 96), (256, 288), (384, 64), (520, 256)])
def test_index_is_a_bijection_onto_the_padded_copy(N, K):
    Np = tb.tiled_rows(N)
    assert Np % 256 == 0 and Np >= N and Np - N < 256
    n, k = np.meshgrid(np.arange(Np, dtype=np.int64), np.arange(K, dtype=np.int64), indexing="ij")
    idx = tb.tiled_index(n, k, K).reshape(-1)
    assert idx.min() == 0 and idx.max() == Np * K - 1 and np.unique(idx).size == Np * K
    # 8 consecutive k (one 16-byte unit) stay consecutive: every kernel moves 16 bytes per lane
    i2 = tb.tiled_index(n, k, K)
    assert np.array_equal(i2[:, 1:][:, (np.arange(1, K) % 8) != 0], i2[:, :-1][:, (np.arange(1, K) % 8) != 0] + 1)


@pytest.mark.parametrize("N,K", [(256, 64), (700, 288)])
def test_blocks_chunks_and_tiles_are_consecutive(N, K):
    Np, nc = tb.tiled_rows(N), K // 32
    for T in range(Np // 256):
        for c in range(nc):
            base = (T * nc + c) * tb.CHUNK_ELEMS                # chunks of a tile follow each other along k, tiles each other
            for p in range(16):                                 # the 16 blocks of a chunk, 1 KiB each
                n, k = np.meshgrid(np.arange(16) + T * 256 + p * 16, np.arange(32) + c * 32, indexing="ij")
                idx = np.sort(tb.tiled_index(n.astype(np.int64), k.astype(np.int64), K).reshape(-1))
                assert np.array_equal(idx, base + p * tb.BLOCK_ELEMS + np.arange(512)), (T, c, p)
    # a 128-row half of a chunk (the 128 x 128 kernel's tile rows) is 8 consecutive blocks
    n, k = np.meshgrid(np.arange(128, 256, dtype=np.int64), np.arange(32, dtype=np.int64), indexing="ij")
    idx = np.sort(tb.tiled_index(n, k, K).reshape(-1))
    assert np.array_equal(idx, 8 * tb.BLOCK_ELEMS + np.arange(8 * 512))


def _lds_image_row_major(w, n0, c, bkt, rows):
    """The LDS image nt_stage builds for tile rows [n0, n0 + rows) and reduction step c of depth bkt: 1-KiB pieces, lane i of
    piece `seg` fetches 8 elements of row seg * rps + i // cpr at unit (i % cpr) ^ swz(row); rows past N are clamped."""
    N, K = w.shape
    cpr, rps = bkt // 8, 64 // (bkt // 8)
    swz = swz32 if bkt == 32 else swz64
    img = np.zeros(rows * bkt, dtype=w.dtype)
    for seg in range(rows // rps):
        for lane in range(64):
            row = seg * rps + lane // cpr
            unit = (lane % cpr) ^ swz(row)
            g = min(n0 + row, N - 1)
            img[seg * 512 + lane * 8: seg * 512 + lane * 8 + 8] = w[g, c * bkt + unit * 8: c * bkt + unit * 8 + 8]
    return img


def test_lds_image_of_the_ping_pong_kernels_is_the_row_major_one():
    """32-deep chunks of a 256-row tile: piece p of the chunk is bytes [1024 p, 1024 p + 1024) of the chunk, lane-linear.  Valid
    rows must give the image the row-major path builds (rows past N differ: zero padding instead of a clamped copy, and are never
    stored)."""
    N, K = 300, 96
    w = (np.arange(N * K, dtype=np.int64) % 65521).astype(np.uint16).reshape(N, K)
    t = tb.tile_reference(torch.from_numpy(w.astype(np.int16))).numpy().astype(np.uint16)
    nc = K // 32
    for T in range(2):
        for c in range(nc):
            chunk = t[(T * nc + c) * tb.CHUNK_ELEMS:(T * nc + c + 1) * tb.CHUNK_ELEMS]      # = the LDS image, piece by piece
            ref = _lds_image_row_major(w, T * 256, c, 32, 256)
            valid = np.repeat(np.arange(256) + T * 256 < N, 32)                               # 64-B LDS rows, row r at r * 32 elements
            assert np.array_equal(chunk[valid], ref[valid]), (T, c)
            assert not chunk[~valid].any()


def test_lds_image_of_the_128_tile_kernel_is_the_row_major_one():
    """64-deep steps of a 128-row tile (nt_stage_tiled): lane i of piece `seg` fetches the unit nt_stage fetches, by its index."""
    N, K = 200, 128
    w = (np.arange(N * K, dtype=np.int64) % 65521).astype(np.uint16).reshape(N, K)
    t = tb.tile_reference(torch.from_numpy(w.astype(np.int16))).numpy().astype(np.uint16)
    for n0 in (0, 128):
        for s in range(K // 64):
            ref = _lds_image_row_major(w, n0, s, 64, 128)
            img = np.zeros_like(ref)
            for seg in range(16):
                for lane in range(64):
                    row = seg * 8 + lane // 8
                    unit = (lane % 8) ^ swz64(row)
                    i = tb.tiled_index(n0 + row, s * 64 + unit * 8, K)
                    img[seg * 512 + lane * 8: seg * 512 + lane * 8 + 8] = t[i:i + 8]
            valid = np.repeat(np.arange(128) + n0 < N, 64)
            assert np.array_equal(img[valid], ref[valid]), (n0, s)
            assert not img[~valid].any()


def test_job_tiles_cover_the_padding_rows():
    assert tb.job_tiles(200, 96, True, False) == (256 // 64) * 2
    assert tb.job_tiles(128, 96, True, True) == (256 // 64) * (256 // 64)
    assert tb.job_tiles(128, 96, False, False) == 2 * 2
