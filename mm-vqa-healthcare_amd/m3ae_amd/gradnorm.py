"""Host side of csrc/gradnorm.hip: the piece table of m3ae_sumsq_segments and the device buffers of one segment table.

A segment table is a sorted, non-overlapping list of [begin, end) element ranges of one fp32 buffer (ParamStore: one per trainable
parameter, the ALIGN padding between them in no segment).  `piece_table` cuts every segment into pieces of at most PIECE elements
at fixed positions (begin + k * PIECE), so the word embedding (38.6 M elements, 1178 pieces) and a bias row (one piece) go
through the same launch chain; the kernel runs one workgroup per piece and one wave per segment folds that segment's pieces in
ascending order.  The sums are a function of (buffer, table) alone -- no atomics -- so deterministic mode uses the same path."""
import ctypes as C

import numpy as np
import torch

from . import _lib

PIECE = 32768   # elements per piece: 128 KiB of fp32, 32 16-byte loads per lane of a 256-lane workgroup


def piece_table(segments, piece=PIECE):
    """(pieces [npieces, 2] int64 {begin, end}, seg_ptr [nseg + 1] int64) of `segments` = [(begin, end), ...]: every element of
    every segment lies in exactly one piece, no piece crosses a segment, a segment's pieces are adjacent and ascending; an empty
    segment owns no piece."""
    if piece <= 0:
        raise ValueError("piece must be positive")
    pieces, ptr, last = [], [0], 0
    for b, e in segments:
        b, e = int(b), int(e)
        if b < last or e < b:
            raise ValueError(f"segments must be sorted, non-overlapping [begin, end) ranges: ({b}, {e}) after end {last}")
        last = e
        for p in range(b, e, piece):
            pieces.append((p, min(p + piece, e)))
        ptr.append(len(pieces))
    return np.asarray(pieces, dtype=np.int64).reshape(-1, 2), np.asarray(ptr, dtype=np.int64)


class SegmentSums:
    """Device tables, workspace and output of m3ae_sumsq_segments for one segment table of an n-element fp32 buffer."""

    def __init__(self, segments, n, device, piece=PIECE):
        pieces, ptr = piece_table(segments, piece)
        if len(pieces) and int(pieces[-1, 1]) > n:
            raise ValueError(f"segment end {int(pieces[-1, 1])} is past the buffer ({n} elements)")
        self.n, self.nseg, self.npieces = int(n), len(ptr) - 1, len(pieces)
        if self.nseg == 0:
            raise ValueError("empty segment table")
        self.pieces = torch.from_numpy(pieces if len(pieces) else np.zeros((1, 2), np.int64)).to(device)
        self.seg_ptr = torch.from_numpy(ptr).to(device)
        self.ws_bytes = int(_lib.lib().m3ae_sumsq_workspace_bytes(self.npieces))
        self.workspace = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=device)
        self.out = torch.zeros(self.nseg, dtype=torch.float64, device=device)

    def run(self, x, stream):
        """out[s] = sum of x[i]^2 over segment s (double), on `stream`; x: the fp32 buffer the table was built for."""
        assert x.dtype == torch.float32 and x.numel() == self.n
        _lib.check(_lib.lib().m3ae_sumsq_segments(C.c_void_p(x.data_ptr()), self.n, C.c_void_p(self.pieces.data_ptr()), self.npieces,
                                                  C.c_void_p(self.seg_ptr.data_ptr()), self.nseg, C.c_void_p(self.out.data_ptr()),
                                                  C.c_void_p(self.workspace.data_ptr()), self.ws_bytes, stream),
                   "m3ae_sumsq_segments")
        return self.out


def clip_finalize(seg_sumsq, grad_scale, max_norm, record, stream):
    """m3ae_clip_finalize over the doubles of a SegmentSums.run: {norm, coef, skip, counters} into `record` (_lib.CLIP_* words)."""
    _lib.check(_lib.lib().m3ae_clip_finalize(C.c_void_p(seg_sumsq.data_ptr()), seg_sumsq.numel(), float(grad_scale), float(max_norm),
                                             C.c_void_p(record.data_ptr()), stream), "m3ae_clip_finalize")
