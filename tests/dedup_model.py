"""Numpy model of the two kernels behind a de-duplicated image batch (csrc/samples.hip), bit for bit:

  m3ae_expand_samples    out[b] = x[index[b]]
  m3ae_segment_sum_rows  d_x[u] = the float32 sum of d_out[m] over the samples m of image u, added in ascending sample order
                         starting FROM the first member (not from zero), then rounded once to the storage dtype
                         (bf16: round-to-nearest-even).

bf16 arrays are uint16 bit patterns here; `to_torch` / `from_torch` convert."""
import numpy as np


def bf16_round(x):
    """float32 array -> bf16 bits (uint16), round-to-nearest-even (finite inputs)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def groups_of(index, n_images=None):
    """(offsets [U + 1], members [B]) of an index list: per image its samples in ascending order."""
    index = np.asarray(index, dtype=np.int64)
    U = int(index.max()) + 1 if n_images is None else n_images
    members = [np.flatnonzero(index == u) for u in range(U)]
    offsets = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
    return offsets, np.concatenate(members).astype(np.int64)


def expand(x, index):
    return x[np.asarray(index, dtype=np.int64)]


def segment_sum(d_out, offsets, members, bf16):
    """d_out: [B, R] float32, or uint16 bf16 bits with bf16=True.  Returns [U, R] in the same representation."""
    d = bf16_to_f32(d_out) if bf16 else np.asarray(d_out, dtype=np.float32)
    U = len(offsets) - 1
    out = np.zeros((U,) + d.shape[1:], dtype=np.float32)
    for u in range(U):
        ms = members[offsets[u]:offsets[u + 1]]
        if len(ms) == 0:
            continue
        acc = d[ms[0]].copy()
        for m in ms[1:]:
            acc = (acc + d[m]).astype(np.float32)
        out[u] = acc
    return bf16_round(out) if bf16 else out


def segment_sum_f64(d_out, offsets, members, bf16):
    """The same sum in float64 (exact for these sizes up to one final rounding), as float64."""
    d = (bf16_to_f32(d_out) if bf16 else np.asarray(d_out, dtype=np.float32)).astype(np.float64)
    return np.stack([d[members[offsets[u]:offsets[u + 1]]].sum(axis=0) for u in range(len(offsets) - 1)])


def to_torch(a, bf16):
    import torch
    if not bf16:
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def from_torch(t):
    import torch
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()
