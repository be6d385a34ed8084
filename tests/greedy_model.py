"""numpy model of the greedy-search kernels of csrc/greedy.hip (include/m3ae_hip.h: m3ae_greedy_argmax, m3ae_greedy_step): the order
key and its per-chunk maxima, the same fixed-size state arrays and the same update per step.  Also the scripted token sequences
the CPU and GPU greedy tests share.  Logits are float32 arrays throughout: bf16 values widen to fp32 exactly."""
import numpy as np

U32 = np.uint32
DEF_CHUNK = 2048


def keys_of(x):
    """x float32 [R, V] -> uint64 [R, V]: (monotone image of the value) << 32 | (2^32 - 1 - column); -0 counts as +0 and every NaN
    takes the top image."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(U32).copy()
    nan = (u & U32(0x7fffffff)) > U32(0x7f800000)
    u[u == U32(0x80000000)] = 0
    o = np.where(u & U32(0x80000000), ~u, u | U32(0x80000000)).astype(U32)
    o[nan] = U32(0xffffffff)
    col = (U32(0xffffffff) - np.arange(x.shape[1], dtype=U32))[None, :]
    return (o.astype(np.uint64) << np.uint64(32)) | col.astype(np.uint64)


def chunk_keys(x, chunk=0):
    """The keys buffer m3ae_greedy_argmax writes: uint64 [R, ceil(V / chunk)], the maximum key of every vocabulary chunk."""
    chunk = chunk or DEF_CHUNK
    k = keys_of(x)
    return np.stack([k[:, v0:v0 + chunk].max(axis=1) for v0 in range(0, x.shape[1], chunk)], axis=1)


def tokens_of(keys):
    """uint64 [R, chunks] -> int64 [R]: the column the row's greatest key carries."""
    return (np.uint64(0xffffffff) - (keys.max(axis=1) & np.uint64(0xffffffff))).astype(np.int64)


def argmax_rule(x):
    """torch.argmax(x, -1) for float32 [R, V]: greatest value, lowest column among equals (+0 == -0), the first NaN above all."""
    return tokens_of(keys_of(x))


class State:
    """The arrays of ops.GreedyState."""

    def __init__(self, B, max_len, cls_id=101, pad_id=0):
        self.B, self.max_len = B, max_len
        self.seq = np.full((B, max_len), pad_id, dtype=np.int64)
        self.len = np.full(B, max_len, dtype=np.int64)
        self.err = np.zeros(1, dtype=np.int64)
        self.last_tok = np.full(B, cls_id, dtype=np.int64)
        self.finished = np.zeros(B, dtype=np.int32)
        self.open_count = np.zeros(max_len, dtype=np.int32)


def step(st, toks, pos, V, sep_id, eos_id, pad_id):
    """One m3ae_greedy_step: toks int64 [B] are the decoded columns of the rows' keys."""
    toks = np.asarray(toks, dtype=np.int64).copy()
    bad = (toks < 0) | (toks >= V)
    if bad.any():
        st.err[0] = 1
        toks[bad] = 0
    st.last_tok[:] = toks
    for r in range(st.B):
        if st.finished[r]:
            st.seq[r, pos] = pad_id
            continue
        st.seq[r, pos] = toks[r]
        if toks[r] == sep_id or (eos_id is not None and eos_id >= 0 and toks[r] == eos_id):
            st.finished[r] = 1
            st.len[r] = pos + 1
    st.open_count[pos] = int((st.finished == 0).sum())


def search(token_script, V, cls_id=101, sep_id=102, eos_id=None, pad_id=0, stop_early=True, on_step=None):
    """token_script int64 [max_len, B]: the argmax of step `pos` for every row.  Returns the final State and the steps run."""
    max_len, B = token_script.shape
    st = State(B, max_len, cls_id, pad_id)
    steps = 0
    for pos in range(max_len):
        step(st, token_script[pos], pos, V, sep_id, eos_id, pad_id)
        steps += 1
        if on_step is not None:
            on_step(st, pos)
        if stop_early and st.open_count[pos] == 0:
            break
    return st, steps


# ---- the scripted cases the CPU and GPU greedy tests share -------------------------------------------------------------------------
SCRIPT_V, SCRIPT_LEN, SEP, EOS, CLS, PAD = 300, 12, 102, 7, 101, 0
SCRIPT_KINDS = ("sep_at_0", "never", "staggered", "second_sep", "eos_rows")


def script(kind, B, seed=0):
    """int64 [SCRIPT_LEN, B] tokens in [0, SCRIPT_V).  Rows keep emitting arbitrary tokens after they have finished (the host loop
    feeds them back all the same).  "eos_rows": odd rows end with EOS instead of [SEP] -- they finish only when eos_id is given."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, SCRIPT_V, size=(SCRIPT_LEN, B)).astype(np.int64)
    t[(t == SEP) | (t == EOS)] = 5
    if kind == "sep_at_0":
        t[0, :] = SEP
    elif kind in ("staggered", "second_sep", "eos_rows"):
        for r in range(B):
            if kind == "staggered" and r % 4 == 3:
                continue                       # this row never finishes
            f = 1 + (5 * r) % (SCRIPT_LEN - 3)
            t[f, r] = EOS if (kind == "eos_rows" and r % 2) else SEP
            if kind == "second_sep":
                t[f + 2, r] = SEP
                t[SCRIPT_LEN - 1, r] = SEP
    elif kind != "never":
        raise KeyError(kind)
    return t


def keys_for_tokens(toks, V, nch=3):
    """A keys buffer uint64 [B, nch] whose row maxima decode to `toks`: the winner sits in chunk slot r % nch, the other slots hold
    keys of lower values and other columns."""
    B = len(toks)
    k = np.empty((B, nch), dtype=np.uint64)
    for r in range(B):
        for c in range(nch):
            k[r, c] = (np.uint64(0x80000000 + 7 * c) << np.uint64(32)) | np.uint64(0xffffffff - ((int(toks[r]) + 1 + c) % V))
        k[r, r % nch] = (np.uint64(0xc0000000) << np.uint64(32)) | np.uint64(0xffffffff - int(toks[r]))
    return k
