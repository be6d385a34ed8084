"""The numpy model of the greedy-search kernels (tests/greedy_model.py) against CPU torch: its argmax rule against torch.argmax on
fp32 and bf16 rows (ties, signed zeros, infinities, NaNs), its search against a transcription of Decoder.search_path's loop and
post-processing on scripted tokens.  The GPU tests (tests/test_gpu_greedy.py) then hold the kernels to this model exactly.  Also
the host-side surface of the feature: the declared symbols, the config key, the argument checks that need no GPU."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import abi_header
import greedy_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32_from_bits(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


POS_NAN, NEG_NAN, NEG_NAN_PAYLOAD = 0x7fc00000, 0xffc00000, 0xffc10000   # all three survive a cut to bf16 (low 16 bits zero)


def edge_rows(V, rng):
    """Rows [n, V] of fp32 values that are also bf16 values, with the tie / zero / infinity / NaN cases of the argmax rule."""
    base = torch.from_numpy(rng.standard_normal(V).astype(np.float32)).to(torch.bfloat16).float().numpy()
    rows = {}
    rows["random"] = base.copy()
    rows["all_equal"] = np.full(V, 0.75, dtype=np.float32)
    r = base.copy(); r[[V // 3, V - 2]] = 9.0; rows["max_twice"] = r
    r = np.full(V, -0.0, dtype=np.float32); r[V // 2] = 0.0; rows["zeros_minus_first"] = r            # equal: column 0
    r = torch.from_numpy(-np.abs(base) - 1.0).to(torch.bfloat16).float().numpy(); r[3] = -0.0; r[V - 1] = 0.0; rows["zeros_among_negatives"] = r          # -0 == +0: column 3
    rows["all_minus_inf"] = np.full(V, -np.inf, dtype=np.float32)
    r = base.copy(); r[V - 1] = np.inf; r[2] = f32_from_bits([POS_NAN])[0]; rows["one_nan_and_inf"] = r
    r = base.copy(); r[V // 2] = f32_from_bits([NEG_NAN])[0]; rows["one_negative_nan"] = r
    r = base.copy(); r[[4, V // 2, V - 1]] = f32_from_bits([NEG_NAN_PAYLOAD, POS_NAN, NEG_NAN]); r[1] = np.inf; rows["nans_both_signs"] = r
    r = base.copy(); r[[5, 6]] = f32_from_bits([POS_NAN, NEG_NAN]); rows["nans_positive_first"] = r
    return rows


def as_bf16(x):
    """float32 array of bf16-representable values -> torch bf16 tensor with the same bits (NaN signs and payloads included)."""
    hi = (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
    return torch.from_numpy(hi.copy()).view(torch.bfloat16)


@pytest.mark.parametrize("V", [9, 257, 4099])
def test_argmax_rule_is_torch_argmax(V):
    rows = edge_rows(V, np.random.default_rng(V))
    x = np.stack(list(rows.values()))
    want = dict(all_equal=0, max_twice=V // 3, zeros_minus_first=0, zeros_among_negatives=3, all_minus_inf=0, one_nan_and_inf=2,
                one_negative_nan=V // 2, nans_both_signs=4, nans_positive_first=5)
    got = M.argmax_rule(x)
    for i, name in enumerate(rows):
        if name in want:
            assert got[i] == want[name], name
    assert got.tolist() == torch.argmax(torch.from_numpy(x), dim=-1).tolist()
    xb = as_bf16(x)
    assert np.array_equal(xb.float().numpy().view(np.uint32), x.view(np.uint32))     # the widening is exact, NaN bits included
    assert got.tolist() == torch.argmax(xb, dim=-1).tolist()
    # wide random rows in either dtype (bf16: ties at the maximum occur by themselves)
    y = np.random.default_rng(V + 1).standard_normal((64, V)).astype(np.float32)
    assert M.argmax_rule(y).tolist() == torch.argmax(torch.from_numpy(y), dim=-1).tolist()
    yb = torch.from_numpy(y).to(torch.bfloat16)
    assert M.argmax_rule(yb.float().numpy()).tolist() == torch.argmax(yb, dim=-1).tolist()


@pytest.mark.parametrize("chunk", [0, 256, 1000])
def test_chunk_keys_fold_to_the_row_argmax(chunk):
    x = np.stack(list(edge_rows(4099, np.random.default_rng(3)).values()))
    k = M.chunk_keys(x, chunk)
    assert k.shape == (x.shape[0], -(-4099 // (chunk or M.DEF_CHUNK)))
    assert M.tokens_of(k).tolist() == M.argmax_rule(x).tolist()


def host_search(script, cls_id, sep_id, eos_id, pad_id):
    """Decoder.search_path's loop and post-processing (m3ae_amd/modules/m3ae_decoder.py) in torch CPU ops, the argmax of step
    `step` replaced by script[step]."""
    max_len, B = script.shape
    seq = torch.full((B, 1), cls_id, dtype=torch.long)
    finished = torch.zeros(B, dtype=torch.bool)
    fed = []
    for step in range(max_len):
        fed.append(seq[:, -1].clone())
        nxt = torch.from_numpy(script[step])
        hit = nxt == sep_id
        if eos_id is not None:
            hit = hit | (nxt == eos_id)
        finished |= hit
        seq = torch.cat([seq, nxt[:, None]], dim=1)
        if bool(finished.all()):
            break
    seq = seq[:, 1:]
    special = seq == sep_id
    if eos_id is not None:
        special = special | (seq == eos_id)
    after = (special.long().cumsum(1) - special.long()) > 0
    seq = torch.where(after, torch.full_like(seq, pad_id), seq)
    return torch.nn.functional.pad(seq, (0, max_len - seq.shape[1]), value=pad_id), step + 1, fed


@pytest.mark.parametrize("eos_id", [None, M.EOS])
@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("kind", M.SCRIPT_KINDS)
def test_model_search_matches_the_host_loop(kind, B, eos_id):
    sc = M.script(kind, B)
    want, steps, fed = host_search(sc, M.CLS, M.SEP, eos_id, M.PAD)
    fed_model = []
    st, n = M.search(sc, M.SCRIPT_V, M.CLS, M.SEP, eos_id, M.PAD,
                     on_step=lambda s, pos: fed_model.append(s.last_tok.copy()))
    assert n == steps and st.err[0] == 0
    assert np.array_equal(st.seq, want.numpy())
    # the token fed to step pos + 1 is the raw argmax of step pos, for finished rows too
    assert all(np.array_equal(a, b.numpy()) for a, b in zip([np.full(B, M.CLS)] + fed_model, fed))
    # steps after every row has finished change nothing in the result
    full, n_full = M.search(sc, M.SCRIPT_V, M.CLS, M.SEP, eos_id, M.PAD, stop_early=False)
    assert n_full == M.SCRIPT_LEN and np.array_equal(full.seq, st.seq) and np.array_equal(full.len, st.len)
    # len = tokens up to and with the first end token, max_len for a row that never finished
    for r in range(B):
        ends = [p for p in range(M.SCRIPT_LEN) if sc[p, r] == M.SEP or (eos_id is not None and sc[p, r] == eos_id)]
        assert full.len[r] == (ends[0] + 1 if ends else M.SCRIPT_LEN)
        assert full.finished[r] == (1 if ends else 0)


def test_scripts_cover_the_cases():
    """[SEP] at step 0, a batch that never finishes, rows finishing at different steps next to rows that never do, a second [SEP]
    after the first, and rows that end only when eos_id is given."""
    assert (M.script("sep_at_0", 3)[0] == M.SEP).all()
    assert M.search(M.script("sep_at_0", 3), M.SCRIPT_V)[1] == 1
    assert M.search(M.script("never", 3), M.SCRIPT_V)[0].finished.sum() == 0
    st, n = M.search(M.script("staggered", 70), M.SCRIPT_V)
    assert n == M.SCRIPT_LEN and 0 < st.finished.sum() < 70 and len(set(st.len.tolist())) > 3
    sc = M.script("second_sep", 3)
    assert all((sc[:, r] == M.SEP).sum() == 3 for r in range(3))
    a, b = M.search(M.script("eos_rows", 70), M.SCRIPT_V)[0], M.search(M.script("eos_rows", 70), M.SCRIPT_V, eos_id=M.EOS)[0]
    assert a.finished.sum() == 35 and b.finished.sum() == 70


def test_model_step_flags_a_token_outside_the_vocabulary():
    st = M.State(3, 4)
    M.step(st, [5, 300, -1], 0, 300, M.SEP, None, M.PAD)
    assert st.err[0] == 1 and st.last_tok.tolist() == [5, 0, 0] and st.seq[:, 0].tolist() == [5, 0, 0]


def test_header_binding_and_stub_agree_on_the_greedy_symbols():
    from m3ae_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_integration_stub as gen
    names = {"m3ae_greedy_workspace_bytes", "m3ae_greedy_argmax", "m3ae_greedy_step"}
    assert {n for n in abi_header.prototypes() if n.startswith("m3ae_greedy_")} == names
    assert {n for n in _lib.EXPORTS if n.startswith("m3ae_greedy_")} == names == set(gen.GREEDY_ENTRIES)
    # (parameter lists against argument lists, and the stub's sections in INTEGRATION.md: tests/test_host_logic.py, for the whole ABI)
    # sizing needs no GPU: 8 bytes per (row, chunk); 0 for a shape the launch would reject
    L = _lib.lib()
    assert L.m3ae_greedy_workspace_bytes(5, 30522, 0) == 5 * 15 * 8
    assert L.m3ae_greedy_workspace_bytes(2, 1001, 256) == 2 * 4 * 8
    assert L.m3ae_greedy_workspace_bytes(0, 9, 0) == L.m3ae_greedy_workspace_bytes(1, 9, 32) == L.m3ae_greedy_workspace_bytes(1, 2 ** 31, 0) == 0


def test_config_key_and_signatures():
    from m3ae_amd import config
    from m3ae_amd.modules.m3ae_decoder import Decoder, DecoderModel
    assert config.DEFAULTS["decoder_search"] == "host"
    assert config.parse_cli(["with", "decoder_search=device"])["decoder_search"] == "device"
    assert config.tiny_config(decoder_search="device")["decoder_search"] == "device"
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError, match="decoder_search"):
            config.tiny_config(decoder_search=bad)
    with pytest.raises(ValueError, match="decoder_search"):
        config.parse_cli(["with", "decoder_search=Device"])
    sig = inspect.signature(Decoder.search_path)
    assert sig.parameters["search"].default == "host" and sig.parameters["lookahead"].default == 2
    sig = inspect.signature(Decoder.search_path_async)
    assert sig.parameters["lookahead"].default == 2 and sig.parameters["chunk"].default == 0
    assert callable(DecoderModel.generate) and callable(DecoderModel.generate_async)


def test_search_path_argument_errors_need_no_gpu():
    from m3ae_amd.modules.m3ae_decoder import Decoder
    d = Decoder(num_layers=1, d_model=16, num_heads=2, d_ff=32, dropout=0.0, max_len=4, target_vocab_size=20)
    feats = torch.zeros(2, 2, 16)
    with pytest.raises(ValueError, match="use_cache"):
        d.search_path(feats, search="device", use_cache=False)
    with pytest.raises(ValueError, match="search must be"):
        d.search_path(feats, search="gpu")
    with pytest.raises(ValueError, match="lookahead"):
        d.search_path_async(feats, lookahead=0)


def test_greedy_ops_reject_cpu_tensors():
    from m3ae_amd import _lib, ops
    with pytest.raises(_lib.M3AEHipError):
        ops.greedy_argmax(torch.zeros(4, 9))
    with pytest.raises(_lib.M3AEHipError):
        ops.greedy_step(None, torch.zeros(1, 1, dtype=torch.int64), 9, 0, 102, None, 0)
