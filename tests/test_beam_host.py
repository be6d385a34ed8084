"""The numpy model of the beam-search kernels (tests/beam_model.py) against the CPU oracle's `t5_beam_search` on scripted logits
L(t, r, :) = T1[t, r, :] + T2[last_token(r), :] -- a form both the oracle and a device loop can evaluate.  The GPU tests
(tests/test_gpu_beam.py) then hold the kernels to this model array by array."""
import itertools

import numpy as np
import pytest
import torch

import beam_model as M


@pytest.mark.parametrize("case", list(M.SCRIPTED), ids=lambda c: "V{}-nb{}-L{}-eos{}".format(*c))
def test_model_search_matches_oracle(monkeypatch, case):
    """Every scripted case is valid (live top-(2 nb + 1) gaps >= 2 tau at every step, asserted) and the model's sequences equal the
    oracle's for both length conventions and both length penalties."""
    V, nb, ml, eos_bias = case
    seed = M.SCRIPTED[case]
    _, worst = M.validate(case, seed)
    assert worst >= 1.0, f"seed {seed} of {case}: minimum live gap is {worst:.3f} x 2 tau -- pick another seed"
    T1, T2 = M.tables(V, nb, ml, eos_bias, M.SCRIPTED_B, seed)
    for len_offset, lp in itertools.product((0, 1), (1.0, 0.7)):
        st = M.search(T1, T2, M.SCRIPTED_B, nb, ml, length_penalty=lp, len_offset=len_offset)
        ref = M.oracle_search(monkeypatch, T1, T2, M.SCRIPTED_B, nb, ml, lp, len_offset)
        assert st.err[0] == 0
        assert M.trimmed(st.seq, st.len, ml).tolist() == ref.tolist(), (case, len_offset, lp)
        # steps after every sample is done change nothing in the result
        full = M.search(T1, T2, M.SCRIPTED_B, nb, ml, length_penalty=lp, len_offset=len_offset, stop_early=False)
        assert np.array_equal(full.seq, st.seq) and np.array_equal(full.len, st.len)


def test_scripted_cases_cover_the_scorer_events():
    """Over the set: an EOS candidate at rank >= nb, samples finishing at different steps of one search, samples still open at
    max_length, and a hypothesis list overflowing nb within one step."""
    seen, spread = set(), False
    for case, seed in M.SCRIPTED.items():
        st, _ = M.validate(case, seed)
        seen |= {e for e in st.events if isinstance(e, str)}
        spread = spread or len({e for e in st.events if not isinstance(e, str)}) >= 2
    assert seen >= {"eos_low_rank", "overflow", "open_at_end"}, seen
    assert spread


def test_model_topk_order_key_and_stable_hypothesis_list():
    """Ties come out in ascending flat index; the hypothesis list keeps a new entry after equal scores and cuts to nb."""
    x = np.zeros((4, 9), dtype=np.float32)
    s, i = M.topk(x, np.zeros(4, dtype=np.float32), 2, 2)
    assert i.tolist() == [[0, 1, 2, 3]] * 2 and np.all(s == s[0, 0])
    st = M.State(1, 2, 4)
    for k, score in enumerate((-1.0, -1.0, -0.5, -1.0)):
        st._push(0, score, np.array([0, 10 + k, 0, 0]), 2)
    assert st.hyp_score[0].tolist() == [-0.5, -1.0] and st.hyp_tok[0, :, 1].tolist() == [12, 10] and st.n_hyp[0] == 2
    assert "overflow" in st.events


def test_config_and_generate_expose_the_mode():
    import inspect
    from m3ae_amd import config
    from m3ae_amd.modules.t5 import T5ForConditionalGeneration
    assert config.DEFAULTS["t5_beam_search"] == "host"
    assert config.parse_cli(["with", "t5_beam_search=device"])["t5_beam_search"] == "device"
    sig = inspect.signature(T5ForConditionalGeneration.generate)
    assert sig.parameters["beam_search"].default == "host"
    assert inspect.signature(T5ForConditionalGeneration.generate_async).parameters["lookahead"].default == 2


def test_beam_ops_reject_cpu_tensors():
    from m3ae_amd import _lib, ops
    with pytest.raises(_lib.M3AEHipError):
        ops.beam_topk(torch.zeros(4, 9), torch.zeros(4), 1, 4)
