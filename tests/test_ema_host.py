"""Host side of the EMA of the weights (config keys ema_decay / ema_warmup / ema_eval / load_ema): validation, the decay schedule,
the weight formed in double, the numpy model's bf16 rounding against torch, and the GPU test's bound checked on the model itself.
No GPU."""
import struct

import numpy as np
import pytest
import torch

from m3ae_amd import config
import ema_model as EM


# ---------------------------------------------------------------------------------------------------------------------------------
# config
# ---------------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_off_and_opt_in():
    cfg = config.tiny_config()
    assert cfg["ema_decay"] == 0.0 and cfg["ema_warmup"] is True and cfg["ema_eval"] is True and cfg["load_ema"] is False
    assert config.ema_decay({}) == 0.0


@pytest.mark.parametrize("v", [0.0, 0, 0.5, 0.9999, 1.0 - 2.0 ** -20])
def test_valid_decays(v):
    cfg = config.tiny_config(ema_decay=v)
    assert cfg["ema_decay"] == float(v) and type(cfg["ema_decay"]) is float


@pytest.mark.parametrize("v", [1.0, 1, 1.5, -0.1, -1e-9, True, False, "0.999", None, float("nan"), float("inf")])
def test_invalid_decays_raise(v):
    with pytest.raises(ValueError, match="ema_decay"):
        config.tiny_config(ema_decay=v)


@pytest.mark.parametrize("key", ["ema_warmup", "ema_eval", "load_ema"])
@pytest.mark.parametrize("v", [1, 0, "True", None, 0.5])
def test_the_switches_are_bools(key, v):
    with pytest.raises(ValueError, match=key):
        config.tiny_config(**{key: v})
    assert config.tiny_config(**{key: True})[key] is True and config.tiny_config(**{key: False})[key] is False


def test_the_keys_pass_through_the_command_line_grammar():
    cfg = config.parse_cli("with task_finetune_vqa_vqa_rad clip16 text_roberta ema_decay=0.999 ema_warmup=False ema_eval=False "
                           "load_ema=True".split())
    assert cfg["ema_decay"] == 0.999 and cfg["ema_warmup"] is False and cfg["ema_eval"] is False and cfg["load_ema"] is True
    with pytest.raises(ValueError, match="ema_decay"):
        config.parse_cli("with task_finetune_vqa_vqa_rad ema_decay=1.0".split())
    with pytest.raises(ValueError, match="load_ema"):
        config.parse_cli("with task_finetune_vqa_vqa_rad load_ema=yes".split())


# ---------------------------------------------------------------------------------------------------------------------------------
# schedule and weight
# ---------------------------------------------------------------------------------------------------------------------------------
def test_warmup_schedule_against_hand_computed_values():
    # (1 + t) / (10 + t) by hand: 2/11, 3/12, 90/99, 91/100; it reaches the cap 0.9 at t = 80 (81/90) and stays there
    hand = {1: 2.0 / 11.0, 2: 0.25, 79: 80.0 / 89.0, 80: 0.9, 81: 0.9, 89: 0.9, 90: 0.9}
    assert 90.0 / 99.0 > 0.9 and 91.0 / 100.0 > 0.9 and 80.0 / 89.0 < 0.9
    for t, want in hand.items():
        assert config.ema_decay_at(0.9, t, True) == want == EM.decay_at(0.9, t, True), t
        assert config.ema_decay_at(0.9, t, False) == 0.9
    assert [config.ema_weight(0.9, t, True) for t in (1, 2, 3)] == [float(np.float32(9.0 / 11.0)), 0.75, float(np.float32(9.0 / 13.0))]
    assert config.ema_weight(0.5, 7, False) == 0.5


def test_the_weight_is_formed_in_double_and_rounded_once():
    w = config.ema_weight(0.9999, 10 ** 6, True)
    want = np.float32(1e-4)
    in_fp32 = np.float32(1.0) - np.float32(0.9999)
    assert struct.pack("f", w) == want.tobytes()
    assert in_fp32 != want and abs(float(in_fp32) - 1e-4) > 1e-8          # what the kernel must never compute: 3e-4 relative off
    for decay, t, warm in ((0.9999, 5, True), (0.999, 3, False), (0.9, 2, True)):
        assert struct.pack("f", config.ema_weight(decay, t, warm)) == EM.weight(decay, t, warm).tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------
def test_model_bf16_rounding_is_torchs_at_the_edges():
    x = np.concatenate([EM.bf16_edge_values(), EM.inputs(4096, 7)[0]])
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = EM.bf16_bits(x)
    assert np.array_equal(got, want), [(hex(a), hex(b), hex(c)) for a, b, c in zip(x.view(np.uint32), got, want) if b != c][:8]
    edge = dict(zip(EM.bf16_edge_values().view(np.uint32).tolist(), EM.bf16_bits(EM.bf16_edge_values()).tolist()))
    assert edge[0x3F808000] == 0x3F80 and edge[0x3F818000] == 0x3F82            # ties go to the even neighbour
    assert edge[0x80000000] == 0x8000 and edge[0x00008000] == 0x0000 and edge[0x00018000] == 0x0002
    assert edge[0x7F7FFFFF] == 0x7F80 and edge[0x7F7F7FFF] == 0x7F7F and edge[0xFF800000] == 0xFF80


@pytest.mark.parametrize("n", EM.SIZES)
def test_the_model_sits_inside_the_bound_on_the_gpu_tests_inputs(n):
    """The reference alone against exact float64, on the inputs and weights tests/test_gpu_ema.py uses: a bound the model missed
    would say nothing about the kernel."""
    p, e = EM.inputs(n, seed=n % 1000)
    assert np.isfinite(p).all() and (np.abs(p) >= np.float32(9e-7)).all() and (np.abs(p) <= np.float32(1.1e3)).all()
    assert (p > 0).any() and (p < 0).any()
    for w in EM.WEIGHTS:
        got = EM.update(p, e, w).astype(np.float64)
        err, lim = np.abs(got - EM.exact(p, e, w)), EM.bound(p, e, w)
        assert (err <= lim).all(), (float(w), float((err / lim).max()))
        if w == 0:
            assert np.array_equal(got.astype(np.float32).view(np.uint32), e.view(np.uint32))
        assert (np.abs(got[got != 0]) >= 2.0 ** -100).all()            # (the bound has no absolute term: nothing near the subnormals)
    same = EM.update(p, p, np.float32(0.5))
    assert np.array_equal(same.view(np.uint32), p.view(np.uint32))


def test_accumulated_budget_reduces_to_the_one_step_bound():
    p, e = EM.inputs(1028, 3)
    w = np.float32(0.5)
    E, B = EM.accumulate([e, p], [w])
    assert np.array_equal(E, EM.exact(p, e, w)) and np.allclose(B, EM.bound(p, e, w), rtol=1e-12, atol=0)
    # three model updates stay inside the three-step budget
    snaps = [e] + [EM.inputs(1028, 10 + k)[0] for k in range(3)]
    ws = [EM.weight(0.9, t, True) for t in (1, 2, 3)]
    got = e
    for P, wk in zip(snaps[1:], ws):
        got = EM.update(P, got, wk)
    E, B = EM.accumulate(snaps, ws)
    assert (np.abs(got.astype(np.float64) - E) <= B).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the store on the host: which calls a step makes, the counter, the state dict -- the library replaced by a recorder
# ---------------------------------------------------------------------------------------------------------------------------------
class Recording:
    """Stands in for the loaded library: records (name, args) of every call and returns 0."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


def _cpu_store(**over):
    """A ParamStore on the CPU in fp32 (no shadow: its construction makes no library call)."""
    from m3ae_amd.param_store import ParamStore
    torch.manual_seed(0)
    mod = torch.nn.Sequential(torch.nn.Linear(5, 3), torch.nn.LayerNorm(3), torch.nn.Linear(3, 70))
    return ParamStore(mod, config.tiny_config(compute_dtype="fp32", **over), "cpu", torch.float32), mod


def _recorder(monkeypatch):
    from m3ae_amd import _lib, ops
    rec = Recording()
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(_lib, "lib", lambda: _lib._lib)
    return rec


def _val(x):
    return getattr(x, "value", x)


def test_key_off_a_step_makes_no_ema_call_and_allocates_nothing(monkeypatch):
    rec = _recorder(monkeypatch)
    st, _ = _cpu_store()
    hyper = st.begin_update(max_steps=10, lr_factor=1.0)
    assert "ema_w" not in hyper and st.ema is None and st.ema_updates == 0
    for gi in range(6):
        a, b = st.segments[gi]
        st.update_range(a, min(b, st.trainable_end), gi, hyper)
    assert rec.calls and {name for name, _ in rec.calls} == {"m3ae_adamw"}
    with pytest.raises(RuntimeError, match="no average"):
        with st.ema_weights():
            pass


@pytest.mark.parametrize("rule", ["adamw", "adam", "sgd"])
def test_key_on_every_optimizer_launch_is_followed_by_the_update_over_the_same_range(monkeypatch, rule):
    rec = _recorder(monkeypatch)
    st, _ = _cpu_store(ema_decay=0.9, optim_type=rule)
    before = st.flat[:st.trainable_end].clone()
    hyper = st.begin_update(max_steps=10, lr_factor=1.0)
    assert torch.equal(st.ema, before) and st.ema.data_ptr() != st.flat.data_ptr()      # a copy of the weights before the step
    assert st.ema_updates == 1 and struct.pack("f", hyper["ema_w"]) == np.float32(9.0 / 11.0).tobytes()
    ranges = [(a, min(b, st.trainable_end)) for a, b in st.segments[:6] if min(b, st.trainable_end) > a]
    for gi in range(6):
        a, b = st.segments[gi]
        st.update_range(a, min(b, st.trainable_end), gi, hyper)
    assert [name for name, _ in rec.calls] == ["m3ae_" + rule, "m3ae_ema_update"] * len(ranges)
    for (a, b), (_, opt_args), (_, args) in zip(ranges, rec.calls[0::2], rec.calls[1::2]):
        p, ema, n, w, clip, stream = args
        assert _val(p) == st.flat.data_ptr() + 4 * a == _val(opt_args[0]) and _val(ema) == st.ema.data_ptr() + 4 * a
        assert n == b - a and w == hyper["ema_w"] and clip is None
    # the second and third ticks of the warmup, and the count
    assert [struct.pack("f", st.begin_update(max_steps=10, lr_factor=1.0)["ema_w"]) for _ in range(2)] == \
        [np.float32(0.75).tobytes(), np.float32(9.0 / 13.0).tobytes()]
    assert st.ema_updates == 3 and st.step_count == 3


def test_the_update_takes_the_steps_clip_record(monkeypatch):
    from m3ae_amd import gradnorm
    rec = _recorder(monkeypatch)
    monkeypatch.setattr(gradnorm, "clip_finalize", lambda *a: None)
    st, _ = _cpu_store(ema_decay=0.5, ema_warmup=False, gradient_clip_val=1.0)

    class Sums:
        def run(self, *a):
            return None
    st._sums = Sums()
    st.update_apply(st.begin_update(max_steps=10, lr_factor=1.0))
    pairs = list(zip(rec.calls[0::2], rec.calls[1::2]))
    assert pairs and all(a[0] == "m3ae_adamw_clip" and b[0] == "m3ae_ema_update" for a, b in pairs)
    for (_, opt_args), (_, args) in pairs:
        assert _val(args[4]) == st._clip_record.data_ptr() == _val(opt_args[-2]) and args[3] == 0.5


def test_state_dict_round_trip_and_refusals_on_the_host(monkeypatch):
    _recorder(monkeypatch)
    st, mod = _cpu_store(ema_decay=0.5)
    with pytest.raises(RuntimeError, match="no average"):
        st.ema_state_dict()
    st.begin_update(max_steps=10, lr_factor=1.0)
    st.ema.add_(1.0)
    sd = st.ema_state_dict()
    assert set(sd) == {n for n, _ in mod.named_parameters()}
    for n, p in mod.named_parameters():
        assert sd[n].shape == p.shape and sd[n].dtype == torch.float32 and torch.equal(sd[n], p.detach() + 1.0), n
    other, _ = _cpu_store(ema_decay=0.5)
    other.load_ema_state_dict(sd, 7)
    back = other.ema_state_dict()                                 # (the ALIGN padding between parameters is in no state dict)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd) and other.ema_updates == 7
    with pytest.raises(ValueError, match="no entry"):
        other.load_ema_state_dict({k: v for k, v in sd.items() if k != "0.bias"}, 1)
    with pytest.raises(ValueError, match="shape"):
        other.load_ema_state_dict(dict(sd, **{"0.bias": torch.zeros(4)}), 1)
    back = other.ema_state_dict()
    assert all(torch.equal(back[k], sd[k]) for k in sd) and other.ema_updates == 7      # a refused load writes nothing
