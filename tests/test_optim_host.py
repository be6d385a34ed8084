"""optim_type (adamw | adam | sgd), the part that needs no GPU: the float32 models of the Adam and SGD kernels against torch.optim on
the CPU, the config key and its validator, the C ABI additions (header, ctypes binding, built library and INTEGRATION.md stub
agree; ABI number unchanged), the argument checks that come before any launch, and the host-side dispatch of ParamStore, the
Flat* optimizers, FlatGradReducer and GraphedStep (no library call is made)."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_header
from m3ae_amd import _lib, config
import optim_model as OM

OPTIM_ENTRIES = ("m3ae_adam", "m3ae_adam_clip", "m3ae_sgd", "m3ae_sgd_clip")
RTOL, ATOL = 1e-5, 1e-6      # the bound tests/test_gpu_ops.py::test_adamw_matches_hf_semantics holds m3ae_adamw to
N, STEPS, GRAD_SCALE = 4096, 5, 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the models against torch.optim
# ---------------------------------------------------------------------------------------------------------------------------------
def _worst(got, want):
    """max of |got - want| / (ATOL + RTOL * |want|): <= 1 is np.allclose(got, want, RTOL, ATOL)."""
    return float(np.max(np.abs(got.astype(np.float64) - want) / (ATOL + RTOL * np.abs(want))))


def _inputs(scale):
    rng = np.random.default_rng(11)
    p0 = rng.standard_normal(N).astype(np.float32)
    grads = [(rng.standard_normal(N) * scale).astype(np.float32) for _ in range(STEPS)]
    return p0, grads


@pytest.mark.parametrize("scale", [1.0, 1e-3, 30.0])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_model_matches_torch_adam(wd, scale):
    p0, grads = _inputs(scale)
    lr = 1e-3
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(N, np.float32), np.zeros(N, np.float32)
    for step, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g) * GRAD_SCALE            # exact: a power of two
        opt.step()
        p, m, v = OM.adam(p, g, m, v, lr, 0.9, 0.999, 1e-8, wd, step, GRAD_SCALE)
        st = opt.state[tp]
        worst = {k: _worst(a, b.detach().numpy().astype(np.float64)) for k, a, b in
                 (("p", p, tp), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"]))}
        print(f"adam wd {wd} scale {scale} step {step}: fraction of the bound {worst}")
        assert max(worst.values()) <= 1.0, (step, worst)
        assert int(st["step"]) == step


@pytest.mark.parametrize("scale", [1.0, 1e-3, 30.0])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_sgd_model_matches_torch_sgd_with_momentum(wd, scale):
    p0, grads = _inputs(scale)
    lr = 1e-2
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.SGD([tp], lr=lr, momentum=0.9, weight_decay=wd)
    p, buf = p0.copy(), np.zeros(N, np.float32)               # a zero buffer: torch's first step sets buf = g'
    for step, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g) * GRAD_SCALE
        opt.step()
        p, buf = OM.sgd(p, g, buf, lr, 0.9, wd, GRAD_SCALE)
        worst = {"p": _worst(p, tp.detach().numpy().astype(np.float64)),
                 "buf": _worst(buf, opt.state[tp]["momentum_buffer"].numpy().astype(np.float64))}
        print(f"sgd wd {wd} scale {scale} step {step}: fraction of the bound {worst}")
        assert max(worst.values()) <= 1.0, (step, worst)


def test_sgd_first_step_from_a_zero_buffer_is_the_gradient_bit_for_bit():
    p0, grads = _inputs(1.0)
    p, buf = OM.sgd(p0, grads[0], np.zeros(N, np.float32), 1e-2, 0.9, 0.0, GRAD_SCALE)
    assert np.array_equal(buf, grads[0] * np.float32(GRAD_SCALE))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. config
# ---------------------------------------------------------------------------------------------------------------------------------
def test_config_key_default_and_validator():
    assert config.DEFAULTS["optim_type"] == "adamw" and config.OPTIM_TYPES == ("adamw", "adam", "sgd")
    base = ["with", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta"]
    assert config.parse_cli(base)["optim_type"] == "adamw"
    for name in config.OPTIM_TYPES:
        assert config.optim_type({"optim_type": name}) == name
        assert config.parse_cli(base + [f"optim_type={name}"])["optim_type"] == name
        assert config.tiny_config(optim_type=name)["optim_type"] == name
    assert config.optim_type({}) == "adamw"
    for bad in ("lion", "AdamW", "SGD", "", None, 1, ["sgd"]):
        with pytest.raises(ValueError, match="optim_type"):
            config.optim_type({"optim_type": bad})
    for bad in ("lion", "AdamW"):
        with pytest.raises(ValueError, match="optim_type"):
            config.parse_cli(base + [f"optim_type={bad}"])
        with pytest.raises(ValueError, match="optim_type"):
            config.tiny_config(optim_type=bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_library_and_stub_agree_and_the_abi_is_still_4():
    """The relations between the optimizer entry points, in the header's text and in the binding.  (Binding against header type
    by type, the stub, the ABI number and the descriptor sizes: tests/test_host_logic.py, for the whole ABI.)"""
    protos = abi_header.prototypes()
    assert all(protos[name][0] == "int" for name in OPTIM_ENTRIES)
    # each _clip form is its plain form plus the record in front of the stream; neither rule takes hyper_dev
    for plain, nargs in (("m3ae_adam", 14), ("m3ae_sgd", 10)):
        a, c = _lib._SIGS[plain][1], _lib._SIGS[plain + "_clip"][1]
        assert len(a) == nargs and c == a[:-1] + [C.c_void_p, a[-1]]
        pa, pc = protos[plain][1], protos[plain + "_clip"][1]
        assert pc == pa[:-1] + ["const float* clip_dev", pa[-1]] and pa[-1] == "void* stream"
        assert not any("hyper_dev" in x for x in pc)
    # m3ae_adam is m3ae_adamw without hyper_dev and with the betas in double; m3ae_adamw keeps its signature
    w = _lib._SIGS["m3ae_adamw"][1]
    assert len(w) == 15 and [C.c_float if x is C.c_double else x for x in _lib._SIGS["m3ae_adam"][1]] == w[:-2] + [w[-1]]
    assert len(protos["m3ae_adamw"][1]) == 15
    assert [x.replace("double", "float") for x in protos["m3ae_adam"][1]] == [x for x in protos["m3ae_adamw"][1] if "hyper_dev" not in x]
    assert protos["m3ae_adam"][1][7:9] == ["double beta1", "double beta2"]


def test_entry_points_check_their_arguments_before_any_launch():
    """Made-up pointers are never read: the checks come first (no device is touched on this machine)."""
    L = _lib.lib()
    x, rec = 0x10000, 0x20000
    adam = (8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0)
    sgd = (8, 1e-2, 0.9, 0.0, 1.0)
    for i in range(4):                                                                  # a null p, g, m or v
        ptrs = [x] * 4
        ptrs[i] = None
        assert L.m3ae_adam(*ptrs, None, *adam, None) == -1
        assert L.m3ae_adam_clip(*ptrs, None, *adam, rec, None) == -1
    for i in range(3):                                                                  # a null p, g or buf
        ptrs = [x] * 3
        ptrs[i] = None
        assert L.m3ae_sgd(*ptrs, None, *sgd, None) == -1
        assert L.m3ae_sgd_clip(*ptrs, None, *sgd, rec, None) == -1
    assert L.m3ae_adam_clip(x, x, x, x, None, *adam, None, None) == -1                  # no record
    assert L.m3ae_sgd_clip(x, x, x, None, *sgd, None, None) == -1
    assert L.m3ae_adam(x, x, x, x, None, 0, *adam[1:], None) == -1                      # n <= 0
    assert L.m3ae_sgd(x, x, x, None, 0, *sgd[1:], None) == -1
    assert L.m3ae_adam(x, x, x, x, None, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, None) == -1     # step < 1
    # n % 4 != 0, a pointer off the 16-byte grid, a record off the 4-byte grid: M3AE_ERR_ALIGN
    assert L.m3ae_adam(x, x, x, x, None, 6, *adam[1:], None) == -3
    assert L.m3ae_sgd(x, x, x, None, 6, *sgd[1:], None) == -3
    for i in range(4):
        ptrs = [x] * 4
        ptrs[i] = x + 4
        assert L.m3ae_adam(*ptrs, None, *adam, None) == -3
    for i in range(3):
        ptrs = [x] * 3
        ptrs[i] = x + 8
        assert L.m3ae_sgd(*ptrs, None, *sgd, None) == -3
    assert L.m3ae_adam_clip(x, x, x, x, None, *adam, rec + 2, None) == -3
    assert L.m3ae_sgd_clip(x, x, x, None, *sgd, rec + 2, None) == -3


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. host-side dispatch: no library call
# ---------------------------------------------------------------------------------------------------------------------------------
class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached: {name}")


class Recording:
    """Stands in for the library: records (name, arguments) of every entry point called and returns 0."""

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


def _val(x):
    return getattr(x, "value", x)


@pytest.mark.parametrize("clip", [0.0, 1.0])
@pytest.mark.parametrize("rule", ["adamw", "adam", "sgd"])
def test_store_dispatches_on_the_rule(monkeypatch, rule, clip):
    """Which entry point a step reaches, with which scalars, and which state it allocates -- the library replaced by a recorder."""
    from m3ae_amd import gradnorm, ops
    monkeypatch.setattr(ops, "_stream", lambda: None)
    st, _ = _cpu_store(optim_type=rule, gradient_clip_val=clip)
    rec = Recording()
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(_lib, "lib", lambda: _lib._lib)
    monkeypatch.setattr(gradnorm, "clip_finalize", lambda *a: None)

    class Sums:
        def run(self, *a):
            return None
    st._sums = Sums()
    assert st.optim == rule and st.exp_avg is None and st.exp_avg_sq is None
    st.optimizer_step(max_steps=10, lr_factor=1.0, grad_scale=0.25)
    name = {"adamw": "m3ae_adamw", "adam": "m3ae_adam", "sgd": "m3ae_sgd"}[rule] + ("_clip" if clip else "")
    nonempty = sum(1 for a, b in st.segments[:6] if b > a)
    assert [c[0] for c in rec.calls] == [name] * nonempty and nonempty >= 2
    assert st.exp_avg is not None and (st.exp_avg_sq is None) == (rule == "sgd")
    hp = st.hparams_fn(st.cfg)
    gi = next(i for i, (a, b) in enumerate(st.segments[:6]) if b > a)
    a0 = rec.calls[0][1]
    if rule == "sgd":
        assert len(a0) == 10 + bool(clip)
        assert _val(a0[2]) == st.exp_avg.data_ptr() + 4 * st.segments[gi][0] and a0[3] is None
        assert a0[4:9] == (st.segments[gi][1] - st.segments[gi][0], hp[gi][0], 0.9, hp[gi][1], 0.25)
    else:
        assert len(a0) == (15 if rule == "adamw" else 14) + bool(clip)
        assert _val(a0[3]) == st.exp_avg_sq.data_ptr() + 4 * st.segments[gi][0] and a0[4] is None
        b2 = 0.98 if rule == "adamw" else 0.999       # the reference's AdamW betas; torch's Adam defaults
        assert a0[5:13] == (st.segments[gi][1] - st.segments[gi][0], hp[gi][0], 0.9, b2, 1e-8, hp[gi][1], 1, 0.25)
        if rule == "adamw":
            assert a0[13] is None                     # hyper_dev
    if clip:
        assert _val(a0[-2]) == st._clip_record.data_ptr()
    # explicit betas reach the kernel under both Adam rules
    if rule != "sgd":
        rec.calls.clear()
        st.optimizer_step(max_steps=10, lr_factor=1.0, betas=(0.8, 0.9))
        assert rec.calls[0][1][7:9] == (0.8, 0.9) and rec.calls[0][1][11] == 2
    # the adamw_* names are AdamW and nothing else
    rec.calls.clear()
    if rule == "adamw":
        st.adamw_step(max_steps=10, lr_factor=1.0)
        hyper = st.begin_update(max_steps=10)
        st.adamw_apply(hyper)
        st.adamw_range(0, 64, 0, hyper)
        assert [c[0] for c in rec.calls] == [name] * (2 * nonempty) + ["m3ae_adamw"]      # (a range call without a record: plain)
    else:
        hyper = st.begin_update(max_steps=10)
        count = st.step_count
        for call in (lambda: st.adamw_step(max_steps=10), lambda: st.adamw_apply(hyper), lambda: st.adamw_range(0, 64, 0, hyper)):
            with pytest.raises(ValueError, match="optim_type"):
                call()
        assert rec.calls == [] and st.step_count == count


def test_a_misspelt_rule_fails_at_the_store():
    from m3ae_amd.param_store import ParamStore
    mod = torch.nn.Linear(4, 4)
    cfg = dict(config.tiny_config(compute_dtype="fp32"), optim_type="Adam")
    with pytest.raises(ValueError, match="optim_type"):
        ParamStore(mod, cfg, "cpu", torch.float32)


def test_make_optimizer_classes_groups_and_state_layout(monkeypatch):
    from m3ae_amd import param_store as PS
    monkeypatch.setattr(_lib, "_lib", NoLibrary())
    monkeypatch.setattr(_lib, "lib", lambda: _lib._lib)
    made = {}
    for rule, cls in (("adamw", PS.FlatAdamW), ("adam", PS.FlatAdam), ("sgd", PS.FlatSGD)):
        st, mod = _cpu_store(optim_type=rule)
        opts, scheds = st.make_optimizer(10)
        opt = opts[0]
        assert type(opt) is cls and isinstance(opt, torch.optim.Optimizer) and scheds[0]["interval"] == "step"
        assert [pg["m3ae_group"] for pg in opt.param_groups] == list(range(6))
        hp = st.hparams_fn(st.cfg)
        assert [pg["initial_lr"] for pg in opt.param_groups] == [lr for lr, _ in hp]
        assert [pg["weight_decay"] for pg in opt.param_groups] == [wd for _, wd in hp]
        made[rule] = (st, mod, opt)
    for pg in made["adamw"][2].param_groups:
        assert pg["betas"] == (0.9, 0.98) and pg["eps"] == 1e-8 and "amsgrad" not in pg and "momentum" not in pg
    for pg in made["adam"][2].param_groups:
        assert pg["betas"] == (0.9, 0.999) and pg["eps"] == 1e-8 and pg["amsgrad"] is False
        assert set(torch.optim.Adam([torch.zeros(1)]).defaults) <= set(pg)
    for pg in made["sgd"][2].param_groups:
        assert pg["momentum"] == 0.9 and pg["dampening"] == 0 and pg["nesterov"] is False and "betas" not in pg
        assert set(torch.optim.SGD([torch.zeros(1)], lr=0.1).defaults) <= set(pg)
    # torch's per-parameter layout
    sd = {rule: made[rule][2].state_dict() for rule in made}
    assert all(set(v) == {"step", "exp_avg", "exp_avg_sq"} for v in sd["adam"]["state"].values()) and sd["adam"]["state"]
    assert all(set(v) == {"momentum_buffer"} for v in sd["sgd"]["state"].values()) and sd["sgd"]["state"]
    assert made["sgd"][0].exp_avg_sq is None and made["sgd"][0].exp_avg is not None
    # the views are the flat buffers
    st, mod, opt = made["sgd"]
    p = next(iter(mod.parameters()))
    assert opt.state[p]["momentum_buffer"].data_ptr() == st.exp_avg.data_ptr() + 4 * st.offset[id(p)]
    # a cross-rule load raises, in every direction
    for a in made:
        for b in made:
            if a != b:
                with pytest.raises(ValueError, match="optim"):
                    made[a][2].load_state_dict(sd[b])
    for rule in made:
        made[rule][2].load_state_dict(sd[rule])
    # a Flat* class over a store of another rule
    with pytest.raises(ValueError, match="optim_type"):
        PS.FlatSGD(made["adam"][0])
    with pytest.raises(ValueError, match="optim_type"):
        PS.FlatAdamW(made["sgd"][0])


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_state_dicts_exchange_with_torch_optim_on_the_cpu(monkeypatch, rule):
    """A state dict of the matching torch.optim class over the same groups loads into the Flat* optimizer, and the reverse."""
    monkeypatch.setattr(_lib, "_lib", NoLibrary())
    monkeypatch.setattr(_lib, "lib", lambda: _lib._lib)
    st, mod = _cpu_store(optim_type=rule)
    opt = st.make_optimizer(10)[0][0]

    def torch_twin():
        groups = [dict(params=[torch.nn.Parameter(p.detach().clone()) for p in pg["params"]], lr=pg["lr"],
                       weight_decay=pg["weight_decay"]) for pg in opt.param_groups]
        return torch.optim.Adam(groups) if rule == "adam" else torch.optim.SGD(groups, lr=1e-3, momentum=0.9)
    ref = torch_twin()
    torch.manual_seed(1)
    for _ in range(2):
        for pg in ref.param_groups:
            for p in pg["params"]:
                p.grad = torch.randn_like(p)
        ref.step()
    opt.load_state_dict(ref.state_dict())
    key = "exp_avg" if rule == "adam" else "momentum_buffer"
    for pg, rg in zip(opt.param_groups, ref.param_groups):
        for p, r in zip(pg["params"], rg["params"]):
            if p.numel():
                o = st.offset[id(p)]
                assert torch.equal(st.exp_avg[o:o + p.numel()].view(p.shape), ref.state[r][key])
                if rule == "adam":
                    assert torch.equal(st.exp_avg_sq[o:o + p.numel()].view(p.shape), ref.state[r]["exp_avg_sq"])
    assert st.step_count == (2 if rule == "adam" else 0) and (st.exp_avg_sq is None) == (rule == "sgd")
    # the reverse: torch loads ours and steps with it
    back = torch_twin()
    back.load_state_dict(opt.state_dict())
    for pg, rg in zip(back.param_groups, ref.param_groups):
        for p, r in zip(pg["params"], rg["params"]):
            if p.numel():
                assert torch.equal(back.state[p][key], ref.state[r][key])
                p.grad = torch.ones_like(p)
    back.step()


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_graphed_step_refuses_the_rule_and_the_reducer_takes_it(monkeypatch, rule):
    from m3ae_amd.ddp import FlatGradReducer
    from m3ae_amd.graph import GraphedStep
    monkeypatch.setattr(_lib, "_lib", NoLibrary())
    monkeypatch.setattr(_lib, "lib", lambda: _lib._lib)
    st, _ = _cpu_store(optim_type=rule)

    class Model:
        store = st
    with pytest.raises(ValueError, match="optim_type"):
        GraphedStep(Model(), {}, 10)

    class HP:
        config = {"optim_type": rule}

    class Model2:
        hparams = HP()
    with pytest.raises(ValueError, match="optim_type"):
        GraphedStep(Model2(), {}, 10)
    assert st.step_count == 0 and st.exp_avg is None
    # update_in_backward is the same per-range call under every rule: the reducer's source names no rule
    import inspect
    src = inspect.getsource(FlatGradReducer)
    assert "update_range(" in src and "adamw_range(" not in src
