"""GPU: optim_type adam / sgd (csrc/misc.hip: m3ae_adam, m3ae_sgd and their _clip forms; ParamStore, the Flat* optimizers,
FlatGradReducer, GraphedStep, trainer).

Bounds.  p, m, v and buf against the float32 models (tests/optim_model.py) and against torch.optim on CPU copies: rtol 1e-5, atol
1e-6, the bound tests/test_gpu_ops.py::test_adamw_matches_hf_semantics holds m3ae_adamw to (the models assume no fused multiply-add,
the compiler may contract: a few ulp per operation, far inside).  The bf16 shadow: 1e-2 / 1e-3, as there.  Everything the _clip
forms do with the record, and every statement about one path against another (generic names against adamw_*, in-backward against
after-backward, a resumed run against an uninterrupted one, in deterministic mode) is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, ops, synth  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from oracle_util import tiny_batch, tiny_config  # noqa: E402
import optim_model as OM  # noqa: E402

FENCE = 64            # elements on either side of every buffer a kernel writes or reads
SENTINEL = -777.0
RTOL, ATOL = 1e-5, 1e-6
EW_CAP = 8192 * 256 * 4            # ew_grid's cap x EW_BLOCK x 4 elements per lane: above it the grid-stride loop runs twice
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
SGD = dict(lr=1e-2, momentum=0.9)
GS = 0.5


@pytest.fixture(autouse=True)
def _deterministic_mode_off_afterwards():
    yield
    ops.set_deterministic(False)


def vp(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def fenced(n, dtype, fill=SENTINEL):
    whole = torch.full((n + 2 * FENCE,), fill, dtype=dtype, device="cuda")
    return whole, whole[FENCE:FENCE + n]


def fences_intact(whole, n, fill=SENTINEL):
    f = torch.full((FENCE,), fill, dtype=whole.dtype, device="cuda")
    return torch.equal(whole[:FENCE], f) and torch.equal(whole[FENCE + n:], f)


def close(got, want, rtol=RTOL, atol=ATOL, msg=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    worst = float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want))))
    assert worst <= 1.0, f"{msg}: {worst:.3g} of the bound"
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels against the models and torch.optim
# ---------------------------------------------------------------------------------------------------------------------------------
def make_state(rule, n, shadow, seed, zero_moments=False):
    """Fenced device buffers {p, g, m, (v), (s)} of one flat segment."""
    g = torch.Generator().manual_seed(seed)
    st = {}
    for name, scale in (("p", 1.0), ("g", 1.0), ("m", 0.05)):
        st[name] = fenced(n, torch.float32)
        st[name][1].copy_(torch.randn(n, generator=g) * scale)
    if rule == "adam":
        st["v"] = fenced(n, torch.float32)
        st["v"][1].copy_(torch.rand(n, generator=g) * 0.01)
    if zero_moments:
        st["m"][1].zero_()
        if "v" in st:
            st["v"][1].zero_()
    if shadow:
        st["s"] = fenced(n, torch.bfloat16)
        st["s"][1].copy_(st["p"][1])
    return st


def launch(rule, st, n, wd, step, grad_scale, record=None, check=True, views=None):
    """m3ae_adam / m3ae_sgd (or the _clip form with `record`) over the state; returns the status code."""
    L = _lib.lib()
    v = views or {k: t[1] for k, t in st.items()}
    sh = vp(v["s"]) if "s" in v else None
    if rule == "adam":
        name = "m3ae_adam"
        args = (vp(v["p"]), vp(v["g"]), vp(v["m"]), vp(v["v"]), sh, n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd, step,
                grad_scale)
    else:
        name = "m3ae_sgd"
        args = (vp(v["p"]), vp(v["g"]), vp(v["m"]), sh, n, SGD["lr"], SGD["momentum"], wd, grad_scale)
    if record is not None:
        name, args = name + "_clip", args + (vp(record),)
    rc = getattr(L, name)(*args, stream())
    torch.cuda.synchronize()
    if check:
        _lib.check(rc, name)
    return rc


def same_state(a, b, n):
    def bits(k, t):
        return t.view(torch.int16 if k == "s" else torch.int32)
    return all(torch.equal(bits(k, a[k][0]), bits(k, b[k][0])) for k in a) and all(fences_intact(a[k][0], n) for k in a)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("n", [4, 64, 4100, EW_CAP + 68])
@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_kernels_match_the_models_and_torch_optim(rule, n, shadow, wd):
    """Steps 1..3 from zero moments (torch's own start), a new gradient every step."""
    st = make_state(rule, n, shadow, seed=5, zero_moments=True)
    host = {k: t[1].cpu().numpy().copy() for k, t in st.items() if k != "s"}
    tp = torch.nn.Parameter(torch.from_numpy(host["p"].copy()))
    if rule == "adam":
        opt = torch.optim.Adam([tp], lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"], weight_decay=wd)
    else:
        opt = torch.optim.SGD([tp], lr=SGD["lr"], momentum=SGD["momentum"], weight_decay=wd)
    gen = torch.Generator().manual_seed(6)
    worst = {}
    for step in (1, 2, 3):
        g = torch.randn(n, generator=gen)
        st["g"][1].copy_(g)
        launch(rule, st, n, wd, step, GS)
        tp.grad = g * GS                                      # exact: a power of two
        opt.step()
        if rule == "adam":
            host["p"], host["m"], host["v"] = OM.adam(host["p"], g.numpy(), host["m"], host["v"], ADAM["lr"], ADAM["b1"], ADAM["b2"],
                                                      ADAM["eps"], wd, step, GS)
            ref = {"p": tp.detach(), "m": opt.state[tp]["exp_avg"], "v": opt.state[tp]["exp_avg_sq"]}
        else:
            host["p"], host["m"] = OM.sgd(host["p"], g.numpy(), host["m"], SGD["lr"], SGD["momentum"], wd, GS)
            ref = {"p": tp.detach(), "m": opt.state[tp]["momentum_buffer"]}
        for k, r in ref.items():
            got = st[k][1].cpu().numpy()
            worst[k] = max(worst.get(k, 0.0), close(got, host[k], msg=f"{rule} {k} step {step} against the model"),
                           close(got, r.numpy(), msg=f"{rule} {k} step {step} against torch.optim"))
        if shadow:
            close(st["s"][1].float().cpu().numpy(), host["p"], 1e-2, 1e-3, msg=f"{rule} shadow step {step}")
        assert all(fences_intact(t[0], n) for t in st.values())
    print(f"{rule} n {n} shadow {shadow} wd {wd}: worst fraction of the bound {worst}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the _clip forms against the plain forms, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
def make_record(coef, skip):
    rec = torch.zeros(_lib.CLIP_RECORD_WORDS, dtype=torch.float32, device="cuda")
    rec[_lib.CLIP_COEF] = float(np.float32(coef))
    rec.view(torch.int32)[_lib.CLIP_SKIP] = int(skip)
    return rec


@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("n", [4, 8, 1028])
@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_clip_forms_equal_the_plain_forms_with_the_scaled_factor_and_skip_touches_nothing(rule, n, shadow):
    wd, step = 0.01, 3
    # coef = 1: the bits of the plain form
    a, b = make_state(rule, n, shadow, 1), make_state(rule, n, shadow, 1)
    before = {k: v[0].clone() for k, v in a.items()}
    launch(rule, a, n, wd, step, GS)
    launch(rule, b, n, wd, step, GS, make_record(1.0, 0))
    assert same_state(a, b, n)
    assert not torch.equal(a["p"][0], before["p"]) and not torch.equal(a["m"][0], before["m"])      # (the step did something)
    # coef = 0.37: the plain form at float32(grad_scale) * float32(0.37)
    a, b = make_state(rule, n, shadow, 2), make_state(rule, n, shadow, 2)
    launch(rule, a, n, wd, step, float(np.float32(GS) * np.float32(0.37)))
    launch(rule, b, n, wd, step, GS, make_record(0.37, 0))
    assert same_state(a, b, n)
    # skip = 1: nothing is touched, whatever the coefficient word holds; the gradient holds an inf
    for coef in (0.0, 1.0):
        a = make_state(rule, n, shadow, 3)
        a["g"][1][n // 2] = float("inf")
        before = {k: (v[0].clone(), None) for k, v in a.items()}
        launch(rule, a, n, wd, step, GS, make_record(coef, 1))
        assert same_state(a, before, n)


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_misaligned_calls_are_refused_without_a_launch(rule):
    n = 64
    for clip in (False, True):
        rec = make_record(1.0, 0) if clip else None
        st = make_state(rule, n + 4, True, 4)
        before = {k: (v[0].clone(), None) for k, v in st.items()}
        assert launch(rule, st, 62, 0.01, 1, GS, rec, check=False) == -3            # n % 4 != 0
        assert launch(rule, st, 0, 0.01, 1, GS, rec, check=False) == -1
        for k in ("p", "g", "m", "v"):                                              # one fp32 pointer 4 bytes off the 16-byte grid
            if k in st:
                views = {q: t[1] for q, t in st.items()}
                views[k] = st[k][1][1:]
                assert launch(rule, st, n, 0.01, 1, GS, rec, check=False, views=views) == -3, k
        if clip:
            off = torch.zeros(_lib.CLIP_RECORD_WORDS * 4 + 2, dtype=torch.uint8, device="cuda")[2:]
            assert launch(rule, st, n, 0.01, 1, GS, off, check=False) == -3         # the record off the 4-byte grid
        assert same_state(st, before, n + 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the tiny model under the real rule
# ---------------------------------------------------------------------------------------------------------------------------------
def to_dev(batch):
    out = {}
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to("cuda")
        elif isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            out[k] = [t.to("cuda") for t in v]
        else:
            out[k] = v
    return out


class StubTrainer:
    max_steps = 20


def build(**over):
    cfg = tiny_config(compute_dtype="bf16", deterministic=True, learning_rate=1e-3, **over)
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    m.eval()
    m.trainer_ref = StubTrainer()
    return m


def backward(m, b):
    m.store.zero_grad()
    m.training_step(b).backward()
    torch.cuda.synchronize()


def state_of(st):
    return [t.clone() for t in (st.flat, st.exp_avg, st.exp_avg_sq, st.shadow) if t is not None]


def states_equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def torch_twin(rule, store, opt):
    """torch.optim.Adam / SGD on the CPU over the same six groups: its parameters are views of ONE flat CPU copy of the trainable
    range, so that the whole buffer compares in one call.  Returns (optimizer, LambdaLR, flat copy, [(param, offset)])."""
    flat = store.flat[:store.trainable_end].cpu().clone()
    groups, where = [], []
    for pg in opt.param_groups:
        ps = []
        for p in pg["params"]:
            if p.numel():
                o = store.offset[id(p)]
                q = torch.nn.Parameter(flat[o:o + p.numel()].view(p.shape))
                assert q.data_ptr() == flat.data_ptr() + 4 * o
                ps.append(q)
                where.append((q, o))
        groups.append(dict(params=ps, lr=pg["initial_lr"], weight_decay=pg["weight_decay"]))
    ref = torch.optim.Adam(groups) if rule == "adam" else torch.optim.SGD(groups, lr=1e-3, momentum=0.9)
    sched = torch.optim.lr_scheduler.LambdaLR(ref, lambda step: store.lr_factor(step, StubTrainer.max_steps))
    return ref, sched, flat, where


RUNS = {}


def three_rounds(rule):
    """Three training_step + optimizer.step() + scheduler.step() rounds of the tiny model under `rule`, with torch.optim driven on
    the CPU from copies of the flat gradient buffer.  Computed once per rule and shared (read-only) by the tests below."""
    if rule in RUNS:
        return RUNS[rule]
    b = to_dev(tiny_batch())
    m = build(optim_type=rule)
    opts, scheds = m.configure_optimizers()
    opt, sched = opts[0], scheds[0]["scheduler"]
    ref, rsched, rflat, where = torch_twin(rule, m.store, opt)
    start = m.store.flat.clone()
    lrs, worst = [], 0.0
    for step in range(3):
        lrs.append([pg["lr"] for pg in opt.param_groups])
        backward(m, b)
        g = m.store.grad.cpu()
        for q, o in where:
            q.grad = g[o:o + q.numel()].view(q.shape)
        opt.step()
        sched.step()
        ref.step()
        rsched.step()
        torch.cuda.synchronize()
        worst = max(worst, close(m.store.flat[:m.store.trainable_end].cpu().numpy(), rflat.numpy(), msg=f"{rule} store.flat step {step}"))
    RUNS[rule] = dict(model=m, opt=opt, sched=sched, ref=ref, rflat=rflat, where=where, start=start, lrs=lrs, worst=worst, batch=b)
    return RUNS[rule]


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_tiny_model_steps_match_torch_optim_over_the_six_groups(rule):
    r = three_rounds(rule)
    m, opt = r["model"], r["opt"]
    st = m.store
    print(f"{rule}: store.flat against torch.optim, worst fraction of the bound {r['worst']}")
    assert type(opt).__name__ == {"adam": "FlatAdam", "sgd": "FlatSGD"}[rule]
    moved = (st.flat - r["start"])[:st.trainable_end].abs().max().item()
    assert moved > 100 * ATOL, moved                                                    # (the comparison saw real steps)
    # the learning rates followed the LambdaLR schedule (warm-up of 2 of 20 steps: 0, 1/2, 1)
    base = [lr for lr, _ in st.hparams_fn(st.cfg)]
    for step, row in enumerate(r["lrs"]):
        np.testing.assert_allclose(row, np.array(base) * st.lr_factor(step, StubTrainer.max_steps), rtol=1e-12, atol=0)
    assert r["lrs"][0] == [0.0] * 6 and r["lrs"][2] == base
    # the moments against torch's, per parameter
    key = "exp_avg" if rule == "adam" else "momentum_buffer"
    for q, o in r["where"]:
        close(st.exp_avg[o:o + q.numel()].cpu().numpy(), r["ref"].state[q][key].reshape(-1).numpy(), msg=f"{rule} {key}")
        if rule == "adam":
            close(st.exp_avg_sq[o:o + q.numel()].cpu().numpy(), r["ref"].state[q]["exp_avg_sq"].reshape(-1).numpy(), msg="adam exp_avg_sq")
    # the bf16 shadow follows the masters
    assert torch.equal(st.shadow[:st.trainable_end], st.flat[:st.trainable_end].to(torch.bfloat16))
    assert st.step_count == 3


def test_sgd_never_allocates_the_second_moment():
    st = three_rounds("sgd")["model"].store
    assert st.exp_avg_sq is None and st.exp_avg is not None and st.exp_avg.abs().max().item() > 0
    st = three_rounds("adam")["model"].store
    assert st.exp_avg_sq is not None and st.exp_avg_sq.abs().max().item() > 0


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_state_dict_round_trip_torch_state_loads_and_a_cross_rule_load_raises(rule):
    r = three_rounds(rule)
    m, opt, sched, b = r["model"], r["opt"], r["sched"], r["batch"]
    sd_opt, sd_sched = opt.state_dict(), sched.state_dict()
    want = {"step", "exp_avg", "exp_avg_sq"} if rule == "adam" else {"momentum_buffer"}
    assert len(sd_opt["state"]) > 50 and all(set(v) == want for v in sd_opt["state"].values())

    def fresh():
        m2 = build(optim_type=rule)
        m2.load_state_dict(m.state_dict())
        m2.store.sync_shadows()
        o2, s2 = m2.configure_optimizers()
        return m2, o2[0], s2[0]["scheduler"]
    m2, o2, s2 = fresh()
    o2.load_state_dict(sd_opt)
    s2.load_state_dict(sd_sched)
    assert states_equal(state_of(m.store), state_of(m2.store)) and m2.store.step_count == (3 if rule == "adam" else 0)
    # the next step on a copy of the first model's state (the shared run stays as it is) and on the fresh model: bit-equal
    m1, o1, s1 = fresh()
    o1.load_state_dict(sd_opt)
    s1.load_state_dict(sd_sched)
    m1.store.step_count = m.store.step_count
    for mm_, oo, ss in ((m1, o1, s1), (m2, o2, s2)):
        backward(mm_, b)
        oo.step()
        ss.step()
    torch.cuda.synchronize()
    assert states_equal(state_of(m1.store), state_of(m2.store))
    assert not torch.equal(m2.store.flat, m.store.flat)
    # a torch.optim state dict over the same groups loads: the flat state holds torch's values
    m3, o3, _ = fresh()
    o3.load_state_dict(r["ref"].state_dict())
    key = "exp_avg" if rule == "adam" else "momentum_buffer"
    for q, o in r["where"]:
        assert torch.equal(m3.store.exp_avg[o:o + q.numel()].cpu(), r["ref"].state[q][key].reshape(-1))
    assert (m3.store.exp_avg_sq is None) == (rule == "sgd") and m3.store.step_count == (3 if rule == "adam" else 0)
    # and ours loads into torch.optim
    back, _, _, where = torch_twin(rule, m.store, opt)
    back.load_state_dict(sd_opt)
    for (q, o), (q0, _) in zip(where, r["where"]):
        close(back.state[q][key].reshape(-1).numpy(), r["ref"].state[q0][key].reshape(-1).numpy(), msg="round trip through torch.optim")
    # state of another rule is refused
    other = "sgd" if rule == "adam" else "adam"
    with pytest.raises(ValueError, match="optim"):
        o3.load_state_dict(three_rounds(other)["opt"].state_dict())
    with pytest.raises(ValueError, match="optim"):
        o3.load_state_dict(three_rounds(other)["ref"].state_dict())
    w = build()
    ow = w.configure_optimizers()[0][0]
    assert type(ow).__name__ == "FlatAdamW"
    with pytest.raises(ValueError, match="optim"):
        o3.load_state_dict(ow.state_dict())
    with pytest.raises(ValueError, match="optim"):
        ow.load_state_dict(sd_opt)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. adamw is unchanged
# ---------------------------------------------------------------------------------------------------------------------------------
class Counting:
    """The loaded library with every call counted by entry point (everything reaches it through _lib.lib())."""

    def __init__(self, L):
        self.L, self.counts = L, {}

    def __getattr__(self, name):
        fn = getattr(self.L, name)
        if not name.startswith("m3ae_"):
            return fn

        def counted(*a):
            self.counts[name] = self.counts.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("clip", [0.0, 1e30])
def test_adamw_makes_the_same_launches_and_the_same_bits_under_the_generic_names(monkeypatch, clip):
    b = to_dev(tiny_batch())
    old, new, opt_m = build(gradient_clip_val=clip), build(gradient_clip_val=clip), build(gradient_clip_val=clip)
    assert old.store.optim == "adamw"
    opt = opt_m.configure_optimizers()[0][0]
    for m in (old, new):      # first step outside the count: lazy buffers
        backward(m, b)
    old.store.adamw_step(max_steps=10, lr_factor=1.0)
    new.store.optimizer_step(max_steps=10, lr_factor=1.0)
    cnt = Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", cnt)
    counts = []
    for m, step in ((old, lambda: old.store.adamw_step(max_steps=10, lr_factor=1.0)),
                    (new, lambda: new.store.update_apply(new.store.begin_update(max_steps=10, lr_factor=1.0)))):
        cnt.counts = {}
        backward(m, b)
        before = dict(cnt.counts)
        step()
        counts.append({k: v - before.get(k, 0) for k, v in cnt.counts.items() if v != before.get(k, 0)})
    torch.cuda.synchronize()
    assert counts[0] == counts[1], counts
    name = "m3ae_adamw_clip" if clip else "m3ae_adamw"
    assert counts[0][name] == 6 and not any(k.startswith(("m3ae_adam", "m3ae_sgd")) and k != name for k in counts[0]), counts[0]
    if clip:
        assert counts[0]["m3ae_sumsq_segments"] == 1 and counts[0]["m3ae_clip_finalize"] == 1
    else:
        assert not any("sumsq" in k or "clip" in k for k in counts[0]), counts[0]
    assert states_equal(state_of(old.store), state_of(new.store))
    # FlatAdamW.step() is the same step: group learning rates of the constant factor 1
    monkeypatch.setattr(_lib, "_lib", cnt.L)
    hp = opt_m.store.hparams_fn(opt_m.store.cfg)
    for _ in range(2):
        backward(opt_m, b)
        for pg, (lr, _) in zip(opt.param_groups, hp):
            pg["lr"] = lr
        opt.step()
    torch.cuda.synchronize()
    assert states_equal(state_of(old.store), state_of(opt_m.store))


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_adamw_names_raise_under_another_rule_and_touch_nothing(rule):
    b = to_dev(tiny_batch())
    m = build(optim_type=rule)
    backward(m, b)
    before = state_of(m.store)
    with pytest.raises(ValueError, match="optim_type"):
        m.store.adamw_step(max_steps=10)
    hyper = m.store.begin_update(max_steps=10)
    with pytest.raises(ValueError, match="optim_type"):
        m.store.adamw_apply(hyper)
    with pytest.raises(ValueError, match="optim_type"):
        m.store.adamw_range(0, 64, 0, hyper)
    torch.cuda.synchronize()
    assert torch.equal(m.store.flat, before[0]) and m.store.exp_avg.abs().max().item() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. in-backward and graphed steps
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_update_in_backward_equals_the_step_after_backward(rule):
    from m3ae_amd.ddp import FlatGradReducer
    b = to_dev(tiny_batch())

    def run(in_backward):
        m = build(optim_type=rule)
        red = FlatGradReducer(m.store, bucket_bytes=64 << 10, tail_bytes=8 << 10, update_in_backward=in_backward)
        assert red.world == 1
        red.attach()
        early = []
        try:
            for step in range(3):
                m.store.zero_grad()
                if in_backward:
                    red.arm_update(max_steps=20, lr_factor=1.0)
                m.training_step(b).backward()
                red.finish()
                if in_backward:
                    early.append(red.updated_in_backward)
                else:
                    m.store.optimizer_step(max_steps=20, lr_factor=1.0)
        finally:
            red.detach()
        torch.cuda.synchronize()
        return state_of(m.store), early, m.store
    s0, _, _ = run(False)
    s1, early, st = run(True)
    print(f"{rule}: buckets updated under backward per step {early}")
    assert early[0] == 0 and max(early[1:]) > 0                 # (the first step learns the schedule; later ones update early)
    assert states_equal(s0, s1)
    assert (st.exp_avg_sq is None) == (rule == "sgd") and st.step_count == 3


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_graphed_step_refuses_the_rule(rule):
    from m3ae_amd.graph import GraphedStep
    m = build(optim_type=rule)
    with pytest.raises(ValueError, match="optim_type"):
        GraphedStep(m, to_dev(tiny_batch()), 10)
    assert m.store.step_count == 0 and m.store.exp_avg is None


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. trainer: sgd + clipping, checkpoint and resume
# ---------------------------------------------------------------------------------------------------------------------------------
def test_trainer_sgd_with_clipping_resumes_to_the_uninterrupted_third_step(tmp_path):
    """What trainer.run does with `data_root=synthetic optim_type=sgd gradient_clip_val=1.0`, piece by piece (run() hands back no
    model, and its data module cycles a pool of four batches from the start of the epoch it resumes in): two steps, a
    non-weights-only checkpoint, a fresh model resumed from it, and the third step -- against three uninterrupted steps.  The
    schedule is the three-step one in every run; one batch in the pool, no dropout anywhere (a resumed fit() restarts the sequence of
    dropout masks), deterministic mode: bit for bit."""
    from m3ae_amd import trainer
    tiny = ("image_size=64 hidden_size=128 num_heads=2 num_top_layer=2 input_image_embed_size=128 input_text_embed_size=128 "
            "vocab_size=1000 vit_width=128 vit_layers=3 text_hidden=128 text_layers=2 text_heads=2 text_inter=512").split()
    dev = torch.device("cuda", 0)

    def make(tag, rule="sgd"):
        argv = (["with", "data_root=synthetic", "num_gpus=1", "num_nodes=1", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta",
                 "exp_name=optim_sgd", "per_gpu_batchsize=4", "batch_size=4", "max_steps=3", "deterministic=True", "drop_rate=0.0",
                 "learning_rate=0.001", f"optim_type={rule}", "gradient_clip_val=1.0", f"log_dir={tmp_path / tag}", "seed=2"]
                + tiny)
        cfg = trainer.config_mod.parse_cli(argv)
        assert cfg["optim_type"] == rule and cfg["gradient_clip_val"] == 1.0
        torch.manual_seed(cfg["seed"])
        model = trainer.build_model(cfg, "cls", dev)
        for mod in model.modules():                  # RoBERTa's own p = 0.1 too: a resumed fit() restarts the mask sequence
            if hasattr(mod, "drop_rate"):
                mod.drop_rate = 0.0
        dm = trainer.SyntheticDataModule(cfg, 0, 1, dev, pool=1, train_samples=16, val_samples=4)
        tr = trainer.Trainer(cfg, model, dm, 0, 1, dev, log_every=1)
        assert type(tr.optimizer).__name__ == {"sgd": "FlatSGD", "adam": "FlatAdam"}[rule] and not tr.weights_only
        return tr, model
    whole, m_whole = make("whole")
    assert whole.fit()["global_step"] == 3
    torch.cuda.synchronize()
    first, m_first = make("first")
    first.plan["max_steps"] = 2                      # stop after two steps of the three-step schedule
    assert first.fit()["global_step"] == 2
    ckpt = first.save("two_steps.ckpt")
    ck = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert all(set(v) == {"momentum_buffer"} for v in ck["optimizer_states"][0]["state"].values()) and ck["optimizer_states"][0]["state"]
    assert ck["hyper_parameters"]["config"]["optim_type"] == "sgd"
    second, m_second = make("second")
    second.resume(ckpt)
    assert second.global_step == 2 and m_second.store.step_count == 2 and m_second.store.exp_avg_sq is None
    assert second.fit()["global_step"] == 3
    torch.cuda.synchronize()
    assert states_equal(state_of(m_whole.store), state_of(m_second.store))
    assert not torch.equal(m_first.store.flat, m_second.store.flat)                     # (the third step moved the parameters)
    s = m_whole.store.grad_stats()
    assert s["steps"] == 3 and s["skipped_steps"] == 0 and s["norm"] > 0
    # a checkpoint written under another optim_type fails loudly
    other, _ = make("other", "adam")
    with pytest.raises(ValueError, match="optim"):
        other.resume(ckpt)
