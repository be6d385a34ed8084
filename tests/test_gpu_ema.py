"""GPU: exponential moving average of the weights (config key `ema_decay`): m3ae_ema_update / m3ae_ema_swap (csrc/misc.hip) against
the numpy model and exact float64 (tests/ema_model.py: bound and derivation), ParamStore's buffer, counter and ema_weights(), the
trainer's evaluation and checkpoints, GraphedStep's refusal.  Every test fails without the feature: the entry points and the keys
do not exist there."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, config, ops, synth  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from m3ae_amd.param_store import PackedParam  # noqa: E402
from oracle_util import tiny_batch, tiny_config  # noqa: E402
import ema_model as EM  # noqa: E402

FENCE = 64            # elements on either side of every buffer a kernel writes or reads (keeps the 16-byte grid)
SENTINEL = -777.0
ERR_ARG, ERR_ALIGN = _lib.ERR_ARG, _lib.ERR_ALIGN


@pytest.fixture(autouse=True)
def _deterministic_mode_off_afterwards():
    yield
    ops.set_deterministic(False)      # (a model built with deterministic=True switches the process-wide mode on)


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def fenced(values, dtype=torch.float32):
    """(whole, view): `values` (numpy, or an element count) on the device between two fences of SENTINEL."""
    n = values if isinstance(values, int) else len(values)
    whole = torch.full((n + 2 * FENCE,), SENTINEL, dtype=dtype, device="cuda")
    view = whole[FENCE:FENCE + n]
    if not isinstance(values, int):
        view.copy_(torch.from_numpy(np.array(values)).to("cuda"))
    return whole, view


def fences_intact(whole, n):
    f = torch.full((FENCE,), SENTINEL, dtype=whole.dtype, device="cuda")
    return torch.equal(whole[:FENCE], f) and torch.equal(whole[FENCE + n:], f)


def bits(t):
    """Bit patterns of a device tensor (fp32 -> int32, bf16 -> int16): equality that tells -0 from +0 and compares inf as a value."""
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def ema_update(p, e, n, w, record=None, check=True):
    rc = _lib.lib().m3ae_ema_update(vp(p), vp(e), n, float(w), vp(record), stream())
    if check:
        assert rc == 0, rc
    return rc


def ema_swap(p, e, shadow, n, check=True):
    rc = _lib.lib().m3ae_ema_swap(vp(p), vp(e), vp(shadow), n, stream())
    if check:
        assert rc == 0, rc
    return rc


@functools.lru_cache(maxsize=None)
def inputs(n):
    """The (p, e) of size n, drawn once and shared; nobody writes to them (the device copies are made per test)."""
    p, e = EM.inputs(n, seed=n % 1000)
    p.setflags(write=False)
    e.setflags(write=False)
    return p, e


def make_record(coef, skip):
    rec = torch.zeros(_lib.CLIP_RECORD_WORDS, dtype=torch.float32, device="cuda")
    rec[_lib.CLIP_COEF] = float(np.float32(coef))
    rec.view(torch.int32)[_lib.CLIP_SKIP] = int(skip)
    return rec


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the update against float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", EM.WEIGHTS, ids=lambda w: f"w{float(w):.6g}")
@pytest.mark.parametrize("n", EM.SIZES)
def test_update_is_inside_the_two_rounding_bound_of_exact_float64(n, w):
    p, e = inputs(n)
    pw, pv = fenced(p)
    ew, ev = fenced(e)
    ema_update(pv, ev, n, w)
    torch.cuda.synchronize()
    got = ev.cpu().numpy()
    err, lim = np.abs(got.astype(np.float64) - EM.exact(p, e, w)), EM.bound(p, e, w)
    worst = float(np.max(err[lim > 0] / lim[lim > 0]))
    off_model = int(np.count_nonzero(got.view(np.uint32) != EM.update(p, e, w).view(np.uint32)))
    print(f"n {n} w {float(w):.6g}: worst |got - E| = {worst:.3f} of the bound; {off_model} elements differ from the model's bits")
    assert (err <= lim).all(), worst
    assert fences_intact(pw, n) and fences_intact(ew, n)                 # nothing outside [0, n)
    assert np.array_equal(pv.cpu().numpy().view(np.uint32), p.view(np.uint32))          # p is read only
    if w == 0:
        assert np.array_equal(got.view(np.uint32), e.view(np.uint32))    # w == 0: every bit of e
    else:
        assert not np.array_equal(got, e)                                # (the launch did something)
    # p == e elementwise: every bit of e, whatever the weight
    sw, sv = fenced(p)
    ema_update(pv, sv, n, w)
    assert np.array_equal(sv.cpu().numpy().view(np.uint32), p.view(np.uint32)) and fences_intact(sw, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the guard
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 4 * 256 + 4])
def test_a_skipped_step_leaves_the_average_and_an_unskipped_record_changes_nothing(n):
    p, e = inputs(n)
    w = EM.WEIGHTS[2]
    _, pv = fenced(p)
    for coef in (0.0, 1.0, 0.37):                      # skip = 1: not one bit moves, whatever the coefficient word holds
        ew, ev = fenced(e)
        ema_update(pv, ev, n, w, make_record(coef, 1))
        assert np.array_equal(ev.cpu().numpy().view(np.uint32), e.view(np.uint32)) and fences_intact(ew, n)
    _, plain = fenced(e)
    ema_update(pv, plain, n, w)
    assert not np.array_equal(plain.cpu().numpy(), e)
    for coef in (1.0, 0.37, 0.0):                      # skip = 0: the bits of the NULL-record call, the coefficient is not read
        ew, ev = fenced(e)
        ema_update(pv, ev, n, w, make_record(coef, 0))
        assert same_bits(ev, plain) and fences_intact(ew, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. argument checks
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    n = 64
    p, e = inputs(4 * 256 + 4)
    pw, pv = fenced(p[:n + 4])
    ew, ev = fenced(e[:n + 4])
    sw, sv = fenced(n + 4, torch.bfloat16)
    before = [t.clone() for t in (pw, ew, sw)]
    rec = make_record(1.0, 0)
    off_rec = torch.zeros(_lib.CLIP_RECORD_WORDS * 4 + 2, dtype=torch.uint8, device="cuda")[2:]
    assert ema_update(pv, ev, 6, 0.5, check=False) == ERR_ALIGN                         # n % 4 != 0
    assert ema_update(pv, ev, 0, 0.5, check=False) == ERR_ARG
    assert ema_update(pv, ev, -4, 0.5, check=False) == ERR_ARG
    assert ema_update(None, ev, n, 0.5, check=False) == ERR_ARG                         # NULL p
    assert ema_update(pv, None, n, 0.5, check=False) == ERR_ARG
    assert ema_update(pv[1:], ev, n, 0.5, check=False) == ERR_ALIGN                     # a pointer 4 bytes off the 16-byte grid
    assert ema_update(pv, ev[1:], n, 0.5, rec, check=False) == ERR_ALIGN
    assert ema_update(pv, ev, n, 0.5, off_rec, check=False) == ERR_ALIGN                # the record off the 4-byte grid
    assert ema_swap(pv, ev, sv, 6, check=False) == ERR_ALIGN
    assert ema_swap(pv, ev, sv, 0, check=False) == ERR_ARG
    assert ema_swap(None, ev, sv, n, check=False) == ERR_ARG
    assert ema_swap(pv, None, None, n, check=False) == ERR_ARG
    assert ema_swap(pv[1:], ev, sv, n, check=False) == ERR_ALIGN
    assert ema_swap(pv, ev[1:], None, n, check=False) == ERR_ALIGN
    assert ema_swap(pv, ev, sv[1:], n, check=False) == ERR_ALIGN                        # the shadow 2 bytes off its 8-byte grid
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip((pw, ew, sw), before))                   # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the swap
# ---------------------------------------------------------------------------------------------------------------------------------
def check_swap(p, e, with_shadow):
    n = len(p)
    pw, pv = fenced(p)
    ew, ev = fenced(e)
    sw, sv = fenced(n, torch.bfloat16) if with_shadow else (None, None)
    ema_swap(pv, ev, sv, n)
    assert np.array_equal(pv.cpu().numpy().view(np.uint32), e.view(np.uint32))          # p holds the old average, every bit
    assert np.array_equal(ev.cpu().numpy().view(np.uint32), p.view(np.uint32))          # and the average the old p
    if with_shadow:
        got, want = sv.view(torch.int16).cpu().numpy().view(np.uint16), EM.bf16_bits(e)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, [(hex(int(e.view(np.uint32)[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
        first = sv.clone()
    ema_swap(pv, ev, sv, n)                                                             # twice: the identity on all three buffers
    assert np.array_equal(pv.cpu().numpy().view(np.uint32), p.view(np.uint32))
    assert np.array_equal(ev.cpu().numpy().view(np.uint32), e.view(np.uint32))
    if with_shadow:
        assert np.array_equal(sv.view(torch.int16).cpu().numpy().view(np.uint16), EM.bf16_bits(p))
        ema_swap(pv, ev, sv, n)
        assert same_bits(sv, first)                                                     # (and the third call writes the first's shadow)
        assert fences_intact(sw, n)
    assert fences_intact(pw, n) and fences_intact(ew, n)


@pytest.mark.parametrize("with_shadow", [True, False], ids=["shadow", "no_shadow"])
@pytest.mark.parametrize("n", EM.SIZES)
def test_swap_exchanges_exactly_rounds_the_shadow_like_the_model_and_twice_is_the_identity(n, with_shadow):
    edge = EM.bf16_edge_values()
    p, e = inputs(n)
    if n == 4:                      # four elements at a time: every edge value passes through the shadow, on either side
        for k in range(0, len(edge), 4):
            check_swap(p.copy(), edge[k:k + 4].copy(), with_shadow)
            check_swap(edge[k:k + 4].copy(), e.copy(), with_shadow)
        return
    p, e = p.copy(), e.copy()
    e[:len(edge)] = edge            # ties, +-0, subnormals, the largest finite value, inf: at the start ...
    e[-len(edge):] = edge           # ... and in the last elements (for the largest n: the grid-stride loop's second trip)
    p[7:7 + len(edge)] = edge[::-1]
    check_swap(p, e, with_shadow)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the store
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


def build(mode="bf16", **over):
    cfg = tiny_config(compute_dtype=mode, deterministic=True, learning_rate=1e-3, drop_rate=0.0, **over)
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16 if mode == "bf16" else torch.float32)
    m.eval()
    m.trainer_ref = StubTrainer()
    return m


def step(m, b):
    """One training step; returns the loss (device tensor)."""
    m.store.zero_grad()
    loss = m.training_step(b)
    loss.backward()
    m.store.optimizer_step(max_steps=20, lr_factor=1.0)
    return loss.detach().clone()


def trainable(st):
    return st.flat[:st.trainable_end].cpu().numpy().copy()


@pytest.mark.parametrize("decay,warmup,want_w", [(0.5, False, [0.5, 0.5, 0.5]), (0.9, True, [9.0 / 11.0, 9.0 / 12.0, 9.0 / 13.0])],
                         ids=["decay0.5", "decay0.9_warmup"])
def test_store_averages_three_steps_inside_the_accumulated_bound(decay, warmup, want_w):
    b = to_dev(tiny_batch())
    m = build(ema_decay=decay, ema_warmup=warmup)
    st = m.store
    assert st.ema is None and st.ema_updates == 0                       # nothing is allocated before the first step
    snaps, ws = [trainable(st)], []
    for k in range(3):
        step(m, b)
        torch.cuda.synchronize()
        snaps.append(trainable(st))
        ws.append(config.ema_weight(decay, st.ema_updates, warmup))
    assert st.ema_updates == 3 and st.step_count == 3
    assert ws == [float(np.float32(x)) for x in want_w]
    assert st.ema.dtype == torch.float32 and st.ema.numel() == st.trainable_end
    got = st.ema.cpu().numpy().astype(np.float64)
    E, B = EM.accumulate(snaps, [np.float32(x) for x in ws])
    err = np.abs(got - E)
    moved = snaps[3] != snaps[0]
    print(f"decay {decay}: {int(moved.sum())} of {moved.size} elements moved; worst |ema - E| / budget = "
          f"{float(np.max(err[B > 0] / B[B > 0])):.3f}")
    assert moved.sum() > 1000                                            # (the steps moved the weights: the check is not vacuous)
    assert (err <= B).all(), float(np.max(err[B > 0] / B[B > 0]))
    assert not np.array_equal(st.ema.cpu().numpy(), snaps[0]) and not np.array_equal(st.ema.cpu().numpy(), snaps[3])
    # state dict: the trainable parameters under their names, the frozen / never-used ones absent
    sd = st.ema_state_dict()
    live = {n for g in st.groups[:6] for n, _ in g}
    dead = {n for g in st.groups[6:] for n, _ in g}
    assert set(sd) == live and dead and not dead & set(sd) and live | dead == {n for n, _ in m.named_parameters()}
    host = st.ema.cpu()
    for n, p in m.named_parameters():
        if n in live:
            o = st.offset[id(p)]
            assert sd[n].device.type == "cpu" and sd[n].dtype == torch.float32 and sd[n].shape == p.shape
            assert torch.equal(sd[n].reshape(-1), host[o:o + p.numel()]), n
    # and back: a fresh store takes the average and the count; a missing name or another shape is a ValueError
    m2 = build(ema_decay=decay, ema_warmup=warmup)
    m2.store.load_ema_state_dict(sd, 3)
    assert torch.equal(m2.store.ema, st.ema) and m2.store.ema_updates == 3
    name = sorted(live)[0]
    with pytest.raises(ValueError, match="no entry"):
        m2.store.load_ema_state_dict({k: v for k, v in sd.items() if k != name}, 3)
    with pytest.raises(ValueError, match="shape"):
        m2.store.load_ema_state_dict(dict(sd, **{name: torch.zeros(3, 5, 7)}), 3)
    assert torch.equal(m2.store.ema, st.ema)


def test_update_in_backward_gives_the_average_of_the_plain_route():
    from m3ae_amd.ddp import FlatGradReducer
    b = to_dev(tiny_batch())

    def run(in_backward):
        m = build(ema_decay=0.5, ema_warmup=False)
        red = FlatGradReducer(m.store, bucket_bytes=64 << 10, tail_bytes=8 << 10, update_in_backward=in_backward)
        assert red.world == 1
        red.attach()
        early = []
        try:
            for _ in range(3):
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
        return m.store, early
    plain, _ = run(False)
    fused, early = run(True)
    assert max(early[1:]) > 0                                            # (buckets were stepped, and averaged, under backward)
    assert torch.equal(plain.flat, fused.flat) and torch.equal(plain.ema, fused.ema)
    assert plain.ema_updates == fused.ema_updates == 3
    assert not torch.equal(plain.ema, plain.flat[:plain.trainable_end])


def test_a_step_the_guard_skips_leaves_the_average_but_consumes_its_warmup_tick():
    b = to_dev(tiny_batch())
    m = build(ema_decay=0.9, ema_warmup=True, gradient_clip_val=1.0)
    st = m.store
    step(m, b)
    flat, ema = st.flat.clone(), st.ema.clone()
    st.zero_grad()
    m.training_step(b).backward()
    st.grad[5] = float("inf")
    st.optimizer_step(max_steps=20, lr_factor=1.0)
    torch.cuda.synchronize()
    assert st.grad_stats()["skipped"] and torch.equal(st.flat, flat) and torch.equal(st.ema, ema)
    assert st.ema_updates == 2 and st.step_count == 2
    step(m, b)
    assert st.ema_updates == 3 and not torch.equal(st.ema, ema)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. evaluation round trip
# ---------------------------------------------------------------------------------------------------------------------------------
def device_copies(m):
    """Every device buffer a forward or backward pass reads weights from: the fp32 masters, the bf16 shadow, and per GEMM weight unit
    the transposed copy and the tiled copies of the shadow and of the transpose."""
    st = m.store
    out = {"flat": st.flat, "shadow": st.shadow}
    for i, u in enumerate(st.units):
        out[f"t{i}"] = getattr(u, "m3ae_t", None)
        out[f"tt{i}"] = getattr(u, "m3ae_tt", None)
        out[f"tb{i}"] = u.m3ae_tb if isinstance(u, PackedParam) else getattr(getattr(u, "m3ae_c", None), "m3ae_tb", None)
    return {k: v for k, v in out.items() if v is not None}


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_evaluation_on_the_average_and_back_bit_for_bit(mode):
    b = to_dev(tiny_batch())
    over = dict(ema_decay=0.5, ema_warmup=False)
    m, twin = build(mode, **over), build(mode, **over)
    for _ in range(3):
        step(m, b)
        step(twin, b)                                   # the run that never enters the context
    st = m.store
    assert torch.equal(st.flat, twin.store.flat) and torch.equal(st.ema, twin.store.ema)
    bufs = device_copies(m)
    assert ("shadow" in bufs) == (mode == "bf16") and (len(bufs) > 2) == (mode == "bf16")
    before = {k: v.clone() for k, v in bufs.items()}
    ema_before = st.ema.clone()
    raw_sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    avg_sd = st.ema_state_dict()
    m.set_task()
    twin.set_task()
    with torch.no_grad():
        raw_logits = m(b)["vqa_logits"].float().clone()
    with st.ema_weights() as inside:
        assert inside is st and not torch.is_grad_enabled()
        assert torch.equal(st.flat[:st.trainable_end], ema_before) and torch.equal(st.ema, before["flat"][:st.trainable_end])
        logits = m(b)["vqa_logits"].float().clone()
        with pytest.raises(RuntimeError, match="ema_weights"):
            st.optimizer_step(max_steps=20, lr_factor=1.0)
        with pytest.raises(RuntimeError, match="ema_weights"):
            st.update_apply(dict(ema_w=0.5))
        with pytest.raises(RuntimeError, match="ema_weights"):
            st.update_range(0, 64, 0, dict(ema_w=0.5))
        with pytest.raises(RuntimeError, match="re-entrant"):
            with st.ema_weights():
                pass
    assert torch.is_grad_enabled() and st.step_count == 3 and st.ema_updates == 3
    assert not torch.equal(logits, raw_logits)
    # a second model of the same config with the averaged weights loaded over the first one's: the same logits, bit for bit
    other = build(mode, **over)
    other.load_state_dict(dict(raw_sd, **avg_sd), strict=False)
    other.store.sync_shadows()
    other.set_task()
    with torch.no_grad():
        want = other(b)["vqa_logits"].float()
    assert torch.equal(logits, want)
    assert torch.equal(other.store.flat[:st.trainable_end], ema_before)
    # back outside: every buffer as before
    torch.cuda.synchronize()
    for k, v in device_copies(m).items():
        assert same_bits(v, before[k]), k
    assert torch.equal(st.ema, ema_before)
    # an exception inside the context still swaps back
    with pytest.raises(KeyError):
        with st.ema_weights():
            raise KeyError("inside")
    for k, v in device_copies(m).items():
        assert same_bits(v, before[k]), k
    assert torch.equal(st.ema, ema_before)
    with st.ema_weights():                              # (and the context opens again afterwards)
        pass
    # the fourth step: the loss bits, the weights and the average of the run that never entered the context
    l_a, l_b = step(m, b), step(twin, b)
    torch.cuda.synchronize()
    assert same_bits(l_a.float().reshape(1), l_b.float().reshape(1))
    assert torch.equal(st.flat, twin.store.flat) and torch.equal(st.ema, twin.store.ema)
    if mode == "bf16":
        assert torch.equal(st.shadow, twin.store.shadow)


def test_ema_weights_without_an_average_raises():
    m = build(ema_decay=0.0)
    with pytest.raises(RuntimeError, match="no average"):
        with m.store.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="no average"):
        m.store.ema_state_dict()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. key off: the step's calls are what they are without the feature
# ---------------------------------------------------------------------------------------------------------------------------------
def test_key_off_never_reaches_an_ema_entry_point(monkeypatch):
    b = to_dev(tiny_batch())
    off, on = build(ema_decay=0.0), build(ema_decay=0.5)
    L = _lib.lib()
    counts = {}

    class Counting:
        """The loaded library with the m3ae_ema_* look-ups counted (every caller reaches its entry points through _lib.lib())."""
        def __getattr__(self, name):
            if name.startswith("m3ae_ema_"):
                counts[name] = counts.get(name, 0) + 1
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Counting())
    step(off, b)
    step(off, b)
    assert counts == {} and off.store.ema is None and off.store.ema_updates == 0
    assert "ema_w" not in off.store.begin_update(max_steps=20, lr_factor=1.0)
    step(on, b)
    segments = sum(1 for a, e in on.store.segments[:6] if min(e, on.store.trainable_end) > a)
    assert counts == {"m3ae_ema_update": segments} and on.store.ema is not None        # one launch per optimizer range


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. trainer: evaluation on the average, checkpoints, resume, load_ema
# ---------------------------------------------------------------------------------------------------------------------------------
TINY = ("image_size=64 hidden_size=128 num_heads=2 num_top_layer=2 input_image_embed_size=128 input_text_embed_size=128 "
        "vocab_size=1000 vit_width=128 vit_layers=3 text_hidden=128 text_layers=2 text_heads=2 text_inter=512").split()


def make_trainer(tmp_path, tag, *extra):
    from m3ae_amd import trainer
    dev = torch.device("cuda", 0)
    argv = (["with", "data_root=synthetic", "num_gpus=1", "num_nodes=1", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta",
             "per_gpu_batchsize=4", "batch_size=4", "max_steps=2", "deterministic=True", "drop_rate=0.0", "learning_rate=0.001",
             "ema_decay=0.5", f"log_dir={tmp_path / tag}", "seed=2"] + TINY + list(extra))
    cfg = trainer.config_mod.parse_cli(argv)
    torch.manual_seed(cfg["seed"])
    model = trainer.build_model(cfg, "cls", dev)
    for mod in model.modules():                          # RoBERTa's own p = 0.1 too: validation leaves the model in train mode
        if hasattr(mod, "drop_rate"):
            mod.drop_rate = 0.0
    dm = trainer.SyntheticDataModule(cfg, 0, 1, dev, pool=1, train_samples=16, val_samples=8)
    return trainer.Trainer(cfg, model, dm, 0, 1, dev, log_every=1), model, cfg


def host_pass(tr, model):
    """The monitored quantity as Trainer.validate forms it on the host, over the weights as they stand."""
    from m3ae_amd import trainer
    model.eval()
    tot, cnt = torch.zeros((), device="cuda"), 0
    with torch.no_grad():
        for batch in tr.dm.val_batches():
            model.set_task()
            ret = model(batch, test=True)
            s, n = trainer.vqa_score(ret["vqa_logits"], ret["vqa_targets"])
            tot += s
            cnt += n
    model.train()
    return (torch.stack([tot, torch.tensor(float(cnt), device="cuda")])[0] / float(cnt)).item(), ret["vqa_logits"].float().clone()


def test_trainer_validates_saves_resumes_and_loads_the_average(tmp_path, capsys):
    import os
    from m3ae_amd import trainer
    tr, model, cfg = make_trainer(tmp_path, "run")
    assert tr.weights_only and tr.ema_eval
    out = tr.fit()
    torch.cuda.synchronize()
    st = model.store
    assert out["global_step"] == 2 and st.ema_updates == 2
    assert "val/the_metric (ema)" in capsys.readouterr().err
    raw = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    avg = st.ema_state_dict()
    assert any(not torch.equal(avg[k], raw[k]) for k in avg)
    for name in ("best.ckpt", "last.ckpt"):              # weights-only checkpoints carry the average too
        ck = torch.load(os.path.join(tr.ckpt_dir, name), map_location="cpu", weights_only=False)
        assert "optimizer_states" not in ck and ck["ema_updates"] == 2
        assert set(ck["state_dict"]) == set(raw) and all(torch.equal(ck["state_dict"][k], raw[k]) for k in raw)       # the raw weights
        assert set(ck["ema_state_dict"]) == set(avg) and all(torch.equal(ck["ema_state_dict"][k], avg[k]) for k in avg)
    tr.weights_only = False
    full = torch.load(tr.save("full.ckpt"), map_location="cpu", weights_only=False)
    assert "optimizer_states" in full and full["ema_updates"] == 2 and set(full["ema_state_dict"]) == set(avg)
    best = os.path.join(tr.ckpt_dir, "best.ckpt")
    # validate(): the value of a host-side pass inside ema_weights(), and `best` was chosen by it
    with st.ema_weights():
        by_hand, avg_logits = host_pass(tr, model)
    raw_value, raw_logits = host_pass(tr, model)
    assert not torch.equal(avg_logits, raw_logits)
    assert tr.validate() == by_hand == out["best"] and tr.validated_on_ema
    assert tr.test() == by_hand
    # ema_eval=False: the same run, validated on the raw weights
    capsys.readouterr()
    tr_raw, model_raw, _ = make_trainer(tmp_path, "raw", "ema_eval=False")
    out_raw = tr_raw.fit()
    torch.cuda.synchronize()
    assert torch.equal(model_raw.store.flat, st.flat) and torch.equal(model_raw.store.ema, st.ema)
    assert "(ema)" not in capsys.readouterr().err
    assert tr_raw.validate() == raw_value == out_raw["best"] and not tr_raw.validated_on_ema
    ck = torch.load(os.path.join(tr_raw.ckpt_dir, "last.ckpt"), map_location="cpu", weights_only=False)
    assert ck["ema_updates"] == 2 and all(torch.equal(ck["ema_state_dict"][k], avg[k]) for k in avg)
    # resume: the average bit for bit, and the count
    tr2, model2, _ = make_trainer(tmp_path, "second")
    assert model2.store.ema is None
    tr2.resume(best)
    assert torch.equal(model2.store.ema, st.ema) and model2.store.ema_updates == 2
    assert torch.equal(model2.store.flat, st.flat)
    assert tr2.validate() == by_hand
    # a checkpoint without the average: it starts from the loaded weights, and the log says so
    plain = str(tmp_path / "plain.ckpt")
    torch.save({k: v for k, v in ck.items() if not k.startswith("ema_")}, plain)
    tr3, model3, _ = make_trainer(tmp_path, "third")
    capsys.readouterr()
    tr3.resume(plain)
    assert "no ema_state_dict" in capsys.readouterr().err
    assert torch.equal(model3.store.ema, model3.store.flat[:model3.store.trainable_end]) and model3.store.ema_updates == 0
    assert torch.equal(model3.store.flat, st.flat)
    # load_path + load_ema: a model with the averaged weights; without the key in the file: ValueError
    loaded = trainer.build_model(dict(cfg, load_path=best, load_ema=True), "cls", torch.device("cuda", 0))
    assert torch.equal(loaded.store.flat[:st.trainable_end], st.ema) and torch.equal(loaded.store.flat[st.trainable_end:], st.flat[st.trainable_end:])
    unaveraged = trainer.build_model(dict(cfg, load_path=best, load_ema=False), "cls", torch.device("cuda", 0))
    assert torch.equal(unaveraged.store.flat, st.flat)
    with pytest.raises(ValueError, match="ema_state_dict"):
        trainer.build_model(dict(cfg, load_path=plain, load_ema=True), "cls", torch.device("cuda", 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. refusal
# ---------------------------------------------------------------------------------------------------------------------------------
def test_graphed_step_refuses_ema_decay():
    from m3ae_amd.graph import GraphedStep
    m = build(ema_decay=0.5)
    with pytest.raises(ValueError, match="ema_decay"):
        GraphedStep(m, to_dev(tiny_batch()), 10)
    assert m.store.step_count == 0 and m.store.ema is None
