"""GPU: gradient clipping by global norm with the non-finite step guard (csrc/gradnorm.hip, m3ae_adamw_clip, ParamStore, trainer).

Bounds.  The square of an fp32 value is exact in float64 and only the adds of m3ae_sumsq_segments round, so for any summation order
|got - exact| <= (len - 1) * 2^-53 * exact (to first order; the tests allow len * 2^-53); with small integers every partial sum is
an integer below 2^53 and the result is exact.  m3ae_clip_finalize rounds norm and coef to fp32 once (2^-24 relative) behind a
handful of float64 operations: 2^-23 relative covers both.  Everything the AdamW kernel does with the factor is compared bit for
bit against m3ae_adamw itself."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from m3ae_amd import _lib, gradnorm, ops, synth  # noqa: E402
from m3ae_amd.modules import M3AETransformerSS  # noqa: E402
from oracle_util import tiny_batch, tiny_config  # noqa: E402
import gradnorm_model as GM  # noqa: E402

P = gradnorm.PIECE
FENCE = 64            # elements on either side of every buffer a kernel writes or reads
SENTINEL = -777.0
U = 2.0 ** -53


@pytest.fixture(autouse=True)
def _deterministic_mode_off_afterwards():
    yield
    ops.set_deterministic(False)


def vp(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def fenced(n, dtype, fill=SENTINEL):
    """(whole, view): `view` is n elements with FENCE elements of `fill` on either side (the view stays 256-byte aligned)."""
    whole = torch.full((n + 2 * FENCE,), fill, dtype=dtype, device="cuda")
    return whole, whole[FENCE:FENCE + n]


def fences_intact(whole, n, fill=SENTINEL):
    f = torch.full((FENCE,), fill, dtype=whole.dtype, device="cuda")
    return torch.equal(whole[:FENCE], f) and torch.equal(whole[FENCE + n:], f)


def run_sumsq(xview, n, segs):
    """m3ae_sumsq_segments through the binding with the host's piece table; output and workspace in fenced buffers."""
    pieces, ptr = gradnorm.piece_table(segs)
    assert GM.check_piece_table(segs, pieces, ptr, P)
    L = _lib.lib()
    npieces, nseg = len(pieces), len(segs)
    ws_bytes = L.m3ae_sumsq_workspace_bytes(npieces)
    assert ws_bytes == 8 * max(npieces, 1)
    ws_whole, ws = fenced(ws_bytes // 8, torch.float64)
    out_whole, out = fenced(nseg, torch.float64)
    pieces_d = torch.from_numpy(pieces if npieces else np.zeros((1, 2), np.int64)).cuda()
    ptr_d = torch.from_numpy(ptr).cuda()
    _lib.check(L.m3ae_sumsq_segments(vp(xview), n, vp(pieces_d), npieces, vp(ptr_d), nseg, vp(out), vp(ws), ws_bytes, stream()),
               "m3ae_sumsq_segments")
    torch.cuda.synchronize()
    assert fences_intact(ws_whole, ws_bytes // 8) and fences_intact(out_whole, nseg)
    return out.cpu().numpy().copy()


def poisoned_buffer(segs, n, values):
    """n fp32 elements, nan outside every segment and in both fences; values(k, len) fills segment k."""
    host = np.full(n, np.nan, dtype=np.float32)
    for k, (b, e) in enumerate(segs):
        host[b:e] = values(k, e - b)
    whole, x = fenced(n, torch.float32, fill=float("nan"))
    x.copy_(torch.from_numpy(host))
    return host, x, whole


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. m3ae_sumsq_segments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sumsq_small_integers_are_exact_with_everything_else_poisoned():
    """Lengths 0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, P - 1, P, P + 1, 3 P + 7 with begins at 0, 1, 2, 3 mod 4 in ONE table: tiny
    and multi-piece segments side by side; every element outside a segment is nan, so one stray read shows as a nan sum."""
    segs, n = GM.shape_segments(P)
    assert sorted({e - b for b, e in segs}) == sorted(GM.shape_lengths(P)) and {b % 4 for b, _ in segs} == {0, 1, 2, 3}
    rng = np.random.default_rng(11)
    host, x, whole = poisoned_buffer(segs, n, lambda k, ln: rng.integers(-8, 9, size=ln).astype(np.float32))
    got = run_sumsq(x, n, segs)
    want = np.array([int((host[b:e].astype(np.int64) ** 2).sum()) for b, e in segs], dtype=np.float64)
    assert want[np.array([e - b == 0 for b, e in segs])].tolist() == [0.0, 0.0]
    print("segments", len(segs), "elements", n, "max sum", want.max())
    assert np.array_equal(got, want), [(s, g, w) for s, g, w in zip(segs, got, want) if g != w]


def test_sumsq_bound_tiny_and_huge_values_and_two_runs_bit_equal():
    segs, n = GM.shape_segments(P)
    rng = np.random.default_rng(12)
    lens = [e - b for b, e in segs]
    tiny_k, huge_k = lens.index(3 * P + 7), lens.index(P + 1)        # a multi-piece segment of 1e-25, a two-piece segment of 3e19
    tiny_k2, huge_k2 = lens.index(257), lens.index(65)

    def values(k, ln):
        if k in (tiny_k, tiny_k2):
            return np.full(ln, 1e-25, dtype=np.float32)
        if k in (huge_k, huge_k2):
            return np.full(ln, 3e19, dtype=np.float32)
        return (rng.standard_normal(ln) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)

    host, x, whole = poisoned_buffer(segs, n, values)
    got = run_sumsq(x, n, segs)
    again = run_sumsq(x, n, segs)
    assert got.tobytes() == again.tobytes()                            # a function of (x, table) alone
    ref = GM.segment_sumsq(host, segs)
    for k, ((b, e), g, r) in enumerate(zip(segs, got, ref)):
        err, bound = abs(g - r), (e - b) * U * r
        if k in (tiny_k, tiny_k2, huge_k, huge_k2):
            print("segment", k, "len", e - b, "got", g, "ref", r, "err", err, "bound", bound)
        assert math.isfinite(g) and err <= bound, (k, e - b, g, r, err, bound)
    for k in (tiny_k, tiny_k2):
        assert got[k] > 0.0                                            # fp32 accumulation would have given 0
    for k in (huge_k, huge_k2):
        assert got[k] > 3.4e38                                         # ... and inf here


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. m3ae_clip_finalize
# ---------------------------------------------------------------------------------------------------------------------------------
def new_record():
    whole, rec = fenced(_lib.CLIP_RECORD_WORDS, torch.float32, fill=0.0)
    return whole, rec


def read_record(rec):
    r = rec.cpu()
    c = r.view(torch.int32)
    return dict(norm=r[_lib.CLIP_NORM].item(), coef=r[_lib.CLIP_COEF].item(), skip=int(c[_lib.CLIP_SKIP]),
                counters=(int(c[_lib.CLIP_STEPS]), int(c[_lib.CLIP_CLIPPED_STEPS]), int(c[_lib.CLIP_SKIPPED_STEPS])),
                coef_bits=int(c[_lib.CLIP_COEF]))


def finalize(sums, grad_scale, max_norm, rec):
    seg = torch.tensor(list(sums), dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().m3ae_clip_finalize(vp(seg), seg.numel(), grad_scale, max_norm, vp(rec), stream()), "m3ae_clip_finalize")
    torch.cuda.synchronize()
    return read_record(rec)


ONE_BITS = 0x3F800000


@pytest.mark.parametrize("nseg", [1, 2, 64, 65, 663])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125, -0.5])
def test_finalize_norm_and_coefficient(nseg, grad_scale):
    rng = np.random.default_rng(nseg)
    sums = (rng.random(nseg) * 10.0 ** rng.integers(-6, 7, size=nseg)).tolist()
    mnorm, _, _, _ = GM.finalize(sums, grad_scale, 1.0)
    for max_norm in (mnorm * 4.0, float("inf"), mnorm * 0.37, 1e-3 * mnorm):
        whole, rec = new_record()
        got = finalize(sums, grad_scale, max_norm, rec)
        norm, coef, skip, counters = GM.finalize(sums, grad_scale, max_norm)
        print("nseg", nseg, "scale", grad_scale, "max_norm", max_norm, "got", got, "model", norm, coef)
        assert got["skip"] == 0 == skip and got["counters"] == counters
        assert abs(got["norm"] - norm) <= 2.0 ** -23 * norm
        if max_norm >= mnorm * 4.0:
            assert got["coef_bits"] == ONE_BITS and counters[1] == 0        # inside the bound: exactly 1.0f
        else:
            assert abs(got["coef"] - coef) <= 2.0 ** -23 * coef and got["coef"] < 1.0 and counters[1] == 1
        assert fences_intact(whole, _lib.CLIP_RECORD_WORDS, 0.0)


@pytest.mark.parametrize("poison", [float("inf"), float("-inf"), float("nan")])
def test_one_non_finite_element_sets_skip(poison):
    segs = [(1, 70), (80, 80 + P + 3), (80 + P + 10, 80 + P + 15)]
    n = 80 + P + 20
    rng = np.random.default_rng(5)
    host, x, whole = poisoned_buffer(segs, n, lambda k, ln: rng.standard_normal(ln).astype(np.float32))
    x[80 + P + 1] = poison                                             # in the second piece of the middle segment
    got = run_sumsq(x, n, segs)
    assert math.isfinite(got[0]) and math.isfinite(got[2]) and not math.isfinite(got[1])
    for max_norm in (1.0, float("inf")):
        _, rec = new_record()
        r = finalize(got.tolist(), 1.0, max_norm, rec)
        assert r["skip"] == 1 and r["coef"] == 0.0 and r["coef_bits"] == 0 and not math.isfinite(r["norm"])
        assert r["counters"] == (1, 0, 1)


def test_finalize_counters_over_a_scripted_sequence():
    script = [([1.0, 3.0], 1.0, 10.0),                 # norm 2, inside
              ([4.0, 12.0], 1.0, 2.0),                 # norm 4, clipped
              ([1.0, float("inf")], 1.0, 2.0),         # skipped
              ([16.0], 0.125, 0.25),                   # norm 0.5, clipped
              ([float("nan"), 1.0], 1.0, float("inf"))]  # skipped
    whole, rec = new_record()
    counters = (0, 0, 0)
    for sums, gs, mx in script:
        got = finalize(sums, gs, mx, rec)
        norm, coef, skip, counters = GM.finalize(sums, gs, mx, counters)
        assert got["counters"] == counters and got["skip"] == skip
        if not skip:
            assert got["norm"] == np.float32(norm) and got["coef"] == np.float32(coef)
    assert counters == (5, 2, 2)
    assert fences_intact(whole, _lib.CLIP_RECORD_WORDS, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. m3ae_adamw_clip against m3ae_adamw, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
HP = dict(lr=3e-3, b1=0.9, b2=0.98, eps=1e-8, wd=0.01, step=3)


def make_record(coef, skip):
    rec = torch.zeros(_lib.CLIP_RECORD_WORDS, dtype=torch.float32, device="cuda")
    rec[_lib.CLIP_COEF] = float(np.float32(coef))
    rec.view(torch.int32)[_lib.CLIP_SKIP] = int(skip)
    return rec


def adamw_state(n, shadow, seed):
    g = torch.Generator().manual_seed(seed)
    st = {}
    for name, scale in (("p", 1.0), ("g", 0.1), ("m", 0.05)):
        st[name] = fenced(n, torch.float32)
        st[name][1].copy_(torch.randn(n, generator=g) * scale)
    st["v"] = fenced(n, torch.float32)
    st["v"][1].copy_(torch.rand(n, generator=g) * 0.01)
    if shadow:
        st["s"] = fenced(n, torch.bfloat16)
        st["s"][1].copy_(st["p"][1])
    return st


def run_adamw(st, n, grad_scale, hyper_dev, record=None):
    L = _lib.lib()
    sh = vp(st["s"][1]) if "s" in st else None
    hd = vp(hyper_dev) if hyper_dev is not None else None
    head = (vp(st["p"][1]), vp(st["g"][1]), vp(st["m"][1]), vp(st["v"][1]), sh, n, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"],
            HP["step"], grad_scale, hd)
    if record is None:
        _lib.check(L.m3ae_adamw(*head, stream()), "m3ae_adamw")
    else:
        _lib.check(L.m3ae_adamw_clip(*head, vp(record), stream()), "m3ae_adamw_clip")
    torch.cuda.synchronize()


def same_state(a, b, n):
    return all(torch.equal(a[k][0].view(torch.int16 if k == "s" else torch.int32), b[k][0].view(torch.int16 if k == "s" else torch.int32))
               for k in a) and all(fences_intact(a[k][0], n) for k in a)


@pytest.mark.parametrize("hyper", [False, True])
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("n", [4, 8, 1028])
def test_adamw_clip_equals_adamw_with_the_scaled_factor_and_skip_touches_nothing(n, shadow, hyper):
    hd = torch.tensor([2e-3, 1.7e-3], dtype=torch.float32, device="cuda") if hyper else None
    gs = 0.5
    # coef = 1: the bits of m3ae_adamw
    a, b = adamw_state(n, shadow, 1), adamw_state(n, shadow, 1)
    before = {k: v[0].clone() for k, v in a.items()}
    run_adamw(a, n, gs, hd)
    run_adamw(b, n, gs, hd, make_record(1.0, 0))
    assert same_state(a, b, n)
    assert not torch.equal(a["p"][0], before["p"]) and not torch.equal(a["m"][0], before["m"])      # (the step did something)
    # coef = 0.37: m3ae_adamw with grad_scale * 0.37 formed in fp32
    a, b = adamw_state(n, shadow, 2), adamw_state(n, shadow, 2)
    run_adamw(a, n, float(np.float32(gs) * np.float32(0.37)), hd)
    run_adamw(b, n, gs, hd, make_record(0.37, 0))
    assert same_state(a, b, n)
    # against the float32 model (an independent statement of the kernel; fused multiply-adds may differ in the last bits)
    ref = adamw_state(n, shadow, 2)
    mp, mm, mv = GM.adamw(ref["p"][1].cpu().numpy(), ref["g"][1].cpu().numpy(), ref["m"][1].cpu().numpy(), ref["v"][1].cpu().numpy(),
                          HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], HP["step"], np.float32(gs) * np.float32(0.37),
                          hyper=(2e-3, 1.7e-3) if hyper else None)
    assert np.allclose(b["p"][1].cpu().numpy(), mp, rtol=1e-5, atol=1e-7) and np.allclose(b["m"][1].cpu().numpy(), mm, rtol=1e-5, atol=1e-8)
    assert np.allclose(b["v"][1].cpu().numpy(), mv, rtol=1e-5, atol=1e-10)
    # skip = 1: nothing is touched, whatever the coefficient word holds
    for coef in (0.0, 1.0):
        a = adamw_state(n, shadow, 3)
        before = {k: (v[0].clone(), None) for k, v in a.items()}
        run_adamw(a, n, gs, hd, make_record(coef, 1))
        assert same_state(a, before, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. ParamStore and trainer
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


def build(**over):
    cfg = tiny_config(compute_dtype="bf16", deterministic=True, **over)
    m = M3AETransformerSS(cfg)
    synth.fill_deterministic(m)
    m.finalize("cuda", torch.bfloat16)
    m.eval()
    return m


def backward(m, b):
    m.store.zero_grad()
    m.training_step(b).backward()
    torch.cuda.synchronize()


def f64_norm(t):
    return math.sqrt(GM.exact_sumsq(t.detach().float().cpu().numpy()))


def state_of(st):
    return [t.clone() for t in (st.flat, st.exp_avg, st.exp_avg_sq, st.shadow) if t is not None]


def states_equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


class Counting:
    """The loaded library with the calls of the optimizer's entry points counted (everything reaches it through _lib.lib())."""
    NAMES = ("m3ae_adamw", "m3ae_adamw_clip", "m3ae_sumsq_segments", "m3ae_sumsq_workspace_bytes", "m3ae_clip_finalize")

    def __init__(self, L):
        self.L, self.counts = L, {n: 0 for n in self.NAMES}

    def __getattr__(self, name):
        fn = getattr(self.L, name)
        if name in self.NAMES:
            def counted(*a):
                self.counts[name] += 1
                return fn(*a)
            return counted
        return fn


def test_key_off_makes_todays_calls_and_key_on_the_clipped_chain(monkeypatch):
    b = to_dev(tiny_batch())
    off, on = build(), build(gradient_clip_val=1e30)
    assert off.store.clip_val() == 0.0 and on.store.clip_val() == 1e30
    for m in (off, on):      # first step outside the count: lazy buffers
        backward(m, b)
        m.store.adamw_step(max_steps=10, lr_factor=1.0)
    cnt = Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", cnt)
    for step in range(2):
        backward(off, b)
        off.store.adamw_step(max_steps=10, lr_factor=1.0)
    assert cnt.counts == {"m3ae_adamw": 12, "m3ae_adamw_clip": 0, "m3ae_sumsq_segments": 0, "m3ae_sumsq_workspace_bytes": 0,
                          "m3ae_clip_finalize": 0}, cnt.counts
    assert off.store._sums is None and off.store._clip_record is None        # nothing allocated
    cnt.counts = {n: 0 for n in cnt.NAMES}
    for step in range(2):
        backward(on, b)
        on.store.adamw_step(max_steps=10, lr_factor=1.0)
    assert cnt.counts == {"m3ae_adamw": 0, "m3ae_adamw_clip": 12, "m3ae_sumsq_segments": 2, "m3ae_sumsq_workspace_bytes": 0,
                          "m3ae_clip_finalize": 2}, cnt.counts
    torch.cuda.synchronize()
    # a bound far above the norm: coef == 1.0f, and three steps with the key equal three steps without it, bit for bit
    assert states_equal(state_of(off.store), state_of(on.store))
    s = on.store.grad_stats()
    assert s["coef"] == 1.0 and s["skipped"] is False and (s["steps"], s["clipped_steps"], s["skipped_steps"]) == (3, 0, 0)
    with pytest.raises(RuntimeError):
        off.store.grad_stats()


def test_two_trainer_steps_with_a_far_bound_equal_the_run_without_the_key(tmp_path, capfd):
    from m3ae_amd import trainer
    tiny = ("image_size=64 hidden_size=128 num_heads=2 num_top_layer=2 input_image_embed_size=128 input_text_embed_size=128 "
            "vocab_size=1000 vit_width=128 vit_layers=3 text_hidden=128 text_layers=2 text_heads=2 text_inter=512").split()
    states, logs = {}, {}
    for tag, extra in (("off", []), ("on", ["gradient_clip_val=1e30"])):
        argv = (["with", "data_root=synthetic", "num_gpus=1", "num_nodes=1", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta",
                 "per_gpu_batchsize=4", "batch_size=8", "max_steps=2", "deterministic=True", "learning_rate=0.0005",
                 f"log_dir={tmp_path / tag}", "seed=2"] + tiny + extra)
        cfg = trainer.config_mod.parse_cli(argv)
        dev = torch.device("cuda", 0)
        torch.manual_seed(cfg["seed"])
        model = trainer.build_model(cfg, "cls", dev)
        dm = trainer.SyntheticDataModule(cfg, 0, 1, dev, train_samples=16, val_samples=4)
        out = trainer.Trainer(cfg, model, dm, 0, 1, dev, log_every=1).fit()
        torch.cuda.synchronize()
        assert out["global_step"] == 2
        states[tag] = state_of(model.store)
        logs[tag] = capfd.readouterr().err
        if tag == "on":
            s = model.store.grad_stats()
            assert (s["steps"], s["clipped_steps"], s["skipped_steps"]) == (2, 0, 0) and s["coef"] == 1.0 and s["norm"] > 0
    assert states_equal(states["off"], states["on"])
    assert "grad_norm" not in logs["off"] and "coef" not in logs["off"]                   # the log line is unchanged without the key
    assert logs["on"].count("grad_norm") == 2 and "coef 1.0000 skipped 0" in logs["on"]


def clipping_case(st, twin, tol=2.0 ** -23):
    """`st` and `twin`: two equal stores with equal gradient buffers.  Bound = half the measured norm; the reported norm against the
    float64 norm of the buffer; the step against m3ae_adamw on the twin at grad_scale = coef."""
    assert torch.equal(st.grad, twin.grad) and torch.equal(st.flat, twin.flat)
    ref = f64_norm(st.grad)                      # the whole buffer: the padding between parameters is zero
    measured = st.grad_norm()
    assert abs(measured - ref) <= st.grad.numel() * U * ref
    st.cfg["gradient_clip_val"] = measured / 2
    assert twin.clip_val() == 0.0
    st.adamw_step(max_steps=10, lr_factor=1.0)
    s = st.grad_stats()
    print("norm", s["norm"], "float64", ref, "coef", s["coef"])
    assert abs(s["norm"] - ref) <= tol * ref
    want = float(np.float32(measured / 2)) / (ref + 1e-6)           # the bound reaches the kernel as an fp32 argument
    assert abs(s["coef"] - want) <= tol * want and s["coef"] < 1.0
    assert s["skipped"] is False and s["clipped_steps"] == 1
    twin.adamw_step(max_steps=10, lr_factor=1.0, grad_scale=s["coef"])
    torch.cuda.synchronize()
    assert states_equal(state_of(st), state_of(twin))


def test_clipping_step_equals_plain_adamw_at_the_coefficient():
    b = to_dev(tiny_batch())
    m, twin = build(gradient_clip_val=1.0), build()
    assert twin.store.cfg is not m.store.cfg
    backward(m, b)
    backward(twin, b)
    before = m.store.flat.clone()
    clipping_case(m.store, twin.store)
    assert not torch.equal(m.store.flat, before)


def test_clipping_step_on_the_two_group_store_of_the_t5_head():
    """group_fn = param_group_of_decoder: two optimizer groups, four empty ones (no launch for them, with or without the record)."""
    from m3ae_amd.modules.t5 import T5ForConditionalGeneration
    from m3ae_amd.param_store import ParamStore, group_hparams_decoder, param_group_of_decoder
    stores = []
    for i in range(2):
        torch.manual_seed(4)
        m = T5ForConditionalGeneration(dict(d_model=512, d_kv=64, d_ff=2048, num_layers=1, num_decoder_layers=1, num_heads=8), 1100)
        st = ParamStore(m, tiny_config(compute_dtype="bf16", gradient_clip_val=1.0 if i == 0 else 0.0), "cuda", torch.bfloat16,
                        m.weight_units, group_fn=param_group_of_decoder, hparams_fn=group_hparams_decoder)
        assert [a == b for a, b in st.segments[:6]] == [False, False, True, True, True, True]
        g = torch.Generator().manual_seed(9)
        for _, p in st.groups[0] + st.groups[1]:
            p.grad.copy_(torch.randn(p.shape, generator=g) * 0.02)      # the views: the padding stays zero
        stores.append((m, st))
    clipping_case(stores[0][1], stores[1][1])


def test_guard_skips_a_non_finite_step_and_the_next_step_updates():
    b = to_dev(tiny_batch())
    m = build(gradient_clip_val=float("inf"))
    st = m.store
    backward(m, b)
    st.adamw_step(max_steps=10, lr_factor=1.0)                 # a normal step first: the moments are no longer zero
    backward(m, b)
    before = state_of(st)
    st.grad[st.grad_segments[3][0] + 1] = float("inf")      # an ordinary float value in one parameter's gradient
    count = st.step_count
    st.adamw_step(max_steps=10, lr_factor=1.0)
    torch.cuda.synchronize()
    assert states_equal(state_of(st), before)               # parameters, moments and shadows untouched
    s = st.grad_stats()
    assert s["skipped"] is True and s["coef"] == 0.0 and (s["steps"], s["clipped_steps"], s["skipped_steps"]) == (2, 0, 1)
    assert st.step_count == count + 1                       # the skipped step consumed its step number
    backward(m, b)
    st.adamw_step(max_steps=10, lr_factor=1.0)
    torch.cuda.synchronize()
    after = state_of(st)
    assert all(not torch.equal(x, y) for x, y in zip(after, before))
    assert all(torch.isfinite(t.float()).all() for t in after)
    s = st.grad_stats()
    assert s["skipped"] is False and s["coef"] == 1.0 and (s["steps"], s["clipped_steps"], s["skipped_steps"]) == (3, 0, 1)


def test_grad_norms_against_float64_per_parameter():
    b = to_dev(tiny_batch())
    m = build()
    backward(m, b)
    got = m.store.grad_norms()
    params = {n: p for n, p in m.named_parameters() if p.requires_grad}
    assert set(got) == set(params) and len(got) > 50
    for n, p in params.items():
        ref = f64_norm(p.grad)
        assert abs(got[n] - ref) <= p.numel() * U * ref, (n, got[n], ref)
    total = math.sqrt(math.fsum(GM.exact_sumsq(p.grad.float().cpu().numpy()) for p in params.values()))
    assert abs(m.store.grad_norm() - total) <= m.store.grad.numel() * U * total
    assert m.store._clip_record is None and m.store.exp_avg is None          # stand-alone: no step, no clipping state


def test_two_virtual_ranks_report_the_norm_of_the_averaged_gradient():
    """The set-up of test_gpu_model.py::test_two_virtual_ranks_equal_the_unsplit_global_batch_step: rank 0's buckets are recorded,
    rank 1's collective adds them, the reducer leaves the SUM in the buffer and 1 / world in grad_scale."""
    from m3ae_amd.ddp import FlatGradReducer
    full = to_dev(synth.synthetic_batch(4, text_len=32, image_size=64, vocab_size=1000, rank=0))

    def half(i):
        h = {}
        for k, v in full.items():
            if isinstance(v, torch.Tensor):
                h[k] = v[2 * i:2 * i + 2]
            elif isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
                h[k] = [t[2 * i:2 * i + 2] for t in v]
            elif isinstance(v, list):
                h[k] = v[2 * i:2 * i + 2]
            else:
                h[k] = v
        return h

    m = build(gradient_clip_val=float("inf"))
    other = torch.zeros_like(m.store.grad)
    phase = {"record": True}

    class Done:
        def wait(self):
            return None

    def collective(t):
        off = (t.data_ptr() - m.store.grad.data_ptr()) // 4
        if phase["record"]:
            other[off:off + t.numel()].copy_(t)
        else:
            t.add_(other[off:off + t.numel()])
        return Done()

    red = FlatGradReducer(m.store, bucket_bytes=64 << 10, tail_bytes=8 << 10, collective=collective, world=2)
    red.attach()
    try:
        for r in (0, 1):
            phase["record"] = r == 0
            m.store.zero_grad()
            m.training_step(half(r)).backward()
            red.finish()
    finally:
        red.detach()
    torch.cuda.synchronize()
    assert red.grad_scale == 0.5
    summed = f64_norm(m.store.grad)
    assert summed > 0
    m.store.adamw_step(max_steps=10, lr_factor=1.0, grad_scale=red.grad_scale)
    s = m.store.grad_stats()
    print("norm", s["norm"], "half of the summed buffer's", 0.5 * summed)
    assert abs(s["norm"] - 0.5 * summed) <= 2.0 ** -23 * 0.5 * summed and s["coef"] == 1.0 and s["skipped"] is False
