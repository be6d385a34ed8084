"""GPU: device-resident beam search (csrc/beam.hip) -- m3ae_beam_topk against a float64 reference and the order key's tie rule,
m3ae_beam_step / m3ae_beam_finalize against the numpy model of tests/beam_model.py array by array, and
T5ForConditionalGeneration.generate(beam_search="device") / generate_async against the host form and the CPU oracle.

tau (beam_model.tau): three correctly rounded fp32 operations on magnitudes up to M = max(1, |score|, max|x - m|) contribute
<= 1.5 ulp32(M), the log of a V-term fp32 sum <= (log2 V + 2) 2^-24 ~ 1e-6 at V = 32128; tau = 4 ulp32(M) + 2e-6 is that with
x2 to x3 headroom.  Indices are compared where the reference's neighbouring gaps exceed 2 tau; inputs are drawn from the next
seed until every rank qualifies."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_model as M  # noqa: E402
from m3ae_amd import _lib, ops  # noqa: E402
from oracle import m3ae_oracle as O  # noqa: E402
from oracle_util import canon_generated, gen_t5_weights, load_golden, tiny_batch, tiny_config  # noqa: E402

DEV = "cuda"


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. m3ae_beam_topk
# ---------------------------------------------------------------------------------------------------------------------------------
TOPK_SHAPES = [(1, 1, 9, 9), (3, 4, 9, 12), (2, 4, 1001, 1004), (3, 2, 1100, 1100), (2, 4, 32128, 32128), (1, 8, 4099, 4100)]


def padded(x, ld):
    """x [R, V] as a view of a [R, ld] buffer whose padding columns hold a value that would win every comparison."""
    buf = torch.full((x.shape[0], ld), 1e30, dtype=torch.float32, device=DEV)
    buf[:, :x.shape[1]] = cuda(x)
    return buf[:, :x.shape[1]]


def draw(B, nb, V, kind, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B * nb, V)) * 2.0).astype(np.float32)
    if kind == "first":
        bs = np.zeros((B, nb), dtype=np.float32)
        bs[:, 1:] = -1e9
    else:
        bs = rng.uniform(-30.0, 0.0, (B, nb)).astype(np.float32)
    return x, bs.reshape(-1)


@pytest.mark.parametrize("kind", ["first", "mid"])
@pytest.mark.parametrize("shape", TOPK_SHAPES, ids=lambda s: "B{}-nb{}-V{}-ld{}".format(*s))
def test_topk_matches_float64_reference(shape, kind):
    B, nb, V, ld = shape
    K = 2 * nb
    for seed in range(50):
        x, bs = draw(B, nb, V, kind, seed)
        vals, idx, spread = M.reference_topk(x, bs, B, nb, K + 1)
        if all(M.live_gaps_ok(vals[b], spread[b]) for b in range(B)):
            break
    else:
        raise AssertionError("no seed below 50 separates the reference's top 2 nb + 1 by 2 tau")
    xd, bd = padded(x, ld), cuda(bs)
    top_s, top_i = ops.beam_topk(xd, bd, B, nb)
    again_s, again_i = ops.beam_topk(xd, bd, B, nb)
    assert torch.equal(top_s, again_s) and torch.equal(top_i, again_i)
    s, i = top_s.cpu().numpy(), top_i.cpu().numpy()
    err = np.abs(s.astype(np.float64) - vals[:, :K])
    tol = np.array([[M.tau(vals[b, r], spread[b]) for r in range(K)] for b in range(B)])
    print(f"{shape} {kind}: seed {seed}, max |top_s - ref| / tau = {(err / tol).max():.3f}")
    assert (err <= tol).all(), (err / tol).max()
    assert np.array_equal(i, idx[:, :K])
    # every vocabulary split gives the same indices and the same fp32 candidates up to the lse's rounding
    for chunk in (256, 1000, 4096):
        cs, ci = ops.beam_topk(xd, bd, B, nb, chunk=chunk)
        assert np.array_equal(ci.cpu().numpy(), idx[:, :K]), chunk
        assert (np.abs(cs.cpu().numpy().astype(np.float64) - vals[:, :K]) <= tol).all(), chunk


def test_topk_tie_rule_equal_logits_and_collapsed_scores():
    """All logits of every row equal, and all beam scores -1e9 with random logits (every score rounds to exactly -1e9f, so a
    pre-selection by raw logit would pick other tokens): the order is the flat index."""
    for B, nb, V in ((2, 4, 1001), (1, 8, 4099), (3, 1, 9)):
        K = 2 * nb
        x = torch.full((B * nb, V), 0.75, dtype=torch.float32, device=DEV)
        s, i = ops.beam_topk(x, torch.zeros(B * nb, device=DEV), B, nb)
        assert i.cpu().tolist() == [list(range(K))] * B
        assert len(set(s.cpu().view(-1).tolist())) == 1
        x, _ = draw(B, nb, V, "mid", 3)
        s, i = ops.beam_topk(cuda(x), torch.full((B * nb,), -1e9, device=DEV), B, nb)
        assert i.cpu().tolist() == [list(range(K))] * B
        assert (s.cpu().numpy() == np.float32(-1e9)).all()


@pytest.mark.parametrize("chunk", [0, 1024])
def test_topk_tie_rule_across_chunk_boundaries(chunk):
    """Two equal maxima on either side of each internal chunk boundary, in two beams whose rows are identical (so the four
    candidates have one fp32 score): lower flat index first."""
    B, nb, V = 2, 4, 4099
    width = chunk or ops.BEAM_TOPK_CHUNK
    for edge in range(width, V, width):
        x = np.zeros((B * nb, V), dtype=np.float32)
        for b in range(B):
            for beam in (1, 3):
                x[b * nb + beam, edge - 1] = x[b * nb + beam, edge] = 5.0
        s, i = ops.beam_topk(cuda(x), torch.zeros(B * nb, device=DEV), B, nb, chunk=chunk)
        want = [1 * V + edge - 1, 1 * V + edge, 3 * V + edge - 1, 3 * V + edge]
        assert i.cpu()[:, :4].tolist() == [want] * B, edge
        assert i.cpu().tolist() == M.topk(x, np.zeros(B * nb, dtype=np.float32), B, nb)[1].tolist()
        assert len(set(s.cpu()[:, :4].reshape(-1).tolist())) == 1


def test_topk_nan_and_inf_keep_indices_in_range_and_distinct():
    B, nb, V = 2, 4, 1001
    x, bs = draw(B, nb, V, "mid", 5)
    x[1, 17], x[1, 500] = np.nan, -np.inf
    x[6, :] = -np.inf
    _, i = ops.beam_topk(cuda(x), cuda(bs), B, nb)
    i = i.cpu().numpy()
    assert ((i >= 0) & (i < nb * V)).all()
    assert all(len(set(row.tolist())) == 2 * nb for row in i)


def test_topk_unsupported_shapes():
    for B, nb, V in ((1, 9, 100), (1, 4, 8)):
        with pytest.raises(_lib.M3AEHipError, match="unsupported"):
            ops.beam_topk(torch.zeros(B * nb, V, device=DEV), torch.zeros(B * nb, device=DEV), B, nb,
                          ws=torch.empty(1 << 16, dtype=torch.int64, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. m3ae_beam_step / m3ae_beam_finalize against the numpy model
# ---------------------------------------------------------------------------------------------------------------------------------
STATE_ARRAYS = ("ids", "last_tok", "beam_scores", "order", "done", "n_hyp", "hyp_score", "hyp_len", "hyp_tok", "open_count", "err")


def assert_state_equal(dev, mod, where):
    assert dev.cur == mod.cur
    for name in STATE_ARRAYS:
        a, b = getattr(dev, name).cpu().numpy(), getattr(mod, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (name, where)      # bit for bit: fp32 beam scores, double hypothesis scores


@pytest.mark.parametrize("case", list(M.SCRIPTED), ids=lambda c: "V{}-nb{}-L{}-eos{}".format(*c))
def test_step_and_finalize_match_the_model(monkeypatch, case):
    """After every step every state array equals the model's (the step is fed the model's top_s / top_i, so no top-k rounding leaks
    in); finalize equals the model and the oracle.  All max_length - 1 steps run, so done samples are stepped too."""
    V, nb, ml, eos_bias = case
    B = M.SCRIPTED_B
    T1, T2 = M.tables(V, nb, ml, eos_bias, B, M.SCRIPTED[case])
    for lp, len_offset in ((1.0, 0), (0.7, 0), (1.0, 1), (0.7, 1)):
        dev = ops.BeamState(B, nb, ml, DEV)

        def on_step(st, cur_len, logits, bs_in, top_s, top_i, was_done):
            ops.beam_step(dev, cuda(top_s), cuda(top_i), V, cur_len, 1, 0, lp)
            assert_state_equal(dev, st, (case, lp, cur_len))

        mod = M.search(T1, T2, B, nb, ml, length_penalty=lp, len_offset=len_offset, on_step=on_step, stop_early=False)
        seq, length = ops.beam_finalize(dev, ml, 1, 0, lp, len_offset)
        assert np.array_equal(seq.cpu().numpy(), mod.seq) and np.array_equal(length.cpu().numpy(), mod.len)
        assert_state_equal(dev, mod, (case, lp, "finalize"))
        ref = M.oracle_search(monkeypatch, T1, T2, B, nb, ml, lp, len_offset)
        assert M.trimmed(seq.cpu().numpy(), length.cpu().numpy(), ml).tolist() == ref.tolist()


def test_step_rejects_an_index_out_of_range():
    """A top_i entry outside [0, nb * V) never becomes an address: the error word is set and the candidate is skipped."""
    B, nb, V, ml = 2, 2, 9, 4
    dev, mod = ops.BeamState(B, nb, ml, DEV), M.State(B, nb, ml)
    top_s = np.linspace(-1, -2, B * 2 * nb).astype(np.float32).reshape(B, 2 * nb)
    top_i = np.array([[3, nb * V, 5, 7], [-1, 2, 2 ** 31 - 1, 4]], dtype=np.int32)
    ops.beam_step(dev, cuda(top_s), cuda(top_i), V, 1, 1, 0)
    M.step(mod, top_s, top_i, V, 1, 1, 0)
    assert mod.err[0] == 1
    assert_state_equal(dev, mod, "range")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the whole loop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_model():
    """The model of test_t5_generate_matches_oracle_and_third_party, built as that test builds it, with a cache of oracle results."""
    from m3ae_amd.modules.t5 import T5ForConditionalGeneration
    from m3ae_amd.param_store import ParamStore, group_hparams_decoder, param_group_of_decoder
    g = load_golden("tiny_t5_generate.npz")
    m = T5ForConditionalGeneration(dict(d_model=512, d_kv=64, d_ff=2048, num_layers=2, num_decoder_layers=2, num_heads=8), 1100)
    sd = gen_t5_weights({"t5." + k: v for k, v in m.state_dict().items()})
    m.load_state_dict({k[3:]: v for k, v in sd.items()})
    ParamStore(m, tiny_config(compute_dtype="fp32"), "cuda", torch.float32, m.weight_units, group_fn=param_group_of_decoder,
               hparams_fn=group_hparams_decoder)
    m.eval()
    sd_cpu = {k: v.detach().cpu() for k, v in sd.items()}
    cache = {}

    def oracle(eos, len_offset):
        if (eos, len_offset) not in cache:
            with torch.no_grad():
                cache[eos, len_offset] = O.t5_beam_search(sd_cpu, torch.from_numpy(g["enc"]), 8, num_beams=4, max_length=8, eos_id=eos,
                                                          len_offset=len_offset).tolist()
        return cache[eos, len_offset]
    return m, g, torch.from_numpy(g["enc"]).cuda(), oracle


@pytest.mark.parametrize("len_offset", [0, 1])
def test_generate_device_matches_host_oracle_and_third_party(fixture_model, len_offset):
    m, g, enc, oracle = fixture_model
    for eos in g["eos_ids"].tolist():
        host = m.generate(enc, num_beams=4, max_length=8, eos_token_id=eos, len_offset=len_offset, beam_search="host")
        dev = m.generate(enc, num_beams=4, max_length=8, eos_token_id=eos, len_offset=len_offset, beam_search="device")
        assert dev.dtype == host.dtype and dev.device == host.device
        assert dev.cpu().tolist() == host.cpu().tolist() == oracle(eos, len_offset), eos
        if len_offset == 1:
            assert canon_generated(dev.cpu().tolist(), eos) == canon_generated(g[f"seq_{eos}"].tolist(), eos), eos


def test_lookahead_changes_no_token_and_leaves_early(fixture_model):
    """lookahead 1, 2 and None give identical seq / len, and the loop runs at most `lookahead` steps past the step that closed the
    last sample (the full run's open_count tells which).  No EOS id of the fixture closes all 12 samples before max_length (open
    counts after the steps, from the CPU model: 420 -> 12 12 11 11 11 11 11, 764 -> 12 12 12 11 10 10 10, 726 -> 12 12 12 12 11 11
    11, 442 / 259 / 1 -> 12 throughout), so that the loop really leaves early is asserted where every sample closes by step 4 of
    7: test_generate_on_scripted_logits, case (9, 4, 8, 2.5), through the same generate loop."""
    m, g, enc, _ = fixture_model
    for eos in g["eos_ids"].tolist():
        full = m.generate_async(enc, num_beams=4, max_length=8, eos_token_id=eos, lookahead=None)
        assert full.steps == 7 and int(full.err.cpu()) == 0
        open_count = full.state.open_count.cpu().tolist()
        closed_at = next((t for t in range(1, 8) if open_count[t] == 0), None)
        for la in (1, 2):
            r = m.generate_async(enc, num_beams=4, max_length=8, eos_token_id=eos, lookahead=la)
            assert torch.equal(r.seq, full.seq) and torch.equal(r.len, full.len), (eos, la)
            # the host has seen step t - la + 1 when it decides about step t + 1: at most `la` steps past the closing one
            if closed_at is not None:
                assert r.steps <= min(closed_at + la, 7), (eos, la, r.steps, closed_at)
            else:
                assert r.steps == 7


@pytest.mark.parametrize("case", [c for c in M.SCRIPTED if c[:3] in ((9, 4, 8), (37, 4, 12))], ids=lambda c: "V{}-nb{}-L{}-eos{}".format(*c))
def test_generate_on_scripted_logits(fixture_model, monkeypatch, case):
    """Host form, device form and oracle on logits scripted through next_token_logits_cached: V just above 2 nb, and max_length
    reached with open beams."""
    m, _, _, _ = fixture_model
    V, nb, ml, eos_bias = case
    B = M.SCRIPTED_B
    T1, T2 = M.tables(V, nb, ml, eos_bias, B, M.SCRIPTED[case])
    T1d, T2d = cuda(T1), cuda(T2)
    monkeypatch.setattr(m, "next_token_logits_cached", lambda enc, last_ids, cross_kv, self_cache, t: T1d[t] + T2d[last_ids.view(-1)])
    enc = torch.zeros(B, 4, 512, device=DEV)
    for len_offset in (0, 1):
        ref = M.oracle_search(monkeypatch, T1, T2, B, nb, ml, 1.0, len_offset).tolist()
        host = m.generate(enc, num_beams=nb, max_length=ml, len_offset=len_offset)
        dev = m.generate(enc, num_beams=nb, max_length=ml, len_offset=len_offset, beam_search="device")
        assert host.cpu().tolist() == ref and dev.cpu().tolist() == ref
    if case == (9, 4, 8, 2.5):      # every sample is done by step 4 of 7 (asserted on the model): the loop leaves early
        mod, _ = M.validate(case, M.SCRIPTED[case])
        assert max(e[1] for e in mod.events if not isinstance(e, str)) == 4 and "open_at_end" not in mod.events
        full = m.generate_async(enc, num_beams=nb, max_length=ml, lookahead=None)
        assert full.steps == ml - 1 and full.state.open_count.cpu().tolist()[1:5] == mod.open_count.tolist()[1:5]
        for la in (1, 2):
            r = m.generate_async(enc, num_beams=nb, max_length=ml, lookahead=la)
            assert r.steps <= 4 + la < ml - 1, (la, r.steps)
            assert torch.equal(r.seq, full.seq) and torch.equal(r.len, full.len)


def test_generate_bf16_full_vocabulary(monkeypatch):
    """bf16, T5-small dimensions at reduced depth, V = 32128, B = 3, random encoder output: device equals host on a seed where the
    host path's own live top-(2 nb + 1) gaps exceed 2 tau (asserted on the scores the host form's torch.topk saw).

    bf16 logits tie EXACTLY wherever two of a row's top values fall into one bf16 step (2^-8 relative), and torch.topk leaves the
    order of ties open, so the condition is a condition on the seed: with Gaussian logits a pair of neighbours among the top of
    32128 ties with probability ~0.1, and no seed survives 11 steps x 3 samples x 8 gaps.  The case is therefore sized for the
    condition to be attainable, not weakened: 2 beams, max_length 5 (4 steps: first step, re-ordered caches, EOS handling, open
    beams at the end), and an LM head whose row norms are heavy-tailed (1 / u, u uniform), which spreads a row's top logits by
    ratios ~ (k + 1) / k instead of a few percent."""
    from m3ae_amd.modules.t5 import T5ForConditionalGeneration
    from m3ae_amd.param_store import ParamStore, group_hparams_decoder, param_group_of_decoder
    B, nb, ml, V = 3, 2, 5, 32128
    m = T5ForConditionalGeneration(dict(d_model=512, d_kv=64, d_ff=2048, num_layers=1, num_decoder_layers=2, num_heads=8), V)
    sd = gen_t5_weights({"t5." + k: v for k, v in m.state_dict().items()})
    scale = 1.0 / np.random.default_rng(0).uniform(1e-5, 1.0, V)
    sd["t5.shared.weight"].mul_(torch.from_numpy(scale / 15.0).float()[:, None])
    m.load_state_dict({k[3:]: v for k, v in sd.items()})
    ParamStore(m, tiny_config(compute_dtype="bf16"), "cuda", torch.bfloat16, m.weight_units, group_fn=param_group_of_decoder,
               hparams_fn=group_hparams_decoder)
    m.eval()
    real_topk, real_logits = torch.topk, m.next_token_logits_cached
    rec = []

    def topk_plus_one(x, k, dim=-1, **kw):
        if x.dim() == 2 and x.shape[1] == nb * V:
            rec[-1]["vals"] = real_topk(x, k + 1, dim=dim)[0].cpu().numpy().astype(np.float64)
            s, i = real_topk(x, k, dim=dim, **kw)
            rec[-1]["top_s"], rec[-1]["top_i"] = s.cpu().numpy(), i.cpu().numpy().astype(np.int32)
            return s, i
        return real_topk(x, k, dim=dim, **kw)

    def logits_recorded(*a):
        out = real_logits(*a)
        rec.append({"spread": (out.max(dim=1)[0] - out.min(dim=1)[0]).view(B, nb).max(dim=1)[0].cpu().numpy()})
        return out

    for seed in range(48):
        enc = (torch.randn(B, 16, 512, generator=torch.Generator().manual_seed(seed)) * 0.5).to(DEV, torch.bfloat16)
        rec.clear()
        monkeypatch.setattr(torch, "topk", topk_plus_one)
        monkeypatch.setattr(m, "next_token_logits_cached", logits_recorded)
        host = m.generate(enc, num_beams=nb, max_length=ml)
        monkeypatch.setattr(torch, "topk", real_topk)
        monkeypatch.setattr(m, "next_token_logits_cached", real_logits)
        # replay the host form's candidates through the model: which samples were live at each step
        mod, worst = M.State(B, nb, ml), np.inf
        for t, r in enumerate(rec):
            for b in range(B):
                if not mod.done[b]:
                    for a, c in zip(r["vals"][b, :-1], r["vals"][b, 1:]):
                        worst = min(worst, (a - c) / (2.0 * max(M.tau(a, r["spread"][b]), M.tau(c, r["spread"][b]))))
            M.step(mod, r["top_s"], r["top_i"], V, t + 1, 1, 0)
        print(f"bf16 seed {seed}: {len(rec)} host steps, minimum live gap = {worst:.2f} x 2 tau")
        if worst >= 1.0:
            break
    assert worst >= 1.0, "no seed below 48 separates the host form's live candidates by 2 tau"
    dev = m.generate(enc, num_beams=nb, max_length=ml, beam_search="device")
    assert dev.cpu().tolist() == host.cpu().tolist()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. no host waits
# ---------------------------------------------------------------------------------------------------------------------------------
def test_generate_async_never_waits_for_the_device(fixture_model, monkeypatch):
    """Guard in use: torch.cuda.set_sync_debug_mode("error") where `.item()` under it raises on this torch / ROCm pair (checked
    first); otherwise calls of Tensor.cpu / item / tolist / __bool__ and torch.cuda.synchronize are counted through monkeypatch."""
    m, g, enc, _ = fixture_model
    eos = g["eos_ids"].tolist()[0]
    want = m.generate_async(enc, num_beams=4, max_length=8, eos_token_id=eos)      # warm: every lazy pack / cast has happened
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            live = False
        except RuntimeError:
            live = True
        if live:
            r = m.generate_async(enc, num_beams=4, max_length=8, eos_token_id=eos)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not live:
        calls = []
        for name in ("cpu", "item", "tolist", "__bool__"):
            real = getattr(torch.Tensor, name)
            monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _r=real, _n=name, **k: (calls.append(_n) if self.is_cuda else None, _r(self, *a, **k))[1])
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
        r = m.generate_async(enc, num_beams=4, max_length=8, eos_token_id=eos)
        monkeypatch.undo()
        assert calls == [], calls
    print("sync guard:", "set_sync_debug_mode" if live else "call counting")
    assert torch.equal(r.seq, want.seq) and torch.equal(r.len, want.len)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. mode off is today's path
# ---------------------------------------------------------------------------------------------------------------------------------
def test_default_generate_calls_no_beam_entry_point(fixture_model, monkeypatch):
    m, g, enc, _ = fixture_model
    L = _lib.lib()
    counts = {}

    class Counting:
        def __getattr__(self, name):
            if name.startswith("m3ae_beam_"):
                counts[name] = counts.get(name, 0) + 1
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Counting())
    eos = g["eos_ids"].tolist()[0]
    m.generate(enc, num_beams=4, max_length=8, eos_token_id=eos)
    assert counts == {}, counts
    m.generate(enc, num_beams=4, max_length=8, eos_token_id=eos, beam_search="device")
    assert {"m3ae_beam_topk", "m3ae_beam_step", "m3ae_beam_finalize"} <= set(counts), counts


@pytest.mark.parametrize("max_length", [3, 2])
def test_generate_async_enqueues_topk_and_step_per_position_then_finalize(fixture_model, monkeypatch, max_length):
    """One call without early exit (B = 2, two beams) under a recording proxy of the library: the ordered search entry points (the
    workspace-size query aside) are top-k, step per position, then finalize; the caches are re-ordered between steps only, so nothing
    at all is enqueued between the last step and finalize (max_length 2: one step, no re-ordering).  Tokens against the host form."""
    m, g, enc, _ = fixture_model
    L = _lib.lib()
    names = []

    class Recording:
        def __getattr__(self, name):
            names.append(name)
            return getattr(L, name)
    monkeypatch.setattr(_lib, "_lib", Recording())
    r = m.generate_async(enc[:2], num_beams=2, max_length=max_length, lookahead=None)
    monkeypatch.undo()
    search = [n for n in names if n.startswith(("m3ae_greedy_", "m3ae_beam_", "m3ae_trie_", "m3ae_triebeam_")) and not n.endswith("_workspace_bytes")]
    assert search == ["m3ae_beam_topk", "m3ae_beam_step"] * (max_length - 1) + ["m3ae_beam_finalize"]
    assert names[-2:] == ["m3ae_beam_step", "m3ae_beam_finalize"] and r.steps == max_length - 1 and int(r.err.cpu()) == 0
    after_first_step = names[names.index("m3ae_beam_step") + 1:]
    assert ("m3ae_gather_rows" in after_first_step) == (max_length > 2)     # (the next step's embedding is a row gather too)
    host = m.generate(enc[:2], num_beams=2, max_length=max_length)
    assert m.generate(enc[:2], num_beams=2, max_length=max_length, beam_search="device").tolist() == host.tolist()
    assert r.seq[:, :host.shape[1]].tolist() == host.tolist()


def test_t5vqa_module_passes_the_mode():
    """T5VQA_MMEncoderInput with t5_beam_search=device returns the generated_ids it returns with host (tiny config, B = 2)."""
    from m3ae_amd import synth
    from m3ae_amd.modules import T5VQA_MMEncoderInput
    dims = dict(d_model=512, d_kv=64, d_ff=2048, num_layers=2, num_decoder_layers=2, num_heads=8)
    out = {}
    for mode in ("host", "device"):
        m = T5VQA_MMEncoderInput(tiny_config(compute_dtype="fp32", t5_beam_search=mode, t5_max_length=8), t5_vocab=1100, t5_dims=dims)
        synth.fill_deterministic(m)
        m.finalize("cuda", torch.float32)
        m.eval()
        assert m.beam_search == mode
        b = {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v] if isinstance(v, list) and v
                 and isinstance(v[0], torch.Tensor) else v) for k, v in tiny_batch().items()}
        out[mode] = m(b, test=True)["generated_ids"].cpu().tolist()
    assert out["host"] == out["device"] and len(out["host"]) == 2
