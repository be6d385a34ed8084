"""CPU: the error model of the fp32x3 GEMM (csrc/gemm_f32x3.hip) on a bit-exact numpy model of its split, and the mode's
plumbing on the host.

The kernel splits every fp32 operand element x into hi = bf16_rne(x), lo = bf16_rne(x - hi) and forms each product as
hi_a hi_b + hi_a lo_b + lo_a hi_b (exact products of bf16 values, fp32 accumulation).  tests/test_gpu_f32x3.py holds it to
    |C - C64| <= c (2^-16 + K 2^-23) (|A||B|)_mn,   c = 3.
The split part: |x - hi| <= 2^-8 |x|, |x - hi - lo| <= 2^-8 |x - hi| <= 2^-16 |x|, so the dropped terms of one product are
< 3 * 2^-16 |a b|; the accumulation part: 3K fp32 roundings of a running sum bounded by sum |a b|, 3K 2^-24 < 3 K 2^-23.
Here the split part is checked exactly (float64 sums of the three products, no accumulation error) and the whole bound with
a sequential fp32 accumulation of the three products per k, the worst order the kernel can take, on adversarial inputs."""
import numpy as np
import pytest

from m3ae_amd import config

C_BOUND = 3.0


def bf16_rne(x):
    """fp32 -> bf16 (as fp32) with round-to-nearest-even, by bit operations (the kernel's v_cvt_pk_bf16_f32)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def split(x):
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    lo = bf16_rne((x - hi).astype(np.float32))   # x - hi is exact in fp32
    return hi, lo


def x3_products(a, b):
    """[M, K] x [K, N] -> the three partial products per (m, k, n) in float64 (each one exact)."""
    ah, al = split(a)
    bh, bl = split(b)
    f = lambda t: t.astype(np.float64)
    return f(ah)[:, :, None] * f(bl)[None], f(al)[:, :, None] * f(bh)[None], f(ah)[:, :, None] * f(bh)[None]


def x3_gemm_fp32(a, b):
    """The kernel's arithmetic with the worst accumulation order: one fp32 accumulator, three roundings per k."""
    p1, p2, p3 = x3_products(a, b)
    acc = np.zeros((a.shape[0], b.shape[1]), dtype=np.float32)
    for k in range(a.shape[1]):
        for p in (p1, p2, p3):
            acc = (acc + p[:, k, :].astype(np.float32)).astype(np.float32)
    return acc


def bound(a, b):
    K = a.shape[1]
    return C_BOUND * (2.0 ** -16 + K * 2.0 ** -23) * (np.abs(a.astype(np.float64)) @ np.abs(b.astype(np.float64)))


def adversarial(rng, shape, kind):
    if kind == "normal":
        return rng.standard_normal(shape).astype(np.float32)
    if kind == "near_bf16_ties":   # halfway between two bf16 values and just beside it: the rounding boundaries of hi
        base = bf16_rne(rng.standard_normal(shape).astype(np.float32))
        ulp = np.abs(base) * 2.0 ** -8
        off = rng.choice([0.5, 0.5 - 2.0 ** -12, 0.5 + 2.0 ** -12, 0.25 + 2.0 ** -9], size=shape)
        return (base + np.sign(rng.standard_normal(shape)) * off * ulp).astype(np.float32)
    if kind == "mixed_exponents":
        return (rng.standard_normal(shape) * 2.0 ** rng.integers(-30, 30, size=shape)).astype(np.float32)
    if kind == "residual_heavy":   # x - hi close to its own bf16 rounding boundary: the worst case of lo
        hi = bf16_rne(rng.standard_normal(shape).astype(np.float32))
        lo_ulp = np.abs(hi) * 2.0 ** -16
        return (hi + hi * 2.0 ** -9 + np.sign(rng.standard_normal(shape)) * 0.5 * lo_ulp).astype(np.float32)
    raise ValueError(kind)


def test_bf16_rne_model_matches_torch():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32), adversarial(rng, (4096,), "near_bf16_ties")])
    ref = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    np.testing.assert_array_equal(bf16_rne(x), ref)


@pytest.mark.parametrize("kind", ["normal", "near_bf16_ties", "mixed_exponents", "residual_heavy"])
def test_split_residual_is_below_2_pow_minus_16(kind):
    rng = np.random.default_rng(1)
    x = adversarial(rng, (1 << 16,), kind)
    hi, lo = split(x)
    r = x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)
    assert np.all(np.abs(x.astype(np.float64) - hi) <= 2.0 ** -8 * np.abs(x))
    assert np.all(np.abs(r) <= 2.0 ** -16 * np.abs(x))


@pytest.mark.parametrize("kind", ["normal", "near_bf16_ties", "mixed_exponents", "residual_heavy"])
def test_dropped_terms_of_one_product_are_below_3_x_2_pow_minus_16(kind):
    rng = np.random.default_rng(2)
    a, b = adversarial(rng, (256, 1), kind), adversarial(rng, (1, 256), kind)
    p1, p2, p3 = x3_products(a, b)
    exact = a.astype(np.float64) @ b.astype(np.float64)
    err = np.abs((p1 + p2 + p3)[:, 0, :] - exact)
    assert np.all(err <= 3.0 * 2.0 ** -16 * np.abs(exact))


@pytest.mark.parametrize("kind,K", [("normal", 577), ("near_bf16_ties", 300), ("mixed_exponents", 128),
                                    ("residual_heavy", 400), ("cancellation", 512)])
def test_whole_bound_with_fp32_accumulation(kind, K):
    rng = np.random.default_rng(3)
    M, N = 8, 8
    if kind == "cancellation":   # sum a b ~ 0 with large |a||b|: the bound is relative to |A||B|, not to |C|
        a = adversarial(rng, (M, K // 2), "normal")
        a = np.concatenate([a, a], axis=1)
        b = adversarial(rng, (K // 2, N), "near_bf16_ties")
        b = np.concatenate([b, -b], axis=0)
    else:
        a, b = adversarial(rng, (M, K), kind), adversarial(rng, (K, N), kind)
    c = x3_gemm_fp32(a, b)
    exact = a.astype(np.float64) @ b.astype(np.float64)
    err = np.abs(c.astype(np.float64) - exact)
    assert np.all(err <= bound(a, b)), (err / bound(a, b)).max()
    # and the bf16-operand GEMM of the same data is far outside it: the lo terms carry the accuracy
    err_bf16 = np.abs(bf16_rne(a).astype(np.float64) @ bf16_rne(b).astype(np.float64) - exact)
    if kind != "cancellation":
        assert err.max() * 30 <= err_bf16.max()


def test_parse_cli_carries_the_fp32x3_mode():
    cfg = config.parse_cli(["with", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta", "compute_dtype=fp32x3"])
    assert cfg["compute_dtype"] == "fp32x3"
    assert config.parse_cli(["with", "task_finetune_vqa_vqa_rad"])["compute_dtype"] == "bf16"


def test_model_records_the_mode_and_keeps_fp32_storage():
    torch = pytest.importorskip("torch")
    from m3ae_amd import ops
    from m3ae_amd.modules import M3AETransformerSS
    with torch.device("meta"):
        m3 = M3AETransformerSS(config.tiny_config(compute_dtype="fp32x3"))
        m32 = M3AETransformerSS(config.tiny_config(compute_dtype="fp32"))
        mbf = M3AETransformerSS(config.tiny_config(compute_dtype="bf16"))
    assert m3.f32x3 and m3._dtype == torch.float32
    assert not m32.f32x3 and m32._dtype == torch.float32
    assert not mbf.f32x3 and mbf._dtype == torch.bfloat16
    m32.set_compute_dtype("fp32x3")
    assert m32.f32x3
    m32.set_compute_dtype(torch.bfloat16)   # bf16 storage: the mode has no fp32 GEMMs to act on
    assert not m32.f32x3


def test_autograd_nodes_carry_the_forward_mode_into_backward():
    """The mode is thread-local; autograd runs backward on a thread of its own: every node saves its forward's mode."""
    torch = pytest.importorskip("torch")
    import threading
    from m3ae_amd import ops
    seen = []

    class Probe(ops.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            seen.append(ops.f32x3_active())
            return g * 2

    for on in (True, False):
        x = torch.ones(3, requires_grad=True)
        with ops.f32x3_mode(on):
            y = Probe.apply(x)
        assert not ops.f32x3_active()
        t = threading.Thread(target=lambda: y.sum().backward())   # a thread that never entered the mode
        t.start()
        t.join()
        assert torch.equal(x.grad, torch.full((3,), 2.0))
    assert seen == [True, False]
