"""Host: the config key clip_residual_dtype, the rounding model behind it (tests/clip_stream_model.py) and the numpy model of the
mixed LayerNorm (fp32 rows in, bf16 rows out)."""
import os

import numpy as np
import pytest
import torch

import abi_header
import clip_stream_model as CM
from m3ae_amd import _lib, config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = range(8)


def test_key_defaults_parses_and_validates():
    assert config.DEFAULTS["clip_residual_dtype"] == "bf16"
    assert config.tiny_config()["clip_residual_dtype"] == "bf16"
    argv = ["with", "task_finetune_vqa_vqa_rad", "clip16", "text_roberta"]
    assert config.parse_cli(argv)["clip_residual_dtype"] == "bf16"
    assert config.parse_cli(argv + ["clip_residual_dtype=fp32"])["clip_residual_dtype"] == "fp32"
    assert config.parse_cli(["clip_residual_dtype=fp32"] + argv)["clip_residual_dtype"] == "fp32"
    assert config.finetune_vqa_rad_config(clip_residual_dtype="fp32", compute_dtype="fp32x3")["clip_residual_dtype"] == "fp32"
    for bad in ("fp16", "float32", "", None, 32, "FP32"):
        with pytest.raises(ValueError, match="clip_residual_dtype"):
            config.tiny_config(clip_residual_dtype=bad)
    with pytest.raises(ValueError, match="clip_residual_dtype"):
        config.parse_cli(argv + ["clip_residual_dtype=fp64"])


def test_modules_carry_the_key_and_refuse_other_values():
    from m3ae_amd.modules import M3AETransformerSS
    from m3ae_amd.modules.clip_model import build_model
    assert build_model("ViT-B/16", 32, 64, 2, 16).visual.residual_dtype == "bf16"
    v = build_model("ViT-B/16", 32, 64, 2, 16, residual_dtype="fp32").visual
    assert v.stream_dtype(torch.bfloat16) == torch.float32 and v.stream_dtype(torch.float32) == torch.float32
    assert build_model("ViT-B/16", 32, 64, 2, 16).visual.stream_dtype(torch.bfloat16) == torch.bfloat16
    with pytest.raises(ValueError, match="clip_residual_dtype"):
        build_model("ViT-B/16", 32, 64, 2, 16, residual_dtype="fp16")
    m = M3AETransformerSS(config.tiny_config(clip_residual_dtype="fp32"))
    assert m.vision_encoder.visual.residual_dtype == "fp32"
    with pytest.raises(ValueError, match="clip_residual_dtype"):
        M3AETransformerSS(dict(config.tiny_config(), clip_residual_dtype="half"))


def test_new_entry_points_are_declared_bound_and_documented():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("m3ae_layernorm_fwd_mixed", "m3ae_layernorm_bwd_mixed", "m3ae_layernorm_bwd_mixed_det"):
        assert name in _lib.EXPORTS and f"lib.{name}.argtypes" in doc, name    # declared == bound: tests/test_host_logic.py
    protos = abi_header.prototypes()
    assert protos["m3ae_layernorm_bwd_mixed"] == protos["m3ae_layernorm_bwd_mixed_det"]           # two wrappers, one signature
    assert _lib._SIGS["m3ae_layernorm_bwd_mixed"] == _lib._SIGS["m3ae_layernorm_bwd_mixed_det"]
    assert "clip_residual_dtype" in doc


@pytest.fixture(scope="module")
def errors():
    """(bf16-stream error, fp32-stream error) per seed at 11 and at 2 blocks: width 128, 2 heads, 34 rows."""
    return {n: [CM.stream_errors(128, 2, n, 34, seed) for seed in SEEDS] for n in (11, 2)}


@pytest.mark.parametrize("n_blocks,least", [(11, 4.0), (2, 2.0)])
def test_rounding_model_stream_roundings_dominate_the_tower_error(errors, n_blocks, least):
    for seed, (e_bf16, e_fp32) in zip(SEEDS, errors[n_blocks]):
        print(f"blocks {n_blocks} seed {seed}: bf16 stream {e_bf16:.3e}  fp32 stream {e_fp32:.3e}  ratio {e_bf16 / e_fp32:.2f}")
        assert e_bf16 / e_fp32 >= least, (n_blocks, seed, e_bf16, e_fp32)


def test_rounding_model_error_of_the_bf16_stream_grows_with_depth(errors):
    for (deep, _), (shallow, _) in zip(errors[11], errors[2]):
        assert deep > 1.5 * shallow


def test_numpy_mixed_layernorm_is_the_fp32_layernorm_rounded_once():
    rng = np.random.default_rng(5)
    for M, D in ((5, 768), (34, 128), (3, 516)):
        x = (rng.standard_normal((M, D)) * 3 + 0.5).astype(np.float32)
        g, b = rng.standard_normal(D).astype(np.float32), rng.standard_normal(D).astype(np.float32)
        bits, mean, rstd = CM.np_layernorm_mixed(x, g, b, 1e-5)
        y32, mean32, rstd32 = CM.np_layernorm_f32(x, g, b, 1e-5)
        assert np.array_equal(mean, mean32) and np.array_equal(rstd, rstd32)
        # one rounding: exactly torch's round-to-nearest-even of the fp32 result
        want = torch.from_numpy(y32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(bits, want)
        # and within half a bf16 ulp (+ the fp32 evaluation error) of the float64 LayerNorm
        ref = CM.layer_norm(torch.from_numpy(x).double(), torch.from_numpy(g).double(), torch.from_numpy(b).double()).numpy()
        err = np.abs(CM.np_bf16_to_f32(bits).astype(np.float64) - ref)
        assert (err <= 2.0 ** -8 * np.abs(ref) * (1 + 2.0 ** -7) + 1e-5).all()
        # rounding the rows to bf16 BEFORE the LayerNorm (the bf16 stream) is a different function
        xb = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
        assert not np.array_equal(CM.np_layernorm_mixed(xb, g, b, 1e-5)[0], bits)


def test_numpy_rne_ties_go_to_even():
    f = lambda hexbits: np.array([hexbits], dtype=np.uint32).view(np.float32)
    assert CM.np_rne_bf16_bits(f(0x3F808000))[0] == 0x3F80      # tie, even below
    assert CM.np_rne_bf16_bits(f(0x3F818000))[0] == 0x3F82      # tie, even above
    assert CM.np_rne_bf16_bits(f(0x3F808001))[0] == 0x3F81
    assert CM.np_rne_bf16_bits(f(0xBF807FFF))[0] == 0xBF80
    x = np.random.default_rng(1).standard_normal(4096).astype(np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(CM.np_rne_bf16_bits(x), want)
