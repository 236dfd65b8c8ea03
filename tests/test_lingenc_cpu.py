"""The native LinguisticEncoder's surface without a GPU: the reference's state-dict keys, shapes and order (so a
reference checkpoint loads strictly), MixGANTTS(..., linguistic_encoder="native")'s full generator key set, the
inference-only and frame_level errors, and the plain-torch restatement (tests/lingenc_torch.py) against the reference's
recorded outputs."""
import numpy as np
import pytest
import torch

import lingenc_torch as LT
from helpers import golden
from lingenc_helpers import CASES, manifest, configs, load_weights, encoder_inputs, assert_outputs


def test_state_dict_matches_reference(tmp_path):
    import mixgan_tts_amd as mg
    man = manifest()
    for name in CASES:
        enc = mg.LinguisticEncoder(*configs(man, name, tmp_path))
        sd = enc.state_dict()
        assert list(sd.keys()) == man[name]["state_dict_order"], name
        assert {k: list(v.shape) for k, v in sd.items()} == man[name]["state_dict"], name
        assert not enc.abs_position_enc.requires_grad and not enc.pitch_bins.requires_grad
        assert enc.kv_position_enc.requires_grad and enc.q_position_enc.requires_grad


def test_bins_and_tables_are_the_references(tmp_path):
    import mixgan_tts_amd as mg
    man = manifest()
    enc = mg.LinguisticEncoder(*configs(man, "lingenc_infer", tmp_path))
    torch.testing.assert_close(enc.pitch_bins.detach(), torch.linspace(-2.0, 8.0, 255), rtol=0, atol=0)
    torch.testing.assert_close(enc.energy_bins.detach(), torch.linspace(-1.5, 7.0, 255), rtol=0, atol=0)
    torch.testing.assert_close(enc.abs_position_enc.detach()[0], LT.sinusoid(1001, 256), rtol=0, atol=0)


def test_mixgantts_native_has_reference_generator_keys(tmp_path):
    import mixgan_tts_amd as mg
    man = manifest()
    pre, mc, tr = configs(man, "lingenc_mixgantts_naive", tmp_path)
    import types
    m = mg.MixGANTTS(types.SimpleNamespace(model="naive"), pre, mc, tr, linguistic_encoder="native")
    sd = m.state_dict()
    assert sorted(sd) == sorted(man["lingenc_mixgantts_naive"]["state_dict"])
    assert {k: list(v.shape) for k, v in sd.items()} == man["lingenc_mixgantts_naive"]["state_dict"]
    with pytest.raises(ValueError):
        mg.MixGANTTS(types.SimpleNamespace(model="naive"), pre, mc, tr, linguistic_encoder="eager")


@pytest.mark.parametrize("which", ["pitch", "energy"])
def test_frame_level_raises(tmp_path, which):
    import mixgan_tts_amd as mg
    pre, mc, tr = configs(manifest(), "lingenc_infer", tmp_path)
    pre["preprocessing"][which]["feature"] = "frame_level"
    with pytest.raises(NotImplementedError):
        mg.LinguisticEncoder(pre, mc, tr)


def test_training_forward_raises(tmp_path):
    import mixgan_tts_amd as mg
    enc = mg.LinguisticEncoder(*configs(manifest(), "lingenc_infer", tmp_path)).eval()
    args = encoder_inputs(golden("lingenc_infer"), "cpu")
    with pytest.raises(NotImplementedError, match="inject the reference"):
        enc(*args)                               # grad enabled, parameters require grad
    enc.train()
    with torch.no_grad(), pytest.raises(NotImplementedError):
        enc(*args)                               # dropout is not implemented


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_fixture(tmp_path, name):
    """The plain-torch restatement the GPU tests use as their large-shape reference reproduces the reference."""
    import mixgan_tts_amd as mg
    man = manifest()
    cfg = configs(man, name, tmp_path)
    enc = mg.LinguisticEncoder(*cfg)
    load_weights(enc, man, name)
    g = golden(name)
    sd = {k: v.detach() for k, v in enc.state_dict().items()}
    with torch.no_grad():
        out, (enc_p, enc_w) = LT.encoder_forward(sd, cfg, *encoder_inputs(g, "cpu"))
    assert_outputs(out, g, 1e-4, {"enc_p_out": enc_p, "enc_w_out": enc_w})
