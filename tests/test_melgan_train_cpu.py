"""MelGAN training's surface without a GPU: forward_train refuses a CPU tensor and a generator the general form cannot
take before anything is launched; the state dict is what it was (keys and order of the plain-torch restatement, so hub
checkpoints and exported ones load strictly); the new entry points reject null operands."""
import pytest
import torch

import melgan_torch as MT

import mixgan_tts_amd as mg
from mixgan_tts_amd._lib import MG_ERR_ARG


def test_forward_train_refuses_a_cpu_tensor():
    with pytest.raises(mg.MixganHipError, match="no CPU fallback"):
        mg.MelGANGenerator().forward_train(torch.zeros(1, 80, 8))
    with pytest.raises(mg.MixganHipError, match="no CPU fallback"):
        mg.MelVocoder().forward_train(torch.zeros(1, 80, 8), {})


class _AsCuda:
    """Stands in for a device tensor: the structural checks come before anything touches the data."""

    def __init__(self, t):
        self.shape = t.shape
        self.is_cuda = True


def test_forward_train_refuses_what_the_general_form_cannot_take():
    with pytest.raises(mg.MixganHipError, match="dilations above 9"):
        mg.MelGANGenerator(n_residual_layers=4).forward_train(_AsCuda(torch.zeros(1, 80, 8)))
    with pytest.raises(mg.MixganHipError, match="multiples of 32"):
        mg.MelGANGenerator(ngf=16).forward_train(_AsCuda(torch.zeros(1, 80, 8)))
    G = mg.MelGANGenerator()
    for shape in ((1, 80, 3), (1, 81, 8)):
        with pytest.raises(ValueError):
            G.forward_train(_AsCuda(torch.zeros(*shape)))


def test_state_dict_keys_and_order_are_unchanged():
    ref = MT.Generator().state_dict()
    ours = mg.MelGANGenerator().state_dict()
    assert list(ours.keys()) == list(ref.keys())
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    voc = mg.MelVocoder()
    assert list(voc.state_dict().keys()) == ["mel2wav." + k for k in ref.keys()]
    assert [k for k, _ in voc.named_parameters()] == ["mel2wav." + k for k, _ in MT.Generator().named_parameters()]


def test_export_writes_the_bare_generator_state_dict(tmp_path):
    voc = mg.MelVocoder()
    path = tmp_path / "linda_johnson.pt"
    mg.vocoder_train.export_melgan_generator(voc, str(path))
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert list(sd.keys()) == list(MT.Generator().state_dict().keys())
    loaded = mg.vocoder.get_vocoder({"vocoder": {"model": "MelGAN", "speaker": "LJSpeech"}}, "cpu",
                                    checkpoint_path=str(path))
    for k, v in voc.mel2wav.state_dict().items():
        assert torch.equal(loaded.mel2wav.state_dict()[k], v), k


def test_new_entry_points_reject_null_operands():
    L = mg.lib()
    assert L.mg_conv1d_reflect_wgrad(None, 0, None, 0, None, None, 1, 32, 32, 10, 3, 1, 0.2, 1.0, 0, None) == MG_ERR_ARG
    assert L.mg_conv1d_reflect_dgrad(None, None, None, 0, None, 0, None, None, 0, 1, 32, 32, 10, 3, 1, 0.2, 1.0,
                                     None) == MG_ERR_ARG
    assert L.mg_reflect_fold_bwd(None, 0, None, 0, None, 0, None, 1, 32, 10, 1, 0.2, None) == MG_ERR_ARG
    assert L.mg_conv1d_reflect_dgrad_workspace_floats(2, 32, 10, 3, 9) == 2 * 32 * 28
    assert L.mg_conv1d_reflect_dgrad_workspace_floats(2, 32, 10, 7, 2) == 0
