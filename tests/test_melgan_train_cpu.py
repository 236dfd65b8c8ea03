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


class _CudaMarked(torch.Tensor):
    """A CPU tensor that says it is on the device: enough for a walk whose library calls are recorders."""
    is_cuda = True


def test_forward_train_walks_the_model_in_order(monkeypatch):
    """forward_train with the autograd entry points replaced by shape-propagating recorders: 18 calls in model order
    with each one's (dilation, padding, input slope, alpha, activation), every bias passed once, 29 taps."""
    from mixgan_tts_amd import autograd as ag
    G = mg.MelGANGenerator()
    path = {p.data_ptr(): n[:-len(".bias")] for n, p in G.named_parameters() if n.endswith(".bias")}
    assert len(path) == 42
    calls, biases = [], []

    def voc_conv(x, w, b, dil, pad, in_slope=1.0, alpha=1.0, act=None):
        calls.append(("conv", path[b.data_ptr()], dil, pad, in_slope, alpha, act))
        biases.append(b.data_ptr())
        assert w.shape[1] == x.shape[1]
        return torch.zeros(x.shape[0], w.shape[0], x.shape[2])

    def voc_up(x, w, b, u, slope, alpha):
        calls.append(("up", path[b.data_ptr()], u, slope, alpha))
        biases.append(b.data_ptr())
        assert w.shape[0] == x.shape[1] and w.shape[2] == 2 * u
        return torch.zeros(x.shape[0], w.shape[1], u * x.shape[2])

    def melgan_resblock(x, w1, b1, w2, b2, ws, bs, dil, slope):
        assert path[b2.data_ptr()] == path[b1.data_ptr()][:-1] + "4"
        assert path[bs.data_ptr()] == path[b1.data_ptr()][:-len("block.2")] + "shortcut"
        calls.append(("block", path[b1.data_ptr()], dil, slope))
        biases.extend(b.data_ptr() for b in (b1, b2, bs))
        C = x.shape[1]
        assert tuple(w1.shape) == (C, C, 3) and tuple(w2.shape) == tuple(ws.shape) == (C, C, 1)
        return torch.zeros_like(x), torch.zeros(x.shape[0], 2 * C, x.shape[2])

    monkeypatch.setattr(ag, "voc_conv", voc_conv)
    monkeypatch.setattr(ag, "voc_up", voc_up)
    monkeypatch.setattr(ag, "melgan_resblock", melgan_resblock)
    taps = {}
    wav = G.forward_train(torch.zeros(1, 80, 4).as_subclass(_CudaMarked), taps, 0.5)
    assert tuple(wav.shape) == (1, 1, 4 * 256)
    assert len(calls) == 18
    assert calls[0] == ("conv", "model.1", 1, ag.REFLECT, 1.0, 0.5, None)
    assert calls[-1] == ("conv", "model.%d" % (len(G.model) - 2), 1, ag.REFLECT, 0.2, 1.0, "tanh")
    for i, r in enumerate((8, 8, 2, 2)):
        base = 2 + 5 * i
        assert calls[1 + 4 * i] == ("up", "model.%d" % (base + 1), r, 0.2, 1.0)
        for j in range(3):
            assert calls[2 + 4 * i + j] == ("block", "model.%d.block.2" % (base + 2 + j), 3 ** j, 0.2)
    assert sorted(biases) == sorted(path)
    assert len(taps) == 29


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
