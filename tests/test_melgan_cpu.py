"""The native MelGAN's surface without a GPU: state-dict keys, shapes and order equal the plain-torch restatement of
mel2wav/modules.py (tests/melgan_torch.py), so a hub checkpoint loads strictly; get_vocoder's MelGAN branch without a
checkpoint; input errors; the argument checks of the new C entry points (they return before any launch)."""
import ctypes

import pytest
import torch

import melgan_torch as MT

from mixgan_tts_amd._lib import MG_ERR_ARG, MG_ERR_SHAPE


def test_state_dict_keys_shapes_order_match_restatement():
    import mixgan_tts_amd as mg
    ours = mg.MelGANGenerator().state_dict()
    ref = MT.Generator().state_dict()
    assert list(ours.keys()) == list(ref.keys())
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    assert "model.4.block.2.weight_g" in ours and "model.4.shortcut.weight_v" in ours and "model.24.bias" in ours
    assert tuple(ours["model.3.weight_g"].shape) == (512, 1, 1)      # ConvTranspose1d: norm over dim 0 = Cin
    assert mg.MelVocoder().mel2wav.fused_stack is True


def test_strict_load_of_restatement_state_dict(tmp_path):
    import mixgan_tts_amd as mg
    sd = MT.seeded_generator(3).state_dict()
    G = mg.MelGANGenerator()
    G.load_state_dict(sd, strict=True)
    for k, v in G.state_dict().items():
        assert torch.equal(v, sd[k]), k
    ck = tmp_path / "linda_johnson.pt"
    torch.save({k: v.detach().clone() for k, v in sd.items()}, ck)
    voc = mg.MelVocoder()
    voc.mel2wav.load_state_dict(torch.load(ck, map_location="cpu", weights_only=True), strict=True)
    # the effective weight of a weight-normed transposed conv is the restatement's
    ref_up = dict(MT.seeded_generator(3).model.named_modules())["3"]
    torch.testing.assert_close(voc.mel2wav.model[3].effective_weight(), ref_up.weight.detach(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("speaker,hub_file", [("LJSpeech", "linda_johnson.pt"), ("universal", "multi_speaker.pt")])
def test_get_vocoder_melgan_needs_checkpoint(speaker, hub_file):
    import mixgan_tts_amd as mg
    cfg = {"vocoder": {"model": "MelGAN", "speaker": speaker}}
    with pytest.raises(mg.vocoder.MelGANCheckpointRequired) as ei:
        mg.vocoder.get_vocoder(cfg, "cpu")
    assert hub_file in str(ei.value)
    with pytest.raises(NotImplementedError):
        mg.vocoder.get_vocoder(cfg, "cpu")
    assert issubclass(mg.vocoder.MelGANCheckpointRequired, mg.MixganHipError)


def test_forward_input_errors():
    import mixgan_tts_amd as mg
    G = mg.MelGANGenerator()
    with pytest.raises(mg.MixganHipError):
        G(torch.zeros(1, 80, 10))                      # CPU input: no fallback
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            G.cuda()(torch.zeros(1, 80, 3, device="cuda"))


class _AsCuda:
    """Stands in for a device tensor: forward checks the device, then the shape, before it touches the data."""

    def __init__(self, t):
        self.shape = t.shape
        self.is_cuda = True


def test_short_input_raises_value_error_before_any_launch():
    import mixgan_tts_amd as mg
    G = mg.MelGANGenerator()
    for L in (0, 1, 3):
        with pytest.raises(ValueError):
            G.forward_scaled(_AsCuda(torch.zeros(1, 80, L)), 1.0)
    with pytest.raises(ValueError):
        G.forward_scaled(_AsCuda(torch.zeros(1, 81, 10)), 1.0)


def test_abi_argument_checks():
    import mixgan_tts_amd as mg
    L = mg.lib()
    p = ctypes.c_void_p(64)      # never dereferenced: every call below fails its checks first
    n = ctypes.c_void_p(0)
    s = ctypes.c_void_p(0)
    # reflect conv: null pointers, bad act, bad K / dilation, L <= pad
    assert L.mg_conv1d_reflect_fwd(n, 0, p, p, p, 0, 1, 32, 100, 32, 3, 1, 1.0, 0, 0.0, 1.0, s) == MG_ERR_ARG
    assert L.mg_conv1d_reflect_fwd(p, 0, p, p, p, 0, 1, 32, 100, 32, 3, 1, 1.0, 9, 0.0, 1.0, s) == MG_ERR_ARG
    assert L.mg_conv1d_reflect_fwd(p, 0, p, p, p, 0, 1, 32, 100, 32, 5, 1, 1.0, 0, 0.0, 1.0, s) == MG_ERR_SHAPE
    assert L.mg_conv1d_reflect_fwd(p, 0, p, p, p, 0, 1, 32, 100, 32, 3, 11, 1.0, 0, 0.0, 1.0, s) == MG_ERR_SHAPE
    assert L.mg_conv1d_reflect_fwd(p, 0, p, p, p, 0, 1, 32, 100, 32, 7, 3, 1.0, 0, 0.0, 1.0, s) == MG_ERR_SHAPE
    assert L.mg_conv1d_reflect_fwd(p, 0, p, p, p, 0, 1, 80, 3, 512, 7, 1, 1.0, 0, 0.0, 1.0, s) == MG_ERR_SHAPE
    assert L.mg_conv1d_reflect_fwd(p, 0, p, p, p, 0, 1, 32, 9, 32, 3, 9, 1.0, 0, 0.0, 1.0, s) == MG_ERR_SHAPE
    assert L.mg_conv1d_reflect_fwd(p, 0, p, p, p, 0, 0, 32, 100, 32, 3, 1, 1.0, 0, 0.0, 1.0, s) == MG_ERR_SHAPE
    # 1x1 with strides
    assert L.mg_conv1x1_fwd_strided(p, 0, n, p, p, 0, 1, 64, 100, 32, s) == MG_ERR_ARG
    assert L.mg_conv1x1_fwd_strided(p, 10, p, p, p, 0, 1, 64, 100, 32, s) == MG_ERR_SHAPE
    assert L.mg_conv1x1_fwd_strided(p, 0, p, p, p, -1, 1, 64, 100, 32, s) == MG_ERR_SHAPE
    # transposed conv into a slice
    assert L.mg_conv_transpose1d_fwd_slice(p, p, p, n, 0, 1, 64, 10, 32, 2, 0.2, 1.0, s) == MG_ERR_ARG
    assert L.mg_conv_transpose1d_fwd_slice(p, p, p, p, 0, 1, 64, 10, 32, 3, 0.2, 1.0, s) == MG_ERR_SHAPE
    assert L.mg_conv_transpose1d_fwd_slice(p, p, p, p, 100, 1, 64, 10, 32, 2, 0.2, 1.0, s) == MG_ERR_SHAPE
    # fused stack
    ptrs = (ctypes.c_void_p * 3)(64, 64, 64)
    nulls = (ctypes.c_void_p * 3)(64, 0, 64)
    assert L.mg_melgan_stack_fwd(p, p, ptrs, ptrs, ptrs, ptrs, 1, 32, 100, s) == MG_ERR_ARG            # in == out
    assert L.mg_melgan_stack_fwd(p, ctypes.c_void_p(128), nulls, ptrs, ptrs, ptrs, 1, 32, 100, s) == MG_ERR_ARG
    assert L.mg_melgan_stack_fwd(p, ctypes.c_void_p(128), ptrs, ptrs, ptrs, ptrs, 1, 48, 100, s) == MG_ERR_SHAPE
    assert L.mg_melgan_stack_fwd(p, ctypes.c_void_p(128), ptrs, ptrs, ptrs, ptrs, 1, 64, 9, s) == MG_ERR_SHAPE
    assert L.mg_melgan_stack_fwd(p, ctypes.c_void_p(128), ptrs, ptrs, ptrs, ptrs, 0, 64, 100, s) == MG_ERR_SHAPE
    assert L.mg_melgan_stack_tile(32) > 13 and L.mg_melgan_stack_tile(64) > 13 and L.mg_melgan_stack_tile(128) == 0
