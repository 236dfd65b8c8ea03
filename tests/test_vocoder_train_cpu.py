"""Host-side checks of the vocoder-training entry points (no GPU): exports and signatures, argument and shape rejection
before any launch, the CPU-tensor error of forward_train, and that the float64 reference helper's `masks=` is the
identity when the masks are its own."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import ROOT, seeded, golden, T

import hifigan_train_ref as HR
import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib

NEW = ["mg_conv1d_wgrad_ex", "mg_lrelu_bwd", "mg_conv_transpose1d_dgrad_workspace_floats", "mg_conv_transpose1d_dgrad",
       "mg_conv_transpose1d_wgrad_scratch_floats", "mg_conv_transpose1d_wgrad", "mg_stft_mel_bwd_workspace_bytes",
       "mg_stft_mel_bwd"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mixgan_hip.h")).read(), flags=re.S)


def test_new_exports_are_declared_bound_and_exported():
    code = _header()
    sig = _lib._signatures()
    L = ctypes.CDLL(mg.library_path())
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, name + " is not declared in the header"
        assert name in sig and name in _lib.EXPORTS, name + " has no ctypes signature"
        assert len(sig[name][1]) == len(m[1].split(",")), name + ": argument count differs from the header"
        assert hasattr(L, name), "libmixgan_hip.so does not export " + name
    for name in ("GeneratorTrainer", "sample_segments", "vocoder_train"):
        assert hasattr(mg, name)
    assert hasattr(mg.vocoder.Generator, "forward_train") and hasattr(mg.audio.TacotronSTFT, "mel_spectrogram_diff")


@pytest.fixture(scope="module")
def P():
    """A non-null pointer that no entry point may touch: every call below must return before its first launch."""
    buf = ctypes.create_string_buffer(64)
    return ctypes.c_void_p(ctypes.addressof(buf)), buf


def test_null_pointers_are_rejected():
    L = mg.lib()
    E = _lib.MG_ERR_ARG
    assert L.mg_conv1d_wgrad_ex(None, 0, None, 0, None, None, 1, 8, 8, 8, 8, 3, 1, 1, 0.1, 1.0, 0, None) == E
    assert L.mg_lrelu_bwd(None, None, None, None, 0.1, 8, None) == E
    assert L.mg_conv_transpose1d_dgrad(None, None, None, None, None, 0, 1, 8, 8, 8, 2, 0.1, 1.0, None) == E
    assert L.mg_conv_transpose1d_wgrad(None, None, None, None, 1, 8, 8, 8, 2, 0.1, 1.0, 0, None) == E
    assert L.mg_stft_mel_bwd(None, 1024, None, 1, 1024, 256, None, None, None, None, 80, None, 5, None, 1024, None, 0,
                             None) == E


def test_unsupported_shapes_are_rejected_before_any_launch(P):
    L = mg.lib()
    p, _ = P
    S = _lib.MG_ERR_SHAPE
    # dilated weight gradient: dil > 5, K outside {3, 7, 11}, a length that is not the convolution's
    assert L.mg_conv1d_wgrad_ex(p, 0, p, 0, p, p, 1, 8, 8, 8, 8, 3, 6, 6, 0.1, 1.0, 0, None) == S
    assert L.mg_conv1d_wgrad_ex(p, 0, p, 0, p, p, 1, 8, 8, 8, 8, 5, 1, 2, 0.1, 1.0, 0, None) == S
    assert L.mg_conv1d_wgrad_ex(p, 0, p, 0, p, p, 1, 8, 8, 9, 8, 3, 1, 1, 0.1, 1.0, 0, None) == S
    assert L.mg_conv1d_wgrad_ex(p, 0, p, 0, p, p, 0, 8, 8, 8, 8, 3, 1, 1, 0.1, 1.0, 0, None) == S
    # transposed convolution: u outside {2, 4, 8}
    for u in (1, 3, 5, 16):
        assert L.mg_conv_transpose1d_dgrad(p, p, p, p, p, 1 << 30, 1, 8, 8, 8, u, 0.1, 1.0, None) == S
        assert L.mg_conv_transpose1d_wgrad(p, p, p, p, 1, 8, 8, 8, u, 0.1, 1.0, 0, None) == S
        assert L.mg_conv_transpose1d_dgrad_workspace_floats(1, 8, 8, 8, u) == 0
        assert L.mg_conv_transpose1d_wgrad_scratch_floats(8, 8, u) == 0
    assert L.mg_conv_transpose1d_dgrad_workspace_floats(2, 64, 10, 32, 8) > 2 * 32 * 8 * 10
    assert L.mg_conv_transpose1d_wgrad_scratch_floats(64, 32, 8) >= 64 * 32 * 16
    # a workspace that is too small is its own error, also before any launch
    assert L.mg_conv_transpose1d_dgrad(p, p, p, p, p, 16, 1, 8, 8, 8, 2, 0.1, 1.0, None) == _lib.MG_ERR_WORKSPACE
    # log-mel gradient: L <= 512, ragged lengths, too many frames, a hop that is no power of two
    big = 1 << 30
    assert L.mg_stft_mel_bwd(p, 512, None, 1, 512, 256, p, p, p, p, 80, p, 3, p, 512, p, big, None) == S
    assert L.mg_stft_mel_bwd(p, 1024, p, 1, 1024, 256, p, p, p, p, 80, p, 5, p, 1024, p, big, None) == S
    assert L.mg_stft_mel_bwd(p, 1024, None, 1, 1024, 256, p, p, p, p, 80, p, 6, p, 1024, p, big, None) == S
    assert L.mg_stft_mel_bwd(p, 1024, None, 1, 1024, 200, p, p, p, p, 80, p, 5, p, 1024, p, big, None) == S
    assert L.mg_stft_mel_bwd(p, 1024, None, 1, 1024, 256, p, p, p, p, 80, p, 5, p, 1024, p, 16, None) == _lib.MG_ERR_WORKSPACE
    assert L.mg_stft_mel_bwd_workspace_bytes(2, 5) == 2 * 5 * 1024 * 4
    assert L.mg_lrelu_bwd(p, p, None, p, 0.1, 0, None) == S


def test_forward_train_on_a_cpu_tensor_raises():
    from oracle import refmath as R
    G = mg.vocoder.Generator(types.SimpleNamespace(**R.HIFIGAN_V1))
    with pytest.raises(mg.MixganHipError):
        G.forward_train(torch.zeros(1, 80, 4))


def test_forward_train_rejects_other_upsamplers_before_touching_the_gpu():
    from oracle import refmath as R
    cfg = dict(R.HIFIGAN_V1)
    cfg["upsample_rates"], cfg["upsample_kernel_sizes"] = [8, 8, 4], [16, 16, 7]
    G = mg.vocoder.Generator(types.SimpleNamespace(**cfg))

    class FakeCuda(torch.Tensor):
        is_cuda = True
    with pytest.raises(mg.MixganHipError, match="upsampler"):
        G.forward_train(torch.zeros(1, 80, 4).as_subclass(FakeCuda))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_reference_helper_masks_of_its_own_run_change_nothing(manifest, dtype):
    W, _ = seeded(manifest, "hifigan", 81)
    g = golden("hifigan")
    for k in g:
        if k.startswith("gain/"):
            W[k[5:]] = T(g[k])
    rng = np.random.default_rng(5)
    mel = torch.from_numpy(rng.uniform(-11.5, 2.0, (1, 80, 2)).astype(np.float32))
    cot = torch.from_numpy(rng.standard_normal((1, 1, 512)).astype(np.float32))
    a = HR.generator_grads(W, mel, cot, dtype)
    b = HR.generator_grads(W, mel, cot, dtype, masks=HR.masks_of(a["taps"]))
    assert set(a) == set(b) and len(a["taps"]) == 4 + 12 * 6 + 1
    for k in a:
        if k == "taps":
            for n in a[k]:
                assert torch.equal(a[k][n], b[k][n]), n
        else:
            assert a[k].dtype == dtype and torch.equal(a[k], b[k]), k


def test_inference_and_training_walk_the_same_sites(monkeypatch):
    """Generator._walk is the one traversal: with the library calls of the inference sites and the autograd entry points
    of the training sites replaced by shape-propagating recorders on CPU tensors, both modes visit the same sequence of
    (module, dilation, padding, alpha, leaky-ReLU slope on the input) for HiFi-GAN V1, every convolution once.  The
    inference path's fused post-activation counts as the next convolution's input slope."""
    from oracle import refmath as R
    from mixgan_tts_amd import ops, autograd as ag, vocoder
    G = vocoder.Generator(types.SimpleNamespace(**R.HIFIGAN_V1))
    path = {p.data_ptr(): n[:-len(".bias")] for n, p in G.named_parameters() if n.endswith(".bias")}
    sites = []

    def conv1d_packed(x, packed, bias, Co, K, stride=1, padding=0, act=None, alpha=1.0, add=None, out=None,
                      accumulate=False, dilation=1, in_slope=1.0, act_slope=0.0):
        fused = getattr(x, "post_slope", None)      # the producer's epilogue already applied this leaky ReLU
        assert fused is None or in_slope == 1.0
        sites.append((path[bias.data_ptr()], dilation, padding, alpha, in_slope if fused is None else fused))
        assert stride == 1 and (add is None or add.shape == x.shape) and (accumulate is False or out is not None)
        y = out if out is not None else torch.zeros(x.shape[0], Co, x.shape[2] + 2 * padding - dilation * (K - 1))
        if act == "lrelu_s":
            y.post_slope = act_slope
        return y

    def conv_transpose1d_packed(x, packed, bias, Co, u, in_slope=1.0, alpha=1.0):
        sites.append((path[bias.data_ptr()], 1, u // 2, alpha, in_slope))       # polyphase: padding u/2 by construction
        return torch.zeros(x.shape[0], Co, u * x.shape[2])

    def voc_conv(x, w, b, dil, pad, in_slope=1.0, alpha=1.0, act=None):
        sites.append((path[b.data_ptr()], dil, pad, alpha, in_slope))
        return torch.zeros(x.shape[0], w.shape[0], x.shape[2] + 2 * pad - dil * (w.shape[2] - 1))

    def voc_up(x, w, b, u, slope, alpha):
        sites.append((path[b.data_ptr()], 1, u // 2, alpha, slope))
        return torch.zeros(x.shape[0], w.shape[1], u * x.shape[2])

    def voc_pair(r, w1, b1, w2, b2, dil, pad1, pad2, slope):
        sites.append((path[b1.data_ptr()], dil, pad1, 1.0, slope))
        sites.append((path[b2.data_ptr()], 1, pad2, 1.0, slope))
        return torch.zeros_like(r), torch.zeros_like(r)

    monkeypatch.setattr(ops, "pack_conv_weight", lambda w, mode=None, out=None: w)
    monkeypatch.setattr(ops, "pack_conv_transpose_weight", lambda w: w)
    monkeypatch.setattr(ops, "conv1d_packed", conv1d_packed)
    monkeypatch.setattr(ops, "conv_transpose1d_packed", conv_transpose1d_packed)
    monkeypatch.setattr(ag, "voc_conv", voc_conv)
    monkeypatch.setattr(ag, "voc_up", voc_up)
    monkeypatch.setattr(ag, "voc_pair", voc_pair)
    mel = torch.zeros(1, 80, 2)
    with torch.no_grad():
        y = G._walk(mel, vocoder._Infer)
    infer, sites = sites, []
    taps = {}
    y_train = G._walk(mel, vocoder._Train, taps)
    assert tuple(y.shape) == tuple(y_train.shape) == (1, 1, 512)
    assert infer == sites
    assert sorted(s[0] for s in sites) == sorted(path.values()) and len(sites) == 1 + 4 + 12 * 6 + 1
    assert sites[0] == ("conv_pre", 1, 3, 1.0, 1.0) and sites[1] == ("ups.0", 1, 4, 1.0, 0.1)
    assert sites[2] == ("resblocks.0.convs1.0", 1, 1, 1.0, 0.1) and sites[-1] == ("conv_post", 1, 3, 1.0 / 3, 0.01)
    assert sites[-2] == ("resblocks.11.convs2.2", 1, 5, 1.0, 0.1) and sites[-3] == ("resblocks.11.convs1.2", 5, 25, 1.0, 0.1)
    assert sites[1 + 1 + 18] == ("ups.1", 1, 4, 1.0 / 3, 0.1)
    assert len(taps) == 4 + 12 * 6 + 1
