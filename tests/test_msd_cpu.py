"""CPU-side checks of the native multi-scale discriminator (hifigan_discriminators.py, csrc/msd.hip): its state dict is
the torch construction's (keys, order, shapes, which entries are buffers) and loads strictly both ways; the float64
restatement the GPU tests trust (tests/hifigan_msd_ref.py) equals the network built from torch's own Conv1d /
weight_norm / spectral_norm / AvgPool1d to 1e-10, power iterations included; the new names are exported, declared and
bound, and the C ABI rejects bad arguments before any launch."""
import ctypes
import re
import os

import pytest
import torch

from helpers import ROOT
import hifigan_msd_ref as MR

import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib

NEW = ("mg_gconv_packed_floats", "mg_gconv_pack", "mg_gconv1d_fwd", "mg_gconv1d_dgrad", "mg_gconv1d_wgrad_scratch_floats",
       "mg_gconv1d_wgrad", "mg_conv1d_c1_fwd", "mg_conv1d_c1_dgrad", "mg_conv1d_c1_wgrad_scratch_floats",
       "mg_conv1d_c1_wgrad", "mg_avgpool4s2_fwd", "mg_avgpool4s2_bwd")


@pytest.fixture(scope="module")
def torch_msd():
    torch.manual_seed(3)
    return MR.TorchMSD()


def test_state_dict_is_the_torch_construction(torch_msd):
    torch.manual_seed(4)
    native = mg.MultiScaleDiscriminator()
    ref, mine = torch_msd.state_dict(), native.state_dict()
    assert list(mine.keys()) == list(ref.keys())
    assert list(mine.keys()) == [n for n, _, _ in MR.msd_keys()]
    for k in ref:
        assert tuple(mine[k].shape) == tuple(ref[k].shape), k
        assert mine[k].dtype == ref[k].dtype, k
    assert [k for k, _ in native.named_parameters()] == [k for k, _ in torch_msd.named_parameters()]
    assert [k for k, _ in native.named_buffers()] == [k for k, _ in torch_msd.named_buffers()] == MR.buffer_names()
    assert [tuple(s) for _, s, _ in MR.msd_keys()] == [tuple(v.shape) for v in ref.values()]
    # attribute names and constructor arguments of the published code
    assert len(native.discriminators) == 3 and len(native.meanpools) == 2
    d = mg.DiscriminatorS(use_spectral_norm=True)
    assert len(d.convs) == 7 and hasattr(d, "conv_post") and "convs.0.weight_orig" in d.state_dict()
    assert "convs.0.weight_g" in mg.DiscriminatorS().state_dict()
    # initialised as torch initialises: g = |v| per row, unit u and v
    c = native.discriminators[1].convs[3]
    assert torch.allclose(c.weight_g.detach().flatten(), c.weight_v.detach().flatten(1).norm(dim=1))
    s = native.discriminators[0].convs[2]
    assert abs(float(s.weight_u.norm()) - 1) < 1e-5 and abs(float(s.weight_v.norm()) - 1) < 1e-5


def test_strict_loads_both_ways(torch_msd):
    torch.manual_seed(5)
    native = mg.MultiScaleDiscriminator()
    native.load_state_dict(torch_msd.state_dict(), strict=True)
    for k, v in torch_msd.state_dict().items():
        assert torch.equal(native.state_dict()[k], v), k
    torch.manual_seed(6)
    other = MR.TorchMSD()
    W = MR.msd_init(11)
    native.load_state_dict(W, strict=True)
    other.load_state_dict(native.state_dict(), strict=True)
    for k, v in W.items():
        assert torch.equal(other.state_dict()[k], v), k


def test_float64_restatement_equals_the_torch_built_network():
    """Train mode, two consecutive forwards (scale 0: four power iterations per layer), then eval mode: outputs, maps
    and u / v afterwards to 1e-10."""
    W = {k: v.double() for k, v in MR.msd_init(12).items()}
    net = MR.TorchMSD().double()
    net.load_state_dict(W, strict=True)
    W = {k: v.clone() for k, v in W.items()}
    gen = torch.Generator().manual_seed(13)
    y, y_hat = torch.randn(1, 1, 300, generator=gen).double(), torch.randn(1, 1, 300, generator=gen).double()

    def same(a, b, what):
        err = float((a - b).abs().max() / b.abs().max())
        assert a.shape == b.shape and err <= 1e-10, "%s: %.2e" % (what, err)

    def compare(train, tag):
        with torch.no_grad():
            got, ref = MR.msd_forward(W, y, y_hat, train=train), net(y, y_hat)
        for i in range(3):
            same(got[0][i], ref[0][i], "%s logits real %d" % (tag, i))
            same(got[1][i], ref[1][i], "%s logits gen %d" % (tag, i))
            assert len(got[2][i]) == len(ref[2][i]) == 8
            for j in range(8):
                same(got[2][i][j], ref[2][i][j], "%s fmap_r %d.%d" % (tag, i, j))
                same(got[3][i][j], ref[3][i][j], "%s fmap_g %d.%d" % (tag, i, j))
        for k in MR.buffer_names():
            same(W[k], net.state_dict()[k], "%s %s" % (tag, k))

    net.train()
    before = {k: W[k].clone() for k in MR.buffer_names()}
    compare(True, "train 1")
    # (conv_post has one output row: its u is the scalar 1 and stays)
    assert all(not torch.equal(before[k], W[k]) for k in before if W[k].numel() > 1), "the power iteration moves u and v"
    compare(True, "train 2")
    net.eval()
    before = {k: W[k].clone() for k in MR.buffer_names()}
    compare(False, "eval")
    assert all(torch.equal(before[k], W[k]) for k in before)
    # scale-0 lengths at T = 2083, the whole-module GPU test's size
    lens, L = [], 2083
    for _, _, k, s, _, p in MR.LAYERS + (MR.POST,):
        L = (L + 2 * p - k) // s + 1
        lens.append(L)
    assert lens == [2083, 1042, 521, 131, 33, 33, 33, 33]


def test_exported_declared_and_bound():
    assert mg.MultiScaleDiscriminator is mg.hifigan_discriminators.MultiScaleDiscriminator
    assert mg.DiscriminatorS is mg.hifigan_discriminators.DiscriminatorS
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mixgan_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(mg.library_path())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for fn in ("gconv_pack", "gconv1d_fwd", "gconv1d_dgrad", "gconv1d_wgrad", "conv1d_c1_fwd", "conv1d_c1_dgrad",
               "conv1d_c1_wgrad", "avgpool4s2_fwd", "avgpool4s2_bwd"):
        assert callable(getattr(mg.ops, fn)), fn
    assert (_lib.MG_GCONV_FWD, _lib.MG_GCONV_DGRAD) == (0, 1)


def test_abi_rejects_bad_arguments_before_any_launch():
    L = mg.lib()
    ARG, SHAPE = _lib.MG_ERR_ARG, _lib.MG_ERR_SHAPE
    one = ctypes.c_void_p(64)       # a non-null pointer that is never dereferenced: every check below fails first
    # the five instantiated forms, at the published widths and at G = 3
    for ci, co, s, g in ((128, 128, 2, 4), (128, 256, 2, 16), (256, 512, 4, 16), (512, 1024, 4, 16), (1024, 1024, 1, 16)):
        cig, cog = ci // g, co // g
        assert L.mg_gconv_packed_floats(ci, co, 41, s, g, 0) == g * ((cog + 31) // 32) * 41 * (cig // 2) * 64
        assert L.mg_gconv_packed_floats(ci, co, 41, s, g, 1) == g * ((cig + 31) // 32) * 41 * (cog // 2) * 64
        assert L.mg_gconv_packed_floats(3 * cig, 3 * cog, 41, s, 3, 0) == 3 * ((cog + 31) // 32) * 41 * (cig // 2) * 64
        assert L.mg_gconv1d_wgrad_scratch_floats(2, ci, co, 33, 41, s, g) >= co * cig * 41
    # forms it does not instantiate: K, stride, widths per group, a channel count the groups do not divide
    for ci, co, k, s, g in ((128, 128, 15, 2, 4), (128, 128, 41, 4, 4), (128, 128, 41, 2, 2), (64, 64, 41, 1, 16),
                            (130, 128, 41, 2, 4), (128, 128, 41, 2, 0)):
        assert L.mg_gconv_packed_floats(ci, co, k, s, g, 0) == 0
        assert L.mg_gconv1d_wgrad_scratch_floats(2, ci, co, 33, k, s, g) == 0
        assert L.mg_gconv_pack(one, one, ci, co, k, s, g, 0, None) == SHAPE
        lout = (64 + 40 - k) // s + 1
        assert L.mg_gconv1d_fwd(one, one, None, one, 2, ci, 64, co, lout, k, s, 20, g, 0, 0.0, None) == SHAPE
        assert L.mg_gconv1d_dgrad(one, one, None, None, one, 2, ci, 64, co, lout, k, s, 20, g, 0.1, None) == SHAPE
        assert L.mg_gconv1d_wgrad(one, one, one, one, 1 << 30, 2, ci, 64, co, lout, k, s, 20, g, None) == SHAPE
    assert L.mg_gconv_packed_floats(128, 128, 41, 2, 4, 2) == 0                     # no such pack mode
    assert L.mg_gconv_pack(one, one, 128, 128, 41, 2, 4, 2, None) == ARG
    # an output length that is not the convolution's, an activation it does not have, a scratch too small
    assert L.mg_gconv1d_fwd(one, one, None, one, 2, 128, 64, 128, 33, 41, 2, 20, 4, 0, 0.0, None) == SHAPE
    assert L.mg_gconv1d_fwd(one, one, None, one, 2, 128, 64, 128, 32, 41, 2, 20, 4, _lib.MG_ACT_TANH, 0.0, None) == ARG
    assert L.mg_gconv1d_wgrad(one, one, one, one, 16, 2, 128, 64, 128, 32, 41, 2, 20, 4, None) == _lib.MG_ERR_WORKSPACE
    # null pointers
    assert L.mg_gconv_pack(None, None, 128, 128, 41, 2, 4, 0, None) == ARG
    assert L.mg_gconv1d_fwd(None, None, None, None, 2, 128, 64, 128, 32, 41, 2, 20, 4, 0, 0.0, None) == ARG
    assert L.mg_gconv1d_dgrad(None, None, None, None, None, 2, 128, 64, 128, 32, 41, 2, 20, 4, 0.1, None) == ARG
    assert L.mg_gconv1d_wgrad(None, None, None, None, 0, 2, 128, 64, 128, 32, 41, 2, 20, 4, None) == ARG
    assert L.mg_conv1d_c1_fwd(None, None, None, None, 2, 64, 128, 15, 7, 0, 0.0, None) == ARG
    assert L.mg_conv1d_c1_dgrad(None, None, None, 2, 64, 128, 15, 7, None) == ARG
    assert L.mg_conv1d_c1_wgrad(None, None, None, None, None, 0, 2, 64, 128, 15, 7, None) == ARG
    assert L.mg_avgpool4s2_fwd(None, None, 2, 64, None) == ARG and L.mg_avgpool4s2_bwd(None, None, 2, 64, None) == ARG
    # the first layer and the pool: sizes they do not take
    assert L.mg_conv1d_c1_fwd(one, one, None, one, 2, 64, 128, 17, 8, 0, 0.0, None) == SHAPE          # K <= 16
    assert L.mg_conv1d_c1_fwd(one, one, None, one, 2, 3, 128, 15, 2, 0, 0.0, None) == SHAPE           # no output
    assert L.mg_conv1d_c1_wgrad_scratch_floats(2, 64, 128, 17) == 0
    assert L.mg_conv1d_c1_wgrad_scratch_floats(2, 64, 128, 15) >= 128 * 17
    assert L.mg_conv1d_c1_wgrad(one, one, one, None, one, 4, 2, 64, 128, 15, 7, None) == _lib.MG_ERR_WORKSPACE
    assert L.mg_avgpool4s2_fwd(one, one, 0, 64, None) == SHAPE and L.mg_avgpool4s2_bwd(one, one, 2, 0, None) == SHAPE


def test_native_forward_has_no_cpu_fallback():
    with pytest.raises(mg.MixganHipError):
        mg.MultiScaleDiscriminator()(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64))
