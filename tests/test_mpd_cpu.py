"""CPU-side checks of the native multi-period discriminator (hifigan_discriminators.py, csrc/mpd.hip): the slot geometry
against a brute-force walk, the state dict against the torch construction (weight_norm(Conv2d)) and
hifigan_disc_ref.mpd_keys(), strict loads both ways, the constructor and device errors, the exports and the plan of the
period case list."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn
from torch.nn.utils import weight_norm

from helpers import ROOT
import hifigan_disc_ref as DR

import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib

NEW = ("mg_period_geometry", "mg_period_fold_fwd", "mg_period_fold_bwd", "mg_period_conv_fwd",
       "mg_period_dgrad3_packed_floats", "mg_period_dgrad3_pack", "mg_period_conv_dgrad")


def geometry(T, p):
    H, S = (ctypes.c_int * 7)(), (ctypes.c_int * 7)()
    rc = mg.lib().mg_period_geometry(T, p, H, S)
    return rc, list(H), list(S)


def walk(T, p):
    """The published forward's heights, by its own steps: pad, view, then Conv2d's output-size rule per layer."""
    pad = (p - T % p) % p
    if pad >= T:      # F.pad(..., "reflect") needs pad < T
        return None
    H = [(T + pad) // p]
    for j in range(4):
        H.append(len(range(0, H[-1] + 2 * 2 - 5 + 1, 3)))       # Conv2d((5,1), (3,1), (2,0))
    H.append(H[-1] + 2 * 2 - 5 + 1)                                 # stride 1, K = 5, padding 2
    H.append(H[-1] + 2 * 1 - 3 + 1)                                 # conv_post: K = 3, padding 1
    return H


@pytest.mark.parametrize("p", DR.PERIODS)
def test_geometry_against_a_brute_force_walk(p):
    for T in list(range(1, 401)) + [8192, 8193]:
        rc, H, S = geometry(T, p)
        ref = walk(T, p)
        if ref is None:
            assert T <= p - 1 - (T - 1) % p
            assert rc == _lib.MG_ERR_SHAPE, (T, p)
            continue
        assert T > p - 1 - (T - 1) % p
        assert rc == _lib.MG_OK and H == ref, (T, p, H, ref)
        assert S[4] == S[5] == S[6] == H[4] + 2
        for j in range(4):
            assert S[j] == 3 * S[j + 1]
        for j in range(7):
            assert S[j] >= H[j] + 2, (T, p, j)
        assert mg.ops.period_geometry(T, p) == (H, S)


def test_geometry_rejects():
    H, S = (ctypes.c_int * 7)(), (ctypes.c_int * 7)()
    L = mg.lib()
    assert L.mg_period_geometry(0, 2, H, S) == _lib.MG_ERR_SHAPE
    assert L.mg_period_geometry(-5, 2, H, S) == _lib.MG_ERR_SHAPE
    assert L.mg_period_geometry(100, 0, H, S) == _lib.MG_ERR_SHAPE
    assert L.mg_period_geometry(1, 3, H, S) == _lib.MG_ERR_SHAPE          # pad 2 on one sample
    assert L.mg_period_geometry(5, 11, H, S) == _lib.MG_ERR_SHAPE         # pad 6 on five samples
    assert L.mg_period_geometry(6, 11, H, S) == _lib.MG_OK                # pad 5 on six
    assert L.mg_period_geometry(100, 2, None, S) == _lib.MG_ERR_ARG
    assert L.mg_period_geometry(100, 2, H, None) == _lib.MG_ERR_ARG
    assert L.mg_period_geometry(2 ** 31 - 1, 1, H, S) == _lib.MG_ERR_SHAPE      # 81 (H4 + 2) would not fit
    with pytest.raises(mg.MixganHipError):
        mg.ops.period_geometry(1, 3)


class TorchDiscriminatorP(nn.Module):
    """The published construction's parameters."""

    def __init__(self, period):
        super().__init__()
        self.period = period
        ch = DR.MPD_CHANNELS
        self.convs = nn.ModuleList([weight_norm(nn.Conv2d(ch[j], ch[j + 1], (5, 1), (3 if j < 4 else 1, 1), padding=(2, 0)))
                                    for j in range(5)])
        self.conv_post = weight_norm(nn.Conv2d(1024, 1, (3, 1), 1, padding=(1, 0)))


class TorchMPD(nn.Module):
    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([TorchDiscriminatorP(p) for p in DR.PERIODS])


@pytest.fixture(scope="module")
def torch_mpd():
    torch.manual_seed(3)
    return TorchMPD()


def test_state_dict_is_the_torch_construction(torch_mpd):
    torch.manual_seed(4)
    native = mg.MultiPeriodDiscriminator()
    ref, mine = torch_mpd.state_dict(), native.state_dict()
    assert list(mine.keys()) == list(ref.keys())
    keys = DR.mpd_keys()
    assert set(mine.keys()) == set(keys)
    for k in ref:
        assert tuple(mine[k].shape) == tuple(ref[k].shape) == tuple(keys[k]), k
        assert mine[k].dtype == ref[k].dtype, k
    assert [k for k, _ in native.named_parameters()] == [k for k, _ in torch_mpd.named_parameters()]
    assert not list(native.named_buffers())
    # attribute names of the published code
    assert [d.period for d in native.discriminators] == list(DR.PERIODS)
    d = mg.DiscriminatorP(7)
    assert d.period == 7 and len(d.convs) == 5 and hasattr(d, "conv_post")
    c = native.discriminators[2].convs[3]
    assert torch.allclose(c.weight_g.detach().flatten(), c.weight_v.detach().flatten(1).norm(dim=1))
    assert mg.MultiPeriodDiscriminator is mg.hifigan_discriminators.MultiPeriodDiscriminator
    assert mg.DiscriminatorP is mg.hifigan_discriminators.DiscriminatorP


def test_strict_loads_both_ways(torch_mpd):
    torch.manual_seed(5)
    native = mg.MultiPeriodDiscriminator()
    native.load_state_dict(torch_mpd.state_dict(), strict=True)
    for k, v in torch_mpd.state_dict().items():
        assert torch.equal(native.state_dict()[k], v), k
    W = DR.mpd_init(11)
    native.load_state_dict(W, strict=True)
    torch.manual_seed(6)
    other = TorchMPD()
    other.load_state_dict(native.state_dict(), strict=True)
    for k, v in W.items():
        assert torch.equal(other.state_dict()[k], v), k


def test_effective_weight_is_weight_norm():
    W = DR.mpd_init(12)
    d = mg.DiscriminatorP(3)
    d.load_state_dict({k[len("discriminators.1."):]: v for k, v in W.items() if k.startswith("discriminators.1.")},
                      strict=True)
    for name, conv in [("convs.%d" % j, c) for j, c in enumerate(d.convs)] + [("conv_post", d.conv_post)]:
        ref = DR.wn(W, "discriminators.1." + name)
        got = conv.effective_weight()
        assert got.dim() == 3 and torch.allclose(got, ref.squeeze(3), rtol=1e-6, atol=0)


@pytest.mark.parametrize("kw", [{"kernel_size": 3}, {"stride": 2}, {"use_spectral_norm": True}])
def test_unsupported_constructor_arguments_raise(kw):
    with pytest.raises(mg.MixganHipError) as e:
        mg.DiscriminatorP(2, **kw)
    assert isinstance(e.value, NotImplementedError)
    assert type(e.value) is mg.hifigan_discriminators.UnsupportedPeriodConfig
    mg.DiscriminatorP(2, kernel_size=5, stride=3, use_spectral_norm=False)


def test_cpu_tensors_raise():
    with pytest.raises(mg.MixganHipError):
        mg.DiscriminatorP(2)(torch.zeros(1, 1, 64))
    with pytest.raises(mg.MixganHipError):
        mg.MultiPeriodDiscriminator()(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64))


def test_exported_declared_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mixgan_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(mg.library_path())
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name + " is not declared in the header"
        assert name in _lib.EXPORTS
    assert re.search(r"^#define\s+MG_CONV_EPI_PERIOD\s+%d\s*$" % _lib.MG_CONV_EPI_PERIOD, header, re.M)


def test_plan_of_the_period_case_list():
    L = mg.lib()
    plan = _lib.ConvPlan()

    def ask(K, stride, rows=512, Ci=128, Lout=5000, epi=_lib.MG_CONV_EPI_PERIOD):
        return L.mg_conv1d_fwd_plan(1, Ci, Lout, rows, K, stride, 1, 0, epi, ctypes.byref(plan))

    for K, stride, ck in ((5, 3, 16), (5, 1, 16), (3, 1, 32), (2, 1, 32)):
        assert ask(K, stride) == _lib.MG_OK
        assert (plan.kw, plan.stride, plan.ck, plan.dilmax) == (K, stride, ck, 1)
        assert plan.grid >= 1 and plan.ksplit == 1
    assert ask(5, 2) == _lib.MG_ERR_SHAPE
    assert ask(9, 1) == _lib.MG_ERR_SHAPE
    assert ask(5, 3, epi=_lib.MG_CONV_EPI_PLAIN) == _lib.MG_ERR_SHAPE      # the existing lists did not grow
    assert ask(5, 2, epi=_lib.MG_CONV_EPI_PLAIN) == _lib.MG_OK
    # the deep period-11 layer is a handful of tiles: with scratch the reduction is split
    assert L.mg_conv1d_fwd_plan(1, 1024, 32 * 11 * 5, 1024, 5, 1, 1, 12 << 20, _lib.MG_CONV_EPI_PERIOD,
                                ctypes.byref(plan)) == _lib.MG_OK
    assert plan.ksplit > 1


def test_argument_checks_return_before_any_launch():
    """Null pointers and geometry errors are decided on the host: no GPU is needed to see them."""
    L = mg.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: every call below fails its checks
    ok = dict(R=6, Ci=32, Lin=6 * 30, S_in=30, Co=128, Lout=6 * 10, S_out=10, H_out=8, K=5, stride=3)

    def fwd(**kw):
        a = dict(ok, **kw)
        return L.mg_period_conv_fwd(a.get("inp", one), one, None, one, a["R"], a["Ci"], a["Lin"], a["S_in"], a["Co"],
                                    a["Lout"], a["S_out"], a["H_out"], a["K"], a["stride"], _lib.MG_ACT_NONE, 0.0, None, 0,
                                    None)

    assert fwd(inp=None) == _lib.MG_ERR_ARG
    for bad in ({"Lin": 181}, {"Lout": 61}, {"S_in": 29}, {"H_out": 9}, {"H_out": 0}, {"stride": 2}, {"K": 7},
                {"K": 3}, {"R": 2 ** 26, "Lin": 0}):
        assert fwd(**bad) == _lib.MG_ERR_SHAPE, bad
    assert L.mg_period_fold_fwd(None, one, 2, 100, 3, None) == _lib.MG_ERR_ARG
    assert L.mg_period_fold_fwd(one, one, 2, 1, 3, None) == _lib.MG_ERR_SHAPE
    assert L.mg_period_fold_bwd(one, one, 0, 100, 3, None) == _lib.MG_ERR_SHAPE
    assert L.mg_period_dgrad3_packed_floats(0, 5) == 0
    assert L.mg_period_dgrad3_packed_floats(128, 32) == 4 * (128 * 2 // 8) * 256
    assert L.mg_period_dgrad3_pack(None, one, 128, 32, None) == _lib.MG_ERR_ARG
    assert L.mg_period_dgrad3_pack(one, one, 0, 32, None) == _lib.MG_ERR_SHAPE
