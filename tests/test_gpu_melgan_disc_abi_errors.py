"""Argument checks of the MelGAN discriminator's entry points (csrc/msd.hip, csrc/gconv_c4.h, csrc/losses.hip) on real
device buffers: null operands give MG_ERR_ARG; a form without an instantiation -- (4, 8, 4), K = 40, stride 2 with four
channels per group -- a mismatched Lout, a pool of one sample, a reflection pad as long as its row or an unknown loss
mode give MG_ERR_SHAPE; and in every such case nothing is launched -- the outputs keep their sentinel."""
import pytest
import torch

from mixgan_tts_amd import _lib
from mixgan_tts_amd._lib import MG_ERR_ARG, MG_ERR_SHAPE, MG_OK, fptr, stream_ptr

pytestmark = pytest.mark.gpu
N, G, CIG, COG, LIN, K, S, PAD = 2, 3, 4, 16, 64, 41, 4, 20
LOUT = (LIN + 2 * PAD - K) // S + 1


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def sentinel(*shape):
    return torch.full(shape, 7.0).cuda()


def untouched(*xs):
    torch.cuda.synchronize()
    return all(bool((x == 7.0).all()) for x in xs)


def test_grouped_entry_points(mg):
    L = mg.lib()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, CIG * G, LIN, generator=g).cuda()
    w = torch.randn(COG * G, CIG, K, generator=g).cuda()
    dy = torch.randn(N, COG * G, LOUT, generator=g).cuda()
    n_pack = L.mg_gconv_packed_floats(CIG * G, COG * G, K, S, G, 0)
    assert n_pack == COG * G * CIG * K
    packed, out, dx, dw = sentinel(n_pack), sentinel(N, COG * G, LOUT), sentinel(N, CIG * G, LIN), sentinel(COG * G, CIG, K)
    n_scr = L.mg_gconv1d_wgrad_scratch_floats(N, CIG * G, COG * G, LOUT, K, S, G)
    scratch = sentinel(n_scr)
    s = stream_ptr()

    def pack(w_=fptr(w), p=fptr(packed), co=COG * G, k=K, st=S, mode=0):
        return L.mg_gconv_pack(w_, p, CIG * G, co, k, st, G, mode, s)

    def fwd(i=fptr(x), p=fptr(packed), o=fptr(out), co=COG * G, lout=LOUT, k=K, st=S):
        return L.mg_gconv1d_fwd(i, p, None, o, N, CIG * G, LIN, co, lout, k, st, PAD, G, 0, 0.0, s)

    def dgrad(d=fptr(dy), p=fptr(packed), o=fptr(dx), co=COG * G, lout=LOUT, k=K, st=S):
        return L.mg_gconv1d_dgrad(d, p, None, None, o, N, CIG * G, LIN, co, lout, k, st, PAD, G, 1.0, s)

    def wgrad(d=fptr(dy), i=fptr(x), o=fptr(dw), sc=fptr(scratch), co=COG * G, lout=LOUT, k=K, st=S):
        return L.mg_gconv1d_wgrad(d, i, o, sc, n_scr, N, CIG * G, LIN, co, lout, k, st, PAD, G, s)

    assert pack(w_=None) == MG_ERR_ARG and pack(p=None) == MG_ERR_ARG and pack(mode=2) == MG_ERR_ARG
    for f, nulls in ((fwd, "ipo"), (dgrad, "dpo"), (wgrad, "dio")):
        for nul in nulls:
            assert f(**{nul: None}) == MG_ERR_ARG, (f.__name__, nul)
    assert wgrad(sc=None) == MG_ERR_ARG
    for f in (pack, fwd, dgrad, wgrad):
        assert f(co=8 * G) == MG_ERR_SHAPE, f.__name__            # (4, 8, 4)
        assert f(k=40) == MG_ERR_SHAPE, f.__name__
        assert f(st=2) == MG_ERR_SHAPE, f.__name__                # stride 2 exists only for wider groups
    for f in (fwd, dgrad, wgrad):
        assert f(lout=LOUT + 1) == MG_ERR_SHAPE and f(lout=LOUT - 1) == MG_ERR_SHAPE, f.__name__
    assert L.mg_gconv_packed_floats(CIG * G, 8 * G, K, S, G, 0) == 0
    assert L.mg_gconv1d_wgrad_scratch_floats(N, CIG * G, COG * G, LOUT, 40, S, G) == 0
    assert untouched(packed, out, dx, dw, scratch)
    assert pack() == MG_OK and fwd() == MG_OK and wgrad() == MG_OK
    assert pack(mode=1) == MG_OK and dgrad() == MG_OK
    assert not untouched(out) and not untouched(dx) and not untouched(dw)


def test_pool_and_reflect_pad(mg):
    L = mg.lib()
    s = stream_ptr()
    x = torch.randn(3, 16, generator=torch.Generator().manual_seed(1)).cuda()
    out, dx, padded = sentinel(3, 8), sentinel(3, 16), sentinel(3, 30)
    assert L.mg_avgpool4s2p1_fwd(None, fptr(out), 3, 16, s) == MG_ERR_ARG
    assert L.mg_avgpool4s2p1_fwd(fptr(x), None, 3, 16, s) == MG_ERR_ARG
    assert L.mg_avgpool4s2p1_bwd(None, fptr(dx), 3, 16, s) == MG_ERR_ARG
    assert L.mg_avgpool4s2p1_bwd(fptr(out), None, 3, 16, s) == MG_ERR_ARG
    assert L.mg_avgpool4s2p1_fwd(fptr(x), fptr(out), 3, 1, s) == MG_ERR_SHAPE
    assert L.mg_avgpool4s2p1_bwd(fptr(out), fptr(dx), 3, 1, s) == MG_ERR_SHAPE
    assert L.mg_avgpool4s2p1_fwd(fptr(x), fptr(out), 0, 16, s) == MG_ERR_SHAPE
    assert L.mg_reflect_pad1d_fwd(None, fptr(padded), 3, 16, 7, s) == MG_ERR_ARG
    assert L.mg_reflect_pad1d_fwd(fptr(x), None, 3, 16, 7, s) == MG_ERR_ARG
    assert L.mg_reflect_pad1d_bwd(None, fptr(dx), 3, 16, 7, s) == MG_ERR_ARG
    assert L.mg_reflect_pad1d_bwd(fptr(padded), None, 3, 16, 7, s) == MG_ERR_ARG
    assert L.mg_reflect_pad1d_fwd(fptr(x), fptr(padded), 3, 7, 7, s) == MG_ERR_SHAPE       # T = 7
    assert L.mg_reflect_pad1d_bwd(fptr(padded), fptr(dx), 3, 7, 7, s) == MG_ERR_SHAPE
    assert L.mg_reflect_pad1d_fwd(fptr(x), fptr(padded), 3, 16, -1, s) == MG_ERR_SHAPE
    assert untouched(out, dx, padded)
    assert L.mg_avgpool4s2p1_fwd(fptr(x), fptr(out), 3, 16, s) == MG_OK
    assert L.mg_reflect_pad1d_fwd(fptr(x), fptr(padded), 3, 16, 7, s) == MG_OK
    assert L.mg_reflect_pad1d_bwd(fptr(padded), fptr(dx), 3, 16, 7, s) == MG_OK
    assert not untouched(out) and not untouched(dx) and not untouched(padded)
    with pytest.raises(mg.MixganHipError):
        mg.ops.avgpool4s2_fwd(torch.zeros(1, 1, 1).cuda(), padding=1, count_include_pad=False)
    with pytest.raises(mg.MixganHipError):
        mg.ops.reflect_pad1d_fwd(torch.zeros(1, 1, 7).cuda(), 7)


def test_unknown_loss_mode(mg):
    L = mg.lib()
    a, da = torch.randn(100).cuda(), sentinel(100)
    scratch = torch.zeros(L.mg_multi_loss_scratch_floats()).cuda()
    out = sentinel(1 + _lib.MG_LOSS_GROUPS + 1)
    g = torch.ones(1).cuda()
    for mode in (4, -1):
        terms = (_lib.LossTerm * 1)(_lib.LossTerm(fptr(a).value, None, fptr(da).value, 100, 1.0, 1.0, mode, 0))
        assert L.mg_multi_loss_fwd(terms, 1, fptr(scratch), fptr(out), stream_ptr()) == MG_ERR_SHAPE
        assert L.mg_multi_loss_bwd(terms, 1, fptr(g), stream_ptr()) == MG_ERR_SHAPE
    assert untouched(out, da) and float(scratch.abs().max()) == 0.0
    terms = (_lib.LossTerm * 1)(_lib.LossTerm(None, None, None, 100, 1.0, 1.0, _lib.MG_LOSSMODE_HINGE, 0))
    assert L.mg_multi_loss_fwd(terms, 1, fptr(scratch), fptr(out), stream_ptr()) == MG_ERR_ARG
    terms = (_lib.LossTerm * 1)(_lib.LossTerm(fptr(a).value, None, fptr(da).value, 100, 1.0, 1.0, _lib.MG_LOSSMODE_HINGE, 0))
    assert L.mg_multi_loss_fwd(terms, 1, fptr(scratch), fptr(out), stream_ptr()) == MG_OK
    assert L.mg_multi_loss_bwd(terms, 1, fptr(g), stream_ptr()) == MG_OK
    assert not untouched(out) and not untouched(da)
