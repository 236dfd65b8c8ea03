"""Argument checks of the multi-period discriminator's entry points (csrc/mpd.hip) on real device buffers: null operands
give MG_ERR_ARG; Lin != R S_in, Lout != R S_out, S_in != stride S_out, a slot without two columns of slack
(H > S - 2), a (K, stride) outside {(5,3), (5,1), (3,1)}, a flat axis past 2^30 columns or a reflect pad that does not
fit give MG_ERR_SHAPE; and in every such case nothing is launched -- the outputs keep their sentinel."""
import pytest
import torch

from mixgan_tts_amd._lib import MG_ERR_ARG, MG_ERR_SHAPE, MG_OK, MG_PACK_PLAIN, MG_PACK_DGRAD, fptr, stream_ptr

pytestmark = pytest.mark.gpu
R, CI, CO, S_OUT, H_OUT = 6, 32, 128, 10, 8
S_IN, H_IN = 3 * S_OUT, 22
LIN, LOUT = R * S_IN, R * S_OUT


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def sentinel(*shape):
    return torch.full(shape, 7.0).cuda()


def untouched(*xs):
    torch.cuda.synchronize()
    return all(bool((x == 7.0).all()) for x in xs)


def test_period_convolutions(mg):
    L = mg.lib()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, CI, LIN, generator=g).cuda()
    d = torch.randn(1, CO, LOUT, generator=g).cuda()
    w = torch.randn(CO, CI, 5, generator=g).cuda()
    w1 = torch.randn(CI, CI, 5, generator=g).cuda()       # a stride-1 layer on the input's axis
    w3 = torch.randn(CI, CI, 3, generator=g).cuda()
    n3 = L.mg_period_dgrad3_packed_floats(CO, CI)
    assert n3 == 4 * (CO * 2 // 8) * 256                  # 96 rows -> four 32-row blocks; two taps of 128 channels
    packed3, out, dx, out1 = sentinel(n3), sentinel(1, CO, LOUT), sentinel(1, CI, LIN), sentinel(1, CI, LIN)
    scratch = sentinel(1 << 16)
    pf = mg.ops.pack_conv_weight(w, MG_PACK_PLAIN)
    pf1, pd1 = mg.ops.pack_conv_weight(w1, MG_PACK_PLAIN), mg.ops.pack_conv_weight(w1, MG_PACK_DGRAD)
    pf3 = mg.ops.pack_conv_weight(w3, MG_PACK_PLAIN)
    s = stream_ptr()

    def pack3(w_=fptr(w), p=fptr(packed3), co=CO, ci=CI):
        return L.mg_period_dgrad3_pack(w_, p, co, ci, s)

    def fwd(i=fptr(x), p=fptr(pf), o=fptr(out), r=R, lin=LIN, s_in=S_IN, lout=LOUT, s_out=S_OUT, h=H_OUT, k=5, st=3, act=0,
            sc=None):
        return L.mg_period_conv_fwd(i, p, None, o, r, CI, lin, s_in, CO, lout, s_out, h, k, st, act, 0.1, sc,
                                    0 if sc is None else scratch.numel(), s)

    def dgrad(i=fptr(d), p=fptr(packed3), o=fptr(dx), r=R, lin=LIN, s_in=S_IN, h=H_IN, lout=LOUT, s_out=S_OUT, k=5, st=3,
              sc=None):
        return L.mg_period_conv_dgrad(i, p, None, None, o, r, CI, lin, s_in, h, CO, lout, s_out, k, st, 0.1, sc,
                                      0 if sc is None else scratch.numel(), s)

    assert pack3(w_=None) == MG_ERR_ARG and pack3(p=None) == MG_ERR_ARG
    assert pack3(co=0) == MG_ERR_SHAPE and pack3(ci=-1) == MG_ERR_SHAPE
    assert L.mg_period_dgrad3_packed_floats(CO, 0) == 0
    for f in (fwd, dgrad):
        for nul in "ipo":
            assert f(**{nul: None}) == MG_ERR_ARG, (f.__name__, nul)
        assert f(lin=LIN + 1) == MG_ERR_SHAPE and f(lin=LIN - S_IN) == MG_ERR_SHAPE, f.__name__       # Lin != R S_in
        assert f(lout=LOUT + 1) == MG_ERR_SHAPE, f.__name__
        assert f(s_in=S_IN - 1, lin=R * (S_IN - 1)) == MG_ERR_SHAPE, f.__name__                         # S_in != 3 S_out
        assert f(st=1) == MG_ERR_SHAPE, f.__name__                                                      # S_in != 1 S_out
        assert f(st=2) == MG_ERR_SHAPE and f(k=7) == MG_ERR_SHAPE and f(k=3) == MG_ERR_SHAPE, f.__name__
        assert f(r=0, lin=0, lout=0) == MG_ERR_SHAPE, f.__name__
        assert f(h=0) == MG_ERR_SHAPE, f.__name__
        big = 2 ** 30 // S_IN + 1       # R S_in past 2^30: would not fit the kernel's int indices
        assert f(r=big, lin=(big * S_IN) % 2 ** 31, lout=(big * S_OUT) % 2 ** 31) == MG_ERR_SHAPE, f.__name__
    assert fwd(h=S_OUT - 1) == MG_ERR_SHAPE and fwd(h=S_OUT) == MG_ERR_SHAPE                            # H_out > S_out - 2
    assert dgrad(h=S_IN - 1) == MG_ERR_SHAPE
    assert fwd(act=1) == MG_ERR_ARG and fwd(act=5) == MG_ERR_ARG                                        # NONE or LRELU only
    assert fwd(sc=fptr(scratch), lin=LIN + 1) == MG_ERR_SHAPE
    assert untouched(packed3, out, dx, out1, scratch)
    assert pack3() == MG_OK and fwd() == MG_OK and dgrad() == MG_OK
    assert not untouched(packed3) and not untouched(out) and not untouched(dx)
    # the stride-1 forms on one axis: (5, 1) and (3, 1), forward and data gradient
    def fwd1(p, k):
        return L.mg_period_conv_fwd(fptr(x), fptr(p), None, fptr(out1), R, CI, LIN, S_IN, CI, LIN, S_IN, H_IN, k, 1, 4, 0.1,
                                    None, 0, s)
    assert fwd1(pf1, 5) == MG_OK and fwd1(pf3, 3) == MG_OK
    assert L.mg_period_conv_dgrad(fptr(x), fptr(pd1), None, None, fptr(out1), R, CI, LIN, S_IN, H_IN, CI, LIN, S_IN, 5, 1,
                                  0.1, None, 0, s) == MG_OK
    torch.cuda.synchronize()
    assert untouched(scratch)


def test_fold(mg):
    L = mg.lib()
    s = stream_ptr()
    N, T, p = 3, 100, 7
    H, S = mg.ops.period_geometry(T, p)
    y = torch.randn(N, T, generator=torch.Generator().manual_seed(1)).cuda()
    in0, dy = sentinel(N * p * S[0]), sentinel(N, T)
    assert L.mg_period_fold_fwd(None, fptr(in0), N, T, p, s) == MG_ERR_ARG
    assert L.mg_period_fold_fwd(fptr(y), None, N, T, p, s) == MG_ERR_ARG
    assert L.mg_period_fold_bwd(None, fptr(dy), N, T, p, s) == MG_ERR_ARG
    assert L.mg_period_fold_bwd(fptr(in0), None, N, T, p, s) == MG_ERR_ARG
    for bad in ((0, T, p), (N, 0, p), (N, T, 0), (N, 3, 7), (2 ** 24, 8192, 2)):      # 3 samples cannot mirror 4
        assert L.mg_period_fold_fwd(fptr(y), fptr(in0), *bad, s) == MG_ERR_SHAPE, bad
        assert L.mg_period_fold_bwd(fptr(in0), fptr(dy), *bad, s) == MG_ERR_SHAPE, bad
    assert untouched(in0, dy)
    assert L.mg_period_fold_fwd(fptr(y), fptr(in0), N, T, p, s) == MG_OK
    assert L.mg_period_fold_bwd(fptr(in0), fptr(dy), N, T, p, s) == MG_OK
    assert not untouched(in0) and not untouched(dy)
    d = mg.DiscriminatorP(7).cuda()
    with pytest.raises(mg.MixganHipError):
        d(torch.zeros(1, 1, 3).cuda())                                # the reflect pad does not fit
    with pytest.raises(mg.MixganHipError):
        d(torch.zeros(2, 2, 64).cuda())                               # not one channel: would fold as [N, T]
    with pytest.raises(mg.MixganHipError):
        d(torch.zeros(2, 64).cuda())
    with pytest.raises(mg.MixganHipError):
        d(torch.zeros(2, 1, 64, dtype=torch.float64).cuda())
    with pytest.raises(mg.MixganHipError):
        mg.autograd.period_stack(torch.zeros(2, 2, 64).cuda(), 7, 0.1)
