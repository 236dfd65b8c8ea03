"""Argument checks of the MelGAN training entry points (csrc/melgan_train.hip) on real device buffers: null operands
give MG_ERR_ARG; L <= p, a (K, dilation) pair without an instantiation, or a batch stride smaller than a plane give
MG_ERR_SHAPE; and in every such case nothing is launched -- the output keeps its sentinel."""
import pytest
import torch

from mixgan_tts_amd._lib import MG_ERR_ARG, MG_ERR_SHAPE, MG_OK, fptr, stream_ptr

pytestmark = pytest.mark.gpu
B, C, L, K, DIL = 2, 32, 40, 3, 3
P = DIL * (K - 1) // 2


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


@pytest.fixture()
def t(mg):
    g = torch.Generator().manual_seed(0)
    d = {"dy": torch.randn(B, C, L, generator=g).cuda(), "x": torch.randn(B, C, L, generator=g).cuda(),
         "w": torch.randn(C, C, K, generator=g).cuda(), "out": torch.full((B, C, L), 7.0).cuda(),
         "dw": torch.full((C, C, K), 7.0).cuda(), "pad": torch.randn(B, C, L + 2 * P, generator=g).cuda()}
    d["packed"] = mg.ops.pack_conv_weight(d["w"], mg.ops.PACK_DGRAD)
    d["scratch"] = torch.empty(mg.lib().mg_conv1d_wgrad_scratch_floats(C, C, K), device="cuda")
    d["ws"] = torch.empty(mg.lib().mg_conv1d_reflect_dgrad_workspace_floats(B, C, L, K, DIL), device="cuda")
    return d


def untouched(x):
    torch.cuda.synchronize()
    return bool((x == 7.0).all())


def test_reflect_wgrad_checks(mg, t):
    f = mg.lib().mg_conv1d_reflect_wgrad
    dy, x, dw, sc, s = fptr(t["dy"]), fptr(t["x"]), fptr(t["dw"]), fptr(t["scratch"]), stream_ptr()

    def call(dy=dy, dy_bs=0, x=x, x_bs=0, dw=dw, sc=sc, L_=L, K_=K, dil=DIL):
        return f(dy, dy_bs, x, x_bs, dw, sc, B, C, C, L_, K_, dil, 0.2, 1.0, 0, s)
    for nul in ("dy", "x", "dw", "sc"):
        assert call(**{nul: None}) == MG_ERR_ARG, nul
    assert call(L_=P) == MG_ERR_SHAPE                        # L <= p
    assert call(K_=3, dil=10) == MG_ERR_SHAPE and call(K_=7, dil=2) == MG_ERR_SHAPE and call(K_=5, dil=1) == MG_ERR_SHAPE
    assert call(x_bs=C * L - 1) == MG_ERR_SHAPE and call(dy_bs=C * L - 1) == MG_ERR_SHAPE and call(x_bs=-1) == MG_ERR_SHAPE
    assert untouched(t["dw"])
    assert call() == MG_OK
    assert not untouched(t["dw"])


def test_reflect_dgrad_checks(mg, t):
    f = mg.lib().mg_conv1d_reflect_dgrad
    dy, pk, x, out, ws, s = fptr(t["dy"]), fptr(t["packed"]), fptr(t["x"]), fptr(t["out"]), fptr(t["ws"]), stream_ptr()
    n = t["ws"].numel()

    def call(dy=dy, pk=pk, x=x, x_bs=0, add=None, add_bs=0, out=out, ws=ws, n_=n, L_=L, K_=K, dil=DIL):
        return f(dy, pk, x, x_bs, add, add_bs, out, ws, n_, B, C, C, L_, K_, dil, 0.2, 1.0, s)
    for nul in ("dy", "pk", "x", "out", "ws"):
        assert call(**{nul: None}) == MG_ERR_ARG, nul
    assert call(L_=P) == MG_ERR_SHAPE
    assert call(K_=3, dil=10) == MG_ERR_SHAPE and call(K_=7, dil=2) == MG_ERR_SHAPE and call(K_=5, dil=1) == MG_ERR_SHAPE
    assert call(x_bs=C * L - 1) == MG_ERR_SHAPE and call(add=x, add_bs=C * L - 1) == MG_ERR_SHAPE
    assert call(n_=n - 1) not in (MG_OK, MG_ERR_ARG, MG_ERR_SHAPE)      # workspace too small: its own code
    assert mg.lib().mg_conv1d_reflect_dgrad_workspace_floats(B, C, L, 3, 10) == 0
    assert n == B * C * (L + 2 * P)
    assert untouched(t["out"])
    assert call() == MG_OK
    assert not untouched(t["out"])


def test_reflect_fold_checks(mg, t):
    f = mg.lib().mg_reflect_fold_bwd
    pd, x, out, s = fptr(t["pad"]), fptr(t["x"]), fptr(t["out"]), stream_ptr()

    def call(pd=pd, p_bs=0, x=x, x_bs=0, add=None, add_bs=0, out=out, L_=L, p=P):
        return f(pd, p_bs, x, x_bs, add, add_bs, out, B, C, L_, p, 0.2, s)
    assert call(pd=None) == MG_ERR_ARG and call(out=None) == MG_ERR_ARG
    assert call(L_=P, p=P) == MG_ERR_SHAPE and call(p=-1) == MG_ERR_SHAPE
    assert call(p_bs=C * (L + 2 * P) - 1) == MG_ERR_SHAPE and call(x_bs=C * L - 1) == MG_ERR_SHAPE
    assert call(add=x, add_bs=C * L - 1) == MG_ERR_SHAPE and call(p_bs=-1) == MG_ERR_SHAPE
    assert untouched(t["out"])
    assert call() == MG_OK and call(x=None) == MG_OK           # no mask is allowed
    assert not untouched(t["out"])
