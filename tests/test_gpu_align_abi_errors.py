"""Error codes of the alignment entry points of the C ABI on a live GPU: every documented limit and the workspace
checks return their code before any launch, and leave the output buffers as they were."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_align_abi_errors():
    import mixgan_tts_amd as mg
    from mixgan_tts_amd import _lib
    L = mg.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    B, T, D, G, S = 2, 6, 5, 3, 4
    x = torch.randn(B, T, D, device="cuda")
    nf = torch.tensor([6, 4], device="cuda", dtype=torch.int32)
    A, Bm, c = -torch.rand(G, D, device="cuda"), torch.randn(G, D, device="cuda"), torch.randn(G, device="cuda")
    ll = torch.full((B, T, G), 7.0, device="cuda")

    def emis(x_=vp(x), nf_=vp(nf), A_=vp(A), c_=vp(c), ll_=vp(ll), B_=B, T_=T, D_=D, G_=G):
        return L.mg_align_emissions(x_, nf_, B_, T_, D_, A_, vp(Bm), c_, G_, ll_, None)

    assert emis(x_=None) == emis(nf_=None) == emis(A_=None) == emis(c_=None) == emis(ll_=None) == _lib.MG_ERR_ARG
    assert emis(B_=0) == emis(T_=0) == emis(D_=0) == emis(D_=_lib.MG_ALIGN_MAX_D + 1) == _lib.MG_ERR_SHAPE
    assert emis(G_=0) == emis(G_=_lib.MG_ALIGN_MAX_G + 1) == emis(B_=65536, T_=64) == _lib.MG_ERR_SHAPE
    torch.cuda.synchronize()
    assert (ll == 7.0).all()
    assert emis() == _lib.MG_OK

    seq = torch.tensor([[0, 1, 2, 0], [0, 2, 0, 0]], device="cuda", dtype=torch.int32)
    skip = torch.tensor([[1, 0, 0, 1], [1, 0, 1, 0]], device="cuda", dtype=torch.uint8)
    ns = torch.tensor([4, 3], device="cuda", dtype=torch.int32)
    dur = torch.full((B, S), -5, device="cuda", dtype=torch.int32)
    score = torch.full((B,), 3.5, device="cuda", dtype=torch.float64)
    ok = torch.full((B,), -5, device="cuda", dtype=torch.int32)
    need = L.mg_align_viterbi_workspace_bytes(B, T, S)
    assert need == B * T * 1 * 2 and L.mg_align_viterbi_workspace_bytes(B, T, 9) == B * T * 2 * 2
    assert L.mg_align_viterbi_workspace_bytes(0, T, S) == 0
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)

    def vit(ll_=vp(ll), seq_=vp(seq), skip_=vp(skip), dur_=vp(dur), score_=vp(score), ok_=vp(ok), ws_=vp(ws),
            bytes_=need, B_=B, T_=T, S_=S, G_=G):
        return L.mg_align_viterbi(ll_, seq_, skip_, vp(nf), vp(ns), B_, T_, S_, G_, dur_, score_, ok_, ws_, bytes_, None)

    assert vit(ll_=None) == vit(seq_=None) == vit(skip_=None) == vit(dur_=None) == vit(score_=None) == vit(ok_=None) \
        == _lib.MG_ERR_ARG
    assert vit(B_=0) == vit(T_=0) == vit(S_=0) == vit(G_=0) == _lib.MG_ERR_SHAPE
    assert vit(T_=_lib.MG_ALIGN_MAX_T + 1) == vit(S_=_lib.MG_ALIGN_MAX_S + 1) == vit(G_=_lib.MG_ALIGN_MAX_G + 1) \
        == _lib.MG_ERR_SHAPE
    assert vit(ws_=None) == vit(bytes_=need - 1) == vit(bytes_=0) == _lib.MG_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (dur == -5).all() and (ok == -5).all() and (score == 3.5).all()
    assert vit() == _lib.MG_OK
    torch.cuda.synchronize()
    assert ok.tolist() == [1, 1] and dur.sum(1).tolist() == [6, 4]

    fi = torch.arange(B * T, device="cuda", dtype=torch.int32)
    off = torch.tensor([0, 4, 4, 12], device="cuda", dtype=torch.int32)
    s1 = torch.full((G, D), 2.5, device="cuda", dtype=torch.float64)
    s2 = torch.full((G, D), 2.5, device="cuda", dtype=torch.float64)

    def stats(x_=vp(x), fi_=vp(fi), off_=vp(off), s1_=vp(s1), s2_=vp(s2), G_=G, D_=D):
        return L.mg_align_stats(x_, fi_, off_, G_, D_, s1_, s2_, None)

    assert stats(x_=None) == stats(fi_=None) == stats(off_=None) == stats(s1_=None) == stats(s2_=None) == _lib.MG_ERR_ARG
    assert stats(G_=0) == stats(G_=_lib.MG_ALIGN_MAX_G + 1) == stats(D_=0) == stats(D_=_lib.MG_ALIGN_MAX_D + 1) \
        == _lib.MG_ERR_SHAPE
    torch.cuda.synchronize()
    assert (s1 == 2.5).all() and (s2 == 2.5).all()
    assert stats() == _lib.MG_OK
    torch.cuda.synchronize()
    assert not s1[1].any() and torch.allclose(s1[0], x.reshape(-1, D)[:4].double().sum(0))
    with pytest.raises(mg.AlignGeometryError):
        mg.viterbi_align(ll, seq.cpu().numpy(), [[1, 1, 0, 0], [0, 0, 0, 0]], nf, ns)
