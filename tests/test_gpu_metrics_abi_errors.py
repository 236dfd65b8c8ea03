"""Error codes of the metric entry points of the C ABI on a live GPU: every null required pointer, every documented
limit and the workspace checks return their code before any launch, and leave the output buffers as they were."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_metrics_abi_errors():
    import mixgan_tts_amd as mg
    from mixgan_tts_amd import _lib
    L = mg.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    B, T, M, NC = 2, 6, 20, 5
    mel = torch.randn(B, T, M, device="cuda")
    nf = torch.tensor([6, 4], device="cuda", dtype=torch.int32)
    cep = torch.full((B, T, NC), 7.0, device="cuda")

    def cepstra(mel_=vp(mel), nf_=vp(nf), out_=vp(cep), B_=B, T_=T, M_=M, nc_=NC):
        return L.mg_mel_cepstra(mel_, nf_, B_, T_, M_, nc_, out_, None)

    assert cepstra(mel_=None) == cepstra(nf_=None) == cepstra(out_=None) == _lib.MG_ERR_ARG
    assert cepstra(B_=0) == cepstra(B_=65536) == cepstra(T_=0) == cepstra(M_=0) == cepstra(nc_=0) == _lib.MG_ERR_SHAPE
    assert cepstra(nc_=M) == cepstra(nc_=M + 1) == cepstra(M_=_lib.MG_CEPSTRA_MAX_M + 1) == _lib.MG_ERR_SHAPE
    torch.cuda.synchronize()
    assert (cep == 7.0).all()
    assert cepstra() == _lib.MG_OK
    torch.cuda.synchronize()
    assert not cep[1, 4:].any() and cep[0].any() and cep[1, :4].any()

    Ta, Tb, D = 6, 20, NC
    a, b = cep, torch.randn(B, Tb, D, device="cuda")
    la, lb = nf, torch.tensor([20, 17], device="cuda", dtype=torch.int32)
    total = torch.full((B,), 3.5, device="cuda")
    path_len = torch.full((B,), -5, device="cuda", dtype=torch.int32)
    path = torch.full((B, Ta + Tb - 1, 2), -5, device="cuda", dtype=torch.int32)
    need = L.mg_dtw_workspace_bytes(B, Ta, Tb)
    # two bits a cell, sixteen cells of a row to a word, and both operands feature-major at the largest D
    assert need == 4 * B * (2 * Ta + _lib.MG_DTW_MAX_D * (Ta + Tb))
    assert L.mg_dtw_workspace_bytes(1, 16, 16) == 4 * (16 + 64 * 32) and L.mg_dtw_workspace_bytes(1, 16, 17) == 4 * (32 + 64 * 33)
    assert L.mg_dtw_workspace_bytes(0, Ta, Tb) == L.mg_dtw_workspace_bytes(B, 0, Tb) == L.mg_dtw_workspace_bytes(B, Ta, 0) == 0
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)

    def dtw(a_=vp(a), b_=vp(b), la_=vp(la), lb_=vp(lb), total_=vp(total), pl_=vp(path_len), path_=vp(path), ws_=vp(ws),
            bytes_=need, B_=B, Ta_=Ta, Tb_=Tb, D_=D):
        return L.mg_dtw(a_, b_, la_, lb_, B_, Ta_, Tb_, D_, total_, pl_, path_, ws_, bytes_, None)

    assert dtw(a_=None) == dtw(b_=None) == dtw(la_=None) == dtw(lb_=None) == dtw(total_=None) == dtw(pl_=None) \
        == _lib.MG_ERR_ARG
    assert dtw(B_=0) == dtw(Ta_=0) == dtw(Tb_=0) == dtw(D_=0) == _lib.MG_ERR_SHAPE
    assert dtw(Ta_=_lib.MG_DTW_MAX_T + 1) == dtw(Tb_=_lib.MG_DTW_MAX_T + 1) == dtw(D_=_lib.MG_DTW_MAX_D + 1) \
        == _lib.MG_ERR_SHAPE
    assert dtw(ws_=None) == dtw(bytes_=need - 1) == dtw(bytes_=0) == _lib.MG_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (total == 3.5).all() and (path_len == -5).all() and (path == -5).all()
    assert dtw() == _lib.MG_OK
    torch.cuda.synchronize()
    assert (total > 0).all() and path_len.tolist()[0] >= 20 and path_len.tolist()[1] >= 17
    assert path[0, 0].tolist() == [0, 0] and path[0, path_len[0] - 1].tolist() == [5, 19]
    assert path[1, path_len[1] - 1].tolist() == [3, 16] and (path[1, path_len[1]:] == -1).all()
    # the path is optional
    total2 = torch.empty_like(total)
    assert dtw(total_=vp(total2), path_=None) == _lib.MG_OK
    torch.cuda.synchronize()
    assert torch.equal(total2, total)
    with pytest.raises(mg.DtwGeometryError):
        mg.dtw(torch.zeros(1, _lib.MG_DTW_MAX_T + 1, 2, device="cuda"), torch.zeros(1, 4, 2, device="cuda"))
