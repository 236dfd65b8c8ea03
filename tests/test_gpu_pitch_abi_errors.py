"""Error codes of the pitch entry points of the C ABI on a live GPU: every bad call returns before any launch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_pitch_abi_errors():
    import mixgan_tts_amd as mg
    from mixgan_tts_amd import _lib
    from mixgan_tts_amd.pitch import _twiddle
    L = mg.lib()
    B, N, hop, T, K = 2, 1000, 256, 4, _lib.MG_PITCH_K
    x = torch.zeros(B, N, device="cuda")
    tw = _twiddle(x.device)
    per, cst = torch.zeros(B, T, K, device="cuda"), torch.zeros(B, T, K, device="cuda")
    rms, nf = torch.zeros(B, T, device="cuda"), torch.full((B,), T, device="cuda", dtype=torch.int32)
    f, i = _lib.fptr, _lib.iptr

    def yin(x_=f(x), tw_=f(tw), per_=f(per), rms_=f(rms), B_=B, hop_=hop, lo=27, hi=311, T_=T, bs=N):
        return L.mg_yin_candidates(x_, bs, None, B_, N, hop_, lo, hi, tw_, per_, f(cst), rms_, T_, None)

    assert yin() == _lib.MG_OK
    assert yin(x_=None) == yin(tw_=None) == yin(per_=None) == yin(rms_=None) == _lib.MG_ERR_ARG
    assert yin(hop_=0) == yin(hop_=-256) == _lib.MG_ERR_SHAPE
    assert yin(B_=0) == yin(T_=0) == yin(T_=T + 1) == yin(bs=N - 1) == _lib.MG_ERR_SHAPE
    assert yin(lo=1) == _lib.MG_ERR_SHAPE                      # tau_min < 2
    assert yin(hi=512) == _lib.MG_ERR_SHAPE                    # tau_max + 1 > N - W: 44100 Hz with a 71 Hz floor
    assert yin(lo=312) == _lib.MG_ERR_SHAPE                    # an empty lag range

    need = L.mg_pitch_track_workspace_bytes(B, T)
    assert need == B * T * 4 and L.mg_pitch_track_workspace_bytes(0, T) == 0
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    f0 = torch.zeros(B, T, device="cuda", dtype=torch.float64)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    good = [22050.0, 311.0, 0.15, 0.05, 0.5, 0.1, 10 ** -2.5]

    def track(per_=f(per), nf_=i(nf, torch.int32), params=good, f0_=vp(f0), ws_=vp(ws), bytes_=need, B_=B):
        p = None if params is None else (ctypes.c_double * len(params))(*params)
        return L.mg_pitch_track(per_, f(cst), f(rms), nf_, B_, T, p, f0_, ws_, bytes_, None)

    assert track() == _lib.MG_OK
    assert track(per_=None) == track(nf_=None) == track(params=None) == track(f0_=None) == _lib.MG_ERR_ARG
    assert track(B_=0) == _lib.MG_ERR_SHAPE
    assert track(params=[0.0] + good[1:]) == _lib.MG_ERR_SHAPE                 # no sampling rate
    assert track(params=[44100.0, 622.0] + good[2:]) == _lib.MG_ERR_SHAPE      # tau_max beyond the analysis span
    assert track(bytes_=need - 1) == track(ws_=None) == _lib.MG_ERR_WORKSPACE
    torch.cuda.synchronize()
    with pytest.raises(mg.MixganHipError):
        _lib.check(_lib.MG_ERR_WORKSPACE)
