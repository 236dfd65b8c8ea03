"""Objective synthesis metrics (csrc/dtw.hip): mel-cepstral distortion (MCD) along a
dynamic-time-warping (DTW) path, and log-F0 RMSE and voiced/unvoiced error read along the same path.

A free-running synthesis predicts its own durations, so its mel cannot be compared with the recording frame by
frame: the two are first aligned.  The cepstra are coefficients 1..n_coef of the orthonormal DCT-II of this project's
natural-log mel (`TacotronSTFT.mel_spectrogram`, the model's output), not WORLD / SPTK mel-cepstra: the figures are
comparable within this project only.  tests/metrics_ref.py restates every figure in float64 numpy.

    cep = mel_cepstra(mel, lengths)                      # [B, T, n_coef]
    total, path_len, path = dtw(cep_ref, cep_syn, ref_lens, syn_lens, return_path=True)
    mcd = mel_cepstral_distortion(mel_ref, mel_syn, ref_lens, syn_lens)      # [B] dB
    report = evaluate_model(model, batch)                # free-running inference against the batch's mel targets
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import fptr, iptr, check, stream_ptr, MixganHipError

MAX_M, MAX_T, MAX_D = _lib.MG_CEPSTRA_MAX_M, _lib.MG_DTW_MAX_T, _lib.MG_DTW_MAX_D
MCD_SCALE = 10.0 / math.log(10.0) * math.sqrt(2.0)


class DtwGeometryError(MixganHipError, NotImplementedError):
    """A shape the metric kernels do not take."""


def _geometry(ok, message):
    if not ok:
        raise DtwGeometryError("metrics: " + message)


def _dtw_geometry(B, Ta, Tb, D):
    _geometry(B >= 1 and 1 <= Ta <= MAX_T and 1 <= Tb <= MAX_T and 1 <= D <= MAX_D,
              "the DTW takes 1 <= Ta, Tb <= %d frames of 1 <= D <= %d features, got B=%d Ta=%d Tb=%d D=%d"
              % (MAX_T, MAX_D, B, Ta, Tb, D))


def _dev(t, what, dtype):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise MixganHipError("metrics: %s must be a CUDA tensor: the HIP path has no CPU fallback" % what)
    return t.to(dtype).contiguous()


def _lengths(lens, B, T, device, what):
    """int32 [B] on the device; None: every row is T long."""
    if lens is None:
        return torch.full((B,), T, device=device, dtype=torch.int32)
    if not isinstance(lens, torch.Tensor):
        lens = torch.as_tensor(np.asarray(lens))
    if tuple(lens.shape) != (B,):
        raise ValueError("metrics: %s must have shape [%d], got %s" % (what, B, tuple(lens.shape)))
    return lens.to(device=device, dtype=torch.int32).contiguous()


# ---------------------------------------------------------------------------------------------
# The kernel calls
# ---------------------------------------------------------------------------------------------
def mel_cepstra(mel, lengths=None, n_coef=13):
    """mel [B, T, M] natural-log mel on the device, lengths int [B] (None: all T) -> float32 [B, T, n_coef]:
    coefficients 1..n_coef of the orthonormal DCT-II over the bins, zero at and past a row's length."""
    if not isinstance(mel, torch.Tensor) or mel.dim() != 3:
        raise ValueError("mel_cepstra: expected mel [B, T, M], got %s" % (tuple(mel.shape) if isinstance(
            mel, torch.Tensor) else type(mel).__name__,))
    B, T, M = mel.shape
    n_coef = int(n_coef)
    _geometry(1 <= B <= 65535 and T >= 1 and 1 <= n_coef < M <= MAX_M,
              "the cepstra take 1 <= n_coef < M <= %d over at least one frame, got B=%d T=%d M=%d n_coef=%d"
              % (MAX_M, B, T, M, n_coef))
    if lengths is not None and isinstance(lengths, torch.Tensor) and tuple(lengths.shape) != (B,):
        raise ValueError("mel_cepstra: lengths must have shape [%d], got %s" % (B, tuple(lengths.shape)))
    mel = _dev(mel, "mel", torch.float32)
    lengths = _lengths(lengths, B, T, mel.device, "lengths")
    out = torch.empty(B, T, n_coef, device=mel.device, dtype=torch.float32)
    check(_lib.lib().mg_mel_cepstra(fptr(mel), iptr(lengths, torch.int32), B, T, M, n_coef, fptr(out), stream_ptr()))
    return out


def dtw(a, b, a_lens=None, b_lens=None, return_path=False):
    """a [B, Ta, D], b [B, Tb, D] on the device, a_lens / b_lens int [B] (None: the padded length) ->
    (total float32 [B], path_len int32 [B][, path int32 [B, Ta + Tb - 1, 2]]) on the device.  The local cost is the
    Euclidean distance of two frames; ties go to the diagonal, then to (i-1, j), then to (i, j-1).  The path lists its
    (i, j) cells in ascending order, -1 past path_len.  A pair with a zero length gives total 0 and path_len 0."""
    for t, what in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError("dtw: expected %s [B, T, D], got %s" % (what, tuple(t.shape) if isinstance(
                t, torch.Tensor) else type(t).__name__))
    if a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
        raise ValueError("dtw: a %s and b %s differ in batch or feature size" % (tuple(a.shape), tuple(b.shape)))
    B, Ta, D = a.shape
    Tb = b.shape[1]
    _dtw_geometry(B, Ta, Tb, D)
    for lens, what in ((a_lens, "a_lens"), (b_lens, "b_lens")):
        if isinstance(lens, torch.Tensor) and tuple(lens.shape) != (B,):
            raise ValueError("dtw: %s must have shape [%d], got %s" % (what, B, tuple(lens.shape)))
    a, b = _dev(a, "a", torch.float32), _dev(b, "b", torch.float32)
    dev = a.device
    a_lens, b_lens = _lengths(a_lens, B, Ta, dev, "a_lens"), _lengths(b_lens, B, Tb, dev, "b_lens")
    L = _lib.lib()
    need = L.mg_dtw_workspace_bytes(B, Ta, Tb)
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    total = torch.empty(B, device=dev, dtype=torch.float32)
    path_len = torch.empty(B, device=dev, dtype=torch.int32)
    path = torch.empty(B, Ta + Tb - 1, 2, device=dev, dtype=torch.int32) if return_path else None
    check(L.mg_dtw(fptr(a), fptr(b), iptr(a_lens, torch.int32), iptr(b_lens, torch.int32), B, Ta, Tb, D, fptr(total),
                   iptr(path_len, torch.int32), iptr(path, torch.int32, allow_none=True), iptr(ws, torch.uint8), need,
                   stream_ptr()))
    return (total, path_len, path) if return_path else (total, path_len)


# ---------------------------------------------------------------------------------------------
# The figures
# ---------------------------------------------------------------------------------------------
def mel_cepstral_distortion(mel_ref, mel_syn, ref_lens=None, syn_lens=None, n_coef=13, align="dtw", return_path=False):
    """MCD in dB per utterance, [B] float32: (10 / ln 10) sqrt(2) total / path_len, the mean over the DTW path of the
    Euclidean distance between the two frames' cepstra 1..n_coef.  align="none" is the teacher-forced case: both sides
    have the same lengths and the distance is averaged frame by frame, with no warp.  An empty utterance gives NaN.
    return_path=True: (mcd, path, path_len); without a warp the path is the diagonal."""
    if align not in ("dtw", "none"):
        raise ValueError("mel_cepstral_distortion: align is 'dtw' or 'none', got %r" % (align,))
    if align == "none" and isinstance(mel_ref, torch.Tensor) and isinstance(mel_syn, torch.Tensor) \
            and mel_ref.shape != mel_syn.shape:
        raise ValueError("mel_cepstral_distortion: align='none' takes two mels of one shape, got %s and %s"
                         % (tuple(mel_ref.shape), tuple(mel_syn.shape)))
    if align == "dtw" and isinstance(mel_ref, torch.Tensor) and isinstance(mel_syn, torch.Tensor) \
            and mel_ref.dim() == mel_syn.dim() == 3:
        _dtw_geometry(mel_ref.shape[0], mel_ref.shape[1], mel_syn.shape[1], int(n_coef))      # before any launch
    c_ref = mel_cepstra(mel_ref, ref_lens, n_coef)
    if align == "dtw":
        c_syn = mel_cepstra(mel_syn, syn_lens, n_coef)
        res = dtw(c_ref, c_syn, ref_lens, syn_lens, return_path=return_path)
        total, path_len, path = res if return_path else res + (None,)
        mcd = MCD_SCALE * total / path_len.to(torch.float32)
        return (mcd, path, path_len) if return_path else mcd
    B, T = c_ref.shape[:2]
    lens = _lengths(ref_lens, B, T, c_ref.device, "ref_lens")
    if syn_lens is not None and not torch.equal(_lengths(syn_lens, B, T, c_ref.device, "syn_lens"), lens):
        raise ValueError("mel_cepstral_distortion: align='none' takes equal lengths on both sides")
    c_syn = mel_cepstra(mel_syn, lens, n_coef)
    n = lens.clamp(0, T)
    # both cepstra are zero past a row's length, so the padded frames add nothing
    mcd = MCD_SCALE * (c_ref - c_syn).square().sum(-1).sqrt().sum(-1) / n.to(torch.float32)
    if not return_path:
        return mcd
    steps = torch.arange(T, device=c_ref.device, dtype=torch.int32)
    path = torch.where(steps[None, :, None] < n[:, None, None], steps[None, :, None].expand(B, T, 2),
                       torch.full((), -1, device=c_ref.device, dtype=torch.int32))
    return mcd, path.contiguous(), n


def f0_metrics(f0_ref, f0_syn, path, path_len):
    """F0 figures along a path.  f0_ref [B, Tr], f0_syn [B, Ts] in Hz with 0 for unvoiced (`pitch.extract_f0`), path
    int [B, P, 2] of (ref frame, syn frame) cells, path_len int [B].  A path index at or past a track's last frame is
    clipped to it (`extract_f0` yields len // hop + 1 frames, which can be one more or fewer than the mel has).
    Returns {"f0_rmse_cents": the RMS of 1200 log2(f_syn / f_ref) over the path cells where both are voiced, NaN when
    there are none; "vuv_error": the share of path cells whose voicing differs}, float64 [B] on the path's device."""
    dev = path.device
    f0_ref = torch.as_tensor(np.asarray(f0_ref) if not isinstance(f0_ref, torch.Tensor) else f0_ref).to(dev, torch.float64)
    f0_syn = torch.as_tensor(np.asarray(f0_syn) if not isinstance(f0_syn, torch.Tensor) else f0_syn).to(dev, torch.float64)
    if f0_ref.dim() != 2 or f0_syn.dim() != 2 or path.dim() != 3 or path.shape[2] != 2 \
            or not (f0_ref.shape[0] == f0_syn.shape[0] == path.shape[0] == path_len.shape[0]):
        raise ValueError("f0_metrics: expected f0_ref [B, Tr], f0_syn [B, Ts], path [B, P, 2] and path_len [B], got %s, "
                         "%s, %s and %s" % (tuple(f0_ref.shape), tuple(f0_syn.shape), tuple(path.shape),
                                            tuple(path_len.shape)))
    if f0_ref.shape[1] < 1 or f0_syn.shape[1] < 1:
        raise ValueError("f0_metrics: an F0 track without frames")
    P = path.shape[1]
    on_path = torch.arange(P, device=dev)[None, :] < path_len.to(dev)[:, None]
    fr = torch.gather(f0_ref, 1, path[..., 0].long().clamp(0, f0_ref.shape[1] - 1))
    fs = torch.gather(f0_syn, 1, path[..., 1].long().clamp(0, f0_syn.shape[1] - 1))
    vr, vs = fr > 0, fs > 0
    both = on_path & vr & vs
    cents = 1200.0 * torch.log2(torch.where(both, fs, torch.ones_like(fs)) / torch.where(both, fr, torch.ones_like(fr)))
    rmse = torch.sqrt((cents.square() * both).sum(1) / both.sum(1))      # 0 / 0 = NaN: no cell voiced on both sides
    vuv = (on_path & (vr != vs)).sum(1).to(torch.float64) / path_len.to(dev, torch.float64)
    return {"f0_rmse_cents": rmse, "vuv_error": vuv}


def synthesis_report(pred_mels, pred_lens, target_mels, target_lens, pred_f0=None, target_f0=None, n_coef=13):
    """A batch of synthesized mels [B, Tp, M] against the recordings' [B, Tt, M] (the DTW's first side), lengths int
    [B].  Returns a dict of per-utterance device tensors -- "mcd" [B] dB, "dtw_total" [B], "path_len" [B], "path"
    [B, Tt + Tp - 1, 2] of (target frame, predicted frame) -- and their batch means "mcd_mean" and "path_len_mean"
    (0-dim; NaN entries, empty utterances, are left out of the mean).  With both F0 tracks [B, frames] also
    "f0_rmse_cents", "vuv_error" [B] and "f0_rmse_cents_mean", "vuv_error_mean"."""
    if (pred_f0 is None) != (target_f0 is None):
        raise ValueError("synthesis_report: the F0 figures need both pred_f0 and target_f0")
    if isinstance(target_mels, torch.Tensor) and isinstance(pred_mels, torch.Tensor) \
            and target_mels.dim() == pred_mels.dim() == 3:
        _dtw_geometry(target_mels.shape[0], target_mels.shape[1], pred_mels.shape[1], int(n_coef))      # before any launch
    c_target, c_pred = mel_cepstra(target_mels, target_lens, n_coef), mel_cepstra(pred_mels, pred_lens, n_coef)
    total, path_len, path = dtw(c_target, c_pred, target_lens, pred_lens, return_path=True)
    mcd = MCD_SCALE * total / path_len.to(torch.float32)
    out = {"mcd": mcd, "dtw_total": total, "path_len": path_len, "path": path, "mcd_mean": torch.nanmean(mcd),
           "path_len_mean": path_len.to(torch.float32).mean()}
    if pred_f0 is not None:
        f0 = f0_metrics(target_f0, pred_f0, path, path_len)
        out.update(f0)
        out["f0_rmse_cents_mean"] = torch.nanmean(f0["f0_rmse_cents"])
        out["vuv_error_mean"] = torch.nanmean(f0["vuv_error"])
    return out


def evaluate_model(model, batch, **controls):
    """Free-running synthesis of a 17-slot device batch (`data.to_device`), the call synthesize.py:114-120 makes -- eval
    mode, no_grad, no mel, duration, pitch or energy targets; `controls` are p_control / e_control / d_control -- and
    the `synthesis_report` of its mel against the batch's mel targets.  The model's own forward synchronises once for
    the predicted frame count; nothing here adds to that.  The model's training flag is restored."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            output = model(*batch[2:9], spker_embeds=batch[9], **controls)[0]
    finally:
        model.train(was_training)
    return synthesis_report(output[0], output[11], batch[11], batch[12])
