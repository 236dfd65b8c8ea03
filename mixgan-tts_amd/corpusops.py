"""Tensor-level wrappers of the corpus-builder kernels (csrc/corpus.hip): the beta-binomial alignment prior and the
frame -> phoneme averages of pitch and energy.  CUDA tensors only, like the rest of the package."""
import ctypes

import torch

from . import _lib
from ._lib import check, stream_ptr, MixganHipError

MAX_PHONEMES, MAX_FRAMES = 2048, 4096      # mg_phoneme_average's limits (PA_MAXT, PA_MAXL)


def _int32_vector(t, what, n=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise MixganHipError("%s must be a CUDA tensor: the HIP path has no CPU fallback" % what)
    if t.dim() != 1 or t.dtype not in (torch.int32, torch.int64) or (n is not None and t.shape[0] != n):
        raise MixganHipError("%s must be an int32 / int64 vector%s, got %s %s"
                             % (what, "" if n is None else " of %d" % n, t.dtype, tuple(t.shape)))
    return t.to(torch.int32).contiguous()


def attn_prior(src_lens, mel_lens, T, L, scaling=1.0, dtype=torch.float32):
    """Padded beta-binomial alignment priors [B, T, L] (preprocessor.py:344-348, :384-393, then pad_3D): for
    i < src_lens[b], k < mel_lens[b] the pmf at k of betabinom(mel_len, scaling (i + 1), scaling (src_len - i)),
    0 elsewhere.  Evaluated in float64 on the device and written as `dtype` (float32 or float64).  No host sync."""
    src = _int32_vector(src_lens, "attn_prior: src_lens")
    mel = _int32_vector(mel_lens, "attn_prior: mel_lens", src.shape[0])
    if dtype not in (torch.float32, torch.float64):
        raise MixganHipError("attn_prior: dtype must be torch.float32 or torch.float64, got %s" % dtype)
    B, T, L = src.shape[0], int(T), int(L)
    s = ctypes.c_double(float(scaling))
    out = torch.empty(B, T, L, device=src.device, dtype=dtype)
    check(_lib.lib().mg_betabinom_prior(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(mel.data_ptr()),
                                        ctypes.byref(s), ctypes.c_void_p(out.data_ptr()), B, T, L,
                                        int(dtype == torch.float64), stream_ptr()))
    return out


def phoneme_average(values, durations, n_frames, n_phon, kind):
    """Frame-level `values` [B, L] -> phoneme level [B, T] by the durations [B, T] (preprocessor.py:311-341).

    kind "energy": float32; out[b, i] = mean(values[b, pos : pos + d_i]), 0 for d_i == 0.
    kind "pitch":  float64; zero frames are first filled by linear interpolation over the non-zero ones (the first /
                   last non-zero value outside them), then averaged the same way.  Every utterance needs at least two
                   non-zero frames (the builder filters the others out before this call): checked here, which costs
                   one host read.
    The reference averages in place; where that makes a segment read earlier results, so does this."""
    if kind not in ("pitch", "energy"):
        raise MixganHipError("phoneme_average: kind must be 'pitch' or 'energy', got %r" % (kind,))
    want = torch.float64 if kind == "pitch" else torch.float32
    if not (isinstance(values, torch.Tensor) and values.is_cuda and isinstance(durations, torch.Tensor)
            and durations.is_cuda):
        raise MixganHipError("phoneme_average: values and durations must be CUDA tensors (no CPU fallback)")
    if values.dim() != 2 or values.dtype != want:
        raise MixganHipError("phoneme_average: %s values must be a %s [B, L] tensor, got %s %s"
                             % (kind, want, values.dtype, tuple(values.shape)))
    B, L = values.shape
    if durations.dim() != 2 or durations.shape[0] != B or durations.dtype not in (torch.int32, torch.int64):
        raise MixganHipError("phoneme_average: durations must be an integer [%d, T] tensor, got %s %s"
                             % (B, durations.dtype, tuple(durations.shape)))
    T = durations.shape[1]
    if not (1 <= T <= MAX_PHONEMES and 1 <= L <= MAX_FRAMES):
        raise MixganHipError("phoneme_average: supports T <= %d phonemes and L <= %d frames, got T=%d L=%d"
                             % (MAX_PHONEMES, MAX_FRAMES, T, L))
    nf = _int32_vector(n_frames, "phoneme_average: n_frames", B)
    npn = _int32_vector(n_phon, "phoneme_average: n_phon", B)
    values, dur = values.contiguous(), durations.to(torch.int32).contiguous()
    if kind == "pitch":
        inside = torch.arange(L, device=values.device)[None, :] < nf[:, None]
        voiced = ((values != 0) & inside).sum(1)
        if int(voiced.min()) <= 1:
            raise MixganHipError("phoneme_average: every utterance needs more than one non-zero pitch frame "
                                 "(got %s); filter the others out first" % voiced.tolist())
    out = torch.empty(B, T, device=values.device, dtype=want)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    check(_lib.lib().mg_phoneme_average(p(values), p(dur), p(nf), p(npn), p(out), B, T, L, int(kind == "pitch"),
                                        stream_ptr()))
    return out
