"""Native pitch extractor (csrc/pitch.hip): F0 tracks for the corpus builder without pyworld.

The reference calls pyworld's dio + stonemask once per utterance on the host.  This is an algorithm of its own, not
a port, and no parity with pyworld is claimed: there is no oracle for it here.  What it keeps is the frame contract
the builder consumes: F0 in Hz as float64, 0 for unvoiced, frame k centred on sample k hop, len // hop + 1 frames.

Stage 1 (`yin_candidates`): YIN (de Cheveigne and Kawahara 2002).  Frame k is the N = 1024 samples from k hop - N / 2
on (zero outside the utterance); d(tau) = sum_{j < W} (x_j - x_{j+tau})^2 over W = 512 samples by FFT, its
cumulative-mean-normalised d', and the K = 4 deepest local minima of d' in [tau_min, tau_max] as candidates, each
with a parabola-refined period and the depth d' as its cost; plus the frame's RMS.
Stage 2 (`pitch_track`): a Viterbi pass per utterance over the K slots and one unvoiced state, in float64.
tests/pitch_oracle.py restates both in numpy; DESIGN.md section 4.9 has the method, its limits and the parameters.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import fptr, iptr, check, stream_ptr, MixganHipError
from .audio import _ragged

N, W, K = _lib.MG_PITCH_N, _lib.MG_PITCH_W, _lib.MG_PITCH_K
F0_FLOOR, F0_CEIL = 71.0, 800.0
# every value can be halved or doubled on its own without losing a frame of the synthetic suite
TRACK_PARAMS = dict(theta=0.15, beta=0.05, lam=0.5, switch=0.1, gate_db=-50.0)


class PitchGeometryError(MixganHipError, NotImplementedError):
    """A sampling rate / F0 range the pitch kernels do not take."""


def pitch_geometry(sampling_rate, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    """(tau_min, tau_max) = (floor(sr / f0_ceil), ceil(sr / f0_floor)); the longest lag and the one after it must fit
    beside the integration window in the analysis span."""
    if not (sampling_rate > 0 and f0_floor > 0 and f0_ceil > f0_floor):
        raise PitchGeometryError("pitch: need sampling_rate > 0 and 0 < f0_floor < f0_ceil, got sampling_rate=%r "
                                 "f0_floor=%r f0_ceil=%r" % (sampling_rate, f0_floor, f0_ceil))
    tau_max, tau_min = int(math.ceil(sampling_rate / f0_floor)), int(math.floor(sampling_rate / f0_ceil))
    if tau_max + 1 > N - W or tau_min < 2:
        raise PitchGeometryError(
            "pitch: sampling_rate=%r with f0_floor=%r needs lags up to %d, the %d-sample span with its %d-sample window "
            "holds %d; and f0_ceil=%r needs a shortest lag of %d >= 2.  Lower the rate (resample) or raise f0_floor / "
            "lower f0_ceil" % (sampling_rate, f0_floor, tau_max + 1, N, W, N - W, f0_ceil, tau_min))
    return tau_min, tau_max


def frame_count(num_samples, hop_length):
    return num_samples // hop_length + 1


_TWIDDLE = {}


def _twiddle(device):
    key = str(device)
    if key not in _TWIDDLE:
        tw = np.exp(-2j * np.pi * np.arange(N) / N)
        _TWIDDLE[key] = torch.from_numpy(np.stack([tw.real, tw.imag], 1).astype(np.float32).reshape(-1)).to(device)
    return _TWIDDLE[key]


def _hop(hop_length):
    if not (isinstance(hop_length, (int, np.integer)) and hop_length >= 1):
        raise PitchGeometryError("pitch: hop_length must be a positive integer, got %r" % (hop_length,))
    return int(hop_length)


def yin_candidates(wav, sampling_rate, hop_length, lengths=None, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL):
    """wav [N] or [B, N] on the GPU -> (period [B, T, K], cost [B, T, K], rms [B, T], n_frames int32 [B]), float32 on
    the device.  lengths makes the batch ragged: nothing at or past lengths[b] is read, row b has
    lengths[b] // hop + 1 frames and equals a call on it alone; T is the largest count, later frames are 0."""
    hop = _hop(hop_length)
    tau_min, tau_max = pitch_geometry(sampling_rate, f0_floor, f0_ceil)
    x, lens, len_dev, _ = _ragged(wav, lengths, "yin_candidates")
    B, L = x.shape
    if L >= 2 ** 31 - N:
        raise PitchGeometryError("pitch: rows of 2^31 samples or more are not supported")
    frames = lens // hop + 1
    T = int(frames.max())
    period = torch.empty(B, T, K, device=x.device, dtype=torch.float32)
    cost = torch.empty_like(period)
    rms = torch.empty(B, T, device=x.device, dtype=torch.float32)
    check(_lib.lib().mg_yin_candidates(fptr(x), L, iptr(len_dev, torch.int32, allow_none=True), B, L, hop, tau_min,
                                       tau_max, fptr(_twiddle(x.device)), fptr(period), fptr(cost), fptr(rms), T,
                                       stream_ptr()))
    return period, cost, rms, torch.from_numpy(frames.astype(np.int32)).to(x.device)


def pitch_track(period, cost, rms, n_frames, sampling_rate, f0_floor=F0_FLOOR, **params):
    """Stage-1 output -> f0 float64 [B, T] on the device: sampling_rate / period on voiced frames, 0 elsewhere and past
    n_frames[b].  params: theta, beta, lam, switch, gate_db (TRACK_PARAMS)."""
    unknown = set(params) - set(TRACK_PARAMS)
    if unknown:
        raise TypeError("pitch_track: unknown parameters %s" % sorted(unknown))
    p = dict(TRACK_PARAMS, **params)
    if not (sampling_rate > 0 and f0_floor > 0):
        raise PitchGeometryError("pitch: need sampling_rate > 0 and f0_floor > 0, got %r and %r"
                                 % (sampling_rate, f0_floor))
    tau_max = int(math.ceil(sampling_rate / f0_floor))
    for t, what in ((period, "period"), (cost, "cost"), (rms, "rms"), (n_frames, "n_frames")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise MixganHipError("pitch_track: %s must be a CUDA tensor: the HIP path has no CPU fallback" % what)
    if period.dim() != 3 or period.shape[2] != K or cost.shape != period.shape or rms.shape != period.shape[:2] \
            or n_frames.shape != period.shape[:1]:
        raise ValueError("pitch_track: expected period and cost [B, T, %d], rms [B, T] and n_frames [B], got %s, %s, "
                         "%s and %s" % (K, tuple(period.shape), tuple(cost.shape), tuple(rms.shape),
                                        tuple(n_frames.shape)))
    B, T = rms.shape
    period, cost, rms = period.float().contiguous(), cost.float().contiguous(), rms.float().contiguous()
    n_frames = n_frames.to(torch.int32).contiguous()
    vals = [0.0] * _lib.MG_PITCH_PARAMS
    vals[_lib.MG_PITCH_P_SR], vals[_lib.MG_PITCH_P_TAU_MAX] = float(sampling_rate), float(tau_max)
    vals[_lib.MG_PITCH_P_THETA], vals[_lib.MG_PITCH_P_BETA] = float(p["theta"]), float(p["beta"])
    vals[_lib.MG_PITCH_P_LAMBDA], vals[_lib.MG_PITCH_P_SWITCH] = float(p["lam"]), float(p["switch"])
    vals[_lib.MG_PITCH_P_GATE] = 10.0 ** (float(p["gate_db"]) / 20.0)
    L = _lib.lib()
    need = L.mg_pitch_track_workspace_bytes(B, T)
    ws = torch.empty(need, device=rms.device, dtype=torch.uint8)
    f0 = torch.empty(B, T, device=rms.device, dtype=torch.float64)
    check(L.mg_pitch_track(fptr(period), fptr(cost), fptr(rms), iptr(n_frames, torch.int32),
                           B, T, (ctypes.c_double * len(vals))(*vals), ctypes.c_void_p(f0.data_ptr()),
                           ctypes.c_void_p(ws.data_ptr()), need, stream_ptr()))
    return f0


def extract_f0(wav, sampling_rate, hop_length, lengths=None, f0_floor=F0_FLOOR, f0_ceil=F0_CEIL, **params):
    """wav [N] or [B, N] on the GPU -> (f0 float64 [B, T], n_frames int32 [B]) on the device: one launch of each
    stage for the whole ragged batch."""
    period, cost, rms, n_frames = yin_candidates(wav, sampling_rate, hop_length, lengths, f0_floor, f0_ceil)
    return pitch_track(period, cost, rms, n_frames, sampling_rate, f0_floor, **params), n_frames


def native_pitch(wav, sampling_rate, frame_period_ms, device="cuda"):
    """A `pitch_fn` for Preprocessor: one utterance as a numpy array -> f0 float64 [len // hop + 1] as numpy, with
    hop = round(frame_period_ms sampling_rate / 1000)."""
    hop = int(round(frame_period_ms * sampling_rate / 1000.0))
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(wav), dtype=np.float32)).to(device)
    f0, _ = extract_f0(x, sampling_rate, hop)
    return f0[0].cpu().numpy()
