"""Audio front end (reference audio/stft.py, audio/audio_processing.py, audio/tools.py) on HIP: the STFT / inverse
STFT, the log-mel + energy extractor that writes the training targets, and Griffin-Lim, the weight-free inversion.

Same names, argument order and return shapes as the reference.  Deviations:
- outputs stay on the input's device (the reference moves the STFT input to the GPU and its result back to the CPU);
- there is no CPU path: a CPU tensor raises MixganHipError;
- `mel_spectrogram(y, lengths)` takes per-item lengths, so a ragged batch is one launch, each item bit-identical to a
  call on it alone;
- `griffin_lim(..., angles=None)` draws its initial phases on the device, and takes given `angles` as they are;
- `inv_mel_spec` uses `_stft.stft_fn`: the reference names `_stft._stft_fn`, which does not exist, so the reference
  function always raises.

Kernels (csrc/audio.hip): one wave transforms two frames with one 1024-point complex FFT in LDS, with the magnitude /
phase, log-mel / energy or phase-only (Griffin-Lim) epilogue; the inverse overlap-adds in ascending frame order and
divides by the window sum-square computed in-kernel.  Window and mel filterbank are built on the host in float64:
the periodic Hann window as scipy.signal.get_window computes it, centre-padded as librosa.util.pad_center does, and
the filterbank as librosa 0.8's filters.mel (Slaney scale, Slaney area normalisation).  librosa is not available to
this project's tests, so parity with librosa itself is unverified; the restatement is checked against the
reference's outputs through the fixtures of tests/golden/make_golden_audio.py.

`resample` and `peak_normalize_int16` (csrc/resample.hip) are the arithmetic of the reference's prepare_align stage:
what `librosa.load(path, sr)` does to a wav of another rate, and `wav / max(abs(wav)) * max_wav_value` as int16.  The
resampler is a zero-delay polyphase FIR over a ragged batch, equal to scipy.signal.resample_poly with the window of
`resample_filter`, the Kaiser-windowed sinc that librosa's historical `kaiser_best` describes.  Bit parity with
librosa's own resampler (resampy, later soxr) is not claimed and cannot be checked here: its filter is a stored,
interpolated table.  Deviation: the int16 conversion saturates, so the positive peak is 32767; the reference's
32768.0 wraps to -32768 in numpy's cast, a full-scale click at the loudest sample of every file.  An all-zero wav is
written as zeros (the reference divides by zero).
"""
import ctypes
import math

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import fptr, iptr, check, stream_ptr, MixganHipError

N_FFT = 1024
MAX_MELS = 128


class AudioGeometryError(MixganHipError, NotImplementedError):
    """An STFT geometry the kernels do not take."""


def _check_geometry(filter_length, hop_length, win_length, window="hann"):
    ok = (filter_length == N_FFT and isinstance(hop_length, int) and 1 <= hop_length <= N_FFT
          and hop_length & (hop_length - 1) == 0 and isinstance(win_length, int) and 1 <= win_length <= N_FFT
          and window == "hann")
    if not ok:
        raise AudioGeometryError(
            "audio: supported STFT geometry is filter_length == 1024, hop_length a power of two dividing 1024, "
            "1 <= win_length <= 1024 and window 'hann'; got filter_length=%r hop_length=%r win_length=%r window=%r"
            % (filter_length, hop_length, win_length, window))


# ---------------------------------------------------------------------------------------------
# Host tables (float64, then fp32)
# ---------------------------------------------------------------------------------------------
def hann_window(win_length):
    """scipy.signal.get_window('hann', win_length, fftbins=True): the (win_length + 1)-point symmetric
    general_cosine window [0.5, 0.5] over linspace(-pi, pi), truncated to win_length points (one point: [1.0], as
    scipy's length guard returns).  float64."""
    if win_length == 1:
        return np.ones(1)
    M = win_length + 1
    fac = np.linspace(-np.pi, np.pi, M)
    w = np.zeros(M)
    for k, a in enumerate((0.5, 0.5)):
        w += a * np.cos(k * fac)
    return w[:win_length]


def pad_center(data, size):
    """librosa.util.pad_center for a 1-D array."""
    n = len(data)
    lpad = (size - n) // 2
    return np.pad(data, (lpad, size - n - lpad), mode="constant")


def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    if mels.ndim:
        t = f >= min_log_hz
        mels[t] = min_log_mel + np.log(f[t] / min_log_hz) / logstep
    elif f >= min_log_hz:
        mels = min_log_mel + np.log(f / min_log_hz) / logstep
    return mels


def _mel_to_hz(mels):
    mels = np.asanyarray(mels, dtype=np.float64)
    f_sp = 200.0 / 3
    freqs = f_sp * mels
    min_log_hz, min_log_mel, logstep = 1000.0, 1000.0 / f_sp, np.log(6.4) / 27.0
    t = mels >= min_log_mel
    freqs[t] = min_log_hz * np.exp(logstep * (mels[t] - min_log_mel))
    return freqs


def mel_filterbank(sr, n_fft, n_mels=128, fmin=0.0, fmax=None):
    """librosa 0.8 filters.mel(sr, n_fft, n_mels, fmin, fmax) with htk=False, norm='slaney': float32
    [n_mels, 1 + n_fft // 2].  Triangles are evaluated in float64 and stored into the float32 array; the Slaney
    area normalisation 2 / (f[i+2] - f[i]) multiplies that float32 array in float64 and stores float32 again."""
    if fmax is None:
        fmax = float(sr) / 2
    n_mels = int(n_mels)
    weights = np.zeros((n_mels, int(1 + n_fft // 2)), dtype=np.float32)
    fftfreqs = np.linspace(0, float(sr) / 2, int(1 + n_fft // 2), endpoint=True)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]
    return weights


def mel_bands(mel_basis):
    """Per-row nonzero bands of a [n_mels, n_bins] filterbank: (band int32 [3 n_mels] = first bins, bin counts,
    offsets; weights float32).  Interior zeros stay in a band; the skipped entries are exact zeros."""
    mel_basis = np.asarray(mel_basis, dtype=np.float32)
    n = mel_basis.shape[0]
    start, length, offset, w = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), []
    pos = 0
    for m in range(n):
        nz = np.nonzero(mel_basis[m])[0]
        if len(nz):
            start[m], length[m] = nz[0], nz[-1] - nz[0] + 1
            w.append(mel_basis[m, nz[0]:nz[-1] + 1])
        offset[m] = pos
        pos += int(length[m])
    w = np.concatenate(w) if w else np.zeros(1, np.float32)
    return np.concatenate([start, length, offset]).astype(np.int32), w.astype(np.float32)


def _cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise MixganHipError("audio: %s must be a CUDA tensor: the HIP path has no CPU fallback" % what)
    return t


def dynamic_range_compression(x, C=1, clip_val=1e-5):
    """log(clamp(x, clip_val) * C), on the device."""
    return torch.log(torch.clamp(_cuda(x, "x"), min=clip_val) * C)


def dynamic_range_decompression(x, C=1):
    """exp(x) / C, on the device."""
    return torch.exp(_cuda(x, "x")) / C


def window_sumsquare(window, n_frames, hop_length, win_length, n_fft, dtype=np.float32, norm=None):
    """Sum-square envelope of the window over n_frames frames (numpy, as the reference's librosa 0.6 copy):
    shape [n_fft + hop_length * (n_frames - 1)].  Only window 'hann' and norm None are taken."""
    if window != "hann" or norm is not None:
        raise AudioGeometryError("window_sumsquare: only window='hann' with norm=None is supported")
    if win_length is None:
        win_length = n_fft
    n = n_fft + hop_length * (n_frames - 1)
    x = np.zeros(n, dtype=dtype)
    win_sq = pad_center(hann_window(win_length) ** 2, n_fft)
    for i in range(n_frames):
        sample = i * hop_length
        x[sample:min(n, sample + n_fft)] += win_sq[:max(0, min(n_fft, n - sample))]
    return x


class _Tables:
    """Device copies of the fp32 window, the float64 squared window and the fp32 twiddles, one set per device."""

    def __init__(self, win_length):
        w64 = pad_center(hann_window(win_length), N_FFT)
        self.window = torch.from_numpy(w64.astype(np.float32))
        self.wsq = torch.from_numpy(pad_center(hann_window(win_length) ** 2, N_FFT))
        tw = np.exp(-2j * np.pi * np.arange(N_FFT) / N_FFT)
        self.twiddle = torch.from_numpy(np.stack([tw.real, tw.imag], 1).astype(np.float32).reshape(-1))
        self._dev = {}

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device) for t in (self.window, self.wsq, self.twiddle))
        return self._dev[key]


def _istft_tile(B, Lout):
    """Output samples per workgroup: the largest of 1024 / 512 / 256 that still gives ~4 waves per CU."""
    for tile in (1024, 512, 256):
        if B * -(-Lout // tile) >= 1024:
            return tile
    return 256


# ---------------------------------------------------------------------------------------------
# Modules
# ---------------------------------------------------------------------------------------------
class STFT(nn.Module):
    """audio/stft.py STFT: the reflect-padded 1024-point STFT and its inverse."""

    def __init__(self, filter_length, hop_length, win_length, window="hann"):
        super().__init__()
        _check_geometry(filter_length, hop_length, win_length, window)
        self.filter_length = filter_length
        self.hop_length = hop_length
        self.win_length = win_length
        self.window = window
        self.forward_transform = None
        self._tables = _Tables(win_length)

    def n_frames(self, num_samples):
        return 1 + num_samples // self.hop_length

    def _signal(self, x):
        _cuda(x, "input_data")
        if x.dim() != 2:
            raise ValueError("STFT: expected a [B, N] signal, got %s" % (tuple(x.shape),))
        if x.shape[1] <= self.filter_length // 2:
            raise ValueError("STFT: a signal of %d samples is too short for the reflect pad of %d (needs > %d)"
                             % (x.shape[1], self.filter_length // 2, self.filter_length // 2))
        return x.contiguous()

    def _spectrum_fwd(self, x, mag, phase, strides, T, lengths=None):
        win, _, tw = self._tables.on(x.device)
        B, L = x.shape
        check(_lib.lib().mg_stft_fwd(fptr(x), L, iptr(lengths, torch.int32, allow_none=True), B, L, self.hop_length,
                                     fptr(win), fptr(tw), fptr(mag, allow_none=True), fptr(phase), *strides, T,
                                     stream_ptr()))

    def _spectrum_inv(self, mag, phase, strides, B, T, out):
        win, wsq, tw = self._tables.on(mag.device)
        if not (wsq.is_cuda and wsq.dtype == torch.float64):
            raise MixganHipError("audio: window table is not a device float64 tensor")
        Lout = (T - 1) * self.hop_length
        check(_lib.lib().mg_istft(fptr(mag), fptr(phase), *strides, B, T, self.hop_length, fptr(win),
                                  ctypes.c_void_p(wsq.data_ptr()), fptr(tw), fptr(out), _istft_tile(B, Lout), stream_ptr()))

    def transform(self, input_data):
        """[B, N] -> (magnitude, phase), each [B, filter_length / 2 + 1, 1 + N // hop]."""
        x = self._signal(input_data)
        B, L = x.shape
        self.num_samples = L
        T = self.n_frames(L)
        nb = self.filter_length // 2 + 1
        mag = torch.empty(B, nb, T, device=x.device, dtype=torch.float32)
        phase = torch.empty_like(mag)
        self._spectrum_fwd(x, mag, phase, (nb * T, T, 1), T)
        return mag, phase

    def inverse(self, magnitude, phase):
        """(magnitude, phase) [B, n_fft / 2 + 1, T] -> [B, 1, (T - 1) hop]."""
        _cuda(magnitude, "magnitude")
        _cuda(phase, "phase")
        nb = self.filter_length // 2 + 1
        if magnitude.dim() != 3 or magnitude.shape[1] != nb or phase.shape != magnitude.shape:
            raise ValueError("STFT.inverse: expected magnitude and phase [B, %d, T] of one shape, got %s and %s"
                             % (nb, tuple(magnitude.shape), tuple(phase.shape)))
        B, _, T = magnitude.shape
        if T < 2:
            raise ValueError("STFT.inverse: needs at least 2 frames, got %d" % T)
        magnitude, phase = magnitude.contiguous(), phase.contiguous()
        out = torch.empty(B, 1, (T - 1) * self.hop_length, device=magnitude.device, dtype=torch.float32)
        self._spectrum_inv(magnitude, phase, (nb * T, T, 1), B, T, out)
        return out

    def forward(self, input_data):
        self.magnitude, self.phase = self.transform(input_data)
        return self.inverse(self.magnitude, self.phase)


class TacotronSTFT(nn.Module):
    """audio/stft.py TacotronSTFT: log-mel spectrogram and energy.  mel_fmax=None means sampling_rate / 2."""

    def __init__(self, filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax):
        super().__init__()
        if not (isinstance(n_mel_channels, int) and 1 <= n_mel_channels <= MAX_MELS):
            raise AudioGeometryError("TacotronSTFT: n_mel_channels must be in [1, %d], got %r"
                                     % (MAX_MELS, n_mel_channels))
        self.n_mel_channels = n_mel_channels
        self.sampling_rate = sampling_rate
        self.stft_fn = STFT(filter_length, hop_length, win_length)
        basis = mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)
        self.register_buffer("mel_basis", torch.from_numpy(basis).float())
        band, band_w = mel_bands(basis)
        self._band, self._band_w = torch.from_numpy(band), torch.from_numpy(band_w)
        self._band_dev = {}

    def spectral_normalize(self, magnitudes):
        return dynamic_range_compression(magnitudes)

    def spectral_de_normalize(self, magnitudes):
        return dynamic_range_decompression(magnitudes)

    def _bands(self, device):
        key = str(device)
        if key not in self._band_dev:
            self._band_dev[key] = (self._band.to(device), self._band_w.to(device))
        return self._band_dev[key]

    def mel_spectrogram(self, y, lengths=None):
        """y [B, N] in [-1, 1] -> (log-mel [B, n_mels, T], energy [B, T]), T = 1 + N // hop.

        lengths (int [B], optional): item b is reflect-padded at its own end and has 1 + lengths[b] // hop frames;
        T is then that count for the longest item, and later frames are 0.  Each item equals a call on
        y[b:b+1, :lengths[b]] alone, bit for bit."""
        x = self.stft_fn._signal(y)
        # the reference's range check: one device reduction, one host read
        assert float(x.abs().amax()) <= 1, "mel_spectrogram: input outside [-1, 1]"
        B, L = x.shape
        hop = self.stft_fn.hop_length
        len_dev = None
        if lengths is not None:
            lens = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths).astype(np.int64)
            if lens.shape != (B,):
                raise ValueError("mel_spectrogram: lengths must have shape [%d], got %s" % (B, lens.shape))
            if (lens <= N_FFT // 2).any() or (lens > L).any():
                raise ValueError("mel_spectrogram: every length must be in (%d, %d], got %s"
                                 % (N_FFT // 2, L, lens.tolist()))
            T = 1 + int(lens.max()) // hop
            len_dev = torch.from_numpy(lens.astype(np.int32)).to(x.device)
        else:
            T = 1 + L // hop
        mel = torch.empty(B, self.n_mel_channels, T, device=x.device, dtype=torch.float32)
        energy = torch.empty(B, T, device=x.device, dtype=torch.float32)
        win, _, tw = self.stft_fn._tables.on(x.device)
        band, band_w = self._bands(x.device)
        check(_lib.lib().mg_stft_mel(fptr(x), L, iptr(len_dev, torch.int32, allow_none=True), B, L, hop, fptr(win),
                                     fptr(tw), iptr(band, torch.int32), fptr(band_w), self.n_mel_channels,
                                     fptr(mel), fptr(energy), T, stream_ptr()))
        return mel, energy

    def mel_spectrogram_diff(self, y):
        """y [B, N] -> log-mel [B, n_mels, 1 + N // hop] with autograd to y (mg_stft_mel / mg_stft_mel_bwd): HiFi-GAN's
        mel-reconstruction term.  The value is mel_spectrogram's, bit for bit.  No `lengths`, no energy, and no range
        check of y (a generator's tanh output is inside [-1, 1]; the check is a host read), so nothing here syncs."""
        from .autograd import mel_diff
        return mel_diff(self.stft_fn._signal(y), self)

    def _mel_args(self, x):
        """(hop, window, twiddle, band, band_w) on x's device, as the two mel kernels take them."""
        win, _, tw = self.stft_fn._tables.on(x.device)
        band, band_w = self._bands(x.device)
        return self.stft_fn.hop_length, win, tw, band, band_w


# ---------------------------------------------------------------------------------------------
# Griffin-Lim and the tools
# ---------------------------------------------------------------------------------------------
def griffin_lim(magnitudes, stft_fn, n_iters=30, angles=None):
    """magnitudes [B, n_fft / 2 + 1, T] -> signal [B, (T - 1) hop] after n_iters Griffin-Lim iterations.

    angles: initial phases [B, n_fft / 2 + 1, T], used as given; None draws them uniformly on the device.  The loop
    is two launches per iteration (phase-only STFT, inverse STFT) on preallocated frame-major buffers, with no host
    synchronisation, so a call can be captured in a graph."""
    _cuda(magnitudes, "magnitudes")
    nb = stft_fn.filter_length // 2 + 1
    if magnitudes.dim() != 3 or magnitudes.shape[1] != nb:
        raise ValueError("griffin_lim: expected magnitudes [B, %d, T], got %s" % (nb, tuple(magnitudes.shape)))
    B, _, T = magnitudes.shape
    Lsig = (T - 1) * stft_fn.hop_length
    if T < 2 or Lsig <= N_FFT // 2:
        raise ValueError("griffin_lim: %d frames give a %d-sample signal, too short for the reflect pad (needs > %d)"
                         % (T, Lsig, N_FFT // 2))
    if angles is None:
        angles = torch.rand(magnitudes.shape, device=magnitudes.device) * (2 * math.pi) - math.pi
    _cuda(angles, "angles")
    if angles.shape != magnitudes.shape:
        raise ValueError("griffin_lim: angles %s do not match magnitudes %s"
                         % (tuple(angles.shape), tuple(magnitudes.shape)))
    # frame-major [B, T, bins]: both kernels then read and write whole frames contiguously
    mags = magnitudes.float().transpose(1, 2).contiguous()
    phase = angles.float().transpose(1, 2).contiguous()
    signal = torch.empty(B, Lsig, device=magnitudes.device, dtype=torch.float32)
    strides = (T * nb, 1, nb)
    stft_fn._spectrum_inv(mags, phase, strides, B, T, signal)
    for _ in range(n_iters):
        stft_fn._spectrum_fwd(signal, None, phase, strides, T)
        stft_fn._spectrum_inv(mags, phase, strides, B, T, signal)
    return signal


def get_mel_from_wav(audio, _stft):
    """One utterance (numpy or tensor, [N]) -> (log-mel [n_mels, T], energy [T]) as float32 numpy.  The signal goes
    to the device of `_stft`'s mel_basis, which must be a GPU."""
    dev = _stft.mel_basis.device
    if dev.type != "cuda":
        raise MixganHipError("get_mel_from_wav: move the TacotronSTFT to the GPU first (no CPU fallback)")
    audio = torch.clip(torch.as_tensor(np.asarray(audio), dtype=torch.float32).unsqueeze(0).to(dev), -1, 1)
    melspec, energy = _stft.mel_spectrogram(audio)
    melspec = torch.squeeze(melspec, 0).cpu().numpy().astype(np.float32)
    energy = torch.squeeze(energy, 0).cpu().numpy().astype(np.float32)
    return melspec, energy


def mel_to_audio(mels, _stft, griffin_iters=60, angles=None):
    """Batched inv_mel_spec on the device: mels [B, n_mels, T] (log) -> signal [B, (T - 2) hop].  exp, the
    mel_basis^T projection times 1000, the drop of the last frame, then Griffin-Lim; angles [B, bins, T - 1]."""
    _cuda(mels, "mels")
    if mels.dim() != 3 or mels.shape[1] != _stft.n_mel_channels:
        raise ValueError("mel_to_audio: expected mels [B, %d, T], got %s"
                         % (_stft.n_mel_channels, tuple(mels.shape)))
    basis = _stft.mel_basis.to(mels.device)
    spec = torch.matmul(basis.t(), _stft.spectral_de_normalize(mels.float())) * 1000
    return griffin_lim(spec[:, :, :-1].contiguous(), _stft.stft_fn, griffin_iters, angles)


def inv_mel_spec(mel, out_filename, _stft, griffin_iters=60):
    """mel [n_mels, T] -> a float32 wav at _stft.sampling_rate, written with scipy.io.wavfile.write."""
    from scipy.io.wavfile import write
    audio = mel_to_audio(mel.unsqueeze(0), _stft, griffin_iters)
    audio = audio.squeeze().cpu().numpy()
    write(out_filename, _stft.sampling_rate, audio)


# ---------------------------------------------------------------------------------------------
# Resampling and peak normalisation (the arithmetic of prepare_align)
# ---------------------------------------------------------------------------------------------
RESAMPLE_TILE = _lib.MG_RESAMPLE_TILE      # consecutive outputs of one workgroup


def resample_ratio(orig_sr, target_sr):
    """(up, down): target_sr / orig_sr in lowest terms."""
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    if orig_sr <= 0 or target_sr <= 0:
        raise ValueError("resample: sampling rates must be positive, got %r -> %r" % (orig_sr, target_sr))
    g = math.gcd(orig_sr, target_sr)
    return target_sr // g, orig_sr // g


def resample_filter(up, down, num_zeros=64, beta=14.769656459379492, rolloff=0.9475937167399596):
    """Low-pass of the up/down resampler, float64 [2 half + 1]: with m = max(up, down), fc = rolloff / m,
    half = num_zeros m and n = -half .. half, h = fc sinc(fc n) kaiser(2 half + 1, beta), scaled to h.sum() == 1.
    The defaults are the parameters of librosa's historical `kaiser_best` (64 zero crossings, its beta and roll-off);
    librosa evaluates a stored table of that window by interpolation, so the taps are not claimed equal to its."""
    m = max(int(up), int(down))
    half = int(num_zeros) * m
    n = np.arange(-half, half + 1, dtype=np.float64)
    fc = float(rolloff) / m
    h = fc * np.sinc(fc * n) * np.kaiser(2 * half + 1, float(beta))
    return h / h.sum()


def polyphase_table(h, up):
    """The tap table mg_resample_poly takes (mixgan_hip.h), float64 [up, Kp]: row r, column j holds
    up h[(Mh - 1 - j) up + r + half] with Mh = half // up + 1, 0 where that index leaves h; Kp = 2 Mh rounded up to a
    multiple of 4."""
    h = np.asarray(h, dtype=np.float64)
    if h.ndim != 1 or len(h) % 2 != 1:
        raise ValueError("polyphase_table: the filter must have odd length, got shape %s" % (h.shape,))
    half = (len(h) - 1) // 2
    Mh = half // up + 1
    Kp = -(-2 * Mh // 4) * 4
    idx = (Mh - 1 - np.arange(Kp))[None, :] * up + np.arange(up)[:, None] + half
    ok = (idx >= 0) & (idx <= 2 * half)
    return np.where(ok, up * h[np.clip(idx, 0, 2 * half)], 0.0)


_RESAMPLE_TABLES = {}


def _resample_table(up, down, device, num_zeros=64, beta=14.769656459379492, rolloff=0.9475937167399596):
    key = (up, down, int(num_zeros), float(beta), float(rolloff), str(device))
    if key not in _RESAMPLE_TABLES:
        h = resample_filter(up, down, num_zeros, beta, rolloff)
        table = polyphase_table(h, up)
        span = (RESAMPLE_TILE - 1) * down // up + table.shape[1] + 2
        if up > _lib.MG_RESAMPLE_MAX_UP or table.shape[1] > _lib.MG_RESAMPLE_MAX_TAPS or span > _lib.MG_RESAMPLE_MAX_SPAN:
            raise AudioGeometryError(
                "resample: ratio %d:%d with %d taps per output is outside the kernel's limits (up <= %d, taps <= %d, "
                "staged span %d <= %d)" % (up, down, table.shape[1], _lib.MG_RESAMPLE_MAX_UP,
                                           _lib.MG_RESAMPLE_MAX_TAPS, span, _lib.MG_RESAMPLE_MAX_SPAN))
        _RESAMPLE_TABLES[key] = (torch.from_numpy(table.astype(np.float32)).to(device), (len(h) - 1) // 2)
    return _RESAMPLE_TABLES[key]


def _ragged(wav, lengths, what):
    """wav [N] or [B, N] on the GPU -> (x [B, N] contiguous fp32, host lengths int64 [B], device int32 [B] or None,
    whether the input was 1-D)."""
    _cuda(wav, "wav")
    if wav.dim() not in (1, 2) or wav.shape[-1] == 0:
        raise ValueError("%s: expected a non-empty [N] or [B, N] signal, got %s" % (what, tuple(wav.shape)))
    x = (wav if wav.dim() == 2 else wav.unsqueeze(0)).float().contiguous()
    B, N = x.shape
    if lengths is None:
        return x, np.full(B, N, dtype=np.int64), None, wav.dim() == 1
    lens = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths).astype(np.int64).reshape(-1)
    if lens.shape != (B,) or (lens < 0).any() or (lens > N).any():
        raise ValueError("%s: lengths must be %d values in [0, %d], got %s" % (what, B, N, lens.tolist()))
    return x, lens, torch.from_numpy(lens.astype(np.int32)).to(x.device), wav.dim() == 1


def resample(wav, orig_sr, target_sr, lengths=None, **filter_params):
    """wav [N] or [B, N] at orig_sr -> (out [M] or [B, M], out_lengths) at target_sr, on the device.

    lengths (B ints, optional) makes the batch ragged: item b is its first lengths[b] samples, nothing beyond them is
    read, and it equals a call on it alone.  out_lengths is a device int32 [B] (B = 1 for a 1-D wav) holding
    ceil(lengths up / down) for the reduced ratio up / down; M is its maximum and out is 0 beyond each length.
    filter_params go to `resample_filter`; tables are built in float64 once per (ratio, parameters, device).
    Equal rates copy."""
    x, lens, len_dev, squeeze = _ragged(wav, lengths, "resample")
    up, down = resample_ratio(orig_sr, target_sr)
    B, N = x.shape
    out_lens = -(-lens * up // down)
    M = max(1, int(out_lens.max()))
    if N >= 2 ** 31 or M >= 2 ** 31:
        raise AudioGeometryError("resample: rows of 2^31 samples or more are not supported")
    out = torch.empty(B, M, device=x.device, dtype=torch.float32)
    if up == down:
        taps, half, Kp = None, 0, 0
    else:
        taps, half = _resample_table(up, down, x.device, **filter_params)
        Kp = taps.shape[1]
    check(_lib.lib().mg_resample_poly(fptr(x), N, iptr(len_dev, torch.int32, allow_none=True), B, N,
                                      fptr(taps, allow_none=True), up, down, Kp, half, fptr(out), M, M, stream_ptr()))
    out_len_dev = torch.from_numpy(out_lens.astype(np.int32)).to(x.device)
    return (out[0] if squeeze else out), out_len_dev


def peak_normalize_int16(wav, lengths=None, max_wav_value=32768.0):
    """wav [N] or [B, N] -> int16 of the same shape: trunc(wav / max|wav| * max_wav_value) per item in float32,
    saturated to [-32768, 32767]; the maximum is over the first lengths[b] samples, the rest is written as 0, and an
    all-zero item stays zero."""
    x, _, len_dev, squeeze = _ragged(wav, lengths, "peak_normalize_int16")
    B, N = x.shape
    out = torch.empty(B, N, device=x.device, dtype=torch.int16)
    check(_lib.lib().mg_peak_normalize_i16(fptr(x), N, iptr(len_dev, torch.int32, allow_none=True), B, N,
                                           float(max_wav_value), ctypes.c_void_p(out.data_ptr()), N, stream_ptr()))
    return out[0] if squeeze else out
