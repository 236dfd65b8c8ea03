#!/usr/bin/env python3
"""Generate tests/golden/audio.npz and tests/golden/audio_manifest.json by running the REAL reference audio package
(audio/stft.py, audio/audio_processing.py, audio/tools.py) on the CPU.

Run in the build container only:   python tests/golden/make_golden_audio.py
It writes data only: three synthetic 22.05 kHz signals, their STFT magnitude / phase, log-mel and energy (mel_fmax 8000
and None), STFT.forward reconstructions, window_sumsquare, and Griffin-Lim of the inv_mel_spec spectrum from stored,
seeded initial angles after 4 and 60 iterations.

librosa is absent, so before `audio` is imported this installs stubs of librosa.util (pad_center, tiny,
normalize(norm=None)) and librosa.filters.mel; the latter is this file's own numpy restatement of librosa 0.8's
Slaney filterbank.  The reference's STFT.transform calls .cuda() unconditionally; during the calls torch.Tensor.cuda
is the identity.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_harness as H  # noqa: E402

H.install_stubs()
import torch  # noqa: E402

torch.set_num_threads(8)

SR, N_FFT, HOP, WIN, N_MELS, FMIN = 22050, 1024, 256, 1024, 80, 0.0
LENGTHS = (11025, 5000, 600)
GL_ITERS = (4, 60)


def _pad_center(data, size, axis=-1, **kw):
    n = data.shape[axis]
    lpad = int((size - n) // 2)
    lengths = [(0, 0)] * data.ndim
    lengths[axis] = (lpad, int(size - n - lpad))
    return np.pad(data, lengths, **kw)


def _tiny(x):
    x = np.asarray(x)
    dt = x.dtype if np.issubdtype(x.dtype, np.floating) or np.issubdtype(x.dtype, np.complexfloating) else np.float32
    return np.finfo(dt).tiny


def _normalize(S, norm=np.inf, axis=0, threshold=None, fill=None):
    assert norm is None, "stub: only norm=None (what audio_processing.window_sumsquare passes)"
    return S


def _mel(sr, n_fft, n_mels=128, fmin=0.0, fmax=None, htk=False, norm="slaney", dtype=np.float32):
    """librosa 0.8 filters.mel, htk=False, norm='slaney' (restated; librosa is not installed)."""
    assert not htk and norm == "slaney"
    if fmax is None:
        fmax = float(sr) / 2
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def hz_to_mel(f):
        f = float(f)
        return min_log_mel + np.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    def mel_to_hz(m):
        hz = f_sp * m
        big = m >= min_log_mel
        hz[big] = min_log_hz * np.exp(logstep * (m[big] - min_log_mel))
        return hz

    weights = np.zeros((int(n_mels), int(1 + n_fft // 2)), dtype=dtype)
    fftfreqs = np.linspace(0, float(sr) / 2, int(1 + n_fft // 2), endpoint=True)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), int(n_mels) + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(int(n_mels)):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]
    return weights


def install_librosa_stubs():
    lib = sys.modules["librosa"]
    util = types.ModuleType("librosa.util")
    util.pad_center, util.tiny, util.normalize = _pad_center, _tiny, _normalize
    filters = types.ModuleType("librosa.filters")
    filters.mel = _mel
    lib.util, lib.filters = util, filters
    sys.modules["librosa.util"], sys.modules["librosa.filters"] = util, filters


def signal(n, seed):
    """Chirp (80 Hz -> 4 kHz) with three harmonics and noise, clipped to [-1, 1]."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    f0 = 80.0 + (4000.0 - 80.0) * t / max(t[-1], 1e-9) / 2
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = 0.6 * np.sin(ph) + 0.25 * np.sin(2 * ph + 0.3) + 0.12 * np.sin(3 * ph + 1.1) + 0.05 * np.sin(5 * ph)
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t)) + 0.08 * rng.standard_normal(n)
    x[n // 3:n // 3 + 40] *= 4.0  # a burst that clips
    return np.clip(x, -1, 1).astype(np.float32)


def main():
    install_librosa_stubs()
    from audio.stft import STFT, TacotronSTFT
    from audio.audio_processing import window_sumsquare, griffin_lim

    out, man = {}, {"sr": SR, "filter_length": N_FFT, "hop_length": HOP, "win_length": WIN, "n_mels": N_MELS,
                    "mel_fmin": FMIN, "lengths": list(LENGTHS), "gl_iters": list(GL_ITERS), "signals": {}}
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        stft = STFT(N_FFT, HOP, WIN)
        tac = {"8000": TacotronSTFT(N_FFT, HOP, WIN, N_MELS, SR, FMIN, 8000),
               "none": TacotronSTFT(N_FFT, HOP, WIN, N_MELS, SR, FMIN, None)}
        for key, t in tac.items():
            out["mel_basis_%s" % key] = t.mel_basis.numpy()
        for i, n in enumerate(LENGTHS):
            x = signal(n, 100 + i)
            xt = torch.from_numpy(x).unsqueeze(0)
            out["x%d" % i] = x
            with torch.no_grad():
                mag, phase = stft.transform(xt)
                out["mag%d" % i], out["phase%d" % i] = mag[0].numpy(), phase[0].numpy()
                out["recon%d" % i] = stft.forward(xt)[0, 0].numpy()
                for key, t in tac.items():
                    mel, energy = t.mel_spectrogram(xt)
                    out["mel%d_%s" % (i, key)], out["energy%d_%s" % (i, key)] = mel[0].numpy(), energy[0].numpy()
            man["signals"]["x%d" % i] = {"n": n, "frames": int(mag.shape[-1])}
        T0 = out["mag0"].shape[-1]
        out["wss"] = window_sumsquare("hann", T0, hop_length=HOP, win_length=WIN, n_fft=N_FFT, dtype=np.float32)
        man["wss_frames"] = T0

        # inv_mel_spec's spectrum (audio/tools.py:19-26) of signal 0's log-mel (mel_fmax 8000), then griffin_lim with
        # the angles it draws from np.random.rand under a fixed seed, recorded here
        t = tac["8000"]
        mel = torch.from_numpy(out["mel0_8000"])
        mel_decompress = t.spectral_de_normalize(torch.stack([mel])).transpose(1, 2)
        spec = torch.mm(mel_decompress[0], t.mel_basis).transpose(0, 1).unsqueeze(0) * 1000
        spec = spec[:, :, :-1].contiguous()
        out["gl_spec"] = spec[0].numpy()
        np.random.seed(1234)
        out["gl_angles"] = np.angle(np.exp(2j * np.pi * np.random.rand(*spec.size()))).astype(np.float32)[0]
        for it in GL_ITERS:
            np.random.seed(1234)
            with torch.no_grad():
                y = griffin_lim(spec, stft, it)
            out["gl%d" % it] = y[0].numpy()
            mag, _ = stft.transform(y)
            sc = float(torch.norm(mag - spec) / torch.norm(spec))
            man["gl%d_spectral_convergence" % it] = sc
    finally:
        torch.Tensor.cuda = cuda

    np.savez_compressed(os.path.join(HERE, "audio.npz"), **out)
    with open(os.path.join(HERE, "audio_manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    print("audio.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "audio.npz"))))


if __name__ == "__main__":
    main()
