#!/usr/bin/env python3
"""Audio front-end timing (profiles/*_audio_bench.jsonl).

  python tools/audio_bench.py [--iters 20] [--out profiles/r07_a_audio_bench.jsonl] [--only native]

Rows: log-mel + energy from B x 256 000 samples (B = 16, 1), and Griffin-Lim with 60 iterations from a log-mel
[B, 80, 1000] (B = 1, 16; the inv_mel_spec path: exp, mel_basis^T projection x 1000, last frame dropped).  Each row runs
three implementations on the same GPU:
  native   mixgan_tts_amd.audio (csrc/audio.hip)
  conv     the reference's algorithm in stock PyTorch-ROCm eager, fp32: conv1d / conv_transpose1d against the
           [1026, 1, 1024] bases, atan2, window-sum division (the sum itself precomputed once, which the reference
           does on the host each call)
  rocfft   torch.stft / torch.istft (rocFFT) with the same window, centre reflect padding, and for the mel row a
           dense matmul with the filterbank
Device events around each call, two warm-up calls, median of --iters.  Every row also prints the bytes it must move
at the least (inputs read once, outputs written once; Griffin-Lim: per iteration the signal and the phase written and
read once, the magnitudes read once) and the time that takes at the 8.0 TB/s HBM peak, as a share of the measured time.
The committed Griffin-Lim rows ran with MIOPEN_FIND_MODE=FAST, which keeps the conv rows' first-call MIOpen search
short; MIOpen then picks its convolution solution by heuristics instead of timing them, so the conv rows may be slower
than after a full search.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mixgan_tts_amd as mg  # noqa: E402

HBM_TBS = 8.0
N_FFT, HOP, WIN, N_MELS, SR = 1024, 256, 1024, 80, 22050
NB = N_FFT // 2 + 1


def timed(fn, iters):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


class ConvSTFT:
    """The reference's STFT (audio/stft.py) on the device in fp32 eager."""

    def __init__(self, dev):
        fb = np.fft.fft(np.eye(N_FFT))
        fb = np.vstack([np.real(fb[:NB]), np.imag(fb[:NB])])
        w = mg.audio.pad_center(mg.audio.hann_window(WIN), N_FFT)
        self.fwd = (torch.FloatTensor(fb[:, None, :]) * torch.from_numpy(w).float()).to(dev)
        self.inv = (torch.FloatTensor(np.linalg.pinv(N_FFT / HOP * fb).T[:, None, :])
                    * torch.from_numpy(w).float()).to(dev)
        self.dev = dev
        self._ws = {}

    def transform(self, x):
        x = F.pad(x.unsqueeze(1), (N_FFT // 2, N_FFT // 2), mode="reflect")
        ft = F.conv1d(x, self.fwd, stride=HOP)
        re, im = ft[:, :NB], ft[:, NB:]
        return torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re)

    def inverse(self, mag, phase):
        y = F.conv_transpose1d(torch.cat([mag * torch.cos(phase), mag * torch.sin(phase)], 1), self.inv, stride=HOP)
        T = mag.shape[-1]
        if T not in self._ws:
            ws = torch.from_numpy(mg.audio.window_sumsquare("hann", T, HOP, WIN, N_FFT)).to(self.dev)
            self._ws[T] = (ws, torch.nonzero(ws > np.finfo(np.float32).tiny)[:, 0])
        ws, nz = self._ws[T]
        y[:, :, nz] /= ws[nz]
        y *= float(N_FFT) / HOP
        return y[:, :, N_FFT // 2:-(N_FFT // 2)]

    def mel(self, x, basis):
        mag, _ = self.transform(x)
        return torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5)), torch.norm(mag, dim=1)

    def griffin_lim(self, mags, angles, n_iters):
        sig = self.inverse(mags, angles).squeeze(1)
        for _ in range(n_iters):
            _, angles = self.transform(sig)
            sig = self.inverse(mags, angles).squeeze(1)
        return sig


class RocfftSTFT:
    """The same transform through torch.stft / torch.istft (rocFFT)."""

    def __init__(self, dev):
        self.win = torch.from_numpy(mg.audio.pad_center(mg.audio.hann_window(WIN), N_FFT)).float().to(dev)

    def spec(self, x):
        return torch.stft(x, N_FFT, HOP, N_FFT, self.win, center=True, pad_mode="reflect", return_complex=True)

    def mel(self, x, basis):
        mag = self.spec(x).abs()
        return torch.log(torch.clamp(torch.matmul(basis, mag), min=1e-5)), torch.norm(mag, dim=1)

    def griffin_lim(self, mags, angles, n_iters):
        L = (mags.shape[-1] - 1) * HOP
        sig = torch.istft(torch.polar(mags, angles), N_FFT, HOP, N_FFT, self.win, center=True, length=L)
        for _ in range(n_iters):
            angles = self.spec(sig).angle()
            sig = torch.istft(torch.polar(mags, angles), N_FFT, HOP, N_FFT, self.win, center=True, length=L)
        return sig


def mel_bytes(B, N):
    T = 1 + N // HOP
    return 4 * (B * N + B * (N_MELS + 1) * T)


def gl_bytes(B, T, iters):
    """T: spectrum frames after the drop.  Initial inverse + iters x (phase STFT + inverse)."""
    sig, spec = 4 * B * (T - 1) * HOP, 4 * B * NB * T
    return 4 * B * N_MELS * (T + 1) + (spec + spec + sig) + iters * ((sig + spec) + (spec + spec + sig))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--gl-iters", type=int, default=60)
    ap.add_argument("--only", default=None, help="native | conv | rocfft")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="mel,gl", help="comma list of row groups: mel, gl")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tac = mg.audio.TacotronSTFT(N_FFT, HOP, WIN, N_MELS, SR, 0.0, 8000).to(dev)
    basis = tac.mel_basis
    conv, rf = ConvSTFT(dev), RocfftSTFT(dev)
    rows = []
    if args.out and os.path.exists(args.out):
        os.remove(args.out)

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    groups = args.rows.split(",")

    N = 256000
    for B in (16, 1) if "mel" in groups else ():
        g = torch.Generator().manual_seed(B)
        x = ((torch.rand(B, N, generator=g) * 2 - 1) * 0.9).to(dev)
        impls = {"native": lambda: tac.mel_spectrogram(x), "conv": lambda: conv.mel(x, basis),
                 "rocfft": lambda: rf.mel(x, basis)}
        for name, fn in impls.items():
            if args.only and name != args.only:
                continue
            with torch.no_grad():
                ms = timed(fn, args.iters)
            nbytes = mel_bytes(B, N)
            emit({"row": "mel_energy", "impl": name, "B": B, "samples": N, "ms": round(ms, 4), "bytes": nbytes,
                  "hbm_bound_ms": round(nbytes / (HBM_TBS * 1e12) * 1e3, 4),
                  "frac_hbm_bound": round(nbytes / (HBM_TBS * 1e12) * 1e3 / ms, 3), "iters": args.iters})

    T_mel = 1000
    for B in (1, 16) if "gl" in groups else ():
        g = torch.Generator().manual_seed(100 + B)
        logmel = (torch.randn(B, N_MELS, T_mel, generator=g) - 5.0).to(dev)
        ang = ((torch.rand(B, NB, T_mel - 1, generator=g) * 2 - 1) * math.pi).to(dev)

        def spec_of(m):
            return (torch.matmul(basis.t(), torch.exp(m)) * 1000)[:, :, :-1].contiguous()

        impls = {"native": lambda: mg.audio.mel_to_audio(logmel, tac, args.gl_iters, angles=ang),
                 "conv": lambda: conv.griffin_lim(spec_of(logmel), ang, args.gl_iters),
                 "rocfft": lambda: rf.griffin_lim(spec_of(logmel), ang, args.gl_iters)}
        for name, fn in impls.items():
            if args.only and name != args.only:
                continue
            with torch.no_grad():
                ms = timed(fn, args.iters)
            nbytes = gl_bytes(B, T_mel - 1, args.gl_iters)
            emit({"row": "griffin_lim", "impl": name, "B": B, "mel_frames": T_mel, "n_iters": args.gl_iters,
                  "ms": round(ms, 3), "bytes": nbytes, "hbm_bound_ms": round(nbytes / (HBM_TBS * 1e12) * 1e3, 4),
                  "frac_hbm_bound": round(nbytes / (HBM_TBS * 1e12) * 1e3 / ms, 3), "iters": args.iters})


if __name__ == "__main__":
    main()
