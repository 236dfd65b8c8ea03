"""Float64 plain-torch restatement of the reference's STFT (audio/stft.py): the reflect-padded conv1d against the
windowed real-DFT basis, conv_transpose1d against its pseudo-inverse, window-sum normalisation, and the log-mel /
energy of TacotronSTFT.mel_spectrogram.  The yardstick of the native audio front end at sizes the fixtures cannot
hold; window and filterbank come from the package's host tables (checked against the fixtures separately)."""
import numpy as np
import torch
import torch.nn.functional as F


class TorchSTFT:
    def __init__(self, hop, win=1024, n_fft=1024, device="cpu"):
        import mixgan_tts_amd as mg
        self.n_fft, self.hop, self.win = n_fft, hop, win
        fb = np.fft.fft(np.eye(n_fft))
        cut = n_fft // 2 + 1
        fb = np.vstack([np.real(fb[:cut]), np.imag(fb[:cut])])
        window = mg.audio.pad_center(mg.audio.hann_window(win), n_fft)
        self.fwd = torch.from_numpy(fb[:, None, :] * window).to(device)
        self.inv = torch.from_numpy(np.linalg.pinv(n_fft / hop * fb).T[:, None, :] * window).to(device)
        self.device = device

    def transform(self, x):
        x = x.to(self.device, torch.float64)
        p = self.n_fft // 2
        x = F.pad(x.unsqueeze(1), (p, p), mode="reflect")
        ft = F.conv1d(x, self.fwd, stride=self.hop)
        cut = self.n_fft // 2 + 1
        re, im = ft[:, :cut], ft[:, cut:]
        return torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re), re, im

    def inverse(self, mag, phase):
        import mixgan_tts_amd as mg
        mag, phase = mag.to(self.device, torch.float64), phase.to(self.device, torch.float64)
        y = F.conv_transpose1d(torch.cat([mag * torch.cos(phase), mag * torch.sin(phase)], 1), self.inv,
                               stride=self.hop)
        T = mag.shape[-1]
        ws = torch.from_numpy(mg.audio.window_sumsquare("hann", T, self.hop, self.win, self.n_fft,
                                                         dtype=np.float64)).to(self.device)
        nz = ws > np.finfo(np.float32).tiny
        y[:, :, nz] /= ws[nz]
        y = y * (self.n_fft / self.hop)
        p = self.n_fft // 2
        return y[:, :, p:-p]

    def mel_energy(self, x, mel_basis):
        mag = self.transform(x)[0]
        mel = torch.matmul(mel_basis.to(self.device, torch.float64), mag)
        return torch.log(torch.clamp(mel, min=1e-5)), torch.norm(mag, dim=1), mel
