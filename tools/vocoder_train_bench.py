#!/usr/bin/env python3
"""HiFi-GAN generator training step timing: forward_train + lambda_mel * L1(mel_diff(y_hat), mel(y)) + backward, at the
shape of hifigan/config.json (B = 16, segment_size 8192 = 32 frames), native (vocoder.py / autograd.py on
vocoder_train.hip) against the same computation as stock PyTorch-ROCm eager autograd (F.conv1d, F.conv_transpose1d,
torch.fft.rfft; same weights with weight norm, same GPU), alternated call by call, each call bracketed by device
events after a warm-up.  No optimizer step on either side.

    python tools/vocoder_train_bench.py [--iters 20] [--warmup 5] [--native-only] [--no-kernels] [--out FILE]
Prints one JSON line and writes it to --out (default profiles/vocoder_train_bench.json).  "kernels": the native step's
device time per kernel name (one profiled step, microseconds, descending)."""
import argparse
import json
import os
import statistics
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mixgan_tts_amd as mg  # noqa: E402

H = {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
     "upsample_initial_channel": 512, "resblock_kernel_sizes": [3, 7, 11],
     "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}


def eager_forward(G, mel):
    """hifigan/models.py:145-165 on torch ops over G's parameters."""
    w = lambda m: m.effective_weight()  # noqa: E731
    x = F.conv1d(mel, w(G.conv_pre), G.conv_pre.bias, padding=3)
    nk = G.num_kernels
    for i, (u, k) in enumerate(zip(H["upsample_rates"], H["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), w(G.ups[i]), G.ups[i].bias, stride=u, padding=(k - u) // 2)
        xs = None
        for j in range(nk):
            rb = G.resblocks[i * nk + j]
            ks, r = rb.kernel_size, x
            for m, d in enumerate(rb.dilation):
                t = F.conv1d(F.leaky_relu(r, 0.1), w(rb.convs1[m]), rb.convs1[m].bias, dilation=d, padding=(ks * d - d) // 2)
                r = F.conv1d(F.leaky_relu(t, 0.1), w(rb.convs2[m]), rb.convs2[m].bias, padding=(ks - 1) // 2) + r
            xs = r if xs is None else xs + r
        x = xs / nk
    return torch.tanh(F.conv1d(F.leaky_relu(x), w(G.conv_post), G.conv_post.bias, padding=3))


def eager_log_mel(y, window, basis, hop=256, n_fft=1024):
    p = F.pad(y[:, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
    spec = torch.fft.rfft(p.unfold(1, n_fft, hop) * window, dim=2)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2)
    return torch.log(torch.clamp(torch.matmul(mag, basis.t()).transpose(1, 2), min=1e-5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocoder_train_bench.json"))
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    G = mg.vocoder.Generator(types.SimpleNamespace(**H)).to(dev).train()
    stft = mg.audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    B, frames = 16, 32
    mel = torch.rand(B, 80, frames, device=dev) * 13.5 - 11.5
    wav = torch.rand(B, 256 * frames, device=dev) * 1.8 - 0.9
    window = stft.stft_fn._tables.on(dev)[0]
    basis = stft.mel_basis.to(dev)
    with torch.no_grad():
        target = stft.mel_spectrogram_diff(wav)

    def native():
        G.zero_grad(set_to_none=True)
        m = stft.mel_spectrogram_diff(G.forward_train(mel).squeeze(1))
        (45.0 * F.l1_loss(m, target)).backward()

    def eager():
        G.zero_grad(set_to_none=True)
        m = eager_log_mel(eager_forward(G, mel).squeeze(1), window, basis)
        (45.0 * F.l1_loss(m, target)).backward()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    sides = [("native", native)] + ([] if a.native_only else [("eager", eager)])
    for _ in range(a.warmup):
        for _, fn in sides:
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in sides}
    for _ in range(a.iters):
        for k, fn in sides:
            ms[k].append(timed(fn))
    res = {"what": "HiFi-GAN generator train step (forward_train + mel L1 + backward)", "B": B, "frames": frames,
           "samples": 256 * frames, "iters": a.iters, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        res[k + "_ms_median"] = round(statistics.median(v), 3)
        res[k + "_ms_min"] = round(min(v), 3)
    if "eager" in ms:
        res["speedup_median"] = round(res["eager_ms_median"] / res["native_ms_median"], 2)
    if not a.no_kernels:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            native()
            torch.cuda.synchronize()
        rows = {}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            if t is None:
                t = getattr(ev, "cuda_time_total", 0.0)
            if t > 0:
                rows[ev.key[:60]] = [round(t, 1), ev.count]
        res["kernels"] = sorted(([k] + v for k, v in rows.items()), key=lambda r: -r[1])[:16]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
