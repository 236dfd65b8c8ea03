#!/usr/bin/env python3
"""MelGAN generator training step timing: one GeneratorTrainer.step (forward_train + lambda_mel * L1(mel_diff(y_hat),
mel(y)) + backward + AdamW) over a MelVocoder at B = 16 x 32 frames (8192 samples), native (melgan.py / autograd.py on
melgan_train.hip) against the same step as stock PyTorch-ROCm eager autograd (F.pad reflect, F.conv1d,
F.conv_transpose1d, torch.fft.rfft; a copy of the same weights with weight norm, its own AdamW, same GPU), alternated
call by call, each call bracketed by device events after a warm-up.

    python tools/melgan_train_bench.py [--iters 20] [--warmup 5] [--native-only] [--no-kernels] [--out FILE]
Prints one JSON line and writes it to --out (default profiles/melgan_train_bench.json).  "kernels": the native step's
device time per kernel name (one profiled step, microseconds, descending)."""
import argparse
import copy
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mixgan_tts_amd as mg  # noqa: E402
from mixgan_tts_amd.melgan import RATIOS, SLOPE  # noqa: E402


def reflect_conv(x, conv, dil=1):
    w = conv.effective_weight()
    p = dil * (w.shape[2] - 1) // 2
    return F.conv1d(F.pad(x, (p, p), mode="reflect"), w, conv.bias, dilation=dil)


def eager_forward(G, mel, scale):
    """mel2wav/modules.py Generator.forward(mel * scale) on torch ops over G's parameters."""
    m, nres = G.model, G.n_residual_layers
    x = reflect_conv(mel * scale, m[1])
    for i, r in enumerate(RATIOS):
        base = 2 + i * (2 + nres)
        up = m[base + 1]
        x = F.conv_transpose1d(F.leaky_relu(x, SLOPE), up.effective_weight(), up.bias, stride=r, padding=r // 2)
        for j in range(nres):
            blk = m[base + 2 + j]
            t = F.leaky_relu(reflect_conv(F.leaky_relu(x, SLOPE), blk.block[2], blk.dilation), SLOPE)
            x = (F.conv1d(x, blk.shortcut.effective_weight(), blk.shortcut.bias)
                 + F.conv1d(t, blk.block[4].effective_weight(), blk.block[4].bias))
    return torch.tanh(reflect_conv(F.leaky_relu(x, SLOPE), m[len(m) - 2]))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "melgan_train_bench.json"))
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    voc = mg.MelVocoder().to(dev).train()
    twin = copy.deepcopy(voc.mel2wav)
    stft = mg.audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
    B, frames = 16, 32
    mel = torch.rand(B, 80, frames, device=dev) * 13.5 - 11.5
    wav = torch.rand(B, 256 * frames, device=dev) * 1.8 - 0.9
    window = stft.stft_fn._tables.on(dev)[0]
    basis = stft.mel_basis.to(dev)
    scale = 1.0 / math.log(10.0)
    tr = mg.GeneratorTrainer(voc, stft)
    opt = torch.optim.AdamW(twin.parameters(), lr=2e-4, betas=(0.8, 0.99))

    def native():
        tr.step(mel, wav)

    def eager():
        opt.zero_grad(set_to_none=True)
        m = eager_log_mel(eager_forward(twin, mel, scale).squeeze(1), window, basis)
        with torch.no_grad():
            target = eager_log_mel(wav, window, basis)
        (45.0 * F.l1_loss(m, target)).backward()
        opt.step()

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
    res = {"what": "MelGAN GeneratorTrainer.step (forward_train + mel L1 + backward + AdamW)", "B": B, "frames": frames,
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
