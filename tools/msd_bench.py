#!/usr/bin/env python3
"""HiFi-GAN multi-scale discriminator timing at the training shape of hifigan/config.json: B = 16 real + 16 generated
segments of 8192 samples.  Two phases of VocoderGANTrainer.step, each forward + loss + backward:
    d: parameters trainable, y_hat detached, hifigan_discriminator_loss
    g: parameters frozen, y_hat requires grad, hifigan_generator_loss + hifigan_feature_loss
native (hifigan_discriminators.py on csrc/msd.hip) against the same network built from torch.nn.Conv1d +
torch.nn.utils.weight_norm / spectral_norm + AvgPool1d in stock PyTorch-ROCm eager mode (same weights, same GPU, same
loss code), alternated call by call, each call bracketed by device events after a warm-up.  No optimizer step.

    python tools/msd_bench.py [--iters 20] [--warmup 5] [--native-only] [--no-kernels] [--out FILE]
Prints one JSON line and writes it to --out (default profiles/msd_bench.json).  "kernels_d" / "kernels_g": the native
phase's device time per kernel name (one profiled call, microseconds, descending)."""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mixgan_tts_amd as mg  # noqa: E402
from mixgan_tts_amd.hifigan_discriminators import MSD_LAYERS, MSD_POST, LRELU_SLOPE  # noqa: E402


class EagerDiscriminatorS(nn.Module):
    def __init__(self, use_spectral_norm=False):
        super().__init__()
        norm = nn.utils.spectral_norm if use_spectral_norm else nn.utils.weight_norm
        self.convs = nn.ModuleList([norm(nn.Conv1d(ci, co, k, s, groups=g, padding=p)) for ci, co, k, s, g, p in MSD_LAYERS])
        self.conv_post = norm(nn.Conv1d(MSD_POST[0], MSD_POST[1], MSD_POST[2], 1, padding=MSD_POST[5]))

    def forward(self, x):
        fmap = []
        for conv in self.convs:
            x = F.leaky_relu(conv(x), LRELU_SLOPE)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap


class EagerMSD(nn.Module):
    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([EagerDiscriminatorS(True), EagerDiscriminatorS(), EagerDiscriminatorS()])
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=2), nn.AvgPool1d(4, 2, padding=2)])

    def forward(self, y, y_hat):
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for i, d in enumerate(self.discriminators):
            if i != 0:
                y, y_hat = self.meanpools[i - 1](y), self.meanpools[i - 1](y_hat)
            r, fr = d(y)
            g, fg = d(y_hat)
            y_d_rs.append(r)
            y_d_gs.append(g)
            fmap_rs.append(fr)
            fmap_gs.append(fg)
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs


def kernel_table(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        if t > 0:
            rows[ev.key[:60]] = [round(t, 1), ev.count]
    return sorted(([k] + v for k, v in rows.items()), key=lambda r: -r[1])[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msd_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("msd_bench: needs the GPU")
    warnings.filterwarnings("ignore", category=FutureWarning)
    dev = "cuda"
    torch.manual_seed(0)
    B, T = 16, 8192
    nets = {"native": mg.MultiScaleDiscriminator().to(dev).train()}
    if not a.native_only:
        nets["eager"] = EagerMSD().to(dev).train()
        nets["eager"].load_state_dict(nets["native"].state_dict(), strict=True)
    y = torch.rand(B, 1, T, device=dev) * 1.8 - 0.9
    y_hat = torch.rand(B, 1, T, device=dev) * 1.8 - 0.9

    def d_phase(net):
        def run():
            net.zero_grad(set_to_none=True)
            y_d_rs, y_d_gs, _, _ = net(y, y_hat)
            mg.hifigan_discriminator_loss(y_d_rs, y_d_gs)[0].backward()
        return run

    def g_phase(net):
        params = list(net.parameters())

        def run():
            yh = y_hat.detach().requires_grad_()
            for p in params:
                p.requires_grad_(False)
            try:
                _, y_d_gs, fmap_rs, fmap_gs = net(y, yh)
                (mg.hifigan_generator_loss(y_d_gs)[0] + mg.hifigan_feature_loss(fmap_rs, fmap_gs)).backward()
            finally:
                for p in params:
                    p.requires_grad_(True)
        return run

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    res = {"what": "HiFi-GAN multi-scale discriminator, forward + loss + backward per trainer phase", "B_real": B,
           "B_generated": B, "samples": T, "iters": a.iters, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0)}
    for phase, make in (("d", d_phase), ("g", g_phase)):
        sides = [(k, make(net)) for k, net in nets.items()]
        for _ in range(a.warmup):
            for _, fn in sides:
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k, _ in sides}
        for _ in range(a.iters):
            for k, fn in sides:
                ms[k].append(timed(fn))
        for k, v in ms.items():
            res["%s_%s_ms_median" % (phase, k)] = round(statistics.median(v), 3)
            res["%s_%s_ms_min" % (phase, k)] = round(min(v), 3)
        if "eager" in ms:
            res["%s_speedup_median" % phase] = round(res["%s_eager_ms_median" % phase] / res["%s_native_ms_median" % phase], 2)
        if not a.no_kernels:
            res["kernels_" + phase] = kernel_table(sides[0][1])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
