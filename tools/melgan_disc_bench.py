#!/usr/bin/env python3
"""MelGAN multi-scale discriminator timing at the training shape: B = 16 real + 16 generated segments of 8192 samples,
Discriminator() at full width (3 scales, ndf 16, 4 grouped layers).  Two phases of VocoderGANTrainer.step with
objective="melgan", each forward + loss + backward:
    d: parameters trainable, y_hat detached, melgan_discriminator_loss (hinge)
    g: parameters frozen, y_hat requires grad, melgan_generator_loss + 10 * melgan_feature_loss
native (melgan_discriminators.py on csrc/gconv_c4.h and csrc/msd.hip) against the same network built from torch.nn.Conv1d
+ torch.nn.utils.weight_norm + ReflectionPad1d + AvgPool1d(4, 2, 1, count_include_pad=False) in stock PyTorch-ROCm eager
mode (same weights, same GPU, same loss code, both sides on the batch [y; y_hat]), alternated call by call, each call
bracketed by device events after a warm-up.  No optimizer step.

    python tools/melgan_disc_bench.py [--iters 20] [--warmup 5] [--native-only] [--no-kernels] [--out FILE]
Prints one JSON line and writes it to --out (default profiles/melgan_disc_bench.json).  "kernels_d" / "kernels_g": the
native phase's device time per kernel name from ONE separate profiled call (microseconds, descending) -- profiled time,
not comparable with the unprofiled medians above."""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mixgan_tts_amd as mg  # noqa: E402
from mixgan_tts_amd.melgan_discriminators import nlayer_geometry, LRELU_SLOPE  # noqa: E402


class EagerNLayerDiscriminator(nn.Module):
    def __init__(self):
        super().__init__()
        geo = nlayer_geometry()
        model = nn.ModuleDict()
        for j, (ci, co, k, s, g, p) in enumerate(geo):
            conv = nn.utils.weight_norm(nn.Conv1d(ci, co, k, stride=s, padding=p, groups=g))
            if j == 0:
                model["layer_0"] = nn.Sequential(nn.ReflectionPad1d(7), conv, nn.LeakyReLU(LRELU_SLOPE, True))
            elif j < len(geo) - 1:
                model["layer_%d" % j] = nn.Sequential(conv, nn.LeakyReLU(LRELU_SLOPE, True))
            else:
                model["layer_%d" % j] = conv
        self.model = model

    def forward(self, x):
        results = []
        for layer in self.model.values():
            x = layer(x)
            results.append(x)
        return results


class EagerDiscriminator(nn.Module):
    def __init__(self, num_D=3):
        super().__init__()
        self.model = nn.ModuleDict({"disc_%d" % i: EagerNLayerDiscriminator() for i in range(num_D)})
        self.downsample = nn.AvgPool1d(4, stride=2, padding=1, count_include_pad=False)

    def forward(self, x):
        results = []
        for disc in self.model.values():
            results.append(disc(x))
            x = self.downsample(x)
        return results

    def forward_pair(self, y, y_hat):
        B = y.shape[0]
        both = self.forward(torch.cat([y, y_hat], 0))
        return [[m[:B] for m in maps] for maps in both], [[m[B:] for m in maps] for maps in both]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "melgan_disc_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("melgan_disc_bench: needs the GPU")
    warnings.filterwarnings("ignore", category=FutureWarning)
    dev = "cuda"
    torch.manual_seed(0)
    B, T = 16, 8192
    nets = {"native": mg.melgan_discriminators.Discriminator().to(dev).train()}
    if not a.native_only:
        nets["eager"] = EagerDiscriminator().to(dev).train()
        nets["eager"].load_state_dict(nets["native"].state_dict(), strict=True)
    y = torch.rand(B, 1, T, device=dev) * 1.8 - 0.9
    y_hat = torch.rand(B, 1, T, device=dev) * 1.8 - 0.9

    def d_phase(net):
        def run():
            net.zero_grad(set_to_none=True)
            mg.melgan_discriminator_loss(*net.forward_pair(y, y_hat)).backward()
        return run

    def g_phase(net):
        params = list(net.parameters())

        def run():
            yh = y_hat.detach().requires_grad_()
            for p in params:
                p.requires_grad_(False)
            try:
                D_real, D_fake = net.forward_pair(y, yh)
                (mg.melgan_generator_loss(D_fake) + 10.0 * mg.melgan_feature_loss(D_real, D_fake)).backward()
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

    res = {"what": "MelGAN multi-scale discriminator, forward + loss + backward per trainer phase", "B_real": B,
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
