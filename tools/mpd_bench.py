#!/usr/bin/env python3
"""HiFi-GAN multi-period discriminator timing at the training shape of hifigan/config.json: B = 16 real + 16 generated
segments of 8192 samples.  Two phases of VocoderGANTrainer.step, each forward + loss + backward:
    d: parameters trainable, y_hat detached, hifigan_discriminator_loss
    g: parameters frozen, y_hat requires grad, hifigan_generator_loss + hifigan_feature_loss
native (hifigan_discriminators.py on csrc/mpd.hip) against the published network built from torch.nn.Conv2d +
torch.nn.utils.weight_norm in stock PyTorch-ROCm eager mode (same weights, loaded by state_dict(); same GPU, same loss
code), alternated call by call, each call bracketed by device events after a warm-up.  No optimizer step.

--step adds the whole VocoderGANTrainer.step at B = 16 x 32 frames (native generator, native multi-scale discriminator,
default AdamW) with the eager and with the native multi-period discriminator, two trainers from the same seed alternated
step by step.

    python tools/mpd_bench.py [--runs 3] [--iters 20] [--warmup 5] [--native-only] [--step] [--out FILE]
runs --runs measurements, each in a fresh child process (the first with the kernel tables), and writes the record of
profiles/mpd_bench.json to --out (that file by default): per phase the medians of every run, the eager side's spread
(max - min of its medians) and whether the native median is below the eager one of the same run by more than that
spread; "kernels_d" / "kernels_g", the native phase's device time per kernel name (one profiled call, microseconds,
descending); "rates", the achieved fraction of the fp32 MFMA rate per convolution case.
    python tools/mpd_bench.py --merge RUN.json RUN.json ...     the same record from single-run files, no GPU
    python tools/mpd_bench.py --single [--no-kernels] [--out RUN.json]     one measurement in this process: prints one
JSON line (the single-run layout) and writes it to --out when one is given."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import types
import warnings

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mixgan_tts_amd as mg  # noqa: E402
from mixgan_tts_amd.hifigan_discriminators import MPD_PERIODS, MPD_CHANNELS, LRELU_SLOPE  # noqa: E402

H_GEN = {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
         "upsample_initial_channel": 512, "resblock_kernel_sizes": [3, 7, 11],
         "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}


class EagerDiscriminatorP(nn.Module):
    """hifigan/models.py DiscriminatorP."""

    def __init__(self, period):
        super().__init__()
        self.period = period
        ch = MPD_CHANNELS
        wn = nn.utils.weight_norm
        self.convs = nn.ModuleList([wn(nn.Conv2d(ch[j], ch[j + 1], (5, 1), (3 if j < 4 else 1, 1), padding=(2, 0)))
                                    for j in range(5)])
        self.conv_post = wn(nn.Conv2d(ch[5], 1, (3, 1), 1, padding=(1, 0)))

    def forward(self, x):
        fmap = []
        b, c, t = x.shape
        if t % self.period != 0:
            x = F.pad(x, (0, self.period - t % self.period), "reflect")
            t = x.shape[2]
        x = x.view(b, c, t // self.period, self.period)
        for conv in self.convs:
            x = F.leaky_relu(conv(x), LRELU_SLOPE)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap


class EagerMPD(nn.Module):
    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([EagerDiscriminatorP(p) for p in MPD_PERIODS])

    def forward(self, y, y_hat):
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for d in self.discriminators:
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
            rows[ev.key[:72]] = [round(t, 1), ev.count]
    return sorted(([k] + v for k, v in rows.items()), key=lambda r: -r[1])[:24]


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def alternate(sides, warmup, iters):
    for _ in range(warmup):
        for _, fn in sides:
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in sides}
    for _ in range(iters):
        for k, fn in sides:
            ms[k].append(timed(fn))
    return ms


PEAK_TFLOPS = 157.3      # fp32 MFMA, v_mfma_f32_32x32x2_f32
CASES = {("5", "3"): "stride3_forward_K5", ("2", "1"): "polyphase_dgrad_K2", ("5", "1"): "stride1_K5_1024to1024_fwd_and_dgrad"}


def rates(run):
    """Fraction of the fp32 MFMA rate per convolution case: GEMM flops issued on the slotted axis of all five periods
    (slack columns and the polyphase pack's zero tap included; `useful` counts live columns and real taps only) over the
    summed device time of that case's conv_mfma_kernel forms in the run's kernel tables."""
    N, T = run["B_real"] + run["B_generated"], run["samples"]
    issued = {k: {"d": 0, "g": 0} for k in CASES.values()}
    useful = {k: 0 for k in CASES.values()}
    for p in MPD_PERIODS:
        H, S = mg.ops.period_geometry(T, p)
        R = N * p
        for j in range(4):
            ci, co = MPD_CHANNELS[j], MPD_CHANNELS[j + 1]
            for ph in "dg":
                issued["stride3_forward_K5"][ph] += 2 * co * ci * 5 * R * S[j + 1]
                if j > 0 or ph == "g":      # the discriminator phase needs no data gradient below layer 0
                    issued["polyphase_dgrad_K2"][ph] += 2 * 3 * ci * co * 2 * R * S[j + 1]
            useful["stride3_forward_K5"] += 2 * co * ci * 5 * R * H[j + 1]
            useful["polyphase_dgrad_K2"] += 2 * co * ci * 5 * R * H[j + 1] if j > 0 else 0
        c = MPD_CHANNELS[5]
        for ph in "dg":
            issued["stride1_K5_1024to1024_fwd_and_dgrad"][ph] += 2 * 2 * c * c * 5 * R * S[5]
        useful["stride1_K5_1024to1024_fwd_and_dgrad"] += 2 * 2 * c * c * 5 * R * H[5]
    out = {"peak": "%.1f TFLOP/s fp32 MFMA" % PEAK_TFLOPS}
    for name in CASES.values():
        row = {"gflop_issued_d": round(issued[name]["d"] / 1e9, 1), "gflop_useful": round(useful[name] / 1e9, 1)}
        for ph in "dg":
            us = 0.0
            for kernel, t, _ in run.get("kernels_" + ph, []):
                m = re.search(r"conv_mfma_kernel<(\d+), (\d+)", kernel)
                if m and CASES.get((m[1], m[2])) == name:
                    us += t
            if us:
                row["us_" + ph] = round(us)
                row["fraction_" + ph] = round(issued[name][ph] / us / 1e6 / PEAK_TFLOPS, 2)
        out[name] = row
    return out


def merge(runs):
    """The record of profiles/mpd_bench.json from single-run results."""
    first = runs[0]
    out = {"what": first["what"] + "; %d runs, each in a fresh process" % len(runs),
           "rule": "a phase clears the margin when the native median is below the eager median of the same run by more "
                   "than the eager side's spread (max - min of its medians over the runs)",
           "gpu": first["gpu"], "B_real": first["B_real"], "B_generated": first["B_generated"], "samples": first["samples"],
           "iters": first["iters"], "warmup": first["warmup"]}
    for key, nat, eag in (("d", "d_native_ms_median", "d_eager_ms_median"), ("g", "g_native_ms_median", "g_eager_ms_median"),
                          ("step", "step_native_mpd_ms_median", "step_eager_mpd_ms_median")):
        if nat not in first:
            continue
        out[key] = {"native_ms_median": [r[nat] for r in runs]}
        if eag in first:
            e = [r[eag] for r in runs]
            gaps = [round(b - a, 3) for a, b in zip(out[key]["native_ms_median"], e)]
            spread = round(max(e) - min(e), 3)
            out[key].update({"eager_ms_median": e, "eager_spread": spread, "eager_minus_native": gaps,
                             "clears_margin": all(g > spread for g in gaps)})
    for k in ("kernels_d", "kernels_g"):
        if k in first:
            out[k] = first[k]
    if "kernels_d" in first:
        out["rates"] = rates(first)
    return out


def write(res, path, indent=None):
    text = json.dumps(res, indent=indent)
    print(text)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--merge", nargs="+", metavar="RUN.json")
    ap.add_argument("--single", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    record = os.path.join(ROOT, "profiles", "mpd_bench.json")
    if a.merge:
        return write(merge([json.load(open(f)) for f in a.merge]), a.out or record, indent=1)
    if not a.single:      # this process stays off the GPU: every measurement is a child of its own
        runs = []
        with tempfile.TemporaryDirectory() as tmp:
            for i in range(a.runs):
                one = os.path.join(tmp, "run%d.json" % i)
                cmd = [sys.executable, os.path.abspath(__file__), "--single", "--out", one, "--iters", str(a.iters),
                       "--warmup", str(a.warmup)]
                cmd += ["--native-only"] * a.native_only + ["--step"] * a.step + ["--no-kernels"] * (i > 0 or a.no_kernels)
                subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
                runs.append(json.load(open(one)))
        return write(merge(runs), a.out or record, indent=1)
    if not torch.cuda.is_available():
        raise SystemExit("mpd_bench: needs the GPU")
    warnings.filterwarnings("ignore", category=FutureWarning)
    dev = "cuda"
    torch.manual_seed(0)
    B, T = 16, 8192
    nets = {"native": mg.MultiPeriodDiscriminator().to(dev).train()}
    if not a.native_only:
        nets["eager"] = EagerMPD().to(dev).train()
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

    res = {"what": "HiFi-GAN multi-period discriminator, forward + loss + backward per trainer phase", "B_real": B,
           "B_generated": B, "samples": T, "iters": a.iters, "warmup": a.warmup, "gpu": torch.cuda.get_device_name(0)}
    for phase, make in (("d", d_phase), ("g", g_phase)):
        sides = [(k, make(net)) for k, net in nets.items()]
        ms = alternate(sides, a.warmup, a.iters)
        for k, v in ms.items():
            res["%s_%s_ms_median" % (phase, k)] = round(statistics.median(v), 3)
            res["%s_%s_ms_min" % (phase, k)] = round(min(v), 3)
        if "eager" in ms:
            res["%s_speedup_median" % phase] = round(res["%s_eager_ms_median" % phase] / res["%s_native_ms_median" % phase], 2)
        if not a.no_kernels:
            res["kernels_" + phase] = kernel_table(sides[0][1])
    if a.step:
        frames = 32
        stft = mg.audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)
        mel = torch.rand(B, 80, frames, device=dev) * 13.5 - 11.5
        wav = torch.rand(B, 256 * frames, device=dev) * 1.8 - 0.9
        sd = {k: v.clone() for k, v in nets["native"].state_dict().items()}
        trainers = {}
        for k in nets:
            torch.manual_seed(1)
            gen = mg.vocoder.Generator(types.SimpleNamespace(**H_GEN)).to(dev).train()
            msd = mg.MultiScaleDiscriminator().to(dev).train()
            mpd = (mg.MultiPeriodDiscriminator() if k == "native" else EagerMPD()).to(dev).train()
            mpd.load_state_dict(sd, strict=True)
            trainers[k] = mg.VocoderGANTrainer(gen, stft, {"mpd": mpd, "msd": msd})
        ms = alternate([(k, (lambda t=t: t.step(mel, wav))) for k, t in trainers.items()], a.warmup, a.iters)
        for k, v in ms.items():
            res["step_%s_mpd_ms_median" % k] = round(statistics.median(v), 3)
            res["step_%s_mpd_ms_min" % k] = round(min(v), 3)
    write(res, a.out)


if __name__ == "__main__":
    main()
