#!/usr/bin/env python3
"""Vocoder timing (profiles/*_vocoder_bench.jsonl): mel [B, 80, 1000] -> audio at B=1 and B=16.

  python tools/vocoder_bench.py [--iters N] [--only melgan_fused]

Rows: native MelGAN with the fused residual stacks (default), native MelGAN in the general form (fused_stack=False),
native HiFi-GAN V1, and the plain-torch MelGAN restatement (tests/melgan_torch.py) in stock PyTorch-ROCm eager on the
same GPU.  Each row times the generator forward alone with device events (median of --iters), after two warm-up calls.
MelGAN does about 90 MFLOP of useful work per mel frame (1.44 TFLOP at B=16, L=1000); the row prints the rate and
its fraction of the 157.3 TFLOP/s fp32 MFMA peak.  Weights are seeded (the restatement's calibrated ones).
"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mixgan_tts_amd as mg  # noqa: E402
import melgan_torch as MT  # noqa: E402

HIFIGAN_V1 = {"upsample_rates": (8, 8, 2, 2), "upsample_kernel_sizes": (16, 16, 4, 4), "upsample_initial_channel": 512,
              "resblock_kernel_sizes": (3, 7, 11), "resblock_dilation_sizes": ((1, 3, 5), (1, 3, 5), (1, 3, 5))}
PEAK_TFLOPS = 157.3


def melgan_flop_per_frame():
    """Useful FLOP per mel frame: 2 x MACs of every conv (transposed convs at their own stride)."""
    f = 2 * 512 * 80 * 7
    C, rate = 512, 1
    for r in (8, 8, 2, 2):
        C, rate = C // 2, rate * r
        f += 2 * (2 * C) * C * 2 * rate            # ConvTranspose1d: 2 taps per output sample
        f += 3 * rate * 2 * (C * C * 3 + 2 * C * C)  # ResnetBlocks: k=3 conv + the two 1x1
    return f + 2 * 32 * 7 * 256


def hifigan_flop_per_frame():
    f = 2 * 512 * 80 * 7
    C, rate = 512, 1
    for r in (8, 8, 2, 2):
        C, rate = C // 2, rate * r
        f += 2 * (2 * C) * C * 2 * rate
        f += rate * 2 * C * C * 2 * 3 * (3 + 7 + 11)
    return f + 2 * 32 * 7 * 256


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default=None, help="one row: melgan_fused | melgan_general | hifigan | melgan_eager")
    ap.add_argument("--batches", default="1,16")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ref = MT.seeded_generator(0)
    G = mg.MelGANGenerator()
    G.load_state_dict(ref.state_dict())
    G = G.to(dev).eval()
    eager = ref.to(dev).eval()
    torch.manual_seed(0)
    H = mg.vocoder.Generator(types.SimpleNamespace(**HIFIGAN_V1)).to(dev).eval()
    H.remove_weight_norm()
    L = 1000
    for B in [int(b) for b in args.batches.split(",")]:
        mel = (torch.randn(B, 80, L, generator=torch.Generator().manual_seed(B)) - 4.0).to(dev)

        def melgan(fused):
            def run():
                G.fused_stack = fused
                return G(mel)
            return run

        def eager_run():
            with torch.no_grad():
                return eager(mel)
        rows = [("melgan_fused", melgan(True), melgan_flop_per_frame()),
                ("melgan_general", melgan(False), melgan_flop_per_frame()),
                ("hifigan", lambda: H(mel), hifigan_flop_per_frame()),
                ("melgan_eager", eager_run, melgan_flop_per_frame())]
        for name, fn, fpf in rows:
            if args.only and name != args.only:
                continue
            ms = timed(fn, args.iters)
            tflops = fpf * B * L / (ms * 1e-3) / 1e12
            print(json.dumps({"row": name, "B": B, "L": L, "ms": round(ms, 3), "useful_tflop": round(fpf * B * L / 1e12, 3),
                              "tflops": round(tflops, 1), "frac_fp32_mfma_peak": round(tflops / PEAK_TFLOPS, 3),
                              "iters": args.iters}), flush=True)


if __name__ == "__main__":
    main()
