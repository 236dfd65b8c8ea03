"""Times the two pitch kernels (csrc/pitch.hip) at corpus-builder shapes: a batch of 16 utterances of 10 s and one
utterance, 22050 Hz, hop 256.  Prints one JSON line per shape: microseconds per launch (median of --iters, after
--warmup) and frames per second.

    python tools/pitch_bench.py [--iters 50] [--warmup 10] [--once]

--once runs each kernel a single time per shape (for a kernel trace)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mixgan_tts_amd as mg  # noqa: E402

SR, HOP = 22050, 256


def speech_like(B, n, seed=0):
    """Voiced stretches (a gliding saw of seven harmonics) between noise and silence."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    out = np.zeros((B, n), dtype=np.float32)
    for b in range(B):
        f0 = 120.0 + 60.0 * b / max(1, B - 1) + 30.0 * np.sin(2 * np.pi * 0.7 * t + b)
        ph = 2 * np.pi * np.cumsum(f0) / SR
        x = sum(np.sin(h * ph) / h for h in range(1, 8))
        voiced = (np.sin(2 * np.pi * 0.9 * t + 0.3 * b) > -0.3)
        x = np.where(voiced, 0.3 * x, 0.02 * rng.standard_normal(n))
        out[b] = x
    return out


def median_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    iters, warmup = (1, 0) if args.once else (args.iters, args.warmup)
    for B, seconds in ((16, 10.0), (1, 10.0)):
        n = int(SR * seconds)
        x = torch.from_numpy(speech_like(B, n)).cuda()
        period, cost, rms, nf = mg.yin_candidates(x, SR, HOP)
        f0 = mg.pitch_track(period, cost, rms, nf, SR)
        torch.cuda.synchronize()
        frames = int(nf.sum())
        t1 = median_us(lambda: mg.yin_candidates(x, SR, HOP), iters, warmup)
        t2 = median_us(lambda: mg.pitch_track(period, cost, rms, nf, SR), iters, warmup)
        print(json.dumps({"shape": "%d x %.0f s" % (B, seconds), "sampling_rate": SR, "hop": HOP, "frames": frames,
                          "voiced_fraction": round(float((f0 > 0).double().mean()), 3),
                          "yin_candidates_us": round(t1, 1), "pitch_track_us": round(t2, 1),
                          "yin_frames_per_s": round(frames / t1 * 1e6), "track_frames_per_s": round(frames / t2 * 1e6),
                          "audio_seconds_per_s": round(B * seconds / (t1 + t2) * 1e6, 1), "iters": iters}))


if __name__ == "__main__":
    main()
