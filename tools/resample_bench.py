#!/usr/bin/env python3
"""Resampler timing (profiles/*_resample_bench.jsonl).

  python tools/resample_bench.py [--launches 200] [--repeats 7] [--cpu-procs 16] [--out profiles/..jsonl]

B = 16 utterances of 10 s at 44100 -> 22050 (1:2, the shared-taps kernel) and 48000 -> 22050 (147:320).  Per ratio:
  cpu     scipy.signal.resample_poly on float32 rows with the same taps, the 16 rows spread over --cpu-procs worker
          processes of the same box (run first, before the GPU is opened); median wall time of --repeats batches
  native  mg_resample_poly (csrc/resample.hip) on preallocated device tensors: two warm-up launches, then --launches
          launches inside one stream-event pair; median over --repeats pairs
Both as seconds of audio per second.  The native row also gives the kernel's work, counted from the shapes (one FMA
and one LDS dword per tap and output, padded taps included), as a share of the fp32 vector peak (157.3 TFLOP/s) and of
the ds_read_b32 rate (75 TB/s over every CU), the two limits such a loop can run into.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_TFLOPS, LDS_B32_TBS = 157.3, 75.0
B, SECONDS, TARGET = 16, 10.0, 22050
_CPU = {}


def _cpu_row(b):
    from scipy.signal import resample_poly
    return resample_poly(_CPU["x"][b], _CPU["up"], _CPU["down"], window=_CPU["h"]).shape[0]


def cpu_rate(x, up, down, h, procs, repeats):
    import multiprocessing as mp
    _CPU.update(x=x, up=up, down=down, h=h.astype(np.float32))
    with mp.get_context("fork").Pool(procs) as pool:
        pool.map(_cpu_row, range(B))      # warm the workers
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            pool.map(_cpu_row, range(B))
            ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-procs", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows, inputs = [], {}
    if args.out and os.path.exists(args.out):
        os.remove(args.out)

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    # the filter without importing the package: the GPU stays closed while the worker processes exist
    def kaiser_sinc(up, down):
        m = max(up, down)
        n = np.arange(-64 * m, 64 * m + 1, dtype=np.float64)
        h = 0.9475937167399596 / m * np.sinc(0.9475937167399596 / m * n) * np.kaiser(len(n), 14.769656459379492)
        return h / h.sum()

    for orig_sr, (up, down) in ((44100, (1, 2)), (48000, (147, 320))):
        n = int(orig_sr * SECONDS)
        x = (np.random.default_rng(orig_sr).random((B, n), dtype=np.float32) * 2 - 1) * 0.9
        inputs[orig_sr] = x
        s = cpu_rate(x, up, down, kaiser_sinc(up, down), args.cpu_procs, max(3, args.repeats // 2))
        emit({"row": "resample", "impl": "cpu", "orig_sr": orig_sr, "target_sr": TARGET, "B": B, "seconds_each": SECONDS,
              "procs": args.cpu_procs, "ms": round(s * 1e3, 2), "audio_s_per_s": round(B * SECONDS / s, 1)})

    import torch
    import mixgan_tts_amd as mg
    from mixgan_tts_amd._lib import fptr, check, stream_ptr
    import ctypes
    dev = torch.device("cuda", 0)
    for orig_sr, x in inputs.items():
        up, down = mg.audio.resample_ratio(orig_sr, TARGET)
        n = x.shape[1]
        m = -(-n * up // down)
        xd = torch.from_numpy(x).to(dev)
        y = torch.empty(B, m, device=dev)
        taps, half = mg.audio._resample_table(up, down, dev)
        Kp = taps.shape[1]
        assert np.allclose(kaiser_sinc(up, down), mg.audio.resample_filter(up, down), rtol=1e-12, atol=0)

        def launch():
            check(mg.lib().mg_resample_poly(fptr(xd), n, ctypes.c_void_p(0), B, n, fptr(taps), up, down, Kp, half,
                                            fptr(y), m, m, stream_ptr()))
        launch()
        launch()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                launch()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / args.launches)
        ms = sorted(ts)[len(ts) // 2]
        fma = B * m * Kp
        emit({"row": "resample", "impl": "native", "orig_sr": orig_sr, "target_sr": TARGET, "B": B,
              "seconds_each": SECONDS, "up": up, "down": down, "taps_per_output": Kp, "ms": round(ms, 4),
              "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
              "audio_s_per_s": round(B * SECONDS / (ms * 1e-3), 1), "fma": fma,
              "tflops": round(2 * fma / (ms * 1e-3) / 1e12, 2),
              "frac_fp32_valu_peak": round(2 * fma / (ms * 1e-3) / 1e12 / VALU_TFLOPS, 3),
              "frac_lds_b32_rate": round(4 * fma / (ms * 1e-3) / 1e12 / LDS_B32_TBS, 3),
              "launches": args.launches, "repeats": args.repeats})


if __name__ == "__main__":
    main()
