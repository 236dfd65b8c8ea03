"""Times the synthesis metrics' kernels (csrc/dtw.hip) at evaluation shapes: `mel_cepstra` of both sides and `dtw`
with its path, for 16 pairs of 1000 x 1100 frames, for one such pair, and for 2 pairs of 4000 x 4000 (the largest
BASELINE shape).  One JSON line per shape, microseconds as the median of --iters after --warmup between two events on
the stream: `*_us` brackets the Python wrapper (its allocations are inside, as an evaluation pays them),
`dtw_kernels_us` one call of the C ABI on buffers that are already there, which is the two kernels and their
launches.  For context only, the last line is the wall time of the float64 numpy restatement (tests/metrics_ref.py) on
one 1000 x 1100 pair on the host.  Nothing in the project did this work before, so there is no ratio to report.

    python tools/metrics_bench.py [--iters 20] [--warmup 3] [--out profiles/rNN_a_metrics_bench.jsonl] [--no-oracle]

Without --out the file takes the next free rNN_ prefix under profiles/."""
import argparse
import ctypes
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mixgan_tts_amd as mg  # noqa: E402
import metrics_ref as R  # noqa: E402

SHAPES = [(16, 1000, 1100), (1, 1000, 1100), (2, 4000, 4000)]
M, N_COEF = 80, 13


def next_profile_path():
    used = [int(m.group(1)) for m in (re.match(r"r(\d+)_", f) for f in os.listdir(os.path.join(ROOT, "profiles"))) if m]
    return os.path.join(ROOT, "profiles", "r%02d_a_metrics_bench.jsonl" % (max(used, default=0) + 1))


def mel_batch(B, Ta, Tb, seed=0):
    """Recordings' log-mels and time-warped, perturbed copies of them, ragged by up to 10 % below the padded lengths."""
    rng = np.random.default_rng(seed)
    la, lb = rng.integers(Ta - Ta // 10, Ta + 1, B), rng.integers(Tb - Tb // 10, Tb + 1, B)
    la[0], lb[0] = Ta, Tb
    ref, syn = np.zeros((B, Ta, M), np.float32), np.zeros((B, Tb, M), np.float32)
    for k in range(B):
        m = R.random_walk_mel(rng, la[k], M)
        ref[k, :la[k]] = m
        syn[k, :lb[k]] = m[R.warp_index(rng, la[k], lb[k])] + rng.normal(0.0, 0.3, (lb[k], M))
    return ref, syn, la.astype(np.int32), lb.astype(np.int32)


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
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench: no GPU; a timing taken elsewhere says nothing")
    out_path = args.out or next_profile_path()
    L, vp = mg.lib(), lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    lines = []
    for B, Ta, Tb in SHAPES:
        ref, syn, la, lb = mel_batch(B, Ta, Tb)
        ref_d, syn_d = torch.from_numpy(ref).cuda(), torch.from_numpy(syn).cuda()
        la_d, lb_d = torch.from_numpy(la).cuda(), torch.from_numpy(lb).cuda()
        c_ref, c_syn = mg.mel_cepstra(ref_d, la_d, N_COEF), mg.mel_cepstra(syn_d, lb_d, N_COEF)
        total, path_len, path = mg.dtw(c_ref, c_syn, la_d, lb_d, return_path=True)
        need = L.mg_dtw_workspace_bytes(B, Ta, Tb)
        ws = torch.empty(need, device="cuda", dtype=torch.uint8)
        stream = mg._lib.stream_ptr()

        def kernels():
            mg._lib.check(L.mg_dtw(vp(c_ref), vp(c_syn), vp(la_d), vp(lb_d), B, Ta, Tb, N_COEF, vp(total), vp(path_len),
                                   vp(path), vp(ws), need, stream))

        def whole():
            mg.mel_cepstral_distortion(ref_d, syn_d, la_d, lb_d, N_COEF, return_path=True)

        torch.cuda.synchronize()
        cep = median_us(lambda: (mg.mel_cepstra(ref_d, la_d, N_COEF), mg.mel_cepstra(syn_d, lb_d, N_COEF)),
                        args.iters, args.warmup)
        dtw_w = median_us(lambda: mg.dtw(c_ref, c_syn, la_d, lb_d, return_path=True), args.iters, args.warmup)
        dtw_k = median_us(kernels, args.iters, args.warmup)
        mcd = median_us(whole, args.iters, args.warmup)
        cells = int((la.astype(np.int64) * lb).sum())
        line = {"shape": "B=%d Ta<=%d Tb<=%d M=%d n_coef=%d" % (B, Ta, Tb, M, N_COEF), "cells": cells,
                "path_len_mean": float(path_len.float().mean()), "workspace_mb": round(need / 2 ** 20, 2),
                "mel_cepstra_both_us": round(cep[0], 1), "dtw_us": round(dtw_w[0], 1),
                "dtw_kernels_us": round(dtw_k[0], 1), "dtw_kernels_min_max_us": [round(dtw_k[1], 1), round(dtw_k[2], 1)],
                "mcd_end_to_end_us": round(mcd[0], 1), "cells_per_us": round(cells / dtw_k[0], 1),
                "mcd_db_mean": round(float(torch.nanmean(mg.mel_cepstral_distortion(ref_d, syn_d, la_d, lb_d))), 4),
                "iters": args.iters, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if not args.no_oracle:
        ref, syn, la, lb = mel_batch(1, 1000, 1100)
        t0 = time.perf_counter()
        a, b = R.cepstra(ref, la, N_COEF)[0], R.cepstra(syn, lb, N_COEF)[0]
        total, _, path = R.dtw(a, b)
        line = {"shape": "float64 numpy restatement on the host, one 1000 x 1100 pair (context only)",
                "wall_ms": round((time.perf_counter() - t0) * 1e3, 1), "mcd_db": round(float(R.mcd(total, len(path))), 4)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    print("wrote " + os.path.relpath(out_path, ROOT))


if __name__ == "__main__":
    main()
