"""Times one alignment pass (csrc/align.hip) at corpus shapes: emissions and the Viterbi pass for 16 utterances of
about 800 frames and about 300 states (D = 80, G = 250), and the statistics of the same batch, beside the float64
numpy oracle's time for the same pass.  Prints one JSON line, microseconds as the median of --iters after --warmup,
between two events on the stream: `*_us` brackets the Python wrapper (its allocations and, for viterbi_align, the
upload of seq, skip and the two length vectors are inside, as a fit pays them), `*_kernel_us` one call of the C ABI
on buffers that are already on the device, which is the kernel and its launch.

    python tools/align_bench.py [--iters 30] [--warmup 5] [--no-oracle]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mixgan_tts_amd as mg  # noqa: E402

B, T, S, D, G = 16, 800, 300, 80, 250


def batch(seed=0):
    rng = np.random.default_rng(seed)
    n_frames = rng.integers(T - 150, T + 1, B).astype(np.int32)
    n_states = rng.integers(S - 60, S + 1, B).astype(np.int32)
    n_states -= 1 - n_states % 2      # odd: silence at both ends
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    seq = rng.integers(1, G, (B, S)).astype(np.int32)
    skip = np.zeros((B, S), np.uint8)
    for b in range(B):
        sil = np.unique(np.concatenate([[0, n_states[b] - 1], np.arange(10, n_states[b] - 2, 10)]))
        skip[b, sil], seq[b, sil] = 1, 0
    mean, var = rng.standard_normal((G, D)), rng.uniform(0.1, 2.0, (G, D))
    return x, n_frames, n_states, seq, skip, mg.aligner.model_tables(mean, var)


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    x, n_frames, n_states, seq, skip, tables = batch()
    xd, nfd = torch.from_numpy(x).cuda(), torch.from_numpy(n_frames).cuda()
    td = [torch.from_numpy(t).cuda() for t in tables]
    ll = mg.emissions(xd, nfd, *td)
    dur, score, ok = mg.viterbi_align(ll, seq, skip, n_frames, n_states)
    gauss = np.full((B, T), -1, np.int64)
    dh = dur.cpu().numpy()
    for b in range(B):
        gauss[b, :n_frames[b]] = np.repeat(seq[b], dh[b])
    gd = torch.from_numpy(gauss).cuda()
    torch.cuda.synchronize()
    out = {"shape": "B=%d T<=%d S<=%d D=%d G=%d" % (B, T, S, D, G), "frames": int(n_frames.sum()),
           "aligned_rows": int(ok.sum()),
           "emissions_us": round(median_us(lambda: mg.emissions(xd, nfd, *td), args.iters, args.warmup), 1),
           "viterbi_us": round(median_us(lambda: mg.viterbi_align(ll, seq, skip, n_frames, n_states), args.iters,
                                         args.warmup), 1),
           "stats_us": round(median_us(lambda: mg.gaussian_stats(xd, gd, G), args.iters, args.warmup), 1),
           "iters": args.iters}
    import ctypes
    L = mg.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    seq_d, skip_d, ns_d = torch.from_numpy(seq).cuda(), torch.from_numpy(skip).cuda(), torch.from_numpy(n_states).cuda()
    need = L.mg_align_viterbi_workspace_bytes(B, T, S)
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    ll2, dur2 = torch.empty_like(ll), torch.empty_like(dur)
    score2, ok2 = torch.empty_like(score), torch.empty_like(ok)

    def k_emis():
        assert L.mg_align_emissions(vp(xd), vp(nfd), B, T, D, vp(td[0]), vp(td[1]), vp(td[2]), G, vp(ll2), None) == 0

    def k_vit():
        assert L.mg_align_viterbi(vp(ll), vp(seq_d), vp(skip_d), vp(nfd), vp(ns_d), B, T, S, G, vp(dur2), vp(score2),
                                  vp(ok2), vp(ws), need, None) == 0

    with torch.cuda.stream(torch.cuda.default_stream()):
        out["emissions_kernel_us"] = round(median_us(k_emis, args.iters, args.warmup), 1)
        out["viterbi_kernel_us"] = round(median_us(k_vit, args.iters, args.warmup), 1)
    out["kernel_outputs_equal_wrapper"] = bool(torch.equal(ll2, ll) and torch.equal(dur2, dur))
    out["workspace_bytes"] = int(need)
    if not args.no_oracle:
        import align_oracle as O
        t0 = time.perf_counter()
        oll, _ = O.emissions(x, n_frames, *tables)
        t1 = time.perf_counter()
        odur, _, _ = O.viterbi(ll.cpu().numpy(), seq, skip, n_frames, n_states)
        t2 = time.perf_counter()
        out.update(oracle_emissions_ms=round((t1 - t0) * 1e3, 1), oracle_viterbi_ms=round((t2 - t1) * 1e3, 1),
                   durations_equal_oracle=bool(np.array_equal(odur, dh)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
