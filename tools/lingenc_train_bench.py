#!/usr/bin/env python3
"""Train-mode LinguisticEncoder timing: what one train.py step runs of the encoder -- a forward under no_grad (the
D phase), a forward with grad and its backward (the G phase) -- at the per-GPU shard of configs[3] (B = 8, ~120
phonemes, ~950 frames), native (linguistic_encoder.py on lingenc.hip / lingenc_train.hip) against the same
computation as stock PyTorch-ROCm eager (tests/lingenc_torch.py under autograd, same weights, same GPU), alternated
call by call, each call bracketed by device events after a warm-up.

The eager restatement has no dropout (it is the eval-mode forward); the native side runs with the reference's dropout,
so it does the extra mask work.  Both sides backpropagate the same scalar: sum(coef * x) + sum(pitch) + sum(energy)
+ the sum of the finite word-level log durations.

    python tools/lingenc_train_bench.py [--iters 20] [--warmup 5] [--native-only] [--out FILE]
Prints one JSON line per configuration (and appends it to --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mixgan_tts_amd as mg  # noqa: E402
import lingenc_torch as LT  # noqa: E402
from helpers import write_stats  # noqa: E402


def make_batch(B, n_ph, n_frames, gen, dev):
    wbs, durs = [], []
    for b in range(B):
        n = n_ph - 4 * b
        w = []
        while sum(w) < n:
            w.append(int(torch.randint(1, 5, (1,), generator=gen)))
        w[-1] -= sum(w) - n
        wbs.append(w)
        total = n_frames - 40 * b
        d = torch.full((n,), total // n)
        d[: total - total // n * n] += 1
        durs.append(d)
    Tw = max(len(w) for w in wbs)
    Tp = max(sum(w) for w in wbs)
    wb = torch.zeros(B, Tw, dtype=torch.long)
    texts = torch.zeros(B, Tp, dtype=torch.long)
    dt = torch.zeros(B, Tp, dtype=torch.long)
    for b, w in enumerate(wbs):
        wb[b, :len(w)] = torch.tensor(w)
        texts[b, :sum(w)] = torch.randint(1, 361, (sum(w),), generator=gen)
        dt[b, :sum(w)] = durs[b]
    src_lens = wb.sum(1)
    src_w_lens = torch.tensor([len(w) for w in wbs])
    src_mask = torch.arange(Tp)[None] < src_lens[:, None]
    src_w_mask = torch.arange(Tw)[None] < src_w_lens[:, None]
    mel_lens = dt.sum(1)
    L = int(mel_lens.max())
    mel_mask = torch.arange(L)[None] < mel_lens[:, None]
    pt = torch.randn(B, Tp, generator=gen) * src_mask
    et = torch.randn(B, Tp, generator=gen) * src_mask
    c = lambda t: t.to(dev)  # noqa: E731
    return (c(texts), c(src_lens), c(wb), c(src_mask), c(src_w_lens), c(src_w_mask), c(mel_mask), L, None, c(pt),
            c(et), c(dt), 1.0, 1.0)


def scalar(out, coef):
    logw = out[3]
    return (coef * out[0]).sum() + out[1].sum() + out[2].sum() + torch.where(torch.isfinite(logw), logw, 0.).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with open(os.path.join(ROOT, "tests", "golden", "lingenc_manifest.json")) as f:
        pre, mc, tr = json.load(f)["lingenc_infer"]["configs"]
    tmp = tempfile.mkdtemp()
    pre["path"]["preprocessed_path"] = write_stats(tmp, np.linspace(-11.5, -9.0, 80), np.linspace(1.0, 2.0, 80))
    dev = "cuda"
    torch.manual_seed(0)
    enc = mg.LinguisticEncoder(pre, mc, tr).to(dev).train()
    gen = torch.Generator().manual_seed(1)
    B, n_ph, n_frames = 8, 120, min(950, mc["max_seq_len"])
    args = make_batch(B, n_ph, n_frames, gen, dev)
    sd = dict(enc.state_dict(keep_vars=True))
    coef = torch.randn(B, args[7], mc["transformer"]["encoder_hidden"], device=dev) * 1e-2

    def native():
        with torch.no_grad():
            enc(*args)
        enc.zero_grad(set_to_none=True)
        scalar(enc(*args), coef).backward()

    def eager():
        with torch.no_grad():
            LT.encoder_forward(sd, (pre, mc, tr), *args)
        enc.zero_grad(set_to_none=True)
        scalar(LT.encoder_forward(sd, (pre, mc, tr), *args)[0], coef).backward()

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
    res = {"what": "LinguisticEncoder train step (no_grad fwd + fwd + bwd)", "B": B, "phonemes": int(args[3].sum(1).max()),
           "frames": int(args[7]), "iters": a.iters, "warmup": a.warmup,
           "gpu": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        res[k + "_ms_median"] = round(statistics.median(v), 3)
        res[k + "_ms_min"] = round(min(v), 3)
    if "eager" in ms:
        res["speedup_median"] = round(res["eager_ms_median"] / res["native_ms_median"], 2)
        res["note"] = "eager = tests/lingenc_torch.py under autograd, without dropout; native includes dropout"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
