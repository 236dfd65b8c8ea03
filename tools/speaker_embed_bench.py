#!/usr/bin/env python3
"""DeepSpeaker speaker embedder timing on the GPU: the fbank front end (trim + crop draw + kernel), the ResCNN network
(convs + head) and both (DeepSpeakerModel.embed) at N in {1, 64, 256} 3-s utterances, median of device-event timings
after warm-up; and the same network as a float32 restatement in stock PyTorch eager (NCHW F.conv2d through MIOpen,
BN folded the same way, clamp / add) on the same inputs.  Useful FLOP: 2 MACs of every conv and the Dense per
utterance (5.33 GFLOP), against the 157.3 TFLOP/s fp32 MFMA peak.

    python tools/speaker_embed_bench.py [--out profiles/r08_a_speaker_embed_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mixgan_tts_amd as mg  # noqa: E402
from mixgan_tts_amd import speaker_embedder as S  # noqa: E402
import deepspeaker_ref as R  # noqa: E402

PEAK_TFLOPS = 157.3


def useful_flop():
    f, h, w, ci = 0, 160, 64, 1
    for _, co, k, s in S.layer_specs():
        ho, wo = S.tf_same_padding(h, k, s)[0], S.tf_same_padding(w, k, s)[0]
        f += 2 * ho * wo * co * k * k * ci
        h, w, ci = ho, wo, co
    return f + 2 * 2048 * 512


def timed(fn, warm, iters):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def eager_net(W):
    """float32 stock-eager restatement with BN folded: closures over device tensors."""
    layers = []
    for name, f, k, s in S.layer_specs():
        sc = W[name + "_bn/gamma:0"] / np.sqrt(W[name + "_bn/moving_variance:0"] + S.BN_EPS)
        w = torch.from_numpy((W[name + "/kernel:0"] * sc).astype(np.float32)).permute(3, 2, 0, 1).contiguous().cuda()
        b = torch.from_numpy(((W[name + "/bias:0"] - W[name + "_bn/moving_mean:0"]) * sc
                              + W[name + "_bn/beta:0"]).astype(np.float32)).cuda()
        layers.append((name, w, b, k, s))
    aw = torch.from_numpy(W["affine/kernel:0"].astype(np.float32)).cuda()
    ab = torch.from_numpy(W["affine/bias:0"].astype(np.float32)).cuda()

    def run(x):
        x = x[:, None]
        for name, w, b, k, s in layers:
            if name.endswith("_2a"):
                block_in = x
            _, pt, pb = S.tf_same_padding(x.shape[2], k, s)
            _, pl, pr = S.tf_same_padding(x.shape[3], k, s)
            x = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, b, stride=s).clamp_(0, 20)
            if name.endswith("_2b"):
                x = (x + block_in).clamp_(0, 20)
        h = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, 2048).mean(1) @ aw + ab
        return h * torch.rsqrt(torch.clamp((h * h).sum(1, keepdim=True), min=1e-12))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_a_speaker_embed_bench.jsonl"))
    ap.add_argument("--sizes", default="1,64,256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "speaker_embed_bench needs the GPU"
    torch.backends.cudnn.benchmark = True
    W = R.seeded_weights()
    model = S.DeepSpeakerModel().load_keras_weights(W)
    eager = eager_net(W)
    flop = useful_flop()
    rows = []
    rng = np.random.default_rng(0)
    for N in [int(v) for v in args.sizes.split(",")]:
        L = 3 * 22050
        audio = torch.from_numpy((0.3 * rng.standard_normal((N, L))).astype(np.float32)).cuda()
        lens = [L] * N
        offsets = model.frontend(audio, lens)[4]
        feats = model.frontend(audio, lens, offsets)[0]
        out_native = model.network(feats)
        with torch.no_grad():
            out_eager = eager(feats)
        diff = float((out_native - out_eager).abs().max())
        cases = [("frontend", lambda: model.frontend(audio, lens, offsets)),
                 ("network", lambda: model.network(feats)),
                 ("embed", lambda: model.embed(audio, lens, offsets)),
                 ("network_stock_eager", lambda: eager(feats))]
        for name, fn in cases:
            with torch.no_grad():
                med, best = timed(fn, args.warmup, args.iters)
            row = {"bench": "speaker_embed", "part": name, "N": N, "seconds_per_utt": 3.0, "ms_median": round(med, 4),
                   "ms_min": round(best, 4), "utt_per_s": round(N / med * 1e3, 1)}
            if name != "frontend":
                tf = flop * N / (med * 1e-3) / 1e12
                row.update({"useful_gflop_per_utt": round(flop / 1e9, 3), "tflops": round(tf, 2),
                            "fraction_of_fp32_mfma_peak": round(tf / PEAK_TFLOPS, 3)})
            if name == "network_stock_eager":
                row["max_abs_diff_vs_native"] = diff
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
