#!/usr/bin/env python
"""What HotPathTrainer(exact_shards=True) costs per training step, on one GPU.

The step of bench.py --workload train (BASELINE configs[3]: multi-speaker naive, batch 8 per GPU, L = 1000) on a world
of ONE with the collectives forced ("nccl" = RCCL, GradBucket.always_exchange), timed with device events around
`--steps` steps after `--warmup` steps per variant, the variants alternating for `--rounds` rounds in one process:

  off            exact_shards off: the mean exchange (what the trainer did before exact mode existed)
  on             exact_shards on, shape= given, equal lengths: + the row-count kernel, the int64 count all-reduce on a side
                 stream, the denominators handed to the loss kernels, a SUM instead of a mean
  on_noshape     ... without shape=: the trainer exchanges it itself (on a world of one that is no collective: only the
                 bookkeeping is timed here; on several ranks it is one host round trip)
  two_length     on; half the items L frames, half L/2 (masked, zero past L/2): the batch a single process would pad too
  short_padded   on; EVERY item L/2 frames and handed over L/2 frames long, shape.max_len = L: a short rank next to a long
                 one -- the trainer pads to L and runs at L
  short_alone    on; the same items with shape.max_len = L/2: what that rank would run if nobody were longer.
                 short_padded - short_alone is what padding to the longest rank costs the short rank.

`--tree DIR` imports the package from another checkout (one that may not know exact_shards: only `off` runs there), so
that the same script times the parent commit's step at the same shape on the same box.  Prints one JSON line; `--out`
also writes it to a file.  Needs the GPU; reads nothing outside the repository."""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants", default="off,on,on_noshape,two_length,short_padded,short_alone")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import torch.distributed as dist
    import mixgan_tts_amd as mg
    from helpers import hot_path_configs, write_stats
    assert os.path.abspath(mg.__file__).startswith(tree), mg.__file__
    if not torch.cuda.is_available():
        raise SystemExit("exact_shards_cost: needs the GPU (a CPU run says nothing about step time)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1)
    B, L, M = args.batch, args.frames, 80
    with tempfile.TemporaryDirectory() as d:
        stats = write_stats(d, [-11.5] * M, [2.0] * M, n_speakers=218)
        a, pre, mc, tr = hot_path_configs("naive", 4, multi_speaker=True, stats_dir=stats)
        G = mg.GaussianDiffusion(a, pre, mc, tr)
        D = mg.JCUDiscriminator(pre, mc, tr)
    gen = torch.Generator().manual_seed(1234)
    with torch.no_grad():
        for p in list(G.parameters()) + list(D.parameters()):
            fan = p[0].numel() if p.dim() > 1 else 1
            p.copy_(torch.randn(p.shape, generator=gen) * (fan ** -0.5 if p.dim() > 1 else 0.1))
    G, D = G.to(dev), D.to(dev)
    trainer = mg.HotPathTrainer(G, D, tr, mc)
    knows_exact = hasattr(trainer, "exact_shards")
    trainer.bucketG.always_exchange = trainer.bucketD.always_exchange = True
    if knows_exact:
        mg.ShardCounts.always_exchange = True
    rng = np.random.default_rng(1234)
    mel = torch.from_numpy(rng.uniform(-11.5, 2.0, (B, L, M)).astype(np.float32)).to(dev)
    cond = torch.from_numpy(rng.standard_normal((B, L, 256)).astype(np.float32)).to(dev)
    spk = torch.from_numpy(rng.standard_normal((B, 256)).astype(np.float32)).to(dev)
    pad = torch.zeros(B, L, dtype=torch.bool, device=dev)
    h = L // 2
    pad2 = pad.clone()
    pad2[B // 2:, h:] = True                                  # half the items end at L/2
    mel2, cond2 = mel * ~pad2[..., None], cond * ~pad2[..., None]
    mel_s, cond_s, pad_s = mel[:, :h].contiguous(), cond[:, :h].contiguous(), pad[:, :h].contiguous()

    def variant(name):
        if name == "off":
            return False, (mel, cond, spk, pad), {}
        shape = mg.BatchShape(B, L, 1)
        if name == "on":
            return True, (mel, cond, spk, pad), {"shape": shape}
        if name == "on_noshape":
            return True, (mel, cond, spk, pad), {}
        if name == "two_length":
            return True, (mel2, cond2, spk, pad2), {"shape": shape}
        if name == "short_padded":
            return True, (mel_s, cond_s, spk, pad_s), {"shape": shape}
        if name == "short_alone":
            return True, (mel_s, cond_s, spk, pad_s), {"shape": mg.BatchShape(B, h, 1)}
        raise SystemExit("unknown variant %r" % name)

    names = [n for n in args.variants.split(",") if n and (knows_exact or n == "off")]

    def run(name, n):
        exact, tensors, kw = variant(name)
        if knows_exact:
            trainer.exact_shards = exact
        out = None
        for _ in range(n):
            out = trainer.step(*tensors, **kw)
        return out

    for name in names:                                        # every shape warm before anything is timed
        run(name, args.warmup)
    torch.cuda.synchronize()
    trainer.check()
    ms = {n: [] for n in names}
    for _ in range(args.rounds):
        for name in names:                                    # alternate the variants inside one process
            run(name, 1)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = run(name, args.steps)
            t1.record()
            t1.synchronize()
            assert all(torch.isfinite(v).all() for v in out.values()), name
            ms[name].append(t0.elapsed_time(t1) / args.steps)
    trainer.check()
    line = {"tool": "exact_shards_cost", "label": args.label, "tree_knows_exact_shards": knows_exact,
            "shape": {"batch": B, "frames": L, "world": 1, "backend": dist.get_backend(), "always_exchange": True},
            "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "timer": "device events",
            "ms_per_step": {n: [round(v, 3) for v in vals] for n, vals in ms.items()},
            "ms_per_step_median": {n: round(statistics.median(vals), 3) for n, vals in ms.items()},
            "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
