#!/usr/bin/env python3
"""Native LinguisticEncoder timing (profiles/*_lingenc_bench.jsonl).

  python tools/lingenc_bench.py [--iters N]

Inference forward (phoneme ids -> the nine outputs, including its one host sync for the frame count) at B=1 and
B=16, ~120 phonemes and ~1000 frames per utterance, timed with device events around each call; the same forward as
stock PyTorch-ROCm eager (the plain-torch restatement tests/lingenc_torch.py on the same GPU), alternated call by
call with the native one; and text -> wav: phoneme ids -> native encoder -> naive T=4 diffusion -> HiFi-GAN (or, with
--vocoder melgan, the native MelGAN).
The configs are the LJSpeech ones recorded in tests/golden/lingenc_manifest.json; weights are the modules' own
initialisation (torch seed 0) with the duration predictor's bias set so that a phoneme lasts ~9 frames.  For launch counts run it under `rocprofv3 --kernel-trace --stats -- python
tools/lingenc_bench.py --iters 3`.
"""
import argparse
import json
import os
import sys
import tempfile
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mixgan_tts_amd as mg  # noqa: E402
import lingenc_torch as LT  # noqa: E402

# HiFi-GAN V1 (hifigan/config_v1.json)
HIFIGAN_V1 = {"upsample_rates": (8, 8, 2, 2), "upsample_kernel_sizes": (16, 16, 4, 4), "upsample_initial_channel": 512,
              "resblock_kernel_sizes": (3, 7, 11), "resblock_dilation_sizes": ((1, 3, 5), (1, 3, 5), (1, 3, 5))}


def configs(name, tmp):
    with open(os.path.join(ROOT, "tests", "golden", "lingenc_manifest.json")) as f:
        pre, mc, tr = json.load(f)[name]["configs"]
    with open(os.path.join(tmp, "stats.json"), "w") as f:
        json.dump({"pitch": [-2.0, 8.0, 0.0, 1.0], "energy": [-1.5, 7.0, 0.0, 1.0],
                   "spec_min": [-11.5] * 80, "spec_max": [2.0] * 80}, f)
    pre["path"]["preprocessed_path"] = tmp
    return pre, mc, tr

DUR_BIAS = 2.2


def batch(B, n_ph, gen, dev):
    wbs = []
    for _ in range(B):
        w = []
        while sum(w) < n_ph:
            w.append(min(int(torch.randint(1, 5, (1,), generator=gen)), n_ph - sum(w)))
        wbs.append(w)
    Tw = max(len(w) for w in wbs)
    wb = torch.zeros(B, Tw, dtype=torch.long)
    for b, w in enumerate(wbs):
        wb[b, :len(w)] = torch.tensor(w)
    src_lens = torch.full((B,), n_ph)
    src_w_lens = torch.tensor([len(w) for w in wbs])
    texts = torch.randint(1, 361, (B, n_ph), generator=gen)
    src_mask = torch.ones(B, n_ph, dtype=torch.bool)
    src_w_mask = torch.arange(Tw)[None] < src_w_lens[:, None]
    return [t.to(dev) for t in (texts, src_lens, wb, src_mask, src_w_lens, src_w_mask)]


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--vocoder", choices=("hifigan", "melgan"), default="hifigan",
                    help="vocoder of the text -> wav rows (melgan: the native MelGAN, fused residual stacks)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp()
    cfg = configs("lingenc_infer", tmp)
    torch.manual_seed(0)
    enc = mg.LinguisticEncoder(*cfg)
    with torch.no_grad():
        enc.duration_predictor.linear_layer.bias.fill_(DUR_BIAS)
    enc = enc.to(dev).eval()
    sd = {k: v.detach() for k, v in enc.state_dict().items()}
    gen = torch.Generator().manual_seed(0)
    for B in (1, 16):
        inp = batch(B, 120, gen, dev)
        with torch.no_grad():
            frames = enc(*inp)[5]
            native = lambda: enc(*inp)  # noqa: E731
            eager = lambda: LT.encoder_forward(sd, cfg, *inp)  # noqa: E731
            for _ in range(3):
                native(), eager()
            tn, te = [], []
            for _ in range(args.iters):       # alternated, call by call
                tn.append(timed(native, 1))
                te.append(timed(eager, 1))
        med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
        print(json.dumps({"config": "LinguisticEncoder inference B=%d, 120 phonemes" % B,
                          "frames_mean": round(float(frames.float().mean()), 1), "frames_max": int(frames.max()),
                          "native_ms": round(med(tn), 3), "eager_ms": round(med(te), 3),
                          "speedup": round(med(te) / med(tn), 1), "iters": args.iters}), flush=True)

    # text -> wav: phoneme ids -> native encoder -> naive T=4 -> HiFi-GAN -> int16
    pre, mc, tr = configs("lingenc_mixgantts_naive", tmp)
    torch.manual_seed(0)
    m = mg.MixGANTTS(types.SimpleNamespace(model="naive"), pre, mc, tr, linguistic_encoder="native")
    with torch.no_grad():
        m.linguistic_encoder.duration_predictor.linear_layer.bias.fill_(DUR_BIAS)
    m = m.to(dev).eval()
    if args.vocoder == "melgan":
        voc = mg.MelVocoder().to(dev).eval()
        vmc = {"vocoder": {"model": "MelGAN", "speaker": "LJSpeech"}}
    else:
        voc = mg.vocoder.Generator(types.SimpleNamespace(**HIFIGAN_V1)).to(dev).eval()
        voc.remove_weight_norm()
        vmc = {"vocoder": {"model": "HiFi-GAN", "speaker": "LJSpeech"}}
    vpre = {"preprocessing": {"audio": {"max_wav_value": 32768.0}}}
    for B in (1, 16):
        texts, src_lens, wb, _, src_w_lens, _ = batch(B, 120, gen, dev)
        spk = torch.zeros(B, dtype=torch.long, device=dev)

        def run():
            with torch.no_grad():
                out = m(spk, texts, src_lens, 120, wb, src_w_lens, int(src_w_lens.max()))[0]
                return out[0], out[11], mg.vocoder.vocoder_infer(out[0].transpose(1, 2).contiguous(), voc, vmc, vpre)
        for _ in range(2):
            run()
        t = timed(run, max(5, args.iters // 4))
        mel, mel_len, _ = run()
        audio = float(mel_len.sum()) * 256 / 22050.0
        print(json.dumps({"config": "e2e phoneme ids -> native encoder -> mel (T=4) -> wav, B=%d, 120 phonemes" % B,
                          "vocoder": vmc["vocoder"]["model"],
                          "frames_max": int(mel.shape[1]), "ms": round(t, 2), "audio_s": round(audio, 1),
                          "real_time_factor": round(t / 1e3 / audio, 5)}), flush=True)


if __name__ == "__main__":
    main()
