#!/usr/bin/env python3
"""Generate tests/golden/lingenc_*.npz and tests/golden/lingenc_manifest.json by running the REAL reference
LinguisticEncoder (model/linguistic_encoder.py) and MixGANTTS (model/mixgantts.py) on CPU.

Run in the build container only:   python tests/golden/make_golden_lingenc.py
Like make_golden.py it writes data only (inputs, outputs, the state_dict manifests); weights are re-drawn on both sides
by oracle/weights.py.  It has its own manifest and RNG streams, so every other fixture stays byte-identical.

Position encodings are not drawn: they keep the reference's sinusoid initialisation (a draw would scale them to
noise).  The duration predictor's output bias is set to DUR_BIAS after the draw (recorded in the manifest as an
override), so that words last a few frames each, as they do in speech.

Draws are rejected (and the inputs re-drawn) when an integer decision of the reference sits within MARGIN of its
boundary -- a bucketize of a pitch / energy value, the rounding of exp(log_duration) - 1, or the truncation after the
multiplication by d_control -- since a last-bit difference would flip it, or when an utterance gets zero frames.
"""
import copy
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_harness as H  # noqa: E402

H.install_stubs()
import torch  # noqa: E402

torch.set_num_threads(8)

from model.linguistic_encoder import LinguisticEncoder  # noqa: E402
from model.mixgantts import MixGANTTS  # noqa: E402
from utils.tools import get_mask_from_lengths  # noqa: E402

from oracle import weights as WR  # noqa: E402

OUT = HERE
MARGIN = 1e-3
DUR_BIAS = 1.2
SPEC_MIN, SPEC_MAX = np.linspace(-11.5, -9.0, 80), np.linspace(1.0, 2.0, 80)
MANIFEST = {}


def configs(helper_type="dga", max_seq_len=None, T=4):
    pre, mc, tr = H.load_configs("LJSpeech")
    mc["denoiser"]["timesteps"] = T
    mc["denoiser"]["shallow_timesteps"] = T
    mc["multi_speaker"] = False
    if max_seq_len is not None:
        mc["max_seq_len"] = max_seq_len
    tr["aligner"]["helper_type"] = helper_type
    return pre, mc, tr


def seed(mod, seed_, name, cfg, prefix=""):
    """Draw every trainable parameter but the position encodings, then apply the duration-bias override."""
    man = {k: list(p.shape) for k, p in mod.named_parameters() if p.requires_grad and not k.endswith("position_enc")}
    override = {prefix + "duration_predictor.linear_layer.bias": DUR_BIAS}
    pre, mc, tr = cfg
    MANIFEST[name] = {"seeded": man, "seed": seed_, "overrides": override,
                      "state_dict": {k: list(v.shape) for k, v in mod.state_dict().items()},
                      "state_dict_order": list(mod.state_dict().keys()),
                      "configs": [pre, mc, tr]}
    w = WR.draw(man, seed_)
    sd = mod.state_dict()
    with torch.no_grad():
        for k, a in w.items():
            sd[k].copy_(torch.from_numpy(a))
        for k, v in override.items():
            sd[k].fill_(v)
    return WR.checksum(w)


def batch(rng, words):
    """words: per utterance, the list of phonemes per word (None: draw 1..4 per word for that many words)."""
    wbs = [list(w) if isinstance(w, (list, tuple)) else list(rng.integers(1, 5, int(w))) for w in words]
    B, Tw = len(wbs), max(len(w) for w in wbs)
    src_lens = torch.tensor([sum(w) for w in wbs])
    Tp = int(src_lens.max())
    wb = torch.zeros(B, Tw, dtype=torch.long)
    texts = torch.zeros(B, Tp, dtype=torch.long)
    for b, w in enumerate(wbs):
        wb[b, :len(w)] = torch.tensor(w)
        texts[b, :sum(w)] = torch.from_numpy(rng.integers(1, 361, sum(w)))
    src_w_lens = torch.tensor([len(w) for w in wbs])
    return texts, src_lens, wb, src_w_lens


def near_bins(v, bins):
    return bool((v.reshape(-1, 1) - bins.reshape(1, -1)).abs().min() < MARGIN)


def decisions_ok(out, enc, d_control, targets):
    """False when an integer decision is within MARGIN of its boundary, or an utterance has no frames."""
    p, e, logw, mel_len = out[1], out[2], out[3], out[5]
    if int(mel_len.min()) <= 0:
        return False
    if near_bins(targets[0] if targets[0] is not None else p, enc.pitch_bins.detach()):
        return False
    if near_bins(targets[1] if targets[1] is not None else e, enc.energy_bins.detach()):
        return False
    if targets[2] is None:
        fin = torch.isfinite(logw)
        v = torch.exp(logw[fin]) - 1
        if ((v - v.floor() - 0.5).abs() < MARGIN).any():
            return False
        if d_control != round(d_control):      # an integer d_control keeps rint(.) * d_control integral
            r = torch.round(v) * d_control
            r = r[r > 0]
            if ((r - r.round()).abs() < MARGIN).any():
                return False
    return True


def record(arrs, out, rec):
    for i, o in enumerate(out):
        if isinstance(o, (list, tuple)):
            for j, oo in enumerate(o):
                arrs["out%d/%d" % (i, j)] = oo
        else:
            arrs["out%d" % i] = o
    arrs["enc_p_out"] = rec["enc_p_out"]
    arrs["enc_w_out"] = rec["enc_w_out"]


def hooks(enc, rec):
    def p_hook(mod, inp):                 # the duration predictor reads the final enc_p_out (:355-357)
        rec["enc_p_out"] = inp[0].detach().clone()

    def w_hook(mod, inp, out):
        rec["enc_w_out"] = out.detach().transpose(1, 2).clone()
    return [enc.duration_predictor.register_forward_pre_hook(p_hook), enc.word_encoder.register_forward_hook(w_hook)]


def save(name, arrs):
    clean = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **clean)
    print("  wrote %-32s %8.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


def encoder_case(name, rng, seed_, words, helper="dga", max_seq_len=None, teacher=False, p_control=1.0,
                 d_control=1.0):
    stats = H.make_stats_dir(SPEC_MIN, SPEC_MAX)
    cfg = configs(helper, max_seq_len)
    pre, mc, tr = copy.deepcopy(cfg)
    pre["path"]["preprocessed_path"] = stats
    torch.manual_seed(seed_)
    enc = LinguisticEncoder(pre, mc, tr)
    cfg[0]["path"]["preprocessed_path"] = None
    ck = seed(enc, seed_, name, cfg)
    enc.eval()
    for attempt in range(5000):
        texts, src_lens, wb, src_w_lens = batch(rng, words)
        B, Tp = texts.shape
        src_mask = get_mask_from_lengths(src_lens, Tp)
        src_w_mask = get_mask_from_lengths(src_w_lens, int(src_w_lens.max()))
        mel_mask = max_len = prior = pt = et = dt = None
        if teacher:
            dt = torch.from_numpy(rng.integers(1, 6, (B, Tp))) * src_mask
            pt = torch.from_numpy(rng.standard_normal((B, Tp)).astype(np.float32) * 2 + 1) * src_mask
            et = torch.from_numpy(rng.standard_normal((B, Tp)).astype(np.float32) * 2 + 1) * src_mask
            mel_lens = dt.sum(1)
            max_len = int(mel_lens.max())     # get_rel_coef pads to the longest expansion (:222-236): no wider
            mel_mask = get_mask_from_lengths(mel_lens, max_len)
            if helper == "ctc":
                prior = torch.from_numpy(rng.uniform(0.01, 1.0, (B, Tp, max_len)).astype(np.float32))
        rec = {}
        hs = hooks(enc, rec)
        with torch.no_grad():
            out = enc(texts, src_lens, wb, src_mask, src_w_lens, src_w_mask, mel_mask, max_len, prior, pt, et, dt,
                      p_control, d_control)
        for h in hs:
            h.remove()
        if decisions_ok(out, enc, d_control, (pt, et, dt)):
            break
    else:
        raise RuntimeError(name + ": no draw clear of the integer boundaries")
    arrs = dict(wsum=ck, texts=texts, src_lens=src_lens, wb=wb, src_w_lens=src_w_lens, src_mask=src_mask,
                src_w_mask=src_w_mask, p_control=np.float64(p_control), d_control=np.float64(d_control),
                attempts=np.int64(attempt + 1))
    for k, v in (("mel_mask", mel_mask), ("max_len", max_len), ("attn_prior", prior), ("pitch_target", pt),
                 ("energy_target", et), ("duration_target", dt)):
        if v is not None:
            arrs[k] = v
    record(arrs, out, rec)
    print(" ", name, "attempts", attempt + 1, "mel_len", out[5].tolist())
    save(name, arrs)


class Tape:
    """Deterministic stand-in for torch.randn inside the reference's diffusion (the draws are recorded)."""

    def __init__(self, rng):
        self.rng, self.log = rng, []

    def randn(self, *shape, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        a = torch.from_numpy(self.rng.standard_normal(shape).astype(np.float32))
        self.log.append(a.numpy().copy())
        return a

    def randn_like(self, x, **kw):
        return self.randn(tuple(x.shape))


def model_case(name, rng, seed_, words, d_control):
    """MixGANTTS naive inference, T=4, with the REAL encoder seeded too and the diffusion's noise taped."""
    stats = H.make_stats_dir(SPEC_MIN, SPEC_MAX)
    cfg = configs("dga")
    pre, mc, tr = copy.deepcopy(cfg)
    pre["path"]["preprocessed_path"] = stats
    torch.manual_seed(seed_)
    m = MixGANTTS(types.SimpleNamespace(model="naive"), pre, mc, tr)
    cfg[0]["path"]["preprocessed_path"] = None
    ck = seed(m, seed_, name, cfg, prefix="linguistic_encoder.")
    m.eval()
    enc = m.linguistic_encoder
    for attempt in range(5000):
        texts, src_lens, wb, src_w_lens = batch(rng, words)
        B, Tp = texts.shape
        rec, enc_out = {}, {}
        hs = hooks(enc, rec)
        hs.append(enc.register_forward_hook(lambda mod, inp, o: enc_out.__setitem__("o", o)))
        tape = Tape(np.random.default_rng(int(rng.integers(1 << 30))))
        saved = torch.randn, torch.randn_like
        torch.randn, torch.randn_like = tape.randn, tape.randn_like
        try:
            with torch.no_grad():
                out, p_targets, coarse = m(torch.zeros(B, dtype=torch.long), texts, src_lens, Tp, wb, src_w_lens,
                                           int(src_w_lens.max()), d_control=d_control)
        finally:
            torch.randn, torch.randn_like = saved
        for h in hs:
            h.remove()
        if decisions_ok(enc_out["o"], enc, d_control, (None, None, None)):
            break
    else:
        raise RuntimeError(name + ": no draw clear of the integer boundaries")
    arrs = dict(wsum=ck, texts=texts, src_lens=src_lens, wb=wb, src_w_lens=src_w_lens, d_control=np.float64(d_control),
                spec_min=SPEC_MIN, spec_max=SPEC_MAX, mel=out[0], attempts=np.int64(attempt + 1))
    record(arrs, enc_out["o"], rec)
    for i, a in enumerate(tape.log):
        arrs["rng%d" % i] = a
    print(" ", name, "attempts", attempt + 1, "mel_len", enc_out["o"][5].tolist())
    save(name, arrs)


def main():
    rng = np.random.default_rng(20261015)
    # 1: inference, ragged; utterance 1 is shorter than window + 1 phonemes, utterance 2 is a single word
    encoder_case("lingenc_infer", rng, 71, [9, [2, 1], [4]], p_control=1.2, d_control=1.3)
    # 2: teacher-forced (pitch, energy and duration targets; max_len past the shorter utterances' summed durations)
    encoder_case("lingenc_teacher", rng, 72, [8, 5, [3]], teacher=True)
    # 3: helper_type "ctc" with an attn_prior
    encoder_case("lingenc_ctc", rng, 73, [7, 4], helper="ctc", teacher=True)
    # 4: max_seq_len 24 with phoneme and frame lengths above it (fresh sinusoid tables in eval)
    encoder_case("lingenc_long", rng, 74, [[3, 4, 2, 4, 3, 4, 3, 4, 3], [4, 3, 4, 4, 3, 4, 4]], max_seq_len=24)
    # 5: the whole model from phoneme ids, naive T=4
    model_case("lingenc_mixgantts_naive", rng, 75, [6, 4], d_control=1.0)
    with open(os.path.join(OUT, "lingenc_manifest.json"), "w") as f:
        json.dump(MANIFEST, f, indent=0, sort_keys=True)
    print("wrote lingenc_manifest.json")


if __name__ == "__main__":
    main()
