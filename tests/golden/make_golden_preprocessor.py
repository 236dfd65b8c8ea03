#!/usr/bin/env python3
"""Generate tests/golden/preprocessor.npz and tests/golden/preprocessor_manifest.json by running the REAL reference
Preprocessor (preprocessor/preprocessor.py) on the CPU over the synthetic corpus of tests/preprocessor_corpus.py.

Run in the build container only:   python tests/golden/make_golden_preprocessor.py
It writes data only: every array the reference writes per utterance, its stats.json, the text of train / val /
filtered_out, and beta_binomial_prior_distribution tables.  Three runs over the same corpus:
  main  -- phoneme_level features, normalised (the tree the end-to-end test compares against);
  raw   -- phoneme_level, normalisation off: the averaged values before (x - mean) / std;
  frame -- frame_level, normalisation off: the reference's own frame-level energy and pitch.

Stubs, installed before the reference is imported (none of these packages is installed):
  tgt.io.read_textgrid  objects built from the recipe's non-empty intervals, the ones the TextGrid files hold;
  librosa.load          the recipe's seeded signal; librosa.util / librosa.filters as make_golden_audio.py;
  pyworld dio/stonemask the recipe's seeded f0 track.
os.listdir is sorted during the runs (the reference takes the file system's order), and torch.Tensor.cuda is the
identity (its STFT calls .cuda() unconditionally).
"""
import json
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_audio as MGA  # noqa: E402  (installs the import stubs of ref_harness)
import preprocessor_corpus as C  # noqa: E402
import torch  # noqa: E402


class _Interval:
    def __init__(self, s, e, text):
        self.start_time, self.end_time, self.text = s, e, text


class _Tier:
    def __init__(self, ivs):
        self._objects = [_Interval(*iv) for iv in ivs if iv[2] != ""]


class _TextGrid:
    def __init__(self, u):
        self._tiers = {"phones": _Tier(u[3]), "words": _Tier(u[4])}

    def get_tier_by_name(self, name):
        return self._tiers[name]


def install_corpus_stubs():
    MGA.install_librosa_stubs()
    sys.modules["librosa"].load = lambda path, *a, **k: (C.load_wav(path), C.SR)
    tgt, io = types.ModuleType("tgt"), types.ModuleType("tgt.io")
    io.read_textgrid = lambda path, *a, **k: _TextGrid(C.UTTERANCES[C.NAMES.index(os.path.basename(path).split(".")[0])])
    tgt.io = io
    sys.modules["tgt"], sys.modules["tgt.io"] = tgt, io
    pw = types.ModuleType("pyworld")
    pw.dio = lambda wav, sr, frame_period=5.0: (C.pitch_fn(wav, sr, frame_period), None)
    pw.stonemask = lambda wav, f0, t, sr: f0
    sys.modules["pyworld"] = pw


def run(Preprocessor, feature, normalization):
    """One reference run in a fresh temporary tree: {kind/name: array}, stats, the three texts, speakers, return."""
    with tempfile.TemporaryDirectory() as root:
        raw, pre = C.write_corpus(root)
        random.seed(C.SHUFFLE_SEED)
        ret = Preprocessor(*C.configs(raw, pre, feature, normalization)).build_from_path()
        arrays = {}
        for kind in C.KINDS:
            for fn in sorted(os.listdir(os.path.join(pre, kind))):
                spk, k, name = fn[:-4].split("-")
                assert k == kind and C.SPEAKER_OF[name] == spk
                arrays["%s/%s" % (kind, name)] = np.ascontiguousarray(np.load(os.path.join(pre, kind, fn)))
        texts = {n: open(os.path.join(pre, n + ".txt"), encoding="utf-8").read() for n in ("train", "val", "filtered_out")}
        stats = json.load(open(os.path.join(pre, "stats.json")))
        speakers = json.load(open(os.path.join(pre, "speakers.json")))
    return arrays, stats, texts, speakers, ret


def main():
    install_corpus_stubs()
    listdir, cuda = os.listdir, torch.Tensor.cuda
    os.listdir = lambda p=".": sorted(listdir(p))
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        from preprocessor.preprocessor import Preprocessor
        out, man = {}, {"names": C.NAMES, "filtered": C.FILTERED}
        for tag, feature, norm in (("main", "phoneme_level", True), ("raw", "phoneme_level", False),
                                   ("frame", "frame_level", False)):
            arrays, stats, texts, speakers, ret = run(Preprocessor, feature, norm)
            for k, v in arrays.items():
                if tag == "main" or k.split("/")[0] in ("pitch", "energy"):
                    out["%s/%s" % (tag, k)] = v
            man[tag] = {"stats": stats, "texts": texts, "speakers": speakers, "returned": ret,
                        "dtypes": {k: str(v.dtype) for k, v in arrays.items()}}
        kept = [n for n in C.NAMES if n not in C.FILTERED]
        assert sorted(k.split("/")[2] for k in out if k.startswith("main/mel/")) == sorted(kept)
        assert man["main"]["texts"]["filtered_out"].split() == C.FILTERED

        # the yardstick of mean / std: two passes in float64 over all kept values; the reference's incremental
        # StandardScaler must lie within 1e-12 relative of it
        two_pass = {}
        for kind in ("pitch", "energy"):
            vals = np.concatenate([Preprocessor.remove_outlier(None, out["raw/%s/%s" % (kind, n)]).astype(np.float64)
                                   for n in kept])
            mean = vals.sum() / vals.size
            std = np.sqrt(((vals - mean) ** 2).sum() / vals.size)
            ref_mean, ref_std = man["main"]["stats"][kind][2:4]
            assert abs(ref_mean - mean) <= 1e-12 * abs(mean) and abs(ref_std - std) <= 1e-12 * std, (kind, ref_mean, mean)
            two_pass[kind] = [float(mean), float(std), int(vals.size)]
        man["two_pass"] = two_pass

        # get_alignment on its own (before the word subdivision), for the TextGrid reader + alignment test
        me = types.SimpleNamespace(sampling_rate=C.SR, hop_length=C.HOP)
        man["alignment"] = {}
        for u in C.UTTERANCES:
            tg = _TextGrid(u)
            phones, durations, start, end, ppw = Preprocessor.get_alignment(me, tg.get_tier_by_name("phones"),
                                                                            tg.get_tier_by_name("words"))
            man["alignment"][u[0]] = {"phones": phones, "durations": [int(d) for d in durations], "start": start,
                                      "end": end, "phones_per_word": [int(x) for x in ppw]}

        for mel_len, n_phon, s in C.PRIOR_CASES:
            table = Preprocessor.beta_binomial_prior_distribution(None, mel_len, n_phon, s)
            assert table.shape == (n_phon, mel_len) and table.dtype == np.float64
            rows, cols = C.prior_subgrid(mel_len, n_phon)
            out["prior/%d_%d_%g" % (mel_len, n_phon, s)] = np.ascontiguousarray(table[np.ix_(rows, cols)])
    finally:
        os.listdir, torch.Tensor.cuda = listdir, cuda

    np.savez_compressed(os.path.join(HERE, "preprocessor.npz"), **out)
    with open(os.path.join(HERE, "preprocessor_manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    print("preprocessor.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(HERE, "preprocessor.npz"))))


if __name__ == "__main__":
    main()
