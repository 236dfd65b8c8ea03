"""CPU-side checks of the corpus builder: the C ABI of csrc/corpus.hip, the TextGrid reader and the alignment
restatement, outlier removal / statistics / normalisation, the split and sort logic and the loader's attn_prior="device"
mode, against the reference run recorded by tests/golden/make_golden_preprocessor.py.  No kernel is launched."""
import ctypes
import json
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

import preprocessor_corpus as C
from helpers import golden as load_golden, GOLDEN

import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib, data as D, preprocessor as P

KEPT = [n for n in C.NAMES if n not in C.FILTERED]


@pytest.fixture(scope="module")
def golden():
    return load_golden("preprocessor")


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "preprocessor_manifest.json")) as f:
        return json.load(f)


def test_abi_exports_and_argument_checks():
    assert {"mg_betabinom_prior", "mg_phoneme_average"} <= set(_lib.EXPORTS)
    L = mg.lib()
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below returns before a launch
    s, zero = ctypes.c_double(1.0), ctypes.c_double(0.0)
    assert L.mg_betabinom_prior(None, None, None, None, 1, 4, 8, 0, None) == _lib.MG_ERR_ARG
    assert L.mg_betabinom_prior(fake, fake, None, fake, 1, 4, 8, 0, None) == _lib.MG_ERR_ARG
    assert L.mg_betabinom_prior(fake, fake, ctypes.byref(s), fake, 1, 4, 8, 2, None) == _lib.MG_ERR_ARG
    assert L.mg_betabinom_prior(fake, fake, ctypes.byref(zero), fake, 1, 4, 8, 0, None) == _lib.MG_ERR_ARG
    for B, T, Lf in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (1 << 20, 1 << 12, 8)):
        assert L.mg_betabinom_prior(fake, fake, ctypes.byref(s), fake, B, T, Lf, 0, None) == _lib.MG_ERR_SHAPE
    assert L.mg_phoneme_average(None, None, None, None, None, 1, 4, 8, 0, None) == _lib.MG_ERR_ARG
    assert L.mg_phoneme_average(fake, fake, fake, fake, fake, 1, 4, 8, 2, None) == _lib.MG_ERR_ARG
    for B, T, Lf in ((0, 4, 8), (1, 0, 8), (1, 2049, 8), (1, 4, 0), (1, 4, 4097)):
        assert L.mg_phoneme_average(fake, fake, fake, fake, fake, B, T, Lf, 1, None) == _lib.MG_ERR_SHAPE


def test_wrappers_have_no_cpu_path():
    lens = torch.tensor([3], dtype=torch.int32)
    with pytest.raises(mg.MixganHipError):
        mg.attn_prior(lens, lens, 3, 3)
    with pytest.raises(mg.MixganHipError):
        mg.phoneme_average(torch.zeros(1, 8, dtype=torch.float64), torch.ones(1, 2, dtype=torch.int32), lens, lens, "pitch")
    with pytest.raises(mg.MixganHipError):
        mg.phoneme_average(torch.zeros(1, 8), torch.ones(1, 2, dtype=torch.int32), lens, lens, "loudness")


def test_textgrid_reader_and_alignment_match_reference(manifest, tmp_path):
    raw, pre = C.write_corpus(str(tmp_path))
    for u in C.UTTERANCES:
        name, spk = u[0], u[1]
        path = os.path.join(pre, "TextGrid", spk, name + ".TextGrid")
        tiers = P.read_textgrid(path)
        assert list(tiers) == ["words", "phones"]
        assert tiers["phones"] == [iv for iv in u[3] if iv[2] != ""] and tiers["words"] == [iv for iv in u[4] if iv[2] != ""]
        assert P.read_textgrid(path, include_empty_intervals=True)["words"] == u[4]
        ref = manifest["alignment"][name]
        phones, durations, start, end, ppw = P.get_alignment(tiers["phones"], tiers["words"], C.SR, C.HOP)
        assert phones == ref["phones"] and durations == ref["durations"] and ppw == ref["phones_per_word"]
        assert start == ref["start"] and end == ref["end"]
    assert manifest["alignment"][C.ALIASED]["durations"][:2] == [0, 0]
    assert P.word_level_subdivision([9, 2, 7, 14, 15], 7) == [7, 2, 2, 7, 7, 7, 7, 7, 1]
    bad = tmp_path / "short.TextGrid"
    bad.write_text('File type = "ooTextFile short"\n"TextGrid"\n0\n1\n')
    with pytest.raises(P.TextGridError):
        P.read_textgrid(str(bad))


def test_textgrid_reader_takes_quotes_and_other_tiers(tmp_path):
    p = tmp_path / "q.TextGrid"
    p.write_text('﻿File type = "ooTextFile"\nObject class = "TextGrid"\n\nxmin = 0\nxmax = 1\ntiers? <exists>\n'
                 'size = 2\nitem []:\n    item [1]:\n        class = "TextTier"\n        name = "marks"\n        xmin = 0\n'
                 '        xmax = 1\n        points: size = 1\n        points [1]:\n            number = 0.5\n'
                 '            mark = "x"\n    item [2]:\n        class = "IntervalTier"\n        name = "words"\n'
                 '        xmin = 0\n        xmax = 1\n        intervals: size = 2\n        intervals [1]:\n'
                 '            xmin = 0\n            xmax = 0.5\n            text = "say ""hi"" = now"\n'
                 '        intervals [2]:\n            xmin = 0.5\n            xmax = 1\n            text = ""\n',
                 encoding="utf-8")
    assert P.read_textgrid(str(p)) == {"words": [(0.0, 0.5, 'say "hi" = now')]}


def test_builder_prepares_utterances_as_the_reference(golden, manifest, tmp_path):
    """The host stage (no GPU): trimmed wav, f0 cut to the frame count, the filter, the word subdivision and the info
    line, against the reference's files and metadata."""
    raw, pre = C.write_corpus(str(tmp_path))
    b = P.Preprocessor(*C.configs(raw, pre), pitch_fn=C.pitch_fn, load_wav=C.load_wav)
    lines = {ln.split("|")[0]: ln for ln in (manifest["main"]["texts"]["train"] + manifest["main"]["texts"]["val"]).split("\n")}
    for n in C.NAMES:
        item = b.prepare_utterance(C.SPEAKER_OF[n], n)
        if n in C.FILTERED:
            assert item is None
            continue
        assert np.array_equal(item["duration"], golden["main/duration/" + n])
        assert np.array_equal(item["phones_per_word"], golden["main/phones_per_word/" + n])
        assert "|".join([n, item["speaker"], item["text"], item["raw_text"]]) == lines[n]
        assert item["wav"].dtype == np.float32 and item["pitch"].dtype == np.float64
        assert np.array_equal(item["pitch"], golden["frame/pitch/" + n])
    assert max(golden["main/phones_per_word/b02"]) == C.MAX_PHONEME_NUM and len(manifest["alignment"]["b02"]["phones_per_word"]) == 2


def test_outliers_statistics_and_normalisation_match_reference(golden, manifest, tmp_path):
    """mean / std: the yardstick is the two-pass float64 value over all kept values (the golden maker holds the
    reference's incremental StandardScaler within 1e-12 of it); 1e-10 is allowed.  Normalised values and their
    extremes then move by at most 1e-10 (|mean| / std + |z|) < 1e-9."""
    st = manifest["main"]["stats"]
    for kind in ("pitch", "energy"):
        moments, n_kept = P.RunningMoments(), 0
        d = tmp_path / kind
        d.mkdir()
        for k, n in enumerate(KEPT):
            raw = golden["raw/%s/%s" % (kind, n)]
            kept = P.remove_outlier(raw)
            p25, p75 = np.percentile(raw, 25), np.percentile(raw, 75)
            inside = (raw > p25 - 1.5 * (p75 - p25)) & (raw < p75 + 1.5 * (p75 - p25))
            assert kept.dtype == raw.dtype and np.array_equal(kept, raw[inside])
            moments.update(kept)
            n_kept += len(kept)
            np.save(str(d / ("%s-%s-%s.npy" % (C.SPEAKER_OF[n], kind, n))), raw)
        mean2, std2, count = manifest["two_pass"][kind]
        assert n_kept == count == moments.n
        for got, want in ((moments.mean, mean2), (moments.std, std2), (moments.mean, st[kind][2]), (moments.std, st[kind][3])):
            assert abs(got - want) <= 1e-10 * abs(want), (kind, got, want)
        lo, hi = P.normalize(str(d), moments.mean, moments.std)
        assert abs(lo - st[kind][0]) <= 1e-9 and abs(hi - st[kind][1]) <= 1e-9
        for n in KEPT:
            got = np.load(str(d / ("%s-%s-%s.npy" % (C.SPEAKER_OF[n], kind, n))))
            ref = golden["main/%s/%s" % (kind, n)]
            assert got.dtype == ref.dtype == np.float64 and np.abs(got - ref).max() <= 1e-9
    one = P.RunningMoments()
    one.update(np.full(5, 3.0))
    assert one.std == 1.0 and one.mean == 3.0          # a constant feature scales by 1, as StandardScaler does
    with pytest.raises(ValueError):
        P.RunningMoments().std


def test_split_and_sort_under_a_fixed_seed(golden, manifest):
    texts = manifest["main"]["texts"]
    lines = {ln.split("|")[0]: ln for ln in (texts["train"] + texts["val"]).split("\n") if ln}
    frames = {n: golden["main/mel/" + n].shape[0] for n in KEPT}
    out = [lines[n] for n in sorted(KEPT)]          # the order the builder meets them in
    random.seed(C.SHUFFLE_SEED)
    train, val = P.split_metadata(out, [], [], None, C.VAL_SIZE, True, frames)
    assert out == manifest["main"]["returned"]
    assert "".join(m + "\n" for m in train) == texts["train"] and "".join(m + "\n" for m in val) == texts["val"]
    assert [frames[m.split("|")[0]] for m in train] == sorted(frames[m.split("|")[0]] for m in train)
    # a pre-defined validation set: only the training lines are shuffled, `out` stays empty
    random.seed(C.SHUFFLE_SEED)
    tr, va = P.split_metadata([], [lines[n] for n in KEPT[:4]], [lines[n] for n in KEPT[4:]], KEPT[4:], 0, False, frames)
    assert sorted(tr) == sorted(lines[n] for n in KEPT[:4]) and va == [lines[n] for n in KEPT[4:]]


def test_default_loaders(tmp_path, monkeypatch):
    from scipy.io import wavfile
    x = (np.array([0, 16384, -32768, 32767], dtype=np.int16))
    wavfile.write(str(tmp_path / "a.wav"), C.SR, x)
    got = P.scipy_load_wav(C.SR)(str(tmp_path / "a.wav"))
    assert got.dtype == np.float32 and np.array_equal(got, x.astype(np.float32) / 32768.0)
    with pytest.raises(P.SamplingRateMismatch):
        P.scipy_load_wav(16000)(str(tmp_path / "a.wav"))
    monkeypatch.setitem(sys.modules, "pyworld", None)          # import pyworld -> ImportError
    with pytest.raises(mg.PitchExtractorRequired, match="pitch_fn"):
        P.pyworld_pitch(np.zeros(2048), C.SR, C.HOP / C.SR * 1000)


def test_dataset_device_prior_opens_no_prior_file(golden, manifest, tmp_path):
    pre = str(tmp_path)
    for kind in ("mel", "pitch", "energy", "duration", "phones_per_word"):          # no attn_prior folder
        os.makedirs(os.path.join(pre, kind))
        for n in KEPT:
            np.save(os.path.join(pre, kind, "%s-%s-%s.npy" % (C.SPEAKER_OF[n], kind, n)), golden["main/%s/%s" % (kind, n)])
    with open(os.path.join(pre, "speakers.json"), "w") as f:
        json.dump(manifest["main"]["speakers"], f)
    with open(os.path.join(pre, "train.txt"), "w", encoding="utf-8") as f:
        f.write(manifest["main"]["texts"]["train"])
    pc, mc, tc = C.configs(os.path.join(pre, "raw"), pre)
    t2s = lambda text, cleaners: [1 + len(p) for p in text.strip("{}").split()]  # noqa: E731
    args = types.SimpleNamespace(model="naive")
    ds = D.Dataset("train.txt", args, pc, mc, tc, text_to_sequence=t2s, attn_prior="device")
    assert ds.prior_scaling == 1.0
    items = [ds[i] for i in range(len(ds))]
    assert all(it["attn_prior"] is None for it in items)
    (batch,) = ds.collate_fn(items)
    assert len(batch) == 17 and batch[D.PRIOR_SLOT] is None
    assert batch[D.MAX_TEXT_SLOT] == max(batch[D.TEXT_LENS_SLOT]) and batch[D.MAX_MEL_SLOT] == max(batch[D.MEL_LENS_SLOT])
    with pytest.raises(ValueError, match="prior_scaling"):
        D.to_device(batch, torch.device("cpu"))
    with pytest.raises(mg.MixganHipError):          # the prior is computed by the HIP kernel only
        D.to_device(batch, torch.device("cpu"), prior_scaling=ds.prior_scaling)
    # the default mode needs the files, and a configuration without the aligner entry still loads in it
    with pytest.raises(FileNotFoundError):
        D.Dataset("train.txt", args, pc, mc, tc, text_to_sequence=t2s)[0]
    del pc["preprocessing"]["aligner"]
    assert D.Dataset("train.txt", args, pc, mc, tc, text_to_sequence=t2s).attn_prior == "disk"
    with pytest.raises(ValueError):
        D.Dataset("train.txt", args, pc, mc, tc, text_to_sequence=t2s, attn_prior="gpu")
