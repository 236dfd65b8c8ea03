"""GPU checks of csrc/resample.hip through audio.resample / audio.peak_normalize_int16, of prepare_align.py end to end
and of the corpus builder's resampling loader, against the float64 direct form of tests/resample_oracle.py.

Tolerance, derived and not measured: for every output sample with K contributing taps,
    |y - y64| <= (K + 3) 2^-24 sum_k |up h x|,
the bound of a float32 dot product of K terms in any order plus the rounding of taps, input and result.  Each test
prints its worst ratio to the bound.  The copy path (equal rates) is bit exact; where prepare_align's int16 is held to
the float64 value, a copied sample counts as one term (K = 1, sum = |x|), which covers the normalisation's division
and multiplication."""
import os

import numpy as np
import pytest
import torch

import resample_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TARGET = 22050


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def _lengths(up, down, tile):
    t1, t2 = -(-tile * down // up), -(-2 * tile * down // up)      # input samples of one and two output tiles
    return [1, 2, 63, t1 - 1, t1, t1 + 1, t2 - 1, t2, t2 + 1, 1237, 5000]


def _batch(lens, seed):
    rng = np.random.default_rng(seed)
    x = np.full((len(lens), max(lens) + 5), np.nan, dtype=np.float32)      # padding poisoned with NaN
    for b, n in enumerate(lens):
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
    return x


def _check(y, out_lens, x, lens, up, down, tag):
    h = O.ref_filter(up, down)
    assert out_lens.dtype == torch.int32 and out_lens.tolist() == [O.out_len(n, up, down) for n in lens]
    assert y.shape == (len(lens), max(out_lens.tolist())) and y.dtype == np.float32
    assert np.isfinite(y).all()
    worst = 0.0
    for b, n in enumerate(lens):
        ref, sabs, K = O.direct(x[b, :n], up, down, h)
        m = len(ref)
        assert (y[b, m:] == 0).all(), "%s row %d: nonzero beyond out_len" % (tag, b)
        bound = O.bound(sabs, K)
        err = np.abs(y[b, :m] - ref)
        assert (err <= bound).all(), "%s row %d (len %d): worst %.3e of the bound" % (
            tag, b, n, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("%s: worst error / bound = %.3f" % (tag, worst))


@pytest.mark.parametrize("orig_sr", [44100, 48000, 24000, 16000])
def test_ragged_batch(mg, orig_sr):
    up, down = O.RATIOS[(orig_sr, TARGET)]
    assert mg.audio.RESAMPLE_TILE == mg._lib.MG_RESAMPLE_TILE
    lens = _lengths(up, down, mg.audio.RESAMPLE_TILE)
    x = _batch(lens, orig_sr)
    y, ol = mg.audio.resample(torch.from_numpy(x).to(DEV), orig_sr, TARGET, lens)
    _check(y.cpu().numpy(), ol.cpu(), x, lens, up, down, "%d->%d" % (orig_sr, TARGET))
    # the same rows in reversed order: a row does not depend on its place in the batch
    yr, olr = mg.audio.resample(torch.from_numpy(x[::-1].copy()).to(DEV), orig_sr, TARGET, lens[::-1])
    _check(yr.cpu().numpy(), olr.cpu(), x[::-1], lens[::-1], up, down, "%d->%d reversed" % (orig_sr, TARGET))
    assert torch.equal(yr.flip(0), y)


def test_equal_rates_copy(mg):
    lens = _lengths(1, 1, mg.audio.RESAMPLE_TILE)
    x = _batch(lens, 1)
    y, ol = mg.audio.resample(torch.from_numpy(x).to(DEV), TARGET, TARGET, torch.tensor(lens))
    y = y.cpu().numpy()
    assert ol.tolist() == lens and y.shape == (len(lens), max(lens))
    for b, n in enumerate(lens):
        assert np.array_equal(y[b, :n], x[b, :n]) and (y[b, n:] == 0).all()


def test_one_dimensional_and_filter_parameters(mg):
    rng = np.random.default_rng(5)
    x = rng.standard_normal(700).astype(np.float32)
    y, ol = mg.audio.resample(torch.from_numpy(x).to(DEV), 48000, TARGET, num_zeros=16, beta=8.0, rolloff=0.9)
    h = O.ref_filter(147, 320, 16, 8.0, 0.9)
    ref, sabs, K = O.direct(x, 147, 320, h)
    assert y.dim() == 1 and ol.tolist() == [len(ref)] and y.shape == (len(ref),)
    assert (np.abs(y.cpu().numpy() - ref) <= O.bound(sabs, K)).all()


def test_index_beyond_2_31(mg):
    """One row of 6.8 M samples at 22050 -> 16000: n down passes 2^31 near output 4.87 M.  The last 2048 outputs."""
    up, down = O.RATIOS[(22050, 16000)]
    n = 6_800_000
    x = np.random.default_rng(31).standard_normal(n).astype(np.float32)
    m = O.out_len(n, up, down)
    assert (m - 2048) * down > 2 ** 31
    y, ol = mg.audio.resample(torch.from_numpy(x).to(DEV), 22050, 16000)
    assert ol.tolist() == [m] and y.shape == (m,)
    tail = y[m - 2048:].cpu().numpy()
    h = O.ref_filter(up, down)
    outs = np.arange(m - 2048, m, dtype=np.int64)      # the direct form of resample_oracle for these outputs only
    half = (len(h) - 1) // 2
    nd = outs * down
    k = (-((half - nd) // up))[:, None] + np.arange(2 * half // up + 1, dtype=np.int64)[None, :]
    hi = nd[:, None] - k * up + half
    ok = (k >= 0) & (k < n) & (hi >= 0) & (hi <= 2 * half)
    terms = np.where(ok, up * h[np.clip(hi, 0, 2 * half)] * x[np.clip(k, 0, n - 1)].astype(np.float64), 0.0)
    ref, bound = terms.sum(1), O.bound(np.abs(terms).sum(1), ok.sum(1))
    err = np.abs(tail - ref)
    print("2^31: worst error / bound = %.3f" % float((err / bound).max()))
    assert np.isfinite(tail).all() and (err <= bound).all()


def test_tones(mg):
    """44100 -> 22050, interior samples (64 max(1, down / up) = 128 outputs skipped at each end): a 1 kHz sine comes
    out as the analytic sine at the new rate within the 1e-3 dB passband figure, a 15 kHz sine below -130 dB."""
    up, down = O.RATIOS[(44100, TARGET)]
    n, amp, skip = 8192, 0.5, 128
    t = np.arange(n, dtype=np.float64)
    x = np.stack([amp * np.sin(2 * np.pi * 1000.0 * t / 44100), amp * np.sin(2 * np.pi * 15000.0 * t / 44100)])
    x32 = x.astype(np.float32)
    y, _ = mg.audio.resample(torch.from_numpy(x32).to(DEV), 44100, TARGET)
    y = y.cpu().numpy()[:, skip:-skip]
    h = O.ref_filter(up, down)
    m = np.arange(n // 2, dtype=np.float64)[skip:-skip]
    for row, want, tol in ((0, amp * np.sin(2 * np.pi * 1000.0 * m / TARGET), amp * (10 ** (1e-3 / 20) - 1)),
                           (1, np.zeros(len(m)), amp * 10 ** (-130 / 20))):
        _, sabs, K = O.direct(x32[row], up, down, h)
        bound = O.bound(sabs, K)[skip:-skip]
        err = np.abs(y[row] - want)
        print("tone %d: worst error %.3e, allowed >= %.3e" % (row, float(err.max()), tol))
        assert (err <= tol + bound).all()


def test_peak_normalize_int16(mg):
    rng = np.random.default_rng(9)
    lens = [700, 1, 333, 257, 64]
    x = np.full((len(lens), 705), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = (0.3 * rng.standard_normal(n)).astype(np.float32)
    x[0, 17] = 1.7          # positive peak -> 32767
    x[2, 40] = -2.5         # negative peak -> -32768
    x[3, :257] = 0.0        # all zero
    x[1, 0] = 0.25          # a single positive sample
    q = mg.audio.peak_normalize_int16(torch.from_numpy(x).to(DEV), lens).cpu().numpy()
    assert q.dtype == np.int16 and q.shape == x.shape
    for b, n in enumerate(lens):
        row = x[b, :n]
        peak = np.abs(row).max()
        v = row / peak * np.float32(32768) if peak > 0 else np.zeros(n, np.float32)
        assert v.dtype == np.float32
        want = np.trunc(np.clip(v, -32768, 32767)).astype(np.int16)
        assert np.array_equal(q[b, :n], want), "row %d" % b
        assert (q[b, n:] == 0).all()
    assert q[0, 17] == 32767 and q[2, 40] == -32768 and q[1, 0] == 32767 and not q[3].any()
    # one-dimensional, other full scale
    q1 = mg.audio.peak_normalize_int16(torch.from_numpy(x[4, :64].copy()).to(DEV), max_wav_value=1000.0).cpu().numpy()
    v = x[4, :64] / np.abs(x[4, :64]).max() * np.float32(1000)
    assert np.array_equal(q1, np.trunc(v).astype(np.int16))


# ---------------------------------------------------------------------------------------------
# prepare_align end to end, and the corpus builder's loader
# ---------------------------------------------------------------------------------------------
def _signal(n, sr, seed, channels=1):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = sum(a * np.sin(2 * np.pi * f * t + p)[:, None] * np.ones(channels)
            for a, f, p in ((0.3, 220.0, 0.1), (0.2, 1870.0, 1.0), (0.1, 6100.0, 2.0)))
    return x + 0.02 * rng.standard_normal((n, channels))


def _mono32(data):
    """What the reader makes of a wav's samples: float32 in [-1, 1), channels averaged."""
    x = data.astype(np.float32) / 32768.0 if data.dtype == np.int16 else data.astype(np.float32)
    return x.mean(axis=1) if x.ndim == 2 else x


def _check_written(path, data, sr):
    from scipy.io import wavfile
    up, down = O.RATIOS.get((sr, TARGET), (1, 1))
    got_sr, q = wavfile.read(path)
    x = _mono32(data)
    assert got_sr == TARGET and q.dtype == np.int16 and q.shape == (O.out_len(len(x), up, down),)
    if (up, down) == (1, 1):
        y, bound = x.astype(np.float64), O.bound(np.abs(x.astype(np.float64)), 1)
    else:
        y, sabs, K = O.direct(x, up, down, O.ref_filter(up, down))
        bound = O.bound(sabs, K)
    peak = np.abs(y).max()
    v, delta = np.abs(y / peak * 32768.0), bound * 32768.0 / peak
    aq = np.abs(q.astype(np.float64))
    assert (aq <= v + delta).all() and (aq > v - 1 - delta).all(), path
    assert (np.sign(q) * np.sign(y) >= 0).all() and aq.max() >= 32767
    print("%s: max delta %.3f" % (os.path.basename(path), float(delta.max())))


def _config(tmp_path, dataset, cleaners):
    return {"dataset": dataset,
            "path": {"corpus_path": str(tmp_path / "corpus"), "raw_path": str(tmp_path / "raw_data")},
            "preprocessing": {"audio": {"sampling_rate": TARGET, "max_wav_value": 32768.0},
                              "text": {"text_cleaners": cleaners}}}


def _write(path, sr, data):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, sr, data)
    return data


def test_prepare_align_ljspeech(mg, tmp_path):
    pytest.importorskip("scipy")
    wavs = tmp_path / "corpus" / "wavs"
    files = {
        "LJ001-0001": (22050, (_signal(6615, 22050, 1)[:, 0] * 20000).astype(np.int16)),
        "LJ001-0002": (44100, (_signal(13230, 44100, 2)[:, 0] * 20000).astype(np.int16)),
        "LJ001-0003": (48000, _signal(14400, 48000, 3, channels=2).astype(np.float32)),
    }
    for name, (sr, data) in files.items():
        _write(str(wavs / (name + ".wav")), sr, data)
    (tmp_path / "corpus" / "metadata.csv").write_text(
        "".join("%s|raw %d|Text Number %d\n" % (name, i, i) for i, name in enumerate(files)), encoding="utf-8")
    mg.prepare_align.prepare_align(_config(tmp_path, "LJSpeech", ["english_cleaners"]),
                                   clean_text=lambda text, cleaners: text.upper())
    out = tmp_path / "raw_data" / "LJSpeech"
    for i, (name, (sr, data)) in enumerate(files.items()):
        _check_written(str(out / (name + ".wav")), data, sr)
        assert (out / (name + ".lab")).read_text() == "TEXT NUMBER %d" % i


def test_prepare_align_aishell3(mg, tmp_path):
    pytest.importorskip("scipy")
    corpus = tmp_path / "corpus"
    a = _write(str(corpus / "train" / "wav" / "SSB0005" / "SSB00050001.wav"), 44100,
               (_signal(13230, 44100, 4)[:, 0] * 12000).astype(np.int16))
    b = _write(str(corpus / "test" / "wav" / "SSB0009" / "SSB00090002.wav"), 44100,
               (_signal(11000, 44100, 5)[:, 0] * 25000).astype(np.int16))
    (corpus / "train" / "content.txt").write_text("SSB00050001.wav\t广 guang3 州 zhou1\nSSB00050007.wav\t女 nv3\n",
                                                  encoding="utf-8")
    (corpus / "test" / "content.txt").write_text("SSB00090002.wav\t大 da4 学 xue2\n", encoding="utf-8")
    mg.prepare_align.prepare_align(_config(tmp_path, "AISHELL3", []))
    raw = tmp_path / "raw_data"
    _check_written(str(raw / "SSB0005" / "SSB00050001.wav"), a, 44100)
    _check_written(str(raw / "SSB0009" / "SSB00090002.wav"), b, 44100)
    assert (raw / "SSB0005" / "SSB00050001.lab").read_text() == "guang3 zhou1"
    assert (raw / "SSB0009" / "SSB00090002.lab").read_text() == "da4 xue2"
    assert sorted(os.listdir(str(raw / "SSB0005"))) == ["SSB00050001.lab", "SSB00050001.wav"]


def test_preprocessor_loader_resamples(mg, tmp_path):
    pytest.importorskip("scipy")
    P = mg.preprocessor
    data = _write(str(tmp_path / "a.wav"), 44100, (_signal(3000, 44100, 6)[:, 0] * 20000).astype(np.int16))
    with pytest.raises(P.SamplingRateMismatch):
        P.scipy_load_wav(TARGET)(str(tmp_path / "a.wav"))
    got = P.scipy_load_wav(TARGET, resample=True)(str(tmp_path / "a.wav"))
    ref, sabs, K = O.direct(_mono32(data), 1, 2, O.ref_filter(1, 2))
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert (np.abs(got - ref) <= O.bound(sabs, K)).all()
    # the builder hands the keyword to its default loader
    import inspect
    assert inspect.signature(P.Preprocessor.__init__).parameters["resample"].default is False
