"""Host side of the resampler and of prepare_align (audio.resample_filter, audio.polyphase_table, the C ABI's argument
checks, prepare_align.py with its device stage stubbed).  The oracle is tests/resample_oracle.py."""
import ctypes
import os

import numpy as np
import pytest

import resample_oracle as O

import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib, audio
from mixgan_tts_amd import prepare_align as PA

RESPONSE_RATIOS = [(1, 2), (147, 320), (441, 320)]


def test_filter_equals_the_restatement():
    for up, down in O.RATIOS.values():
        h, ref = audio.resample_filter(up, down), O.ref_filter(up, down)
        assert h.dtype == np.float64 and h.shape == ref.shape == (2 * 64 * max(up, down) + 1,)
        assert np.abs(h - ref).max() <= 1e-14 * np.abs(ref).max()
        assert abs(h.sum() - 1) <= 1e-14
    h = audio.resample_filter(3, 2, num_zeros=8, beta=6.0, rolloff=0.8)
    assert np.abs(h - O.ref_filter(3, 2, 8, 6.0, 0.8)).max() <= 1e-14 * np.abs(h).max()


@pytest.mark.parametrize("up,down", RESPONSE_RATIOS)
def test_frequency_response(up, down):
    """Zero-padded FFT of h (DC gain 1); frequencies in units of the filter's own rate orig_sr * up, where the lower
    Nyquist is 0.5 / max(up, down) cycles per sample."""
    h = audio.resample_filter(up, down)
    nfft = 1 << int(np.ceil(np.log2(len(h) * 16)))
    H = np.abs(np.fft.rfft(h, nfft))
    f = np.arange(len(H)) / nfft
    nyq = 0.5 / max(up, down)
    db = 20 * np.log10(np.maximum(H, 1e-300))
    pass_dev = float(np.abs(db[f <= 0.85 * nyq]).max())
    stop = float(db[f >= 1.05 * nyq].max())
    print("%d:%d passband deviation %.3e dB, stopband %.1f dB" % (up, down, pass_dev, stop))
    assert pass_dev <= 1e-3
    assert stop <= -130


def test_polyphase_rows():
    for up, down in O.RATIOS.values():
        h = audio.resample_filter(up, down)
        half = (len(h) - 1) // 2
        t = audio.polyphase_table(h, up)
        Mh = half // up + 1
        assert t.shape[0] == up and t.shape[1] % 4 == 0 and 2 * Mh <= t.shape[1] < 2 * Mh + 4
        assert np.abs(t.sum(1) - 1).max() <= 1e-7                      # every row's DC gain
        assert abs(t.sum() - up) <= 1e-12 * up                          # every tap is in the table exactly once
        # the documented element, and the limits of the kernel
        r, j = up // 2, 3
        i = (Mh - 1 - j) * up + r + half
        assert t[r, j] == (up * h[i] if 0 <= i <= 2 * half else 0.0)
        assert up <= _lib.MG_RESAMPLE_MAX_UP and t.shape[1] <= _lib.MG_RESAMPLE_MAX_TAPS
        assert (_lib.MG_RESAMPLE_TILE - 1) * down // up + t.shape[1] + 2 <= _lib.MG_RESAMPLE_MAX_SPAN


def test_table_form_equals_the_definition():
    """y[n] = sum_j taps[r, j] x[q - Mh + 1 + j], as the header states it, against the direct form."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(300)
    for up, down in O.RATIOS.values():
        h = audio.resample_filter(up, down)
        half = (len(h) - 1) // 2
        t, Mh = audio.polyphase_table(h, up), half // up + 1
        y, sabs, _ = O.direct(x, up, down, h)
        xp = np.concatenate([np.zeros(t.shape[1] + Mh), x, np.zeros(t.shape[1] + Mh + down)])
        for n in (0, 1, len(y) // 2, len(y) - 1):
            q, r = divmod(n * down, up)
            s = q - Mh + 1 + t.shape[1] + Mh
            assert abs(t[r] @ xp[s:s + t.shape[1]] - y[n]) <= 1e-13 * max(sabs[n], 1e-300)


def test_oracle_equals_scipy_resample_poly():
    sig = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(0).standard_normal(1237)
    for up, down in O.RATIOS.values():
        h = O.ref_filter(up, down)
        y, _, _ = O.direct(x, up, down, h)
        ref = sig.resample_poly(x, up, down, window=h)
        assert y.shape == ref.shape == (O.out_len(1237, up, down),)
        assert np.abs(y - ref).max() <= 1e-12


def test_resample_ratio():
    for (src, dst), ud in O.RATIOS.items():
        assert audio.resample_ratio(src, dst) == ud
    assert audio.resample_ratio(22050, 22050) == (1, 1)
    with pytest.raises(ValueError):
        audio.resample_ratio(0, 22050)


def test_abi_symbols_and_argument_checks():
    assert {"mg_resample_poly", "mg_peak_normalize_i16"} <= set(_lib.EXPORTS)
    L = mg.lib()
    p, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)      # never dereferenced: every call below returns before a launch
    ok = dict(x=p, x_bs=100, lengths=null, B=1, N=100, taps=p, up=1, down=2, Kp=260, half=128, y=p, y_bs=50, M=50)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mg_resample_poly(a["x"], a["x_bs"], a["lengths"], a["B"], a["N"], a["taps"], a["up"], a["down"],
                                  a["Kp"], a["half"], a["y"], a["y_bs"], a["M"], null)
    assert call(x=null) == _lib.MG_ERR_ARG and call(y=null) == _lib.MG_ERR_ARG and call(taps=null) == _lib.MG_ERR_ARG
    assert call(taps=ctypes.c_void_p(4100)) == _lib.MG_ERR_ARG                      # not 16-byte aligned
    for bad in (dict(B=0), dict(N=0), dict(M=0), dict(up=0), dict(down=0), dict(x_bs=99), dict(y_bs=49),
                dict(up=_lib.MG_RESAMPLE_MAX_UP + 1, Kp=4, half=0),
                dict(Kp=_lib.MG_RESAMPLE_MAX_TAPS + 4), dict(Kp=258), dict(Kp=256),  # Kp % 4, Kp < 2 (half / up + 1)
                dict(up=3, down=64, Kp=260, half=128)):                               # staged span beyond the limit
        assert call(**bad) == _lib.MG_ERR_SHAPE, bad

    def norm(x=p, x_bs=10, B=1, N=10, mwv=32768.0, out=p, out_bs=10):
        return L.mg_peak_normalize_i16(x, x_bs, null, B, N, mwv, out, out_bs, null)
    assert norm(x=null) == _lib.MG_ERR_ARG and norm(out=null) == _lib.MG_ERR_ARG and norm(mwv=0.0) == _lib.MG_ERR_ARG
    for bad in (dict(B=0), dict(N=0), dict(x_bs=9), dict(out_bs=9)):
        assert norm(**bad) == _lib.MG_ERR_SHAPE, bad


def test_no_cpu_path():
    import torch
    with pytest.raises(mg.MixganHipError):
        audio.resample(torch.zeros(100), 44100, 22050)
    with pytest.raises(mg.MixganHipError):
        audio.peak_normalize_int16(torch.zeros(100))


# ---------------------------------------------------------------------------------------------
# prepare_align's host logic, the device stage stubbed
# ---------------------------------------------------------------------------------------------
def _config(tmp_path, dataset, cleaners):
    return {"dataset": dataset,
            "path": {"corpus_path": str(tmp_path / "corpus"), "raw_path": str(tmp_path / "raw_data")},
            "preprocessing": {"audio": {"sampling_rate": 22050, "max_wav_value": 32768.0},
                              "text": {"text_cleaners": cleaners}}}


@pytest.fixture
def stub(monkeypatch):
    calls = []

    def convert_group(wavs, orig_sr, target_sr, max_wav_value, device):
        calls.append((orig_sr, [len(w) for w in wavs]))
        up, down = audio.resample_ratio(orig_sr, target_sr)
        return [np.full(O.out_len(len(w), up, down), 7, dtype=np.int16) for w in wavs]
    monkeypatch.setattr(PA, "convert_group", convert_group)
    return calls


def _write(path, sr, data):
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, sr, data)


def test_prepare_align_ljspeech_layout(tmp_path, stub):
    pytest.importorskip("scipy")
    from scipy.io import wavfile
    corpus = tmp_path / "corpus"
    _write(str(corpus / "wavs" / "LJ001-0001.wav"), 22050, np.zeros(100, np.int16))
    _write(str(corpus / "wavs" / "LJ001-0002.wav"), 44100, np.zeros(201, np.int16))
    _write(str(corpus / "wavs" / "LJ001-0004.wav"), 22050, np.zeros((50, 2), np.float32))
    (corpus / "metadata.csv").write_text("LJ001-0001|Raw one|Normalised One\nLJ001-0002|Raw 2|Normalised two\n"
                                         "LJ001-0003|Raw 3|no such wav\nLJ001-0004|Raw 4|Four\n", encoding="utf-8")
    cfg = _config(tmp_path, "LJSpeech", ["english_cleaners"])
    with pytest.raises(PA.CleanTextRequired, match="clean_text"):
        PA.prepare_align(cfg)
    seen = []

    def clean(text, cleaners):
        seen.append((text, tuple(cleaners)))
        return text.lower()
    PA.prepare_align(cfg, clean_text=clean, batch_utterances=2, device="stub")
    out = tmp_path / "raw_data" / "LJSpeech"
    assert sorted(os.listdir(str(out))) == ["LJ001-0001.lab", "LJ001-0001.wav", "LJ001-0002.lab", "LJ001-0002.wav",
                                            "LJ001-0004.lab", "LJ001-0004.wav"]
    assert (out / "LJ001-0002.lab").read_text() == "normalised two"
    assert ("Normalised One", ("english_cleaners",)) in seen
    for name, n in (("LJ001-0001", 100), ("LJ001-0002", 101), ("LJ001-0004", 50)):
        sr, q = wavfile.read(str(out / (name + ".wav")))
        assert sr == 22050 and q.dtype == np.int16 and q.shape == (n,)
    # batches of two listed wavs that exist, each grouped by source rate; stereo was averaged to mono
    assert stub == [(22050, [100]), (44100, [201]), (22050, [50])]
    # no cleaners configured: no function needed, the text is written as it is
    PA.prepare_align(_config(tmp_path, "LJSpeech", []), device="stub")
    assert (out / "LJ001-0002.lab").read_text() == "Normalised two"


def test_prepare_align_aishell3_layout(tmp_path, stub):
    pytest.importorskip("scipy")
    from scipy.io import wavfile
    corpus = tmp_path / "corpus"
    _write(str(corpus / "train" / "wav" / "SSB0005" / "SSB00050001.wav"), 44100, np.zeros(441, np.int16))
    _write(str(corpus / "test" / "wav" / "SSB0009" / "SSB00090002.wav"), 44100, np.zeros(300, np.int16))
    (corpus / "train" / "content.txt").write_text("SSB00050001.wav\t广 guang3 州 zhou1\n"
                                                  "SSB00050007.wav\t女 nv3\n", encoding="utf-8")
    (corpus / "test" / "content.txt").write_text("SSB00090002.wav\t大 da4 学 xue2 生 sheng1\n", encoding="utf-8")
    PA.prepare_align(_config(tmp_path, "AISHELL3", []), device="stub")
    raw = tmp_path / "raw_data"
    assert sorted(os.listdir(str(raw))) == ["SSB0005", "SSB0009"]
    assert sorted(os.listdir(str(raw / "SSB0005"))) == ["SSB00050001.lab", "SSB00050001.wav"]
    assert (raw / "SSB0005" / "SSB00050001.lab").read_text() == "guang3 zhou1"
    assert (raw / "SSB0009" / "SSB00090002.lab").read_text() == "da4 xue2 sheng1"
    sr, q = wavfile.read(str(raw / "SSB0005" / "SSB00050001.wav"))
    assert sr == 22050 and q.dtype == np.int16 and q.shape == (221,)
    assert stub == [(44100, [441, 300])]      # one batch across both sets, one group per source rate
