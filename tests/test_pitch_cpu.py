"""The pitch extractor's float64 oracle (tests/pitch_oracle.py) against signals whose F0 is known, the geometry
errors, the frame count, and the new exports.  No GPU.  The oracle is a restatement of this project's own algorithm
(YIN candidates + a Viterbi track); nothing here measures parity with pyworld."""
import os
import re

import numpy as np
import pytest

import pitch_oracle as O
from helpers import ROOT

SR, HOP = 22050, 256
# The oracle's worst error on the constant tones of the suite at 22050 / 256 is 0.792 cents (650 Hz; 0.551 at 400,
# 0.181 at 220, 0.071 at 120, 0.033 at 80: the three-point parabola on a 34-sample period); twice that is allowed.
FINE_CENTS = 2 * 0.792


@pytest.fixture(scope="module")
def suite():
    return O.suite(SR)


@pytest.mark.parametrize("name", ["tone80", "tone120", "tone220", "tone400", "tone650", "glide", "second_strongest",
                                  "mixed", "zeros"])
def test_oracle_against_ground_truth(suite, name):
    x, truth = suite[name]
    f0 = O.extract_f0(x, SR, HOP)
    assert f0.dtype == np.float64 and f0.shape == (len(x) // HOP + 1,) and np.isfinite(f0).all()
    worst, count = O.judge(f0, truth, HOP, FINE_CENTS, glide=name == "glide")
    print("%s: %d voiced frames checked, worst %.3f cents" % (name, count, worst))
    if name == "zeros":
        assert not f0.any()
    elif name != "mixed":
        assert count > 70


def test_an_all_zero_frame_has_no_candidates_and_finite_values():
    s = O.stage1(np.zeros(700, dtype=np.float32), SR, HOP)
    assert (s["dprime"] == 1).all() and not s["period"].any() and (s["cost"] == float(O.EMPTY_COST)).all()
    assert not s["rms"].any()


def test_geometry_errors():
    import mixgan_tts_amd as mg
    assert mg.pitch.pitch_geometry(22050) == (27, 311) == O.geometry(22050)
    assert mg.pitch.pitch_geometry(16000) == O.geometry(16000) and mg.pitch.pitch_geometry(24000) == O.geometry(24000)
    with pytest.raises(mg.PitchGeometryError, match="sampling_rate=44100.*f0_floor=71"):
        mg.pitch.pitch_geometry(44100, 71.0)
    with pytest.raises(mg.PitchGeometryError, match="sampling_rate"):
        mg.pitch.pitch_geometry(1500)                  # tau_min = 1
    assert mg.pitch.pitch_geometry(1600) == (2, 23)
    with pytest.raises(mg.PitchGeometryError):
        mg.pitch.pitch_geometry(36500)                 # ceil(36500 / 71) + 1 = 516 > 512
    assert mg.pitch.pitch_geometry(36000)[1] == 508
    assert issubclass(mg.PitchGeometryError, mg.MixganHipError) and issubclass(mg.PitchGeometryError, NotImplementedError)
    with pytest.raises(O.GeometryError):
        O.geometry(44100)


@pytest.mark.parametrize("n", [1, HOP - 1, HOP, HOP + 1])
def test_frame_count(n):
    import mixgan_tts_amd as mg
    want = n // HOP + 1
    assert mg.pitch.frame_count(n, HOP) == want == O.n_frames(n, HOP)
    x = 0.1 * np.random.default_rng(n).standard_normal(n).astype(np.float32)
    assert O.extract_f0(x, SR, HOP).shape == (want,)
    assert O.frames(x, HOP).shape == (want, O.N)
    assert (O.frames(x, HOP)[0, :O.N // 2] == 0).all() and O.frames(x, HOP)[0, O.N // 2] == x[0]


def test_plog2_is_log2_to_the_last_bits():
    x = np.concatenate([np.linspace(2.0, 520.0, 4001), 2.0 ** np.arange(1, 10), [0.70710678118654757, 1.0, 1.5]])
    assert np.abs(O.plog2(x) - np.log2(x)).max() < 4e-16 * 10


def test_exports_are_in_the_header_and_the_binding():
    import mixgan_tts_amd as mg
    from mixgan_tts_amd import _lib
    header = open(os.path.join(ROOT, "include", "mixgan_hip.h")).read()
    for name in ("mg_yin_candidates", "mg_pitch_track", "mg_pitch_track_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS
    for name in ("yin_candidates", "pitch_track", "extract_f0", "native_pitch"):
        assert callable(getattr(mg, name))
    assert (_lib.MG_PITCH_N, _lib.MG_PITCH_W, _lib.MG_PITCH_K) == (O.N, O.W, O.K)
    assert mg.pitch.TRACK_PARAMS == O.DEFAULTS


def test_native_is_an_option_and_the_default_still_needs_pyworld(tmp_path):
    import preprocessor_corpus as C
    import mixgan_tts_amd as mg
    raw, pre = C.write_corpus(str(tmp_path))
    assert mg.Preprocessor(*C.configs(raw, pre), pitch_fn="native", load_wav=C.load_wav).native_pitch
    with pytest.raises(ValueError, match="native"):
        mg.Preprocessor(*C.configs(raw, pre), pitch_fn="pyworld")
    pc, mc, tc = C.configs(raw, pre)
    pc["preprocessing"]["audio"]["sampling_rate"] = 44100
    with pytest.raises(mg.PitchGeometryError):
        mg.Preprocessor(pc, mc, tc, pitch_fn="native")


@pytest.mark.parametrize("sr,hop", sorted(O.STAGE1_ROWS))
def test_the_oracle_keeps_its_margin_on_the_stage1_rows(sr, hop):
    """What tests/test_gpu_pitch.py relies on: on its ragged batch at most 2 % of a row's frames have a decision
    margin under 1e-3, with the oracle alone."""
    lengths = [n for n, _, _ in O.STAGE1_ROWS[(sr, hop)]]
    assert lengths == [1, hop - 1, hop, hop + 1, 511, 512, 513, 1237, 5000, sr]
    for x in O.stage1_rows(sr, hop):
        m = O.stage1(x, sr, hop)["margin"]
        assert (m < O.MARGIN_MIN).sum() <= int(O.MARGIN_CAP * len(m)), (len(x), np.sort(m)[:3])
