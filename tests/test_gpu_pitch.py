"""The native pitch extractor (csrc/pitch.hip, mixgan_tts_amd/pitch.py) on the GPU against its float64 oracle
(tests/pitch_oracle.py), against signals of known F0, and inside the corpus builder.  The extractor is this project's
own algorithm; nothing here measures parity with pyworld."""
import os

import numpy as np
import pytest
import torch

import pitch_oracle as O
import preprocessor_corpus as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SR, HOP = 22050, 256
FINE_CENTS = 2 * 0.792      # test_pitch_cpu.py: twice the oracle's own worst error on the constant tones


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd as m
    assert torch.cuda.is_available()
    m.lib()
    return m


def _batch(rows, fill=np.nan):
    lens = np.array([len(r) for r in rows])
    x = np.full((len(rows), int(lens.max())), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x).to(DEV), lens


_ORACLE = {}


def _oracle(sr, hop):
    if (sr, hop) not in _ORACLE:
        rows = O.stage1_rows(sr, hop)
        _ORACLE[(sr, hop)] = (rows, [O.stage1(r, sr, hop) for r in rows])
    return _ORACLE[(sr, hop)]


def _cost_bound(s, k, lag):
    """Bound on |d'_kernel - d'_oracle| at one lag of frame k.  After the FFTs the kernel works in float64, so d is off
    by 2 eps_r, eps_r the error of the correlation r.  With u = 2^-24, a radix-4 pass (one complex multiply by a
    rounded twiddle, two levels of additions) moves the 2-norm by at most 6 u of its own, five passes by rho = 30 u.
    E is the frame's energy, ||a||, ||b|| <= sqrt(E):
      first FFT and split:  ||dA||, ||dB|| <= rho sqrt(N) sqrt(2 E);  |dr| <= ||dP||_1 / N <= (2 sqrt(2) rho + 4 u) E
      second FFT:           |dr| <= rho ||FFT(P)||_2 / N <= rho ||a||_1 sqrt(E) <= rho sqrt(W) E
    so eps_r = ((2 sqrt 2 + sqrt W) rho + 4 u) E.  d' = d tau / C with C the running sum, itself off by at most
    tau 2 eps_r:  |dd'| <= tau 2 eps_r (1 + d') / (C - tau 2 eps_r), plus the float32 rounding of the output."""
    rho = 30 * U
    eps_d = 2 * ((2 * np.sqrt(2) + np.sqrt(O.W)) * rho + 4 * U) * s["energy"][k]
    run, dp = s["run"][k, lag - 1], s["dprime"][k, lag]
    if lag * eps_d >= run / 2:
        return np.inf
    return lag * eps_d * (1 + dp) / (run - lag * eps_d) + U * dp


@pytest.mark.parametrize("sr,hop", sorted(O.STAGE1_ROWS))
def test_stage1_matches_the_oracle(mg, sr, hop):
    rows, ref = _oracle(sr, hop)
    x, lens = _batch(rows)
    period, cost, rms, nf = mg.yin_candidates(x, sr, hop, lens)
    xr, lens_r = _batch(rows[::-1])
    out_r = mg.yin_candidates(xr, sr, hop, lens_r)
    torch.cuda.synchronize()
    T = int(lens.max()) // hop + 1
    assert period.shape == cost.shape == (len(rows), T, O.K) and rms.shape == (len(rows), T)
    assert period.dtype == cost.dtype == rms.dtype == torch.float32 and nf.dtype == torch.int32
    assert nf.cpu().tolist() == [n // hop + 1 for n in lens]
    for got, rev in zip((period, cost, rms, nf), out_r):
        assert torch.equal(got, rev.flip(0)), "a row depends on its place in the batch"
    period, cost, rms = period.cpu().numpy(), cost.cpu().numpy(), rms.cpu().numpy()
    assert np.isfinite(period).all() and np.isfinite(cost).all() and np.isfinite(rms).all()
    worst_ratio = worst_cost = worst_period = worst_rms = 0.0
    for b, s in enumerate(ref):
        Tb = len(s["rms"])
        assert not period[b, Tb:].any() and not cost[b, Tb:].any() and not rms[b, Tb:].any()
        r32 = s["rms"].astype(np.float32)
        err = np.abs(rms[b, :Tb].astype(np.float64) - r32)
        assert (err <= 5 * U * r32).all(), (b, err.max())      # 4 * 2^-24 relative and one rounding
        worst_rms = max(worst_rms, float((err[r32 > 0] / r32[r32 > 0]).max()) if (r32 > 0).any() else 0.0)
        keep = s["margin"] >= O.MARGIN_MIN
        assert (~keep).sum() <= int(O.MARGIN_CAP * Tb)
        for k in np.nonzero(keep)[0]:
            for c in range(O.K):
                lag = s["lag"][k, c]
                if lag == 0:
                    assert period[b, k, c] == 0 and cost[b, k, c] == O.EMPTY_COST, (b, k, c)
                    continue
                assert abs(float(period[b, k, c]) - lag) <= 0.5 + 1e-4, (b, k, c, period[b, k], s["lag"][k])
                rel = abs(float(period[b, k, c]) - s["period"][k, c]) / s["period"][k, c]
                worst_period = max(worst_period, rel)
                assert rel <= 1e-5, (b, k, c, period[b, k, c], s["period"][k, c])
                e, bound = abs(float(cost[b, k, c]) - s["cost"][k, c]), _cost_bound(s, k, lag)
                worst_cost = max(worst_cost, e)
                if np.isfinite(bound):
                    worst_ratio = max(worst_ratio, e / bound)
                assert e <= bound, (b, k, c, e, bound)
    print("stage 1 at %d / %d: worst cost error %.3e (%.3f of its bound), period %.3e relative, rms %.3e relative"
          % (sr, hop, worst_cost, worst_ratio, worst_period, worst_rms))


def _track_case(mg, rows, sr, tau_floor=71.0, **params):
    """rows: [(period [T, K], cost [T, K], rms [T])] float32 -> the kernel's f0 rows, checked bit for bit."""
    T = max(len(r[2]) for r in rows)
    B = len(rows)
    per, cst = np.zeros((B, T, O.K), np.float32), np.zeros((B, T, O.K), np.float32)
    rm, nf = np.zeros((B, T), np.float32), np.zeros(B, np.int32)
    for b, (p, c, r) in enumerate(rows):
        nf[b] = len(r)
        per[b, :nf[b]], cst[b, :nf[b]], rm[b, :nf[b]] = p, c, r
    dev = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    f0 = mg.pitch_track(dev(per), dev(cst), dev(rm), dev(nf), sr, tau_floor, **params)
    torch.cuda.synchronize()
    assert f0.dtype == torch.float64 and f0.shape == (B, T)
    f0 = f0.cpu().numpy()
    tau_max = int(np.ceil(sr / tau_floor))
    paths = []
    for b, (p, c, r) in enumerate(rows):
        want, path = O.track(p, c, r, sr, tau_max, **dict(O.DEFAULTS, **params))
        assert not f0[b, nf[b]:].any()
        assert np.array_equal(f0[b, :nf[b]], want), (b, np.nonzero(f0[b, :nf[b]] != want)[0][:5])
        # the path, read back from the F0: the slots of a frame hold different periods
        got_path = np.full(nf[b], O.UNVOICED)
        for t in np.nonzero(f0[b, :nf[b]])[0]:
            slots = np.nonzero(p[t])[0]
            got_path[t] = int(slots[np.nonzero(sr / p[t][slots].astype(np.float64) == f0[b, t])[0][0]])
        assert np.array_equal(got_path, path), b
        paths.append(path)
    return f0, paths


def test_stage2_equals_the_oracle_bit_for_bit(mg):
    suite = O.suite(SR)
    rows = []
    for name in ("mixed", "glide", "tone80", "tone650", "second_strongest"):
        s = O.stage1(suite[name][0], SR, HOP)
        rows.append((s["period"].astype(np.float32), s["cost"].astype(np.float32), s["rms"].astype(np.float32)))
    assert (rows[2][0][10] == 0).any() and (rows[2][0][10] != 0).any()      # tone80: empty slots beside a candidate
    rows.append(tuple(a[:1] for a in rows[1]))                              # a row of one frame
    _, paths = _track_case(mg, rows, SR)
    assert (paths[0] == O.UNVOICED).any() and (paths[0] != O.UNVOICED).any()
    # every frame gated: the gate lies above the loudest frame
    f0, paths = _track_case(mg, rows[:2], SR, gate_db=6.0)
    assert not f0.any() and all((p == O.UNVOICED).all() for p in paths)


def test_stage2_ties_go_to_the_lowest_state(mg):
    T = 5
    per = np.tile(np.array([100.0, 50.0, 0.0, 0.0], np.float32), (T, 1))
    cst = np.tile(np.array([0.125, 0.125, 1e30, 1e30], np.float32), (T, 1))
    rms = np.full(T, 0.1, np.float32)
    # equal slots, no period bias, no pull between periods: slot 0; the same cost as the unvoiced state: still slot 0
    f0, paths = _track_case(mg, [(per, cst, rms)], 22050, beta=0.0, lam=0.0, theta=0.125)
    assert (paths[0] == 0).all() and (f0[0] == 22050 / 100.0).all()
    # the tie is between slot 1 and unvoiced once slot 0 is dearer
    cst2 = cst.copy()
    cst2[:, 0] = 0.5
    f0, paths = _track_case(mg, [(per, cst2, rms)], 22050, beta=0.0, lam=0.0, theta=0.125)
    assert (paths[0] == 1).all()


@pytest.fixture(scope="module")
def suite_f0(mg):
    suite = O.suite(SR)
    names = sorted(suite)
    rows = [suite[n][0] for n in names]
    rows[names.index("mixed")] = rows[names.index("mixed")][:-3000]      # a shorter row: its padding is NaN
    x, lens = _batch(rows)
    f0, nf = mg.extract_f0(x, SR, HOP, lens)
    torch.cuda.synchronize()
    assert f0.dtype == torch.float64 and nf.cpu().tolist() == [n // HOP + 1 for n in lens]
    return names, rows, {n: suite[n][1][:len(r)] for n, r in zip(names, rows)}, f0.cpu().numpy(), nf.cpu().numpy()


def test_extract_f0_against_ground_truth_and_the_oracle(mg, suite_f0):
    names, rows, truth, f0, nf = suite_f0
    assert np.isfinite(f0).all()
    for b, name in enumerate(names):
        got = f0[b, :nf[b]]
        assert not f0[b, nf[b]:].any()
        worst, count = O.judge(got, truth[name], HOP, FINE_CENTS, glide=name == "glide")
        want = O.extract_f0(rows[b], SR, HOP)
        both = (got > 0) & (want > 0)
        differ = int(((got > 0) != (want > 0)).sum())
        rel = float(np.abs(got[both] / want[both] - 1).max()) if both.any() else 0.0
        print("%s: %d frames against the truth, worst %.3f cents; against the oracle %.3e relative, %d of %d frames "
              "differ in voicing" % (name, count, worst, rel, differ, nf[b]))
        assert rel <= 1e-5 and differ <= int(0.02 * nf[b])
        if name == "zeros":
            assert not got.any()


def test_native_pitch_is_a_pitch_fn(mg):
    x = O.suite(SR)["tone220"][0][:6000]
    f0 = mg.native_pitch(x.astype(np.float64), SR, HOP / SR * 1000)
    assert isinstance(f0, np.ndarray) and f0.dtype == np.float64 and f0.shape == (len(x) // HOP + 1,)
    assert abs(f0[10] / 220.0 - 1) < 1e-3
    with pytest.raises(mg.PitchGeometryError, match="sampling_rate=44100"):
        mg.native_pitch(x, 44100, 256 / 44100 * 1000)
    with pytest.raises(mg.MixganHipError):
        mg.yin_candidates(torch.zeros(100), SR, HOP)      # a CPU tensor: no fallback


def _oracle_pitch_fn(wav, sr, frame_period_ms):
    return O.extract_f0(wav.astype(np.float32), sr, int(round(frame_period_ms * sr / 1000)))


def _build(mg, root, pitch_fn, feature, batch):
    raw, pre = C.write_corpus(str(root))
    mg.Preprocessor(*C.configs(raw, pre, feature, False), pitch_fn=pitch_fn, load_wav=C.load_wav,
                    batch_utterances=batch).build_from_path()
    return pre


def _pitch_files(pre):
    return {f: np.load(os.path.join(pre, "pitch", f)) for f in sorted(os.listdir(os.path.join(pre, "pitch")))}


def test_the_builder_with_native_pitch_matches_the_oracle_as_pitch_fn(mg, tmp_path, monkeypatch):
    """pitch_fn="native" against pitch_fn=<the oracle>, without pyworld.  The kernel's F0 is within 1e-5 relative of the
    oracle's on frames both call voiced (stage 1 leaves in float32), so frame-level files agree to that, and the
    phoneme averages, means of values interpolated linearly between voiced frames, to 1e-5 of the utterance's largest
    F0 plus the 1e-12 the averaging kernel is held to.  An utterance whose voicing differs (at most 2 % of its frames
    may) is left out of the value comparison, in both trees."""
    import builtins
    real_import = builtins.__import__

    def no_pyworld(name, *a, **kw):
        if name == "pyworld":
            raise ImportError("no pyworld in this test")
        return real_import(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_pyworld)

    frame_n = _pitch_files(_build(mg, tmp_path / "fn", "native", "frame_level", 4))
    frame_o = _pitch_files(_build(mg, tmp_path / "fo", _oracle_pitch_fn, "frame_level", 16))
    assert sorted(frame_n) == sorted(frame_o) and len(frame_n) >= 4
    same_voicing = []
    for f in frame_n:
        a, b = frame_n[f], frame_o[f]
        assert a.dtype == b.dtype == np.float64 and a.shape == b.shape
        differ = int(((a > 0) != (b > 0)).sum())
        assert differ <= int(0.02 * len(a)), (f, differ, len(a))
        both = (a > 0) & (b > 0)
        assert np.abs(a[both] / b[both] - 1).max() <= 1e-5, f
        if differ == 0:
            same_voicing.append(f)
    assert len(same_voicing) >= len(frame_n) // 2
    phon_n = _pitch_files(_build(mg, tmp_path / "pn", "native", "phoneme_level", 16))
    phon_o = _pitch_files(_build(mg, tmp_path / "po", _oracle_pitch_fn, "phoneme_level", 2))
    assert sorted(phon_n) == sorted(phon_o) == sorted(frame_n)
    for f in same_voicing:
        a, b = phon_n[f], phon_o[f]
        assert a.shape == b.shape and np.abs(a - b).max() <= (1e-5 + 1e-12) * frame_o[f].max(), f
    for name in ("train.txt", "val.txt", "filtered_out.txt", "stats.json", "speakers.json"):
        assert os.path.exists(os.path.join(str(tmp_path / "pn"), "preprocessed", name))


def test_the_default_pitch_fn_still_needs_pyworld(mg, tmp_path, monkeypatch):
    import builtins
    real_import = builtins.__import__

    def no_pyworld(name, *a, **kw):
        if name == "pyworld":
            raise ImportError("no pyworld in this test")
        return real_import(name, *a, **kw)
    monkeypatch.setattr(builtins, "__import__", no_pyworld)
    raw, pre = C.write_corpus(str(tmp_path))
    b = mg.Preprocessor(*C.configs(raw, pre), load_wav=C.load_wav)
    with pytest.raises(mg.PitchExtractorRequired, match="pitch_fn"):
        b.build_from_path()
