"""mixgan_tts_amd.metrics on the GPU against tests/metrics_ref.py, the float64 restatement fed the same float32 arrays:
the cepstra, the DTW total and path at the issue's shapes and at Ta above a workgroup's 1024 threads, where a thread
owns several rows, known answers,
determinism, an empty pair, one long pair, the MCD and F0 figures and `evaluate_model`.

The DTW inputs are a cepstrum sequence and a piecewise time-warped, noisy copy of it (metrics_ref.warped_pair), so the
optimal path warps for real; tests/test_metrics_cpu.py holds the committed seeds to that.  Paths are never compared
cell by cell with the reference's: near-ties may resolve differently in float32.  What is checked is that the path is
a valid one and that its float64 cost is within the total's bar of the float64 optimum."""
import functools

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(Ta, Tb, D=13):
    """(a, b, float64 total) of the seeded pair; computed once and shared."""
    a, b = R.warped_pair(R.pair_seed(Ta, Tb, D), Ta, Tb, D)
    return a, b, R.dtw(a, b)[0]


def run_dtw(pairs, Ta=None, Tb=None, return_path=True):
    """The pairs [(a, b), ...] as one batch padded with NaN to (Ta, Tb) -> numpy (total, path_len, path)."""
    import mixgan_tts_amd as mg
    Ta = Ta or max(len(a) for a, _ in pairs)
    Tb = Tb or max(len(b) for _, b in pairs)
    D = pairs[0][0].shape[1]
    A = np.full((len(pairs), Ta, D), np.nan, np.float32)
    Bm = np.full((len(pairs), Tb, D), np.nan, np.float32)
    for k, (a, b) in enumerate(pairs):
        A[k, :len(a)], Bm[k, :len(b)] = a, b
    la = torch.tensor([len(a) for a, _ in pairs], dtype=torch.int32).cuda()
    lb = torch.tensor([len(b) for _, b in pairs], dtype=torch.int32).cuda()
    out = mg.dtw(torch.from_numpy(A).cuda(), torch.from_numpy(Bm).cuda(), la, lb, return_path=return_path)
    return tuple(None if o is None else o.cpu().numpy() for o in (out if return_path else out + (None,)))


def check_pair(total, path_len, path, a, b, ref, what):
    n, m = len(a), len(b)
    bar = R.total_bar(n, m, ref)
    print("%s: total %.9g ref %.9g |diff| %.3g bar %.3g path_len %d" % (what, total, ref, abs(total - ref), bar, path_len))
    assert abs(float(total) - ref) <= bar, what
    assert path.shape == (path.shape[0], 2) and path_len == int((path[:, 0] >= 0).sum()), what
    assert (path[path_len:] == -1).all() and (path[:path_len] >= 0).all(), what
    R.check_path(path[:path_len], n, m)
    cost = R.path_cost(a, b, path[:path_len])
    print("%s: float64 cost of the kernel's path %.12g, optimum %.12g" % (what, cost, ref))
    assert ref - 1e-9 * ref <= cost <= ref + bar, what


# ------------------------------------------------------------------ cepstra
@pytest.mark.parametrize("n_coef", [1, 13])
@pytest.mark.parametrize("B,T,M,lens", [(1, 1, 80, [1]), (3, 37, 80, [37, 20, 1]), (2, 130, 20, [130, 65])])
def test_cepstra_match_float64(B, T, M, lens, n_coef):
    check_cepstra(B, T, M, lens, n_coef)


def test_cepstra_at_the_documented_limit():
    """M = 128 bins and n_coef = 127: the largest cosine table the kernel keeps in LDS (65024 bytes)."""
    check_cepstra(2, 70, 128, [70, 3], 127)


def check_cepstra(B, T, M, lens, n_coef):
    import mixgan_tts_amd as mg
    rng = np.random.default_rng(100 * T + M)
    mel = np.stack([R.random_walk_mel(rng, T, M) for _ in range(B)])
    ref = R.cepstra(mel, lens, n_coef)
    live = np.arange(T)[None, :] < np.array(lens)[:, None]
    mel[~live] = np.nan      # nothing at or past a row's length is read
    out = mg.mel_cepstra(torch.from_numpy(mel).cuda(), torch.tensor(lens).cuda(), n_coef).cpu().numpy()
    assert out.shape == (B, T, n_coef) and out.dtype == np.float32
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    print("cepstra B=%d T=%d M=%d n_coef=%d: max err %.3g of max abs %.3g" % (B, T, M, n_coef, err, scale))
    assert err <= 1e-5 * scale
    assert not out[~live].any()
    if min(lens) == T:
        full = mg.mel_cepstra(torch.from_numpy(mel).cuda(), None, n_coef).cpu().numpy()
        assert np.array_equal(full, out)


# ------------------------------------------------------------------ DTW against float64
@pytest.mark.parametrize("D", R.DTW_FEATURES)
def test_dtw_total_and_path_match_float64(D):
    for Ta, Tb in R.DTW_SHAPES:
        a, b, ref = case(Ta, Tb, D)
        total, path_len, path = run_dtw([(a, b)])
        assert path.shape == (1, Ta + Tb - 1, 2)
        check_pair(total[0], path_len[0], path[0], a, b, ref, "D=%d (%d, %d)" % (D, Ta, Tb))


@pytest.mark.parametrize("D", R.DTW_FEATURES)
def test_dtw_ragged_batch(D):
    shapes = [(63, 65), (37, 130), (300, 270), (5, 1)]
    cases = [case(Ta, Tb, D) for Ta, Tb in shapes]
    total, path_len, path = run_dtw([(a, b) for a, b, _ in cases], Ta=320, Tb=290)
    for k, (a, b, ref) in enumerate(cases):
        check_pair(total[k], path_len[k], path[k], a, b, ref, "D=%d ragged %s" % (D, shapes[k]))


@pytest.mark.parametrize("Ta,Tb", R.DTW_LONG_SHAPES)
def test_dtw_with_several_rows_per_thread(Ta, Tb):
    """Ta > 1024: the workgroup has 1024 threads and thread tid owns the rows tid + 1024 r.  (1100, 40): two live rows
    for some threads; (2100, 17): three; (40, 1100): the long side is b and every thread owns one row; (1100, 900): a
    path that warps for real across row 1024."""
    a, b, ref = case(Ta, Tb)
    total, path_len, path = run_dtw([(a, b)])
    assert path.shape == (1, Ta + Tb - 1, 2)
    check_pair(total[0], path_len[0], path[0], a, b, ref, "(%d, %d)" % (Ta, Tb))


def test_dtw_long_ragged_batch():
    """The long shapes under one padding, beside a short pair: rows past a pair's length stay idle."""
    shapes = R.DTW_LONG_SHAPES + [(63, 65)]
    cases = [case(Ta, Tb) for Ta, Tb in shapes]
    total, path_len, path = run_dtw([(a, b) for a, b, _ in cases], Ta=2111, Tb=1101)
    for k, (a, b, ref) in enumerate(cases):
        check_pair(total[k], path_len[k], path[k], a, b, ref, "long ragged %s" % (shapes[k],))
        alone = run_dtw([(a, b)])
        n = alone[1][0]
        assert alone[0][0].tobytes() == total[k].tobytes() and n == path_len[k]
        assert np.array_equal(alone[2][0][:n], path[k][:n])


def test_one_large_pair():
    """About 2100 anti-diagonals: the rolling diagonals hold up, and a thread's column passes many word boundaries."""
    a, b, ref = case(1000, 1100)
    total, path_len, path = run_dtw([(a, b)])
    check_pair(total[0], path_len[0], path[0], a, b, ref, "(1000, 1100)")


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("T", [1, 64, 300, 1100])
def test_self_alignment_is_the_diagonal(T):
    a = case(T, T)[0] if T in (1, 64) else case(T, {300: 270, 1100: 40}[T])[0]
    total, path_len, path = run_dtw([(a, a)])
    assert total[0] == 0.0 and path_len[0] == T
    assert path[0, :T].tolist() == [[t, t] for t in range(T)] and (path[0, T:] == -1).all()


def test_repeated_frames_cost_nothing():
    a, b = R.repeated_copy(11, 1100)      # more rows than the workgroup has threads
    assert len(a) > 1024 and len(b) > len(a)
    total, path_len, path = run_dtw([(a, b)])
    assert total[0] == 0.0 and path_len[0] == len(b)
    R.check_path(path[0, :path_len[0]], len(a), len(b))
    assert R.path_cost(a, b, path[0, :path_len[0]]) == 0.0


# ------------------------------------------------------------------ determinism, empty pairs
def test_dtw_is_deterministic_and_independent_of_batch_position():
    a, b, _ = case(300, 270)
    others = [case(63, 65)[:2], case(37, 130)[:2], case(64, 64)[:2]]
    alone = run_dtw([(a, b)])
    again = run_dtw([(a, b)])
    for x, y in zip(alone, again):
        assert x.tobytes() == y.tobytes()
    batch = run_dtw(others + [(a, b)], Ta=333, Tb=301)
    assert batch[0][3].tobytes() == alone[0][0].tobytes() and batch[1][3] == alone[1][0]
    n = alone[1][0]
    assert np.array_equal(batch[2][3][:n], alone[2][0][:n]) and (batch[2][3][n:] == -1).all()
    # and a pair some of whose threads own two rows, alone and at position 3 under a padding of 2100 rows
    a2, b2, _ = case(1100, 40)
    alone2 = run_dtw([(a2, b2)])
    batch2 = run_dtw(others + [(a2, b2)], Ta=2100, Tb=131)
    n2 = alone2[1][0]
    assert batch2[0][3].tobytes() == alone2[0][0].tobytes() and batch2[1][3] == n2
    assert np.array_equal(batch2[2][3][:n2], alone2[2][0][:n2]) and (batch2[2][3][n2:] == -1).all()
    no_path = run_dtw(others + [(a, b)], Ta=333, Tb=301, return_path=False)
    assert no_path[2] is None
    assert no_path[0].tobytes() == batch[0].tobytes() and np.array_equal(no_path[1], batch[1])


def test_empty_pairs_inside_a_batch():
    a, b, ref = case(63, 65)
    empty_a, empty_b = a[:0], b[:0]
    total, path_len, path = run_dtw([(empty_a, b), (a, b), (a, empty_b), (empty_a, empty_b)], Ta=70, Tb=66)
    assert total[[0, 2, 3]].tolist() == [0.0, 0.0, 0.0] and path_len[[0, 2, 3]].tolist() == [0, 0, 0]
    assert (path[[0, 2, 3]] == -1).all()
    check_pair(total[1], path_len[1], path[1], a, b, ref, "between empty pairs")
    alone = run_dtw([(a, b)])
    assert alone[0][0].tobytes() == total[1].tobytes() and alone[1][0] == path_len[1]


# ------------------------------------------------------------------ MCD and F0
def _mel_pairs():
    """Two utterances: the recording's log-mel and a time-warped, perturbed copy of it, NaN past the lengths."""
    rng = np.random.default_rng(77)
    lens_r, lens_s = [90, 61], [104, 57]
    ref = np.full((2, 90, 80), np.nan, np.float32)
    syn = np.full((2, 104, 80), np.nan, np.float32)
    for k in range(2):
        m = R.random_walk_mel(rng, lens_r[k])
        ref[k, :lens_r[k]] = m
        syn[k, :lens_s[k]] = m[R.warp_index(rng, lens_r[k], lens_s[k])] + rng.normal(0.0, 0.3, (lens_s[k], 80))
    return ref, syn, lens_r, lens_s


def test_mcd_is_the_formula_on_the_kernels_total():
    import mixgan_tts_amd as mg
    ref, syn, lens_r, lens_s = _mel_pairs()
    ref_d, syn_d = torch.from_numpy(ref).cuda(), torch.from_numpy(syn).cuda()
    lr, ls = torch.tensor(lens_r).cuda(), torch.tensor(lens_s).cuda()
    mcd, path, path_len = mg.mel_cepstral_distortion(ref_d, syn_d, lr, ls, return_path=True)
    c_r, c_s = mg.mel_cepstra(ref_d, lr), mg.mel_cepstra(syn_d, ls)
    total, pl, p = mg.dtw(c_r, c_s, lr, ls, return_path=True)
    assert torch.equal(pl, path_len) and torch.equal(p, path)
    want = R.mcd(total.double().cpu().numpy(), pl.cpu().numpy())
    np.testing.assert_allclose(mcd.cpu().numpy(), want, rtol=1e-6)
    assert torch.equal(mg.mel_cepstral_distortion(ref_d, syn_d, lr, ls), mcd)
    # and against float64 end to end, from the same float32 mels
    for k in range(2):
        cr, cs = R.cepstra(ref[k:k + 1, :lens_r[k]])[0], R.cepstra(syn[k:k + 1, :lens_s[k]])[0]
        t64, _, p64 = R.dtw(cr, cs)
        print("utterance %d: MCD %.6f dB, float64 %.6f dB" % (k, mcd[k].item(), R.mcd(t64, len(p64))))
        assert len(p64) not in (lens_r[k], lens_s[k])
    # the report gives the same figures
    rep = mg.synthesis_report(syn_d, ls, ref_d, lr)
    assert torch.equal(rep["mcd"], mcd) and torch.equal(rep["path"], path) and torch.equal(rep["dtw_total"], total)
    assert rep["mcd_mean"].item() == pytest.approx(mcd.mean().item(), rel=1e-6)


def test_mcd_without_a_warp_matches_float64():
    import mixgan_tts_amd as mg
    ref, _, lens, _ = _mel_pairs()
    rng = np.random.default_rng(78)
    syn = ref + rng.normal(0.0, 0.3, ref.shape).astype(np.float32)
    ref_d, syn_d, ld = torch.from_numpy(ref).cuda(), torch.from_numpy(syn).cuda(), torch.tensor(lens).cuda()
    mcd, path, path_len = mg.mel_cepstral_distortion(ref_d, syn_d, ld, ld, align="none", return_path=True)
    for k in range(2):
        n = lens[k]
        want = R.mcd_framewise(R.cepstra(ref[k:k + 1, :n])[0], R.cepstra(syn[k:k + 1, :n])[0], n)
        print("utterance %d: frame-wise MCD %.7f dB, float64 %.7f dB" % (k, mcd[k].item(), want))
        assert abs(mcd[k].item() - want) <= 1e-5 * want
        assert path_len[k].item() == n and path[k, :n].tolist() == [[t, t] for t in range(n)]
        assert (path[k, n:] == -1).all()
    with pytest.raises(ValueError):
        mg.mel_cepstral_distortion(ref_d, syn_d, ld, ld - 1, align="none")


def test_f0_metrics_on_the_kernels_path():
    import mixgan_tts_amd as mg
    ref, syn, lens_r, lens_s = _mel_pairs()
    lr, ls = torch.tensor(lens_r).cuda(), torch.tensor(lens_s).cuda()
    _, path, path_len = mg.mel_cepstral_distortion(torch.from_numpy(ref).cuda(), torch.from_numpy(syn).cuda(), lr, ls,
                                                   return_path=True)
    rng = np.random.default_rng(79)
    # voiced stretches of 120 .. 260 Hz between unvoiced ones; the reference track is one frame shorter than its mel,
    # so the path's last index is clipped
    f_ref = np.where(np.sin(np.arange(89) / 5.0) > -0.3, 190.0 + 70.0 * np.sin(np.arange(89) / 11.0), 0.0)
    f_ref = np.stack([f_ref, np.roll(f_ref, 17)])
    f_syn = np.where(np.sin(np.arange(105) / 6.0) > -0.2, 200.0 + 60.0 * np.cos(np.arange(105) / 9.0), 0.0)
    f_syn = np.stack([f_syn * rng.uniform(0.9, 1.1, 105), np.roll(f_syn, 5)])
    out = mg.f0_metrics(torch.from_numpy(f_ref), torch.from_numpy(f_syn), path, path_len)
    assert out["f0_rmse_cents"].is_cuda and out["f0_rmse_cents"].dtype == torch.float64
    path_h, n_h = path.cpu().numpy(), path_len.cpu().numpy()
    for k in range(2):
        rmse, vuv = R.f0_figures(f_ref[k], f_syn[k], path_h[k, :n_h[k]])
        print("utterance %d: F0 RMSE %.3f cents, V/UV error %.4f" % (k, rmse, vuv))
        assert 0.0 < vuv < 1.0 and rmse > 0.0
        np.testing.assert_allclose(out["f0_rmse_cents"][k].item(), rmse, rtol=1e-10)
        np.testing.assert_allclose(out["vuv_error"][k].item(), vuv, rtol=1e-12)
    rep = mg.synthesis_report(torch.from_numpy(syn).cuda(), ls, torch.from_numpy(ref).cuda(), lr,
                              pred_f0=torch.from_numpy(f_syn), target_f0=torch.from_numpy(f_ref))
    assert torch.equal(rep["f0_rmse_cents"], out["f0_rmse_cents"]) and torch.equal(rep["vuv_error"], out["vuv_error"])


# ------------------------------------------------------------------ evaluate_model
class ReplayEncoder(torch.nn.Module):
    """Stands in for the linguistic encoder: returns what the reference's encoder returned for the fixture's batch."""

    def __init__(self, outputs):
        super().__init__()
        self.outputs = outputs

    def forward(self, *args, **kwargs):
        return self.outputs


def test_evaluate_model_is_the_report_of_the_models_own_inference(manifest, tmp_path):
    """A random-weight MixGANTTS over the recorded encoder outputs of the inference fixture, as
    tests/test_gpu_mixgantts.py builds it.  No quality claim: the figures are those of noise."""
    import mixgan_tts_amd as mg
    from helpers import golden, T, Tape, hot_path_configs, write_stats, mixgantts_encoder_outputs, mixgantts_tapes
    from oracle import weights as WR
    g = golden("mixgantts_naive_ms0_infer")
    stats = write_stats(tmp_path, np.linspace(-11.5, -9.0, 80), np.linspace(1.0, 2.0, 80), n_speakers=5)
    m = mg.MixGANTTS(*hot_path_configs("naive", 4, stats_dir=stats),
                     linguistic_encoder=ReplayEncoder(mixgantts_encoder_outputs(g, False, "cuda")))
    sd = m.state_dict()
    for k, a in WR.draw(manifest["mixgantts_naive_ms0"]["seeded"], 61).items():
        sd[k] = torch.from_numpy(a)
    m.load_state_dict(sd)
    m = m.cuda().train()
    rng, _ = mixgantts_tapes(g)
    dev = lambda k: T(g[k]).cuda()  # noqa: E731
    tgt_rng = np.random.default_rng(5)
    tgt_lens = [20, 12]
    mels = np.zeros((2, 20, 80), np.float32)
    for k in range(2):
        mels[k, :tgt_lens[k]] = R.random_walk_mel(tgt_rng, tgt_lens[k])
    batch = [["a", "b"], ["", ""], dev("speakers"), dev("texts"), dev("src_lens"), int(g["src_lens"].max()), dev("wb"),
             dev("src_w_lens"), 3, None, None, torch.from_numpy(mels).cuda(), torch.tensor(tgt_lens).cuda(), 20,
             None, None, None]
    m.diffusion.noise_fn = Tape(rng)
    rep = mg.evaluate_model(m, batch, d_control=4.0)
    assert m.training      # restored
    m.eval()
    m.diffusion.noise_fn = Tape(rng)
    with torch.no_grad():
        out = m(*batch[2:9], spker_embeds=None, d_control=4.0)[0]
    want = mg.synthesis_report(out[0], out[11], batch[11], batch[12])
    assert sorted(rep) == sorted(want) and {"mcd", "mcd_mean", "path", "path_len", "dtw_total"} <= set(rep)
    for k in rep:
        assert torch.equal(rep[k], want[k]), k
    assert out[11].tolist() == [8, 16] and rep["mcd"].shape == (2,) and bool(torch.isfinite(rep["mcd"]).all())
    print("MCD of a random-weight model against random targets: %s dB" % rep["mcd"].tolist())
