"""The float64 restatement of the synthesis metrics (tests/metrics_ref.py) against known answers, the seeded inputs of
tests/test_gpu_metrics.py, and the argument checks mixgan_tts_amd.metrics makes before it touches the library."""
import numpy as np
import pytest
import torch

import metrics_ref as R


def test_dct_rows_are_orthonormal():
    for M, n_coef in ((80, 13), (80, 79), (20, 1), (128, 127)):
        C = R.dct_rows(M, n_coef)
        np.testing.assert_allclose(C @ C.T, np.eye(n_coef), atol=1e-12)
        # c0 is left out: every row sums to zero over the bins, so a frame's level does not reach the cepstra
        np.testing.assert_allclose(C.sum(1), 0.0, atol=1e-12)
    mel = R.random_walk_mel(np.random.default_rng(3), 5)[None]
    c = R.cepstra(mel, [3], 13)
    assert c.shape == (1, 5, 13) and not c[0, 3:].any() and c[0, :3].any()
    np.testing.assert_allclose(R.cepstra(mel + 2.5, [3], 13), c, atol=1e-10)


def test_dtw_of_a_sequence_against_itself():
    for T, D in ((1, 13), (7, 1), (40, 13)):
        a, _ = R.warped_pair(5, T, T, D)
        total, Dacc, path = R.dtw(a, a)
        assert total == 0.0 and Dacc.shape == (T, T)
        assert path.tolist() == [[t, t] for t in range(T)]
        assert R.path_cost(a, a, path) == 0.0


def test_dtw_of_a_copy_with_repeated_frames():
    for seed in (1, 2, 3):
        a, b = R.repeated_copy(seed, 30)
        assert len(b) > len(a)
        total, _, path = R.dtw(a, b)
        assert total == 0.0 and len(path) == len(b)
        R.check_path(path, len(a), len(b))
        assert R.path_cost(a, b, path) == 0.0


def test_vectorised_and_cell_by_cell_dtw_agree():
    for Ta, Tb in ((1, 5), (5, 1), (37, 20), (20, 33)):
        a, b = R.warped_pair(R.pair_seed(Ta, Tb, 13), Ta, Tb)
        total, Dacc, path = R.dtw(a, b)
        total2, path2 = R.dtw_loops(a, b)
        assert total == total2 and path.tolist() == path2.tolist()
        R.check_path(path, Ta, Tb)
        np.testing.assert_allclose(R.path_cost(a, b, path), total, rtol=1e-13)
    # the tie rule on a hand-made case: all costs equal, so every route costs by its length and the ties decide
    z = np.zeros((3, 1))
    assert R.dtw(z, np.zeros((2, 1)))[2].tolist() == [[0, 0], [1, 0], [2, 1]]
    assert R.dtw(np.zeros((2, 1)), z)[2].tolist() == [[0, 0], [0, 1], [1, 2]]


def test_the_gpu_tests_inputs_warp():
    """Independent random walks give an almost pure diagonal and would hide a wrong predecessor: on the committed
    seeds the optimal path must be longer than both sides in at least one case, and use all three moves."""
    warped, moves = 0, set()
    for Ta, Tb in R.DTW_SHAPES:
        a, b = R.warped_pair(R.pair_seed(Ta, Tb, 13), Ta, Tb)
        assert a.shape == (Ta, 13) and b.shape == (Tb, 13) and a.dtype == b.dtype == np.float32
        _, _, path = R.dtw(a, b)
        R.check_path(path, Ta, Tb)
        warped += len(path) not in (Ta, Tb)
        moves |= {tuple(s) for s in np.diff(path, axis=0).tolist()}
    assert warped >= 3 and moves == {(1, 1), (1, 0), (0, 1)}


def test_f0_figures_on_a_hand_made_path():
    f_ref = np.array([0.0, 100.0, 200.0, 0.0])
    f_syn = np.array([100.0, 200.0, 0.0])
    path = np.array([[0, 0], [1, 0], [1, 1], [2, 1], [3, 2], [4, 3]])      # the last cell is clipped to (3, 2)
    # cells: (0,100) differs; (100,100) 0 cents; (100,200) 1200; (200,200) 0; (0,0) both unvoiced; (0,0)
    rmse, vuv = R.f0_figures(f_ref, f_syn, path)
    assert vuv == pytest.approx(1 / 6) and rmse == pytest.approx(np.sqrt(1200.0 ** 2 / 3))
    rmse, vuv = R.f0_figures(np.zeros(3), f_syn, path[:3])
    assert np.isnan(rmse) and vuv == 1.0
    assert R.mcd(3.0, 2) == pytest.approx(10 / np.log(10) * np.sqrt(2) * 1.5)


def test_python_checks_come_before_the_library(monkeypatch):
    import mixgan_tts_amd as mg
    from mixgan_tts_amd import _lib, metrics

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", touched)
    assert issubclass(mg.DtwGeometryError, mg.MixganHipError) and issubclass(mg.DtwGeometryError, NotImplementedError)
    assert (metrics.MAX_T, metrics.MAX_D, metrics.MAX_M) == (4096, 64, 128)
    z = torch.zeros
    for a, b in ((z(1, 4097, 13), z(1, 5, 13)), (z(1, 5, 13), z(1, 4097, 13)), (z(1, 5, 65), z(1, 5, 65)),
                 (z(0, 5, 13), z(0, 5, 13)), (z(1, 0, 13), z(1, 5, 13)), (z(1, 5, 0), z(1, 5, 0))):
        with pytest.raises(mg.DtwGeometryError):
            mg.dtw(a, b)
    for mel, n_coef in ((z(1, 4, 129), 13), (z(1, 4, 80), 80), (z(1, 4, 80), 0), (z(1, 0, 80), 13), (z(1, 4, 1), 1)):
        with pytest.raises(mg.DtwGeometryError):
            mg.mel_cepstra(mel, n_coef=n_coef)
    with pytest.raises(mg.DtwGeometryError):
        mg.mel_cepstral_distortion(z(1, 4097, 80), z(1, 10, 80))
    with pytest.raises(ValueError):
        mg.dtw(z(1, 5, 13), z(2, 5, 13))
    with pytest.raises(ValueError):
        mg.dtw(z(1, 5, 13), z(1, 5, 12))
    with pytest.raises(ValueError):
        mg.dtw(z(5, 13), z(5, 13))
    with pytest.raises(ValueError):
        mg.dtw(z(2, 5, 13), z(2, 5, 13), a_lens=z(3))
    with pytest.raises(ValueError):
        mg.mel_cepstra(z(4, 80))
    with pytest.raises(ValueError):
        mg.mel_cepstra(z(2, 4, 80), lengths=z(3))
    with pytest.raises(ValueError):
        mg.mel_cepstral_distortion(z(1, 4, 80), z(1, 5, 80), align="none")
    with pytest.raises(ValueError):
        mg.mel_cepstral_distortion(z(1, 4, 80), z(1, 4, 80), align="linear")
    with pytest.raises(ValueError):
        mg.synthesis_report(z(1, 4, 80), None, z(1, 4, 80), None, pred_f0=z(1, 4))
    # valid shapes on the host: there is no CPU fallback
    with pytest.raises(mg.MixganHipError):
        mg.dtw(z(1, 5, 13), z(1, 5, 13))
    with pytest.raises(mg.MixganHipError):
        mg.mel_cepstra(z(1, 4, 80))


def test_f0_metrics_on_the_host_matches_the_restatement():
    """f0_metrics is plain torch on the path's device: on a hand-made path it equals the float64 figures."""
    import mixgan_tts_amd as mg
    f_ref = torch.tensor([[0.0, 100.0, 200.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    f_syn = torch.tensor([[100.0, 200.0, 0.0], [110.0, 0.0, 0.0]])
    path = torch.tensor([[[0, 0], [1, 0], [1, 1], [2, 1], [3, 2], [4, 3]],
                         [[0, 0], [1, 1], [2, 2], [-1, -1], [-1, -1], [-1, -1]]], dtype=torch.int32)
    path_len = torch.tensor([6, 3], dtype=torch.int32)
    out = mg.f0_metrics(f_ref, f_syn, path, path_len)
    for b in range(2):
        rmse, vuv = R.f0_figures(f_ref[b].numpy(), f_syn[b].numpy(), path[b, :path_len[b]].numpy())
        np.testing.assert_allclose(out["f0_rmse_cents"][b].item(), rmse, rtol=1e-12, equal_nan=True)
        np.testing.assert_allclose(out["vuv_error"][b].item(), vuv, rtol=1e-12)
    assert torch.isnan(out["f0_rmse_cents"][1]) and out["vuv_error"][1].item() == pytest.approx(1 / 3)
