"""GPU parity of the native audio front end (mixgan-tts_amd/audio.py, csrc/audio.hip) against the reference's
audio package (fixtures of tests/golden/make_golden_audio.py) and, at full size, against the float64 plain-torch
restatement of its conv1d / conv_transpose1d STFT (tests/audio_torch.py)."""
import json
import os

import numpy as np
import pytest
import torch

import audio_torch as AT
from helpers import golden as load_golden, GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


@pytest.fixture(scope="module")
def golden():
    return load_golden("audio")


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "audio_manifest.json")) as f:
        return json.load(f)


def _rel(out, ref):
    dt = np.complex128 if np.iscomplexobj(out) or np.iscomplexobj(ref) else np.float64
    out, ref = np.asarray(out).astype(dt), np.asarray(ref).astype(dt)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert np.isfinite(out).all()
    return float(np.abs(out - ref).max() / np.abs(ref).max())


def _tac(mg, key, hop=256):
    return mg.audio.TacotronSTFT(1024, hop, 1024, 80, 22050, 0.0, 8000 if key == "8000" else None).to(DEV)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_transform_and_forward_match_reference(mg, golden, i):
    stft = mg.audio.STFT(1024, 256, 1024)
    x = torch.from_numpy(golden["x%d" % i])[None].to(DEV)
    mag, phase = stft.transform(x)
    assert mag.device == x.device and phase.device == x.device
    assert mag.shape == (1, 513, 1 + x.shape[1] // 256) == phase.shape
    ours = (mag.double() * torch.exp(1j * phase.double()))[0].cpu().numpy()
    ref = golden["mag%d" % i].astype(np.float64) * np.exp(1j * golden["phase%d" % i].astype(np.float64))
    e = _rel(ours, ref)
    print("spectrum %d: %.2e" % (i, e))
    assert e <= 1e-5
    assert _rel(mag[0].cpu().numpy(), golden["mag%d" % i]) <= 1e-5
    y = stft(x)
    assert y.shape == (1, 1, (mag.shape[-1] - 1) * 256)
    e = _rel(y[0, 0].cpu().numpy(), golden["recon%d" % i])
    print("recon %d: %.2e" % (i, e))
    assert e <= 1e-5


@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("key", ["8000", "none"])
def test_mel_energy_match_reference(mg, golden, i, key):
    tac = _tac(mg, key)
    x = torch.from_numpy(golden["x%d" % i])[None].to(DEV)
    logmel, energy = tac.mel_spectrogram(x)
    ref_log, ref_e = golden["mel%d_%s" % (i, key)], golden["energy%d_%s" % (i, key)]
    assert logmel.shape == (1, 80, ref_log.shape[1]) and energy.shape == (1, ref_e.shape[0])
    e_mel = _rel(np.exp(logmel[0].double().cpu().numpy()), np.exp(ref_log.astype(np.float64)))
    e_en = _rel(energy[0].cpu().numpy(), ref_e)
    big = np.exp(ref_log.astype(np.float64)) >= 1e-2
    e_log = float(np.abs(logmel[0].double().cpu().numpy() - ref_log)[big].max())
    print("mel %d %s: mel %.2e energy %.2e log %.2e" % (i, key, e_mel, e_en, e_log))
    assert e_mel <= 1e-5 and e_en <= 1e-5 and e_log <= 1e-4
    # get_mel_from_wav: numpy in, numpy float32 out, same values
    m2, en2 = mg.audio.get_mel_from_wav(golden["x%d" % i], tac)
    assert m2.dtype == np.float32 and np.array_equal(m2, logmel[0].cpu().numpy())
    assert np.array_equal(en2, energy[0].cpu().numpy())


def test_window_sumsquare_matches_reference(mg, golden, manifest):
    """The host envelope, and the kernel's own (evaluated in-kernel): frames of all ones through the inverse give
    sum_t w[n - t hop] / wss[n], so with the reference's envelope the inverse of the spectrum of a window-free frame
    is reproduced; here the transform of a constant signal must invert to that constant."""
    T = manifest["wss_frames"]
    ws = mg.audio.window_sumsquare("hann", T, 256, 1024, 1024)
    assert _rel(ws, golden["wss"]) <= 1e-5
    stft = mg.audio.STFT(1024, 256, 1024)
    x = torch.full((1, (T - 1) * 256), 0.5, device=DEV)
    y = stft(x)
    assert _rel(y[0, 0].cpu().numpy(), np.full((T - 1) * 256, 0.5)) <= 1e-5


def test_griffin_lim_matches_reference(mg, golden, manifest):
    stft = mg.audio.STFT(1024, 256, 1024)
    spec = torch.from_numpy(golden["gl_spec"])[None].to(DEV)
    ang = torch.from_numpy(golden["gl_angles"])[None].to(DEV)
    y4 = mg.audio.griffin_lim(spec, stft, 4, angles=ang)
    assert y4.shape == golden["gl4"][None].shape
    e = _rel(y4[0].cpu().numpy(), golden["gl4"])
    print("griffin-lim 4: %.2e" % e)
    assert e <= 1e-4
    y60 = mg.audio.griffin_lim(spec, stft, 60, angles=ang)
    mag, _ = stft.transform(y60)
    sc = float(torch.norm(mag.double() - spec.double()) / torch.norm(spec.double()))
    ref = manifest["gl60_spectral_convergence"]
    print("griffin-lim 60: spectral convergence %.5f (reference %.5f)" % (sc, ref))
    assert abs(sc - ref) <= 0.01 * ref


def test_mel_to_audio_matches_reference_spectrum(mg, golden):
    """mel_to_audio's projection equals inv_mel_spec's spectrum, then Griffin-Lim as above."""
    tac = _tac(mg, "8000")
    mel = torch.from_numpy(golden["mel0_8000"])[None].to(DEV)
    ang = torch.from_numpy(golden["gl_angles"])[None].to(DEV)
    y = mg.audio.mel_to_audio(mel, tac, griffin_iters=4, angles=ang)
    e = _rel(y[0].cpu().numpy(), golden["gl4"])
    print("mel_to_audio 4: %.2e" % e)
    assert e <= 1e-4


@pytest.mark.parametrize("hop", [256, 128])
def test_full_size_against_torch_restatement(mg, hop):
    B, N = 16, 256000
    g = torch.Generator().manual_seed(hop)
    t = torch.arange(N, dtype=torch.float64) / 22050
    f = torch.rand(B, 1, generator=g, dtype=torch.float64) * 300 + 100
    x = (0.5 * torch.sin(2 * np.pi * f * t * (1 + t / 20)) + 0.1 * torch.randn(B, N, generator=g, dtype=torch.float64))
    x = x.clamp(-1, 1).float()
    xd = x.to(DEV)
    ref = AT.TorchSTFT(hop, device=DEV)
    tac = _tac(mg, "8000", hop)
    mag, phase = tac.stft_fn.transform(xd)
    rmag, rph, re, im = ref.transform(xd)
    ours = torch.complex(mag.double() * torch.cos(phase.double()), mag.double() * torch.sin(phase.double()))
    e_spec = float((ours - torch.complex(re, im)).abs().max() / torch.complex(re, im).abs().max())
    logmel, energy = tac.mel_spectrogram(xd)
    rlog, ren, rmel = ref.mel_energy(xd, tac.mel_basis)
    e_mel = float((logmel.double().exp() - rmel.clamp(min=1e-5)).abs().max() / rmel.abs().max())
    e_en = float((energy.double() - ren).abs().max() / ren.abs().max())
    big = rmel >= 1e-2
    e_log = float((logmel.double() - rlog).abs()[big].max())
    y = tac.stft_fn.inverse(mag, phase)
    ry = ref.inverse(rmag, rph)
    e_rec = float((y.double() - ry).abs().max() / ry.abs().max())
    print("B=16 N=256000 hop=%d: spectrum %.2e mel %.2e energy %.2e log %.2e recon %.2e"
          % (hop, e_spec, e_mel, e_en, e_log, e_rec))
    assert e_spec <= 1e-5 and e_mel <= 1e-5 and e_en <= 1e-5 and e_log <= 1e-4 and e_rec <= 1e-5


def test_ragged_batch_bit_identical_to_single_items(mg):
    tac = _tac(mg, "8000")
    lens = [11025, 5000, 600, 4097, 8192, 513]
    L = max(lens) + 300
    g = torch.Generator().manual_seed(7)
    x = torch.zeros(len(lens), L)
    for b, n in enumerate(lens):
        x[b, :n] = (torch.rand(n, generator=g) * 2 - 1) * 0.9
    mel, en = tac.mel_spectrogram(x.to(DEV), lengths=torch.tensor(lens))
    T = 1 + max(lens) // 256
    assert mel.shape == (len(lens), 80, T) and en.shape == (len(lens), T)
    for b, n in enumerate(lens):
        m1, e1 = tac.mel_spectrogram(x[b:b + 1, :n].to(DEV))
        Tb = m1.shape[-1]
        assert torch.equal(mel[b, :, :Tb], m1[0]), b
        assert torch.equal(en[b, :Tb], e1[0]), b
        assert not mel[b, :, Tb:].any() and not en[b, Tb:].any()


def test_griffin_lim_graph_capture_replays_bit_identical(mg):
    stft = mg.audio.STFT(1024, 256, 1024)
    g = torch.Generator().manual_seed(3)
    spec = (torch.rand(2, 513, 40, generator=g) * 4).to(DEV)
    ang = ((torch.rand(2, 513, 40, generator=g) * 2 - 1) * np.pi).to(DEV)
    eager = mg.audio.griffin_lim(spec, stft, 8, angles=ang)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mg.audio.griffin_lim(spec, stft, 8, angles=ang)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mg.audio.griffin_lim(spec, stft, 8, angles=ang)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_griffin_lim_random_angles_on_device(mg):
    stft = mg.audio.STFT(1024, 256, 1024)
    spec = torch.rand(1, 513, 12, device=DEV)
    y = mg.audio.griffin_lim(spec, stft, 2)
    assert y.device.type == "cuda" and y.shape == (1, 11 * 256) and torch.isfinite(y).all()


def test_inv_mel_spec_writes_wav(mg, golden, tmp_path):
    wavfile = pytest.importorskip("scipy.io.wavfile")
    tac = _tac(mg, "8000")
    mel = torch.from_numpy(golden["mel0_8000"]).to(DEV)
    path = str(tmp_path / "gl.wav")
    mg.audio.inv_mel_spec(mel, path, tac, griffin_iters=3)
    sr, data = wavfile.read(path)
    assert sr == 22050 and data.dtype == np.float32
    assert data.shape == ((mel.shape[1] - 2) * 256,)


def test_out_of_range_input_asserts(mg):
    tac = _tac(mg, "8000")
    x = torch.zeros(1, 2000, device=DEV)
    x[0, 17] = 1.0001
    with pytest.raises(AssertionError):
        tac.mel_spectrogram(x)
    with pytest.raises(ValueError):
        tac.mel_spectrogram(torch.zeros(1, 512, device=DEV))
