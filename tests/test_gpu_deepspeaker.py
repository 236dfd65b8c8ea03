"""DeepSpeaker speaker embedder on the HIP path (csrc/deepspeaker.hip): the fbank front end against the real
reference's model inputs (tests/golden/deepspeaker.npz) and the restatement on a ragged batch, the 2-D convolution
against float64 F.conv2d for every layer shape of the net, the whole model against the float64 restatement
(tests/deepspeaker_ref.py, calibrated seeded weights), batch independence, PreDefinedEmbedder and the multi-speaker
MixGANTTS path fed from save_speaker_embeddings.  Bar: max |err| / max |ref| <= 1e-3."""
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deepspeaker_ref as R
from helpers import golden, GOLDEN, T, hot_path_configs, write_stats, mixgantts_encoder_outputs

import mixgan_tts_amd as mg
from mixgan_tts_amd import speaker_embedder as S

pytestmark = pytest.mark.gpu
TOL = 1e-3


def _rel(got, ref, what):
    got, ref = got.double().cpu(), torch.as_tensor(ref).double().cpu()
    err = float((got - ref).abs().max() / ref.abs().max())
    print("%s: max-abs err / max-abs ref = %.3e" % (what, err))
    assert err <= TOL, (what, err)
    return err


def _batch(signals):
    L = max(len(x) for x in signals)
    a = torch.zeros(len(signals), L)
    for i, x in enumerate(signals):
        a[i, :len(x)] = torch.from_numpy(np.asarray(x, np.float32))
    return a.cuda(), [len(x) for x in signals]


def _utterances(n, seconds=3.0, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        L = int(seconds * R.SR * rng.uniform(0.5, 1.0))
        t = np.arange(L) / R.SR
        f0 = rng.uniform(90, 300)
        v = sum(np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6)) / h for h in range(1, 10))
        v = v * (0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(1, 5) * t)) + 0.3 * rng.standard_normal(L)
        m = int(0.1 * R.SR)
        v[:m] *= 1e-3
        v[-m:] *= 1e-3
        out.append((0.3 * v / np.abs(v).max()).astype(np.float32))
    return out


@pytest.fixture(scope="module")
def model():
    return S.DeepSpeakerModel().load_keras_weights(R.seeded_weights())


def test_fbank_matches_reference_fixture(model):
    g = golden("deepspeaker")
    with open(os.path.join(GOLDEN, "deepspeaker_manifest.json")) as f:
        man = json.load(f)
    audio, lens = _batch([g[s["name"]] for s in man["signals"]])
    random.seed(man["seed"])
    feats, start, end, nfr, offsets = model.frontend(audio, lens)
    for i, s in enumerate(man["signals"]):
        assert (start[i], end[i], nfr[i]) == (s["start"], s["end"], s["frames"])
        assert offsets[i] == max(s["offset"], 0)
        _rel(feats[i], g[s["name"] + "_input"][:, :, 0], "fbank vs reference " + s["name"])
        if s["frames"] < 160:
            assert not feats[i, s["frames"]:].any()


def test_fbank_matches_restatement_ragged(model):
    sig = _utterances(6, 2.5, seed=9)
    sig[2] = sig[2][:5000]  # about 20 frames after the trim
    sig[4] = sig[4][:900]   # a single frame
    audio, lens = _batch(sig)
    feats, start, end, nfr, offsets = model.frontend(audio, lens)
    for i, x in enumerate(sig):
        assert (start[i], end[i]) == R.trim(x)
        _rel(feats[i], R.model_input(x, offsets[i]), "fbank vs restatement item %d (%d frames)" % (i, nfr[i]))
        assert not feats[i, nfr[i]:].any()


CONV_SHAPES = [(1, 64, 5, 2), (64, 64, 3, 1), (64, 128, 5, 2), (128, 128, 3, 1), (128, 256, 5, 2), (256, 256, 3, 1),
               (256, 512, 5, 2), (512, 512, 3, 1)]


@pytest.mark.parametrize("ci,co,k,s", CONV_SHAPES)
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("N,H,W", [(3, 13, 7), (2, 20, 9)])
def test_conv2d_matches_float64(ci, co, k, s, residual, N, H, W):
    g = torch.Generator().manual_seed(ci * 7 + co + k + H)
    x = torch.rand(N, H, W, ci, generator=g, dtype=torch.float64) * 2
    w = (torch.rand(k, k, ci, co, generator=g, dtype=torch.float64) - 0.5) * (2.0 / (k * (ci ** 0.5)))
    b = torch.rand(co, generator=g, dtype=torch.float64) - 0.3
    Ho, pt, pb = S.tf_same_padding(H, k, s)
    Wo, pl, pr = S.tf_same_padding(W, k, s)
    res = torch.rand(N, Ho, Wo, co, generator=g, dtype=torch.float64) * 4 - 1 if residual else None
    ref = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb)), w.permute(3, 2, 0, 1), b, stride=s)
    ref = ref.permute(0, 2, 3, 1).clamp(0, 20)
    if residual:
        ref = (ref + res).clamp(0, 20)
    y, ho, wo = S.conv2d_same(x.float().cuda(), w.reshape(k * k * ci, co).float().cuda().contiguous(),
                              b.float().cuda(), N, H, W, ci, co, k, s,
                              res.float().cuda() if residual else None)
    assert (ho, wo) == (Ho, Wo)
    _rel(y, ref, "conv ci=%d co=%d k=%d s=%d res=%d N=%d H=%d W=%d" % (ci, co, k, s, residual, N, H, W))


@pytest.mark.parametrize("N", [1, 5, 64])
def test_embed_matches_restatement(model, N):
    sig = _utterances(N, seed=N)
    audio, lens = _batch(sig)
    feats, start, end, nfr, offsets = model.frontend(audio, lens)
    emb = model.embed(audio, lens, offsets)
    assert emb.shape == (N, 512) and emb.dtype == torch.float32 and emb.is_cuda
    inputs = np.stack([R.model_input(x, o) for x, o in zip(sig, offsets)])
    ref = R.rescnn(torch.from_numpy(inputs).cuda(), R.seeded_weights())
    _rel(emb, ref, "embed N=%d" % N)
    _rel(model.network(torch.from_numpy(inputs).cuda()), ref, "network on restated inputs N=%d" % N)
    np.testing.assert_allclose(emb.norm(dim=1).cpu().numpy(), 1.0, atol=1e-5)


def test_embed_is_batch_independent_bitwise(model):
    sig = _utterances(7, seed=21)
    audio, lens = _batch(sig)
    offsets = model.frontend(audio, lens)[4]
    full = model.embed(audio, lens, offsets)
    one, l1 = _batch([sig[3]])
    alone = model.embed(one, l1, offsets[3:4])
    assert torch.equal(full[3:4], alone)
    small = S.DeepSpeakerModel(chunk=2).load_keras_weights(R.seeded_weights())
    assert torch.equal(small.embed(audio, lens, offsets), full)


def test_embed_draws_offsets_like_the_reference(model):
    sig = _utterances(4, seed=2)
    audio, lens = _batch(sig)
    random.seed(77)
    _, start, end, nfr, offsets = model.frontend(audio, lens)
    random.seed(77)
    expect = [random.choice(range(0, n - 160 + 1)) if n >= 160 else 0 for n in nfr]
    assert offsets == expect
    random.seed(77)
    a = model.embed(audio, lens)
    assert torch.equal(a, model.embed(audio, lens, expect))


def test_silent_utterance_raises(model):
    audio, lens = _batch([np.zeros(5000, np.float32), _utterances(1)[0]])
    with pytest.raises(ValueError, match="utterance 0"):
        model.embed(audio, lens)


def _config(tmp_path):
    return {"preprocessing": {"audio": {"sampling_rate": 22050}, "stft": {"win_length": 1024},
                              "speaker_embedder": "DeepSpeaker", "speaker_embedder_cuda": False}}


def test_predefined_embedder(tmp_path, monkeypatch):
    cfg = _config(tmp_path)
    with pytest.raises(S.DeepSpeakerCheckpointRequired):
        S.PreDefinedEmbedder(cfg, checkpoint_path=str(tmp_path / "absent.h5"))
    ckpt = tmp_path / "weights.h5"
    ckpt.write_bytes(b"")
    monkeypatch.setattr(S.DeepSpeakerModel, "from_h5", classmethod(
        lambda cls, path, **kw: cls(**kw).load_keras_weights(R.seeded_weights())))
    emb = mg.PreDefinedEmbedder(cfg, checkpoint_path=str(ckpt))
    wav = _utterances(1, seed=3)[0]
    random.seed(5)
    out = emb(wav)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (1, 512)
    random.seed(5)
    out64 = emb(wav.astype(np.float64))  # a float64 wav trims in float64, as numpy would
    assert out64.dtype == np.float32 and out64.shape == (1, 512)
    random.seed(5)
    s, e = R.trim(wav)
    n = S.num_frames(e - s, 551, 221)
    o = random.choice(range(0, n - 159)) if n >= 160 else 0
    ref = R.rescnn(torch.from_numpy(R.model_input(wav, o)[None]), R.seeded_weights())
    _rel(torch.from_numpy(out), ref, "PreDefinedEmbedder.forward")


def test_multispeaker_mixgantts_runs_on_saved_embeddings(model, tmp_path):
    g = golden("mixgantts_naive_ms0_infer")
    B = int(g["src_lens"].shape[0])
    stats = write_stats(tmp_path, np.linspace(-11.5, -9.0, 80), np.linspace(1.0, 2.0, 80), n_speakers=B)
    sig = _utterances(2 * B, seed=13)
    audio, lens = _batch(sig)
    emb = model.embed(audio, lens, [0] * (2 * B)).cpu()
    for i in range(B):
        mg.save_speaker_embeddings(str(tmp_path), "spk%d" % i, [emb[2 * i:2 * i + 1], emb[2 * i + 1:2 * i + 2]])
    loaded = np.concatenate([np.load(os.path.join(str(tmp_path), "spker_embed", "spk%d-spker_embed.npy" % i),
                                     allow_pickle=False) for i in range(B)])
    assert loaded.shape == (B, 512) and loaded.dtype == np.float32
    args, pre, mc, tr = hot_path_configs("naive", 4, multi_speaker=True, stats_dir=stats)
    pre["preprocessing"]["speaker_embedder"] = "DeepSpeaker"
    mc["external_speaker_dim"] = 512

    class Replay(torch.nn.Module):
        def __init__(self, outputs):
            super().__init__()
            self.outputs = outputs

        def forward(self, *a, **k):
            return self.outputs

    enc = mixgantts_encoder_outputs(g, False, "cuda")
    m = mg.MixGANTTS(args, pre, mc, tr, linguistic_encoder=Replay(enc)).cuda().eval()
    assert isinstance(m.speaker_emb, torch.nn.Linear) and m.speaker_emb.in_features == 512
    dev = lambda k: T(g[k]).cuda()  # noqa: E731

    gen = torch.Generator(device="cuda").manual_seed(0)
    m.diffusion.noise_fn = lambda shape: torch.randn(shape, generator=gen, device="cuda")
    spk = torch.from_numpy(loaded).cuda()
    with torch.no_grad():
        out = m(dev("speakers"), dev("texts"), dev("src_lens"), int(g["src_lens"].max()), dev("wb"),
                dev("src_w_lens"), 3, spker_embeds=spk, d_control=4.0)[0]
        proj = m.speaker_emb(spk)
    assert out[0].shape[0] == B and torch.isfinite(out[0]).all()
    assert torch.equal(out[2], proj) and proj.shape == (B, 256)
