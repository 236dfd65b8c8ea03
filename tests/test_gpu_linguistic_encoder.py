"""The native LinguisticEncoder (mixgan-tts_amd/linguistic_encoder.py, csrc/lingenc.hip) on the GPU:
every fixture case of tests/golden/make_golden_lingenc.py (the REAL reference on CPU) with all nine outputs,
the two attention kernels against the plain-torch restatement (tests/lingenc_torch.py) over short, window-sized,
ragged and long shapes, the full encoder at B=16 against the restatement, run-to-run bit identity, the whole model
from phoneme ids, and a reference-layout checkpoint through get_model(..., linguistic_encoder="native")."""
import types

import numpy as np
import pytest
import torch

import lingenc_torch as LT
from helpers import golden, assert_close, Tape, T
from lingenc_helpers import CASES, manifest, configs, load_weights, encoder_inputs, assert_outputs

pytestmark = pytest.mark.gpu
TOL = 1e-4
TRAIN_TOL = 1e-3
GRAD_CASES = ("lingenc_infer", "lingenc_teacher", "lingenc_ctc")


def native(tmp_path, name, overrides=None):
    import mixgan_tts_amd as mg
    man = manifest()
    cfg = configs(man, name, tmp_path)
    enc = mg.LinguisticEncoder(*cfg)
    load_weights(enc, man, name)
    if overrides:
        with torch.no_grad():
            for k, v in overrides.items():
                enc.state_dict()[k].fill_(v)
    return enc.cuda().eval(), cfg


@pytest.mark.parametrize("name,grad", [pytest.param(n, False, id=n) for n in CASES] +
                         [pytest.param(n, True, id=n + "-grad") for n in GRAD_CASES])
def test_encoder_matches_reference_fixture(tmp_path, name, grad):
    """grad: an eval-mode forward with grad enabled, which runs the train kernels without dropout, so it is held to
    the train tests' bar (past max_seq_len it raises by design: no lingenc_long)."""
    enc, _ = native(tmp_path, name)
    g = golden(name)
    enc.record = True
    with torch.set_grad_enabled(grad):
        out = enc(*encoder_inputs(g, "cuda"))
    torch.cuda.synchronize()
    assert_outputs(out, g, TRAIN_TOL if grad else TOL, enc.recorded)


def _ragged_valid(B, L, gen):
    lens = [L] + [int(torch.randint(1, L + 1, (1,), generator=gen)) for _ in range(B - 1)]
    return (torch.arange(L)[None] < torch.tensor(lens)[:, None]).to(torch.uint8)


@pytest.mark.parametrize("L", [1, 4, 5, 9, 64, 65, 200, 1100])
def test_rel_attention_kernel(L):
    import mixgan_tts_amd as mg
    gen = torch.Generator().manual_seed(L)
    B, H, D, w = 3, 2, 128, 4
    qkv = torch.randn(B, 3 * H * D, L, generator=gen)
    ek = torch.randn(2 * w + 1, D, generator=gen) * D ** -0.5
    ev = torch.randn(2 * w + 1, D, generator=gen) * D ** -0.5
    valid = _ragged_valid(B, L, gen)
    ref = LT.rel_attention(qkv.double(), valid, ek.double(), ev.double(), H, w)
    out = mg.linguistic_encoder.rel_attention(qkv.cuda(), valid.cuda(), ek.cuda(), ev.cuda(), H, w)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), "padded queries must come out finite"
    assert_close(out.cpu(), ref.float(), TOL, "rel_attention L=%d" % L)


@pytest.mark.parametrize("Lq,Lk,ctc", [(7, 3, False), (150, 37, True), (2000, 300, False), (2000, 300, True)])
def test_w2p_attention_kernel(Lq, Lk, ctc):
    import mixgan_tts_amd as mg
    gen = torch.Generator().manual_seed(Lq + Lk)
    B, H, D = 2, 2, 128
    q = torch.randn(B, H * D, Lq, generator=gen)
    kv = torch.randn(B, 2 * H * D, Lk, generator=gen)
    kvalid = _ragged_valid(B, Lk, gen)
    qvalid = _ragged_valid(B, Lq, gen)
    mapping = (torch.rand(B, Lq, Lk, generator=gen) < 0.3).to(torch.uint8)
    prior = torch.rand(B, Lk, Lq, generator=gen) + 1e-3 if ctc else None
    ref = LT.w2p_attention(q.double(), kv.double(), kvalid, qvalid, mapping, None if prior is None else prior.double(), H)
    got = mg.linguistic_encoder.w2p_attention(q.cuda(), kv.cuda(), kvalid.cuda(), qvalid.cuda(), mapping.cuda(),
                                              None if prior is None else prior.cuda(), H)
    torch.cuda.synchronize()
    for name, a, r in zip(("out", "attn", "attn_raw", "logprob"), got, ref):
        a, r = a.cpu(), r.float()
        assert a.shape == r.shape, name
        fin = torch.isfinite(r)
        assert torch.equal(torch.isfinite(a), fin) and torch.equal(a[~fin], r[~fin]), name
        assert_close(torch.where(fin, a, 0), torch.where(fin, r, 0), TOL, name)


def _big_batch(B, n_ph, frames_per_ph, gen):
    wbs = []
    for b in range(B):
        n = n_ph - int(torch.randint(0, n_ph // 4, (1,), generator=gen)) if b else n_ph
        w = []
        while sum(w) < n:
            w.append(min(int(torch.randint(1, 5, (1,), generator=gen)), n - sum(w)))
        wbs.append(w)
    Tw, Tp = max(len(w) for w in wbs), max(sum(w) for w in wbs)
    wb = torch.zeros(B, Tw, dtype=torch.long)
    src_lens = torch.tensor([sum(w) for w in wbs])
    for b, w in enumerate(wbs):
        wb[b, :len(w)] = torch.tensor(w)
    src_mask = torch.arange(Tp)[None] < src_lens[:, None]
    src_w_lens = torch.tensor([len(w) for w in wbs])
    src_w_mask = torch.arange(Tw)[None] < src_w_lens[:, None]
    texts = torch.randint(1, 361, (B, Tp), generator=gen) * src_mask
    dur = torch.randint(frames_per_ph - 1, frames_per_ph + 2, (B, Tp), generator=gen) * src_mask
    mel_lens = dur.sum(1)
    max_len = int(mel_lens.max())
    mel_mask = torch.arange(max_len)[None] < mel_lens[:, None]
    pitch = torch.randn(B, Tp, generator=gen) * 2 * src_mask
    energy = torch.randn(B, Tp, generator=gen) * 2 * src_mask
    return (texts, src_lens, wb, src_mask, src_w_lens, src_w_mask, mel_mask, max_len, None, pitch, energy, dur, 1.0, 1.0)


@pytest.mark.parametrize("frames_per_ph", [7, 9])
def test_full_encoder_b16_against_restatement(tmp_path, frames_per_ph):
    """B=16, ~120 phonemes, ~900 / above 1000 frames (past max_seq_len: fresh sinusoid tables), targets given so that
    no integer decision depends on the last bit."""
    enc, cfg = native(tmp_path, "lingenc_infer")
    gen = torch.Generator().manual_seed(frames_per_ph)
    args = _big_batch(16, 120, frames_per_ph, gen)
    cuda = tuple(a.cuda() if isinstance(a, torch.Tensor) else a for a in args)
    sd = {k: v.detach() for k, v in enc.state_dict().items()}
    enc.record = True
    with torch.no_grad():
        out = enc(*cuda)
        ref, (enc_p, enc_w) = LT.encoder_forward(sd, cfg, *cuda)
    torch.cuda.synchronize()
    Lq = out[0].shape[1]
    assert (Lq > 1000) == (frames_per_ph == 9), Lq
    g = {k: (v.cpu().numpy()) for k, v in LT_flat(ref).items()}
    g["enc_p_out"], g["enc_w_out"] = enc_p.cpu().numpy(), enc_w.cpu().numpy()
    assert_outputs(out, g, TOL, enc.recorded)


def LT_flat(out):
    from lingenc_helpers import flat_outputs
    return flat_outputs(out)


def test_runs_are_bit_identical(tmp_path):
    enc, _ = native(tmp_path, "lingenc_infer")
    g = golden("lingenc_infer")
    with torch.no_grad():
        a = LT_flat(enc(*encoder_inputs(g, "cuda")))
        b = LT_flat(enc(*encoder_inputs(g, "cuda")))
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _model(tmp_path):
    import mixgan_tts_amd as mg
    man = manifest()
    name = "lingenc_mixgantts_naive"
    pre, mc, tr = configs(man, name, tmp_path)
    g = golden(name)
    from helpers import write_stats
    pre["path"]["preprocessed_path"] = write_stats(tmp_path, g["spec_min"], g["spec_max"])
    m = mg.MixGANTTS(types.SimpleNamespace(model="naive"), pre, mc, tr, linguistic_encoder="native")
    np.testing.assert_allclose(load_weights(m, man, name), g["wsum"], rtol=1e-12)
    return m, (pre, mc, tr), g


def _synthesize(m, g):
    d = lambda k: T(g[k]).cuda()  # noqa: E731
    m.diffusion.noise_fn = Tape([g["rng%d" % i] for i in range(len([k for k in g if k.startswith("rng")]))])
    m.linguistic_encoder.record = True
    B = g["texts"].shape[0]
    with torch.no_grad():
        out, _, _ = m(torch.zeros(B, dtype=torch.long).cuda(), d("texts"), d("src_lens"), int(g["src_lens"].max()),
                      d("wb"), d("src_w_lens"), int(g["src_w_lens"].max()), d_control=float(g["d_control"]))
    torch.cuda.synchronize()
    assert m.diffusion.noise_fn.i == len(m.diffusion.noise_fn.items)
    return out


def test_mixgantts_native_from_phoneme_ids(tmp_path):
    m, _, g = _model(tmp_path)
    m = m.cuda().eval()
    out = _synthesize(m, g)
    enc_out = (out[0], out[4], out[5], out[6], out[7], out[11], ~out[9], out[12], out[13])
    assert_close(out[0], g["mel"], TOL, "mel")
    for i, k in ((1, "out1"), (2, "out2"), (3, "out3")):
        a, r = enc_out[i].cpu().numpy(), g[k]
        fin = np.isfinite(r)
        assert np.array_equal(a[~fin], r[~fin]), k
        assert_close(np.where(fin, a, 0), np.where(fin, r, 0), TOL, k)
    assert np.array_equal(out[7].cpu().numpy(), g["out4"]) and np.array_equal(out[11].cpu().numpy(), g["out5"])
    assert_close(m.linguistic_encoder.recorded["enc_p_out"], g["enc_p_out"], TOL, "enc_p_out")


def test_checkpoint_roundtrip_native(tmp_path):
    """A reference-layout generator state dict saved by save_checkpoint loads strictly through
    get_model(..., linguistic_encoder="native") and synthesizes the same mel."""
    import mixgan_tts_amd as mg
    m, (pre, mc, tr), g = _model(tmp_path)
    man = manifest()
    assert sorted(m.state_dict()) == sorted(man["lingenc_mixgantts_naive"]["state_dict"])
    tr = dict(tr, path=dict(tr["path"], ckpt_path=str(tmp_path / "ckpt")))
    disc = mg.JCUDiscriminator(pre, mc, tr)
    optG_fs2 = mg.ScheduledOptim(m, tr, mc, 0)
    optG = torch.optim.Adam(m.parameters(), lr=1e-4)
    optD = torch.optim.Adam(disc.parameters(), lr=1e-4)
    sdlG = torch.optim.lr_scheduler.ExponentialLR(optG, 0.999)
    sdlD = torch.optim.lr_scheduler.ExponentialLR(optD, 0.999)
    mg.save_checkpoint(tr, 7, 1, m, disc, optG_fs2, optG, optD, sdlG, sdlD)
    args = types.SimpleNamespace(model="naive", restore_step=7)
    m2 = mg.get_model(args, (pre, mc, tr), "cuda", linguistic_encoder="native")
    assert not hasattr(m2, "skipped_checkpoint_keys")
    out = _synthesize(m2, g)
    assert_close(out[0], g["mel"], TOL, "mel after restore")
