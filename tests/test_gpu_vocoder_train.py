"""GPU parity of the vocoder-training kernels, the differentiable log-mel, Generator.forward_train and
GeneratorTrainer against float64 torch autograd on the CPU (tests/hifigan_train_ref.py).

Error measure: max-abs error over max-abs reference (helpers.assert_close).  Bars: 2e-5 maps,
5e-5 data gradients, 1e-4 parameter gradients; where the float32 CPU restatement's own error against float64 exceeds
bar / 8 on a tensor, that tensor's bar is 8 x that error.

Leaky-ReLU kinks (whole generator, trainer): the float64 restatement adopts the product's sign pattern (`masks=`), and
the test asserts what makes that sound: every element whose product sign differs from the float64 run's own sign has
|pre64| <= 1e-4 max|pre64| of its tensor, and such elements are at most 1e-3 of the tensor.
"""
import json
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, assert_close, check, load_seeded, seeded, T
from oracle import refmath as R
import hifigan_train_ref as HR

pytestmark = pytest.mark.gpu
BAR_MAP, BAR_DATA, BAR_PARAM = 2e-5, 5e-5, 1e-4


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


# ------------------------------------------------------------------------------------------------------------------
# 1, 2: dilated weight gradient, data gradient + leaky-ReLU backward + residual add
# ------------------------------------------------------------------------------------------------------------------
CONV_CASES = [(3, 1, 64, 64, 2, 333, 0.1), (3, 5, 32, 32, 2, 257, 0.1), (7, 3, 128, 128, 2, 400, 0.1),
              (11, 5, 32, 32, 1, 129, 0.1), (11, 1, 256, 256, 1, 64, 1.0), (7, 1, 32, 1, 2, 515, 0.01),
              (7, 1, 80, 512, 2, 5, 1.0), (7, 5, 64, 64, 1, 9, 0.1)]
# the remaining workgroup-tile forms of the weight-gradient kernel (32 / 64 / 128 rows x 32 / 64 / 128 columns, chosen
# from Co and Ci), at a length of two chunks and a part
TILE_CASES = [(3, 2, 64, 32, 2, 150, 0.1), (3, 2, 128, 16, 2, 150, 0.1), (3, 2, 100, 64, 2, 150, 0.1),
              (3, 2, 32, 128, 2, 150, 0.1), (3, 2, 48, 96, 2, 150, 0.1)]
_conv_ref = {}


def conv_case(case):
    """Inputs and the float64 / float32 CPU gradients of sum(cot * (conv(lrelu(x)) + x')), x' = x only where Co = Ci."""
    if case in _conv_ref:
        return _conv_ref[case]
    K, dil, Ci, Co, B, L, s = case
    gen = torch.Generator().manual_seed(K * 1000 + dil * 100 + L)
    x = torch.randn(B, Ci, L, generator=gen)
    w = torch.randn(Co, Ci, K, generator=gen) / (Ci * K) ** 0.5
    cot = torch.randn(B, Co, L, generator=gen)
    pad = (K * dil - dil) // 2
    # the residual branch: conv(lrelu(x)) + x where the shapes agree (its cotangent is cot); where Co != Ci the branch
    # is x with a cotangent of its own, which is all the backward kernel sees of it
    res = cot if Co == Ci else torch.randn(B, Ci, L, generator=gen)
    out = {"x": x, "w": w, "cot": cot, "pad": pad, "res": res}
    for dt in (torch.float64, torch.float32):
        xd, wd = x.to(dt, copy=True).requires_grad_(), w.to(dt, copy=True).requires_grad_()
        y = F.conv1d(F.leaky_relu(xd, s), wd, None, 1, pad, dil)
        if Co == Ci:
            ((y + xd) * cot.to(dt)).sum().backward()
        else:
            ((y * cot.to(dt)).sum() + (xd * res.to(dt)).sum()).backward()
        out[dt] = {"dw": wd.grad, "dx": xd.grad}
    _conv_ref[case] = out
    return out


@pytest.mark.parametrize("case", CONV_CASES + TILE_CASES, ids=lambda c: "K%d_d%d_%dx%d_B%d_L%d" % c[:6])
def test_conv1d_wgrad_ex(mg, case):
    K, dil, Ci, Co, B, L, s = case
    c = conv_case(case)
    r64, r32 = c[torch.float64]["dw"], c[torch.float32]["dw"]
    x, cot = c["x"].cuda(), c["cot"].cuda()
    dw = mg.ops.conv1d_wgrad_ex(cot, x, K, dil, c["pad"], s)
    check(dw, r32, r64, BAR_PARAM, "dw")
    assert torch.equal(dw, mg.ops.conv1d_wgrad_ex(cot, x, K, dil, c["pad"], s)), "not reproducible"
    check(mg.ops.conv1d_wgrad_ex(cot, x, K, dil, c["pad"], s, alpha=0.5), 0.5 * r32, 0.5 * r64, BAR_PARAM, "dw alpha=0.5")
    base = torch.randn(Co, Ci, K, generator=torch.Generator().manual_seed(3))
    acc = base.cuda()
    mg.ops.conv1d_wgrad_ex(cot, x, K, dil, c["pad"], s, alpha=0.5, out=acc, accumulate=True)
    check(acc, base + 0.5 * r32, base.double() + 0.5 * r64, BAR_PARAM, "dw accumulated")


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "K%d_d%d_%dx%d_B%d_L%d" % c[:6])
def test_dilated_dgrad_lrelu_bwd_residual(mg, case):
    K, dil, Ci, Co, B, L, s = case
    c = conv_case(case)
    r64, r32 = c[torch.float64], c[torch.float32]
    x, cot, res = c["x"].cuda(), c["cot"].cuda(), c["res"].cuda()
    wp = mg.ops.pack_conv_weight(c["w"].cuda(), mg.ops.PACK_DGRAD)
    d = mg.ops.conv1d_packed(cot, wp, None, Ci, K, 1, dil * (K - 1) - c["pad"], Lout=L, dilation=dil)
    dx = mg.ops.lrelu_bwd(d, x, s, add=res)
    check(dx, r32["dx"], r64["dx"], BAR_DATA, "dx")
    # in place over dy
    mg.ops.lrelu_bwd(d, x, s, add=res, out=d)
    assert torch.equal(d, dx)


def test_lrelu_bwd_takes_the_slope_at_zero(mg):
    x = torch.tensor([-1.0, -0.0, 0.0, 2.0, -3.0]).cuda()
    dy = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]).cuda()
    out = mg.ops.lrelu_bwd(dy, x, 0.1)
    assert torch.equal(out.cpu(), torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]) * torch.tensor([0.1, 0.1, 0.1, 1.0, 0.1]))


# ------------------------------------------------------------------------------------------------------------------
# 3: ConvTranspose1d backward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u,Ci,Co,B,L", [(8, 512, 256, 2, 13), (8, 64, 32, 3, 133), (2, 128, 64, 2, 77), (2, 64, 32, 1, 1),
                                          (4, 32, 16, 2, 300), (8, 24, 4, 1, 50), (2, 16, 2, 2, 700)])
def test_conv_transpose_backward(mg, u, Ci, Co, B, L):
    gen = torch.Generator().manual_seed(u * 1000 + L)
    x = torch.randn(B, Ci, L, generator=gen)
    w = torch.randn(Ci, Co, 2 * u, generator=gen) / (2 * Ci) ** 0.5
    cot = torch.randn(B, Co, u * L, generator=gen)
    ref = {}
    for dt in (torch.float64, torch.float32):
        xd, wd = x.to(dt, copy=True).requires_grad_(), w.to(dt, copy=True).requires_grad_()
        y = 0.5 * F.conv_transpose1d(F.leaky_relu(xd, 0.1), wd, None, u, u // 2)
        (y * cot.to(dt)).sum().backward()
        ref[dt] = (xd.grad, wd.grad)
    xc, wc, gc = x.cuda(), w.cuda(), cot.cuda()
    dx = mg.ops.conv_transpose1d_dgrad(gc, wc, xc, 0.1, 0.5)
    check(dx, ref[torch.float32][0], ref[torch.float64][0], BAR_DATA, "convT dx")
    dw = mg.ops.conv_transpose1d_wgrad(gc, xc, Co, u, 0.1, 0.5)
    check(dw, ref[torch.float32][1], ref[torch.float64][1], BAR_PARAM, "convT dw")
    assert torch.equal(dw, mg.ops.conv_transpose1d_wgrad(gc, xc, Co, u, 0.1, 0.5)), "not reproducible"
    base = torch.randn(Ci, Co, 2 * u, generator=torch.Generator().manual_seed(4))
    acc = base.cuda()
    mg.ops.conv_transpose1d_wgrad(gc, xc, Co, u, 0.1, 0.5, out=acc, accumulate=True)
    check(acc, base + ref[torch.float32][1], base.double() + ref[torch.float64][1], BAR_PARAM, "convT dw accumulated")


# ------------------------------------------------------------------------------------------------------------------
# 4: differentiable log-mel
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stft(mg):
    return mg.audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)


def mel_tables(stft):
    return stft.stft_fn._tables.window.double(), stft.mel_basis.double().cpu()


@pytest.mark.parametrize("B,L", [(1, 513), (2, 768), (3, 2148), (1, 8192)])
def test_mel_spectrogram_diff(mg, stft, B, L):
    rng = np.random.default_rng(L)
    y = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, L)).astype(np.float32))
    T_ = 1 + L // 256
    cot = torch.from_numpy(rng.standard_normal((B, 80, T_)).astype(np.float32))
    win, basis = mel_tables(stft)
    ref = {}
    for dt in (torch.float64, torch.float32):
        yd = y.to(dt, copy=True).requires_grad_()
        m = HR.log_mel(yd, win, basis)
        (m * cot.to(dt)).sum().backward()
        ref[dt] = (m.detach(), yd.grad)
    yc = y.cuda().requires_grad_()
    mel = stft.mel_spectrogram_diff(yc)
    assert tuple(mel.shape) == (B, 80, T_)
    assert torch.equal(mel.detach(), stft.mel_spectrogram(y.cuda())[0]), "forward differs from mel_spectrogram"
    check(mel, ref[torch.float32][0], ref[torch.float64][0], BAR_MAP, "log-mel")
    (mel * cot.cuda()).sum().backward()
    check(yc.grad, ref[torch.float32][1], ref[torch.float64][1], BAR_DATA, "d log-mel / d signal")
    y2 = y.cuda().requires_grad_()
    (stft.mel_spectrogram_diff(y2) * cot.cuda()).sum().backward()
    assert torch.equal(y2.grad, yc.grad), "second call gives other bits"


def test_mel_spectrogram_diff_zero_row(mg, stft):
    """|X| = 0 and the clamp make torch's own gradient NaN on a silent row; the kernel's is exactly zero."""
    rng = np.random.default_rng(1)
    y = torch.from_numpy(rng.uniform(-0.9, 0.9, (2, 768)).astype(np.float32))
    y[1] = 0
    yc = y.cuda().requires_grad_()
    mel = stft.mel_spectrogram_diff(yc)
    (mel * torch.from_numpy(rng.standard_normal((2, 80, 4)).astype(np.float32)).cuda()).sum().backward()
    assert torch.isfinite(yc.grad).all()
    assert (yc.grad[1] == 0).all() and (yc.grad[0] != 0).any()


# ------------------------------------------------------------------------------------------------------------------
# 5: the whole generator
# ------------------------------------------------------------------------------------------------------------------
def _h():
    return types.SimpleNamespace(**R.HIFIGAN_V1)


def seeded_weights(manifest):
    g = golden("hifigan")
    W, _ = seeded(manifest, "hifigan", 81)
    for k in g:
        if k.startswith("gain/"):
            W[k[5:]] = T(g[k])
    return W


def seeded_generator(mg, W):
    G = mg.vocoder.Generator(_h())
    G.load_state_dict({k: v.detach().clone() for k, v in W.items()})
    return G.cuda()


def assert_kinks_sound(product_taps, own64_taps):
    """The condition under which the float64 restatement may adopt the product's signs.  Returns the masks."""
    masks = {}
    assert set(product_taps) == set(own64_taps)
    for k, p in product_taps.items():
        pos = (p.detach() > 0).cpu()
        pre = own64_taps[k]
        flip = pos != (pre > 0)
        n = int(flip.sum())
        if n:
            worst = float(pre[flip].abs().max() / pre.abs().max())
            assert worst <= 1e-4, "%s: a flipped sign at |pre64| / max = %.2e" % (k, worst)
            assert n <= 1e-3 * pre.numel(), "%s: %d of %d signs flipped" % (k, n, pre.numel())
        masks[k] = pos
    return masks


def generator_against_reference(G, W, mel, cot):
    G.zero_grad(set_to_none=True)
    taps = {}
    mc = mel.cuda().requires_grad_()
    y = G.forward_train(mc, taps)
    assert y.requires_grad and tuple(y.shape) == (mel.shape[0], 1, 256 * mel.shape[2])
    assert_close(y.detach().cpu(), G(mel.cuda()).cpu(), 1e-5, "forward_train vs eval forward")
    (y * cot.cuda()).sum().backward()
    own = HR.generator_grads(W, mel, cot, torch.float64)
    masks = assert_kinks_sound(taps, own["taps"])
    r64 = HR.generator_grads(W, mel, cot, torch.float64, masks=masks)
    r32 = HR.generator_grads(W, mel, cot, torch.float32, masks=masks)
    check(y, r32["out"], r64["out"], BAR_MAP, "waveform")
    check(mc.grad, r32["d_mel"], r64["d_mel"], BAR_DATA, "d mel")
    params = dict(G.named_parameters())
    assert set(params) == set(W)
    for k, p in params.items():
        assert p.grad is not None, k
        check(p.grad, r32["param/" + k], r64["param/" + k], BAR_PARAM, "d " + k)


@pytest.mark.parametrize("B,L", [(2, 3), (1, 9)])
def test_generator_forward_train(mg, manifest, B, L):
    W = seeded_weights(manifest)
    G = seeded_generator(mg, W)
    rng = np.random.default_rng(100 + L)
    mel = torch.from_numpy(rng.uniform(-11.5, 2.0, (B, 80, L)).astype(np.float32))
    cot = torch.from_numpy(rng.standard_normal((B, 1, 256 * L)).astype(np.float32))
    generator_against_reference(G, W, mel, cot)
    # the same after remove_weight_norm: the effective weights are the parameters
    G.remove_weight_norm()
    W2 = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    assert "conv_pre.weight" in W2 and "conv_pre.weight_g" not in W2
    generator_against_reference(G, W2, mel, cot)


def test_forward_train_rejects_what_it_cannot_differentiate(mg):
    cfg = dict(R.HIFIGAN_V1)
    cfg["upsample_rates"], cfg["upsample_kernel_sizes"] = [8, 8, 4], [16, 16, 7]
    G = mg.vocoder.Generator(types.SimpleNamespace(**cfg)).cuda()
    with pytest.raises(mg.MixganHipError):
        G.forward_train(torch.zeros(1, 80, 4).cuda())
    with pytest.raises(mg.MixganHipError):
        mg.vocoder.Generator(_h()).forward_train(torch.zeros(1, 80, 4))


# ------------------------------------------------------------------------------------------------------------------
# 6: trainer
# ------------------------------------------------------------------------------------------------------------------
def trainer_batch():
    rng = np.random.default_rng(7)
    mel = torch.from_numpy(rng.uniform(-11.5, 2.0, (2, 80, 4)).astype(np.float32))
    wav = torch.from_numpy(rng.uniform(-0.9, 0.9, (2, 1024)).astype(np.float32))
    return mel, wav


def test_trainer_sgd_two_steps_match_float64(mg, manifest, stft):
    """lr = 1e-5: in the float64 restatement the loss goes 51.47 -> 49.95 -> 48.60, 3 % a step against a bar of 2e-5."""
    LR = 1e-5
    W = seeded_weights(manifest)
    G = seeded_generator(mg, W)
    tr = mg.GeneratorTrainer(G, stft, optimizer=torch.optim.SGD, lr=LR)
    mel, wav = trainer_batch()
    win, basis = mel_tables(stft)
    state = {dt: {k: v.detach().to(dt, copy=True).requires_grad_() for k, v in W.items()}
             for dt in (torch.float64, torch.float32)}
    ref_losses = {torch.float64: [], torch.float32: []}
    got = []
    for step in range(2):
        taps = {}
        with torch.no_grad():
            G.forward_train(mel.cuda(), taps)           # the sign pattern this step's backward will use
        own = {}
        HR.generator_forward({k: v.detach() for k, v in state[torch.float64].items()}, mel.double(), taps=own)
        masks = assert_kinks_sound(taps, own)
        got.append(tr.step(mel.cuda(), wav.cuda()))
        for dt, Wd in state.items():
            for v in Wd.values():
                v.grad = None
            m = HR.log_mel(HR.generator_forward(Wd, mel.to(dt), masks=masks)[:, 0], win, basis)
            loss = 45.0 * (m - HR.log_mel(wav.to(dt), win, basis)).abs().mean()
            loss.backward()
            ref_losses[dt].append(loss.detach())
            with torch.no_grad():
                for v in Wd.values():
                    v -= LR * v.grad
    l64 = ref_losses[torch.float64]
    assert abs(float(l64[1] - l64[0])) > 100 * BAR_MAP * float(l64[0]), "the second step does not see the update"
    for i in range(2):
        assert got[i]["loss"].is_cuda and got[i]["loss"].dim() == 0
        check(got[i]["loss"].reshape(1), ref_losses[torch.float32][i].reshape(1), l64[i].reshape(1), BAR_MAP,
              "loss of step %d" % i)
    for k, p in G.named_parameters():
        check(p, state[torch.float32][k], state[torch.float64][k].detach(), BAR_PARAM, "post-step " + k)


def test_trainer_default_optimizer_and_checkpoint(mg, manifest, stft, tmp_path):
    W = seeded_weights(manifest)
    G = seeded_generator(mg, W)
    tr = mg.GeneratorTrainer(G, stft)
    assert isinstance(tr.optimizer, torch.optim.AdamW) and tr.optimizer.defaults["betas"] == (0.8, 0.99)
    assert tr.optimizer.defaults["lr"] == 2e-4 and tr.lambda_mel == 45.0
    mel, wav = trainer_batch()
    losses = [tr.step(mel.cuda(), wav.cuda())["loss"] for _ in range(3)]
    assert all(bool(torch.isfinite(l)) for l in losses)
    for k, p in G.named_parameters():
        assert not torch.equal(p.detach().cpu(), W[k]), k + " did not move"
    ck = tmp_path / "generator_trained.pth.tar"
    tr.save(str(ck))
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps(R.HIFIGAN_V1))
    voc = mg.vocoder.get_vocoder({"vocoder": {"model": "HiFi-GAN", "speaker": "LJSpeech"}}, "cuda", config_path=str(cfg),
                                 checkpoint_path=str(ck))
    # load() restores the same generator into a fresh trainer
    G2 = mg.vocoder.Generator(_h()).cuda()
    tr2 = mg.GeneratorTrainer(G2, stft).load(str(ck))
    assert tr2.steps == 3
    for (k, a), (_, b) in zip(G.state_dict().items(), G2.state_dict().items()):
        assert torch.equal(a, b), k
    G.eval()
    G.cpu().remove_weight_norm()          # on the host, where get_vocoder folds the norm
    G.cuda()
    assert torch.equal(voc(mel.cuda()), G(mel.cuda()))


def test_sample_segments_are_aligned(mg):
    B, Fmax, frames = 5, 50, 32
    lens = [32, 33, 40, 50, 47]
    mels = torch.arange(Fmax, dtype=torch.float32).repeat(B, 80, 1)
    wavs = torch.arange(256 * Fmax, dtype=torch.float32).repeat(B, 1)
    gen = torch.Generator().manual_seed(0)
    seen = set()
    for _ in range(8):
        mel, wav, offs = mg.sample_segments(mels, wavs, lens, frames=frames, generator=gen)
        assert tuple(mel.shape) == (B, 80, frames) and tuple(wav.shape) == (B, 256 * frames)
        for b in range(B):
            o = int(offs[b])
            seen.add((b, o))
            assert 0 <= o and o + frames <= lens[b]
            assert int(mel[b, 0, 0]) == o and int(mel[b, 0, -1]) == o + frames - 1
            assert int(wav[b, 0]) == 256 * o and int(wav[b, -1]) == 256 * (o + frames) - 1
    assert len(seen) > B, "offsets never vary"
    with pytest.raises(ValueError):
        mg.sample_segments(mels, wavs, [31] + lens[1:], frames=frames)
