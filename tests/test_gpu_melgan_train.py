"""GPU parity of MelGAN generator training (csrc/melgan_train.hip, autograd.voc_conv with pad = REFLECT / melgan_resblock,
MelGANGenerator.forward_train, the two vocoder trainers over a MelVocoder) against float64 torch autograd on the CPU,
computed here.  The reference conv is F.conv1d(F.pad(F.leaky_relu(x, s), (p, p), mode="reflect"), w, dilation=dil).

Error measure and bars: those of tests/test_gpu_vocoder_train.py through helpers.check -- max-abs error over max-abs
reference; 2e-5 maps, 5e-5 data gradients, 1e-4 parameter gradients; where the float32 CPU run's own error against
float64 exceeds bar / 8 on a tensor, that tensor's bar is 8 x that error.

Leaky-ReLU kinks (whole generator, trainer): the float64 restatement (tests/melgan_train_ref.py) adopts the product's
sign pattern, and the test asserts what makes that sound: every element whose product sign differs from the float64
run's own has |pre64| <= 1e-4 max|pre64| of its tensor, and such elements are at most 1e-3 of the tensor.
"""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import check
import hifigan_train_ref as HR
import melgan_torch as MT
import melgan_train_ref as MR
from test_gpu_vocoder_train import assert_kinks_sound, mel_tables

pytestmark = pytest.mark.gpu
BAR_MAP, BAR_DATA, BAR_PARAM = 2e-5, 5e-5, 1e-4


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


@pytest.fixture(scope="module")
def stft(mg):
    return mg.audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)


# ------------------------------------------------------------------------------------------------------------------
# 1, 2: reflect weight gradient, reflect data gradient
# ------------------------------------------------------------------------------------------------------------------
CONV_CASES = [(3, 1, 32, 32, 2, 2, .2),       # L = p + 1
              (3, 9, 32, 32, 2, 10, .2),      # L = p + 1; the mirrors overlap
              (3, 9, 64, 64, 2, 18, .2),      # L = 2p
              (3, 3, 128, 128, 1, 150, .2),   # two 64-frame chunks and a part
              (3, 9, 256, 256, 2, 333, .2),
              (7, 1, 80, 512, 2, 4, 1.0),     # first conv, shortest mel
              (7, 1, 32, 1, 2, 515, .2),      # last conv, one output row
              (3, 9, 48, 96, 2, 150, .2)]     # ragged tiles
_conv_ref = {}


def conv_case(case):
    """Inputs and the float64 / float32 CPU gradients of sum(cot * conv(reflect(lrelu(x)))) + sum(res * x)."""
    if case in _conv_ref:
        return _conv_ref[case]
    K, dil, Ci, Co, B, L, s = case
    gen = torch.Generator().manual_seed(K * 1000 + dil * 100 + L)
    x = torch.randn(B, Ci, L, generator=gen)
    w = torch.randn(Co, Ci, K, generator=gen) / (Ci * K) ** 0.5
    cot = torch.randn(B, Co, L, generator=gen)
    res = torch.randn(B, Ci, L, generator=gen)
    p = dil * (K - 1) // 2
    out = {"x": x, "w": w, "cot": cot, "res": res}
    for dt in (torch.float64, torch.float32):
        xd, wd = x.to(dt, copy=True).requires_grad_(), w.to(dt, copy=True).requires_grad_()
        y = F.conv1d(F.pad(F.leaky_relu(xd, s), (p, p), mode="reflect"), wd, dilation=dil)
        (y * cot.to(dt)).sum().backward()
        out[dt] = {"dw": wd.grad, "dx": xd.grad}
    _conv_ref[case] = out
    return out


def in_wide_buffer(x, gen_seed):
    """x [B, C, L] as channels [0, C) of a [B, 2C, L] buffer whose other half is noise."""
    B, C, L = x.shape
    buf = torch.randn(B, 2 * C, L, generator=torch.Generator().manual_seed(gen_seed))
    buf[:, :C] = x
    return buf.cuda()


IDS = lambda c: "K%d_d%d_%dx%d_B%d_L%d" % c[:6]


@pytest.mark.parametrize("case", CONV_CASES, ids=IDS)
def test_reflect_wgrad(mg, case):
    K, dil, Ci, Co, B, L, s = case
    c = conv_case(case)
    r64, r32 = c[torch.float64]["dw"], c[torch.float32]["dw"]
    x, cot = c["x"].cuda(), c["cot"].cuda()
    wg = mg.ops.conv1d_reflect_wgrad
    dw = wg(cot, x, K, dil, s)
    check(dw, r32, r64, BAR_PARAM, "dw")
    assert torch.equal(dw, wg(cot, x, K, dil, s)), "not reproducible"
    check(wg(cot, x, K, dil, s, alpha=0.5), 0.5 * r32, 0.5 * r64, BAR_PARAM, "dw alpha=0.5")
    base = torch.randn(Co, Ci, K, generator=torch.Generator().manual_seed(3))
    acc = base.cuda()
    wg(cot, x, K, dil, s, alpha=0.5, out=acc, accumulate=True)
    check(acc, base + 0.5 * r32, base.double() + 0.5 * r64, BAR_PARAM, "dw accumulated")
    dws = wg(cot, in_wide_buffer(c["x"], 5), K, dil, s, x_bs=2 * Ci * L, C=Ci)
    assert torch.equal(dws, dw), "x in a [B, 2C, L] buffer gives other bits"
    dws = wg(in_wide_buffer(c["cot"], 8), in_wide_buffer(c["x"], 5), K, dil, s, x_bs=2 * Ci * L, C=Ci, dy_bs=2 * Co * L,
             Co=Co)
    assert torch.equal(dws, dw), "dy in a [B, 2Co, L] buffer gives other bits"


@pytest.mark.parametrize("case", CONV_CASES, ids=IDS)
def test_reflect_dgrad(mg, case):
    K, dil, Ci, Co, B, L, s = case
    c = conv_case(case)
    r64, r32 = c[torch.float64]["dx"], c[torch.float32]["dx"]
    x, cot, res, w = c["x"].cuda(), c["cot"].cuda(), c["res"].cuda(), c["w"].cuda()
    dg = mg.ops.conv1d_reflect_dgrad
    dx = dg(cot, w, x, dil, s)
    assert tuple(dx.shape) == (B, Ci, L)
    check(dx, r32, r64, BAR_DATA, "dx")
    assert torch.equal(dx, dg(cot, w, x, dil, s)), "not reproducible"
    check(dg(cot, w, x, dil, s, alpha=0.5), 0.5 * r32, 0.5 * r64, BAR_DATA, "dx alpha=0.5")
    dxa = dg(cot, w, x, dil, s, add=res)
    check(dxa, r32 + c["res"], r64 + c["res"].double(), BAR_DATA, "dx + add")
    # x and add inside [B, 2C, L] buffers
    dxs = dg(cot, w, in_wide_buffer(c["x"], 6), dil, s, add=in_wide_buffer(c["res"], 7), x_bs=2 * Ci * L,
             add_bs=2 * Ci * L, C=Ci)
    assert torch.equal(dxs, dxa), "batch strides give other bits"
    # in place over add
    inp = res.clone()
    dg(cot, w, x, dil, s, add=inp, out=inp)
    assert torch.equal(inp, dxa)


def test_fold_takes_the_slope_at_zero_and_counts_each_mirror_once(mg):
    """L = 3, p = 2: both mirrors reach i = 1.  The expected sums are written out from ReflectionPad1d's index map."""
    from mixgan_tts_amd._lib import fptr, check as ok, stream_ptr
    L, p = 3, 2
    P = torch.arange(1.0, 8.0).reshape(1, 1, L + 2 * p)            # P[j] = j + 1
    x = torch.tensor([[[1.0, -0.0, -2.0]]])
    Pc, xc, out = P.cuda(), x.cuda(), torch.empty(1, 1, L, device="cuda")
    ok(mg.lib().mg_reflect_fold_bwd(fptr(Pc), 0, fptr(xc), 0, None, 0, fptr(out), 1, 1, L, p, 0.5, stream_ptr()))
    # padded index j reads a[refl(j - p)]: j = 0..6 -> a[2], a[1], a[0], a[1], a[2], a[1], a[0]
    da = torch.tensor([P[0, 0, 2] + P[0, 0, 6], P[0, 0, 1] + P[0, 0, 3] + P[0, 0, 5], P[0, 0, 0] + P[0, 0, 4]])
    assert torch.equal(out.cpu().flatten(), da * torch.tensor([1.0, 0.5, 0.5]))


# ------------------------------------------------------------------------------------------------------------------
# 3: the ResnetBlock Function
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [10, 77, 200])
@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("C", [32, 64, 256])
def test_resblock_function(mg, C, dil, L):
    B = 2
    torch.manual_seed(C + 10 * dil + L)
    blk = MT.ResnetBlock(C, dil)
    for m in (blk.block[2], blk.block[4], blk.shortcut):
        torch.nn.utils.remove_weight_norm(m)
    gen = torch.Generator().manual_seed(C * dil + L)
    x = torch.randn(B, C, L, generator=gen)
    cot = torch.randn(B, C, L, generator=gen)
    ref = {}
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(blk).to(dt)
        xd = x.to(dt, copy=True).requires_grad_()
        y = r(xd)
        (y * cot.to(dt)).sum().backward()
        out = {"y": y.detach(), "dx": xd.grad}
        for n, m in (("1", r.block[2]), ("2", r.block[4]), ("s", r.shortcut)):
            out["w" + n], out["b" + n] = m.weight.grad, m.bias.grad
        ref[dt] = out
    p = {}
    for n, m in (("1", blk.block[2]), ("2", blk.block[4]), ("s", blk.shortcut)):
        p["w" + n] = m.weight.detach().cuda().requires_grad_()
        p["b" + n] = m.bias.detach().cuda().requires_grad_()
    xc = x.cuda().requires_grad_()
    y, xt = mg.autograd.melgan_resblock(xc, p["w1"], p["b1"], p["w2"], p["b2"], p["ws"], p["bs"], dil, 0.2)
    assert tuple(xt.shape) == (B, 2 * C, L) and not xt.requires_grad and torch.equal(xt[:, :C], xc.detach())
    r64, r32 = ref[torch.float64], ref[torch.float32]
    check(y, r32["y"], r64["y"], BAR_MAP, "block output")
    (y * cot.cuda()).sum().backward()
    check(xc.grad, r32["dx"], r64["dx"], BAR_DATA, "dx")
    for k in ("w1", "b1", "w2", "b2", "ws", "bs"):
        check(p[k].grad, r32[k], r64[k], BAR_PARAM, "d " + k)


# ------------------------------------------------------------------------------------------------------------------
# 4, 5: the whole generator
# ------------------------------------------------------------------------------------------------------------------
_seeded = {}


def seeded_weights(seed=0):
    if seed not in _seeded:
        _seeded[seed] = {k: v.detach().clone() for k, v in MT.seeded_generator(seed).state_dict().items()}
    return _seeded[seed]


def seeded_generator(mg, W):
    G = mg.MelGANGenerator()
    G.load_state_dict({k: v.clone() for k, v in W.items()}, strict=True)
    return G.cuda()


def seeded_mel(B, L, seed):
    return torch.randn(B, 80, L, generator=torch.Generator().manual_seed(seed)) - 4.0


@pytest.mark.parametrize("B,L", [(2, 4), (1, 11), (2, 37)])
def test_forward_train_equals_forward(mg, B, L):
    G = seeded_generator(mg, seeded_weights())
    assert G.fused_stack
    mel = seeded_mel(B, L, 40 + L).cuda()
    with torch.no_grad():
        y = G.forward_train(mel)
    ref = G(mel).cpu()
    check(y, ref, ref.double(), BAR_MAP, "forward_train vs forward")
    with torch.no_grad():
        ys = G.forward_train(mel, None, 0.5)
    ref = G.forward_scaled(mel, 0.5).cpu()
    check(ys, ref, ref.double(), BAR_MAP, "forward_train vs forward_scaled(0.5)")


@pytest.mark.parametrize("B,L", [(2, 4), (2, 11)])
def test_generator_forward_train(mg, B, L):
    W = seeded_weights()
    G = seeded_generator(mg, W)
    mel = seeded_mel(B, L, 100 + L)
    cot = torch.randn(B, 1, 256 * L, generator=torch.Generator().manual_seed(200 + L))
    taps = {}
    mc = mel.cuda().requires_grad_()
    y = G.forward_train(mc, taps)
    assert y.requires_grad and tuple(y.shape) == (B, 1, 256 * L) and len(taps) == 29
    (y * cot.cuda()).sum().backward()
    own = MR.generator_grads(W, mel, cot, torch.float64)
    masks = assert_kinks_sound(taps, own["taps"])
    r64 = MR.generator_grads(W, mel, cot, torch.float64, masks=masks)
    r32 = MR.generator_grads(W, mel, cot, torch.float32, masks=masks)
    check(y, r32["out"], r64["out"], BAR_MAP, "waveform")
    check(mc.grad, r32["d_mel"], r64["d_mel"], BAR_DATA, "d mel")
    params = dict(G.named_parameters())
    assert set(params) == set(W)
    for k, p in params.items():
        assert p.grad is not None, k
        check(p.grad, r32["param/" + k], r64["param/" + k], BAR_PARAM, "d " + k)


# ------------------------------------------------------------------------------------------------------------------
# 6: trainers
# ------------------------------------------------------------------------------------------------------------------
def seeded_vocoder(mg, W):
    voc = mg.MelVocoder()
    voc.mel2wav.load_state_dict({k: v.clone() for k, v in W.items()}, strict=True)
    return voc.cuda()


def trainer_batch(frames=8):
    rng = np.random.default_rng(7)
    mel = torch.from_numpy(rng.normal(-4.0, 1.0, (2, 80, frames)).astype(np.float32))
    wav = torch.from_numpy(rng.uniform(-0.9, 0.9, (2, 256 * frames)).astype(np.float32))
    return mel, wav


def test_generator_trainer_loss_and_gradients_match_float64(mg, stft):
    W = seeded_weights()
    voc = seeded_vocoder(mg, W)
    tr = mg.GeneratorTrainer(voc, stft)
    mel, wav = trainer_batch()
    scale = 1.0 / math.log(10.0)
    win, basis = mel_tables(stft)
    taps = {}
    loss, y_hat = tr.loss(mel.cuda(), wav.cuda())
    with torch.no_grad():
        assert torch.equal(voc.forward_train(mel.cuda(), taps), y_hat.detach())
    loss.backward()
    own = {}
    MR.generator_forward({k: v.double() for k, v in W.items()}, mel.double(), taps=own, scale=scale)
    masks = assert_kinks_sound(taps, own)
    ref = {}
    for dt in (torch.float64, torch.float32):
        Wd = {k: v.detach().to(dt, copy=True).requires_grad_() for k, v in W.items()}
        m = HR.log_mel(MR.generator_forward(Wd, mel.to(dt), masks=masks, scale=scale)[:, 0], win, basis)
        l = 45.0 * (m - HR.log_mel(wav.to(dt), win, basis)).abs().mean()
        l.backward()
        ref[dt] = (l.detach(), {k: v.grad for k, v in Wd.items()})
    check(loss.reshape(1), ref[torch.float32][0].reshape(1), ref[torch.float64][0].reshape(1), BAR_MAP, "loss")
    before = {}
    for k, p in voc.mel2wav.named_parameters():
        check(p.grad, ref[torch.float32][1][k], ref[torch.float64][1][k], BAR_PARAM, "d " + k)
        before[k] = p.detach().clone()
    out = tr.step(mel.cuda(), wav.cuda())
    assert out["loss"].is_cuda and bool(torch.isfinite(out["loss"]))
    for k, p in voc.mel2wav.named_parameters():
        assert not torch.equal(p.detach(), before[k]), k + " did not move"


def test_export_loads_through_get_vocoder_and_infers_the_trained_function(mg, stft, tmp_path):
    voc = seeded_vocoder(mg, seeded_weights())
    tr = mg.GeneratorTrainer(voc, stft)
    mel, wav = trainer_batch()
    tr.step(mel.cuda(), wav.cuda())
    path = tmp_path / "linda_johnson.pt"
    mg.vocoder_train.export_melgan_generator(voc, str(path))
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert list(sd.keys()) == list(MT.Generator().state_dict().keys())
    cfg = {"vocoder": {"model": "MelGAN", "speaker": "LJSpeech"}}
    loaded = mg.vocoder.get_vocoder(cfg, "cuda", checkpoint_path=str(path))
    pre = {"preprocessing": {"audio": {"max_wav_value": 32768.0}}}
    got = mg.vocoder.vocoder_infer(mel.cuda(), loaded, cfg, pre)
    with torch.no_grad():
        want = voc.mel2wav.forward_scaled(mel.cuda(), 1.0 / math.log(10.0)).squeeze(1) * 32768.0
    want = want.to(torch.int32).to(torch.int16).cpu().numpy()
    assert len(got) == 2
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_gan_trainer_steps_a_melvocoder_with_the_native_msd(mg, stft):
    W = seeded_weights()
    voc = seeded_vocoder(mg, W)
    torch.manual_seed(11)
    msd = mg.MultiScaleDiscriminator().cuda()
    tr = mg.VocoderGANTrainer(voc, stft, {"msd": msd})
    mel, wav = trainer_batch()
    out = tr.step(mel.cuda(), wav.cuda())
    assert set(out) == {"loss_d", "loss_g", "mel_l1", "adv", "fm"}
    for k, v in out.items():
        assert v.is_cuda and bool(torch.isfinite(v)), k
    for k, p in voc.mel2wav.named_parameters():
        assert not torch.equal(p.detach().cpu(), W[k]), k + " did not move"
