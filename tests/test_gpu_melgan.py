"""GPU parity of the native MelGAN generator (mixgan-tts_amd/melgan.py, csrc/melgan.hip) against the plain-torch
restatement of mel2wav/modules.py (tests/melgan_torch.py), evaluated in float64 on the CPU.  Bar: the vocoder's 1e-3
(max abs error / max abs reference); the measured error is printed."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import melgan_torch as MT

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def _err(out, ref):
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all()
    return float((out - ref).abs().max() / ref.abs().max())


def _reflect_conv_ref(x, w, b, d, in_slope, act):
    pad = d * (w.shape[2] - 1) // 2
    x = x.double()
    x = torch.where(x > 0, x, x * in_slope)
    y = F.conv1d(F.pad(x, (pad, pad), mode="reflect"), w.double(), b.double(), dilation=d)
    return torch.tanh(y) if act == "tanh" else y


@pytest.mark.parametrize("Ci,Co,K,d", [(32, 32, 3, 1), (32, 32, 3, 3), (32, 32, 3, 9), (64, 64, 3, 1), (64, 64, 3, 9),
                                       (256, 256, 3, 3), (256, 256, 3, 9), (80, 512, 7, 1), (32, 1, 7, 1)])
def test_reflect_conv(mg, Ci, Co, K, d):
    from mixgan_tts_amd.ops import pack_conv_weight, ACT
    from mixgan_tts_amd._lib import fptr, check, stream_ptr
    g = torch.Generator().manual_seed(Ci * 100 + Co + K + d)
    w = torch.randn(Co, Ci, K, generator=g) / (Ci * K) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    act, in_slope = ("tanh", 0.2) if Co == 1 else (None, 0.2 if K == 3 else 1.0)
    pad = d * (K - 1) // 2
    wp, bd = pack_conv_weight(w.cuda()), b.cuda()
    worst = 0.0
    for B, L in [(1, pad + 1), (2, pad + 2), (1, 127), (2, 128), (1, 129), (2, 255), (1, 256), (1, 257), (3, 700)]:
        x = torch.randn(B, Ci, L, generator=g)
        xd = x.cuda()
        out = torch.empty(B, Co, L, device="cuda")
        check(mg.lib().mg_conv1d_reflect_fwd(fptr(xd), 0, fptr(wp), fptr(bd), fptr(out), 0, B, Ci, L, Co, K,
                                             d, float(in_slope), ACT[act], 0.0, 1.0, stream_ptr()))
        e = _err(out, _reflect_conv_ref(x, w, b, d, in_slope, act))
        worst = max(worst, e)
        assert e < TOL, (B, L, e)
    print("reflect conv Ci=%d Co=%d K=%d d=%d: max rel err %.2e" % (Ci, Co, K, d, worst))


def _blocks(mg, C, seed):
    torch.manual_seed(seed)
    ref = [MT.ResnetBlock(C, 3 ** j).eval() for j in range(3)]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for r in ref:
            for name, p in r.named_parameters():
                if name.endswith("weight_g"):
                    p.copy_(torch.rand(p.shape, generator=g) * 0.4 + 0.4)
                elif name.endswith("bias"):
                    p.copy_(torch.rand(p.shape, generator=g) * 0.1 - 0.05)
    ours = []
    for j, r in enumerate(ref):
        o = mg.melgan.ResnetBlock(C, 3 ** j)
        o.load_state_dict(r.state_dict(), strict=True)
        ours.append(o.cuda())
    return ref, ours


def _stack_ref(ref, x):
    with torch.no_grad():
        h = x.double()
        for r in ref:
            h = r.double()(h)
        return h


@pytest.mark.parametrize("C", [32, 64])
def test_fused_stack_matches_restatement(mg, C):
    ref, ours = _blocks(mg, C, C)
    T = mg.lib().mg_melgan_stack_tile(C)
    g = torch.Generator().manual_seed(7)
    worst = 0.0
    for B in (1, 3):
        for L in (10, 11, 40, T - 1, T, T + 3, T + 13, T + 14, 2 * T, 5 * T + 17):
            x = torch.randn(B, C, L, generator=g)
            out = mg.melgan.residual_stack_fused(x.cuda(), ours)
            e = _err(out, _stack_ref(ref, x))
            worst = max(worst, e)
            assert e < TOL, (B, L, e)
    print("fused stack C=%d (tile %d): max rel err %.2e" % (C, T, worst))


@pytest.mark.parametrize("C", [32, 64])
def test_general_blocks_match_restatement(mg, C):
    """The general form (reflect conv into [x ; t], one K = 1 GEMM over it) at the fused stack's channel counts."""
    from mixgan_tts_amd._lib import fptr, check, stream_ptr
    ref, ours = _blocks(mg, C, C + 1)
    g = torch.Generator().manual_seed(8)
    for B, L in [(1, 10), (2, 129), (3, 1000)]:
        x = torch.randn(B, C, L, generator=g)
        buf = [torch.empty(B, 2 * C, L, device="cuda") for _ in range(2)]
        buf[0][:, :C].copy_(x.cuda())
        out = torch.empty(B, C, L, device="cuda")
        for j, o in enumerate(ours):
            o.forward_general(buf[j % 2], buf[(j + 1) % 2] if j < 2 else out, 2 * C * L if j < 2 else 0)
        e = _err(out, _stack_ref(ref, x))
        assert e < TOL, (B, L, e)


def _generator(mg, seed=0):
    ref = MT.seeded_generator(seed)
    G = mg.MelGANGenerator()
    G.load_state_dict(ref.state_dict(), strict=True)
    return ref, G.cuda().eval()


def _mel(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 80, L, generator=g) - 4.0


def _ref_wav(ref, mel):
    with torch.no_grad():
        return ref.double()(mel.double())


@pytest.mark.parametrize("B,L", [(1, 4), (3, 37), (2, 200)])
def test_generator_matches_restatement(mg, B, L):
    ref, G = _generator(mg)
    mel = _mel(B, L, B * 1000 + L)
    r = _ref_wav(ref, mel)
    for fused in (True, False):
        G.fused_stack = fused
        out = G(mel.cuda())
        assert out.shape == (B, 1, 256 * L)
        e = _err(out, r)
        print("generator B=%d L=%d fused=%s: max rel err %.2e" % (B, L, fused, e))
        assert e < TOL


def test_generator_full_size_prefix(mg):
    """B=16, L=1000 on the GPU; utterances 0 and 15 against the restatement on their first 120 frames (the receptive
    field is a few frames, so the first 100 frames' audio does not see the cut)."""
    ref, G = _generator(mg)
    mel = _mel(16, 1000, 5)
    out = G(mel.cuda())
    assert out.shape == (16, 1, 256000)
    for i in (0, 15):
        r = _ref_wav(ref, mel[i:i + 1, :, :120])[..., :25600]
        e = _err(out[i:i + 1, :, :25600], r)
        print("generator B=16 L=1000, utterance %d prefix: max rel err %.2e" % (i, e))
        assert e < TOL


def test_fused_and_general_agree(mg):
    _, G = _generator(mg, 1)
    mel = _mel(4, 300, 11).cuda()
    G.fused_stack = True
    a = G(mel)
    G.fused_stack = False
    b = G(mel)
    e = _err(a, b)
    print("fused vs general B=4 L=300: max rel diff %.2e" % e)
    assert e < TOL


def test_two_runs_bit_identical(mg):
    _, G = _generator(mg, 2)
    mel = _mel(3, 123, 12).cuda()
    for fused in (True, False):
        G.fused_stack = fused
        assert torch.equal(G(mel), G(mel))


def test_get_vocoder_and_vocoder_infer_melgan(mg, tmp_path):
    ref = MT.seeded_generator(4)
    ck = tmp_path / "linda_johnson.pt"
    torch.save({k: v.detach().clone() for k, v in ref.state_dict().items()}, ck)
    mc = {"vocoder": {"model": "MelGAN", "speaker": "LJSpeech"}}
    voc = mg.vocoder.get_vocoder(mc, "cuda", checkpoint_path=str(ck))
    assert isinstance(voc, mg.MelVocoder) and not voc.mel2wav.training
    assert "model.1.weight_g" in voc.mel2wav.state_dict()
    mel = _mel(2, 40, 13)
    pre = {"preprocessing": {"audio": {"max_wav_value": 32768.0}}}
    wavs = mg.vocoder.vocoder_infer(mel.cuda(), voc, mc, pre, lengths=[10240, 5000])
    r = _ref_wav(ref, mel / np.log(10)).squeeze(1).float().numpy()
    r16 = (r * 32768.0).astype("int16")
    assert [w.dtype.name for w in wavs] == ["int16", "int16"] and [len(w) for w in wavs] == [10240, 5000]
    for w, rr in zip(wavs, r16):
        assert np.abs(w.astype(np.int32) - rr[:len(w)].astype(np.int32)).max() <= 1
    inv = voc.inverse(mel.cuda() / math.log(10.0))
    assert inv.shape == (2, 10240)
    assert _err(inv, torch.from_numpy(r)) < TOL
