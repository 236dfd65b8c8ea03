"""GPU parity of HiFi-GAN's GAN losses (losses.hifigan_*) and of VocoderGANTrainer's step against float64 torch autograd
on the CPU (tests/hifigan_disc_ref.py).  The generator is the native one; the discriminators are torch modules (a
narrow multi-period and a small multi-scale discriminator), which is what the trainer accepts.

Error measure: max-abs error over max-abs reference (helpers.assert_close).  Bars: 2e-5 maps and
losses, 5e-5 data gradients, 1e-4 parameters; where the float32 CPU restatement's own error against float64 exceeds
bar / 8 on a tensor, that tensor's bar is 8 x that error.

Leaky-ReLU kinks (trainer): the float64 restatement adopts the GPU run's sign pattern (`masks=`), and
hifigan_disc_ref.kink_masks asserts what makes that sound: every element whose sign differs from the float64 run's own
has |pre64| <= 1e-4 max|pre64| of its tensor, and such elements are at most 1e-3 of the tensor.
"""
import json
import types

import numpy as np
import pytest
import torch

from helpers import golden, assert_close, rel_err, seeded, T
from oracle import refmath as R
import hifigan_train_ref as HR
import hifigan_disc_ref as DR

pytestmark = pytest.mark.gpu
BAR_MAP, BAR_DATA, BAR_PARAM = 2e-5, 5e-5, 1e-4
NARROW = (1, 8, 16, 32, 32, 32)      # the multi-period discriminator's channels in these tests
PERIODS = (2, 3)


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def bar_for(ref32, ref64, bar):
    """The project's fallback rule: `bar`, or 8 x the float32 CPU restatement's own error where that exceeds bar / 8."""
    e = rel_err(ref32.detach().double().numpy(), ref64.detach().numpy())
    return bar if e <= bar / 8 else 8 * e


def check(got, ref32, ref64, bar, what):
    b = bar_for(ref32, ref64, bar)
    e = rel_err(got.detach().cpu().double().numpy(), ref64.detach().numpy())
    print("%-44s err %.3e  bar %.1e" % (what, e, b))
    assert_close(got.detach().cpu().double(), ref64.detach(), b, what)


# ------------------------------------------------------------------------------------------------------------------
# 1: the three losses on lists of tensors.  5 discriminators: one launch; 9: the 18 terms of the discriminator loss take
# two; 48 feature maps: three launches.  Sizes: odd, one element, and one past a reduction workgroup's share.
# ------------------------------------------------------------------------------------------------------------------
LOSS_CASES = [(5, 6), (9, 6), (1, 1)]      # (discriminators, maps per discriminator)
_loss = {}


def loss_case(n_disc, n_maps):
    key = (n_disc, n_maps)
    if key in _loss:
        return _loss[key]
    gen = torch.Generator().manual_seed(100 * n_disc + n_maps)
    sizes = [(2, 1), (2, 37), (3, 70001), (2, 1025), (1, 5), (2, 333), (2, 64), (4, 129), (2, 4097)]
    outs_r = [torch.randn(sizes[i % len(sizes)], generator=gen) * 0.7 + 0.5 for i in range(n_disc)]
    outs_g = [torch.randn(sizes[i % len(sizes)], generator=gen) * 0.7 for i in range(n_disc)]
    shapes = [(2, 3, 17, 2), (2, 5, 7, 3), (2, 8, 1, 5), (2, 1, 41), (2, 16, 301), (2, 1, 1, 11)]
    fr = [[torch.randn(shapes[(i + j) % len(shapes)], generator=gen) for j in range(n_maps)] for i in range(n_disc)]
    fg = [[torch.randn(shapes[(i + j) % len(shapes)], generator=gen) for j in range(n_maps)] for i in range(n_disc)]
    res = {"in": (outs_r, outs_g, fr, fg)}
    for dt in (torch.float64, torch.float32):
        lr_ = [t.to(dt, copy=True).requires_grad_() for t in outs_r]
        lg_ = [t.to(dt, copy=True).requires_grad_() for t in outs_g]
        fr_ = [[t.to(dt, copy=True).requires_grad_() for t in d] for d in fr]
        fg_ = [[t.to(dt, copy=True).requires_grad_() for t in d] for d in fg]
        d_total, r_losses, g_losses = DR.discriminator_loss(lr_, lg_)
        d_total.backward()
        d_grads = ([t.grad.clone() for t in lr_], [t.grad.clone() for t in lg_])
        for t in lg_:
            t.grad = None
        g_total, gen_losses = DR.generator_loss(lg_)
        fm = DR.feature_loss(fr_, fg_)
        (g_total + fm).backward()
        res[dt] = {"d_total": d_total.detach(), "r_losses": r_losses, "g_losses": g_losses, "d_grads": d_grads,
                   "g_total": g_total.detach(), "gen_losses": gen_losses, "fm": fm.detach(),
                   "g_grads": [t.grad for t in lg_], "fm_grads": [[t.grad for t in d] for d in fg_]}
    _loss[key] = res
    return res


@pytest.mark.parametrize("n_disc,n_maps", LOSS_CASES)
def test_discriminator_loss(mg, n_disc, n_maps):
    c = loss_case(n_disc, n_maps)
    r64, r32 = c[torch.float64], c[torch.float32]
    lr_ = [t.cuda().requires_grad_() for t in c["in"][0]]
    lg_ = [t.cuda().requires_grad_() for t in c["in"][1]]
    total, r_losses, g_losses = mg.hifigan_discriminator_loss(lr_, lg_)
    assert total.is_cuda and total.dim() == 0 and len(r_losses) == len(g_losses) == n_disc
    check(total.reshape(1), r32["d_total"].reshape(1), r64["d_total"].reshape(1), BAR_MAP, "discriminator loss")
    check(torch.stack(r_losses), torch.stack(r32["r_losses"]), torch.stack(r64["r_losses"]), BAR_MAP, "r_losses")
    check(torch.stack(g_losses), torch.stack(r32["g_losses"]), torch.stack(r64["g_losses"]), BAR_MAP, "g_losses")
    assert not any(v.requires_grad for v in r_losses + g_losses)
    total.backward()
    for i in range(n_disc):
        check(lr_[i].grad, r32["d_grads"][0][i], r64["d_grads"][0][i], BAR_DATA, "d loss / d real[%d]" % i)
        check(lg_[i].grad, r32["d_grads"][1][i], r64["d_grads"][1][i], BAR_DATA, "d loss / d generated[%d]" % i)


@pytest.mark.parametrize("n_disc,n_maps", LOSS_CASES)
def test_generator_and_feature_loss(mg, n_disc, n_maps):
    c = loss_case(n_disc, n_maps)
    r64, r32 = c[torch.float64], c[torch.float32]
    lg_ = [t.cuda().requires_grad_() for t in c["in"][1]]
    fr_ = [[t.cuda().requires_grad_() for t in d] for d in c["in"][2]]
    fg_ = [[t.cuda().requires_grad_() for t in d] for d in c["in"][3]]
    adv, gen_losses = mg.hifigan_generator_loss(lg_)
    fm = mg.hifigan_feature_loss(fr_, fg_)
    assert len(gen_losses) == n_disc and fm.dim() == 0 and adv.dim() == 0
    check(adv.reshape(1), r32["g_total"].reshape(1), r64["g_total"].reshape(1), BAR_MAP, "generator loss")
    check(torch.stack(gen_losses), torch.stack(r32["gen_losses"]), torch.stack(r64["gen_losses"]), BAR_MAP, "gen_losses")
    check(fm.reshape(1), r32["fm"].reshape(1), r64["fm"].reshape(1), BAR_MAP, "feature loss")
    (adv + fm).backward()
    for i in range(n_disc):
        check(lg_[i].grad, r32["g_grads"][i], r64["g_grads"][i], BAR_DATA, "d adv / d generated[%d]" % i)
        for j in range(n_maps):
            check(fg_[i][j].grad, r32["fm_grads"][i][j], r64["fm_grads"][i][j], BAR_DATA, "d fm / d fmap_g[%d][%d]" % (i, j))
            assert fr_[i][j].grad is None, "the real maps are targets"
    # a second evaluation gives the same bits
    adv2, _ = mg.hifigan_generator_loss([t.detach() for t in lg_])
    fm2 = mg.hifigan_feature_loss(fr_, [[t.detach() for t in d] for d in fg_])
    assert torch.equal(adv2, adv.detach()) and torch.equal(fm2, fm.detach())


# ------------------------------------------------------------------------------------------------------------------
# 2: trainer
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


def trainer_batch():
    rng = np.random.default_rng(7)
    mel = torch.from_numpy(rng.uniform(-11.5, 2.0, (2, 80, 4)).astype(np.float32))
    wav = torch.from_numpy(rng.uniform(-0.9, 0.9, (2, 1024)).astype(np.float32))
    return mel, wav


@pytest.fixture(scope="module")
def stft(mg):
    return mg.audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)


def mpd_fwd(W, y, y_hat, taps=None, masks=None):
    return DR.mpd_forward(W, y, y_hat, taps, masks, PERIODS)


def build_trainer(mg, manifest, stft, **kw):
    Wg, Wp, Ws = seeded_weights(manifest), DR.mpd_init(4, PERIODS, NARROW), DR.small_msd_init(5)
    G = mg.vocoder.Generator(_h())
    G.load_state_dict({k: v.detach().clone() for k, v in Wg.items()})
    discs = {"mpd": DR.TorchMPD(Wp, PERIODS).cuda(), "msd": DR.SmallMSD(Ws).cuda()}
    return mg.VocoderGANTrainer(G.cuda(), stft, discs, **kw), Wg, Wp, Ws


def test_trainer_sgd_two_steps_match_float64(mg, manifest, stft):
    """lr = 1e-5 for the generator, 1e-3 for the discriminators: in the float64 restatement loss_g goes 69.78 -> 67.70
    (3 % a step against a bar of 2e-5), and a discriminator step moves the adversarial + feature terms by 2.5 %, so a
    generator phase that ran through the OLD discriminators would fail."""
    LR, LR_D = 1e-5, 1e-3
    tr, Wg, Wp, Ws = build_trainer(mg, manifest, stft, optimizer=torch.optim.SGD, lr=LR)
    for group in tr.optim_d.param_groups:
        group["lr"] = LR_D
    mel, wav = trainer_batch()
    win, basis = stft.stft_fn._tables.window.double(), stft.mel_basis.double().cpu()
    fwd = {"mpd": mpd_fwd, "msd": DR.small_msd_forward}
    prefix = {"mpd": "discriminators", "msd": "scales"}
    state = {dt: {"g": {k: v.detach().to(dt, copy=True).requires_grad_() for k, v in Wg.items()},
                  "mpd": {k: v.detach().to(dt, copy=True).requires_grad_() for k, v in Wp.items()},
                  "msd": {k: v.detach().to(dt, copy=True).requires_grad_() for k, v in Ws.items()}}
             for dt in (torch.float64, torch.float32)}
    got, ref, stale = [], {torch.float64: [], torch.float32: []}, []
    for step in range(2):
        taps = {}
        got.append(tr.step(mel.cuda(), wav.cuda(), taps=taps))
        for dt, st in state.items():
            y = wav.to(dt)[:, None, :]
            first = dt == torch.float64
            discs = {n: (fwd[n], st[n]) for n in ("mpd", "msd")}
            if first:       # the float64 run's own signs against the GPU run's, phase by phase
                own_g = {}
                with torch.no_grad():
                    y_own = HR.generator_forward(st["g"], mel.to(dt), taps=own_g)
                masks = {"generator": DR.kink_masks(taps["generator"], own_g)}
                own_d = {}
                with torch.no_grad():
                    DR.d_phase_loss(discs, y, y_own, taps=own_d)
                    stale.append(sum(DR.g_phase_loss(discs, y, y_own)))      # through the discriminators BEFORE their step
                masks["d"] = {n: DR.kink_masks(DR.taps_of_fmaps(prefix[n], *taps["d"][n]), own_d[n]) for n in discs}
            y_hat = HR.generator_forward(st["g"], mel.to(dt), masks=masks["generator"])
            for n in discs:
                for v in st[n].values():
                    v.grad = None
            loss_d = DR.d_phase_loss(discs, y, y_hat, masks=masks["d"])
            loss_d.backward()
            with torch.no_grad():
                for n in discs:
                    for v in st[n].values():
                        v -= LR_D * v.grad
            if first:
                own_gp = {}
                with torch.no_grad():
                    DR.g_phase_loss(discs, y, y_hat.detach(), taps=own_gp)
                masks["g"] = {n: DR.kink_masks(DR.taps_of_fmaps(prefix[n], *taps["g"][n]), own_gp[n]) for n in discs}
            for v in st["g"].values():
                v.grad = None
            for n in discs:
                for v in st[n].values():
                    v.requires_grad_(False)
            adv, fm = DR.g_phase_loss(discs, y, y_hat, masks=masks["g"])
            mel_l1 = (HR.log_mel(y_hat[:, 0], win, basis) - HR.log_mel(wav.to(dt), win, basis)).abs().mean()
            loss_g = adv + fm + 45.0 * mel_l1
            loss_g.backward()
            for n in discs:
                for v in st[n].values():
                    v.requires_grad_(True)
            with torch.no_grad():
                for v in st["g"].values():
                    v -= LR * v.grad
            ref[dt].append({"loss_d": loss_d.detach(), "loss_g": loss_g.detach(), "mel_l1": mel_l1.detach(),
                            "adv": adv.detach(), "fm": fm.detach()})
    r64 = ref[torch.float64]
    for i in range(2):
        fresh = float(r64[i]["adv"] + r64[i]["fm"])
        assert abs(fresh - float(stale[i])) > 100 * BAR_MAP * abs(fresh), "the generator phase does not see the D step"
        assert set(got[i]) == {"loss_d", "loss_g", "mel_l1", "adv", "fm"}
        for k, v in got[i].items():
            assert v.is_cuda and v.dim() == 0 and not v.requires_grad, k
            check(v.reshape(1), ref[torch.float32][i][k].reshape(1), r64[i][k].reshape(1), BAR_MAP,
                  "%s of step %d" % (k, i))
    assert abs(float(r64[1]["loss_g"] - r64[0]["loss_g"])) > 100 * BAR_MAP * float(r64[0]["loss_g"]), \
        "the second step does not see the update"
    for k, p in tr.generator.named_parameters():
        check(p, state[torch.float32]["g"][k], state[torch.float64]["g"][k].detach(), BAR_PARAM, "post-step G " + k)
    for n in ("mpd", "msd"):
        for k, p in tr.discriminators[n].dict().items():
            check(p, state[torch.float32][n][k], state[torch.float64][n][k].detach(), BAR_PARAM,
                  "post-step %s %s" % (n, k))
    assert tr.steps == 2
    assert all(p.requires_grad for d in tr.discriminators.values() for p in d.parameters())


def test_hifigan_step_computes_the_mel_term_at_weight_zero(mg, manifest, stft):
    """objective="hifigan" with lambda_mel = 0 still evaluates the mel term (only objective="melgan" may skip it):
    "mel_l1" is the real value, the bits of _mel_l1 on the pre-step weights, and loss_g is adv + fm."""
    tr, _, _, _ = build_trainer(mg, manifest, stft, lambda_mel=0.0)
    mel, wav = (t.cuda() for t in trainer_batch())
    with torch.no_grad():
        expected = mg.vocoder_train._mel_l1(stft, tr.generator.forward_train(mel).squeeze(1), wav)
    out = tr.step(mel, wav)
    print("mel_l1 %.6f (expected %.6f)  loss_g %.6f  adv %.6f  fm %.6f"
          % tuple(float(v) for v in (out["mel_l1"], expected, out["loss_g"], out["adv"], out["fm"])))
    assert bool(torch.isfinite(out["mel_l1"])) and float(out["mel_l1"]) != 0.0
    assert torch.equal(out["mel_l1"], expected)
    assert torch.equal(out["loss_g"], out["adv"] + out["fm"])


def test_trainer_defaults_and_checkpoint(mg, manifest, stft, tmp_path):
    tr, Wg, Wp, _ = build_trainer(mg, manifest, stft)
    assert isinstance(tr.optim_g, torch.optim.AdamW) and isinstance(tr.optim_d, torch.optim.AdamW)
    mel, wav = trainer_batch()
    out = [tr.step(mel.cuda(), wav.cuda()) for _ in range(2)]
    assert all(bool(torch.isfinite(v)) for o in out for v in o.values())
    G, mpd = tr.generator, tr.discriminators["mpd"]
    assert not torch.equal(G.conv_post.weight_v.detach().cpu(), Wg["conv_post.weight_v"])
    k = "discriminators.1.convs.4.weight_v"
    assert not torch.equal(mpd.dict()[k].detach().cpu(), Wp[k])
    ck = tmp_path / "do_00000002"
    tr.save(str(ck))
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps(R.HIFIGAN_V1))
    voc = mg.vocoder.get_vocoder({"vocoder": {"model": "HiFi-GAN", "speaker": "LJSpeech"}}, "cuda", config_path=str(cfg),
                                 checkpoint_path=str(ck))
    tr2, _, _, _ = build_trainer(mg, manifest, stft)
    assert tr2.load(str(ck)).steps == 2
    for name in ("mpd", "msd"):
        for (ka, a), (_, b) in zip(tr.discriminators[name].state_dict().items(),
                                   tr2.discriminators[name].state_dict().items()):
            assert torch.equal(a, b), ka
    for (ka, a), (_, b) in zip(G.state_dict().items(), tr2.generator.state_dict().items()):
        assert torch.equal(a, b), ka
    # the loaded optimizer state continues the run: the third step of both trainers agrees (Adam's moments came along)
    a, b = tr.step(mel.cuda(), wav.cuda()), tr2.step(mel.cuda(), wav.cuda())
    for k in a:
        assert_close(b[k].reshape(1), a[k].reshape(1), 1e-4, "third step, " + k)
    # get_vocoder holds the checkpoint's generator (two steps)
    tr3, _, _, _ = build_trainer(mg, manifest, stft)
    G3 = tr3.load(str(ck)).generator.eval()
    G3.cpu().remove_weight_norm()          # on the host, where get_vocoder folds the norm
    G3.cuda()
    assert torch.equal(voc(mel.cuda()), G3(mel.cuda()))
