"""HiFi-GAN training on the HIP path: vocoder.Generator.forward_train (the generator's one walk with its training sites),
the mel-reconstruction loss through audio.TacotronSTFT.mel_spectrogram_diff, and checkpoints that vocoder.get_vocoder
loads.  The two trainers share the optimizer rule, the mel-L1 term and the checkpoint helpers below.

GeneratorTrainer trains on the mel term alone.  VocoderGANTrainer is HiFi-GAN's full step: the discriminator phase and
the generator phase with the adversarial and feature-matching terms (losses.hifigan_*: the fused HIP loss kernels), over
any discriminator modules with the published calling convention.  Both of HiFi-GAN's are native
(hifigan_discriminators.MultiScaleDiscriminator and MultiPeriodDiscriminator); a torch module with the same forward works too.

Both trainers need only .parameters(), .forward_train(mel[, taps]) and .state_dict() of their generator, so a
melgan.MelVocoder trains in them as a vocoder.Generator does; export_melgan_generator writes what get_vocoder loads for
MelGAN.
"""
import collections

import torch
import torch.nn.functional as F

from . import _lib
from .losses import hifigan_discriminator_loss, hifigan_generator_loss, hifigan_feature_loss
from .losses import melgan_discriminator_loss, melgan_generator_loss, melgan_feature_loss


def sample_segments(mels, wavs, mel_lens, frames=32, generator=None, hop=256):
    """Cut one aligned training segment per utterance (HiFi-GAN's segment_size = frames * hop samples).

    mels [B, n_mels, Fmax], wavs [B, >= hop * Fmax], mel_lens: the utterances' frame counts (each >= frames).
    Returns (mel [B, n_mels, frames], wav [B, hop * frames], offsets [B] int64 on the host): the wav slice of item b
    starts at hop * offsets[b], and offsets[b] + frames <= mel_lens[b].  `generator`: a CPU torch.Generator."""
    lens = [int(v) for v in (mel_lens.tolist() if isinstance(mel_lens, torch.Tensor) else mel_lens)]
    if len(lens) != mels.shape[0] or wavs.shape[0] != mels.shape[0]:
        raise ValueError("sample_segments: %d mels, %d wavs, %d lengths" % (mels.shape[0], wavs.shape[0], len(lens)))
    offs = []
    for b, n in enumerate(lens):
        if n < frames or n > mels.shape[2] or hop * n > wavs.shape[1]:
            raise ValueError("sample_segments: item %d has %d frames; needs %d <= frames <= %d and %d samples"
                             % (b, n, frames, mels.shape[2], hop * n))
        offs.append(int(torch.randint(0, n - frames + 1, (1,), generator=generator)))
    mel = torch.stack([mels[b, :, o:o + frames] for b, o in enumerate(offs)]).contiguous()
    wav = torch.stack([wavs[b, hop * o:hop * (o + frames)] for b, o in enumerate(offs)]).contiguous()
    return mel, wav, torch.tensor(offs, dtype=torch.int64)


def _optimizer(optimizer, params, lr, betas):
    """None -> torch.optim.AdamW; a class is built as optimizer(params, lr=lr); an instance is used as it is."""
    if optimizer is None:
        return torch.optim.AdamW(params, lr=lr, betas=betas)
    return optimizer(params, lr=lr) if isinstance(optimizer, type) else optimizer


def _mel_l1(stft, y_hat, y):
    """L1 between the differentiable log-mel of y_hat [B, N] and the log-mel of y [B, N], over the common frames."""
    m_hat = stft.mel_spectrogram_diff(y_hat)
    with torch.no_grad():
        m_ref = stft.mel_spectrogram_diff(y)
    T = min(m_hat.shape[2], m_ref.shape[2])
    return F.l1_loss(m_hat[:, :, :T], m_ref[:, :, :T])


def _cpu_state(module):
    return {k: v.detach().cpu() for k, v in module.state_dict().items()}


def export_melgan_generator(vocoder, path):
    """Write the bare `mel2wav` state dict of a melgan.MelVocoder (or of a MelGANGenerator) -- the layout of the
    melgan-neurips hub files -- which vocoder.get_vocoder({"vocoder": {"model": "MelGAN", ...}}, checkpoint_path=path)
    loads."""
    torch.save(_cpu_state(getattr(vocoder, "mel2wav", vocoder)), path)


def _load_present(ckpt, **targets):
    for key, obj in targets.items():
        if key in ckpt:
            obj.load_state_dict(ckpt[key])


class GeneratorTrainer:
    """One optimizer over a vocoder.Generator with the mel term of HiFi-GAN's generator loss.

    Defaults: hifigan/config.json (learning_rate 2e-4, adam_b1 0.8, adam_b2 0.99, lr_decay 0.999 per epoch) and the
    paper's lambda_mel = 45.  optimizer: None -> torch.optim.AdamW; a class is built as optimizer(params, lr=lr);
    an instance is used as it is."""

    def __init__(self, generator, stft, optimizer=None, lr=2e-4, betas=(0.8, 0.99), lr_decay=0.999, lambda_mel=45.0):
        self.generator = generator
        self.stft = stft
        self.lambda_mel = float(lambda_mel)
        params = [p for p in generator.parameters() if p.requires_grad]
        self.optimizer = _optimizer(optimizer, params, lr, betas)
        self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, gamma=lr_decay)
        self.steps = 0

    def loss(self, mel, wav):
        """(lambda_mel * L1(mel_diff(G(mel)), mel(wav)) over the common frames, G(mel) [B, 1, N])."""
        y_hat = self.generator.forward_train(mel)
        if wav.dim() == 3:
            wav = wav.squeeze(1)
        return self.lambda_mel * _mel_l1(self.stft, y_hat.squeeze(1), wav), y_hat

    def step(self, mel, wav):
        """mel [B, 80, F], wav [B, 256 F]: forward, loss, backward, optimizer step.  Returns {"loss", "mel_l1"} as
        device scalars; nothing here reads the device."""
        if not mel.is_cuda or not wav.is_cuda:
            raise _lib.MixganHipError("GeneratorTrainer.step: tensors must be on the GPU (no CPU fallback)")
        self.optimizer.zero_grad(set_to_none=True)
        loss, _ = self.loss(mel, wav)
        loss.backward()
        self.optimizer.step()
        self.steps += 1
        loss = loss.detach()
        return {"loss": loss, "mel_l1": loss / self.lambda_mel}

    def end_epoch(self):
        """lr *= lr_decay (hifigan train.py steps its ExponentialLR once per epoch)."""
        self.scheduler.step()

    def save(self, path):
        """{"generator": state_dict, ...}: the layout vocoder.get_vocoder(..., checkpoint_path=path) loads."""
        torch.save({"generator": _cpu_state(self.generator), "optimizer": self.optimizer.state_dict(),
                    "scheduler": self.scheduler.state_dict(), "steps": self.steps}, path)

    def load(self, path):
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        self.generator.load_state_dict(ckpt["generator"])
        _load_present(ckpt, optimizer=self.optimizer, scheduler=self.scheduler)
        self.steps = int(ckpt.get("steps", 0))
        return self


# What VocoderGANTrainer.step takes from its objective.  call(d, y, y_hat) -> one discriminator's outputs `out`;
# tap(out): what taps["d"] / taps["g"] record; d_loss(out): the D-phase term; adv_fm(out): the G-phase pair.
# weighs_fm: fm enters the total times lambda_feat.  mel_optional: lambda_mel == 0 skips the mel term's computation.
_Objective = collections.namedtuple("_Objective", "call tap d_loss adv_fm weighs_fm mel_optional")
_OBJECTIVES = {
    "hifigan": _Objective(      # out = (y_d_rs, y_d_gs, fmap_rs, fmap_gs)
        call=lambda d, y, y_hat: d(y, y_hat),
        tap=lambda out: (out[2], out[3]),
        d_loss=lambda out: hifigan_discriminator_loss(out[0], out[1])[0],
        adv_fm=lambda out: (hifigan_generator_loss(out[1])[0], hifigan_feature_loss(out[2], out[3])),
        weighs_fm=False, mel_optional=False),
    "melgan": _Objective(       # out = (D_real, D_fake)
        call=lambda d, y, y_hat: d.forward_pair(y, y_hat),
        tap=tuple,
        d_loss=lambda out: melgan_discriminator_loss(out[0], out[1]),
        adv_fm=lambda out: (melgan_generator_loss(out[1]), melgan_feature_loss(out[0], out[1])),
        weighs_fm=True, mel_optional=True),
}


class VocoderGANTrainer:
    """HiFi-GAN's training step (Kong et al. 2020, train.py) over a vocoder.Generator and a dict name -> discriminator.

    A discriminator is any module whose forward(y, y_hat) on [B, 1, T] tensors returns (y_d_rs, y_d_gs, fmap_rs,
    fmap_gs) -- per sub-discriminator the logits of the real and of the generated half, and their lists of feature
    maps -- as the published MultiPeriodDiscriminator / MultiScaleDiscriminator do.  Defaults as GeneratorTrainer: two
    AdamW optimizers (2e-4, betas 0.8 / 0.99), two ExponentialLR(0.999) schedulers stepped by end_epoch(),
    lambda_mel = 45.
    optimizer: None -> torch.optim.AdamW; a class is built as optimizer(params, lr=lr) for each side.

    objective="melgan" is MelGAN's step (Kumar et al. 2019, scripts/train.py) in the same frame: a discriminator is a
    melgan_discriminators.Discriminator, called as forward_pair(y, y_hat) -> (D_real, D_fake), one list of maps per
    scale; the D phase is the hinge loss, the G phase adv + lambda_feat * fm + lambda_mel * mel_l1 with the hinge
    generator term and the weighted feature matching of losses.melgan_*.  lambda_mel = 0 (upstream has no mel term)
    skips the mel term's computation; "mel_l1" is then a zero.  taps "d" / "g" hold (D_real, D_fake)."""

    def __init__(self, generator, stft, discriminators, optimizer=None, lr=2e-4, betas=(0.8, 0.99), lr_decay=0.999,
                 lambda_mel=45.0, objective="hifigan", lambda_feat=10.0):
        if objective not in _OBJECTIVES:
            raise ValueError("objective: 'hifigan' or 'melgan', got %r" % (objective,))
        self.objective = objective
        self.lambda_feat = float(lambda_feat)
        if not discriminators:
            raise ValueError("VocoderGANTrainer needs at least one discriminator")
        for name in discriminators:
            if name in ("generator", "optim_g", "optim_d", "sched_g", "sched_d", "steps"):
                raise ValueError("discriminator name %r is a checkpoint key" % name)
        self.generator = generator
        self.stft = stft
        self.discriminators = dict(discriminators)
        self.lambda_mel = float(lambda_mel)
        g_params = [p for p in generator.parameters() if p.requires_grad]
        self._d_params = [p for d in self.discriminators.values() for p in d.parameters() if p.requires_grad]
        if optimizer is not None and not isinstance(optimizer, type):
            raise TypeError("optimizer: None or an optimizer class (two instances are built)")
        self.optim_g, self.optim_d = (_optimizer(optimizer, ps, lr, betas) for ps in (g_params, self._d_params))
        self.scheduler_g = torch.optim.lr_scheduler.ExponentialLR(self.optim_g, gamma=lr_decay)
        self.scheduler_d = torch.optim.lr_scheduler.ExponentialLR(self.optim_d, gamma=lr_decay)
        self.steps = 0

    def step(self, mel, wav, taps=None):
        """mel [B, 80, F], wav [B, 256 F] (or [B, 1, 256 F]).  y_hat = G(mel); the discriminators learn on
        y_hat.detach() and step; then the generator learns on lambda_mel * mel L1 + adversarial + feature matching
        through the UPDATED discriminators, whose parameters need no gradient for the duration, and steps.
        Returns {"loss_d", "loss_g", "mel_l1", "adv", "fm"} as device scalars; nothing here reads the device.
        taps: a dict that receives what fixes the step's leaky-ReLU sign patterns: "generator" (forward_train's taps)
        and "d" / "g": name -> (fmap_rs, fmap_gs) of the discriminator and of the generator phase.  _OBJECTIVES holds
        what objective="melgan" does differently (the class docstring)."""
        if not mel.is_cuda or not wav.is_cuda:
            raise _lib.MixganHipError("VocoderGANTrainer.step: tensors must be on the GPU (no CPU fallback)")
        y = wav.unsqueeze(1) if wav.dim() == 2 else wav
        if taps is not None:
            taps.update({"generator": {}, "d": {}, "g": {}})
        y_hat = self.generator.forward_train(mel, None if taps is None else taps["generator"])
        if y_hat.shape != y.shape:
            raise ValueError("wav must be %s, got %s" % (tuple(y_hat.shape), tuple(y.shape)))
        obj = _OBJECTIVES[self.objective]

        self.optim_d.zero_grad(set_to_none=True)
        y_hat_d = y_hat.detach()
        loss_d = None
        for name, d in self.discriminators.items():
            out = obj.call(d, y, y_hat_d)
            if taps is not None:
                taps["d"][name] = obj.tap(out)
            part = obj.d_loss(out)
            loss_d = part if loss_d is None else loss_d + part
        loss_d.backward()
        self.optim_d.step()

        self.optim_g.zero_grad(set_to_none=True)
        skip_mel = obj.mel_optional and self.lambda_mel == 0.0
        mel_l1 = None if skip_mel else _mel_l1(self.stft, y_hat.squeeze(1), y.squeeze(1))
        for p in self._d_params:
            p.requires_grad_(False)
        try:
            adv = fm = None
            for name, d in self.discriminators.items():
                out = obj.call(d, y, y_hat)
                if taps is not None:
                    taps["g"][name] = obj.tap(out)
                a, f = obj.adv_fm(out)
                adv, fm = (a, f) if adv is None else (adv + a, fm + f)
            loss_g = adv + (self.lambda_feat * fm if obj.weighs_fm else fm)
            if mel_l1 is not None:
                loss_g = loss_g + self.lambda_mel * mel_l1
            loss_g.backward()
        finally:
            for p in self._d_params:
                p.requires_grad_(True)
        self.optim_g.step()
        self.steps += 1
        mel_l1 = torch.zeros_like(loss_g.detach()) if mel_l1 is None else mel_l1.detach()
        return {"loss_d": loss_d.detach(), "loss_g": loss_g.detach(), "mel_l1": mel_l1, "adv": adv.detach(),
                "fm": fm.detach()}

    def end_epoch(self):
        """lr *= lr_decay on both sides, once per epoch."""
        self.scheduler_g.step()
        self.scheduler_d.step()

    def save(self, path):
        """{"generator": state_dict, <name>: state_dict per discriminator, "optim_g", "optim_d", "steps", ...}: the
        "generator" entry is what vocoder.get_vocoder(..., checkpoint_path=path) loads."""
        ckpt = {name: _cpu_state(m) for name, m in [("generator", self.generator), *self.discriminators.items()]}
        ckpt.update({"optim_g": self.optim_g.state_dict(), "optim_d": self.optim_d.state_dict(),
                     "sched_g": self.scheduler_g.state_dict(), "sched_d": self.scheduler_d.state_dict(),
                     "steps": self.steps})
        torch.save(ckpt, path)

    def load(self, path):
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        self.generator.load_state_dict(ckpt["generator"])
        for name, d in self.discriminators.items():
            d.load_state_dict(ckpt[name])
        _load_present(ckpt, optim_g=self.optim_g, optim_d=self.optim_d, sched_g=self.scheduler_g,
                      sched_d=self.scheduler_d)
        self.steps = int(ckpt.get("steps", 0))
        return self
