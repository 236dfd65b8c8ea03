"""Generator half of HiFi-GAN training on the HIP path: vocoder.Generator.forward_train, HiFi-GAN's mel-reconstruction
loss through audio.TacotronSTFT.mel_spectrogram_diff, and checkpoints that vocoder.get_vocoder loads.

The MPD / MSD discriminators and the adversarial and feature-matching terms are not here; forward_train returns an
ordinary autograd tensor, so any PyTorch loss or discriminator can be put on top of it.
"""
import torch
import torch.nn.functional as F

from . import _lib


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
        if optimizer is None:
            optimizer = torch.optim.AdamW(params, lr=lr, betas=betas)
        elif isinstance(optimizer, type):
            optimizer = optimizer(params, lr=lr)
        self.optimizer = optimizer
        self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimizer, gamma=lr_decay)
        self.steps = 0

    def loss(self, mel, wav):
        """(lambda_mel * L1(mel_diff(G(mel)), mel(wav)) over the common frames, G(mel) [B, 1, N])."""
        y_hat = self.generator.forward_train(mel)
        if wav.dim() == 3:
            wav = wav.squeeze(1)
        m_hat = self.stft.mel_spectrogram_diff(y_hat.squeeze(1))
        with torch.no_grad():
            m_ref = self.stft.mel_spectrogram_diff(wav)
        T = min(m_hat.shape[2], m_ref.shape[2])
        return self.lambda_mel * F.l1_loss(m_hat[:, :, :T], m_ref[:, :, :T]), y_hat

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
        torch.save({"generator": {k: v.detach().cpu() for k, v in self.generator.state_dict().items()},
                    "optimizer": self.optimizer.state_dict(), "scheduler": self.scheduler.state_dict(),
                    "steps": self.steps}, path)

    def load(self, path):
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        self.generator.load_state_dict(ckpt["generator"])
        if "optimizer" in ckpt:
            self.optimizer.load_state_dict(ckpt["optimizer"])
        if "scheduler" in ckpt:
            self.scheduler.load_state_dict(ckpt["scheduler"])
        self.steps = int(ckpt.get("steps", 0))
        return self
