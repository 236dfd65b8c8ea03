"""HiFi-GAN V1 generator (hifigan/models.py:112-173) on the HIP conv kernel -- SURVEY.md section 8 f3,
the step right after the path (mel [B, 80, L] -> waveform [B, 1, 256 L]; `utils/model.py:108-126`).

Same constructor (`Generator(h)` with the attribute-style config of hifigan/config.json), parameter
names (`conv_pre`, `ups.{i}`, `resblocks.{j}.convs{1,2}.{m}`, `conv_post`, each with `weight_g` /
`weight_v` / `bias`, or `weight` / `bias` after `remove_weight_norm()`), and forward as the
reference, so its checkpoints load unchanged (none ship with the reference: `.MISSING_LARGE_BLOBS`).

Kernel mapping: every Conv1d (k in {3,7,11}, dilation in {1,3,5}) is the MFMA implicit-GEMM conv with
the pre-activation leaky ReLU applied while the input tile is staged and the post-activation / residual
add in the epilogue; ConvTranspose1d (k = 2*stride) is a polyphase 3-tap GEMM over the input (leaky ReLU
fused in staging, phases interleaved by the epilogue; other (k, stride) fall back to zero insertion plus a
stride-1 convolution on the transposed, tap-flipped pack); the three ResBlocks of a stage accumulate into
one buffer and the 1/3 is folded into the next convolution (leaky ReLU is positively homogeneous).

The network is walked in one place, Generator._walk, with one of two site sets: _Infer (`forward`: no_grad, cached packs,
post-activations fused into epilogues) or _Train (`forward_train`: autograd Functions that keep each pre-activation and
differentiate in csrc/vocoder_train.hip; weight norm stays a torch expression).  vocoder_train's trainers put HiFi-GAN's
mel loss and the full GAN step on forward_train (both discriminators are native, hifigan_discriminators.py: the
multi-scale one on csrc/msd.hip, the multi-period one on csrc/mpd.hip).
"""
import math

import torch
from torch import nn

from . import ops, _lib, autograd as ag

LRELU_SLOPE = 0.1


class _WNConv(nn.Module):
    """Parameter holder of weight_norm(Conv1d / ConvTranspose1d): weight_g [C0,1,1], weight_v [C0,C1,K], bias."""

    def __init__(self, shape, bias_n, std=None):
        super().__init__()
        v = torch.empty(*shape)
        if std is None:
            nn.init.kaiming_uniform_(v, a=5 ** 0.5)
        else:
            v.normal_(0.0, std)           # init_weights (hifigan/models.py:10-13)
        self.weight_v = nn.Parameter(v)
        self.weight_g = nn.Parameter(v.detach().flatten(1).norm(dim=1).view(-1, 1, 1).clone())
        self.bias = nn.Parameter(torch.zeros(bias_n).uniform_(-0.05, 0.05))

    def effective_weight(self):
        if "weight" in self._parameters:
            return self.weight
        return ag.weight_norm(self.weight_v, self.weight_g)

    def remove_weight_norm(self):
        if "weight" not in self._parameters:
            w = self.effective_weight().detach().clone()
            del self.weight_g, self.weight_v
            self.weight = nn.Parameter(w)

    def packed(self, mode):
        """MFMA pack of the effective weight, cached until a parameter changes."""
        ps = [p for p in self.parameters()]
        key = (mode,) + tuple((p.data_ptr(), p._version) for p in ps)
        hit = self.__dict__.get("_mg_pack")
        if hit is None or hit[0] != key:
            with torch.no_grad():
                w = self.effective_weight().contiguous()
                hit = (key, ops.pack_conv_transpose_weight(w) if mode == ops.PACK_TPOSE else ops.pack_conv_weight(w, mode))
            self.__dict__["_mg_pack"] = hit
        return hit[1]


class ResBlock(nn.Module):
    """hifigan/models.py:20-109."""

    def __init__(self, h, channels, kernel_size=3, dilation=(1, 3, 5)):
        super().__init__()
        self.h, self.kernel_size, self.dilation = h, kernel_size, tuple(dilation)
        self.convs1 = nn.ModuleList([_WNConv((channels, channels, kernel_size), channels, 0.01) for _ in dilation])
        self.convs2 = nn.ModuleList([_WNConv((channels, channels, kernel_size), channels, 0.01) for _ in dilation])

    def remove_weight_norm(self):
        for l in list(self.convs1) + list(self.convs2):
            l.remove_weight_norm()


def _polyphase(k, u):
    """The upsamplers with a polyphase kernel (forward and backward): kernel = 2 * stride, stride in {2, 4, 8}."""
    return k == 2 * u and u in (2, 4, 8)


class _Infer:
    """Generator._walk's sites in inference: cached packs, detached biases, activations and sums in the epilogues."""

    @staticmethod
    def conv(c, x, Co, k, pad, in_slope=1.0, alpha=1.0, act=None):
        return ops.conv1d_packed(x, c.packed(ops.PACK_PLAIN), c.bias.detach(), Co, k, 1, pad, act=act, alpha=alpha,
                                 in_slope=in_slope)

    @staticmethod
    def up(c, x, Co, k, u, slope, alpha):
        if _polyphase(k, u):                  # 3-tap GEMM with Co*u rows, lrelu fused in staging
            return ops.conv_transpose1d_packed(x, c.packed(ops.PACK_TPOSE), c.bias.detach(), Co, u, in_slope=slope,
                                               alpha=alpha)
        L = x.shape[2]                        # general (k, u): lrelu + zero insertion, flipped stride-1 conv
        pad = (k - u) // 2
        z = ops.upsample_zero(x, u, (L - 1) * u + 1, slope=slope)
        return ops.conv1d_packed(z, c.packed(ops.PACK_DGRAD), c.bias.detach(), Co, k, 1, k - 1 - pad, alpha=alpha,
                                 Lout=(L - 1) * u - 2 * pad + k)

    @staticmethod
    def pair(c1, c2, r, k, d, pad1, pad2, slope, acc, last):
        C = r.shape[1]     # t leaves the first epilogue already activated: this walk has no taps to give
        t = ops.conv1d_packed(r, c1.packed(ops.PACK_PLAIN), c1.bias.detach(), C, k, 1, pad1, act="lrelu_s",
                              act_slope=slope, dilation=d, in_slope=slope)
        # the last pair of a block writes (conv + bias + r) straight into the stage sum
        r = ops.conv1d_packed(t, c2.packed(ops.PACK_PLAIN), c2.bias.detach(), C, k, 1, pad2, add=r,
                              out=acc if last else None, accumulate=last and acc is not None)
        return r, t, (r if last else acc)


class _Train:
    """Generator._walk's sites in training: autograd Functions on the effective weights and the pre-activations."""

    @staticmethod
    def conv(c, x, Co, k, pad, in_slope=1.0, alpha=1.0, act=None):
        return ag.voc_conv(x, c.effective_weight(), c.bias, 1, pad, in_slope, alpha, act)

    @staticmethod
    def up(c, x, Co, k, u, slope, alpha):
        return ag.voc_up(x, c.effective_weight(), c.bias, u, slope, alpha)

    @staticmethod
    def pair(c1, c2, r, k, d, pad1, pad2, slope, acc, last):
        r, t = ag.voc_pair(r, c1.effective_weight(), c1.bias, c2.effective_weight(), c2.bias, d, pad1, pad2, slope)
        if last:
            acc = r if acc is None else acc + r
        return r, t, acc


class Generator(nn.Module):
    """hifigan/models.py:112-173."""

    def __init__(self, h):
        super().__init__()
        self.h = h
        self.num_kernels = len(h.resblock_kernel_sizes)
        self.num_upsamples = len(h.upsample_rates)
        c0 = h.upsample_initial_channel
        self.conv_pre = _WNConv((c0, 80, 7), c0)
        self.ups = nn.ModuleList([
            _WNConv((c0 // (2 ** i), c0 // (2 ** (i + 1)), k), c0 // (2 ** (i + 1)), 0.01)
            for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes))])
        self.resblocks = nn.ModuleList()
        for i in range(len(self.ups)):
            ch = c0 // (2 ** (i + 1))
            for k, d in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
                self.resblocks.append(ResBlock(h, ch, k, d))
        self.conv_post = _WNConv((1, ch, 7), 1, 0.01)

    def remove_weight_norm(self):
        for l in self.ups:
            l.remove_weight_norm()
        for l in self.resblocks:
            l.remove_weight_norm()
        self.conv_pre.remove_weight_norm()
        self.conv_post.remove_weight_norm()

    def _walk(self, x, site, taps=None):
        """conv_pre; per stage an upsampler and num_kernels ResBlocks of dilation pairs, summed; conv_post.  `site`
        (_Infer or _Train) runs each convolution, upsampler and pair; `taps`: see forward_train."""
        h, nk, c0 = self.h, self.num_kernels, self.h.upsample_initial_channel
        x = site.conv(self.conv_pre, x.contiguous(), c0, 7, 3)
        scale = 1.0
        for i, (u, uk) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
            if taps is not None:
                taps["ups.%d" % i] = x
            x = site.up(self.ups[i], x, c0 // (2 ** (i + 1)), uk, u, LRELU_SLOPE, scale)
            acc = None
            for jj in range(i * nk, (i + 1) * nk):
                rb = self.resblocks[jj]
                k, r = rb.kernel_size, x
                for m, d in enumerate(rb.dilation):
                    rin = r
                    r, t, acc = site.pair(rb.convs1[m], rb.convs2[m], rin, k, d, (k * d - d) // 2, (k - 1) // 2,
                                          LRELU_SLOPE, acc, m == len(rb.dilation) - 1)
                    if taps is not None:
                        taps["resblocks.%d.convs1.%d" % (jj, m)] = rin
                        taps["resblocks.%d.convs2.%d" % (jj, m)] = t
            x = acc                       # = num_kernels * (xs / num_kernels); the division rides on the next conv
            scale = 1.0 / self.num_kernels
        if taps is not None:
            taps["conv_post"] = x
        # F.leaky_relu(x) with the DEFAULT slope 0.01 (hifigan/models.py:161), conv_post, tanh
        return site.conv(self.conv_post, x, 1, 7, 3, in_slope=0.01, alpha=scale, act="tanh")

    @torch.no_grad()
    def forward(self, x):
        """x: mel [B, 80, L] -> [B, 1, L * prod(upsample_rates)]."""
        if not x.is_cuda:
            raise _lib.MixganHipError("hifigan.Generator on %s: the HIP path has no CPU fallback" % x.device)
        return self._walk(x, _Infer)

    def forward_train(self, x, taps=None):
        """x: mel [B, 80, L] -> [B, 1, L * prod(upsample_rates)] as an autograd tensor: gradients reach every
        parameter (weight_g / weight_v through the torch expression effective_weight(), the effective weight's own
        gradient from the HIP backward) and x when it requires grad.  Same function as forward(); each leaky ReLU's
        pre-activation is what the backward keeps.  taps (dict, optional) receives those tensors: "ups.i" the input of
        upsampler i, "resblocks.j.convs1.m" / "resblocks.j.convs2.m" the inputs of the two convolutions of a pair,
        "conv_post" the input of the last convolution (stage sums are kept undivided: the 1/num_kernels rides on the
        next convolution and does not move a sign)."""
        if not x.is_cuda:
            raise _lib.MixganHipError("hifigan.Generator on %s: the HIP path has no CPU fallback" % x.device)
        for u, k in zip(self.h.upsample_rates, self.h.upsample_kernel_sizes):
            if not _polyphase(k, u):
                raise _lib.MixganHipError("forward_train: upsampler (kernel %d, stride %d) has no HIP backward; only "
                                          "kernel = 2 * stride with stride in {2, 4, 8}" % (k, u))
        return self._walk(x, _Train, taps)


class AttrDict(dict):
    """hifigan/__init__.py / env.py: json config with attribute access."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.__dict__ = self


class MelGANCheckpointRequired(_lib.MixganHipError, NotImplementedError):
    """get_vocoder for MelGAN without `checkpoint_path`: the reference fetches the weights with torch.hub, which is a
    download and is not mirrored here."""


MELGAN_HUB_FILES = {"LJSpeech": "linda_johnson.pt", "universal": "multi_speaker.pt"}


def get_vocoder(config, device, config_path="hifigan/config.json", checkpoint_path=None):
    """utils/model.py:74-105.  "HiFi-GAN": build from hifigan/config.json, load the `generator` state dict of
    hifigan/generator_<speaker>.pth.tar, eval, remove_weight_norm, move to the device.  "MelGAN": build
    melgan.MelVocoder and load `checkpoint_path` -- the generator state dict of descriptinc/melgan-neurips
    models/<name>.pt (linda_johnson.pt for LJSpeech, multi_speaker.pt for universal) -- into `.mel2wav`, eval,
    move to the device; weight norm stays, as in the hub.  Nothing is fetched: without `checkpoint_path` MelGAN
    raises MelGANCheckpointRequired."""
    import json
    name = config["vocoder"]["model"]
    speaker = config["vocoder"]["speaker"]
    if name == "MelGAN":
        hub_file = MELGAN_HUB_FILES.get(speaker, "multi_speaker.pt")
        if checkpoint_path is None:
            raise MelGANCheckpointRequired(
                "vocoder MelGAN (speaker %r): pass checkpoint_path= the melgan-neurips state dict models/%s; the "
                "reference's torch.hub download is not mirrored" % (speaker, hub_file))
        from .melgan import MelVocoder
        vocoder = MelVocoder()
        sd = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
        vocoder.mel2wav.load_state_dict(sd)
        vocoder.mel2wav.eval()
        vocoder.mel2wav.to(device)
        return vocoder
    if name != "HiFi-GAN":
        raise NotImplementedError("vocoder %r: only HiFi-GAN and MelGAN are on the HIP path" % name)
    with open(config_path, "r") as f:
        h = AttrDict(json.load(f))
    vocoder = Generator(h)
    if checkpoint_path is None:
        checkpoint_path = "hifigan/generator_%s.pth.tar" % speaker
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    vocoder.load_state_dict(ckpt["generator"])
    vocoder.eval()
    vocoder.remove_weight_norm()
    vocoder.to(device)
    return vocoder


def vocoder_infer(mels, vocoder, model_config, preprocess_config, lengths=None):
    """utils/model.py:108-126: mels [B, 80, L] -> list of int16 numpy waveforms (cropped to `lengths`).  The scaling
    and the int16 conversion run on the device, so the host copy is half the bytes of the reference's."""
    name = model_config["vocoder"]["model"]
    if name not in ("HiFi-GAN", "MelGAN"):
        raise NotImplementedError("only HiFi-GAN and MelGAN are on the HIP path")
    with torch.no_grad():
        if name == "MelGAN":   # vocoder.inverse(mels / np.log(10)), the 1/ln 10 on the first conv's alpha
            wavs = vocoder.mel2wav.forward_scaled(mels, 1.0 / math.log(10.0)).squeeze(1)
        else:
            wavs = vocoder(mels).squeeze(1)
        scaled = wavs * float(preprocess_config["preprocessing"]["audio"]["max_wav_value"])
        wavs = scaled.to(torch.int32).to(torch.int16).cpu().numpy()     # truncation toward zero, as numpy's astype
    wavs = [w for w in wavs]
    for i in range(len(mels)):
        if lengths is not None:
            wavs[i] = wavs[i][: lengths[i]]
    return wavs
