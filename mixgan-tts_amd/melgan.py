"""MelGAN generator (descriptinc/melgan-neurips mel2wav/modules.py, `Generator(input_size=80, ngf=32,
n_residual_layers=3)`) on HIP -- the reference's second vocoder (`vocoder.model: "MelGAN"`, utils/model.py:80-90,
111-112), which it fetches with torch.hub.  Same module tree (`model.<index>.`, ResnetBlock `block.2`, `block.4`,
`shortcut`; weight norm kept: `bias`, `weight_g`, `weight_v`), so a hub checkpoint (`models/<name>.pt`) loads
strictly.

Kernel mapping (csrc/melgan.hip): the first and last conv are reflect-padded implicit GEMMs (ReflectionPad1d(3) in
the staging; tanh and the last leaky ReLU fused); every upsampler is the polyphase transposed conv of the HiFi-GAN
path with its leaky ReLU in the staging.  A ResnetBlock in the general form is two launches: the dilated k=3 conv
(reflect padding, both leaky ReLUs fused) writes t next to x in a [B, 2C, L] buffer, and one K=1 GEMM over [x ; t]
with the packs of shortcut and block.4 concatenated gives shortcut(x) + block(x).  With `fused_stack` (default), the
three blocks of the 64- and 32-channel stages run as one launch each, holding a tile and its 13-sample halo in LDS.

Training (csrc/melgan_train.hip, autograd.voc_conv with pad = REFLECT / melgan_resblock / voc_up): `forward_train` is
the same `_walk` with the `_Train` sites, every stage in the general form, the backward in the HIP library: the reflect-padded
weight gradient mirrors the frame index while it stages the saved pre-activation, the data gradient is the zero-padded
correlation over the padded length folded back through the reflection, and a ResnetBlock's K = 1 gradients run once
over [x ; t].  vocoder_train's trainers take a MelVocoder as they take a HiFi-GAN generator.
"""
import ctypes
import math

import torch
from torch import nn

from . import ops, _lib, autograd as ag
from ._lib import fptr, check, stream_ptr
from .vocoder import _WNConv

SLOPE = 0.2
RATIOS = (8, 8, 2, 2)


class _MelWNConv(_WNConv):
    """weight_norm(Conv1d / ConvTranspose1d) with torch.nn.utils.weight_norm's parameter order: bias, weight_g,
    weight_v.  `shape` is the weight's ([Co, Ci, K], or [Ci, Co, K] for the transposed conv); `bias_n` its bias."""

    def __init__(self, shape, bias_n):
        nn.Module.__init__(self)
        v = torch.empty(*shape)
        nn.init.kaiming_uniform_(v, a=5 ** 0.5)
        fan_in = shape[1] * shape[2]
        bound = 1.0 / math.sqrt(fan_in)
        self.bias = nn.Parameter(torch.empty(bias_n).uniform_(-bound, bound))
        self.weight_g = nn.Parameter(v.flatten(1).norm(dim=1).view(-1, 1, 1).clone())
        self.weight_v = nn.Parameter(v)


class ResnetBlock(nn.Module):
    """mel2wav/modules.py ResnetBlock(dim, dilation): shortcut(x) + block(x)."""

    def __init__(self, dim, dilation=1):
        super().__init__()
        self.dim, self.dilation = dim, dilation
        self.block = nn.Sequential(
            nn.LeakyReLU(SLOPE),
            nn.ReflectionPad1d(dilation),
            _MelWNConv((dim, dim, 3), dim),
            nn.LeakyReLU(SLOPE),
            _MelWNConv((dim, dim, 1), dim),
        )
        self.shortcut = _MelWNConv((dim, dim, 1), dim)

    def mix_pack(self, permuted):
        """[Ws | W2] packed along the reduction (K = 1, Ci = 2C) and bs + b2, cached until a parameter changes.
        permuted: W2's columns in the fused stack's accumulator order (mg_melgan_stack_fwd)."""
        ws, w2 = self.shortcut, self.block[4]
        key = (permuted,) + tuple((p.data_ptr(), p._version) for p in list(ws.parameters()) + list(w2.parameters()))
        cache = self.__dict__.setdefault("_mg_mix", {})
        hit = cache.get(permuted)
        if hit is None or hit[0] != key:
            C = self.dim
            with torch.no_grad():
                a = ws.effective_weight().contiguous()
                b = w2.effective_weight()
                if permuted:
                    j = torch.arange(C)
                    g, e, h = j // 8, (j % 8) // 2, j % 2
                    b = b[:, (8 * g + 4 * h + e).to(b.device)]
                b = b.contiguous()
                L = _lib.lib()
                n = L.mg_conv_packed_floats(C, 2 * C, 1, ops.PACK_PLAIN)
                if n == 0 or C % 32:
                    raise _lib.MixganHipError("MelGAN ResnetBlock: %d channels are not taken (multiple of 32)" % C)
                packed = torch.zeros(n, device=a.device, dtype=torch.float32)
                Q = C // 8
                check(L.mg_conv_pack_at(fptr(a), fptr(packed), C, C, 1, ops.PACK_PLAIN, 0, 2 * Q, stream_ptr()))
                check(L.mg_conv_pack_at(fptr(b), fptr(packed), C, C, 1, ops.PACK_PLAIN, Q, 2 * Q, stream_ptr()))
                bias = (ws.bias.detach() + w2.bias.detach()).contiguous()
            hit = cache[permuted] = (key, packed, bias)
        return hit[1], hit[2]

    def forward_general(self, buf, out, out_bs):
        """buf [B, 2C, L] with x in channels [0, C): t -> channels [C, 2C); the block output -> out (batch stride out_bs)."""
        c1 = self.block[2]
        ag.melgan_block_fwd(buf, c1.packed(ops.PACK_PLAIN), c1.bias.detach(), lambda: self.mix_pack(False), self.dim,
                            self.dilation, SLOPE, out, out_bs)


def residual_stack_fused(x, blocks):
    """The three ResnetBlocks (dilations 1, 3, 9) of a 32- or 64-channel stage in one launch: x [B, C, L] -> [B, C, L]."""
    B, C, L = x.shape
    w1, b1, wm, bm = [], [], [], []
    for blk in blocks:
        conv1 = blk.block[2]
        p, bias = blk.mix_pack(True)
        w1.append(conv1.packed(ops.PACK_PLAIN))
        b1.append(conv1.bias.detach())
        wm.append(p)
        bm.append(bias)
    arr = lambda ts: (ctypes.c_void_p * 3)(*[fptr(t).value for t in ts])
    out = torch.empty_like(x)
    check(_lib.lib().mg_melgan_stack_fwd(fptr(x), fptr(out), arr(w1), arr(b1), arr(wm), arr(bm), B, C, L, stream_ptr()))
    return out


class _Infer:
    """MelGANGenerator._walk's sites at inference."""

    @staticmethod
    def conv(c, x, Co, K, in_slope=1.0, alpha=1.0, act=None):
        return ops.conv1d_reflect_packed(x, c.packed(ops.PACK_PLAIN), c.bias.detach(), Co, K, in_slope=in_slope, act=act,
                                         alpha=alpha)

    @staticmethod
    def stage(up, blocks, x, C, r, fused):
        nres = len(blocks)
        if nres == 0 or (fused and nres == 3 and C in (32, 64)):
            y = ops.conv_transpose1d_packed(x, up.packed(ops.PACK_TPOSE), up.bias.detach(), C, r, in_slope=SLOPE)
            return (residual_stack_fused(y, blocks) if nres else y), ()
        # general form: [B, 2C, L] buffers, x in [0, C), t in [C, 2C); the upsampler writes the first x, block j the next
        B, Cin, Lin = x.shape
        L = Lin * r
        bufs = [torch.empty(B, 2 * C, L, device=x.device, dtype=torch.float32) for _ in range(min(nres, 2))]
        check(_lib.lib().mg_conv_transpose1d_fwd_slice(fptr(x), fptr(up.packed(ops.PACK_TPOSE)), fptr(up.bias.detach()),
                                                       fptr(bufs[0]), 2 * C * L, B, Cin, Lin, C, r, float(SLOPE), 1.0,
                                                       stream_ptr()))
        for j, blk in enumerate(blocks):
            last = j + 1 == nres
            out = torch.empty(B, C, L, device=x.device, dtype=torch.float32) if last else bufs[(j + 1) % 2]
            blk.forward_general(bufs[j % 2], out, 0 if last else 2 * C * L)
        return out, ()


class _Train:
    """MelGANGenerator._walk's sites in training; a stage also returns (block input, t) per block for the taps."""

    @staticmethod
    def conv(c, x, Co, K, in_slope=1.0, alpha=1.0, act=None):
        return ag.voc_conv(x, c.effective_weight(), c.bias, 1, ag.REFLECT, in_slope, alpha, act)

    @staticmethod
    def stage(up, blocks, x, C, r, fused):      # fused: inference only
        x = ag.voc_up(x, up.effective_weight(), up.bias, r, SLOPE, 1.0)
        signs = []
        for blk in blocks:
            c1, c2, cs = blk.block[2], blk.block[4], blk.shortcut
            y, xt = ag.melgan_resblock(x, c1.effective_weight(), c1.bias, c2.effective_weight(), c2.bias,
                                       cs.effective_weight(), cs.bias, blk.dilation, SLOPE)
            signs.append((x, xt[:, blk.dim:]))
            x = y
        return x, signs


class MelGANGenerator(nn.Module):
    """mel2wav/modules.py Generator(input_size, ngf, n_residual_layers): mel [B, input_size, L] -> [B, 1, 256 L]."""

    def __init__(self, input_size=80, ngf=32, n_residual_layers=3):
        super().__init__()
        self.input_size, self.ngf, self.n_residual_layers = input_size, ngf, n_residual_layers
        self.hop_length = 1
        for r in RATIOS:
            self.hop_length *= r
        mult = 2 ** len(RATIOS)
        model = [nn.ReflectionPad1d(3), _MelWNConv((mult * ngf, input_size, 7), mult * ngf)]
        for r in RATIOS:
            cin, cout = mult * ngf, mult * ngf // 2
            model += [nn.LeakyReLU(SLOPE), _MelWNConv((cin, cout, 2 * r), cout)]
            model += [ResnetBlock(cout, dilation=3 ** j) for j in range(n_residual_layers)]
            mult //= 2
        model += [nn.LeakyReLU(SLOPE), nn.ReflectionPad1d(3), _MelWNConv((1, ngf, 7), 1), nn.Tanh()]
        self.model = nn.Sequential(*model)
        self.fused_stack = True

    def forward(self, mel):
        return self.forward_scaled(mel, 1.0)

    def _check_input(self, mel):
        """(B, Ci, L) of a mel both forwards can take."""
        if not mel.is_cuda:
            raise _lib.MixganHipError("MelGANGenerator on %s: the HIP path has no CPU fallback" % mel.device)
        B, Ci, L = mel.shape
        if Ci != self.input_size:
            raise ValueError("MelGANGenerator: expected %d mel channels, got %d" % (self.input_size, Ci))
        if L < 4:
            raise ValueError("MelGANGenerator: %d frames; ReflectionPad1d(3) needs at least 4" % L)
        if self.n_residual_layers > 3:
            raise _lib.MixganHipError("MelGANGenerator: dilations above 9 are not taken by the HIP conv")
        return B, Ci, L

    def _walk(self, mel, site, scale, taps=None):
        """First reflect conv (alpha = scale); per ratio one stage, an upsampler and its blocks at half the channels; last
        reflect conv, tanh.  `site` (_Infer or _Train) runs each convolution and stage; `taps`: see forward_train."""
        m, nres = self.model, self.n_residual_layers
        tap = (lambda path, t: None) if taps is None else taps.__setitem__
        C = 2 ** len(RATIOS) * self.ngf
        x = site.conv(m[1], mel, C, 7, alpha=scale)
        for i, r in enumerate(RATIOS):
            base = 2 + i * (2 + nres)
            C //= 2
            tap("model.%d" % base, x)
            x, signs = site.stage(m[base + 1], [m[base + 2 + j] for j in range(nres)], x, C, r, self.fused_stack)
            for j, (xin, t) in enumerate(signs):
                tap("model.%d.block.0" % (base + 2 + j), xin)
                tap("model.%d.block.3" % (base + 2 + j), t)
        last = len(m) - 2
        tap("model.%d" % (last - 2), x)
        return site.conv(m[last], x, 1, 7, in_slope=SLOPE, act="tanh")

    @torch.no_grad()
    def forward_scaled(self, mel, scale):
        """forward(mel * scale), the scale riding on the first conv's alpha (no pass over the mel)."""
        self._check_input(mel)
        return self._walk(mel.float().contiguous(), _Infer, scale)

    def forward_train(self, mel, taps=None, scale=1.0):
        """forward_scaled(mel, scale) as an autograd tensor: gradients reach every weight_g / weight_v (through the
        torch expression effective_weight(); the effective weight's own gradient comes from the HIP backward), every
        bias, and mel when it requires grad.  Every stage runs the general form.  taps (dict, optional) receives, under
        its module path, what fixes each leaky ReLU's side: the input of "model.<i>" (the four in front of the
        upsamplers and the one in front of the last conv) and of "model.<i>.block.0", and for "model.<i>.block.3" its
        OUTPUT t, which the backward keeps instead of the input: same sign, same zeros, the negative side scaled by
        the slope."""
        self._check_input(mel)
        if self.ngf % 32:
            raise _lib.MixganHipError("MelGANGenerator.forward_train: ngf = %d; the general form takes channel counts "
                                      "that are multiples of 32" % self.ngf)
        return self._walk(mel.float(), _Train, float(scale), taps)


class MelVocoder(nn.Module):
    """The parts of the hub's MelVocoder (mel2wav/interface.py) the reference uses: `.mel2wav` and `.inverse`."""

    def __init__(self, input_size=80, ngf=32, n_residual_layers=3):
        super().__init__()
        self.mel2wav = MelGANGenerator(input_size, ngf, n_residual_layers)

    def inverse(self, mel):
        """mel [B, 80, L] -> audio [B, 256 L]."""
        with torch.no_grad():
            return self.mel2wav(mel).squeeze(1)

    def forward(self, mel):
        return self.inverse(mel)

    def forward_train(self, mel, taps=None):
        """mel [B, 80, L] (natural log, as audio.TacotronSTFT gives it) -> [B, 1, 256 L] as an autograd tensor, the
        1 / ln 10 of vocoder_infer on the first conv: what GeneratorTrainer / VocoderGANTrainer train, so that the
        trained generator is used at inference as it was trained."""
        return self.mel2wav.forward_train(mel, taps, 1.0 / math.log(10.0))
