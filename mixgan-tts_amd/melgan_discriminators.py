"""MelGAN's multi-scale discriminator (Kumar et al. 2019, mel2wav/modules.py) on the HIP kernels of csrc/msd.hip and
csrc/gconv_c4.h.

NLayerDiscriminator / Discriminator keep the published constructor arguments, attribute names (model, downsample) and
the state-dict keys of the torch construction, Conv1d under torch.nn.utils.weight_norm:
`model.disc_0.model.layer_0.1.{bias, weight_g, weight_v}`, `...layer_1.0.{...}`, ..., `...layer_6.{...}` -- the
ReflectionPad1d and LeakyReLU entries of the Sequentials are kept as parameterless placeholders so that the indices
agree; forward never calls them.  forward(x) returns one list of n_layers + 3 maps per scale, the last the raw logits.

Upstream applies `weights_init` after construction, which draws N(0, 0.02) into the `weight` ATTRIBUTE of every conv.
Under weight_norm that attribute is not a parameter: the hook recomputes it from weight_g and weight_v before every
forward.  Checked with torch on the CPU (tests/test_melgan_disc_cpu.py): weight_g, weight_v and bias keep their bits and
the next forward's output is unchanged, so upstream's networks start from Conv1d's default initialisation, and so does
this one.

Supported: ndf = 16 and downsampling_factor = 4 (groups of four input channels, stride 4, K = 41: the two grouped
forms of gconv_c4.h), n_layers >= 4, num_D >= 1.  Anything else raises ValueError at construction.
"""
import torch
from torch import nn

from . import autograd as A
from ._lib import MixganHipError
from .hifigan_discriminators import NormConv1d, scale_walk

LRELU_SLOPE = 0.2
_PAD0 = 7


def nlayer_geometry(ndf=16, n_layers=4, downsampling_factor=4):
    """[(Ci, Co, K, stride, groups, padding)] of layer_0 .. layer_{n_layers + 2}."""
    layers = [(1, ndf, 15, 1, 1, 0)]      # after ReflectionPad1d(7)
    nf, stride = ndf, downsampling_factor
    for _ in range(n_layers):
        nf_prev, nf = nf, min(nf * stride, 1024)
        layers.append((nf_prev, nf, stride * 10 + 1, stride, nf_prev // 4, stride * 5))
    nf2 = min(nf * 2, 1024)
    layers.append((nf, nf2, 5, 1, 1, 2))
    layers.append((nf2, 1, 3, 1, 1, 1))
    return layers


class NLayerDiscriminator(nn.Module):
    def __init__(self, ndf=16, n_layers=4, downsampling_factor=4):
        super().__init__()
        if ndf != 16 or downsampling_factor != 4 or int(n_layers) != n_layers or n_layers < 4:
            raise ValueError("NLayerDiscriminator: the HIP kernels cover ndf = 16, downsampling_factor = 4, n_layers >= 4 "
                             "(got ndf %r, n_layers %r, downsampling_factor %r)" % (ndf, n_layers, downsampling_factor))
        self.n_layers = int(n_layers)
        self.geometry = nlayer_geometry(ndf, self.n_layers, downsampling_factor)
        model = nn.ModuleDict()
        for j, g in enumerate(self.geometry):
            conv = NormConv1d(*g, spectral=False)
            if j == 0:
                model["layer_0"] = nn.Sequential(nn.ReflectionPad1d(_PAD0), conv, nn.LeakyReLU(LRELU_SLOPE, True))
            elif j < len(self.geometry) - 1:
                model["layer_%d" % j] = nn.Sequential(conv, nn.LeakyReLU(LRELU_SLOPE, True))
            else:
                model["layer_%d" % j] = conv
        self.model = model

    def convs(self):
        """The n_layers + 3 weight-normed convolutions in order."""
        n = len(self.geometry)
        return [self.model["layer_%d" % j][1 if j == 0 else 0] if j < n - 1 else self.model["layer_%d" % j]
                for j in range(n)]

    def forward(self, x):
        """x [N, 1, T], T > 7 -> [n_layers + 2 activated maps, the raw logit map]."""
        if not x.is_cuda:
            raise MixganHipError("NLayerDiscriminator: tensors must be on the GPU (no CPU fallback)")
        # layer_0 and the grouped layers: one node
        return scale_walk(self.convs(), A.reflect_pad1d(x, _PAD0), LRELU_SLOPE, self.n_layers + 1)


class Downsample(nn.Module):
    """AvgPool1d(4, stride=2, padding=1, count_include_pad=False)."""
    kernel_size, stride, padding, count_include_pad = 4, 2, 1, False

    def forward(self, x):
        return A.avgpool4s2(x, self.padding, self.count_include_pad)


class Discriminator(nn.Module):
    def __init__(self, num_D=3, ndf=16, n_layers=4, downsampling_factor=4):
        super().__init__()
        if int(num_D) != num_D or num_D < 1:
            raise ValueError("Discriminator: num_D >= 1, got %r" % (num_D,))
        self.model = nn.ModuleDict()
        for i in range(int(num_D)):
            self.model["disc_%d" % i] = NLayerDiscriminator(ndf, n_layers, downsampling_factor)
        self.downsample = Downsample()

    def forward(self, x):
        """x [N, 1, T] -> one list of maps per scale; x is pooled between scales."""
        if not x.is_cuda:
            raise MixganHipError("Discriminator: tensors must be on the GPU (no CPU fallback)")
        results = []
        last = len(self.model) - 1
        for i, disc in enumerate(self.model.values()):
            results.append(disc(x))
            if i < last:
                x = self.downsample(x)
        return results

    def forward_pair(self, y, y_hat):
        """Every scale once on the batch [y; y_hat] (weight norm: one weight for both halves) ->
        (D_real, D_fake), each as forward's result on its half."""
        if y.shape != y_hat.shape:
            raise ValueError("forward_pair: %s vs %s" % (tuple(y.shape), tuple(y_hat.shape)))
        B = y.shape[0]
        both = self.forward(torch.cat([y, y_hat], 0))
        return [[m[:B] for m in maps] for maps in both], [[m[B:] for m in maps] for maps in both]
