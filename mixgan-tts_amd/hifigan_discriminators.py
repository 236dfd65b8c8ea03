"""HiFi-GAN's discriminators (Kong et al. 2020): the multi-scale one on the HIP kernels of csrc/msd.hip, the multi-period
one (DiscriminatorP / MultiPeriodDiscriminator, at the end of this file) on csrc/mpd.hip -- state-dict keys of
weight_norm(Conv2d): `bias, weight_g [Co,1,1,1], weight_v [Co,Ci,K,1]`.

DiscriminatorS / MultiScaleDiscriminator keep the published constructor arguments, attribute names (convs, conv_post,
discriminators, meanpools), forward(y, y_hat) -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) and the state-dict keys of the torch
construction (Conv1d under torch.nn.utils.weight_norm / spectral_norm): `bias, weight_g, weight_v` per weight-norm
layer, `bias, weight_orig` plus the buffers `weight_u, weight_v` per spectral-norm layer.

The effective weight is a torch expression, as vocoder.Generator.effective_weight(): HIP differentiates with respect to
it and torch carries the gradient to weight_g / weight_v / weight_orig.  Spectral norm is torch's legacy hook: in
training mode one power iteration per sub-forward under no_grad, updating u and v in place, sigma = u . (W v) with u, v
constants of the graph; no iteration in eval mode.
"""
import torch
import torch.nn.functional as F
from torch import nn

from . import autograd as A
from . import ops
from ._lib import MixganHipError

LRELU_SLOPE = 0.1
# (Ci, Co, K, stride, groups, padding) of DiscriminatorS.convs; conv_post is (1024, 1, 3, 1, 1, 1)
MSD_LAYERS = ((1, 128, 15, 1, 1, 7), (128, 128, 41, 2, 4, 20), (128, 256, 41, 2, 16, 20), (256, 512, 41, 4, 16, 20),
              (512, 1024, 41, 4, 16, 20), (1024, 1024, 41, 1, 16, 20), (1024, 1024, 5, 1, 1, 2))
MSD_POST = (1024, 1, 3, 1, 1, 1)
_STACK = 6      # convs[:6] run as one node of msd.hip kernels; convs[6] and conv_post go through the MFMA conv kernel


class NormConv1d(nn.Module):
    """The parameters of one Conv1d under weight_norm (bias, weight_g, weight_v) or spectral_norm (bias, weight_orig;
    buffers weight_u, weight_v), initialised as torch initialises them, and the effective weight as a torch expression."""

    def __init__(self, ci, co, k, stride, groups, padding, spectral):
        super().__init__()
        self.geometry = (ci, co, k, stride, groups, padding)
        self.spectral, self.eps = bool(spectral), 1e-12
        ref = nn.Conv1d(ci, co, k, stride, padding=padding, groups=groups)
        w = ref.weight.detach()
        self.bias = nn.Parameter(ref.bias.detach().clone())
        if spectral:
            self.weight_orig = nn.Parameter(w.clone())
            self.register_buffer("weight_u", F.normalize(torch.randn(co), dim=0, eps=self.eps))
            self.register_buffer("weight_v", F.normalize(torch.randn(w[0].numel()), dim=0, eps=self.eps))
        else:
            self.weight_g = nn.Parameter(w.flatten(1).norm(dim=1).view(-1, 1, 1))
            self.weight_v = nn.Parameter(w.clone())

    def effective_weight(self):
        """weight_norm: g v / |v| per output row.  spectral_norm: W / sigma after this call's power iteration."""
        if not self.spectral:
            return A.weight_norm(self.weight_v, self.weight_g)
        W = self.weight_orig
        mat = W.flatten(1)
        u, v = self.weight_u, self.weight_v
        if self.training:
            with torch.no_grad():
                F.normalize(torch.mv(mat.t(), u), dim=0, eps=self.eps, out=v)
                F.normalize(torch.mv(mat, v), dim=0, eps=self.eps, out=u)
                u, v = u.clone(), v.clone()
        return W / torch.dot(u, torch.mv(mat, v))


def scale_walk(convs, x, slope, stack):
    """One discriminator scale over its NormConv1d list, effective weights taken in layer order: convs[:stack] (the
    one-channel first layer and the grouped layers) as one node of msd.hip kernels, then the dense K = 5 layer and the
    logit layer through the MFMA conv kernel.  x [N, 1, T] -> [len(convs) - 1 activated maps, the raw logit map]."""
    params = []
    for conv in convs[:stack]:
        params += [conv.effective_weight(), conv.bias]
    maps = list(A.scale_stack(x, slope, [conv.geometry[3:] for conv in convs[:stack]], *params))
    dense, post = convs[stack:]
    maps.append(A.conv1d(maps[-1], dense.effective_weight(), dense.bias, 1, dense.geometry[5], "lrelu_s",
                         act_slope=slope))
    maps.append(A.conv1d(maps[-1], post.effective_weight(), post.bias, 1, post.geometry[5]))
    return maps


class DiscriminatorS(nn.Module):
    def __init__(self, use_spectral_norm=False):
        super().__init__()
        self.convs = nn.ModuleList([NormConv1d(*g, spectral=use_spectral_norm) for g in MSD_LAYERS])
        self.conv_post = NormConv1d(*MSD_POST, spectral=use_spectral_norm)

    def forward(self, x):
        """x [N, 1, T] -> (logits [N, T'], [seven activated maps, conv_post's raw map])."""
        if not x.is_cuda:
            raise MixganHipError("DiscriminatorS: tensors must be on the GPU (no CPU fallback)")
        fmap = scale_walk([*self.convs, self.conv_post], x, LRELU_SLOPE, _STACK)
        return torch.flatten(fmap[-1], 1, -1), fmap


class MeanPool(nn.Module):
    """AvgPool1d(4, 2, padding=2)."""
    kernel_size, stride, padding, count_include_pad = 4, 2, 2, True

    def forward(self, x):
        return A.avgpool4s2(x, self.padding, self.count_include_pad)


class MultiScaleDiscriminator(nn.Module):
    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorS(use_spectral_norm=True), DiscriminatorS(), DiscriminatorS()])
        self.meanpools = nn.ModuleList([MeanPool(), MeanPool()])

    def forward(self, y, y_hat):
        """The published forward runs every scale on y, then on y_hat.  Scale 0 does exactly that, so that its spectral
        norm iterates twice and the halves see different weights; scales 1 and 2 (weight norm: one weight for both)
        and the pools run once on the batch [y; y_hat]."""
        B = y.shape[0]
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        both = None
        for i, d in enumerate(self.discriminators):
            if i == 0:
                (r, fr), (g, fg) = d(y), d(y_hat)
            else:
                both = self.meanpools[i - 1](torch.cat([y, y_hat], 0) if both is None else both)
                out, fmap = d(both)
                r, g = out[:B], out[B:]
                fr, fg = [f[:B] for f in fmap], [f[B:] for f in fmap]
            y_d_rs.append(r)
            y_d_gs.append(g)
            fmap_rs.append(fr)
            fmap_gs.append(fg)
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs


# ------------------------------------------------------------------------------------------------------------------
# the multi-period discriminator (csrc/mpd.hip)
# ------------------------------------------------------------------------------------------------------------------
MPD_PERIODS = (2, 3, 5, 7, 11)
MPD_CHANNELS = (1, 32, 128, 512, 1024, 1024)      # DiscriminatorP.convs: K = 5, stride 3 (the last one stride 1)


class UnsupportedPeriodConfig(MixganHipError, NotImplementedError):
    """A DiscriminatorP constructor argument the HIP path has no kernels for: both MixganHipError (no fallback) and
    NotImplementedError (the published multi-period discriminator never uses it)."""


class NormConv2d(nn.Module):
    """The parameters of one Conv2d(ci, co, (k, 1)) under weight_norm -- bias, weight_g [Co,1,1,1], weight_v [Co,Ci,k,1] --
    initialised as torch initialises them, and the effective [Co, Ci, k] weight as a torch expression."""

    def __init__(self, ci, co, k, stride, padding):
        super().__init__()
        self.geometry = (ci, co, k, stride, padding)
        ref = nn.Conv2d(ci, co, (k, 1), (stride, 1), padding=(padding, 0))
        w = ref.weight.detach()
        self.bias = nn.Parameter(ref.bias.detach().clone())
        self.weight_g = nn.Parameter(w.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
        self.weight_v = nn.Parameter(w.clone())

    def effective_weight(self):
        return A.weight_norm(self.weight_v.squeeze(3), self.weight_g.squeeze(3))


class DiscriminatorP(nn.Module):
    """One period of the multi-period discriminator.  The input is folded onto a slotted flat axis (one slot per
    (n, w) row of the published [N, C, H, period] map) on which every layer is a plain 1-D convolution; the returned maps
    are strided views of those buffers with the published shapes and values."""

    def __init__(self, period, kernel_size=5, stride=3, use_spectral_norm=False):
        super().__init__()
        if kernel_size != 5 or stride != 3 or use_spectral_norm:
            raise UnsupportedPeriodConfig("DiscriminatorP: the HIP path has kernel_size 5, stride 3 under weight norm (the "
                                         "published multi-period discriminator), got kernel_size %r, stride %r, "
                                         "use_spectral_norm %r" % (kernel_size, stride, use_spectral_norm))
        if int(period) != period or period < 1:
            raise ValueError("DiscriminatorP: period must be a positive integer, got %r" % (period,))
        self.period = int(period)
        ch = MPD_CHANNELS
        self.convs = nn.ModuleList([NormConv2d(ch[j], ch[j + 1], 5, 3 if j < 4 else 1, 2) for j in range(5)])
        self.conv_post = NormConv2d(ch[5], 1, 3, 1, 1)

    def forward(self, x):
        """x [N, 1, T] -> (logits [N, H6 period], [five activated maps, conv_post's raw map], each [N, C, H, period])."""
        if not x.is_cuda:
            raise MixganHipError("DiscriminatorP: tensors must be on the GPU (no CPU fallback)")
        if x.dim() != 3 or x.shape[1] != 1 or x.dtype != torch.float32:
            raise MixganHipError("DiscriminatorP: expected a float32 waveform [N, 1, T], got %s %s"
                                 % (x.dtype, tuple(x.shape)))
        N, _, T = x.shape
        p = self.period
        H, S = ops.period_geometry(T, p)
        params = []
        for conv in [*self.convs, self.conv_post]:
            params += [conv.effective_weight(), conv.bias]
        bufs = A.period_stack(x, p, LRELU_SLOPE, *params)
        fmap = [b.view(b.shape[1], N, p, S[j + 1]).permute(1, 0, 3, 2)[:, :, :H[j + 1]] for j, b in enumerate(bufs)]
        return torch.flatten(fmap[-1], 1, -1), fmap


class MultiPeriodDiscriminator(nn.Module):
    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorP(p) for p in MPD_PERIODS])

    def forward(self, y, y_hat):
        """Every period runs once on the batch [y; y_hat]: weight norm gives one weight for both halves."""
        if not y.is_cuda or not y_hat.is_cuda:
            raise MixganHipError("MultiPeriodDiscriminator: tensors must be on the GPU (no CPU fallback)")
        B = y.shape[0]
        both = torch.cat([y, y_hat], 0)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for d in self.discriminators:
            out, fmap = d(both)
            y_d_rs.append(out[:B])
            y_d_gs.append(out[B:])
            fmap_rs.append([f[:B] for f in fmap])
            fmap_gs.append([f[B:] for f in fmap])
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs
