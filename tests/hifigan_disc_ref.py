"""Plain-torch restatement, from the paper's definitions (Kong et al. 2020: DiscriminatorP, MultiPeriodDiscriminator,
discriminator_loss, generator_loss, feature_loss and the D / G phases of the training step), of what the vocoder GAN
tests compare against.  Runs in the dtype of its inputs; float64 on the CPU is the reference.

Leaky-ReLU inputs are exposed (`taps`: name -> pre-activation) and their sign patterns can be imposed (`masks`), as in
hifigan_train_ref.py.  Tap names: "discriminators.{i}.convs.{j}" for the multi-period discriminator and
"scales.{i}.convs.{j}" for the small multi-scale one; both halves of the batch [y; y_hat] share a tap.  A run on the
GPU hands back only POST-activation maps; with slope 0.1 > 0 their signs are the pre-activations'.

mpd_init / TorchMPD: the multi-period discriminator with upstream's keys and shapes (MPD_CHANNELS) or narrower layers.
small_msd_* / SmallMSD: a reduced multi-scale discriminator (two scales, grouped Conv1d stacks, an average pool
between them, no spectral norm).  Both are torch modules with the forward(y, y_hat) convention, which is all
vocoder_train.VocoderGANTrainer asks of a discriminator.
"""
import torch
import torch.nn.functional as F
from torch import nn


PERIODS = (2, 3, 5, 7, 11)
MPD_CHANNELS = (1, 32, 128, 512, 1024, 1024)


def lrelu(x, slope, name, taps, masks):
    """leaky_relu(x, slope); records x in taps[name]; with masks[name] (bool, True = positive side) the side of every
    element is the mask's, not sign(x)'s -- the same function wherever the two agree."""
    if taps is not None:
        taps[name] = x
    pos = (x > 0) if masks is None else masks[name].to(x.device)
    return torch.where(pos, x, x * slope)


def wn(W, name):
    """weight_norm over all dims but the first."""
    v, g = W[name + ".weight_v"], W[name + ".weight_g"]
    return v * (g / v.flatten(1).norm(dim=1).view(-1, *([1] * (v.dim() - 1))))


def mpd_keys(periods=PERIODS, channels=MPD_CHANNELS):
    """name -> shape of MultiPeriodDiscriminator's state dict."""
    out = {}
    for i in range(len(periods)):
        for j in range(5):
            p = "discriminators.%d.convs.%d." % (i, j)
            ci, co = channels[j], channels[j + 1]
            out[p + "weight_g"], out[p + "weight_v"], out[p + "bias"] = (co, 1, 1, 1), (co, ci, 5, 1), (co,)
        p = "discriminators.%d.conv_post." % i
        out[p + "weight_g"], out[p + "weight_v"], out[p + "bias"] = (1, 1, 1, 1), (1, channels[5], 3, 1), (1,)
    return out


def mpd_init(seed, periods=PERIODS, channels=MPD_CHANNELS):
    """Seeded weights under mpd_keys' names: v ~ N(0, 1 / fan_in), gains 1 .. 1.5 times the identity's, small biases."""
    gen = torch.Generator().manual_seed(seed)
    W = {}
    for k, shape in mpd_keys(periods, channels).items():
        if k.endswith("weight_v"):
            W[k] = torch.randn(shape, generator=gen) / (shape[1] * shape[2]) ** 0.5
            W[k[:-1] + "g"] = W[k].flatten(1).norm(dim=1).view(-1, 1, 1, 1) * (1.0 + 0.5 * torch.rand(shape[0], 1, 1, 1,
                                                                                                 generator=gen))
        elif k.endswith("bias"):
            W[k] = 0.1 * torch.randn(shape, generator=gen)
    return W


def disc_p_forward(W, prefix, x, period, taps=None, masks=None):
    """x [N, 1, T] -> (logits [N, H' p], six maps [N, C, H', p])."""
    N, C, T = x.shape
    if T % period:
        x = F.pad(x, (0, period - T % period), "reflect")
    x = x.view(N, C, x.shape[2] // period, period)
    fmap = []
    for j in range(5):
        name = prefix + "convs.%d" % j
        x = F.conv2d(x, wn(W, name), W[name + ".bias"], stride=(3 if j < 4 else 1, 1), padding=(2, 0))
        x = lrelu(x, 0.1, name, taps, masks)
        fmap.append(x)
    x = F.conv2d(x, wn(W, prefix + "conv_post"), W[prefix + "conv_post.bias"], padding=(1, 0))
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def _halves(forward_one, n_discs, y, y_hat):
    B = y.shape[0]
    x = torch.cat([y, y_hat], 0)
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
    for i in range(n_discs):
        out, fmap = forward_one(i, x)
        y_d_rs.append(out[:B])
        y_d_gs.append(out[B:])
        fmap_rs.append([f[:B] for f in fmap])
        fmap_gs.append([f[B:] for f in fmap])
    return y_d_rs, y_d_gs, fmap_rs, fmap_gs


def mpd_forward(W, y, y_hat, taps=None, masks=None, periods=PERIODS):
    return _halves(lambda i, x: disc_p_forward(W, "discriminators.%d." % i, x, periods[i], taps, masks), len(periods), y,
                   y_hat)


def discriminator_loss(disc_real, disc_gen):
    loss, r_losses, g_losses = 0, [], []
    for dr, dg in zip(disc_real, disc_gen):
        r, g = torch.mean((1 - dr) ** 2), torch.mean(dg ** 2)
        loss = loss + (r + g)
        r_losses.append(r.detach())
        g_losses.append(g.detach())
    return loss, r_losses, g_losses


def generator_loss(disc_gen):
    loss, gen_losses = 0, []
    for dg in disc_gen:
        g = torch.mean((1 - dg) ** 2)
        gen_losses.append(g.detach())
        loss = loss + g
    return loss, gen_losses


def feature_loss(fmap_r, fmap_g):
    loss = 0
    for dr, dg in zip(fmap_r, fmap_g):
        for r, g in zip(dr, dg):
            loss = loss + torch.mean(torch.abs(r - g))
    return loss * 2


# ------------------------------------------------------------------------------------------------------------------
# a small multi-scale discriminator
# ------------------------------------------------------------------------------------------------------------------
MSD_LAYERS = [(1, 16, 15, 1, 1, 7), (16, 32, 41, 4, 4, 20), (32, 32, 5, 1, 1, 2)]   # (Ci, Co, K, stride, groups, pad)
MSD_SCALES = 2


def small_msd_init(seed):
    gen = torch.Generator().manual_seed(seed)
    W = {}
    for i in range(MSD_SCALES):
        for j, (ci, co, k, _, g, _) in enumerate(MSD_LAYERS + [(32, 1, 3, 1, 1, 1)]):
            name = "scales.%d.%s" % (i, "convs.%d" % j if j < len(MSD_LAYERS) else "conv_post")
            v = torch.randn(co, ci // g, k, generator=gen) / (ci // g * k) ** 0.5
            W[name + ".weight_v"] = v
            W[name + ".weight_g"] = v.flatten(1).norm(dim=1).view(-1, 1, 1) * (1 + 0.1 * torch.rand(co, 1, 1, generator=gen))
            W[name + ".bias"] = 0.1 * torch.randn(co, generator=gen)
    return W


def small_msd_forward(W, y, y_hat, taps=None, masks=None):
    def one(i, x):
        for _ in range(i):
            x = F.avg_pool1d(x, 4, 2, padding=2)
        fmap = []
        for j, (_, _, _, s, g, pad) in enumerate(MSD_LAYERS):
            name = "scales.%d.convs.%d" % (i, j)
            x = F.conv1d(x, wn(W, name), W[name + ".bias"], stride=s, padding=pad, groups=g)
            x = lrelu(x, 0.1, name, taps, masks)
            fmap.append(x)
        name = "scales.%d.conv_post" % i
        x = F.conv1d(x, wn(W, name), W[name + ".bias"], padding=1)
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap
    return _halves(one, MSD_SCALES, y, y_hat)


class _DictModule(nn.Module):
    """A functional restatement as a module: parameter names are the dict's with dots replaced by "__"."""

    def __init__(self, W):
        super().__init__()
        self.weights = nn.ParameterDict({k.replace(".", "__"): nn.Parameter(v.clone()) for k, v in W.items()})

    def dict(self):
        return {k.replace("__", "."): v for k, v in self.weights.items()}


class SmallMSD(_DictModule):
    def forward(self, y, y_hat):
        return small_msd_forward(self.dict(), y, y_hat)


class TorchMPD(_DictModule):
    def __init__(self, W, periods=PERIODS):
        super().__init__(W)
        self.periods = tuple(periods)

    def forward(self, y, y_hat):
        return mpd_forward(self.dict(), y, y_hat, periods=self.periods)


# ------------------------------------------------------------------------------------------------------------------
# leaky-ReLU kinks and the two phases of the step
# ------------------------------------------------------------------------------------------------------------------
def kink_masks(product_taps, own64_taps):
    """name -> (product tensor > 0), after asserting what makes adopting the product's signs sound: every element
    whose product sign differs from the float64 run's own has |pre64| <= 1e-4 max|pre64| of its tensor, and such
    elements are at most 1e-3 of the tensor."""
    masks = {}
    assert set(product_taps) == set(own64_taps), sorted(set(product_taps) ^ set(own64_taps))
    for k, p in product_taps.items():
        pos = (p.detach() > 0).cpu()
        pre = own64_taps[k].detach()
        assert pos.shape == pre.shape, (k, pos.shape, pre.shape)
        flip = pos != (pre > 0)
        n = int(flip.sum())
        if n:
            worst = float(pre[flip].abs().max() / pre.abs().max())
            assert worst <= 1e-4, "%s: a flipped sign at |pre64| / max = %.2e" % (k, worst)
            assert n <= 1e-3 * pre.numel(), "%s: %d of %d signs flipped" % (k, n, pre.numel())
        masks[k] = pos
    return masks


def taps_of_fmaps(prefix, fmap_rs, fmap_gs):
    """The maps a discriminator returned, as taps: "<prefix>.{i}.convs.{j}" -> [real; generated] (conv_post's map, the
    last of each list, passes through no activation and is left out)."""
    out = {}
    for i, (fr, fg) in enumerate(zip(fmap_rs, fmap_gs)):
        for j in range(len(fr) - 1):
            out["%s.%d.convs.%d" % (prefix, i, j)] = torch.cat([fr[j], fg[j]], 0).detach()
    return out


def d_phase_loss(discs, y, y_hat, taps=None, masks=None):
    """discs: name -> (forward(W, y, y_hat, taps, masks), W).  The discriminator phase's loss on a detached y_hat.
    taps / masks: name -> dict."""
    total = 0
    for name, (fwd, W) in discs.items():
        y_d_rs, y_d_gs, _, _ = fwd(W, y, y_hat.detach(), None if taps is None else taps.setdefault(name, {}),
                                   None if masks is None else masks[name])
        total = total + discriminator_loss(y_d_rs, y_d_gs)[0]
    return total


def g_phase_loss(discs, y, y_hat, taps=None, masks=None):
    """(adversarial, feature matching) of the generator phase."""
    adv = fm = 0
    for name, (fwd, W) in discs.items():
        _, y_d_gs, fmap_rs, fmap_gs = fwd(W, y, y_hat, None if taps is None else taps.setdefault(name, {}),
                                          None if masks is None else masks[name])
        adv = adv + generator_loss(y_d_gs)[0]
        fm = fm + feature_loss(fmap_rs, fmap_gs)
    return adv, fm
