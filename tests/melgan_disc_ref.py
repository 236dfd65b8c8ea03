"""Plain-torch restatement, from the paper's definitions (Kumar et al. 2019: NLayerDiscriminator, Discriminator and the
hinge objective of scripts/train.py), of what the MelGAN discriminator tests compare against.  Runs in the dtype of its
inputs; float64 on the CPU is the reference.  Weight norm, the reflection pad and the pool that does not count its
padding are written out by hand over a dict of tensors with the torch construction's keys; TorchDiscriminator builds the
same network from torch.nn modules, and tests/test_melgan_disc_cpu.py pins the restatement to it.

taps / masks as in hifigan_disc_ref.py: tap "disc_{i}.layer_{j}" is the pre-activation of the batch the scale ran on,
masks impose a sign pattern on the leaky ReLUs.
"""
import torch
import torch.nn.functional as F
from torch import nn

from hifigan_disc_ref import lrelu, wn, kink_masks  # noqa: F401  (re-exported for the tests)

SLOPE = 0.2


def geometry(ndf=16, n_layers=4, factor=4):
    """[(Ci, Co, K, stride, groups, padding)] of layer_0 .. layer_{n_layers + 2}; layer_0 follows ReflectionPad1d(7)."""
    out = [(1, ndf, 15, 1, 1, 0)]
    nf = ndf
    for _ in range(n_layers):
        nf_prev, nf = nf, min(nf * factor, 1024)
        out.append((nf_prev, nf, factor * 10 + 1, factor, nf_prev // 4, factor * 5))
    nf2 = min(nf * 2, 1024)
    return out + [(nf, nf2, 5, 1, 1, 2), (nf2, 1, 3, 1, 1, 1)]


def conv_names(i, n_layers=4):
    """State-dict prefixes of scale i's convolutions: layer_0.1, layer_j.0, and the bare last layer."""
    n = n_layers + 3
    return ["model.disc_%d.model.layer_%d%s" % (i, j, ".1" if j == 0 else (".0" if j < n - 1 else "")) for j in range(n)]


def disc_keys(num_D=3, n_layers=4):
    """(name, shape) in the torch construction's state-dict order."""
    out = []
    for i in range(num_D):
        for name, (ci, co, k, _, g, _) in zip(conv_names(i, n_layers), geometry(n_layers=n_layers)):
            out += [(name + ".bias", (co,)), (name + ".weight_g", (co, 1, 1)), (name + ".weight_v", (co, ci // g, k))]
    return out


def disc_init(seed, num_D=3, n_layers=4):
    """Seeded weights: v ~ N(0, 1 / fan_in), gains 1 .. 1.5 times the identity's, small biases."""
    gen = torch.Generator().manual_seed(seed)
    W = {}
    for name, shape in disc_keys(num_D, n_layers):
        if name.endswith("bias"):
            W[name] = 0.1 * torch.randn(shape, generator=gen)
        elif name.endswith("weight_g"):
            W[name] = 1.0 + 0.5 * torch.rand(shape, generator=gen)
        else:
            W[name] = torch.randn(shape, generator=gen) / (shape[1] * shape[2]) ** 0.5
    for name in [n for n in W if n.endswith("weight_g")]:
        W[name] = W[name] * W[name[:-1] + "v"].flatten(1).norm(dim=1).view(-1, 1, 1)
    return W


def reflect_pad(x, p):
    return torch.cat([x[..., 1:p + 1].flip(-1), x, x[..., -p - 1:-1].flip(-1)], -1)


def pool(x):
    """AvgPool1d(4, 2, padding 1) dividing every window by its number of in-range samples."""
    s = F.pad(x, (1, 1)).unfold(-1, 4, 2).sum(-1)
    n = F.pad(torch.ones_like(x[:1, :1]), (1, 1)).unfold(-1, 4, 2).sum(-1)
    return s / n


def nlayer_forward(W, i, x, n_layers=4, taps=None, masks=None):
    """x [N, 1, T] -> the n_layers + 2 activated maps and the raw logit map."""
    names, geo = conv_names(i, n_layers), geometry(n_layers=n_layers)
    maps = []
    x = reflect_pad(x, 7)
    for j, (name, (_, _, _, s, g, pad)) in enumerate(zip(names, geo)):
        x = F.conv1d(x, wn(W, name), W[name + ".bias"], stride=s, padding=pad, groups=g)
        if j < len(names) - 1:
            x = lrelu(x, SLOPE, "disc_%d.layer_%d" % (i, j), taps, masks)
        maps.append(x)
    return maps


def disc_forward(W, x, num_D=3, n_layers=4, taps=None, masks=None):
    out = []
    for i in range(num_D):
        out.append(nlayer_forward(W, i, x, n_layers, taps, masks))
        if i < num_D - 1:
            x = pool(x)
    return out


def disc_forward_pair(W, y, y_hat, num_D=3, n_layers=4, taps=None, masks=None):
    B = y.shape[0]
    both = disc_forward(W, torch.cat([y, y_hat], 0), num_D, n_layers, taps, masks)
    return [[m[:B] for m in maps] for maps in both], [[m[B:] for m in maps] for maps in both]


def taps_of_maps(D_real, D_fake):
    """The activated maps a product run returned, as taps (their signs are the pre-activations': slope > 0)."""
    return {"disc_%d.layer_%d" % (i, j): torch.cat([r[j], f[j]], 0).detach()
            for i, (r, f) in enumerate(zip(D_real, D_fake)) for j in range(len(r) - 1)}


def discriminator_loss(D_real, D_fake):
    return sum(F.relu(1 - r[-1]).mean() + F.relu(1 + f[-1]).mean() for r, f in zip(D_real, D_fake))


def generator_loss(D_fake):
    return sum(-f[-1].mean() for f in D_fake)


def feature_loss(D_real, D_fake):
    num_D, n_layers = len(D_fake), len(D_fake[0]) - 3
    wt = (1.0 / num_D) * 4.0 / (n_layers + 1)
    return sum(wt * (f[j] - r[j].detach()).abs().mean() for r, f in zip(D_real, D_fake) for j in range(len(f) - 1))


# ------------------------------------------------------------------------------------------------------------------
# the same network from torch's own modules
# ------------------------------------------------------------------------------------------------------------------
class TorchNLayerDiscriminator(nn.Module):
    def __init__(self, ndf=16, n_layers=4, downsampling_factor=4):
        super().__init__()
        geo = geometry(ndf, n_layers, downsampling_factor)
        model = nn.ModuleDict()
        for j, (ci, co, k, s, g, p) in enumerate(geo):
            conv = nn.utils.weight_norm(nn.Conv1d(ci, co, k, stride=s, padding=p, groups=g))
            if j == 0:
                model["layer_0"] = nn.Sequential(nn.ReflectionPad1d(7), conv, nn.LeakyReLU(SLOPE, True))
            elif j < len(geo) - 1:
                model["layer_%d" % j] = nn.Sequential(conv, nn.LeakyReLU(SLOPE, True))
            else:
                model["layer_%d" % j] = conv
        self.model = model

    def forward(self, x):
        results = []
        for _, layer in self.model.items():
            x = layer(x)
            results.append(x)
        return results


class TorchDiscriminator(nn.Module):
    def __init__(self, num_D=3, ndf=16, n_layers=4, downsampling_factor=4):
        super().__init__()
        self.model = nn.ModuleDict()
        for i in range(num_D):
            self.model["disc_%d" % i] = TorchNLayerDiscriminator(ndf, n_layers, downsampling_factor)
        self.downsample = nn.AvgPool1d(4, stride=2, padding=1, count_include_pad=False)

    def forward(self, x):
        results = []
        for _, disc in self.model.items():
            results.append(disc(x))
            x = self.downsample(x)
        return results
