"""Plain-torch restatement of the MelGAN generator spec (descriptinc/melgan-neurips mel2wav/modules.py,
Generator(input_size=80, ngf=32, n_residual_layers=3)): nn.Conv1d / nn.ConvTranspose1d under
torch.nn.utils.weight_norm, nn.ReflectionPad1d.  The reference for the native MelGAN's parity tests; the hub code and
checkpoints are a download and are not used."""
import warnings

import torch
from torch import nn

with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    from torch.nn.utils import weight_norm as _weight_norm


def WNConv1d(*args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _weight_norm(nn.Conv1d(*args, **kwargs))


def WNConvTranspose1d(*args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _weight_norm(nn.ConvTranspose1d(*args, **kwargs))


class ResnetBlock(nn.Module):
    def __init__(self, dim, dilation=1):
        super().__init__()
        self.block = nn.Sequential(
            nn.LeakyReLU(0.2),
            nn.ReflectionPad1d(dilation),
            WNConv1d(dim, dim, kernel_size=3, dilation=dilation),
            nn.LeakyReLU(0.2),
            WNConv1d(dim, dim, kernel_size=1),
        )
        self.shortcut = WNConv1d(dim, dim, kernel_size=1)

    def forward(self, x):
        return self.shortcut(x) + self.block(x)


class Generator(nn.Module):
    def __init__(self, input_size=80, ngf=32, n_residual_layers=3, ratios=(8, 8, 2, 2)):
        super().__init__()
        self.hop_length = 1
        for r in ratios:
            self.hop_length *= r
        mult = 2 ** len(ratios)
        model = [nn.ReflectionPad1d(3), WNConv1d(input_size, mult * ngf, kernel_size=7, padding=0)]
        for r in ratios:
            model += [nn.LeakyReLU(0.2),
                      WNConvTranspose1d(mult * ngf, mult * ngf // 2, kernel_size=r * 2, stride=r,
                                        padding=r // 2 + r % 2, output_padding=r % 2)]
            model += [ResnetBlock(mult * ngf // 2, dilation=3 ** j) for j in range(n_residual_layers)]
            mult //= 2
        model += [nn.LeakyReLU(0.2), nn.ReflectionPad1d(3), WNConv1d(ngf, 1, kernel_size=7, padding=0), nn.Tanh()]
        self.model = nn.Sequential(*model)

    def forward(self, x):
        return self.model(x)


def seeded_generator(seed=0, L=16):
    """A restatement generator with seeded weights (weight_v ~ N(0, 1), weight_g ~ U(0.5, 1), biases ~ U(-0.05, 0.05))
    whose gains are then calibrated stage by stage on a seeded mel of L frames so that every stage's output has unit
    standard deviation and the tanh input about 0.7: the parity tests then look at unsaturated audio."""
    g = torch.Generator().manual_seed(seed)
    G = Generator()
    with torch.no_grad():
        for name, p in G.named_parameters():
            if name.endswith("weight_v"):
                p.copy_(torch.randn(p.shape, generator=g))
            elif name.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=g) * 0.1 - 0.05)
            elif name.endswith("weight_g"):
                p.copy_(torch.rand(p.shape, generator=g) * 0.5 + 0.5)
        h = torch.randn(2, 80, L, generator=g) - 4.0
        for m in G.model:
            if isinstance(m, ResnetBlock):
                scaled = [m.shortcut.weight_g, m.block[4].weight_g]
            elif isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
                scaled = [m.weight_g]
            else:
                h = m(h)
                continue
            target = 0.7 if m is G.model[24] else 1.0
            f = target / float(m(h).std())
            for p in scaled:
                p.mul_(f)
            h = m(h)
    return G.eval()
