"""Plain-torch restatement, from the paper's definitions (Kong et al. 2020: DiscriminatorS, MultiScaleDiscriminator), of
what the multi-scale discriminator tests compare against.  Runs in the dtype of its inputs; float64 on the CPU is the
reference.  Weight norm and spectral norm are written out by hand over a dict of tensors with the torch construction's
keys; TorchMSD builds the same network from torch.nn.Conv1d + torch.nn.utils.weight_norm / spectral_norm + AvgPool1d,
and tests/test_msd_cpu.py pins the restatement to it.

Spectral norm (scale 0): torch's legacy hook.  With train=True every sub-forward (one on y, one on y_hat) does one power
iteration per layer under no_grad, v <- normalize(W^T u), u <- normalize(W v), eps 1e-12, written IN PLACE into the
dict's weight_u / weight_v; sigma = u . (W v) with u, v constants; W / sigma.  clone_buffers() gives a dict whose buffers
are copies, for a run that must not advance them.

taps / masks as in hifigan_disc_ref.py: tap "discriminators.{i}.convs.{j}" is the pre-activation of the batch [y; y_hat]
(scale 0 runs the halves one after the other and joins them), masks impose a sign pattern.
"""
import torch
import torch.nn.functional as F
from torch import nn

from hifigan_disc_ref import lrelu, wn, kink_masks, taps_of_fmaps  # noqa: F401  (re-exported for the tests)
from hifigan_disc_ref import discriminator_loss, generator_loss, feature_loss, d_phase_loss, g_phase_loss  # noqa: F401

SLOPE = 0.1
# (Ci, Co, K, stride, groups, padding)
LAYERS = ((1, 128, 15, 1, 1, 7), (128, 128, 41, 2, 4, 20), (128, 256, 41, 2, 16, 20), (256, 512, 41, 4, 16, 20),
          (512, 1024, 41, 4, 16, 20), (1024, 1024, 41, 1, 16, 20), (1024, 1024, 5, 1, 1, 2))
POST = (1024, 1, 3, 1, 1, 1)
SCALES = 3
EPS = 1e-12


def layer_names(i):
    return ["discriminators.%d.convs.%d" % (i, j) for j in range(len(LAYERS))] + ["discriminators.%d.conv_post" % i]


def msd_keys():
    """(name, shape, is_buffer) in the torch construction's state-dict order."""
    out = []
    for i in range(SCALES):
        for name, (ci, co, k, _, g, _) in zip(layer_names(i), LAYERS + (POST,)):
            w = (co, ci // g, k)
            if i == 0:
                out += [(name + ".bias", (co,), False), (name + ".weight_orig", w, False),
                        (name + ".weight_u", (co,), True), (name + ".weight_v", (w[1] * w[2],), True)]
            else:
                out += [(name + ".bias", (co,), False), (name + ".weight_g", (co, 1, 1), False),
                        (name + ".weight_v", w, False)]
    return out


def msd_init(seed):
    """Seeded weights under msd_keys' names: weights ~ N(0, 1 / fan_in), gains 1 .. 1.5 times the identity's, small
    biases, unit-norm u and v."""
    gen = torch.Generator().manual_seed(seed)
    W = {}
    for name, shape, is_buffer in msd_keys():
        if name.endswith("bias"):
            W[name] = 0.1 * torch.randn(shape, generator=gen)
        elif name.endswith("weight_g"):
            W[name] = 1.0 + 0.5 * torch.rand(shape, generator=gen)      # times |v| below
        elif is_buffer:
            W[name] = F.normalize(torch.randn(shape, generator=gen), dim=0, eps=EPS)
        else:
            W[name] = torch.randn(shape, generator=gen) / (shape[1] * shape[2]) ** 0.5
    for name in [n for n in W if n.endswith("weight_g")]:
        W[name] = W[name] * W[name[:-1] + "v"].flatten(1).norm(dim=1).view(-1, 1, 1)
    return W


def buffer_names():
    return [n for n, _, b in msd_keys() if b]


def clone_buffers(W):
    """W with weight_u / weight_v copied (parameters shared)."""
    bufs = set(buffer_names())
    return {k: (v.clone() if k in bufs else v) for k, v in W.items()}


def sn(W, name, train):
    """spectral_norm's weight; with train one power iteration first, in place on W[name.weight_u / weight_v]."""
    w = W[name + ".weight_orig"]
    mat = w.flatten(1)
    u, v = W[name + ".weight_u"], W[name + ".weight_v"]
    if train:
        with torch.no_grad():
            v.copy_(F.normalize(torch.mv(mat.t(), u), dim=0, eps=EPS))
            u.copy_(F.normalize(torch.mv(mat, v), dim=0, eps=EPS))
    u, v = u.clone(), v.clone()
    return w / torch.dot(u, torch.mv(mat, v))


def disc_s_forward(W, i, x, train=True, taps=None, masks=None):
    """x [N, 1, T] -> (logits [N, T'], the seven activated maps and conv_post's raw one)."""
    weight = (lambda n: sn(W, n, train)) if i == 0 else (lambda n: wn(W, n))
    names = layer_names(i)
    fmap = []
    for name, (_, _, _, s, g, pad) in zip(names, LAYERS):
        x = F.conv1d(x, weight(name), W[name + ".bias"], stride=s, padding=pad, groups=g)
        x = lrelu(x, SLOPE, name, taps, masks)
        fmap.append(x)
    x = F.conv1d(x, weight(names[-1]), W[names[-1] + ".bias"], padding=POST[5])
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def msd_forward(W, y, y_hat, taps=None, masks=None, train=True):
    """The published forward: per scale (pooled cumulatively from the second on) one sub-forward on y, one on y_hat."""
    B = y.shape[0]
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
    for i in range(SCALES):
        if i:
            y, y_hat = F.avg_pool1d(y, 4, 2, padding=2), F.avg_pool1d(y_hat, 4, 2, padding=2)
        halves = []
        for h, x in enumerate((y, y_hat)):
            t = None if taps is None else {}
            m = None if masks is None else {k: v[h * B:(h + 1) * B] for k, v in masks.items() if
                                            k.startswith("discriminators.%d." % i)}
            halves.append(disc_s_forward(W, i, x, train, t, m) + (t,))
        if taps is not None:
            for k in halves[0][2]:
                taps[k] = torch.cat([halves[0][2][k], halves[1][2][k]], 0)
        y_d_rs.append(halves[0][0])
        y_d_gs.append(halves[1][0])
        fmap_rs.append(halves[0][1])
        fmap_gs.append(halves[1][1])
    return y_d_rs, y_d_gs, fmap_rs, fmap_gs


# ------------------------------------------------------------------------------------------------------------------
# the same network from torch's own modules and parameterisations
# ------------------------------------------------------------------------------------------------------------------
class TorchDiscriminatorS(nn.Module):
    def __init__(self, use_spectral_norm=False):
        super().__init__()
        norm = nn.utils.spectral_norm if use_spectral_norm else nn.utils.weight_norm
        self.convs = nn.ModuleList([norm(nn.Conv1d(ci, co, k, s, groups=g, padding=p)) for ci, co, k, s, g, p in LAYERS])
        self.conv_post = norm(nn.Conv1d(POST[0], POST[1], POST[2], 1, padding=POST[5]))

    def forward(self, x):
        fmap = []
        for conv in self.convs:
            x = F.leaky_relu(conv(x), SLOPE)
            fmap.append(x)
        x = self.conv_post(x)
        fmap.append(x)
        return torch.flatten(x, 1, -1), fmap


class TorchMSD(nn.Module):
    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList([TorchDiscriminatorS(True), TorchDiscriminatorS(), TorchDiscriminatorS()])
        self.meanpools = nn.ModuleList([nn.AvgPool1d(4, 2, padding=2), nn.AvgPool1d(4, 2, padding=2)])

    def forward(self, y, y_hat):
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for i, d in enumerate(self.discriminators):
            if i != 0:
                y, y_hat = self.meanpools[i - 1](y), self.meanpools[i - 1](y_hat)
            y_d_r, fmap_r = d(y)
            y_d_g, fmap_g = d(y_hat)
            y_d_rs.append(y_d_r)
            fmap_rs.append(fmap_r)
            y_d_gs.append(y_d_g)
            fmap_gs.append(fmap_g)
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs
