"""Plain-torch restatement, from the math, of what the MelGAN training tests differentiate: the generator of
mel2wav/modules.py (Generator(80, ngf=32, n_residual_layers=3)) as a function of its state dict, with its leaky-ReLU
inputs exposed (`taps`) and their sign patterns imposed (`masks`), as tests/hifigan_train_ref.py does for HiFi-GAN.
Runs in the dtype of its inputs; float64 on the CPU is the tests' reference.

Tap names are the module paths MelGANGenerator.forward_train uses: "model.<i>" for the leaky ReLU in front of every
upsampler and of the last conv, "model.<i>.block.0" and "model.<i>.block.3" inside a ResnetBlock.  The product's
"block.3" tap is that leaky ReLU's OUTPUT (what its backward keeps), which has its input's signs; here it is the input.
"""
import torch
import torch.nn.functional as F

from hifigan_train_ref import wn, lrelu

RATIOS = (8, 8, 2, 2)
SLOPE = 0.2


def reflect_conv(x, w, b, dil=1):
    p = dil * (w.shape[2] - 1) // 2
    return F.conv1d(F.pad(x, (p, p), mode="reflect"), w, b, dilation=dil)


def resblock(W, p, x, dil, taps=None, masks=None):
    """ResnetBlock(dim, dil) under the key prefix p ("model.4."): shortcut(x) + block(x)."""
    t = lrelu(x, SLOPE, p + "block.0", taps, masks)
    t = reflect_conv(t, wn(W, p + "block.2"), W[p + "block.2.bias"], dil)
    t = lrelu(t, SLOPE, p + "block.3", taps, masks)
    return F.conv1d(t, wn(W, p + "block.4"), W[p + "block.4.bias"]) + F.conv1d(x, wn(W, p + "shortcut"),
                                                                                  W[p + "shortcut.bias"])


def generator_forward(W, mel, taps=None, masks=None, scale=1.0, nres=3):
    """mel [B, 80, L] -> wav [B, 1, 256 L] of Generator.forward(mel * scale)."""
    x = reflect_conv(mel * scale, wn(W, "model.1"), W["model.1.bias"])
    i = 2
    for r in RATIOS:
        x = lrelu(x, SLOPE, "model.%d" % i, taps, masks)
        x = F.conv_transpose1d(x, wn(W, "model.%d" % (i + 1)), W["model.%d.bias" % (i + 1)], stride=r, padding=r // 2)
        for j in range(nres):
            x = resblock(W, "model.%d." % (i + 2 + j), x, 3 ** j, taps, masks)
        i += 2 + nres
    x = lrelu(x, SLOPE, "model.%d" % i, taps, masks)
    return torch.tanh(reflect_conv(x, wn(W, "model.%d" % (i + 2)), W["model.%d.bias" % (i + 2)]))


def generator_grads(W, mel, cot, dtype, masks=None, scale=1.0):
    """out, taps and every gradient of sum(out * cot) in `dtype`.  Keys: "out", "taps", "d_mel", "param/<key>"."""
    Wd = {k: v.detach().to(dtype, copy=True).requires_grad_() for k, v in W.items()}
    x = mel.detach().to(dtype, copy=True).requires_grad_()
    taps = {}
    out = generator_forward(Wd, x, taps=taps, masks=masks, scale=scale)
    (out * cot.to(dtype)).sum().backward()
    res = {"out": out.detach(), "taps": {k: v.detach() for k, v in taps.items()}, "d_mel": x.grad}
    for k, v in Wd.items():
        res["param/" + k] = v.grad
    return res
