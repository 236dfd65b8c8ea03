"""Plain-torch restatement, from the math, of what the vocoder-training tests differentiate: the HiFi-GAN V1 generator
(hifigan/models.py:112-173) with its leaky-ReLU inputs exposed (`taps`) and their sign patterns imposed (`masks`), and
the log-mel of audio/stft.py.  Runs in the dtype of its inputs; float64 on the CPU is the tests' reference.

Tap names are those of vocoder.Generator.forward_train: "ups.i", "resblocks.j.convs1.m", "resblocks.j.convs2.m",
"conv_post".  The product keeps stage sums undivided (the 1/num_kernels rides on the next convolution); here the tap is
the divided tensor, which has the same signs and the same |x| / max|x|.
"""
import torch
import torch.nn.functional as F

HIFIGAN_V1 = {"upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4],
              "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}


def wn(W, name):
    """weight_norm over all dims but the first, or the plain weight after remove_weight_norm."""
    if name + ".weight" in W:
        return W[name + ".weight"]
    v, g = W[name + ".weight_v"], W[name + ".weight_g"]
    return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))


def lrelu(x, slope, name, taps, masks):
    """leaky_relu(x, slope); records x in taps[name]; with masks[name] (bool, True = positive side) the side of every
    element is the mask's, not sign(x)'s -- the same function wherever the two agree."""
    if taps is not None:
        taps[name] = x
    pos = (x > 0) if masks is None else masks[name].to(x.device)
    return x * torch.where(pos, torch.ones((), dtype=x.dtype), torch.full((), slope, dtype=x.dtype))


def generator_forward(W, mel, taps=None, masks=None, h=HIFIGAN_V1):
    """mel [B, 80, L] -> wav [B, 1, 256 L]."""
    nk = len(h["resblock_kernel_sizes"])
    x = F.conv1d(mel, wn(W, "conv_pre"), W["conv_pre.bias"], padding=3)
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = lrelu(x, 0.1, "ups.%d" % i, taps, masks)
        x = F.conv_transpose1d(x, wn(W, "ups.%d" % i), W["ups.%d.bias" % i], stride=u, padding=(k - u) // 2)
        xs = None
        for j, (ks, dils) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            p = "resblocks.%d." % (i * nk + j)
            r = x
            for m, d in enumerate(dils):
                t = lrelu(r, 0.1, p + "convs1.%d" % m, taps, masks)
                t = F.conv1d(t, wn(W, p + "convs1.%d" % m), W[p + "convs1.%d.bias" % m], dilation=d,
                             padding=(ks * d - d) // 2)
                t = lrelu(t, 0.1, p + "convs2.%d" % m, taps, masks)
                t = F.conv1d(t, wn(W, p + "convs2.%d" % m), W[p + "convs2.%d.bias" % m], padding=(ks - 1) // 2)
                r = t + r
            xs = r if xs is None else xs + r
        x = xs / nk
    x = lrelu(x, 0.01, "conv_post", taps, masks)
    x = F.conv1d(x, wn(W, "conv_post"), W["conv_post.bias"], padding=3)
    return torch.tanh(x)


def masks_of(taps):
    """The sign pattern of a run: name -> (tensor > 0) on the CPU."""
    return {k: (v.detach() > 0).cpu() for k, v in taps.items()}


def log_mel(y, window, basis, hop=256, n_fft=1024):
    """y [B, N] -> log(clamp(basis |STFT(y)|, 1e-5)) [B, n_mels, 1 + N // hop]: reflect padding of n_fft / 2, frames of
    n_fft at every hop, times `window` [n_fft], one-sided DFT, magnitude, `basis` [n_mels, n_fft / 2 + 1]."""
    p = F.pad(y[:, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
    frames = p.unfold(1, n_fft, hop) * window.to(y.dtype)                 # [B, T, n_fft]
    spec = torch.fft.rfft(frames, dim=2)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2)                     # [B, T, bins]
    mel = torch.matmul(mag, basis.to(y.dtype).t()).transpose(1, 2)
    return torch.log(torch.clamp(mel, min=1e-5))


def generator_grads(W, mel, cot, dtype, masks=None):
    """out, taps and every gradient of sum(out * cot) in `dtype`.  Keys: "out", "taps", "d_mel", "param/<key>"."""
    Wd = {k: v.detach().to(dtype, copy=True).requires_grad_() for k, v in W.items()}
    x = mel.detach().to(dtype, copy=True).requires_grad_()
    taps = {}
    out = generator_forward(Wd, x, taps=taps, masks=masks)
    (out * cot.to(dtype)).sum().backward()
    res = {"out": out.detach(), "taps": {k: v.detach() for k, v in taps.items()}, "d_mel": x.grad}
    for k, v in Wd.items():
        res["param/" + k] = v.grad
    return res
