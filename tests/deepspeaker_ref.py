"""Plain restatement of the DeepSpeaker embedder for the tests (no HIP): the front end in numpy (python_speech_features
0.6 fbank, normalize_frames, sample_from_mfcc) and the ResCNN in Keras semantics in float64 torch (NHWC weights,
explicit TF 'same' padding, inference BatchNorm with eps 1e-3, clipped ReLU at 20, Reshape (-1, 2048) in w * 512 + c
order, mean, Dense, l2_normalize).  Also seeded Keras-named weights whose BatchNorm moving statistics are calibrated
on real activations, so that every clipped ReLU works in its linear range."""
import decimal
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

SR, WIN = 22050, 1024
NUM_FRAMES, NUM_FBANKS = 160, 64
FILTERS = (64, 128, 256, 512)
BN_EPS = 1e-3


# ------------------------------------------------------------------ front end
def round_half_up(x):
    return int(decimal.Decimal(x).quantize(decimal.Decimal("1"), rounding=decimal.ROUND_HALF_UP))


def trim(audio):
    """read_mfcc's trim: (start, end) with audio[start:end] kept; IndexError when nothing exceeds the threshold."""
    e = np.abs(audio)
    idx = np.where(e > np.percentile(e, 95))[0]
    return int(idx[0]), int(idx[-1])


def filterbank(nfilt, nfft, sr):
    hz2mel = lambda h: 2595 * np.log10(1 + h / 700.)  # noqa: E731
    mel2hz = lambda m: 700 * (10 ** (m / 2595.0) - 1)  # noqa: E731
    b = np.floor((nfft + 1) * mel2hz(np.linspace(hz2mel(0), hz2mel(sr / 2), nfilt + 2)) / sr)
    fb = np.zeros([nfilt, nfft // 2 + 1])
    for j in range(nfilt):
        i = np.arange(int(b[j]), int(b[j + 1]))
        fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        i = np.arange(int(b[j + 1]), int(b[j + 2]))
        fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def nfft_for(sr, win_length):
    n = 1
    while n < win_length / sr * sr:
        n *= 2
    return n


def fbank_features(signal, sr=SR, win_length=WIN):
    """Normalised fbank features [n_frames, 64] float32 of an already trimmed signal."""
    nfft = nfft_for(sr, win_length)
    y = np.append(signal[0], signal[1:] - 0.97 * signal[:-1])  # in the signal's dtype, as the reference
    flen, fstep = round_half_up(0.025 * sr), round_half_up(0.01 * sr)
    slen = len(y)
    nfr = 1 if slen <= flen else 1 + int(math.ceil((1.0 * slen - flen) / fstep))
    pad = np.concatenate((y, np.zeros(((nfr - 1) * fstep + flen - slen,))))
    frames = pad[np.arange(flen)[None, :] + fstep * np.arange(nfr)[:, None]]
    pspec = 1.0 / nfft * np.square(np.absolute(np.fft.rfft(frames, nfft)))
    feat = np.dot(pspec, filterbank(NUM_FBANKS, nfft, sr).T)
    feat = np.where(feat == 0, np.finfo(float).eps, feat)
    out = [(v - np.mean(v)) / max(np.std(v), 1e-12) for v in feat]
    return np.array(out, dtype=np.float32)


def model_input(audio, offset, sr=SR, win_length=WIN):
    """read_mfcc + sample_from_mfcc with a given crop offset (ignored below 160 frames): [160, 64] float32."""
    s, e = trim(audio)
    m = fbank_features(audio[s:e], sr, win_length)
    if len(m) >= NUM_FRAMES:
        return m[offset:offset + NUM_FRAMES]
    return np.vstack([m, np.zeros((NUM_FRAMES - len(m), NUM_FBANKS), np.float32)])


# ------------------------------------------------------------------ network
def tf_same(n, k, s):
    o = -(-n // s)
    t = max((o - 1) * s + k - n, 0)
    return o, t // 2, t - t // 2


def conv_names():
    names = []
    for st, f in enumerate(FILTERS, 1):
        names.append(("conv%d-s" % f, f, 5, 2))
        for i in range(3):
            names += [("res%d_%d_branch_2a" % (st, i), f, 3, 1), ("res%d_%d_branch_2b" % (st, i), f, 3, 1)]
    return names


def conv_bn_clip(x, W, name, k, s, res=None):
    """x NCHW float64; Keras Conv2D(padding='same') + BatchNormalization + clipped ReLU (+ add + clip)."""
    _, pt, pb = tf_same(x.shape[2], k, s)
    _, pl, pr = tf_same(x.shape[3], k, s)
    w = torch.as_tensor(W[name + "/kernel:0"], dtype=x.dtype, device=x.device).permute(3, 2, 0, 1)
    b = torch.as_tensor(W[name + "/bias:0"], dtype=x.dtype, device=x.device)
    y = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, b, stride=s)
    g = lambda p: torch.as_tensor(W["%s_bn/%s:0" % (name, p)], dtype=x.dtype, device=x.device)[None, :, None, None]  # noqa: E731
    y = (y - g("moving_mean")) / torch.sqrt(g("moving_variance") + BN_EPS) * g("gamma") + g("beta")
    y = y.clamp(0, 20)
    if res is not None:
        y = (y + res).clamp(0, 20)
    return y


def rescnn(inputs, W, record=None):
    """inputs [N, 160, 64] -> [N, 512] embeddings (float64, on the inputs' device)."""
    x = torch.as_tensor(inputs, dtype=torch.float64)[:, None]
    for name, f, k, s in conv_names():
        if name.endswith("_2a"):
            block_in = x
        x = conv_bn_clip(x, W, name, k, s, block_in if name.endswith("_2b") else None)
        if record is not None:
            record[name] = x
    N = x.shape[0]
    h = x.permute(0, 2, 3, 1).reshape(N, -1, 2048).mean(1)
    h = h @ torch.as_tensor(W["affine/kernel:0"], dtype=x.dtype, device=x.device) + \
        torch.as_tensor(W["affine/bias:0"], dtype=x.dtype, device=x.device)
    return h * torch.rsqrt(torch.clamp((h * h).sum(1, keepdim=True), min=1e-12))


def _calibration_inputs(n=6, seed=7):
    """Front-end outputs of seeded synthetic utterances (harmonic tones over noise)."""
    rng = np.random.default_rng(seed)
    xs = []
    for i in range(n):
        L = 36000 + 4000 * i
        t = np.arange(L) / SR
        f0 = 100.0 + 37.0 * i
        v = sum(np.sin(2 * np.pi * f0 * h * t + 0.3 * h * i) / h for h in range(1, 10))
        v = v * (0.6 + 0.4 * np.sin(2 * np.pi * (2 + i) * t)) + 0.2 * rng.standard_normal(L)
        xs.append(model_input((0.3 * v / np.abs(v).max()).astype(np.float32), 0))
    return np.stack(xs)


@functools.lru_cache(maxsize=None)
def seeded_weights(seed=0):
    """Keras-named weights: glorot-uniform kernels, small biases, gamma in [0.8, 1.5], beta in [0.1, 0.8]; each BN's
    moving mean / variance are the batch statistics of its conv's output on calibration utterances, so every
    BN output is about N(beta, gamma^2) and the clips at 0 and 20 cut only part of it."""
    rng = np.random.default_rng(seed)
    W = {}
    x = torch.as_tensor(_calibration_inputs(), dtype=torch.float64)[:, None]
    ci = 1
    for name, f, k, s in conv_names():
        lim = math.sqrt(6.0 / (k * k * ci + k * k * f))
        W[name + "/kernel:0"] = rng.uniform(-lim, lim, (k, k, ci, f))
        W[name + "/bias:0"] = rng.uniform(-0.05, 0.05, f)
        W[name + "_bn/gamma:0"] = rng.uniform(0.8, 1.5, f)
        W[name + "_bn/beta:0"] = rng.uniform(0.1, 0.8, f)
        if name.endswith("_2a"):
            block_in = x
        _, pt, pb = tf_same(x.shape[2], k, s)
        _, pl, pr = tf_same(x.shape[3], k, s)
        raw = F.conv2d(F.pad(x, (pl, pr, pt, pb)), torch.as_tensor(W[name + "/kernel:0"]).permute(3, 2, 0, 1),
                       torch.as_tensor(W[name + "/bias:0"]), stride=s)
        W[name + "_bn/moving_mean:0"] = raw.mean((0, 2, 3)).numpy()
        W[name + "_bn/moving_variance:0"] = raw.var((0, 2, 3), unbiased=False).numpy()
        x = conv_bn_clip(x, W, name, k, s, block_in if name.endswith("_2b") else None)
        ci = f
    lim = math.sqrt(6.0 / (2048 + 512))
    W["affine/kernel:0"] = rng.uniform(-lim, lim, (2048, 512))
    W["affine/bias:0"] = rng.uniform(-0.05, 0.05, 512)
    return W


def saturation(inputs, W):
    """Per conv layer: (fraction of outputs at 0, fraction at 20) on the given model inputs."""
    rec = {}
    rescnn(inputs, W, rec)
    return {k: (float((v == 0).double().mean()), float((v == 20).double().mean())) for k, v in rec.items()}
