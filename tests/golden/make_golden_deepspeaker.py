#!/usr/bin/env python3
"""Generate tests/golden/deepspeaker.npz and tests/golden/deepspeaker_manifest.json by running the REAL reference
DeepSpeaker front end and model builder (deepspeaker/audio_ds.py read_mfcc, deepspeaker/batcher.py sample_from_mfcc,
deepspeaker/conv_models.py DeepSpeakerModel) on the CPU.

Run in the build container only:   python tests/golden/make_golden_deepspeaker.py
It writes data only: four synthetic 22.05 kHz float32 signals with silence margins, their trim bounds, frame counts,
the crop offsets a seeded `random` drew, the [160, 64, 1] model inputs; and the layer graph of DeepSpeakerModel()
(name, type, filters, kernel, strides, padding, order), without weights.

Absent packages are stubbed before the reference is imported: librosa (read_mfcc does not use it),
python_speech_features (its 0.6 `fbank`, restated below) and tensorflow, whose keras layers are replaced by classes
that record their configuration and call order.
"""
import decimal
import json
import math
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SR, WIN = 22050, 1024
SEED = 1234


# ------------------------------------------------------------------ python_speech_features 0.6 fbank (restated)
def _round_half_up(number):
    return int(decimal.Decimal(number).quantize(decimal.Decimal("1"), rounding=decimal.ROUND_HALF_UP))


def _preemphasis(signal, coeff=0.95):
    return np.append(signal[0], signal[1:] - coeff * signal[:-1])


def _framesig(sig, frame_len, frame_step, winfunc=lambda x: np.ones((x,))):
    slen = len(sig)
    frame_len = int(_round_half_up(frame_len))
    frame_step = int(_round_half_up(frame_step))
    if slen <= frame_len:
        numframes = 1
    else:
        numframes = 1 + int(math.ceil((1.0 * slen - frame_len) / frame_step))
    padlen = int((numframes - 1) * frame_step + frame_len)
    padsignal = np.concatenate((sig, np.zeros((padlen - slen,))))
    indices = np.tile(np.arange(0, frame_len), (numframes, 1)) + \
        np.tile(np.arange(0, numframes * frame_step, frame_step), (frame_len, 1)).T
    frames = padsignal[indices.astype(np.int32, copy=False)]
    return frames * np.tile(winfunc(frame_len), (numframes, 1))


def _powspec(frames, nfft):
    return 1.0 / nfft * np.square(np.absolute(np.fft.rfft(frames, nfft)))


def _hz2mel(hz):
    return 2595 * np.log10(1 + hz / 700.)


def _mel2hz(mel):
    return 700 * (10 ** (mel / 2595.0) - 1)


def _get_filterbanks(nfilt, nfft, samplerate, lowfreq, highfreq):
    highfreq = highfreq or samplerate / 2
    melpoints = np.linspace(_hz2mel(lowfreq), _hz2mel(highfreq), nfilt + 2)
    bins = np.floor((nfft + 1) * _mel2hz(melpoints) / samplerate)
    fb = np.zeros([nfilt, nfft // 2 + 1])
    for j in range(nfilt):
        for i in range(int(bins[j]), int(bins[j + 1])):
            fb[j, i] = (i - bins[j]) / (bins[j + 1] - bins[j])
        for i in range(int(bins[j + 1]), int(bins[j + 2])):
            fb[j, i] = (bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])
    return fb


def fbank(signal, samplerate=16000, winlen=0.025, winstep=0.01, nfilt=26, nfft=512, lowfreq=0, highfreq=None,
          preemph=0.97, winfunc=lambda x: np.ones((x,))):
    highfreq = highfreq or samplerate / 2
    signal = _preemphasis(signal, preemph)
    frames = _framesig(signal, winlen * samplerate, winstep * samplerate, winfunc)
    pspec = _powspec(frames, nfft)
    energy = np.sum(pspec, 1)
    energy = np.where(energy == 0, np.finfo(float).eps, energy)
    fb = _get_filterbanks(nfilt, nfft, samplerate, lowfreq, highfreq)
    feat = np.dot(pspec, fb.T)
    feat = np.where(feat == 0, np.finfo(float).eps, feat)
    return feat, energy


# ------------------------------------------------------------------ recording keras stubs
GRAPH = []


class _T:
    """Symbolic tensor stand-in."""


class _Layer:
    kind = "Layer"

    def __init__(self, *args, **kw):
        self.args, self.kw = args, kw
        self.name = kw.get("name")

    def config(self):
        return {}

    def __call__(self, x):
        rec = {"type": self.kind, "name": self.name}
        rec.update(self.config())
        GRAPH.append(rec)
        return _T()


class Conv2D(_Layer):
    kind = "Conv2D"

    def config(self):
        k = self.kw.get("kernel_size")
        s = self.kw.get("strides", 1)
        return {"filters": self.args[0] if self.args else self.kw["filters"],
                "kernel": list(k) if isinstance(k, (tuple, list)) else [k, k],
                "strides": list(s) if isinstance(s, (tuple, list)) else [s, s],
                "padding": self.kw.get("padding", "valid"), "activation": self.kw.get("activation"),
                "use_bias": self.kw.get("use_bias", True)}


class BatchNormalization(_Layer):
    kind = "BatchNormalization"

    def config(self):
        return {"epsilon": self.kw.get("epsilon", 1e-3)}


class Lambda(_Layer):
    kind = "Lambda"

    def __init__(self, fn, **kw):
        super().__init__(**kw)


class Reshape(_Layer):
    kind = "Reshape"

    def config(self):
        return {"target_shape": list(self.args[0])}


class Dense(_Layer):
    kind = "Dense"

    def config(self):
        return {"units": self.args[0], "activation": self.kw.get("activation")}


class Dropout(_Layer):
    kind = "Dropout"


def Input(batch_shape=None, name=None, **kw):
    GRAPH.append({"type": "Input", "name": name, "batch_shape": list(batch_shape)})
    return _T()


def _add(xs):
    GRAPH.append({"type": "Add", "name": None, "inputs": len(xs)})
    return _T()


class Model:
    def __init__(self, inputs, outputs, name=None):
        self.name = name


def _install_stubs():
    sys.dont_write_bytecode = True
    sys.modules["librosa"] = types.ModuleType("librosa")
    psf = types.ModuleType("python_speech_features")
    psf.fbank = fbank
    sys.modules["python_speech_features"] = psf
    tf = types.ModuleType("tensorflow")
    keras = types.ModuleType("tensorflow.keras")
    backend = types.ModuleType("tensorflow.keras.backend")
    layers = types.ModuleType("tensorflow.keras.layers")
    for c in (Conv2D, BatchNormalization, Lambda, Reshape, Dense, Dropout):
        setattr(layers, c.__name__, c)
    layers.Input = Input
    layers.add = _add
    regs = types.ModuleType("tensorflow.keras.regularizers")
    regs.l2 = lambda l=0.0: ("l2", l)  # noqa: E741
    models = types.ModuleType("tensorflow.keras.models")
    models.Model = Model
    opts = types.ModuleType("tensorflow.keras.optimizers")
    opts.Adam = object
    keras.backend, keras.layers, keras.regularizers, keras.models, keras.optimizers = backend, layers, regs, models, opts
    tf.keras = keras
    for name, m in (("tensorflow", tf), ("tensorflow.keras", keras), ("tensorflow.keras.backend", backend),
                    ("tensorflow.keras.layers", layers), ("tensorflow.keras.regularizers", regs),
                    ("tensorflow.keras.models", models), ("tensorflow.keras.optimizers", opts)):
        sys.modules[name] = m
    if REF not in sys.path:
        sys.path.insert(0, REF)


# ------------------------------------------------------------------ signals
def _signal(rng, n_voiced, lead, tail, f0, kind):
    t = np.arange(n_voiced) / SR
    env = 0.5 * (1 - np.cos(2 * np.pi * np.minimum(t / 0.05, 0.5)))  # 25 ms fade-in
    env = env * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t))
    if kind == "harmonic":
        v = sum(np.sin(2 * np.pi * f0 * h * t + h) / h for h in range(1, 12))
    elif kind == "chirp":
        v = np.sin(2 * np.pi * (f0 * t + 400.0 * t * t)) + 0.3 * rng.standard_normal(n_voiced)
    else:
        v = np.sign(np.sin(2 * np.pi * f0 * t)) * 0.5 + 0.2 * rng.standard_normal(n_voiced)
    v = 0.3 * env * v / np.abs(v).max()
    sil = lambda n: 1e-4 * rng.standard_normal(n)  # noqa: E731
    return np.concatenate([sil(lead), v, sil(tail)]).astype(np.float32)


SIGNALS = (  # (voiced samples, lead silence, tail silence, f0, kind): frame counts > 160, < 160, > 160, < 160
    (44100, 2205, 4410, 140.0, "harmonic"),
    (19845, 3300, 1100, 220.0, "chirp"),
    (38000, 1000, 2000, 95.0, "square"),
    (9000, 500, 700, 310.0, "harmonic"),
)


def main():
    _install_stubs()
    from deepspeaker.audio_ds import read_mfcc, calculate_nfft
    from deepspeaker.batcher import sample_from_mfcc
    from deepspeaker.constants import NUM_FRAMES
    from deepspeaker.conv_models import DeepSpeakerModel

    rng = np.random.default_rng(SEED)
    out, man = {}, {"sample_rate": SR, "win_length": WIN, "seed": SEED, "signals": []}
    man["nfft"] = calculate_nfft(SR, WIN / SR)
    random.seed(SEED)
    for i, spec in enumerate(SIGNALS):
        x = _signal(rng, *spec)
        e = np.abs(x)
        thr = np.percentile(e, 95)
        idx = np.where(e > thr)[0]
        mfcc = read_mfcc(x, SR, WIN)
        state = random.getstate()
        s = sample_from_mfcc(mfcc, NUM_FRAMES)
        random.setstate(state)
        r = random.choice(range(0, len(mfcc) - NUM_FRAMES + 1)) if len(mfcc) >= NUM_FRAMES else -1
        random.setstate(state)
        s2 = sample_from_mfcc(mfcc, NUM_FRAMES)  # the same draw again: the recorded offset is the one used
        assert np.array_equal(s, s2)
        if r >= 0:
            assert np.array_equal(s[:, :, 0], mfcc[r:r + NUM_FRAMES])
        out["x%d" % i] = x
        out["x%d_input" % i] = s.astype(np.float32)
        man["signals"].append({"name": "x%d" % i, "n": int(len(x)), "start": int(idx[0]), "end": int(idx[-1]),
                               "threshold": float(thr), "frames": int(len(mfcc)), "offset": int(r)})
    nfr = [s["frames"] for s in man["signals"]]
    assert any(n < NUM_FRAMES for n in nfr) and any(n > NUM_FRAMES for n in nfr), nfr

    GRAPH.clear()
    DeepSpeakerModel()
    man["graph"] = list(GRAPH)
    np.savez_compressed(os.path.join(HERE, "deepspeaker.npz"), **out)
    with open(os.path.join(HERE, "deepspeaker_manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    print("frames", nfr, "graph layers", len(man["graph"]),
          "npz bytes", os.path.getsize(os.path.join(HERE, "deepspeaker.npz")))


if __name__ == "__main__":
    main()
