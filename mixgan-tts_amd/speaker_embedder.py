"""DeepSpeaker ResCNN speaker embedder (reference model/speaker_embedder.py over deepspeaker/audio_ds.py, batcher.py,
conv_models.py, embedding.py) on HIP: the external speaker embeddings `spker_embed/<spk>-spker_embed.npy` that
`data.Dataset` reads and `MixGANTTS.speaker_emb` projects.

Pipeline per utterance (csrc/deepspeaker.hip):
- trim: keep audio[first : last) of the samples whose |x| exceeds numpy's 95th percentile of |x| (device sort, the
  interpolation done in the audio's dtype in numpy's own order, so the bounds equal numpy's);
- the python_speech_features 0.6 `fbank` (pre-emphasis 0.97, 25 ms / 10 ms rectangular frames, power spectrum of the
  smallest power-of-two FFT >= win_length, 64 triangular mel filters, not logged) of the 160 frames sample_from_mfcc
  keeps, each frame normalised over its filters;
- the ResCNN (four stages of a 5x5 stride-2 conv and three identity blocks, BatchNorm folded into the convs at load
  time, clipped ReLU at 20), the time mean, Dense 2048 -> 512 and l2 normalisation.

There is no CPU path: audio must be on the GPU (PreDefinedEmbedder.forward moves its numpy input there).
"""
import decimal
import math
import os
import random
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._lib import fptr, iptr, check, stream_ptr, MixganHipError
from .audio import N_FFT, mel_bands

NUM_FRAMES = 160
NUM_FBANKS = 64
EMBED_DIM = 512
STAGE_FILTERS = (64, 128, 256, 512)
BN_EPS = 1e-3  # Keras BatchNormalization default
DEFAULT_CHECKPOINT = "./deepspeaker/pretrained_models/ResCNN_triplet_training_checkpoint_265.h5"


class DeepSpeakerCheckpointRequired(MixganHipError, FileNotFoundError):
    """PreDefinedEmbedder without the Keras checkpoint: the reference ships no weights for it."""


def round_half_up(number):
    """python_speech_features.sigproc.round_half_up."""
    return int(decimal.Decimal(number).quantize(decimal.Decimal("1"), rounding=decimal.ROUND_HALF_UP))


def calculate_nfft(samplerate, winlen):
    """Smallest power of two >= winlen * samplerate (deepspeaker/audio_ds.py calculate_nfft)."""
    window_length_samples = winlen * samplerate
    nfft = 1
    while nfft < window_length_samples:
        nfft *= 2
    return nfft


def tf_same_padding(n, k, stride):
    """TensorFlow 'same' padding of one axis: (output size, pad before, pad after)."""
    out = -(-n // stride)
    total = max((out - 1) * stride + k - n, 0)
    return out, total // 2, total - total // 2


def fbank_filters(nfilt, nfft, samplerate, lowfreq=0, highfreq=None):
    """python_speech_features 0.6 get_filterbanks: float64 [nfilt, nfft // 2 + 1]."""
    highfreq = highfreq or samplerate / 2
    hz2mel = lambda hz: 2595 * np.log10(1 + hz / 700.)  # noqa: E731
    mel2hz = lambda mel: 700 * (10 ** (mel / 2595.0) - 1)  # noqa: E731
    melpoints = np.linspace(hz2mel(lowfreq), hz2mel(highfreq), nfilt + 2)
    bins = np.floor((nfft + 1) * mel2hz(melpoints) / samplerate)
    fb = np.zeros([nfilt, nfft // 2 + 1])
    for j in range(nfilt):
        for i in range(int(bins[j]), int(bins[j + 1])):
            fb[j, i] = (i - bins[j]) / (bins[j + 1] - bins[j])
        for i in range(int(bins[j + 1]), int(bins[j + 2])):
            fb[j, i] = (bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])
    return fb


def num_frames(slen, frame_len, frame_step):
    """python_speech_features 0.6 framesig's frame count."""
    if slen <= frame_len:
        return 1
    return 1 + int(math.ceil((1.0 * slen - frame_len) / frame_step))


def layer_specs():
    """The ResCNN's convolutions in graph order: (name, filters, kernel, stride).  Each is followed by BatchNorm
    `<name>_bn` and a clipped ReLU; `_2b` convs add the identity block's input and clip again."""
    specs = []
    for stage, f in enumerate(STAGE_FILTERS, 1):
        specs.append(("conv%d-s" % f, f, 5, 2))
        for i in range(3):
            specs.append(("res%d_%d_branch_2a" % (stage, i), f, 3, 1))
            specs.append(("res%d_%d_branch_2b" % (stage, i), f, 3, 1))
    return specs


def keras_weight_shapes():
    """Keras weight names -> shapes the model loads, in graph order (Conv2D HWIO kernel + bias, BatchNormalization
    gamma / beta / moving_mean / moving_variance, Dense `affine`)."""
    shapes = OrderedDict()
    ci = 1
    for name, f, k, _ in layer_specs():
        shapes[name + "/kernel:0"] = (k, k, ci, f)
        shapes[name + "/bias:0"] = (f,)
        for p in ("gamma", "beta", "moving_mean", "moving_variance"):
            shapes["%s_bn/%s:0" % (name, p)] = (f,)
        ci = f
    shapes["affine/kernel:0"] = (2048, EMBED_DIM)
    shapes["affine/bias:0"] = (EMBED_DIM,)
    return shapes


def _percentile95_plan(n, dtype):
    """numpy.percentile(e, 95) of n values, method 'linear', as numpy 2 computes it in the array's dtype: the sorted
    positions (lo, hi) and gamma, 1 - gamma in that dtype."""
    q = np.asanyarray(np.true_divide(95, dtype.type(100)))
    vi = np.asanyarray((n - 1) * q)
    prev = np.floor(vi)
    gamma = np.asanyarray(vi - prev, dtype=vi.dtype)
    if vi >= n - 1:
        lo = hi = n - 1
    else:
        lo = int(prev)
        hi = lo + 1
    return lo, hi, gamma[()], np.asanyarray(1 - gamma)[()]


def trim_bounds(audio, lengths):
    """deepspeaker read_mfcc's trim for each row of audio [B, L] (item b has lengths[b] samples): (start, end) int64
    device tensors with audio[b, start : end) the kept samples, and a bool tensor `found` (False where no sample
    exceeds the threshold, where the reference raises).  Runs on any device; the bounds equal numpy's exactly."""
    B, L = audio.shape
    dt = np.dtype({torch.float32: np.float32, torch.float64: np.float64}[audio.dtype])
    dev = audio.device
    e = audio.abs()
    pos = torch.arange(L, device=dev)
    lens = torch.as_tensor(lengths, device=dev, dtype=torch.int64)
    valid = pos[None, :] < lens[:, None]
    srt = torch.where(valid, e, torch.full_like(e, float("inf"))).sort(dim=1).values
    plans = [_percentile95_plan(int(n), dt) for n in lengths]
    lo = torch.tensor([p[0] for p in plans], device=dev)
    hi = torch.tensor([p[1] for p in plans], device=dev)
    gamma = torch.tensor(np.array([p[2] for p in plans], dtype=dt), device=dev)
    omg = torch.tensor(np.array([p[3] for p in plans], dtype=dt), device=dev)
    a = srt.gather(1, lo[:, None])[:, 0]
    b = srt.gather(1, hi[:, None])[:, 0]
    diff = b - a
    thr = torch.where(gamma >= 0.5, b - diff * omg, a + diff * gamma)
    above = (e > thr[:, None]) & valid
    found = above.any(dim=1)
    first = above.to(torch.uint8).argmax(dim=1)
    last = L - 1 - above.flip(1).to(torch.uint8).argmax(dim=1)
    return first, last, found


class DeepSpeakerModel:
    """The reference's DeepSpeakerModel (include_softmax=False) at inference, with its front end: embed() maps raw
    utterances to l2-normalised [N, 512] speaker embeddings."""

    def __init__(self, sample_rate=22050, win_length=1024, device="cuda", chunk=256):
        self.sample_rate = sample_rate
        self.win_length = win_length
        self.nfft = calculate_nfft(sample_rate, win_length / sample_rate)
        if self.nfft != N_FFT:
            raise MixganHipError("DeepSpeaker: the fbank kernel takes a %d-point FFT; win_length %d gives %d"
                                 % (N_FFT, win_length, self.nfft))
        self.frame_len = round_half_up(0.025 * sample_rate)
        self.frame_step = round_half_up(0.01 * sample_rate)
        if self.frame_len > N_FFT:
            raise MixganHipError("DeepSpeaker: a %d-sample frame does not fit the %d-point FFT"
                                 % (self.frame_len, N_FFT))
        self.device = torch.device(device)
        self.chunk = int(chunk)
        fb = fbank_filters(NUM_FBANKS, self.nfft, sample_rate)
        band, band_w = mel_bands(fb)
        tw = np.exp(-2j * np.pi * np.arange(N_FFT) / N_FFT)
        self._band = torch.from_numpy(band).to(self.device)
        self._band_w = torch.from_numpy(band_w).to(self.device)
        self._tw = torch.from_numpy(np.stack([tw.real, tw.imag], 1).astype(np.float32).reshape(-1)).to(self.device)
        self.convs = None  # [(name, packed weight [k k ci, co], bias [co], ci, co, k, stride)]
        self.affine = None

    # ------------------------------------------------------------------ weights
    def load_keras_weights(self, mapping):
        """Load Keras-named weights ({"conv64-s/kernel:0": array, ...}); extra names are ignored (load_weights
        by_name), missing or mis-shaped ones raise.  BatchNorm is folded into each conv's weight and bias."""
        shapes = keras_weight_shapes()
        missing = [k for k in shapes if k not in mapping]
        if missing:
            raise KeyError("DeepSpeaker: missing weights %s" % missing)
        W = {}
        for k, shp in shapes.items():
            a = np.asarray(mapping[k], dtype=np.float64)
            if a.shape != shp:
                raise ValueError("DeepSpeaker: weight %s has shape %s, expected %s" % (k, a.shape, shp))
            W[k] = a
        convs = []
        for name, f, k, s in layer_specs():
            kern = W[name + "/kernel:0"]
            scale = W[name + "_bn/gamma:0"] / np.sqrt(W[name + "_bn/moving_variance:0"] + BN_EPS)
            bias = (W[name + "/bias:0"] - W[name + "_bn/moving_mean:0"]) * scale + W[name + "_bn/beta:0"]
            ci = kern.shape[2]
            packed = (kern * scale).reshape(k * k * ci, f)
            convs.append((name, torch.from_numpy(packed.astype(np.float32)).to(self.device),
                          torch.from_numpy(bias.astype(np.float32)).to(self.device), ci, f, k, s))
        self.convs = convs
        self.affine = (torch.from_numpy(W["affine/kernel:0"].astype(np.float32)).to(self.device),
                       torch.from_numpy(W["affine/bias:0"].astype(np.float32)).to(self.device))
        return self

    @classmethod
    def from_h5(cls, path, **kwargs):
        """Load a Keras checkpoint (.h5, saved by model.save_weights) by layer name."""
        try:
            import h5py
        except ImportError as e:
            raise MixganHipError("DeepSpeakerModel.from_h5 needs h5py to read %s; it is not installed. Load the "
                                 "weights yourself and pass them to load_keras_weights()" % path) from e
        mapping = {}
        with h5py.File(path, "r") as f:
            root = f["model_weights"] if "model_weights" in f else f

            def visit(name, obj):
                if isinstance(obj, h5py.Dataset):
                    parts = name.split("/")
                    mapping["/".join(parts[-2:])] = obj[()]
            root.visititems(visit)
        return cls(**kwargs).load_keras_weights(mapping)

    # ------------------------------------------------------------------ front end
    def _check_audio(self, audio, lengths):
        if not (isinstance(audio, torch.Tensor) and audio.is_cuda):
            raise MixganHipError("DeepSpeaker: audio must be a CUDA tensor: the HIP path has no CPU fallback")
        if audio.dim() != 2 or audio.dtype not in (torch.float32, torch.float64):
            raise ValueError("DeepSpeaker: expected float audio [N, L], got %s %s" % (audio.dtype, tuple(audio.shape)))
        lengths = [int(n) for n in (lengths.tolist() if torch.is_tensor(lengths) else lengths)]
        if len(lengths) != audio.shape[0] or any(n < 2 or n > audio.shape[1] for n in lengths):
            raise ValueError("DeepSpeaker: lengths must give 2 <= length <= %d for each of the %d items"
                             % (audio.shape[1], audio.shape[0]))
        return audio.contiguous(), lengths

    def frontend(self, audio, lengths, offsets=None, first_index=0):
        """Trim, draw the crops and compute the model input: (feats [N, 160, 64] fp32, start, end, frame counts,
        offsets), the last four as host lists."""
        audio, lengths = self._check_audio(audio, lengths)
        first, last, found = trim_bounds(audio, lengths)
        bounds = torch.stack([first, last, found.to(first.dtype)]).cpu().tolist()  # the one host sync
        start, end = bounds[0], bounds[1]
        for i, ok in enumerate(bounds[2]):
            if not ok or end[i] <= start[i]:
                raise ValueError("DeepSpeaker: utterance %d has no sample above its 95th-percentile |x| to keep "
                                 "(the reference raises IndexError on it)" % (first_index + i))
        nfr = [num_frames(e - s, self.frame_len, self.frame_step) for s, e in zip(start, end)]
        if offsets is None:
            offsets = [random.choice(range(0, n - NUM_FRAMES + 1)) if n >= NUM_FRAMES else 0 for n in nfr]
        else:
            offsets = [int(o) for o in offsets]
            if len(offsets) != len(nfr) or any(o < 0 or (n >= NUM_FRAMES and o > n - NUM_FRAMES) or
                                               (n < NUM_FRAMES and o != 0) for o, n in zip(offsets, nfr)):
                raise ValueError("DeepSpeaker: offsets must lie in [0, frames - 160] (0 below 160 frames)")
        dev = audio.device
        x = audio if audio.dtype == torch.float32 else audio.float()
        B = x.shape[0]
        meta = torch.tensor([start, end, offsets], dtype=torch.int32).to(dev)
        out = torch.empty(B, NUM_FRAMES, NUM_FBANKS, device=dev)
        check(_lib.lib().mg_ds_fbank(fptr(x), x.shape[1], iptr(meta[0], torch.int32), iptr(meta[1], torch.int32),
                                     iptr(meta[2], torch.int32), B, NUM_FRAMES, self.frame_len, self.frame_step,
                                     fptr(self._tw), iptr(self._band, torch.int32), fptr(self._band_w), NUM_FBANKS,
                                     fptr(out), stream_ptr()))
        return out, start, end, nfr, offsets

    # ------------------------------------------------------------------ network
    def network(self, feats):
        """ResCNN + head on the model input [N, 160, 64] (NHWC with one channel): [N, 512]."""
        if self.convs is None:
            raise MixganHipError("DeepSpeaker: no weights loaded (load_keras_weights / from_h5)")
        feats = feats.contiguous()
        B, H, W = feats.shape
        x = feats
        for name, w, b, ci, co, k, s in self.convs:
            if name.endswith("_2a"):
                block_in = x
            res = block_in if name.endswith("_2b") else None
            x, H, W = conv2d_same(x, w, b, B, H, W, ci, co, k, s, res)
        D = W * x.shape[-1]
        out = torch.empty(B, EMBED_DIM, device=x.device)
        kw, kb = self.affine
        if kw.shape[0] != D:
            raise MixganHipError("DeepSpeaker: the head takes %d features, the net gives %d" % (kw.shape[0], D))
        check(_lib.lib().mg_ds_head(fptr(x), fptr(kw), fptr(kb), fptr(out), B, H, D, EMBED_DIM, stream_ptr()))
        return out

    def embed(self, audio, lengths, offsets=None):
        """Embeddings [N, 512] fp32 on the device of utterances audio[n, :lengths[n]] (float, CUDA).  offsets: the
        first kept frame of each utterance; None draws them with random.choice in utterance order, as the
        reference's sample_from_mfcc.  Large batches run in chunks of `chunk` utterances."""
        audio, lengths = self._check_audio(audio, lengths)
        outs = []
        for c0 in range(0, audio.shape[0], self.chunk):
            c1 = min(c0 + self.chunk, audio.shape[0])
            feats = self.frontend(audio[c0:c1], lengths[c0:c1], None if offsets is None else offsets[c0:c1],
                                  first_index=c0)[0]
            outs.append(self.network(feats))
        return outs[0] if len(outs) == 1 else torch.cat(outs)


def conv2d_same(x, w, bias, B, H, W, ci, co, k, stride, res=None):
    """One ResCNN conv (NHWC, TF 'same' padding, BN folded into w / bias) with its clipped-ReLU epilogue and
    optional residual: (y [B, Ho, Wo, co], Ho, Wo)."""
    Ho, Wo = tf_same_padding(H, k, stride)[0], tf_same_padding(W, k, stride)[0]
    y = torch.empty(B, Ho, Wo, co, device=x.device)
    check(_lib.lib().mg_ds_conv2d(fptr(x), fptr(w), fptr(bias), fptr(res, allow_none=True), fptr(y), B, H, W, ci, co,
                                  k, stride, stream_ptr()))
    return y, Ho, Wo


class PreDefinedEmbedder(torch.nn.Module):
    """model/speaker_embedder.py PreDefinedEmbedder: forward(wav) -> np.float32 [1, 512].  `speaker_embedder_cuda`
    is read and ignored (the embedder always runs on the GPU)."""

    def __init__(self, config, checkpoint_path=None):
        super().__init__()
        self.sampling_rate = config["preprocessing"]["audio"]["sampling_rate"]
        self.win_length = config["preprocessing"]["stft"]["win_length"]
        self.embedder_type = config["preprocessing"]["speaker_embedder"]
        self.embedder_cuda = config["preprocessing"].get("speaker_embedder_cuda", True)
        self.checkpoint_path = checkpoint_path or DEFAULT_CHECKPOINT
        self.embedder = self._get_speaker_embedder()

    def _get_speaker_embedder(self):
        if self.embedder_type != "DeepSpeaker":
            raise NotImplementedError(self.embedder_type)
        if not os.path.isfile(self.checkpoint_path):
            raise DeepSpeakerCheckpointRequired(
                "speaker embedder DeepSpeaker: checkpoint %s not found; the reference ships no weights for it, pass "
                "checkpoint_path= the ResCNN triplet-training .h5" % self.checkpoint_path)
        return DeepSpeakerModel.from_h5(self.checkpoint_path, sample_rate=self.sampling_rate,
                                        win_length=self.win_length)

    def forward(self, audio):
        x = torch.as_tensor(np.asarray(audio)).reshape(1, -1)
        if x.dtype not in (torch.float32, torch.float64):
            x = x.float()
        emb = self.embedder.embed(x.to(self.embedder.device), [x.shape[1]])
        return emb.cpu().numpy().astype(np.float32)


def save_speaker_embeddings(out_dir, speaker, embeds):
    """Write out_dir/spker_embed/<speaker>-spker_embed.npy: np.mean over the utterance embeddings (each [1, 512]
    float32), a float32 [1, 512], as the reference's preprocessor writes and data.Dataset reads."""
    arr = [np.asarray(e.detach().cpu().numpy() if torch.is_tensor(e) else e, dtype=np.float32).reshape(1, EMBED_DIM)
           for e in embeds]
    if not arr:
        raise ValueError("save_speaker_embeddings: no embeddings for speaker %r" % speaker)
    mean = np.mean(arr, axis=0).astype(np.float32)
    d = os.path.join(out_dir, "spker_embed")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "%s-spker_embed.npy" % speaker)
    np.save(path, mean, allow_pickle=False)
    return path
