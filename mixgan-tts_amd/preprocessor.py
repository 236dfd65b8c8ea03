"""Corpus builder (reference preprocessor/preprocessor.py): raw wavs + MFA TextGrids -> the tree data.Dataset reads.

Same constructor arguments, config keys, `build_from_path()` and output tree as the reference:
`<preprocessed_path>/{mel,pitch,energy,duration,phones_per_word,attn_prior}/<spk>-<kind>-<base>.npy`, `spker_embed/`,
`speakers.json`, `stats.json`, `train.txt`, `val.txt`, `filtered_out.txt`.  Mel and energy (csrc/audio.hip), the
phoneme-level averages and the alignment prior (csrc/corpus.hip) are computed on the GPU for `batch_utterances`
utterances at a time, with one device -> host copy per array kind.

Injected, as `text_to_sequence` is in data.py:
- `pitch_fn(wav_float64, sampling_rate, frame_period_ms) -> f0 [frames]`; the default is pyworld's dio + stonemask,
  imported when first needed (PitchExtractorRequired names the argument when pyworld is missing).
  `pitch_fn="native"` needs neither: the batch's wavs go to the device once, pitch.extract_f0 tracks them all in one
  launch pair (csrc/pitch.hip, an extractor of this project's own, not pyworld's), and mel and energy read the same
  upload;
- `load_wav(path) -> float array in [-1, 1)`; the default reads with scipy.io.wavfile.  A file whose rate is not
  `sampling_rate` raises SamplingRateMismatch, or with `resample=True` is resampled on the device by
  audio.resample (the reference resamples silently through librosa.load; prepare_align.py is the stage that brings a
  whole corpus to the configured rate).

Deviations from the reference:
- directory entries are visited in sorted order (the reference takes the file system's order, which also decides
  its speaker ids and the order that `random.shuffle` starts from);
- a wav without a TextGrid is skipped altogether (the reference feeds the previous utterance's statistics to its
  scalers a second time, or fails on the first file);
- mean and standard deviation are float64 running moments merged batch by batch (the reference: sklearn's
  StandardScaler.partial_fit);
- the mel file is written C-contiguous [L, n_mels] (the reference saves a transposed view, same content);
- the t-SNE plot of the speaker embeddings is not made.
"""
import json
import os
import random
import re

import numpy as np
import torch

from . import audio as Audio
from . import corpusops
from . import pitch as Pitch
from ._lib import MixganHipError
from .speaker_embedder import PreDefinedEmbedder, save_speaker_embeddings

SIL_PHONES = ("sil", "sp", "spn")


class PitchExtractorRequired(MixganHipError, ImportError):
    """No pitch extractor: pyworld is not installed and no pitch_fn was given."""


class SamplingRateMismatch(MixganHipError, ValueError):
    """A wav whose sampling rate is not the configured one, met without resample=True."""


class TextGridError(MixganHipError, ValueError):
    """A TextGrid this reader cannot take."""


# ---------------------------------------------------------------------------------------------
# TextGrid (Praat long text format, what the Montreal Forced Aligner writes)
# ---------------------------------------------------------------------------------------------
_TG_ATTR = re.compile(r"^\s*(\w+)\s*=\s*(.*?)\s*$")


def _tg_string(v):
    if len(v) < 2 or v[0] != '"' or v[-1] != '"':
        raise TextGridError("TextGrid: expected a quoted string, got %r" % v)
    return v[1:-1].replace('""', '"')


def read_textgrid(path, include_empty_intervals=False, encoding="utf-8"):
    """Interval tiers of a long-format TextGrid: {tier name: [(start, end, text), ...]} in file order.  Intervals with
    empty text are dropped unless `include_empty_intervals` (the default of the reader the reference uses)."""
    with open(path, "r", encoding=encoding) as f:
        lines = f.read().lstrip("\ufeff").splitlines()
    head = [ln.strip() for ln in lines[:2]]
    if (len(head) < 2 or "ooTextFile" not in head[0] or "short" in head[0] or not head[1].startswith("Object class")
            or "TextGrid" not in head[1]):
        raise TextGridError("%s: not a long-format TextGrid (header %r)" % (path, head))
    tiers, tier, cur = {}, None, {}
    for ln in lines[2:]:
        s = ln.strip()
        if re.match(r"^item\s*\[\d+\]\s*:", s):
            tier, cur = {"class": None, "name": None, "intervals": []}, {}
            continue
        if tier is None:
            continue
        if re.match(r"^(intervals|points)\s*\[\d+\]\s*:?", s):
            cur = {}
            continue
        m = _TG_ATTR.match(s)
        if not m:
            continue
        key, val = m[1], m[2]
        if key == "class":
            tier["class"] = _tg_string(val)
        elif key == "name":
            tier["name"] = _tg_string(val)
            if tier["class"] == "IntervalTier":
                if tier["name"] in tiers:
                    raise TextGridError("%s: two tiers named %r" % (path, tier["name"]))
                tiers[tier["name"]] = tier["intervals"]
        elif key in ("xmin", "xmax") and tier["name"] is not None:
            cur[key] = float(val)
        elif key == "text" and tier["class"] == "IntervalTier":
            if "xmin" not in cur or "xmax" not in cur:
                raise TextGridError("%s: interval text without xmin / xmax" % path)
            text = _tg_string(val)
            if text.strip() != "" or include_empty_intervals:
                tier["intervals"].append((cur["xmin"], cur["xmax"], text))
            cur = {}
    return tiers


def write_textgrid(path, tiers, xmax, encoding="utf-8"):
    """Interval tiers {name: [(start, end, text), ...]} (or a list of such pairs, in file order) -> a long-format
    TextGrid that `read_textgrid` reads back.  Every time is written with %r, the shortest text that gives the same
    float again, so two boundaries written from one float compare equal after reading (`get_alignment` matches a
    word's end to its last phone's with ==) and `round(t sampling_rate / hop)` of a time k hop / sampling_rate is k."""
    tiers = list(tiers.items()) if isinstance(tiers, dict) else list(tiers)
    xmax = float(xmax)
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", "xmax = %r" % xmax,
           "tiers? <exists>", "size = %d" % len(tiers), "item []:"]
    for t, (name, ivs) in enumerate(tiers, 1):
        out += ["    item [%d]:" % t, '        class = "IntervalTier"', '        name = "%s"' % name.replace('"', '""'),
                "        xmin = 0", "        xmax = %r" % xmax, "        intervals: size = %d" % len(ivs)]
        for j, (s, e, text) in enumerate(ivs, 1):
            if "\n" in text or "\r" in text:
                raise TextGridError("%s: an interval text with a line break: %r" % (path, text))
            out += ["        intervals [%d]:" % j, "            xmin = %r" % float(s), "            xmax = %r" % float(e),
                    '            text = "%s"' % text.replace('"', '""')]
    with open(path, "w", encoding=encoding) as f:
        f.write("\n".join(out) + "\n")


# ---------------------------------------------------------------------------------------------
# Host pieces of process_utterance / build_from_path
# ---------------------------------------------------------------------------------------------
def get_alignment(tier_p, tier_w, sampling_rate, hop_length):
    """preprocessor.py:395-452 on (start, end, text) intervals: (phones, durations, start, end, phones_per_word).
    Leading and trailing silences are trimmed, `spn` counts as a word of its own."""
    phones_per_word, phones, durations = [], [], []
    word_idx = phone_count = 0
    start_time = end_time = 0
    end_idx = 0
    for s, e, p in tier_p:
        if phones == []:
            if p in SIL_PHONES:
                if p == "spn":
                    word_idx += 1
                continue
            start_time = s
        phones.append(p)
        if p not in SIL_PHONES:
            end_time = e
            end_idx = len(phones)
            phone_count += 1
            if tier_w[word_idx][1] == e:
                phones_per_word.append(phone_count)
                phone_count = 0
                word_idx += 1
        else:
            phones_per_word.append(1)
            phone_count = 0
            if p == "spn":
                word_idx += 1
        durations.append(int(np.round(e * sampling_rate / hop_length) - np.round(s * sampling_rate / hop_length)))
    trim_len = len(phones[end_idx:])
    if trim_len:
        phones_per_word = phones_per_word[:-trim_len]
    phones, durations = phones[:end_idx], durations[:end_idx]
    if len(phones) != sum(phones_per_word):
        raise TextGridError("alignment: %d phones but the words hold %d" % (len(phones), sum(phones_per_word)))
    return phones, durations, start_time, end_time, phones_per_word


def word_level_subdivision(phones_per_word, max_phoneme_num):
    """utils/tools.py word_level_subdivision: words longer than max_phoneme_num are cut into pieces of that size."""
    res = []
    for n in phones_per_word:
        if n <= max_phoneme_num:
            res.append(n)
        else:
            s, r = divmod(n, max_phoneme_num)
            res += [max_phoneme_num] * s + ([r] if r else [])
    return res


def remove_outlier(values):
    """preprocessor.py:458-466: keep what lies strictly inside the 1.5 IQR fences."""
    values = np.array(values)
    p25, p75 = np.percentile(values, 25), np.percentile(values, 75)
    lower, upper = p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)
    return values[np.logical_and(values > lower, values < upper)]


class RunningMoments:
    """float64 count / mean / sum of squared deviations, merged chunk by chunk (Chan et al.); `std` is the population
    one, and 1.0 for a constant feature, as sklearn's StandardScaler.scale_ is.  mean and std are numpy float64
    scalars, so that normalising a float32 file gives a float64 one as it does in the reference."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0, np.float64(0.0), np.float64(0.0)

    def update(self, values):
        v = np.asarray(values, dtype=np.float64).ravel()
        if v.size == 0:
            return
        mean = v.mean()
        m2 = ((v - mean) ** 2).sum()
        if self.n == 0:
            self.n, self.mean, self.m2 = v.size, mean, m2
            return
        n = self.n + v.size
        delta = mean - self.mean
        self.m2 += m2 + delta * delta * self.n * v.size / n
        self.mean += delta * v.size / n
        self.n = n

    @property
    def std(self):
        if self.n == 0:
            raise ValueError("no values were seen")
        var = self.m2 / self.n
        eps = np.finfo(np.float64).eps
        if var <= self.n * eps * var + (self.n * self.mean * eps) ** 2:
            return np.float64(1.0)
        return np.sqrt(var)


def normalize(in_dir, mean, std):
    """preprocessor.py:468-479: rewrite every file of in_dir as (x - mean) / std; returns (min, max) over all."""
    max_value, min_value = np.finfo(np.float64).min, np.finfo(np.float64).max
    for filename in sorted(os.listdir(in_dir)):
        filename = os.path.join(in_dir, filename)
        values = (np.load(filename) - mean) / std
        np.save(filename, values)
        if len(values):
            max_value, min_value = max(max_value, values.max()), min(min_value, values.min())
    return min_value, max_value


def split_metadata(out, train, val, val_prior, val_size, sort_data, mel_frame_len):
    """preprocessor.py:233-248: shuffle under the caller's `random` seed, split off `val_size` lines (or honour the
    pre-defined validation names), sort by frame count when `sort_data`.  Returns (train, val); `out` is shuffled in
    place as the reference's is."""
    if val_prior is not None:
        assert len(out) == 0
        random.shuffle(train)
    else:
        assert len(train) == 0 and len(val) == 0
        random.shuffle(out)
        train, val = out[val_size:], out[:val_size]
    if sort_data:
        train.sort(key=lambda x: mel_frame_len[x.split("|")[0]])
        val.sort(key=lambda x: mel_frame_len[x.split("|")[0]])
    return train, val


def read_wav(path):
    """(rate, float32 mono samples) of a wav of any rate, read with scipy.io.wavfile: integer PCM scaled to [-1, 1),
    float taken as it is, channels averaged."""
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if x.dtype == np.uint8:
        x = (x.astype(np.float32) - 128.0) / 128.0
    elif np.issubdtype(x.dtype, np.integer):
        x = x.astype(np.float32) / float(2 ** (8 * x.dtype.itemsize - 1))
    else:
        x = x.astype(np.float32)
    return int(sr), (x.mean(axis=1) if x.ndim == 2 else x)


def scipy_load_wav(sampling_rate, resample=False, device="cuda"):
    """load_wav default: `read_wav`.  A file at another rate raises SamplingRateMismatch, or with `resample` goes
    through audio.resample on `device` (what the reference's librosa.load does silently)."""
    def load(path):
        sr, x = read_wav(path)
        if sr != sampling_rate:
            if not resample:
                raise SamplingRateMismatch("%s is sampled at %d Hz, the corpus is configured for %d Hz: run "
                                           "prepare_align first, pass resample=True, or pass load_wav="
                                           % (path, sr, sampling_rate))
            out, _ = Audio.resample(torch.from_numpy(np.ascontiguousarray(x)).to(device), sr, sampling_rate)
            x = out.cpu().numpy()
        return x
    return load


def pyworld_pitch(wav, sampling_rate, frame_period_ms):
    """pitch_fn default (preprocessor.py:295-300): pyworld dio + stonemask."""
    try:
        import pyworld as pw
    except ImportError as e:
        raise PitchExtractorRequired(
            "pitch extraction needs pyworld, which is not installed (%s): pass "
            "pitch_fn=callable(wav_float64, sampling_rate, frame_period_ms) -> f0 to Preprocessor" % e)
    pitch, t = pw.dio(wav, sampling_rate, frame_period=frame_period_ms)
    return pw.stonemask(wav, pitch, t, sampling_rate)


# ---------------------------------------------------------------------------------------------
# The builder
# ---------------------------------------------------------------------------------------------
class Preprocessor:
    def __init__(self, preprocess_config, model_config, train_config, pitch_fn=None, load_wav=None,
                 batch_utterances=16, device="cuda", resample=False):
        pp = preprocess_config["preprocessing"]
        self.preprocess_config = preprocess_config
        self.in_dir = preprocess_config["path"]["raw_path"]
        self.corpus_dir = preprocess_config["path"]["corpus_path"]
        self.out_dir = preprocess_config["path"]["preprocessed_path"]
        self.val_size = pp["val_size"]
        self.sampling_rate = pp["audio"]["sampling_rate"]
        self.hop_length = pp["stft"]["hop_length"]
        self.multi_speaker = model_config["multi_speaker"]
        self.sort_data = pp["sort_data"]
        self.sub_divide_word = pp["text"]["sub_divide_word"]
        self.max_phoneme_num = pp["text"]["max_phoneme_num"]
        self.beta_binomial_scaling_factor = pp["aligner"]["beta_binomial_scaling_factor"]
        assert pp["pitch"]["feature"] in ["phoneme_level", "frame_level"]
        assert pp["energy"]["feature"] in ["phoneme_level", "frame_level"]
        self.pitch_phoneme_averaging = pp["pitch"]["feature"] == "phoneme_level"
        self.energy_phoneme_averaging = pp["energy"]["feature"] == "phoneme_level"
        self.pitch_normalization = pp["pitch"]["normalization"]
        self.energy_normalization = pp["energy"]["normalization"]
        self.n_mel_channels = pp["mel"]["n_mel_channels"]
        self.STFT = Audio.TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"],
                                       pp["mel"]["n_mel_channels"], pp["audio"]["sampling_rate"],
                                       pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])
        self.val_prior = self.val_prior_names(os.path.join(self.out_dir, "val.txt"))
        self.native_pitch = isinstance(pitch_fn, str)
        if self.native_pitch:
            if pitch_fn != "native":
                raise ValueError("Preprocessor: pitch_fn must be a callable, None or \"native\", got %r" % (pitch_fn,))
            Pitch.pitch_geometry(self.sampling_rate)      # a rate the kernels do not take fails here, not mid-corpus
        self.pitch_fn = None if self.native_pitch else (pitch_fn or pyworld_pitch)
        self.batch_utterances = max(1, int(batch_utterances))
        self.device = torch.device(device)
        self.load_wav = load_wav or scipy_load_wav(self.sampling_rate, resample, self.device)
        self.speaker_emb = None
        self.in_sub_dirs = [p for p in sorted(os.listdir(self.in_dir)) if os.path.isdir(os.path.join(self.in_dir, p))]
        if self.multi_speaker and pp["speaker_embedder"] != "none":
            self.speaker_emb = PreDefinedEmbedder(preprocess_config)
            self.speaker_emb_dict = {spker: [] for spker in self.in_sub_dirs}

    def val_prior_names(self, val_prior_path):
        if not os.path.isfile(val_prior_path):
            return None
        print("Load pre-defined validation set...")
        with open(val_prior_path, "r", encoding="utf-8") as f:
            return list({m.split("|")[0] for m in f.readlines()})

    # ------------------------------------------------------------------ host stage of one utterance
    def _tg_path(self, speaker, basename):
        return os.path.join(self.out_dir, "TextGrid", speaker, "{}.TextGrid".format(basename))

    def prepare_utterance(self, speaker, basename, save_speaker_emb=False):
        """preprocessor.py:263-304: alignment, trimmed wav, raw text and f0.  None when the utterance is filtered out
        (empty alignment, or at most one voiced frame).  With pitch_fn="native" the item leaves without "pitch":
        `native_pitch_batch` adds it, and applies the voiced-frame rule, for the whole batch."""
        tiers = read_textgrid(self._tg_path(speaker, basename))
        for name in ("phones", "words"):
            if name not in tiers:
                raise TextGridError("%s: no interval tier named %r" % (self._tg_path(speaker, basename), name))
        phone, duration, start, end, phones_per_word = get_alignment(tiers["phones"], tiers["words"],
                                                                     self.sampling_rate, self.hop_length)
        if self.sub_divide_word:
            phones_per_word = word_level_subdivision(phones_per_word, self.max_phoneme_num)
        if start >= end:
            return None
        wav = np.asarray(self.load_wav(os.path.join(self.in_dir, speaker, "{}.wav".format(basename))))
        spker_embed = self.speaker_emb(wav) if save_speaker_emb else None
        wav = wav[int(self.sampling_rate * start):int(self.sampling_rate * end)].astype(np.float32)
        with open(os.path.join(self.in_dir, speaker, "{}.lab".format(basename)), "r") as f:
            raw_text = f.readline().strip("\n")
        pitch = None
        if not self.native_pitch:
            pitch = np.asarray(self.pitch_fn(wav.astype(np.float64), self.sampling_rate,
                                             self.hop_length / self.sampling_rate * 1000), dtype=np.float64)
            pitch = pitch[:sum(duration)]
            if np.sum(pitch != 0) <= 1:
                return None
        return {"speaker": speaker, "basename": basename, "text": "{" + " ".join(phone) + "}", "raw_text": raw_text,
                "duration": duration, "phones_per_word": phones_per_word, "wav": wav, "pitch": pitch,
                "spker_embed": spker_embed}

    # ------------------------------------------------------------------ device stage of a batch
    def _upload(self, items):
        """The batch's wavs, clipped to [-1, 1] and zero-padded to the longest: (device [B, max len], lengths)."""
        wav_len = np.array([len(it["wav"]) for it in items], dtype=np.int64)
        wavs = np.zeros((len(items), max(1, int(wav_len.max()))), dtype=np.float32)
        for b, it in enumerate(items):
            wavs[b, :wav_len[b]] = np.clip(it["wav"], -1, 1)
        return torch.from_numpy(wavs).to(self.device), wav_len

    def native_pitch_batch(self, items):
        """pitch_fn="native": F0 of every item of the batch in one launch pair, cut to sum(duration) as the host path
        cuts it.  Returns (kept items, dropped items, the kept rows of the upload): an item with at most one voiced
        frame is dropped, as prepare_utterance drops it on the host path."""
        wavs, wav_len = self._upload(items)
        f0, _ = Pitch.extract_f0(wavs, self.sampling_rate, self.hop_length, wav_len)
        f0 = f0.cpu().numpy()
        kept, dropped, rows = [], [], []
        for b, it in enumerate(items):
            pitch = f0[b, :min(Pitch.frame_count(int(wav_len[b]), self.hop_length), sum(it["duration"]))].copy()
            if np.sum(pitch != 0) <= 1:
                dropped.append(it)
                continue
            it["pitch"] = pitch
            kept.append(it)
            rows.append(b)
        if len(rows) != len(items):
            wavs = wavs[torch.tensor(rows, dtype=torch.long, device=wavs.device)] if rows else None
        return kept, dropped, wavs

    def process_batch(self, items, wavs=None):
        """preprocessor.py:306-382 for a list of prepare_utterance results: mel, energy, phoneme averages and prior on
        the GPU, the files, and per item (info line, kept pitch, kept energy, n frames, mel min, mel max).  wavs: the
        items' rows of `_upload`, when the caller holds them already."""
        dev, B = self.device, len(items)
        n_phon = np.array([len(it["duration"]) for it in items], dtype=np.int32)
        total = np.array([sum(it["duration"]) for it in items], dtype=np.int64)
        wav_len = np.array([len(it["wav"]) for it in items], dtype=np.int64)
        if wavs is None:
            wavs, _ = self._upload(items)
        if self.STFT.mel_basis.device != dev:
            self.STFT = self.STFT.to(dev)
        mel, energy = self.STFT.mel_spectrogram(wavs, wav_len)
        mel_len = np.minimum(total, 1 + wav_len // self.hop_length).astype(np.int32)
        L, T = int(mel_len.max()), int(n_phon.max())
        mel, energy = mel[:, :, :L], energy[:, :L].contiguous()
        dur = np.zeros((B, T), dtype=np.int32)
        for b, it in enumerate(items):
            dur[b, :n_phon[b]] = it["duration"]
        dur_d = torch.from_numpy(dur).to(dev)
        n_phon_d, mel_len_d = torch.from_numpy(n_phon).to(dev), torch.from_numpy(mel_len).to(dev)

        if self.energy_phoneme_averaging:
            energy = corpusops.phoneme_average(energy, dur_d, mel_len_d, n_phon_d, "energy")
        pitch_len = np.array([len(it["pitch"]) for it in items], dtype=np.int32)
        if self.pitch_phoneme_averaging:
            pitch = np.zeros((B, int(pitch_len.max())), dtype=np.float64)
            for b, it in enumerate(items):
                pitch[b, :pitch_len[b]] = it["pitch"]
            pitch = corpusops.phoneme_average(torch.from_numpy(pitch).to(dev), dur_d, torch.from_numpy(pitch_len).to(dev),
                                              n_phon_d, "pitch").cpu().numpy()
        prior = corpusops.attn_prior(n_phon_d, mel_len_d, T, L, self.beta_binomial_scaling_factor, torch.float64)
        # one device -> host copy per array kind
        mel_h = mel.transpose(1, 2).contiguous().cpu().numpy()      # [B, L, n_mels]
        energy_h, prior_h = energy.cpu().numpy(), prior.cpu().numpy()

        results = []
        for b, it in enumerate(items):
            speaker, basename, n, p = it["speaker"], it["basename"], int(mel_len[b]), int(n_phon[b])
            mel_b = np.ascontiguousarray(mel_h[b, :n])
            pitch_b = pitch[b, :p].copy() if self.pitch_phoneme_averaging else it["pitch"]
            energy_b = energy_h[b, :p if self.energy_phoneme_averaging else n].copy()
            self._save("mel", speaker, basename, mel_b)
            self._save("pitch", speaker, basename, pitch_b)
            self._save("energy", speaker, basename, energy_b)
            self._save("duration", speaker, basename, np.array(it["duration"]))
            self._save("phones_per_word", speaker, basename, np.array(it["phones_per_word"]))
            self._save("attn_prior", speaker, basename, np.ascontiguousarray(prior_h[b, :p, :n]))
            results.append(("|".join([basename, speaker, it["text"], it["raw_text"]]), remove_outlier(pitch_b),
                            remove_outlier(energy_b), n, mel_b.min(axis=0), mel_b.max(axis=0)))
        return results

    def _save(self, kind, speaker, basename, arr):
        np.save(os.path.join(self.out_dir, kind, "{}-{}-{}.npy".format(speaker, kind, basename)), arr)

    # ------------------------------------------------------------------ the whole corpus
    def build_from_path(self):
        for kind in ("mel", "pitch", "energy", "duration", "phones_per_word", "attn_prior", "spker_embed"):
            os.makedirs(os.path.join(self.out_dir, kind), exist_ok=True)
        embedding_dir = os.path.join(self.out_dir, "spker_embed")

        print("Processing Data ...")
        filtered_out = set()
        out, train, val = [], [], []
        n_frames, max_seq_len = 0, -float("inf")
        mel_frame_len_dict = {}
        mel_min = np.ones(self.n_mel_channels) * float("inf")
        mel_max = np.ones(self.n_mel_channels) * -float("inf")
        pitch_moments, energy_moments = RunningMoments(), RunningMoments()
        skip_speakers = {name.split("-")[0] for name in os.listdir(embedding_dir)}

        speakers = {}
        for i, speaker in enumerate(sorted(os.listdir(self.in_dir))):
            save_speaker_emb = self.speaker_emb is not None and speaker not in skip_speakers
            speakers[speaker] = i
            if not os.path.isdir(os.path.join(self.in_dir, speaker)):
                continue
            names = [w.split(".")[0] for w in sorted(os.listdir(os.path.join(self.in_dir, speaker))) if ".wav" in w]
            names = [n for n in names if os.path.exists(self._tg_path(speaker, n))]
            for k in range(0, len(names), self.batch_utterances):
                items = []
                for basename in names[k:k + self.batch_utterances]:
                    item = self.prepare_utterance(speaker, basename, save_speaker_emb)
                    if item is None:
                        filtered_out.add(basename)
                    else:
                        items.append(item)
                wavs = None
                if self.native_pitch and items:
                    items, dropped, wavs = self.native_pitch_batch(items)
                    filtered_out.update(it["basename"] for it in dropped)
                if not items:
                    continue
                for item, (info, pitch, energy, n, m_min, m_max) in zip(items, self.process_batch(items, wavs)):
                    basename = item["basename"]
                    if self.val_prior is not None:
                        (val if basename in self.val_prior else train).append(info)
                    else:
                        out.append(info)
                    pitch_moments.update(pitch)
                    energy_moments.update(energy)
                    if save_speaker_emb:
                        self.speaker_emb_dict[speaker].append(item["spker_embed"])
                    mel_min, mel_max = np.minimum(mel_min, m_min), np.maximum(mel_max, m_max)
                    max_seq_len = max(max_seq_len, n)
                    n_frames += n
                    mel_frame_len_dict[basename] = n
            if save_speaker_emb and self.speaker_emb_dict[speaker]:
                save_speaker_embeddings(self.out_dir, speaker, self.speaker_emb_dict[speaker])

        print("Computing statistic quantities ...")
        pitch_mean, pitch_std = (pitch_moments.mean, pitch_moments.std) if self.pitch_normalization else (0, 1)
        energy_mean, energy_std = (energy_moments.mean, energy_moments.std) if self.energy_normalization else (0, 1)
        pitch_min, pitch_max = normalize(os.path.join(self.out_dir, "pitch"), pitch_mean, pitch_std)
        energy_min, energy_max = normalize(os.path.join(self.out_dir, "energy"), energy_mean, energy_std)

        with open(os.path.join(self.out_dir, "speakers.json"), "w") as f:
            f.write(json.dumps(speakers))
        with open(os.path.join(self.out_dir, "stats.json"), "w") as f:
            f.write(json.dumps({
                "pitch": [float(pitch_min), float(pitch_max), float(pitch_mean), float(pitch_std)],
                "energy": [float(energy_min), float(energy_max), float(energy_mean), float(energy_std)],
                "spec_min": mel_min.tolist(),
                "spec_max": mel_max.tolist(),
                "max_seq_len": max_seq_len,
            }))
        print("Total time: {} hours".format(n_frames * self.hop_length / self.sampling_rate / 3600))

        train, val = split_metadata(out, train, val, self.val_prior, self.val_size, self.sort_data,
                                    mel_frame_len_dict)
        for name, lines in (("train.txt", train), ("val.txt", val), ("filtered_out.txt", sorted(filtered_out))):
            with open(os.path.join(self.out_dir, name), "w", encoding="utf-8") as f:
                for m in lines:
                    f.write(str(m) + "\n")
        return out
