"""The tiny synthetic corpus of the corpus-builder tests: a seeded recipe that tests/golden/make_golden_preprocessor.py
runs the reference Preprocessor over, and that the tests replay for the native one.  Two speakers, seven utterances
of 0.3 - 0.6 s at 22.05 kHz.  Pure numpy; reads nothing outside the directory it is told to write."""
import os

import numpy as np

SR, HOP, N_FFT, WIN, N_MELS = 22050, 256, 1024, 1024, 80
MAX_PHONEME_NUM = 7
VAL_SIZE = 2
SHUFFLE_SEED = 1234

# name, speaker, f0 kind, phones [(start, end, text)], words [(start, end, text)], total seconds.  An empty text is
# written to the TextGrid and dropped by the reader.
UTTERANCES = [
    # plain: leading / trailing sil, an sp between two words
    ("a01", "spkA", "voiced", [
        (0.0, 0.05, "sil"), (0.05, 0.11, "HH"), (0.11, 0.17, "AH0"), (0.17, 0.22, "L"), (0.22, 0.31, "OW1"),
        (0.31, 0.34, "sp"), (0.34, 0.39, "W"), (0.39, 0.47, "ER1"), (0.47, 0.51, "L"), (0.51, 0.56, "D"),
        (0.56, 0.6, "sil")],
     [(0.0, 0.05, ""), (0.05, 0.31, "hello"), (0.31, 0.34, ""), (0.34, 0.56, "world"), (0.56, 0.6, "")], 0.6),
    # two phones shorter than half a frame first: durations [0, 0, ...], so the in-place averaging of the third
    # segment reads entries 0 and 1 after they were overwritten
    ("a02", "spkA", "voiced", [
        (0.0, 0.048, "sil"), (0.048, 0.05, "T"), (0.05, 0.052, "AH0"), (0.052, 0.15, "M"), (0.15, 0.24, "AA1"),
        (0.24, 0.3, "T"), (0.3, 0.38, "OW2"), (0.38, 0.45, "")],
     [(0.0, 0.048, ""), (0.048, 0.38, "tomato"), (0.38, 0.45, "")], 0.45),
    # spn (a word of its own) and sp inside
    ("a03", "spkA", "voiced", [
        (0.0, 0.04, "sil"), (0.04, 0.1, "DH"), (0.1, 0.16, "AH0"), (0.16, 0.27, "spn"), (0.27, 0.3, "sp"),
        (0.3, 0.37, "K"), (0.37, 0.46, "AE1"), (0.46, 0.52, "T"), (0.52, 0.55, "sil")],
     [(0.0, 0.04, ""), (0.04, 0.16, "the"), (0.16, 0.27, "<unk>"), (0.27, 0.3, ""), (0.3, 0.52, "cat"),
      (0.52, 0.55, "")], 0.55),
    # at most one voiced frame: filtered out
    ("b01", "spkB", "unvoiced", [
        (0.0, 0.03, "sil"), (0.03, 0.12, "S"), (0.12, 0.2, "IH1"), (0.2, 0.3, "T"), (0.3, 0.35, "sil")],
     [(0.0, 0.03, ""), (0.03, 0.3, "sit"), (0.3, 0.35, "")], 0.35),
    # a nine-phone word: cut into 7 + 2
    ("b02", "spkB", "voiced", [
        (0.0, 0.02, "sil"), (0.02, 0.07, "IH0"), (0.07, 0.12, "K"), (0.12, 0.17, "S"), (0.17, 0.22, "T"),
        (0.22, 0.27, "R"), (0.27, 0.33, "AE1"), (0.33, 0.38, "V"), (0.38, 0.43, "AH0"), (0.43, 0.5, "G"),
        (0.5, 0.54, "AH0"), (0.54, 0.58, "N"), (0.58, 0.6, "sil")],
     [(0.0, 0.02, ""), (0.02, 0.5, "extravag"), (0.5, 0.58, "un"), (0.58, 0.6, "")], 0.6),
    # trailing sp + sil are trimmed
    ("b03", "spkB", "voiced", [
        (0.0, 0.06, "sil"), (0.06, 0.14, "G"), (0.14, 0.25, "OW1"), (0.25, 0.29, "sp"), (0.29, 0.35, "sil")],
     [(0.0, 0.06, ""), (0.06, 0.25, "go"), (0.25, 0.35, "")], 0.35),
    # a leading spn is trimmed and skips its word
    ("b04", "spkB", "voiced", [
        (0.0, 0.03, "sil"), (0.03, 0.09, "spn"), (0.09, 0.17, "R"), (0.17, 0.29, "EH1"), (0.29, 0.36, "D"),
        (0.36, 0.41, "IY0"), (0.41, 0.47, "sil")],
     [(0.0, 0.03, ""), (0.03, 0.09, "<unk>"), (0.09, 0.41, "ready"), (0.41, 0.47, "")], 0.47),
]
NAMES = [u[0] for u in UTTERANCES]
SPEAKER_OF = {u[0]: u[1] for u in UTTERANCES}
FILTERED = ["b01"]
ALIASED = "a02"


def signal(name):
    """The utterance's whole signal (float32 in [-1, 1]): a chirp with harmonics, tremolo and noise."""
    k = NAMES.index(name)
    n = int(round(UTTERANCES[k][5] * SR))
    rng = np.random.default_rng(500 + k)
    t = np.arange(n) / SR
    f0 = 90.0 + 25.0 * k + (2500.0 - 90.0) * t / t[-1] / 2
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = 0.5 * np.sin(ph) + 0.2 * np.sin(2 * ph + 0.3) + 0.1 * np.sin(3 * ph + 1.1)
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 5.0 * t)) + 0.05 * rng.standard_normal(n)
    return np.clip(x, -1, 1).astype(np.float32)


def load_wav(path):
    """load_wav for the builder (and what the stubbed librosa.load returns): the seeded signal of the file's name."""
    return signal(os.path.basename(path).split(".")[0])


def _trimmed_len(u):
    ph = [p for p in u[3] if p[2] != ""]
    sil = ("sil", "sp", "spn")
    first = next(i for i, p in enumerate(ph) if p[2] not in sil)
    last = max(i for i, p in enumerate(ph) if p[2] not in sil)
    return int(SR * ph[last][1]) - int(SR * ph[first][0])


KIND_BY_LEN = {_trimmed_len(u): (k, u[2]) for k, u in enumerate(UTTERANCES)}
assert len(KIND_BY_LEN) == len(UTTERANCES), "trimmed lengths must be unique: pitch_fn tells the utterances by them"


def pitch_fn(wav, sr, frame_period_ms):
    """Seeded f0 track for a trimmed signal: 1 + len // hop frames, unvoiced (0) runs at the start, in the middle and
    at the end; the 'unvoiced' utterance keeps a single voiced frame."""
    assert wav.dtype == np.float64 and sr == SR and abs(frame_period_ms - HOP / SR * 1000) < 1e-9
    k, kind = KIND_BY_LEN[len(wav)]
    n = 1 + len(wav) // HOP
    rng = np.random.default_rng(900 + k)
    t = np.arange(n)
    f0 = 110.0 + 12.0 * k + 35.0 * np.sin(2 * np.pi * t / 17.0 + 0.4 * k) + 3.0 * rng.standard_normal(n)
    f0[:2 + k % 3] = 0.0
    mid = n // 2 + (k % 2)
    f0[mid:mid + 3 + k % 2] = 0.0
    f0[n - (1 + k % 3):] = 0.0
    if kind == "unvoiced":
        keep = f0[5]
        f0[:] = 0.0
        f0[5] = keep
    return f0


def textgrid_text(u):
    """The utterance's TextGrid in Praat's long text format, empty intervals included."""
    name, _, _, phones, words, total = u
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", "xmax = %r" % total,
           "tiers? <exists>", "size = 2", "item []:"]
    for t, (tier, ivs) in enumerate((("words", words), ("phones", phones)), 1):
        out += ["    item [%d]:" % t, '        class = "IntervalTier"', '        name = "%s"' % tier,
                "        xmin = 0", "        xmax = %r" % total, "        intervals: size = %d" % len(ivs)]
        for j, (s, e, text) in enumerate(ivs, 1):
            out += ["        intervals [%d]:" % j, "            xmin = %r" % s, "            xmax = %r" % e,
                    '            text = "%s"' % text.replace('"', '""')]
    return "\n".join(out) + "\n"


def write_corpus(root):
    """raw_data/<spk>/<name>.{wav,lab} and preprocessed/TextGrid/<spk>/<name>.TextGrid under root; returns
    (raw_path, preprocessed_path).  The wav files are 16-bit PCM of the seeded signals."""
    from scipy.io import wavfile
    raw, pre = os.path.join(root, "raw_data"), os.path.join(root, "preprocessed")
    for u in UTTERANCES:
        name, spk = u[0], u[1]
        os.makedirs(os.path.join(raw, spk), exist_ok=True)
        os.makedirs(os.path.join(pre, "TextGrid", spk), exist_ok=True)
        wavfile.write(os.path.join(raw, spk, name + ".wav"), SR, np.round(signal(name) * 32767).astype(np.int16))
        with open(os.path.join(raw, spk, name + ".lab"), "w") as f:
            f.write(" ".join(w[2] for w in u[4] if w[2]) + "\n")
        with open(os.path.join(pre, "TextGrid", spk, name + ".TextGrid"), "w", encoding="utf-8") as f:
            f.write(textgrid_text(u))
    return raw, pre


def configs(raw, pre, feature="phoneme_level", normalization=True):
    """(preprocess_config, model_config, train_config) with the reference's LJSpeech preprocessing values."""
    preprocess = {
        "dataset": "Synth",
        "path": {"corpus_path": os.path.join(os.path.dirname(raw), "corpus"), "lexicon_path": "", "raw_path": raw,
                 "preprocessed_path": pre},
        "preprocessing": {
            "sort_data": True, "val_size": VAL_SIZE, "speaker_embedder": "none",
            "text": {"text_cleaners": ["english_cleaners"], "language": "en", "sub_divide_word": True,
                     "max_phoneme_num": MAX_PHONEME_NUM},
            "audio": {"sampling_rate": SR, "max_wav_value": 32768.0},
            "stft": {"filter_length": N_FFT, "hop_length": HOP, "win_length": WIN},
            "mel": {"n_mel_channels": N_MELS, "mel_fmin": 0, "mel_fmax": 8000},
            "pitch": {"feature": feature, "normalization": normalization},
            "energy": {"feature": feature, "normalization": normalization},
            "aligner": {"beta_binomial_scaling_factor": 1.0},
        },
    }
    return preprocess, {"multi_speaker": False}, {"optimizer": {"batch_size": 4, "batch_size_shallow": 4}}


KINDS = ("mel", "pitch", "energy", "duration", "phones_per_word", "attn_prior")
# (mel_len, n_phonemes, scaling) of the stored beta_binomial_prior_distribution tables, and the strides of the sub-grid
# kept of the large ones
PRIOR_CASES = [(37, 5, 1.0), (800, 100, 1.0), (613, 87, 0.5), (3, 1, 1.0)]
PRIOR_ROW_STEP, PRIOR_COL_STEP = 3, 5


def prior_subgrid(mel_len, n_phon):
    """Row and column indices kept of a [n_phon, mel_len] table: all of a small one, a strided grid plus the last row
    and column of a large one."""
    if n_phon * mel_len <= 4096:
        return np.arange(n_phon), np.arange(mel_len)
    rows = np.unique(np.concatenate([np.arange(0, n_phon, PRIOR_ROW_STEP), [n_phon - 1]]))
    cols = np.unique(np.concatenate([np.arange(0, mel_len, PRIOR_COL_STEP), [mel_len - 1]]))
    return rows, cols
