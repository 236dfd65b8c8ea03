"""The synthetic corpus of the forced-aligner tests: a seeded recipe of utterances whose phone boundaries are known to
the sample.  Twelve utterances of 0.6 - 1.2 s at 22.05 kHz; ten phones, each a stationary sum of three sinusoids at
its own frequencies over noise; silence is the noise alone.  Every phone lasts at least four frames and its
boundaries fall anywhere between frame centres.  One word of the transcripts is missing from the lexicon (-> spn);
one utterance has a real pause between two words, no other has any.  Pure numpy; writes only where it is told to."""
import os

import numpy as np

SR, HOP, N_FFT, WIN, N_MELS, FMIN, FMAX = 22050, 256, 1024, 1024, 80, 0, 8000
# the noise floor sits about 20 dB under a partial in its mel band: what a window leaks across a boundary from a frame
# away (9 % of the amplitude) drowns in it, so only the frame on the boundary is a mixture
NOISE, TONE = 0.05, 0.12

# three partials per phone, harmonics of the phone's own fundamental (so that a pitch extractor finds it voiced) and
# well apart from the other phones' on the mel axis: (fundamental in Hz, harmonic numbers)
PHONES = {
    "a": (155.0, (2, 8, 19)), "e": (150.0, (3, 13, 23)), "i": (125.0, (2, 18, 31)), "o": (130.0, (4, 7, 20)),
    "u": (100.0, (2, 7, 21)), "k": (250.0, (6, 17, 24)), "s": (260.0, (12, 20, 27)), "t": (235.0, (11, 20, 28)),
    "m": (150.0, (1, 7, 11)), "n": (190.0, (2, 8, 23)),
}
UNKNOWN_SOUND = (200.0, (3, 18, 29))      # what the out-of-lexicon word sounds like
# every phone meets several different neighbours: a phone that always precedes the same one cannot be told from it
_WORDS = "kato semi nuki tasu mone ika sano ame toki nesu ota umi eki uso inu ate oku kesa mito sune"
LEXICON = {w: list(w) for w in _WORDS.split()}
LEXICON["KATO"] = ["s", "s", "s"]      # the first entry of a word wins, and the lookup is lower-cased
OOV = "zorb"
# name, words, index of the word a real pause follows (or None)
UTTERANCES = [
    ("u01", ["kato", "semi"], None), ("u02", ["nuki", "tasu", "ika"], None), ("u03", ["mone", OOV, "ame"], None),
    ("u04", ["sano", "toki"], 0), ("u05", ["nesu", "ota", "umi"], None), ("u06", ["Semi", "eki"], None),
    ("u07", ["uso", "inu", "ate"], None), ("u08", ["oku", OOV, "umi"], None), ("u09", ["kesa", "mito", "sune"], None),
    ("u10", ["tasu", "kato"], None), ("u11", ["mone", "ika", "toki"], None), ("u12", ["nesu", "sano", "nuki"], None),
]
NAMES = [u[0] for u in UTTERANCES]
SPEAKER = "spk"
PAUSED, WITH_OOV = "u04", ("u03", "u08")


def _plan(k):
    """Segments of utterance k as (phone or 'sil' / 'sp' / 'spn', n samples, word index or -1), seeded."""
    name, words, pause_after = UTTERANCES[k]
    rng = np.random.default_rng(4100 + k)
    n_ph = sum(len(LEXICON.get(w.lower(), [None] * 2)) for w in words)
    lo, hi = (4 * HOP + 8, 6 * HOP) if n_ph >= 10 else (5 * HOP, 9 * HOP)
    segs = [("sil", int(rng.integers(5 * HOP, 9 * HOP)), -1)]
    for w, word in enumerate(words):
        phones = LEXICON.get(word.lower())
        if phones is None:
            segs.append(("spn", int(rng.integers(10 * HOP, 14 * HOP)), w))
        else:
            segs += [(p, int(rng.integers(lo, hi)), w) for p in phones]
        if pause_after == w:
            segs.append(("sp", int(rng.integers(8 * HOP, 11 * HOP)), -1))
    segs.append(("sil", int(rng.integers(5 * HOP, 9 * HOP)), -1))
    return segs


def signal(name, noise=NOISE):
    """float32 signal of the utterance: every segment a stationary tone complex (phase continuous inside it), over
    noise that runs through the whole file.  noise: its standard deviation, for a quieter rendering of the same
    utterance (same boundaries, same tones)."""
    k = NAMES.index(name)
    segs = _plan(k)
    rng = np.random.default_rng(7300 + k)
    x = noise * rng.standard_normal(sum(n for _, n, _ in segs))
    pos = 0
    for phone, n, _ in segs:
        sound = UNKNOWN_SOUND if phone == "spn" else PHONES.get(phone)
        if sound:
            t = np.arange(n) / SR
            for j, h in enumerate(sound[1]):
                x[pos:pos + n] += TONE / (1 + j) * np.sin(2 * np.pi * sound[0] * h * t + 0.7 * j)
        pos += n
    return x.astype(np.float32)


def truth(name):
    """(phones, words) tiers of the utterance as (start, end, text) in seconds, and its length in samples."""
    segs = _plan(NAMES.index(name))
    words_txt = UTTERANCES[NAMES.index(name)][1]
    phones, words, pos = [], [], 0
    for phone, n, w in segs:
        s, e = pos / SR, (pos + n) / SR
        phones.append((s, e, phone))
        text = "" if w < 0 else ("<unk>" if phone == "spn" else words_txt[w])
        if words and w >= 0 and words[-1][3] == w:
            words[-1] = (words[-1][0], e, text, w)
        else:
            words.append((s, e, text, w))
        pos += n
    return phones, [w[:3] for w in words], pos


def lexicon():
    """LEXICON as a reader of its file sees it: lower-cased words, the first entry of a word wins."""
    out = {}
    for w, ph in LEXICON.items():
        out.setdefault(w.lower(), ph)
    return out


def load_wav(path):
    return signal(os.path.basename(path).split(".")[0])


def load_wav_quiet(path):
    """The same utterances with a tenth of the noise.  At NOISE a pitch extractor rightly calls every frame unvoiced
    (the noise is a fifth of the power); a stage that needs voiced frames reads this rendering."""
    return signal(os.path.basename(path).split(".")[0], NOISE / 10)


def write_lexicon(path):
    with open(path, "w", encoding="utf-8") as f:
        for w, ph in LEXICON.items():
            f.write("%s %s\n" % (w, " ".join(ph)))
    return path


def write_corpus(root):
    """raw_data/spk/<name>.{wav,lab} and lexicon.txt under root; returns (raw_path, preprocessed_path, lexicon_path)."""
    from scipy.io import wavfile
    raw, pre = os.path.join(root, "raw_data"), os.path.join(root, "preprocessed")
    os.makedirs(os.path.join(raw, SPEAKER), exist_ok=True)
    os.makedirs(pre, exist_ok=True)
    for name, words, _ in UTTERANCES:
        wavfile.write(os.path.join(raw, SPEAKER, name + ".wav"), SR, np.round(signal(name) * 32767).astype(np.int16))
        with open(os.path.join(raw, SPEAKER, name + ".lab"), "w") as f:
            f.write(" ".join(words) + "\n")
    return raw, pre, write_lexicon(os.path.join(root, "lexicon.txt"))


def configs(raw, pre, lexicon_path):
    """(preprocess_config, model_config, train_config), as tests/preprocessor_corpus.py builds them."""
    preprocess = {
        "dataset": "Synth",
        "path": {"corpus_path": os.path.join(os.path.dirname(raw), "corpus"), "lexicon_path": lexicon_path,
                 "raw_path": raw, "preprocessed_path": pre},
        "preprocessing": {
            "sort_data": True, "val_size": 2, "speaker_embedder": "none",
            "text": {"text_cleaners": [], "language": "en", "sub_divide_word": True, "max_phoneme_num": 7},
            "audio": {"sampling_rate": SR, "max_wav_value": 32768.0},
            "stft": {"filter_length": N_FFT, "hop_length": HOP, "win_length": WIN},
            "mel": {"n_mel_channels": N_MELS, "mel_fmin": FMIN, "mel_fmax": FMAX},
            "pitch": {"feature": "phoneme_level", "normalization": True},
            "energy": {"feature": "phoneme_level", "normalization": True},
            "aligner": {"beta_binomial_scaling_factor": 1.0},
        },
    }
    return preprocess, {"multi_speaker": False}, {"optimizer": {"batch_size": 4, "batch_size_shallow": 4}}
