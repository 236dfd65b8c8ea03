"""Raw corpus -> raw_data (reference prepare_align.py, preprocessor/ljspeech.py, preprocessor/aishell3.py): every wav
resampled to `preprocessing.audio.sampling_rate`, peak-normalised and written as int16 to
`raw_path/<speaker>/<name>.wav`, with the transcript the aligner and the corpus builder read beside it as `<name>.lab`.

Same corpus layouts, output names and text rules as the reference.  The arithmetic runs on the GPU
(csrc/resample.hip through audio.resample and audio.peak_normalize_int16): the files of a batch are grouped by source
rate, and each group is one resample launch, one normalisation launch and one device -> host copy.

Injected, as `text_to_sequence` is in data.py: `clean_text(text, cleaner_names) -> text`, the reference's
`text._clean_text`.  LJSpeech applies it to the transcript; with cleaners configured and no function given,
CleanTextRequired names the argument.  AISHELL3 needs none.

Deviations from the reference:
- wavs are read with scipy.io.wavfile (integer PCM scaled to [-1, 1), channels averaged), not librosa's audioread;
- the resampler is the Kaiser-windowed sinc of audio.resample_filter, not librosa's stored table (audio.py);
- the int16 conversion saturates: the loudest positive sample is 32767, where the reference's 32768.0 wraps to -32768;
- an all-zero wav is written as zeros (the reference divides by zero);
- a wav is written only after its whole batch has been converted, so an interrupted run leaves whole files.
"""
import os

import numpy as np
import torch

from . import audio as Audio
from ._lib import MixganHipError
from .preprocessor import read_wav


class CleanTextRequired(MixganHipError, ValueError):
    """Text cleaners are configured and no clean_text function was given."""


def convert_group(wavs, orig_sr, target_sr, max_wav_value, device):
    """The device stage of one group of float32 wavs of one rate: list of int16 arrays at target_sr.  One resample
    launch, one normalisation launch, one device -> host copy."""
    lens = np.array([len(w) for w in wavs], dtype=np.int64)
    batch = np.zeros((len(wavs), max(1, int(lens.max()))), dtype=np.float32)
    for b, w in enumerate(wavs):
        batch[b, :lens[b]] = w
    out, out_lens = Audio.resample(torch.from_numpy(batch).to(device), orig_sr, target_sr, lens)
    q = Audio.peak_normalize_int16(out, out_lens, max_wav_value).cpu().numpy()
    up, down = Audio.resample_ratio(orig_sr, target_sr)
    return [q[b, :-(-int(lens[b]) * up // down)].copy() for b in range(len(wavs))]


def _convert(entries, sampling_rate, max_wav_value, batch_utterances, device):
    """entries: (wav_path, out_wav_path, lab_path, text) of existing wavs.  Converts and writes them batch by batch."""
    from scipy.io import wavfile
    batch_utterances = max(1, int(batch_utterances))
    batch = []

    def flush():
        loaded = [read_wav(e[0]) for e in batch]
        results = [None] * len(batch)
        for sr in sorted({sr for sr, _ in loaded}):
            idx = [i for i, (s, _) in enumerate(loaded) if s == sr]
            for i, q in zip(idx, convert_group([loaded[i][1] for i in idx], sr, sampling_rate, max_wav_value, device)):
                results[i] = q
        for (_, out_wav, lab, text), q in zip(batch, results):
            os.makedirs(os.path.dirname(out_wav), exist_ok=True)
            wavfile.write(out_wav, sampling_rate, q)
            with open(lab, "w") as f:
                f.write(text)
        del batch[:]

    n = 0
    for e in entries:
        batch.append(e)
        n += 1
        if len(batch) == batch_utterances:
            flush()
    if batch:
        flush()
    return n


def ljspeech(config, clean_text=None, batch_utterances=16, device="cuda"):
    """preprocessor/ljspeech.py: `corpus_path/metadata.csv` lines `name|text|normalised text`, wavs under
    `corpus_path/wavs/`; everything goes to the speaker "LJSpeech".  Returns the number of wavs written."""
    in_dir, out_dir = config["path"]["corpus_path"], config["path"]["raw_path"]
    audio_cfg = config["preprocessing"]["audio"]
    cleaners = config["preprocessing"]["text"]["text_cleaners"]
    if clean_text is None and cleaners:
        raise CleanTextRequired("prepare_align: the config asks for the text cleaners %r: pass "
                                "clean_text=callable(text, cleaner_names) -> text (the reference's text._clean_text)"
                                % (cleaners,))
    speaker = "LJSpeech"

    def entries():
        with open(os.path.join(in_dir, "metadata.csv"), encoding="utf-8") as f:
            for line in f:
                parts = line.strip().split("|")
                base_name, text = parts[0], parts[2]
                if clean_text is not None:
                    text = clean_text(text, cleaners)
                wav_path = os.path.join(in_dir, "wavs", "{}.wav".format(base_name))
                if os.path.exists(wav_path):
                    yield (wav_path, os.path.join(out_dir, speaker, "{}.wav".format(base_name)),
                           os.path.join(out_dir, speaker, "{}.lab".format(base_name)), text)

    return _convert(entries(), audio_cfg["sampling_rate"], audio_cfg["max_wav_value"], batch_utterances, device)


def aishell3(config, batch_utterances=16, device="cuda"):
    """preprocessor/aishell3.py: `corpus_path/{train,test}/content.txt` lines `wav name<TAB>char pinyin char pinyin ..`,
    wavs under `corpus_path/<set>/wav/<speaker>/`.  The speaker is the first 7 characters of the wav name, the lab
    name its first 11, the text every second token.  Returns the number of wavs written."""
    in_dir, out_dir = config["path"]["corpus_path"], config["path"]["raw_path"]
    audio_cfg = config["preprocessing"]["audio"]

    def entries():
        for dataset in ["train", "test"]:
            print("Processing {}ing set...".format(dataset))
            with open(os.path.join(in_dir, dataset, "content.txt"), encoding="utf-8") as f:
                for line in f:
                    wav_name, text = line.strip("\n").split("\t")
                    speaker = wav_name[:7]
                    text = text.split(" ")[1::2]
                    wav_path = os.path.join(in_dir, dataset, "wav", speaker, wav_name)
                    if os.path.exists(wav_path):
                        yield (wav_path, os.path.join(out_dir, speaker, wav_name),
                               os.path.join(out_dir, speaker, "{}.lab".format(wav_name[:11])), " ".join(text))

    return _convert(entries(), audio_cfg["sampling_rate"], audio_cfg["max_wav_value"], batch_utterances, device)


def prepare_align(config, clean_text=None, batch_utterances=16, device="cuda"):
    """prepare_align.py main(config): dispatch on config["dataset"]."""
    if "LJSpeech" in config["dataset"]:
        ljspeech(config, clean_text, batch_utterances, device)
    if "AISHELL3" in config["dataset"]:
        aishell3(config, batch_utterances, device)
