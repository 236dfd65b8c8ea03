"""Native forced aligner (csrc/align.hip): raw_data wavs and `.lab` transcripts -> the TextGrids the corpus builder
reads, without the Montreal Forced Aligner.

This is an algorithm of this project's own, not a port, and no parity with MFA's alignments is claimed: MFA remains
the way to get MFA's alignments.  What it keeps is the contract `read_textgrid` / `get_alignment` / `Preprocessor`
consume: a long-format TextGrid with a `words` and a `phones` tier, `sil` / `sp` / `spn` for silence and unknown
words, and boundaries that fall on frame starts.

The acoustic model is a monophone, left-to-right HMM with one diagonal Gaussian per state, flat-started and trained by
Viterbi (hard) EM on the corpus it aligns: no SGD, no random initialisation, no atomics, so a fit of the same items
in the same order is reproducible bit for bit.  The stages (tests/align_oracle.py restates them in float64 numpy):
1. features: the log-mel of `TacotronSTFT.mel_spectrogram` minus the utterance's mean over its own frames,
   T = len // hop + 1 frames of D = n_mel_channels values, zero past them;
2. state sequence: every word's phones from the lexicon (an unknown word is the phone `spn`, word text `<unk>`),
   `states_per_phone` states a phone, and one skippable `sil` state before the first word, between every two words and
   after the last;
3. flat start: uniform segmentation, then at most `n_iters` rounds of statistics -> model -> emissions -> Viterbi,
   ending early when no duration changed (`converged`); the default of 8 is a cap that bounds the cost of a large
   corpus, and the synthetic corpus of the tests needs 14 rounds to reach its fixed point;
4. model update in float64 on the host from the kernel's float64 sums; a Gaussian with fewer than `min_count` frames
   takes the global mean and variance;
5. output: state durations summed to phones.

Time convention: frame k of the features is centred on sample k hop, and a state whose first frame is k is written as
starting at k hop / sr, half a frame before the centre of its first frame.  The first interval starts at 0 and the
last ends at n_samples / sr.  `round(t sr / hop)` of every boundary but the last is its frame index, so the
durations `get_alignment` derives are the aligner's frame counts.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from . import audio as Audio
from ._lib import fptr, iptr, check, stream_ptr, MixganHipError

MAX_D, MAX_G, MAX_S, MAX_T = _lib.MG_ALIGN_MAX_D, _lib.MG_ALIGN_MAX_G, _lib.MG_ALIGN_MAX_S, _lib.MG_ALIGN_MAX_T
SIL, SP, SPN, UNK = "sil", "sp", "spn", "<unk>"
_PUNCT = ".,!?;:\"()[]{}<>"


class AlignGeometryError(MixganHipError, NotImplementedError):
    """A shape the alignment kernels do not take."""


def _geometry(rc_ok, message):
    if not rc_ok:
        raise AlignGeometryError("align: %s (%s)" % (message, _lib.lib().mg_error_string(_lib.MG_ERR_SHAPE).decode()))


def _dev(t, what, dtype):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise MixganHipError("align: %s must be a CUDA tensor: the HIP path has no CPU fallback" % what)
    return t.to(dtype).contiguous()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------
# The three kernel calls
# ---------------------------------------------------------------------------------------------
def emissions(x, n_frames, A, Bm, c):
    """x [B, T, D], n_frames int [B], A, Bm [G, D], c [G] on the device -> ll float32 [B, T, G]:
    ll[b, t, g] = sum_d (A x^2 + Bm x) + c for t < n_frames[b], 0 elsewhere."""
    for t, what in ((x, "x"), (n_frames, "n_frames"), (A, "A"), (Bm, "Bm"), (c, "c")):
        if not isinstance(t, torch.Tensor):
            raise MixganHipError("align: %s must be a CUDA tensor: the HIP path has no CPU fallback" % what)
    if x.dim() != 3 or A.dim() != 2 or A.shape[1] != x.shape[2] or Bm.shape != A.shape or c.shape != A.shape[:1] \
            or n_frames.shape != x.shape[:1]:
        raise ValueError("emissions: expected x [B, T, D], n_frames [B], A and Bm [G, D] and c [G], got %s, %s, %s, %s "
                         "and %s" % (tuple(x.shape), tuple(n_frames.shape), tuple(A.shape), tuple(Bm.shape),
                                     tuple(c.shape)))
    B, T, D = x.shape
    G = A.shape[0]
    _geometry(B >= 1 and T >= 1 and 1 <= D <= MAX_D and 1 <= G <= MAX_G and B * T <= 65535 * 64,
              "emissions take 1 <= D <= %d features and 1 <= G <= %d Gaussians over at least one frame, got B=%d T=%d "
              "D=%d G=%d" % (MAX_D, MAX_G, B, T, D, G))
    x, A, Bm, c = (_dev(t, n, torch.float32) for t, n in ((x, "x"), (A, "A"), (Bm, "Bm"), (c, "c")))
    n_frames = _dev(n_frames, "n_frames", torch.int32)
    ll = torch.empty(B, T, G, device=x.device, dtype=torch.float32)
    check(_lib.lib().mg_align_emissions(fptr(x), iptr(n_frames, torch.int32), B, T, D, fptr(A), fptr(Bm), fptr(c), G,
                                        fptr(ll), stream_ptr()))
    return ll


def viterbi_align(ll, seq, skip, n_frames, n_states):
    """ll float32 [B, T, G] on the device; seq int [B, S], skip bool [B, S], n_frames and n_states int [B], numpy or
    tensors -> (durations int32 [B, S], score float64 [B], ok int32 [B]) on the device.  A skippable state must have
    non-skippable neighbours inside its row: two adjacent ones raise AlignGeometryError here, on the host."""
    if not isinstance(ll, torch.Tensor):
        raise MixganHipError("align: ll must be a CUDA tensor: the HIP path has no CPU fallback")
    host = [np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a) for a in (seq, skip, n_frames, n_states)]
    seq_h, skip_h, nf_h, ns_h = host[0].astype(np.int32), host[1].astype(np.uint8), host[2].astype(np.int32), \
        host[3].astype(np.int32)
    if ll.dim() != 3 or seq_h.ndim != 2 or skip_h.shape != seq_h.shape or nf_h.shape != ll.shape[:1] \
            or ns_h.shape != ll.shape[:1] or seq_h.shape[0] != ll.shape[0]:
        raise ValueError("viterbi_align: expected ll [B, T, G], seq and skip [B, S], n_frames and n_states [B], got %s, "
                         "%s, %s, %s and %s" % (tuple(ll.shape), seq_h.shape, skip_h.shape, nf_h.shape, ns_h.shape))
    B, T, G = ll.shape
    S = seq_h.shape[1]
    _geometry(B >= 1 and 1 <= S <= MAX_S and 1 <= T <= MAX_T and 1 <= G <= MAX_G,
              "the Viterbi pass takes 1 <= S <= %d states, 1 <= T <= %d frames and 1 <= G <= %d Gaussians, got S=%d "
              "T=%d G=%d" % (MAX_S, MAX_T, MAX_G, S, T, G))
    live = np.arange(S)[None, :] < np.clip(ns_h, 0, S)[:, None]
    sk = (skip_h != 0) & live
    _geometry(not (sk[:, 1:] & sk[:, :-1]).any(), "two adjacent skippable states")
    if ((seq_h < 0) | (seq_h >= G))[live].any():
        raise ValueError("viterbi_align: seq holds a Gaussian outside [0, %d)" % G)
    ll = _dev(ll, "ll", torch.float32)
    dev = ll.device
    seq_d, skip_d = torch.from_numpy(seq_h).to(dev), torch.from_numpy(np.ascontiguousarray(sk.astype(np.uint8))).to(dev)
    nf_d, ns_d = torch.from_numpy(nf_h).to(dev), torch.from_numpy(ns_h).to(dev)
    L = _lib.lib()
    need = L.mg_align_viterbi_workspace_bytes(B, T, S)
    ws = torch.empty(need, device=dev, dtype=torch.uint8)
    durations = torch.empty(B, S, device=dev, dtype=torch.int32)
    score = torch.empty(B, device=dev, dtype=torch.float64)
    ok = torch.empty(B, device=dev, dtype=torch.int32)
    check(L.mg_align_viterbi(fptr(ll), _vp(seq_d), _vp(skip_d), _vp(nf_d), _vp(ns_d), B, T, S, G, _vp(durations),
                             _vp(score), _vp(ok), _vp(ws), need, stream_ptr()))
    return durations, score, ok


def gaussian_stats(x, gauss, G):
    """x [..., D] on the device, gauss int [...] the Gaussian of every row (negative: the row is not used) ->
    (sum, sumsq float64 [G, D], count int64 [G]) on the device.  The rows are sorted by Gaussian on the device, stably,
    and each Gaussian's are added in that order."""
    x = _dev(x, "x", torch.float32)
    gauss = _dev(gauss, "gauss", torch.int64).reshape(-1)
    D = x.shape[-1]
    x = x.reshape(-1, D)
    if gauss.shape[0] != x.shape[0]:
        raise ValueError("gaussian_stats: %d rows of features, %d Gaussian ids" % (x.shape[0], gauss.shape[0]))
    _geometry(1 <= D <= MAX_D and 1 <= G <= MAX_G and x.shape[0] < 2 ** 31,
              "statistics take 1 <= D <= %d and 1 <= G <= %d, got D=%d G=%d" % (MAX_D, MAX_G, D, G))
    if x.shape[0] and int(gauss.max()) >= G:
        raise ValueError("gaussian_stats: a Gaussian id beyond G = %d" % G)
    rows = torch.nonzero(gauss >= 0).reshape(-1)
    order = torch.sort(gauss[rows], stable=True).indices
    frame_index = rows[order].to(torch.int32).contiguous()
    count = torch.bincount(gauss[rows], minlength=G)
    offsets = torch.zeros(G + 1, device=x.device, dtype=torch.int64)
    offsets[1:] = torch.cumsum(count, 0)
    offsets = offsets.to(torch.int32).contiguous()
    s1 = torch.empty(G, D, device=x.device, dtype=torch.float64)
    s2 = torch.empty_like(s1)
    if frame_index.numel() == 0:
        frame_index = torch.zeros(1, device=x.device, dtype=torch.int32)
    check(_lib.lib().mg_align_stats(fptr(x), _vp(frame_index), _vp(offsets), G, D, _vp(s1), _vp(s2), stream_ptr()))
    return s1, s2, count


# ---------------------------------------------------------------------------------------------
# Host pieces: lexicon, state sequences, flat start, model, intervals
# ---------------------------------------------------------------------------------------------
def read_lexicon(path, encoding="utf-8"):
    """`word phone phone ...` lines -> {lower-cased word: [phones]}; the first entry of a word wins."""
    lexicon = {}
    with open(path, "r", encoding=encoding) as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 2 and parts[0].lower() not in lexicon:
                lexicon[parts[0].lower()] = parts[1:]
    return lexicon


def transcript_words(text):
    """The words of a `.lab` line: split at white space, punctuation at either end dropped."""
    words = [w.strip(_PUNCT) for w in text.split()]
    return [w for w in words if w]


def phone_inventory(lexicon):
    """Sorted phones of a lexicon, with `spn`; `sil` is the model's Gaussian 0 and not listed."""
    phones = {p for ph in lexicon.values() for p in ph} | {SPN}
    phones.discard(SIL)
    return sorted(phones)


def state_sequence(words, lexicon, phone_id, states_per_phone):
    """(seq, skip, units) of one transcript.  seq: the Gaussian of every state; skip: which states may be passed over
    (the silences); units: per phone or silence (first state, state count, phone, word index or -1, word text)."""
    seq, skip, units = [], [], []

    def silence():
        units.append((len(seq), 1, SIL, -1, ""))
        seq.append(0)
        skip.append(1)

    silence()
    for w, word in enumerate(words):
        phones = lexicon.get(word.lower())
        text = word
        if not phones or any(p not in phone_id for p in phones):
            phones, text = [SPN], UNK
        for p in phones:
            units.append((len(seq), states_per_phone, p, w, text))
            for k in range(states_per_phone):
                seq.append(1 + phone_id[p] * states_per_phone + k)
                skip.append(0)
        silence()
    return np.array(seq, dtype=np.int32), np.array(skip, dtype=np.uint8), units


def flat_start(skip, n_frames):
    """Uniform segmentation: the non-skippable states and the two outer silences share the frames equally, the
    remainder goes to the earliest, one frame each; inter-word silences get none.  None when there are fewer frames
    than shares."""
    S = len(skip)
    share = np.asarray(skip) == 0
    share[0] = share[S - 1] = True
    n = int(share.sum())
    if n_frames < n:
        return None
    dur = np.zeros(S, dtype=np.int32)
    q, r = divmod(int(n_frames), n)
    dur[share] = q
    dur[np.nonzero(share)[0][:r]] += 1
    return dur


def update_model(s1, s2, count, var_floor, min_count):
    """float64 sums -> (mean, var) [G, D]: mean = sum / n, var = max(sumsq / n - mean^2, var_floor); a Gaussian with
    n < min_count takes the mean and variance of all frames together."""
    s1, s2, count = np.asarray(s1, np.float64), np.asarray(s2, np.float64), np.asarray(count, np.float64)
    n_all = count.sum()
    g_mean = s1.sum(0) / n_all
    g_var = np.maximum(s2.sum(0) / n_all - g_mean * g_mean, var_floor)
    n = np.maximum(count, 1.0)[:, None]
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, var_floor)
    poor = count < min_count
    mean[poor], var[poor] = g_mean, g_var
    return mean, var


def model_tables(mean, var):
    """(A, Bm, c) float32 of the emission kernel: -0.5 / var, mean / var, -0.5 sum_d (mean^2 / var + log(2 pi var))."""
    A, Bm = -0.5 / var, mean / var
    c = -0.5 * (mean * mean / var + np.log(2.0 * np.pi * var)).sum(1)
    return A.astype(np.float32), Bm.astype(np.float32), c.astype(np.float32)


def intervals(units, durations, n_samples, hop, sr):
    """State durations -> (phones, words, xmax) interval lists, or None when the last phone would have no length in
    time.  A silence that took no frame is not written; an inter-word silence is `sp`, the outer ones `sil`; the
    words tier has "" over silences."""
    xmax = n_samples / float(sr)
    spans, pos = [], 0
    for k, (first, count, phone, w, text) in enumerate(units):
        d = int(np.sum(durations[first:first + count]))
        if d == 0:
            continue
        if phone == SIL and 0 < k < len(units) - 1:
            phone = SP
        spans.append([pos, pos + d, phone, w, text])
        pos += d
    bounds = [s[0] * hop / float(sr) for s in spans] + [xmax]
    bounds[0] = 0.0
    # n_samples a multiple of hop: the last frame starts at xmax, and a last interval of that frame alone has no
    # length in time.  A silence is then not written; a phone cannot be left out, and the row has no alignment.
    if len(spans) > 1 and not bounds[-2] < xmax:
        if spans[-1][3] >= 0:
            return None
        spans.pop()
        bounds.pop(-2)
    phones = [(bounds[i], bounds[i + 1], s[2]) for i, s in enumerate(spans)]
    words, i = [], 0
    while i < len(spans):
        j = i
        if spans[i][3] >= 0:
            while j + 1 < len(spans) and spans[j + 1][3] == spans[i][3]:
                j += 1
        words.append((bounds[i], bounds[j + 1], spans[i][4]))      # the very floats of the phones tier
        i = j + 1
    return phones, words, xmax


# ---------------------------------------------------------------------------------------------
# The aligner
# ---------------------------------------------------------------------------------------------
class ForcedAligner:
    def __init__(self, preprocess_config, lexicon=None, states_per_phone=3, n_iters=8, var_floor=1e-2, min_count=None,
                 batch_utterances=16, load_wav=None, device="cuda"):
        pp = preprocess_config["preprocessing"]
        self.in_dir = preprocess_config["path"]["raw_path"]
        self.out_dir = preprocess_config["path"]["preprocessed_path"]
        self.sampling_rate = pp["audio"]["sampling_rate"]
        self.hop_length = pp["stft"]["hop_length"]
        self.n_mel_channels = pp["mel"]["n_mel_channels"]
        if lexicon is None:
            lexicon = preprocess_config["path"]["lexicon_path"]
        self.lexicon = read_lexicon(lexicon) if isinstance(lexicon, (str, os.PathLike)) else \
            {w.lower(): list(p) for w, p in lexicon.items()}
        self.states_per_phone = int(states_per_phone)
        self.phones = phone_inventory(self.lexicon)
        self.n_iters, self.var_floor = int(n_iters), float(var_floor)
        # a variance from fewer frames than this is not trusted: twice the states of a phone
        self.min_count = 2 * self.states_per_phone if min_count is None else int(min_count)
        self.batch_utterances = max(1, int(batch_utterances))
        self.device = torch.device(device)
        _geometry(self.states_per_phone >= 1 and self.n_gaussians <= MAX_G and self.n_mel_channels <= MAX_D,
                  "%d phones of %d states need %d Gaussians, the kernels take %d of up to %d features"
                  % (len(self.phones), self.states_per_phone, self.n_gaussians, MAX_G, MAX_D))
        self.STFT = Audio.TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"],
                                       pp["mel"]["n_mel_channels"], pp["audio"]["sampling_rate"],
                                       pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])
        if load_wav is None:
            from .preprocessor import scipy_load_wav
            load_wav = scipy_load_wav(self.sampling_rate, False, self.device)
        self.load_wav = load_wav
        self.mean = self.var = None
        self.iterations, self.converged = 0, False

    @property
    def n_gaussians(self):
        return 1 + len(self.phones) * self.states_per_phone

    @property
    def _phone_id(self):
        return {p: i for i, p in enumerate(self.phones)}

    # ------------------------------------------------------------------ one batch
    def _load(self, items):
        """Per item (wav or None, words): the clipped float32 signal and the transcript's words."""
        out = []
        for speaker, basename in items:
            wav = np.clip(np.asarray(self.load_wav(os.path.join(self.in_dir, speaker, basename + ".wav")),
                                     dtype=np.float32), -1, 1)
            with open(os.path.join(self.in_dir, speaker, basename + ".lab"), "r", encoding="utf-8") as f:
                words = transcript_words(f.readline())
            out.append((wav, words))
        return out

    def features(self, wavs):
        """List of float32 signals -> (x [B, T, D] on the device, n_frames int32 numpy): mean-removed log-mel.  A row
        does not depend on what else is in the batch."""
        lens = np.array([len(w) for w in wavs], dtype=np.int64)
        batch = np.zeros((len(wavs), int(lens.max())), dtype=np.float32)
        for b, w in enumerate(wavs):
            batch[b, :lens[b]] = w
        if self.STFT.mel_basis.device != self.device:
            self.STFT = self.STFT.to(self.device)
        mel, _ = self.STFT.mel_spectrogram(torch.from_numpy(batch).to(self.device), lens)
        n_frames = (lens // self.hop_length + 1).astype(np.int32)
        x = torch.zeros(mel.shape[0], mel.shape[2], mel.shape[1], device=self.device, dtype=torch.float32)
        for b, n in enumerate(n_frames):
            # float64 over the row's own frames alone: the reduction has the same shape, so the same bits, whatever the
            # rest of the batch is
            row = mel[b, :, :n].transpose(0, 1).double()
            x[b, :n] = (row - row.mean(0, keepdim=True)).float()
        return x, n_frames

    def _prepare(self, items):
        """Batches of what the passes need: kept item indices, features, frame counts, padded state sequences, units;
        and {item index: reason} for what cannot be aligned at all."""
        batches, reasons = [], {}
        for k in range(0, len(items), self.batch_utterances):
            loaded = self._load(items[k:k + self.batch_utterances])
            keep, wavs, seqs = [], [], []
            for j, (wav, words) in enumerate(loaded):
                seq, skip, units = state_sequence(words, self.lexicon, self._phone_id, self.states_per_phone)
                n_frames = len(wav) // self.hop_length + 1
                if not words:
                    reasons[k + j] = "empty transcript"
                elif len(wav) <= Audio.N_FFT // 2:
                    reasons[k + j] = "audio shorter than the analysis window"
                elif len(seq) > MAX_S or n_frames > MAX_T:
                    reasons[k + j] = "%d states over %d frames: the kernels take %d and %d" % (len(seq), n_frames,
                                                                                               MAX_S, MAX_T)
                else:
                    keep.append(k + j)
                    wavs.append(wav)
                    seqs.append((seq, skip, units))
            if not keep:
                continue
            x, n_frames = self.features(wavs)
            S = max(len(s[0]) for s in seqs)
            seq = np.zeros((len(keep), S), dtype=np.int32)
            skip = np.zeros((len(keep), S), dtype=np.uint8)
            for b, (q, sk, _) in enumerate(seqs):
                seq[b, :len(q)], skip[b, :len(q)] = q, sk
            batches.append({"index": keep, "x": x, "n_frames": n_frames, "seq": seq, "skip": skip,
                            "n_states": np.array([len(s[0]) for s in seqs], dtype=np.int32),
                            "units": [s[2] for s in seqs], "n_samples": [len(w) for w in wavs]})
        return batches, reasons

    def _tables(self):
        if self.mean is None:
            raise MixganHipError("ForcedAligner: no model: call fit() or load() first")
        return [torch.from_numpy(t).to(self.device) for t in model_tables(self.mean, self.var)]

    def _decode(self, batch, tables):
        ll = emissions(batch["x"], torch.from_numpy(batch["n_frames"]).to(self.device), *tables)
        dur, score, ok = viterbi_align(ll, batch["seq"], batch["skip"], batch["n_frames"], batch["n_states"])
        return dur.cpu().numpy(), score.cpu().numpy(), ok.cpu().numpy()

    def _stats(self, batch, durations, train):
        """Sums of one batch under its rows' state durations; rows outside `train` give nothing."""
        B, T = batch["x"].shape[:2]
        gauss = np.full((B, T), -1, dtype=np.int64)
        for b in range(B):
            if train[b]:
                n = int(batch["n_states"][b])
                gauss[b, :batch["n_frames"][b]] = np.repeat(batch["seq"][b, :n], durations[b][:n])
        s1, s2, count = gaussian_stats(batch["x"], torch.from_numpy(gauss).to(self.device), self.n_gaussians)
        return s1.cpu().numpy(), s2.cpu().numpy(), count.cpu().numpy()

    # ------------------------------------------------------------------ the public passes
    def fit(self, items):
        """Flat start and up to n_iters rounds of hard EM over `items` ((speaker, basename) under raw_path).  n_iters is
        a cap, not a promise of convergence: `iterations` and `converged` say how the fit ended, and a fit that hit
        the cap can be repeated with a larger one.  The features of the whole list stay on the device for the rounds.  Returns {item: reason} of what was left out."""
        items = list(items)
        batches, reasons = self._prepare(items)
        durs, train = [], []
        for bt in batches:
            d = [flat_start(bt["skip"][b, :bt["n_states"][b]], int(bt["n_frames"][b])) for b in range(len(bt["index"]))]
            for b, v in enumerate(d):
                if v is None:
                    reasons[bt["index"][b]] = "fewer frames than states"
            train.append([v is not None for v in d])
            durs.append([v if v is not None else np.zeros(bt["n_states"][b], np.int32) for b, v in enumerate(d)])
        if not any(any(t) for t in train):
            raise MixganHipError("ForcedAligner.fit: no utterance can be aligned: %s" % sorted(set(reasons.values())))
        G, D = self.n_gaussians, self.n_mel_channels
        self.iterations, self.converged = 0, False
        for _ in range(self.n_iters):
            s1, s2, count = np.zeros((G, D)), np.zeros((G, D)), np.zeros(G, dtype=np.int64)
            for bt, d, tr in zip(batches, durs, train):
                a, b_, c = self._stats(bt, d, tr)
                s1, s2, count = s1 + a, s2 + b_, count + c
            self.mean, self.var = update_model(s1, s2, count, self.var_floor, self.min_count)
            tables = self._tables()
            changed = False
            for bt, d, tr in zip(batches, durs, train):
                new, _, ok = self._decode(bt, tables)
                for b in range(len(d)):
                    n = int(bt["n_states"][b])
                    if tr[b] and ok[b] and not np.array_equal(new[b, :n], d[b]):
                        d[b] = new[b, :n].copy()
                        changed = True
            self.iterations += 1
            if not changed:
                self.converged = True
                break
        return {items[i]: r for i, r in sorted(reasons.items())}

    def align(self, items):
        """Per item, in order: (phones, words, xmax) with the tiers as (start, end, text) lists, or a string saying why
        the item cannot be aligned."""
        items = list(items)
        batches, reasons = self._prepare(items)
        tables = self._tables()
        out = [reasons.get(i) for i in range(len(items))]
        for bt in batches:
            dur, _, ok = self._decode(bt, tables)
            for b, i in enumerate(bt["index"]):
                if not ok[b]:
                    out[i] = "fewer frames than states"
                    continue
                out[i] = intervals(bt["units"][b], dur[b], bt["n_samples"][b], self.hop_length, self.sampling_rate) \
                    or "the last phone has no length in time"
        return out

    def corpus_items(self):
        """(speaker, basename) of every wav with a `.lab` beside it under raw_path, sorted."""
        items = []
        for speaker in sorted(os.listdir(self.in_dir)):
            d = os.path.join(self.in_dir, speaker)
            if not os.path.isdir(d):
                continue
            for name in sorted(os.listdir(d)):
                base, ext = os.path.splitext(name)
                if ext == ".wav" and os.path.exists(os.path.join(d, base + ".lab")):
                    items.append((speaker, base))
        return items

    def build_from_path(self):
        """Fit on everything under raw_path, align it, and write preprocessed_path/TextGrid/<speaker>/<name>.TextGrid.
        Returns {(speaker, basename): reason} of what was skipped."""
        from .preprocessor import write_textgrid
        items = self.corpus_items()
        self.fit(items)
        skipped = {}
        for k in range(0, len(items), self.batch_utterances):
            chunk = items[k:k + self.batch_utterances]
            for (speaker, basename), res in zip(chunk, self.align(chunk)):
                if isinstance(res, str):
                    skipped[(speaker, basename)] = res
                    continue
                phones, words, xmax = res
                os.makedirs(os.path.join(self.out_dir, "TextGrid", speaker), exist_ok=True)
                write_textgrid(os.path.join(self.out_dir, "TextGrid", speaker, basename + ".TextGrid"),
                               {"words": words, "phones": phones}, xmax)
        return skipped

    # ------------------------------------------------------------------ the model on disk
    def save(self, path):
        if self.mean is None:
            raise MixganHipError("ForcedAligner.save: no model")
        with open(path, "wb") as f:
            np.savez(f, mean=self.mean, var=self.var, phones=np.array(self.phones, dtype=np.str_),
                     states_per_phone=np.int64(self.states_per_phone), sampling_rate=np.int64(self.sampling_rate),
                     hop_length=np.int64(self.hop_length))

    def load(self, path):
        with np.load(path, allow_pickle=False) as z:
            phones, spp = [str(p) for p in z["phones"]], int(z["states_per_phone"])
            if phones != self.phones or spp != self.states_per_phone or int(z["hop_length"]) != self.hop_length \
                    or int(z["sampling_rate"]) != self.sampling_rate \
                    or z["mean"].shape != (self.n_gaussians, self.n_mel_channels):
                raise MixganHipError("ForcedAligner.load: %s was fitted with another lexicon, state count or feature "
                                     "geometry" % path)
            self.mean, self.var = z["mean"].astype(np.float64), z["var"].astype(np.float64)
        return self
