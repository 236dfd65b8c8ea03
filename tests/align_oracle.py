"""The forced aligner's float64 oracle: a numpy restatement of the five stages of mixgan_tts_amd/aligner.py (features,
state sequences, flat start, model update, intervals) and of the definitions of the three kernels of csrc/align.hip
(emissions, Viterbi, statistics).  It is this project's own algorithm stated a second time, plainly and slowly; there
is no third party to compare with.  Host tables (window, mel filterbank) come from the package."""
import numpy as np

SIL, SP, SPN, UNK = "sil", "sp", "spn", "<unk>"
N_FFT = 1024
NEG = -np.inf


# ---------------------------------------------------------------------------------------------
# The three kernels
# ---------------------------------------------------------------------------------------------
def emissions(x, n_frames, A, Bm, c):
    """x [B, T, D], tables [G, D] and [G] -> (ll [B, T, G], mag [B, T, G]) in float64; mag is the sum of the absolute
    values of every term of ll's sum, what a rounding bound of a float32 evaluation scales with.  Both are 0 at
    t >= n_frames[b]."""
    x, A, Bm, c = (np.asarray(a, dtype=np.float64) for a in (x, A, Bm, c))
    x2 = x * x
    ll = np.einsum("btd,gd->btg", x2, A) + np.einsum("btd,gd->btg", x, Bm) + c
    mag = np.einsum("btd,gd->btg", x2, np.abs(A)) + np.einsum("btd,gd->btg", np.abs(x), np.abs(Bm)) + np.abs(c)
    live = np.arange(x.shape[1])[None, :] < np.asarray(n_frames)[:, None]
    return ll * live[:, :, None], mag * live[:, :, None]


def viterbi_row(e, skip):
    """e [T, S] float64 emission scores of one row's states, skip [S] -> (durations [S], score, ok).
    delta_0(s) = e_0(s) for s = 0 and, if skip[0], s = 1; delta_t(s) = e_t(s) + max(stay, advance, skip over s - 1 if
    it is skippable), ties to the smallest jump; the end is S - 1, or S - 2 when skip[S - 1] and strictly better."""
    T, S = e.shape
    dur = np.zeros(S, dtype=np.int32)
    if T == 0 or S == 0:
        return dur, NEG, 0
    skip = np.asarray(skip) != 0
    delta = np.full(S, NEG)
    delta[0] = e[0, 0]
    if S > 1 and skip[0]:
        delta[1] = e[0, 1]
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        adv, skp = np.full(S, NEG), np.full(S, NEG)
        adv[1:] = delta[:-1]
        if S > 2:
            skp[2:] = np.where(skip[1:-1], delta[:-2], NEG)
        best, arg = delta.copy(), np.zeros(S, dtype=np.int8)
        m = adv > best
        best[m], arg[m] = adv[m], 1
        m = skp > best
        best[m], arg[m] = skp[m], 2
        delta = e[t] + best
        back[t] = arg
    s = S - 1
    if S >= 2 and skip[S - 1] and delta[S - 2] > delta[S - 1]:
        s = S - 2
    score = delta[s]
    if not score > NEG:
        return dur, NEG, 0
    for t in range(T - 1, 0, -1):
        dur[s] += 1
        s -= int(back[t, s])
    dur[s] += 1
    return dur, score, 1


def viterbi(ll, seq, skip, n_frames, n_states):
    """ll [B, T, G] (any float type; taken to float64 as it is) -> (durations [B, S], score [B], ok [B])."""
    ll = np.asarray(ll).astype(np.float64)
    B, S = np.asarray(seq).shape
    dur, score, ok = np.zeros((B, S), np.int32), np.full(B, NEG), np.zeros(B, np.int32)
    for b in range(B):
        nf, ns = int(n_frames[b]), int(n_states[b])
        e = ll[b, :nf][:, np.asarray(seq[b, :ns], dtype=np.int64)]
        dur[b, :ns], score[b], ok[b] = viterbi_row(e, skip[b, :ns])
    return dur, score, ok


def brute_force(e, skip):
    """The best path of viterbi_row's graph by enumerating every path: (durations, score) or (None, -inf).  Among
    paths of equal score the one viterbi_row's tie rule picks is not decided here; callers compare scores, and
    durations only where the best is unique."""
    T, S = e.shape
    skip = np.asarray(skip) != 0
    starts = [0] + ([1] if S > 1 and skip[0] else [])
    ends = [S - 1] + ([S - 2] if S >= 2 and skip[S - 1] else [])
    found = []

    def walk(t, s, total, path):
        if t == T - 1:
            if s in ends:
                found.append((total, tuple(path)))
            return
        for jump in (0, 1, 2):
            n = s + jump
            if n >= S or (jump == 2 and not skip[s + 1]):
                continue
            walk(t + 1, n, total + e[t + 1, n], path + [n])

    for s in starts:
        walk(0, s, e[0, s], [s])
    return found


def stats(x, frame_index, offsets, G):
    """x [rows, D] -> (sum, sumsq) float64 [G, D]: Gaussian g adds the rows frame_index[offsets[g] : offsets[g + 1]] in
    list order (np.cumsum is a running sum in order; np.sum is not)."""
    x = np.asarray(x).astype(np.float64)
    D = x.shape[1]
    s1, s2 = np.zeros((G, D)), np.zeros((G, D))
    for g in range(G):
        rows = np.asarray(frame_index[offsets[g]:offsets[g + 1]], dtype=np.int64)
        if len(rows):
            s1[g] = np.cumsum(x[rows], axis=0)[-1]
            s2[g] = np.cumsum(x[rows] * x[rows], axis=0)[-1]
    return s1, s2


def sorted_frames(gauss, G):
    """Per-row Gaussian ids (negative: unused) -> (frame_index, offsets): rows stably sorted by id."""
    gauss = np.asarray(gauss).reshape(-1)
    rows = np.nonzero(gauss >= 0)[0]
    order = np.argsort(gauss[rows], kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(gauss[rows], minlength=G))])
    return rows[order].astype(np.int32), offsets.astype(np.int32)


# ---------------------------------------------------------------------------------------------
# The five stages
# ---------------------------------------------------------------------------------------------
def features(wav, sr, hop, n_mels, fmin, fmax, win=1024):
    """Stage 1: log-mel of the reflect-padded signal (frame k centred on sample k hop, len // hop + 1 frames) minus its
    mean over the frames: [T, n_mels] float64."""
    import mixgan_tts_amd as mg
    x = np.pad(np.clip(np.asarray(wav, dtype=np.float64), -1, 1), N_FFT // 2, mode="reflect")
    T = len(wav) // hop + 1
    window = mg.audio.pad_center(mg.audio.hann_window(win), N_FFT)
    frames = np.stack([x[k * hop:k * hop + N_FFT] for k in range(T)]) * window
    mag = np.abs(np.fft.rfft(frames, axis=1))
    basis = mg.audio.mel_filterbank(sr, N_FFT, n_mels, fmin, fmax).astype(np.float64)
    mel = np.log(np.maximum(mag @ basis.T, 1e-5))
    return mel - mel.mean(0, keepdims=True)


def state_sequence(words, lexicon, phones, spp):
    """Stage 2: (seq, skip, units); units = (first state, state count, phone, word index or -1, word text)."""
    pid = {p: i for i, p in enumerate(phones)}
    seq, skip, units = [0], [1], [(0, 1, SIL, -1, "")]
    for w, word in enumerate(words):
        ph, text = lexicon.get(word.lower()), word
        if not ph:
            ph, text = [SPN], UNK
        for p in ph:
            units.append((len(seq), spp, p, w, text))
            seq += [1 + pid[p] * spp + k for k in range(spp)]
            skip += [0] * spp
        units.append((len(seq), 1, SIL, -1, ""))
        seq.append(0)
        skip.append(1)
    return np.array(seq, np.int32), np.array(skip, np.uint8), units


def flat_start(skip, T):
    """Stage 3, iteration 0: equal shares for the non-skippable states and the two outer silences, the remainder to
    the earliest; None when T is smaller than the number of shares."""
    share = [i for i in range(len(skip)) if not skip[i] or i in (0, len(skip) - 1)]
    if T < len(share):
        return None
    dur = np.zeros(len(skip), np.int32)
    for k, i in enumerate(share):
        dur[i] = T // len(share) + (1 if k < T % len(share) else 0)
    return dur


def update_model(s1, s2, count, var_floor, min_count):
    """Stage 4: (mean, var) and the float32 tables (A, Bm, c)."""
    count = np.asarray(count, dtype=np.float64)
    n_all = count.sum()
    g_mean = s1.sum(0) / n_all
    g_var = np.maximum(s2.sum(0) / n_all - g_mean ** 2, var_floor)
    mean, var = np.empty_like(s1), np.empty_like(s1)
    for g in range(len(count)):
        if count[g] < min_count:
            mean[g], var[g] = g_mean, g_var
        else:
            mean[g] = s1[g] / count[g]
            var[g] = np.maximum(s2[g] / count[g] - mean[g] ** 2, var_floor)
    return mean, var


def tables(mean, var):
    A, Bm = -0.5 / var, mean / var
    c = -0.5 * (mean ** 2 / var + np.log(2 * np.pi * var)).sum(1)
    return A.astype(np.float32), Bm.astype(np.float32), c.astype(np.float32)


def intervals(units, dur, n_samples, hop, sr):
    """Stage 5: (phones, words, xmax).  A state that starts at frame k starts at k hop / sr; the first interval starts
    at 0, the last ends at n_samples / sr."""
    xmax = n_samples / sr
    spans, pos = [], 0
    for k, (first, count, phone, w, text) in enumerate(units):
        d = int(dur[first:first + count].sum())
        if d:
            spans.append((pos, SP if phone == SIL and 0 < k < len(units) - 1 else phone, w, text))
            pos += d
    bounds = [0.0] + [s[0] * hop / sr for s in spans[1:]] + [xmax]
    if len(spans) > 1 and bounds[-2] >= xmax:      # the last interval is the one frame that starts at the signal's end
        if spans[-1][2] >= 0:
            return None                            # a phone without length: no alignment
        del spans[-1], bounds[-2]                  # a silence without length: not written
    phones = [(bounds[i], bounds[i + 1], s[1]) for i, s in enumerate(spans)]
    words = []
    for i, s in enumerate(spans):
        if words and s[2] >= 0 and i and spans[i - 1][2] == s[2]:
            words[-1] = (words[-1][0], bounds[i + 1], s[3])
        else:
            words.append((bounds[i], bounds[i + 1], s[3]))
    return phones, words, xmax


def fit_and_align(wavs, transcripts, lexicon, sr, hop, n_mels, fmin, fmax, spp=3, n_iters=8, var_floor=1e-2,
                  min_count=None):
    """The whole pipeline on a list of signals and word lists: (per utterance (phones, words, xmax), iterations run,
    (mean, var))."""
    phones = sorted(({p for ph in lexicon.values() for p in ph} | {SPN}) - {SIL})
    G = 1 + len(phones) * spp
    min_count = 2 * spp if min_count is None else min_count
    feats = [features(w, sr, hop, n_mels, fmin, fmax) for w in wavs]
    seqs = [state_sequence(t, lexicon, phones, spp) for t in transcripts]
    durs = [flat_start(s[1], len(f)) for s, f in zip(seqs, feats)]
    train = [d is not None for d in durs]
    D = feats[0].shape[1]
    iters, model = 0, None
    for _ in range(n_iters):
        s1, s2, count = np.zeros((G, D)), np.zeros((G, D)), np.zeros(G)
        for f, (seq, _, _), d, tr in zip(feats, seqs, durs, train):
            if tr:
                gauss = np.repeat(seq, d)
                fi, off = sorted_frames(gauss, G)
                a, b = stats(f, fi, off, G)
                s1, s2, count = s1 + a, s2 + b, count + np.diff(off)
        model = update_model(s1, s2, count, var_floor, min_count)
        A, Bm, c = tables(*model)
        changed = False
        for i, (f, (seq, skip, _)) in enumerate(zip(feats, seqs)):
            if not train[i]:
                continue
            ll, _ = emissions(f[None], [len(f)], A, Bm, c)
            d, _, ok = viterbi(ll, seq[None], skip[None], [len(f)], [len(seq)])
            if ok[0] and not np.array_equal(d[0], durs[i]):
                durs[i], changed = d[0], True
        iters += 1
        if not changed:
            break
    A, Bm, c = tables(*model)
    out = []
    for f, (seq, skip, units), w in zip(feats, seqs, wavs):
        ll, _ = emissions(f[None], [len(f)], A, Bm, c)
        d, _, ok = viterbi(ll, seq[None], skip[None], [len(f)], [len(seq)])
        out.append(intervals(units, d[0], len(w), hop, sr) if ok[0] else None)      # None: no alignment
    return out, iters, model


def boundary_error(phones, truth, sr, hop):
    """Absolute errors, in frames, of the start and the end of every phone that is not a silence, matched in order.
    None when the two tiers do not hold the same such phones."""
    got = [(s, e, p) for s, e, p in phones if p not in (SIL, SP)]
    want = [(s, e, p) for s, e, p in truth if p not in (SIL, SP)]
    if [p for _, _, p in got] != [p for _, _, p in want]:
        return None
    return [abs(g[k] - w[k]) * sr / hop for g, w in zip(got, want) for k in (0, 1)]
