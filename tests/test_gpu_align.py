"""The forced aligner on the GPU (csrc/align.hip, mixgan_tts_amd/aligner.py) against its float64 oracle
(tests/align_oracle.py): each kernel on its own, then fit / align on the synthetic corpus of tests/align_corpus.py
against the boundaries the corpus was built with, then the chain into the corpus builder."""
import os

import numpy as np
import pytest
import torch

import align_corpus as C
import align_oracle as O
from test_align_cpu import E_O, N_ITERS

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ emissions
@pytest.mark.parametrize("D", [3, 80])
@pytest.mark.parametrize("G", [1, 65, 130])
def test_emissions_against_the_oracle(D, G):
    """|ll - oracle| <= (2 D + 4) 2^-24 (sum_d |A x^2| + |Bm x| + |c|) per element, the bound of a float32 dot product
    of 2 D + 1 terms in any order with its products rounded; padding is exact zeros; a row keeps its bits wherever it
    sits in the batch."""
    import mixgan_tts_amd as mg
    rng = np.random.default_rng(1000 * D + G)
    n_frames = np.array([1, 33, 70], dtype=np.int32)
    x = rng.standard_normal((3, 70, D)).astype(np.float32)
    x[np.arange(70)[None, :] >= n_frames[:, None]] = np.nan      # what lies past a row's frames is not read
    var = rng.uniform(0.05, 2.0, (G, D))
    mean = rng.standard_normal((G, D))
    A, Bm, c = O.tables(mean, var)
    ll = mg.emissions(_dev(x), _dev(n_frames), _dev(A), _dev(Bm), _dev(c))
    torch.cuda.synchronize()
    assert ll.shape == (3, 70, G) and ll.dtype == torch.float32
    ll = ll.cpu().numpy()
    want, mag = O.emissions(np.nan_to_num(x), n_frames, A, Bm, c)
    live = np.arange(70)[None, :] < n_frames[:, None]
    assert (ll[~live] == 0).all() and np.isfinite(ll).all()
    tol = (2 * D + 4) * 2.0 ** -24 * mag
    excess = (np.abs(ll - want) - tol)[live]
    print("D=%d G=%d: worst |err| / tol = %.3f" % (D, G, (np.abs(ll - want)[live] / tol[live]).max()))
    assert (excess <= 0).all()
    rev = mg.emissions(_dev(x[::-1]), _dev(n_frames[::-1]), _dev(A), _dev(Bm), _dev(c)).cpu().numpy()
    assert np.array_equal(rev[::-1], ll)


# ------------------------------------------------------------------ Viterbi
def _viterbi_case(ll, seq, skip, n_frames, n_states):
    import mixgan_tts_amd as mg
    dur, score, ok = mg.viterbi_align(_dev(ll), seq, skip, n_frames, n_states)
    torch.cuda.synchronize()
    dur, score, ok = dur.cpu().numpy(), score.cpu().numpy(), ok.cpu().numpy()
    odur, oscore, ook = O.viterbi(ll, seq, skip, n_frames, n_states)
    assert np.array_equal(ok, ook), (ok, ook)
    assert np.array_equal(dur, odur), np.nonzero(dur != odur)
    assert score.tobytes() == oscore.tobytes(), (score, oscore)
    assert (dur.sum(1)[ok != 0] == np.asarray(n_frames)[ok != 0]).all() and not dur[ok == 0].any()
    return dur, score, ok


def _alternating_skip(S, first):
    skip = np.zeros(S, np.uint8)
    skip[first::2] = 1
    return skip


def test_viterbi_small_cases():
    rng = np.random.default_rng(7)
    G = 5
    ll = rng.standard_normal((1, 9, G)).astype(np.float32)
    one = np.array([[2]], np.int32)
    dur, _, ok = _viterbi_case(ll, one, np.zeros((1, 1), np.uint8), [9], [1])      # S = 1
    assert ok[0] and dur[0, 0] == 9
    two = np.array([[0, 3]], np.int32)
    _viterbi_case(ll, two, np.array([[1, 0]], np.uint8), [9], [2])                  # S = 2 with skip[0]
    _viterbi_case(ll[:, :1], two, np.array([[1, 0]], np.uint8), [1], [2])           # one frame: only by skipping state 0
    seq = np.array([[0, 1, 2, 0, 3, 4, 0]], np.int32)
    skip = np.array([[1, 0, 0, 1, 0, 0, 1]], np.uint8)
    dur, _, ok = _viterbi_case(ll, seq, skip, [4], [7])                             # no slack: T = non-skippable states
    assert ok[0] and list(dur[0]) == [0, 1, 1, 0, 1, 1, 0]
    dur, score, ok = _viterbi_case(ll, seq, skip, [3], [7])                         # one frame short
    assert not ok[0] and score[0] == -np.inf
    _viterbi_case(ll, seq, skip, [0], [7])                                          # no frames
    _viterbi_case(ll, seq, skip, [9], [0])                                          # no states
    dur, score, ok = _viterbi_case(np.zeros((1, 9, G), np.float32), seq, skip, [9], [7])      # the tie rule alone
    assert ok[0] and score[0] == 0.0


@pytest.mark.parametrize("S", [257, 513])
@pytest.mark.parametrize("T", [65, 130])
def test_viterbi_across_chunk_and_word_boundaries(S, T):
    """More states than a thread's eight and than a block of back-pointer half-words, a last half-word with one state
    in it, more frames than several backtrace blocks; T < the non-skippable states of the dense row gives ok = 0
    there.  With T <= 130 a live path has at most 259 states, all inside the first wave's 512: the case below this one
    crosses the wave boundary."""
    rng = np.random.default_rng(S + T)
    G = 37
    ll = (3 * rng.standard_normal((3, T, G))).astype(np.float32)
    seq = rng.integers(0, G, (3, S)).astype(np.int32)
    skip = np.stack([_alternating_skip(S, 0), _alternating_skip(S, 1), np.zeros(S, np.uint8)])
    n_states = [min(S, 2 * T - 1), min(S, T), S]
    dur, _, ok = _viterbi_case(ll, seq, skip, [T, T - 3, T], n_states)
    assert ok[0] and ok[1] and not ok[2]


def test_viterbi_live_path_across_the_wave_boundary():
    """S = 600 over T = 320 frames: two waves (thread 63 hands its last two delta to thread 64 through LDS), live
    paths that end in or next to states 598, 599 and 299, and a backtrace that starts above half-word group 64."""
    rng = np.random.default_rng(600)
    S, T, G = 600, 320, 23
    ll = (3 * rng.standard_normal((3, T, G))).astype(np.float32)
    seq = rng.integers(0, G, (3, S)).astype(np.int32)
    skip = np.stack([_alternating_skip(S, 0), _alternating_skip(S, 1), np.zeros(S, np.uint8)])
    dur, _, ok = _viterbi_case(ll, seq, skip, [T, T - 7, T], [599, 600, 300])
    assert ok.all() and dur[0, 512:].sum() > 0 and dur[1, 512:].sum() > 0


def test_viterbi_ragged_batch_and_its_reverse():
    rng = np.random.default_rng(11)
    B, T, S, G = 6, 70, 41, 19
    ll = (2 * rng.standard_normal((B, T, G))).astype(np.float32)
    seq = rng.integers(0, G, (B, S)).astype(np.int32)
    skip = np.zeros((B, S), np.uint8)
    for b in range(B):
        for s in range(0, S, 1 + b % 3 + 1):
            skip[b, s] = rng.integers(0, 2)
        skip[b, 1:][(skip[b, 1:] != 0) & (skip[b, :-1] != 0)] = 0
    n_frames, n_states = np.array([70, 1, 33, 64, 12, 50]), np.array([41, 2, 17, 40, 9, 33])
    skip[1, :2] = [1, 0]
    dur, score, ok = _viterbi_case(ll, seq, skip, n_frames, n_states)
    assert ok.sum() >= 5
    rdur, rscore, rok = _viterbi_case(ll[::-1], seq[::-1], skip[::-1], n_frames[::-1], n_states[::-1])
    assert np.array_equal(rdur[::-1], dur) and rscore[::-1].tobytes() == score.tobytes() and np.array_equal(rok[::-1], ok)


# ------------------------------------------------------------------ statistics
def test_statistics_against_the_oracle():
    """Both sides add the same float64 values in the same order; 1e-12 relative is margin only."""
    import mixgan_tts_amd as mg
    rng = np.random.default_rng(5)
    rows, D, G = 700, 80, 9
    x = rng.standard_normal((rows, D)).astype(np.float32)
    gauss = rng.integers(-1, G, rows)
    gauss[gauss == 4] = 5            # Gaussian 4 owns nothing
    gauss[:3] = 8
    s1, s2, count = mg.gaussian_stats(_dev(x), _dev(gauss), G)
    again = mg.gaussian_stats(_dev(x), _dev(gauss), G)
    torch.cuda.synchronize()
    fi, off = O.sorted_frames(gauss, G)
    o1, o2 = O.stats(x, fi, off, G)
    s1, s2, count = s1.cpu().numpy(), s2.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(count, np.diff(off)) and count[4] == 0 and not s1[4].any() and not s2[4].any()
    scale1 = np.abs(x.astype(np.float64)).sum(0).max()
    assert np.abs(s1 - o1).max() <= 1e-12 * scale1 and np.abs(s2 - o2).max() <= 1e-12 * np.abs(o2).max()
    assert torch.equal(again[0].cpu(), torch.from_numpy(s1)) and torch.equal(again[1].cpu(), torch.from_numpy(s2))
    # an odd D, one row, a segment that is no multiple of the four rows loaded ahead
    x3 = rng.standard_normal((6, 3)).astype(np.float32)
    g3 = np.array([1, 1, 0, 1, 1, 1])
    a1, a2, _ = mg.gaussian_stats(_dev(x3), _dev(g3), 2)
    b1, b2 = O.stats(x3, *O.sorted_frames(g3, 2), 2)
    assert np.array_equal(a1.cpu().numpy(), b1) and np.array_equal(a2.cpu().numpy(), b2)


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("align"))
    raw, pre, lex = C.write_corpus(root)
    return C.configs(raw, pre, lex)


def _aligner(corpus, **kw):
    import mixgan_tts_amd as mg
    return mg.ForcedAligner(corpus[0], n_iters=N_ITERS + 6, batch_utterances=5, load_wav=C.load_wav, **kw)


def test_fit_is_reproducible_and_finds_the_known_boundaries(corpus, tmp_path):
    """Mean absolute boundary error <= 2 E_O: the margin tests/test_gpu_pitch.py gives its oracle, here for float32
    emissions and features against the oracle's float64."""
    items = [(C.SPEAKER, n) for n in C.NAMES]
    a, b = _aligner(corpus), _aligner(corpus)
    assert a.fit(items) == {} and b.fit(items) == {}
    assert a.mean.tobytes() == b.mean.tobytes() and a.var.tobytes() == b.var.tobytes() and a.iterations == b.iterations
    assert a.iterations < N_ITERS + 6, "no fixed point within %d rounds" % (N_ITERS + 6)
    d = _aligner(corpus)
    d.n_iters = 8      # the constructor's default: a cap, reached here before the fixed point
    d.fit(items)
    assert (d.iterations, d.converged, a.converged) == (8, False, True) and a.iterations > 8
    res = a.align(items)
    errs = []
    for name, r in zip(C.NAMES, res):
        assert not isinstance(r, str), (name, r)
        phones, words, xmax = r
        truth_ph, _, n = C.truth(name)
        e = O.boundary_error(phones, truth_ph, C.SR, C.HOP)
        assert e is not None, (name, phones)
        errs += e
        labels = [p for _, _, p in phones]
        assert ("sp" in labels) == (name == C.PAUSED), (name, labels)           # the one real pause, no other
        assert ("spn" in labels) == (name in C.WITH_OOV), (name, labels)
        assert ("<unk>" in [w for _, _, w in words]) == (name in C.WITH_OOV)
        assert xmax == n / C.SR and phones[-1][1] == xmax and phones[0][0] == 0.0 and "" not in labels
    err = float(np.mean(errs))
    print("aligner: mean |boundary error| = %.4f frames (oracle %.4f), worst %.3f, %d rounds"
          % (err, E_O, max(errs), a.iterations))
    assert err <= 2 * E_O
    # the model on disk
    path = str(tmp_path / "model.npz")
    a.save(path)
    c = _aligner(corpus).load(path)
    assert c.mean.tobytes() == a.mean.tobytes() and c.align(items[:2]) == res[:2]


def test_build_from_path_feeds_the_corpus_builder(corpus):
    """TextGrids written by build_from_path are read by the existing Preprocessor, and the durations it stores are the
    aligner's frame counts of the phones it keeps (everything between the outer silences).  The builder loads the
    quiet rendering of the utterances (C.load_wav_quiet): under the corpus's own noise its pitch extractor finds no
    voiced frame, every utterance is filtered out and there is nothing to normalise; the durations come from the
    TextGrids alone either way.  Of the quiet rendering the builder keeps every utterance."""
    import mixgan_tts_amd as mg
    al = _aligner(corpus)
    assert al.build_from_path() == {}
    pre = corpus[0]["path"]["preprocessed_path"]
    res = al.align([(C.SPEAKER, n) for n in C.NAMES])
    mg.Preprocessor(*corpus, pitch_fn="native", load_wav=C.load_wav_quiet).build_from_path()
    with open(os.path.join(pre, "filtered_out.txt")) as f:
        assert f.read().split() == []
    for name, (phones, words, xmax) in zip(C.NAMES, res):
        tiers = mg.read_textgrid(os.path.join(pre, "TextGrid", C.SPEAKER, name + ".TextGrid"), True)
        assert tiers["phones"] == phones and tiers["words"] == words
        frames = [int(round(e * C.SR / C.HOP)) - int(round(s * C.SR / C.HOP)) for s, e, _ in phones[1:-1]]
        stored = np.load(os.path.join(pre, "duration", "%s-duration-%s.npy" % (C.SPEAKER, name)))
        assert phones[0][2] == "sil" and phones[-1][2] == "sil" and stored.tolist() == frames, name
