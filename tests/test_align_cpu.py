"""The forced aligner without a GPU: the TextGrid writer against the reader, the new exports against the header and
the binding, the argument errors raised on the host, the oracle's Viterbi (tests/align_oracle.py) against brute-force
enumeration, and the oracle's whole pipeline on the synthetic corpus (tests/align_corpus.py) against its known
boundaries.  The oracle restates this project's own algorithm; nothing here measures parity with another aligner."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import align_corpus as C
import align_oracle as O
from helpers import ROOT

import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib, aligner

# What the oracle pipeline reaches on the corpus with the default parameters: the mean absolute error, in frames, of the
# start and end of every phone that is not a silence.  A boundary at x frames is at best written as ceil(x) (a state
# starts with the first frame centred past the boundary): 0.5 frames on average from the convention alone, the rest is
# the frame that straddles the boundary under the 4-frame window.
# Round N_ITERS changed no duration.  That is more than the aligner's default cap of 8 rounds, so the tests fit with
# a cap of N_ITERS + 6.
E_O = 0.906
N_ITERS = 14


# ------------------------------------------------------------------ TextGrid
def test_write_textgrid_round_trip(tmp_path):
    words = [(0.0, 0.1, ""), (0.1, 0.58049886621315194, 'say "hi"'), (0.58049886621315194, 0.7, "<unk>"), (0.7, 0.9, "")]
    phones = [(0.0, 0.1, "sil"), (0.1, 3 * 256 / 22050, "s"), (3 * 256 / 22050, 0.58049886621315194, "ei"),
              (0.58049886621315194, 0.7, "spn"), (0.7, 0.9, "sil")]
    path = str(tmp_path / "a.TextGrid")
    mg.write_textgrid(path, {"words": words, "phones": phones}, 0.9)
    full = mg.read_textgrid(path, include_empty_intervals=True)
    assert list(full) == ["words", "phones"] and full["words"] == words and full["phones"] == phones
    kept = mg.read_textgrid(path)
    assert kept["words"] == words[1:3] and kept["phones"] == phones
    # a frame boundary comes back as its frame, and a word's end as its last phone's end, the same float
    assert round(kept["phones"][1][1] * 22050 / 256) == 3 and kept["words"][0][1] == kept["phones"][2][1]
    mg.write_textgrid(path, [("phones", [(np.float64(0.0), np.float32(0.5), "a")])], np.float64(0.5))
    assert mg.read_textgrid(path) == {"phones": [(0.0, 0.5, "a")]}
    with pytest.raises(mg.preprocessor.TextGridError):
        mg.write_textgrid(path, {"phones": [(0.0, 0.5, "a\nb")]}, 0.5)


def test_written_textgrid_feeds_get_alignment(tmp_path):
    """Interval lists as the aligner builds them: get_alignment finds the frame durations, the word grouping, and
    counts spn as a word of its own."""
    hop, sr = 256, 22050
    units = [(0, 1, "sil", -1, ""), (1, 2, "k", 0, "ka"), (3, 2, "a", 0, "ka"), (5, 1, "sil", -1, ""),
             (6, 2, "spn", 1, "<unk>"), (8, 1, "sil", -1, ""), (9, 2, "o", 2, "o"), (11, 1, "sil", -1, "")]
    dur = np.array([3, 2, 2, 1, 4, 0, 3, 2, 4, 1, 2, 5])
    phones, words, xmax = aligner.intervals(units, dur, 27 * hop - 10, hop, sr)
    assert [p for _, _, p in phones] == ["sil", "k", "a", "spn", "sp", "o", "sil"]
    assert [w for _, _, w in words] == ["", "ka", "<unk>", "", "o", ""]
    assert phones[0][0] == 0.0 and phones[-1][1] == xmax == (27 * hop - 10) / sr
    assert phones == O.intervals(units, dur, 27 * hop - 10, hop, sr)[0]
    assert words == O.intervals(units, dur, 27 * hop - 10, hop, sr)[1]
    path = str(tmp_path / "b.TextGrid")
    mg.write_textgrid(path, {"words": words, "phones": phones}, xmax)
    tiers = mg.read_textgrid(path)
    ph, d, start, end, ppw = mg.preprocessor.get_alignment(tiers["phones"], tiers["words"], sr, hop)
    assert ph == ["k", "a", "spn", "sp", "o"] and d == [4, 5, 5, 4, 3] and ppw == [2, 1, 1, 1]
    assert start == 3 * hop / sr and end == 24 * hop / sr


def test_a_last_frame_that_starts_at_the_end_of_the_signal():
    """n_samples a multiple of hop: frame n_samples / hop starts at xmax.  A last silence of that frame alone is not
    written; a last phone of that frame alone has no length, and the row has no alignment.  Both restatements agree."""
    hop, sr, n = 256, 22050, 10 * 256      # 11 frames
    units = [(0, 1, "sil", -1, ""), (1, 1, "a", 0, "a"), (2, 1, "sil", -1, ""), (3, 1, "o", 1, "o"),
             (4, 1, "sil", -1, "")]
    for fn in (aligner.intervals, O.intervals):
        phones, words, xmax = fn(units, np.array([2, 4, 0, 4, 1]), n, hop, sr)
        assert [p for _, _, p in phones] == ["sil", "a", "o"] and phones[-1][1] == xmax == n / sr
        assert phones[-1][0] == 6 * hop / sr and words[-1] == (6 * hop / sr, xmax, "o")
        assert all(s < e for s, e, _ in phones + words)
        assert fn(units, np.array([2, 4, 4, 1, 0]), n, hop, sr) is None
        phones, _, _ = fn(units, np.array([2, 4, 0, 3, 2]), n, hop, sr)      # two frames of silence: it has length
        assert [p for _, _, p in phones] == ["sil", "a", "o", "sil"] and phones[-1][:2] == (9 * hop / sr, xmax)
    assert aligner.intervals(units, np.array([2, 4, 0, 4, 1]), n, hop, sr) == \
        O.intervals(units, np.array([2, 4, 0, 4, 1]), n, hop, sr)


# ------------------------------------------------------------------ exports and host-side errors
def test_exports_are_in_the_header_and_the_binding():
    header = open(os.path.join(ROOT, "include", "mixgan_hip.h")).read()
    for name in ("mg_align_emissions", "mg_align_viterbi", "mg_align_viterbi_workspace_bytes", "mg_align_stats"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(mg.library_path()), name)
    for name, value in (("MG_ALIGN_MAX_D", 128), ("MG_ALIGN_MAX_G", 1024), ("MG_ALIGN_MAX_S", 2048),
                        ("MG_ALIGN_MAX_T", 4096)):
        assert getattr(_lib, name) == value and re.search(r"#define %s %d\b" % (name, value), header)
    for name in ("emissions", "viterbi_align", "gaussian_stats", "read_lexicon", "write_textgrid"):
        assert callable(getattr(mg, name))
    assert issubclass(mg.AlignGeometryError, mg.MixganHipError) and issubclass(mg.AlignGeometryError, NotImplementedError)
    assert "align.hip" in open(os.path.join(ROOT, "mixgan-tts_amd", "csrc", "Makefile")).read()


def test_c_abi_argument_errors_return_before_any_launch():
    """Null pointers, limits and the workspace: each refused on the host, so no GPU is needed (the non-null pointers
    are never followed)."""
    L = mg.lib()
    p = ctypes.c_void_p(4096)
    assert L.mg_align_emissions(None, p, 1, 4, 8, p, p, p, 2, p, None) == _lib.MG_ERR_ARG
    assert L.mg_align_emissions(p, p, 1, 4, 8, p, p, p, 2, None, None) == _lib.MG_ERR_ARG
    for B, T, D, G in ((0, 4, 8, 2), (1, 0, 8, 2), (1, 4, 0, 2), (1, 4, 129, 2), (1, 4, 8, 0), (1, 4, 8, 1025),
                       (65536, 64, 8, 2)):
        assert L.mg_align_emissions(p, p, B, T, D, p, p, p, G, p, None) == _lib.MG_ERR_SHAPE, (B, T, D, G)
    assert L.mg_align_viterbi_workspace_bytes(3, 10, 17) == 3 * 10 * 3 * 2       # two bits a state, in half-words
    assert L.mg_align_viterbi_workspace_bytes(16, 4096, 2048) == 16 * 4096 * 512
    assert L.mg_align_viterbi_workspace_bytes(0, 10, 17) == 0 == L.mg_align_viterbi_workspace_bytes(1, 10, 0)

    def vit(ll=p, ok=p, B=2, T=10, S=17, G=5, ws=p, nbytes=2 * 10 * 3 * 2):
        return L.mg_align_viterbi(ll, p, p, p, p, B, T, S, G, p, p, ok, ws, nbytes, None)

    assert vit(ll=None) == vit(ok=None) == _lib.MG_ERR_ARG
    assert vit(B=0) == vit(T=0) == vit(T=4097) == vit(S=0) == vit(S=2049) == vit(G=0) == vit(G=1025) == _lib.MG_ERR_SHAPE
    assert vit(ws=None) == vit(nbytes=2 * 10 * 3 * 2 - 1) == _lib.MG_ERR_WORKSPACE
    assert L.mg_align_stats(None, p, p, 2, 8, p, p, None) == L.mg_align_stats(p, p, p, 2, 8, p, None, None) \
        == _lib.MG_ERR_ARG
    for G, D in ((0, 8), (1025, 8), (2, 0), (2, 129)):
        assert L.mg_align_stats(p, p, p, G, D, p, p, None) == _lib.MG_ERR_SHAPE, (G, D)


def test_wrapper_errors_are_raised_on_the_host():
    z = torch.zeros
    with pytest.raises(mg.AlignGeometryError, match="D=129"):
        mg.emissions(z(1, 4, 129), z(1), z(2, 129), z(2, 129), z(2))
    with pytest.raises(mg.AlignGeometryError, match="G=1025"):
        mg.emissions(z(1, 4, 3), z(1), z(1025, 3), z(1025, 3), z(1025))
    with pytest.raises(ValueError, match="expected x"):
        mg.emissions(z(1, 4, 3), z(1), z(2, 4), z(2, 4), z(2))
    seq, nf, ns = np.zeros((1, 4), np.int32), np.array([5]), np.array([4])
    with pytest.raises(mg.AlignGeometryError, match="adjacent"):
        mg.viterbi_align(z(1, 5, 2), seq, np.array([[1, 1, 0, 0]]), nf, ns)
    with pytest.raises(mg.AlignGeometryError, match="S=2049"):
        mg.viterbi_align(z(1, 5, 2), np.zeros((1, 2049), np.int32), np.zeros((1, 2049), np.uint8), nf, ns)
    with pytest.raises(mg.AlignGeometryError, match="T=4097"):
        mg.viterbi_align(z(1, 4097, 2), seq, np.zeros((1, 4), np.uint8), nf, ns)
    with pytest.raises(ValueError, match="outside"):
        mg.viterbi_align(z(1, 5, 2), seq + 2, np.zeros((1, 4), np.uint8), nf, ns)
    # two skippable states past the row's own states are nobody's neighbours
    if not torch.cuda.is_available():
        with pytest.raises(mg.MixganHipError, match="no CPU fallback"):
            mg.viterbi_align(z(1, 5, 2), seq, np.array([[1, 0, 1, 1]]), nf, np.array([3]))
        with pytest.raises(mg.MixganHipError, match="no CPU fallback"):
            mg.emissions(z(1, 4, 3), z(1), z(2, 3), z(2, 3), z(2))
        with pytest.raises(mg.MixganHipError, match="no CPU fallback"):
            mg.gaussian_stats(z(4, 3), z(4), 2)


def test_lexicon_and_state_sequences(tmp_path):
    lex = mg.read_lexicon(C.write_lexicon(str(tmp_path / "lexicon.txt")))
    assert lex == C.lexicon() and lex["kato"] == ["k", "a", "t", "o"]
    phones = aligner.phone_inventory(lex)
    assert phones == sorted(list(C.PHONES) + ["spn"])
    pid = {p: i for i, p in enumerate(phones)}
    seq, skip, units = aligner.state_sequence(["Kato", C.OOV], lex, pid, 3)
    oseq, oskip, ounits = O.state_sequence(["Kato", C.OOV], lex, phones, 3)
    assert (seq == oseq).all() and (skip == oskip).all() and units == ounits
    assert len(seq) == 1 + 4 * 3 + 1 + 3 + 1 and list(np.nonzero(skip)[0]) == [0, 13, 17]
    assert [u[2:] for u in units if u[3] == 1] == [("spn", 1, "<unk>")]
    assert aligner.transcript_words(' "Hello, world!"  (yes) ') == ["Hello", "world", "yes"]
    for T in (4, 16, 17, 33, 100):
        a, b = aligner.flat_start(skip, T), O.flat_start(skip, T)
        assert (a is None and b is None and T < 17) or ((a == b).all() and a.sum() == T and a[13] == 0)


def test_model_update_matches_the_oracle():
    rng = np.random.default_rng(3)
    count = np.array([40, 0, 5, 6, 17])
    s1 = rng.standard_normal((5, 7)) * count[:, None]
    s2 = (rng.random((5, 7)) + 1.5) * count[:, None]
    s2[4, 2] = s1[4, 2] ** 2 / 17      # a variance under the floor
    mean, var = aligner.update_model(s1, s2, count, 1e-2, 6)
    omean, ovar = O.update_model(s1, s2, count, 1e-2, 6)
    np.testing.assert_array_equal(mean, omean)
    np.testing.assert_array_equal(var, ovar)
    assert (mean[1] == mean[2]).all() and (var[1] == var[2]).all() and var[4, 2] == 1e-2 and (var >= 1e-2).all()
    for a, b in zip(aligner.model_tables(mean, var), O.tables(mean, var)):
        assert a.dtype == np.float32 and np.array_equal(a, b)


# ------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("S,T", [(1, 1), (1, 4), (2, 1), (2, 3), (3, 2), (3, 5), (4, 3), (4, 6)])
def test_oracle_viterbi_against_enumeration(S, T):
    """Every skip pattern without two adjacent skippable states: the oracle's score is the best path's, no path exists
    exactly when it says so, and where the best path is unique the durations are that path's."""
    rng = np.random.default_rng(100 * S + T)
    for skip in itertools.product((0, 1), repeat=S):
        if any(a and b for a, b in zip(skip, skip[1:])):
            continue
        for trial in range(4):
            e = rng.standard_normal((T, S)) if trial else np.round(rng.standard_normal((T, S)))      # trial 0: ties
            dur, score, ok = O.viterbi_row(e, np.array(skip))
            found = O.brute_force(e, skip)
            assert bool(ok) == bool(found), (skip, T)
            if not found:
                assert not dur.any() and score == -np.inf
                continue
            best = max(f[0] for f in found)
            assert abs(score - best) <= 1e-12 * max(1.0, abs(best)) and dur.sum() == T
            winners = [f[1] for f in found if f[0] == best]
            if len(winners) == 1 and trial:
                assert list(dur) == [winners[0].count(s) for s in range(S)]


def test_oracle_tie_rule_is_stay_then_advance_then_skip():
    dur, score, ok = O.viterbi_row(np.zeros((6, 5)), np.array([0, 1, 0, 1, 0]))
    # all paths tie: the last state is entered as late as can be, each time by the smallest jump that still arrives
    assert ok and score == 0.0 and dur.sum() == 6
    again = O.viterbi_row(np.zeros((6, 5)), np.array([0, 1, 0, 1, 0]))[0]
    assert (dur == again).all()
    # backtrace from the end prefers to have stayed: the end state holds every frame it can
    assert list(dur) == [1, 0, 1, 0, 4]


@pytest.fixture(scope="module")
def oracle_run():
    wavs = [C.signal(n) for n in C.NAMES]
    return O.fit_and_align(wavs, [u[1] for u in C.UTTERANCES], C.lexicon(), C.SR, C.HOP, C.N_MELS, C.FMIN, C.FMAX,
                           n_iters=N_ITERS + 6)


def test_corpus_is_what_its_docstring_says():
    total = 0
    for name in C.NAMES:
        phones, words, n = C.truth(name)
        assert 0.6 <= n / C.SR <= 1.2 and len(C.signal(name)) == n
        assert all((e - s) * C.SR >= 4 * C.HOP for s, e, _ in phones)
        assert ("sp" in [p for _, _, p in phones]) == (name == C.PAUSED)
        assert ("spn" in [p for _, _, p in phones]) == (name in C.WITH_OOV)
        assert words[-1][1] == phones[-1][1] and [w for _, _, w in words if w] != []
        total += 1
    assert total == 12 and len(C.PHONES) == 10 and C.OOV not in C.lexicon()


def test_oracle_pipeline_finds_the_known_boundaries(oracle_run):
    out, iters, (mean, var) = oracle_run
    assert iters == N_ITERS, "the oracle needed %d rounds" % iters
    errs = []
    for name, res in zip(C.NAMES, out):
        phones, words, xmax = res
        truth_ph, truth_w, n = C.truth(name)
        e = O.boundary_error(phones, truth_ph, C.SR, C.HOP)
        assert e is not None, name
        errs += e
        labels = [p for _, _, p in phones]
        assert ("sp" in labels) == (name == C.PAUSED) and ("spn" in labels) == (name in C.WITH_OOV)
        assert labels[0] == "sil" and labels[-1] == "sil" and "" not in labels
        assert [w for _, _, w in words if w] == [w if w.lower() in C.lexicon() else "<unk>"
                                                 for w in C.UTTERANCES[C.NAMES.index(name)][1]]
        assert xmax == n / C.SR and phones[-1][1] == xmax and words[-1][1] == xmax
    e_o = float(np.mean(errs))
    print("oracle: mean |boundary error| = %.4f frames over %d boundaries, worst %.3f" % (e_o, len(errs), max(errs)))
    assert e_o < 1.0
    assert abs(e_o - E_O) < 5e-4, "E_O is out of date: %.4f" % e_o
    assert (var >= 1e-2).all() and np.isfinite(mean).all()
