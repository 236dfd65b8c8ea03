"""GPU parity of the corpus builder (mixgan-tts_amd/preprocessor.py, corpusops.py, csrc/corpus.hip) against the
reference Preprocessor's outputs over the synthetic corpus of tests/preprocessor_corpus.py (fixtures of
tests/golden/make_golden_preprocessor.py).

Tolerances, none of them taken from what the code under test gives:
- prior, float64: relative 1e-9 where the golden is >= 1e-300, absolute 1e-300 below (the float64 lgamma form agrees
  with scipy to 5e-12 on a CPU; the device's lgamma / log are allowed two more decades);
- prior, float32: one float32 unit in the last place of float32(golden), subnormals included; padding exactly 0;
- pitch averages: relative 1e-12 (same operations, only the summation order over <= ~100 positive values differs);
- energy averages: relative 1e-6 (numpy's float32 pairwise mean is within log2(d) 2^-24 of the exact mean);
- mel and energy out of the STFT: what tests/test_gpu_audio.py holds them to (max-norm relative 1e-5 of exp(mel) and
  of energy, |log| difference 1e-4 where exp(mel) >= 1e-2); phoneme means are convex combinations of frame
  energies, so they inherit the max-norm bound, and the normalised values / stats.json entries the bound
  propagated through (x - mean) / std (see _z_tol).
"""
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import preprocessor_corpus as C
from helpers import golden as load_golden, GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEPT = [n for n in C.NAMES if n not in C.FILTERED]


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


@pytest.fixture(scope="module")
def golden():
    return load_golden("preprocessor")


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(GOLDEN, "preprocessor_manifest.json")) as f:
        return json.load(f)


def _i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def _prior_ref(golden, case):
    mel_len, n_phon, s = case
    rows, cols = C.prior_subgrid(mel_len, n_phon)
    return golden["prior/%d_%d_%g" % case], rows, cols


def _check_f64(out, ref, tag):
    assert out.dtype == np.float64 and out.shape == ref.shape and np.isfinite(out).all()
    big = ref >= 1e-300
    rel = float((np.abs(out - ref)[big] / ref[big]).max()) if big.any() else 0.0
    small = float(np.abs(out - ref)[~big].max()) if (~big).any() else 0.0
    print("prior f64 %s: max rel %.3e (golden >= 1e-300), max abs below %.3e" % (tag, rel, small))
    assert rel <= 1e-9 and small <= 1e-300
    return rel


def _ulps(a, b):
    """Distance in float32 units in the last place (subnormals included; both non-negative)."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# (cases in one batch, scaling, extra T, extra L): [800 x 100 | 37 x 5 | 3 x 1] takes the vector stores (L % 4 == 0);
# T and L beyond the longest item, odd L and the 613-frame item take the element stores and more padding
BATCHES = [([(800, 100, 1.0), (37, 5, 1.0), (3, 1, 1.0)], 1.0, 0, 0),
           ([(37, 5, 1.0), (800, 100, 1.0), (3, 1, 1.0)], 1.0, 1, 3),
           ([(37, 5, 1.0), (3, 1, 1.0)], 1.0, 0, 0),
           ([(3, 1, 1.0)], 1.0, 0, 0),
           ([(613, 87, 0.5)], 0.5, 0, 0),
           ([(613, 87, 0.5)], 0.5, 2, 1027 - 613)]


@pytest.mark.parametrize("k", range(len(BATCHES)))
def test_prior_float64_matches_reference(mg, golden, k):
    cases, s, dT, dL = BATCHES[k]
    T, L = max(c[1] for c in cases) + dT, max(c[0] for c in cases) + dL
    out = mg.attn_prior(_i32(c[1] for c in cases), _i32(c[0] for c in cases), T, L, s, torch.float64)
    assert out.shape == (len(cases), T, L) and out.dtype == torch.float64 and out.is_cuda
    out = out.cpu().numpy()
    for b, case in enumerate(cases):
        ref, rows, cols = _prior_ref(golden, case)
        _check_f64(out[b][np.ix_(rows, cols)], ref, "%s in batch %d" % (case, k))
        assert (out[b, case[1]:] == 0).all() and (out[b, :, case[0]:] == 0).all()


@pytest.mark.parametrize("k", range(len(BATCHES)))
def test_prior_float32_within_one_ulp_and_padding_zero(mg, golden, k):
    cases, s, dT, dL = BATCHES[k]
    T, L = max(c[1] for c in cases) + dT, max(c[0] for c in cases) + dL
    out = mg.attn_prior(_i32(c[1] for c in cases), _i32(c[0] for c in cases), T, L, s)
    assert out.shape == (len(cases), T, L) and out.dtype == torch.float32
    out = out.cpu().numpy()
    for b, case in enumerate(cases):
        ref, rows, cols = _prior_ref(golden, case)
        d = _ulps(np.ascontiguousarray(out[b][np.ix_(rows, cols)]), ref.astype(np.float32))
        print("prior f32 %s in batch %d: max %d ulp, %d of %d elements differ" % (case, k, d.max(), (d > 0).sum(), d.size))
        assert d.max() <= 1
        assert (out[b, case[1]:] == 0).all() and (out[b, :, case[0]:] == 0).all()
    # int64 length vectors (what the loader holds) give the same table
    out64 = mg.attn_prior(_i32(c[1] for c in cases).long(), _i32(c[0] for c in cases).long(), T, L, s)
    assert np.array_equal(out64.cpu().numpy(), out)


def test_prior_far_tails_against_scipy(mg):
    """Rows whose tails fall below the float64 normal range (the golden tables stay above 1e-135): the function the
    reference calls, evaluated here, same tolerance."""
    from scipy.stats import betabinom
    n, T, s = 3000, 400, 1.0
    out = mg.attn_prior(_i32([T]), _i32([n]), T, n, s, torch.float64)[0].cpu().numpy()
    x = np.arange(n)
    rows = [0, 1, 7, 199, 200, 398, 399]
    ref = np.stack([betabinom(n, s * (i + 1), s * (T - i)).pmf(x) for i in rows])
    assert ref.min() < 1e-300
    _check_f64(out[rows], ref, "far tails n=%d T=%d" % (n, T))


def test_wrappers_reject_cpu_tensors_and_unvoiced_pitch(mg):
    with pytest.raises(mg.MixganHipError):
        mg.attn_prior(torch.tensor([3], dtype=torch.int32), torch.tensor([5], dtype=torch.int32), 3, 5)
    with pytest.raises(mg.MixganHipError):
        mg.phoneme_average(torch.zeros(1, 8), torch.ones(1, 2, dtype=torch.int32), torch.tensor([8]), torch.tensor([2]),
                           "energy")
    f0 = torch.zeros(2, 8, dtype=torch.float64, device=DEV)
    f0[0, 2:5] = 100.0
    f0[1, 3] = 100.0          # one voiced frame: the builder filters such an utterance out before the call
    with pytest.raises(mg.MixganHipError):
        mg.phoneme_average(f0, torch.full((2, 2), 4, dtype=torch.int32, device=DEV), _i32([8, 8]), _i32([2, 2]), "pitch")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("corpus"))
    raw, pre = C.write_corpus(root)
    return raw, pre


def _builder(mg, raw, pre, feature="phoneme_level", normalization=True, **kw):
    return mg.Preprocessor(*C.configs(raw, pre, feature, normalization), pitch_fn=C.pitch_fn, load_wav=C.load_wav, **kw)


def _rel_elementwise(out, ref, tol, tag):
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape and out.dtype == ref.dtype, (tag, out.shape, ref.shape, out.dtype, ref.dtype)
    assert np.isfinite(out).all()
    err = np.abs(out.astype(np.float64) - ref.astype(np.float64))
    nz = ref != 0
    rel = float((err[nz] / np.abs(ref[nz].astype(np.float64))).max()) if nz.any() else 0.0
    print("%s: max rel %.3e" % (tag, rel))
    assert (out[~nz] == 0).all(), tag
    assert rel <= tol, (tag, rel)


def test_phoneme_average_pitch_matches_reference(mg, golden, corpus):
    raw, pre = corpus
    b = _builder(mg, raw, pre)
    items = [b.prepare_utterance(C.SPEAKER_OF[n], n) for n in KEPT]
    assert b.prepare_utterance("spkB", "b01") is None          # at most one voiced frame
    T, L = max(len(it["duration"]) for it in items), max(len(it["pitch"]) for it in items)
    f0, dur = np.zeros((len(items), L)), np.zeros((len(items), T), dtype=np.int32)
    for k, it in enumerate(items):
        f0[k, :len(it["pitch"])] = it["pitch"]
        dur[k, :len(it["duration"])] = it["duration"]
        assert (it["pitch"] == 0).any()
    out = mg.phoneme_average(torch.from_numpy(f0).to(DEV), torch.from_numpy(dur).to(DEV),
                             _i32(len(it["pitch"]) for it in items), _i32(len(it["duration"]) for it in items), "pitch")
    assert out.dtype == torch.float64 and out.shape == (len(items), T)
    out = out.cpu().numpy()
    for k, n in enumerate(KEPT):
        p = len(items[k]["duration"])
        _rel_elementwise(out[k, :p], golden["raw/pitch/" + n], 1e-12, "pitch " + n)
        assert (out[k, p:] == 0).all()
    assert list(items[KEPT.index(C.ALIASED)]["duration"][:2]) == [0, 0]      # the in-place aliasing case was in the batch


def test_phoneme_average_energy_matches_reference(mg, golden, manifest):
    frames = [golden["frame/energy/" + n] for n in KEPT]
    durs = [manifest["alignment"][n]["durations"] for n in KEPT]
    T, L = max(map(len, durs)), max(map(len, frames))
    en, dur = np.zeros((len(KEPT), L), dtype=np.float32), np.zeros((len(KEPT), T), dtype=np.int32)
    for k in range(len(KEPT)):
        assert frames[k].dtype == np.float32 and len(frames[k]) == sum(durs[k])
        en[k, :len(frames[k])] = frames[k]
        dur[k, :len(durs[k])] = durs[k]
    out = mg.phoneme_average(torch.from_numpy(en).to(DEV), torch.from_numpy(dur).to(DEV), _i32(map(len, frames)),
                             _i32(map(len, durs)), "energy")
    assert out.dtype == torch.float32
    out = out.cpu().numpy()
    for k, n in enumerate(KEPT):
        _rel_elementwise(out[k, :len(durs[k])], golden["raw/energy/" + n], 1e-6, "energy " + n)
        assert (out[k, len(durs[k]):] == 0).all()
    assert durs[KEPT.index(C.ALIASED)][:2] == [0, 0]


def _mel_check(ours, ref, tag):
    assert ours.dtype == np.float32 and ours.shape == ref.shape, (tag, ours.shape, ref.shape)
    eo, er = np.exp(ours.astype(np.float64)), np.exp(ref.astype(np.float64))
    e_mel = float(np.abs(eo - er).max() / er.max())
    big = er >= 1e-2
    e_log = float(np.abs(ours.astype(np.float64) - ref)[big].max()) if big.any() else 0.0
    print("%s: mel %.2e log %.2e" % (tag, e_mel, e_log))
    assert e_mel <= 1e-5 and e_log <= 1e-4


def _z_tol(e_max, std, z_max):
    """Bound on a normalised energy value: frame energies within 1e-5 e_max (test_gpu_audio.py) give phoneme means,
    their mean within 1e-5 e_max and their std within 2e-5 e_max; through z = (x - mean) / std that is
    (|dx| + |dmean|) / std + |z| |dstd| / std."""
    return 1e-5 * e_max / std * (2 + 2 * z_max)


def _compare_tree(pre, golden, man, tag):
    e_max = max(float(golden["frame/energy/" + n].max()) for n in KEPT)
    st, phoneme = man["stats"], tag != "frame"
    norm = tag == "main"
    e_std = st["energy"][3]
    with open(os.path.join(pre, "stats.json")) as f:
        stats = json.load(f)
    for n in KEPT:
        load = lambda kind: np.load(os.path.join(pre, kind, "%s-%s-%s.npy" % (C.SPEAKER_OF[n], kind, n)))  # noqa: E731
        key = lambda kind: "%s/%s/%s" % (tag, kind, n)                                                       # noqa: E731
        pitch, energy = load("pitch"), load("energy")
        # pitch: relative 1e-12 on the averaged values; normalised ones move by the 1e-10 allowed on mean and std
        ref = golden[key("pitch")]
        assert pitch.dtype == ref.dtype and pitch.shape == ref.shape
        if norm:
            err = float(np.abs(pitch - ref).max())
            print("%s pitch %s: max abs %.3e" % (tag, n, err))
            assert err <= 1e-9
        else:
            _rel_elementwise(pitch, ref, 1e-12 if phoneme else 0.0, "%s pitch %s" % (tag, n))
        ref = golden[key("energy")]
        assert energy.dtype == ref.dtype and energy.shape == ref.shape, (energy.dtype, ref.dtype)
        err = float(np.abs(energy.astype(np.float64) - ref).max())
        tol = _z_tol(e_max, e_std, float(np.abs(ref).max())) if norm else 1e-5 * e_max
        print("%s energy %s: max abs %.3e (bound %.3e)" % (tag, n, err, tol))
        assert err <= tol
        if tag != "main":
            continue
        _mel_check(load("mel"), golden[key("mel")], "mel " + n)
        for kind in ("duration", "phones_per_word"):
            got = load(kind)
            assert got.dtype == golden[key(kind)].dtype and np.array_equal(got, golden[key(kind)]), (kind, n)
        prior = load("attn_prior")
        assert prior.shape == golden[key("attn_prior")].shape
        _check_f64(prior, golden[key("attn_prior")], "file " + n)
    for name in ("train", "val", "filtered_out"):
        with open(os.path.join(pre, name + ".txt"), encoding="utf-8") as f:
            assert f.read() == man["texts"][name], name
    with open(os.path.join(pre, "speakers.json")) as f:
        assert json.load(f) == man["speakers"]
    # the reference's key order (the manifest is stored with sorted keys, so the order is stated here)
    assert list(stats) == ["pitch", "energy", "spec_min", "spec_max", "max_seq_len"] and set(st) == set(stats)
    assert stats["max_seq_len"] == st["max_seq_len"]
    if norm:
        p, q = stats["pitch"], st["pitch"]
        assert abs(p[2] - q[2]) <= 1e-10 * abs(q[2]) and abs(p[3] - q[3]) <= 1e-10 * q[3]
        assert abs(p[0] - q[0]) <= 1e-9 and abs(p[1] - q[1]) <= 1e-9
        p, q = stats["energy"], st["energy"]
        assert abs(p[2] - q[2]) <= 1e-5 * e_max and abs(p[3] - q[3]) <= 2e-5 * e_max
        tol = _z_tol(e_max, e_std, max(abs(q[0]), abs(q[1])))
        assert abs(p[0] - q[0]) <= tol and abs(p[1] - q[1]) <= tol
    else:
        assert stats["pitch"][2:] == [0.0, 1.0] and stats["energy"][2:] == [0.0, 1.0]
    # per-bin mel extremes: the max-norm bound of the mel, in the linear domain
    m_max = max(float(np.exp(golden["main/mel/" + n].astype(np.float64)).max()) for n in KEPT)
    for k in ("spec_min", "spec_max"):
        assert len(stats[k]) == C.N_MELS
        assert np.abs(np.exp(np.array(stats[k])) - np.exp(np.array(st[k]))).max() <= 1e-5 * m_max, k


@pytest.mark.parametrize("tag,feature,norm,batch", [("main", "phoneme_level", True, 4), ("raw", "phoneme_level", False, 16),
                                                    ("frame", "frame_level", False, 1)])
def test_build_from_path_matches_reference(mg, golden, manifest, tmp_path, tag, feature, norm, batch):
    raw, pre = C.write_corpus(str(tmp_path))
    random.seed(C.SHUFFLE_SEED)
    ret = _builder(mg, raw, pre, feature, norm, batch_utterances=batch).build_from_path()
    assert ret == manifest[tag]["returned"]
    _compare_tree(pre, golden, manifest[tag], tag)


def test_pre_defined_validation_set_is_honoured(mg, tmp_path):
    raw, pre = C.write_corpus(str(tmp_path))
    with open(os.path.join(pre, "val.txt"), "w", encoding="utf-8") as f:
        f.write("b02|spkB|{x}|x\nb01|spkB|{x}|x\n")
    random.seed(C.SHUFFLE_SEED)
    assert _builder(mg, raw, pre).build_from_path() == []
    names = lambda fn: [ln.split("|")[0] for ln in open(os.path.join(pre, fn), encoding="utf-8")]  # noqa: E731
    assert names("val.txt") == ["b02"] and sorted(names("train.txt")) == sorted(n for n in KEPT if n != "b02")
    assert names("filtered_out.txt") == ["b01\n"]


def test_dataset_device_prior_agrees_with_disk(mg, tmp_path):
    """The written tree through data.Dataset in both attn_prior modes, through to_device and through PrefetchLoader:
    every slot equal, the prior slot within one float32 ulp."""
    from mixgan_tts_amd import data as D
    raw, pre = C.write_corpus(str(tmp_path))
    random.seed(C.SHUFFLE_SEED)
    pc, mc, tc = C.configs(raw, pre)
    _builder(mg, raw, pre).build_from_path()
    symbols = {}
    t2s = lambda text, cleaners: [symbols.setdefault(p, len(symbols) + 1) for p in text.strip("{}").split()]  # noqa: E731
    args = types.SimpleNamespace(model="naive")
    disk = D.Dataset("train.txt", args, pc, mc, tc, sort=True, text_to_sequence=t2s)
    os.rename(os.path.join(pre, "attn_prior"), os.path.join(pre, "attn_prior_moved"))
    try:
        dev = D.Dataset("train.txt", args, pc, mc, tc, sort=True, text_to_sequence=t2s, attn_prior="device")
        dev_items = [dev[i] for i in range(len(dev))]
        smp = D.RankShardSampler(len(dev), len(dev), shuffle=False)
        loaded = list(D.PrefetchLoader(dev, smp, DEV))
        torch.cuda.synchronize()
    finally:
        os.rename(os.path.join(pre, "attn_prior_moved"), os.path.join(pre, "attn_prior"))
    a = [D.to_device(b, DEV) for b in disk.collate_fn([disk[i] for i in range(len(disk))])]
    raw_b = dev.collate_fn(dev_items)
    assert all(b[D.PRIOR_SLOT] is None for b in raw_b)
    with pytest.raises(ValueError):
        D.to_device(raw_b[0], DEV)
    for other in ([D.to_device(b, DEV, prior_scaling=dev.prior_scaling) for b in raw_b], loaded[0]):
        assert len(a) == len(other) >= 1
        for x, y in zip(a, other):
            assert len(x) == len(y) == 17
            for j, (u, v) in enumerate(zip(x, y)):
                if j == D.PRIOR_SLOT:
                    assert v.dtype == torch.float32 and v.shape == u.shape and v.is_cuda
                    d = _ulps(np.ascontiguousarray(v.cpu().numpy()), np.ascontiguousarray(u.cpu().numpy()))
                    print("loader prior: max %d ulp" % d.max())
                    assert d.max() <= 1
                elif torch.is_tensor(u):
                    assert u.dtype == v.dtype and torch.equal(u, v), j
                else:
                    assert np.all(np.asarray(u) == np.asarray(v)), j


def _in_place_average(values, dur, pitch):
    """numpy restatement of preprocessor.py:311-341 for one utterance: interp1d's linear fill (numpy's interp with the
    end values held), then the in-place segment means."""
    v = values.copy()
    if pitch:
        nz = np.where(v != 0)[0]
        v = np.interp(np.arange(len(v)), nz, v[nz])
    pos = 0
    for i, d in enumerate(dur):
        v[i] = np.mean(v[pos:pos + d]) if d > 0 else 0
        pos += d
    return v[:len(dur)]


@pytest.mark.parametrize("kind", ["pitch", "energy"])
def test_phoneme_average_at_corpus_shapes(mg, kind):
    """Utterances of 1000 - 4096 frames and 300 - 2048 phonemes, where a thread scans several phonemes and frames:
    unvoiced runs longer than a thread's chunk, and two utterances whose leading zero-length phones make the in-place
    loop read its own results (one of them for every segment).  Reference: the numpy restatement above; same bounds
    as against the golden files (pitch relative 1e-12, energy 1e-6)."""
    rng = np.random.default_rng(42)
    shapes = [(3000, 400), (4096, 2048), (1000, 300)]
    durs = []
    for u, (L, T) in enumerate(shapes):
        d = np.zeros(T, dtype=np.int64)
        lead = (0, 600, 5)[u]                                   # zero-length phones in front
        live = rng.permutation(np.arange(lead, T))[:min(T - lead, L // 2)]
        d[live] = 1
        for _ in range(L - int(d.sum())):                       # spread the remaining frames
            d[live[int(rng.integers(len(live)))]] += 1
        assert d.sum() == L
        durs.append(d)
    pos1 = np.concatenate([[0], np.cumsum(durs[1])[:-1]])
    assert ((pos1 < np.arange(len(pos1))) & (durs[1] > 0)).sum() > 256      # aliased well beyond one segment
    Lm, Tm = max(s[0] for s in shapes), max(s[1] for s in shapes)
    dt = np.float64 if kind == "pitch" else np.float32
    vals, dur = np.zeros((len(shapes), Lm), dtype=dt), np.zeros((len(shapes), Tm), dtype=np.int32)
    for u, (L, T) in enumerate(shapes):
        x = 100.0 + 50.0 * np.sin(np.arange(L) / 23.0 + u) + rng.standard_normal(L)
        if kind == "pitch":
            x[:37] = 0.0
            x[L - 41:] = 0.0
            for start in rng.integers(50, L - 100, 12):
                x[start:start + int(rng.integers(1, 45))] = 0.0
        vals[u, :L] = x.astype(dt)
        dur[u, :T] = durs[u]
    out = mg.phoneme_average(torch.from_numpy(vals).to(DEV), torch.from_numpy(dur).to(DEV), _i32(s[0] for s in shapes),
                             _i32(s[1] for s in shapes), kind).cpu().numpy()
    for u, (L, T) in enumerate(shapes):
        ref = _in_place_average(vals[u, :L], durs[u], kind == "pitch")
        _rel_elementwise(out[u, :T], ref.astype(dt), 1e-12 if kind == "pitch" else 1e-6, "%s %dx%d" % (kind, L, T))
        assert (out[u, T:] == 0).all()


def test_multi_speaker_embeddings_are_written_and_present_speakers_skipped(mg, tmp_path, monkeypatch):
    """preprocessor.py:66-68, 111-118, 149-165 with a stub embedder: one mean [1, 512] float32 file per speaker from
    the embeddings of the whole (untrimmed) wav of every kept utterance; a speaker whose file exists is left alone."""
    from mixgan_tts_amd import preprocessor as P
    calls = []

    class StubEmbedder:
        def __init__(self, config):
            assert config["preprocessing"]["speaker_embedder"] == "DeepSpeaker"

        def __call__(self, wav):
            calls.append(len(wav))
            return np.full((1, 512), np.float32(len(wav)) / 1000, dtype=np.float32)

    monkeypatch.setattr(P, "PreDefinedEmbedder", StubEmbedder)
    raw, pre = C.write_corpus(str(tmp_path))
    pc, mc, tc = C.configs(raw, pre)
    pc["preprocessing"]["speaker_embedder"], mc["multi_speaker"] = "DeepSpeaker", True
    os.makedirs(os.path.join(pre, "spker_embed"))
    present = np.full((1, 512), 7.0, dtype=np.float32)
    np.save(os.path.join(pre, "spker_embed", "spkB-spker_embed.npy"), present)
    random.seed(C.SHUFFLE_SEED)
    mg.Preprocessor(pc, mc, tc, pitch_fn=C.pitch_fn, load_wav=C.load_wav, batch_utterances=2).build_from_path()
    assert sorted(os.listdir(os.path.join(pre, "spker_embed"))) == ["spkA-spker_embed.npy", "spkB-spker_embed.npy"]
    assert np.array_equal(np.load(os.path.join(pre, "spker_embed", "spkB-spker_embed.npy")), present)
    lens = [len(C.signal(n)) for n in ("a01", "a02", "a03")]
    assert calls == lens          # spkA's three utterances only, the whole signals
    got = np.load(os.path.join(pre, "spker_embed", "spkA-spker_embed.npy"))
    want = np.mean([np.full((1, 512), np.float32(n) / 1000, dtype=np.float32) for n in lens], axis=0)
    assert got.dtype == np.float32 and got.shape == (1, 512) and np.array_equal(got, want)
