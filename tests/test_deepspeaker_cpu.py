"""DeepSpeaker speaker embedder, CPU side: the test restatement (tests/deepspeaker_ref.py) against a run of the real
reference front end (tests/golden/deepspeaker.npz, made by tests/golden/make_golden_deepspeaker.py), the native
module's weight names / shapes / layer order against the recorded Keras graph, the TF 'same' padding rule, the
device-agnostic trim against numpy, and save_speaker_embeddings through data.Dataset."""
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import deepspeaker_ref as R
from helpers import golden, GOLDEN

import mixgan_tts_amd  # noqa: F401  (alias module)
from mixgan_tts_amd import speaker_embedder as S
from mixgan_tts_amd import data as D


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "deepspeaker_manifest.json")) as f:
        return golden("deepspeaker"), json.load(f)


def test_restatement_front_end_matches_reference(fixture):
    g, man = fixture
    assert man["nfft"] == S.calculate_nfft(man["sample_rate"], man["win_length"] / man["sample_rate"]) == 1024
    random.seed(man["seed"])
    for sig in man["signals"]:
        x = g[sig["name"]]
        assert (sig["start"], sig["end"]) == R.trim(x)
        m = R.fbank_features(x[sig["start"]:sig["end"]])
        assert len(m) == sig["frames"] == S.num_frames(sig["end"] - sig["start"], 551, 221)
        # the crop the reference drew from the same seeded global random, in the same order
        r = random.choice(range(0, len(m) - R.NUM_FRAMES + 1)) if len(m) >= R.NUM_FRAMES else -1
        assert r == sig["offset"]
        ref = g[sig["name"] + "_input"][:, :, 0]
        got = R.model_input(x, max(r, 0))
        assert got.dtype == np.float32 and got.shape == ref.shape == (160, 64)
        assert np.abs(got.astype(np.float64) - ref).max() <= 1e-12, sig["name"]
        if r < 0:
            assert not ref[len(m):].any()


def test_trim_bounds_equal_numpy_percentile(fixture):
    g, man = fixture
    rng = np.random.default_rng(3)
    items = [g[s["name"]] for s in man["signals"]]
    for n in (2, 3, 7, 20, 21, 101, 1000, 4097):
        items.append((rng.standard_normal(n) * rng.uniform(0.01, 1)).astype(np.float32))
        items.append(np.round(rng.standard_normal(n) * 4) / 4)  # ties at the threshold, float64
    for dt in (np.float32, np.float64):
        its = [a for a in items if a.dtype == dt]
        L = max(len(a) for a in its)
        audio = torch.zeros(len(its), L, dtype=torch.float32 if dt == np.float32 else torch.float64)
        for i, a in enumerate(its):
            audio[i, :len(a)] = torch.from_numpy(a)
            audio[i, len(a):] = 5.0  # padding past the length must not count
        first, last, found = S.trim_bounds(audio, [len(a) for a in its])
        for i, a in enumerate(its):
            e = np.abs(a)
            idx = np.where(e > np.percentile(e, 95))[0]
            assert bool(found[i]) == (len(idx) > 0)
            if len(idx):
                assert (int(first[i]), int(last[i])) == (int(idx[0]), int(idx[-1])), (dt, len(a))


def test_native_weight_names_shapes_and_order_match_recorded_graph(fixture):
    _, man = fixture
    convs = [(l["name"], l["filters"], l["kernel"], l["strides"]) for l in man["graph"] if l["type"] == "Conv2D"]
    assert all(l["padding"] == "same" and l["use_bias"] and l["activation"] is None
               for l in man["graph"] if l["type"] == "Conv2D")
    assert [(n, f, [k, k], [s, s]) for n, f, k, s in S.layer_specs()] == convs
    bns = [l for l in man["graph"] if l["type"] == "BatchNormalization"]
    assert [l["name"] for l in bns] == [n + "_bn" for n, _, _, _ in S.layer_specs()]
    assert all(l["epsilon"] == S.BN_EPS for l in bns)
    # every conv is followed by its BN and a clipped ReLU; identity blocks add, then clip again
    seq = [l["type"] for l in man["graph"]]
    assert seq[0] == "Input" and man["graph"][0]["batch_shape"] == [None, 160, 64, 1]
    assert seq.count("Add") == 12
    for i, l in enumerate(man["graph"]):
        if l["type"] == "Conv2D":
            assert seq[i + 1:i + 3] == ["BatchNormalization", "Lambda"]
            assert man["graph"][i + 2]["name"].startswith("clipped_relu_")
            if l["name"].endswith("_2b"):
                assert seq[i + 3:i + 5] == ["Add", "Lambda"]
    tail = man["graph"][-4:]
    assert tail[0]["type"] == "Reshape" and tail[0]["target_shape"] == [-1, 2048]
    assert tail[1]["name"] == "average" and tail[3]["name"] == "ln"
    assert tail[2]["name"] == "affine" and tail[2]["units"] == S.EMBED_DIM and tail[2]["activation"] is None
    shapes = S.keras_weight_shapes()
    W = R.seeded_weights()
    assert list(shapes) == [k for k in shapes if k in W] and set(shapes) == set(W)
    assert all(W[k].shape == shp for k, shp in shapes.items())


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 10, 20, 40, 63, 64, 80, 160])
@pytest.mark.parametrize("k,s", [(5, 2), (3, 1)])
def test_tf_same_padding_rule(n, k, s):
    out, before, after = S.tf_same_padding(n, k, s)
    assert out == -(-n // s)
    # the padded input covers exactly the taps of the out outputs
    assert (n + before + after - k) // s + 1 == out and before + after == max((out - 1) * s + k - n, 0)
    if s == 2 and k == 5:
        assert (before, after) == ((1, 2) if n % 2 == 0 else (2, 2)) or n < 3
    assert (before, after) == R.tf_same(n, k, s)[1:]
    if s == 1:
        assert (before, after) == (1, 1)


def test_network_sizes_follow_the_padding_rule():
    h, w = 160, 64
    for _ in R.FILTERS:
        h, w = S.tf_same_padding(h, 5, 2)[0], S.tf_same_padding(w, 5, 2)[0]
    assert (h, w) == (10, 4) and w * R.FILTERS[-1] == 2048


def test_seeded_weights_keep_activations_in_range():
    W = R.seeded_weights()
    sat = R.saturation(R._calibration_inputs(3, seed=11), W)
    for name, (z, top) in sat.items():
        assert z < 0.8 and top < 0.01, (name, z, top)


def test_save_speaker_embeddings_loads_through_dataset(tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(0)
    embeds = {"spkA": [rng.standard_normal((1, 512)).astype(np.float32) for _ in range(3)],
              "spkB": [torch.from_numpy(rng.standard_normal((1, 512)).astype(np.float32))]}
    for spk, es in embeds.items():
        S.save_speaker_embeddings(d, spk, es)
    with open(os.path.join(d, "speakers.json"), "w") as f:
        json.dump({"spkA": 0, "spkB": 1}, f)
    kinds = ("mel", "pitch", "energy", "duration", "phones_per_word", "attn_prior")
    lines = []
    for i, spk in enumerate(("spkA", "spkB", "spkA")):
        base = "u%d" % i
        for k in kinds:
            os.makedirs(os.path.join(d, k), exist_ok=True)
            arr = {"mel": np.zeros((6, 80), np.float32), "pitch": np.zeros(3, np.float32),
                   "energy": np.zeros(3, np.float32), "duration": np.full(3, 2, np.int64),
                   "phones_per_word": np.array([1, 2], np.int64), "attn_prior": np.zeros((3, 6), np.float32)}[k]
            np.save(os.path.join(d, k, "%s-%s-%s.npy" % (spk, k, base)), arr)
        lines.append("%s|%s|{a b c}|a b" % (base, spk))
    with open(os.path.join(d, "train.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    pre = {"dataset": "Synth", "path": {"preprocessed_path": d},
           "preprocessing": {"text": {"text_cleaners": ["english_cleaners"]}, "speaker_embedder": "DeepSpeaker"}}
    train = {"optimizer": {"batch_size": 3, "batch_size_shallow": 3}}
    ds = D.Dataset("train.txt", types.SimpleNamespace(model="naive"), pre, {"multi_speaker": True}, train,
                   text_to_sequence=lambda t, c: [1, 2, 3], mmap=False)
    batch = ds.reprocess([ds[i] for i in range(3)], [0, 1, 2])
    spk_embeds = batch[9]
    assert spk_embeds.shape == (3, 512) and spk_embeds.dtype == np.float32
    ref = {s: np.mean(es if s == "spkA" else [e.numpy() for e in es], axis=0) for s, es in embeds.items()}
    for i, spk in enumerate(("spkA", "spkB", "spkA")):
        np.testing.assert_array_equal(spk_embeds[i], ref[spk][0])
