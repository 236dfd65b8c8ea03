"""Shared set-up of the linguistic-encoder tests: fixture configs, seeded weights (tests/golden/lingenc_manifest.json,
made by tests/golden/make_golden_lingenc.py) and the fixture inputs."""
import copy
import json
import os

import numpy as np
import torch

from helpers import GOLDEN, write_stats, T
from oracle import weights as WR

CASES = ("lingenc_infer", "lingenc_teacher", "lingenc_ctc", "lingenc_long")


def manifest():
    with open(os.path.join(GOLDEN, "lingenc_manifest.json")) as f:
        return json.load(f)


def configs(man, name, tmpdir):
    pre, mc, tr = copy.deepcopy(man[name]["configs"])
    pre["path"]["preprocessed_path"] = write_stats(tmpdir, np.linspace(-11.5, -9.0, 80), np.linspace(1.0, 2.0, 80))
    return pre, mc, tr


def load_weights(module, man, name):
    """The fixture's weights: the recipe's draw, then the manifest's overrides; other entries keep their init."""
    ent = man[name]
    sd = module.state_dict()
    assert list(sd.keys()) == ent["state_dict_order"]
    w = WR.draw(ent["seeded"], ent["seed"])
    for k, a in w.items():
        assert tuple(sd[k].shape) == a.shape, k
        sd[k] = torch.from_numpy(a)
    for k, v in ent["overrides"].items():
        sd[k] = torch.full_like(sd[k], v)
    module.load_state_dict(sd)
    return WR.checksum(w)


def encoder_inputs(g, device):
    """The 14 forward arguments of the fixture, in order."""
    d = lambda k: T(g[k]).to(device) if k in g else None  # noqa: E731
    max_len = int(g["max_len"]) if "max_len" in g else None
    return (d("texts"), d("src_lens"), d("wb"), d("src_mask"), d("src_w_lens"), d("src_w_mask"), d("mel_mask"), max_len,
            d("attn_prior"), d("pitch_target"), d("energy_target"), d("duration_target"), float(g["p_control"]),
            float(g["d_control"]))


def flat_outputs(out):
    d = {}
    for i, o in enumerate(out):
        if isinstance(o, (list, tuple)):
            for j, oo in enumerate(o):
                d["out%d/%d" % (i, j)] = oo
        else:
            d["out%d" % i] = o
    return d


def assert_outputs(out, g, tol, extra=None):
    """Floats to `tol` max-abs / max-ref on the finite entries with identical -inf positions; integers and masks
    exactly; dtypes and shapes as recorded."""
    from helpers import assert_close
    got = flat_outputs(out)
    if extra:
        got.update(extra)
    for k, v in got.items():
        ref = g[k]
        a = v.detach().cpu().numpy()
        assert a.shape == ref.shape and a.dtype == ref.dtype, (k, a.shape, a.dtype, ref.shape, ref.dtype)
        if a.dtype.kind == "f":
            fin = np.isfinite(ref)
            assert np.array_equal(np.isfinite(a), fin), k + ": non-finite positions differ"
            assert np.array_equal(a[~fin], ref[~fin]), k + ": non-finite values differ"
            assert_close(np.where(fin, a, 0), np.where(fin, ref, 0), tol, k)
        else:
            assert (a == ref).all(), k
