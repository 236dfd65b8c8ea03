"""Shared set-up of the linguistic-encoder training tests: the fixtures of tests/golden/make_golden_lingenc_train.py
(the REAL reference encoder in train mode), their manifest, and the nine encoder outputs laid into the slots of
MixGANTTS.forward's output list that LinguisticEncoderLoss reads."""
import json
import os

import numpy as np
import torch

from helpers import GOLDEN, T

TRAIN_CASES = ("lingenc_train_dga", "lingenc_train_ctc")


def train_manifest():
    with open(os.path.join(GOLDEN, "lingenc_train_manifest.json")) as f:
        return json.load(f)


def fixture_masks(g):
    return [g["mask%03d" % i] for i in range(int(g["n_masks"]))]


class MaskReplay:
    """DROPOUT_FN that hands out the fixture's keep-masks in order, checking each requested shape."""

    def __init__(self, masks):
        self.masks, self.i = masks, 0

    def __call__(self, shape, p, device):
        m = self.masks[self.i]
        assert tuple(shape) == m.shape, ("mask %d" % self.i, tuple(shape), m.shape)
        self.i += 1
        return torch.from_numpy(m).to(device)


def model_slots(out, src_mask, src_lens, src_w_mask):
    """Encoder outputs -> the 16-slot list positions LinguisticEncoderLoss reads (4-8, 10-14)."""
    x, p, e, logd, dur, mel_len, mel_mask, attns, logp = out
    return [x, None, None, None, p, e, logd, dur, src_mask, ~mel_mask, src_lens, mel_len, attns, logp, src_w_mask, None]


def fixture_batch(g, device):
    """The reference batch positions the loss reads (14: pitch, 15: energy targets)."""
    b = [None] * 17
    b[14], b[15] = T(g["pitch_target"]).to(device), T(g["energy_target"]).to(device)
    return b


def fixture_loss_inputs(g, device):
    d = lambda k: T(g[k]).to(device)  # noqa: E731
    out = (d("out0"), d("out1"), d("out2"), d("out3"), d("out4"), d("out5"), d("out6"), (d("out7/0"), d("out7/1")),
           d("out8"))
    return model_slots(out, d("src_mask"), d("src_lens"), d("src_w_mask")), fixture_batch(g, device)


def loss_terms_close(got, g, tol):
    for k in ("duration_loss", "pitch_loss", "energy_loss", "helper_loss", "total", "attn_loss", "ctc_loss"):
        if "loss/" + k not in g:
            continue
        ref = float(g["loss/" + k])
        v = float(got[k])
        assert np.isfinite(v) and abs(v - ref) <= tol * max(1.0, abs(ref)), (k, v, ref)
