#!/usr/bin/env python3
"""Generate tests/golden/lingenc_train_{dga,ctc}.npz and tests/golden/lingenc_train_manifest.json by running the REAL
reference LinguisticEncoder (model/linguistic_encoder.py) in train mode on CPU, with grad.

Run in the build container only:   python tests/golden/make_golden_lingenc_train.py
Data only, like make_golden_lingenc.py (whose batch / seeding helpers it uses): inputs, every dropout keep-mask in the
order the reference draws it (F.dropout taped, as make_golden.py's DropTape), the nine outputs, the reference's own
duration / pitch / energy / helper loss terms (model/loss.py:128-195 with its GuidedAttentionLoss / ForwardSumLoss),
and the gradients of   loss = lambda_d dur + lambda_p pitch + lambda_e energy + helper + sum(coef * x)   (coef a
seeded [B, Lq, 256] array, stored): in full for the small parameters, as (sum, abs-sum, corner) digests for the large
ones.  Own RNG stream and manifest: every other fixture stays byte-identical.
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_lingenc as MG  # noqa: E402  (installs the reference harness and its stubs)
import torch  # noqa: E402
import torch.nn.functional as _F  # noqa: E402

from model.linguistic_encoder import LinguisticEncoder  # noqa: E402
from model.loss import GuidedAttentionLoss, ForwardSumLoss  # noqa: E402
from utils.tools import get_mask_from_lengths  # noqa: E402

SMALL = 4096        # parameters up to this many elements keep their full gradient
CTC_STEP = 1000


def run_case(name, rng, seed_, words, helper):
    stats = MG.H.make_stats_dir(MG.SPEC_MIN, MG.SPEC_MAX)
    cfg = MG.configs(helper)
    cfg[2]["step"]["ctc_step"] = CTC_STEP
    pre, mc, tr = copy.deepcopy(cfg)
    pre["path"]["preprocessed_path"] = stats
    torch.manual_seed(seed_)
    enc = LinguisticEncoder(pre, mc, tr)
    cfg[0]["path"]["preprocessed_path"] = None
    ck = MG.seed(enc, seed_, name, cfg)
    for attempt in range(5000):
        texts, src_lens, wb, src_w_lens = MG.batch(rng, words)
        B, Tp = texts.shape
        src_mask = get_mask_from_lengths(src_lens, Tp)
        src_w_mask = get_mask_from_lengths(src_w_lens, int(src_w_lens.max()))
        dt = torch.from_numpy(rng.integers(1, 5, (B, Tp))) * src_mask
        pt = torch.from_numpy(rng.standard_normal((B, Tp)).astype(np.float32) * 2 + 1) * src_mask
        et = torch.from_numpy(rng.standard_normal((B, Tp)).astype(np.float32) * 2 + 1) * src_mask
        if not (MG.near_bins(pt, enc.pitch_bins.detach()) or MG.near_bins(et, enc.energy_bins.detach())):
            break
    else:
        raise RuntimeError(name + ": no draw clear of the bucket boundaries")
    mel_lens = dt.sum(1)
    max_len = int(mel_lens.max())
    mel_mask = get_mask_from_lengths(mel_lens, max_len)
    prior = None
    if helper == "ctc":
        prior = torch.from_numpy(rng.uniform(0.01, 1.0, (B, Tp, max_len)).astype(np.float32))

    masks = []
    drng = np.random.default_rng(int(rng.integers(1 << 30)))

    def drop_tape(x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        keep = (drng.random(tuple(x.shape)) >= p)
        masks.append(keep.astype(np.uint8))
        return x * torch.from_numpy(keep.astype(np.float32)) / (1.0 - p)

    enc.train()
    saved = _F.dropout
    _F.dropout = drop_tape
    try:
        out = enc(texts, src_lens, wb, src_mask, src_w_lens, src_w_mask, mel_mask, max_len, prior, pt, et, dt, 1.0, 1.0)
    finally:
        _F.dropout = saved
    x, p_pred, e_pred, logd, dur, mlen, mmask, attns, logp = out

    # model/loss.py:128-195 (phoneme-level pitch / energy, naive model)
    lc, al = tr["loss"], tr["aligner"]
    mse = torch.nn.MSELoss()
    logd_t = torch.log(dur.float() + 1)
    duration_loss = mse(logd.masked_select(src_w_mask), logd_t.masked_select(src_w_mask))
    pitch_loss = mse(p_pred.masked_select(src_mask), pt.masked_select(src_mask))
    energy_loss = mse(e_pred.masked_select(src_mask), et.masked_select(src_mask))
    terms = {}
    if helper == "dga":
        ga = GuidedAttentionLoss(sigma=al["guided_sigma"], alpha=al["guided_lambda"])
        attn_loss = torch.zeros(1)
        for a in attns[1]:
            attn_loss = attn_loss + ga(a, src_lens, mel_lens)
        helper_loss = al["guided_weight"] * attn_loss
        terms["attn_loss"] = attn_loss
    else:
        fs = ForwardSumLoss()
        ctc_loss = torch.zeros(1)
        for lp in logp:
            ctc_loss = ctc_loss + fs(lp, src_lens, mel_lens)
        ctc_loss = ctc_loss.mean()
        helper_loss = al["ctc_weight_start"] * ctc_loss          # step 1 <= ctc_step
        terms["ctc_loss"] = ctc_loss
    total = lc["lambda_d"] * duration_loss + lc["lambda_p"] * pitch_loss + lc["lambda_e"] * energy_loss + helper_loss
    coef = torch.from_numpy(rng.standard_normal(tuple(x.shape)).astype(np.float32) * 1e-2)
    (total.sum() + (coef * x).sum()).backward()

    arrs = dict(wsum=ck, texts=texts, src_lens=src_lens, wb=wb, src_w_lens=src_w_lens, src_mask=src_mask,
                src_w_mask=src_w_mask, mel_mask=mel_mask, max_len=max_len, pitch_target=pt, energy_target=et,
                duration_target=dt, p_control=np.float64(1.0), d_control=np.float64(1.0), coef=coef,
                n_masks=np.int64(len(masks)))
    if prior is not None:
        arrs["attn_prior"] = prior
    for i, m in enumerate(masks):
        arrs["mask%03d" % i] = m
    MG.record(arrs, out, {"enc_p_out": torch.zeros(0), "enc_w_out": torch.zeros(0)})
    del arrs["enc_p_out"], arrs["enc_w_out"]
    for k, v in dict(duration_loss=duration_loss, pitch_loss=pitch_loss, energy_loss=energy_loss,
                     helper_loss=helper_loss, total=total, **terms).items():
        arrs["loss/" + k] = np.float64(v.detach().reshape(-1)[0].item())
    for k, p in enc.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None, k
        if p.numel() <= SMALL:
            arrs["grad/" + k] = p.grad
        else:
            g = p.grad.detach().double()
            arrs["dw_sum/" + k] = np.array([g.sum().item(), g.abs().sum().item()])
            arrs["dw_corner/" + k] = g[tuple(slice(0, min(4, s)) for s in g.shape)].float().numpy()
    print(" ", name, "masks", len(masks), "mel_len", mlen.tolist(), "total", float(total))
    MG.save(name, arrs)


def main():
    rng = np.random.default_rng(20261016)
    run_case("lingenc_train_dga", rng, 71, [5, 3], "dga")
    run_case("lingenc_train_ctc", rng, 72, [4, 4, 2], "ctc")
    with open(os.path.join(HERE, "lingenc_train_manifest.json"), "w") as f:
        json.dump(MG.MANIFEST, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()
