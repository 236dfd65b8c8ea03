"""The references and input sets of tests/test_gpu_attention_forms.py and tests/test_gpu_lingenc_forms.py, checked with no
GPU: every restatement against torch's own operator (or the restatement the older tests use), the CPU emulation of the
fp16-operand kernel against the figures its bar rests on, and the margins every input set promises."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_ref as AR
import lingenc_torch as LT
import test_gpu_lingenc_forms as GF
from helpers import rel_err
from small_ops_ref import BAR_RED, KINK_BAND, KINK_SHARE, gen


@pytest.mark.parametrize("mask", AR.MASKS)
def test_attention_restatement_is_torch_sdpa(mask):
    qkv, pad = AR.case(65, "unit", mask)
    q, k, v = [t.double().transpose(2, 3) for t in AR.split_heads(qkv, AR.N_HEAD)]
    m = None if pad is None else ~pad.bool()[:, None, None, :]
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=m).transpose(2, 3).reshape(AR.B, -1, 65)
    assert rel_err(AR.attention(qkv.double(), pad, AR.N_HEAD).numpy(), ref.numpy()) < 1e-14


def test_attention_input_sets():
    for L in sorted(set(AR.COMMON_L + (127, 128, 129, 255, 256, 257))):
        for mask in AR.MASKS:
            pad = AR.key_mask(L, mask)
            if pad is None:
                continue
            assert pad.shape == (AR.B, L) and int((pad == 0).sum(1).min()) >= 1
            if mask == "scattered" and L >= 128:
                assert bool(pad[:, :32].all()) and bool(pad[:, 96:128].all())
            if mask == "suffix":
                assert int((pad[1] == 0).sum()) == 1 and int(pad[0].sum()) == 0
            qkv, _ = AR.case(L, "late_max", mask)
            HD = AR.N_HEAD * AR.D_HEAD
            if bool(pad.any()):
                assert bool((qkv[:, 2 * HD:].transpose(1, 2)[pad.bool()] == 1.0e4).all())
            assert bool(torch.isfinite(AR.refs(L, "late_max", mask)[1]).all())
    # the late maximum: in a good share of the rows the last valid key holds the row maximum
    qkv, _ = AR.case(700, "late_max", "none")
    q, k, _ = AR.split_heads(qkv.double(), AR.N_HEAD)
    s = torch.einsum("bhdq,bhdk->bhqk", q, k)
    share = float((s.argmax(-1) == 699).double().mean())
    assert 0.2 < share < 0.4, share      # P(6 z > the largest of 699 unit normals, about 3.2) = 0.30


@pytest.mark.parametrize("inputs,lo,hi", [("unit", 3e-5, 4e-4), ("peaked", 3e-5, 4e-4)])
def test_f16_emulation_figures(inputs, lo, hi):
    """The emulation's distance from the rounded-operand reference is about 1e-4 of the tensor maximum, with or without
    the running maximum; the rounding of the operands alone is a few 1e-4 (unit variance) to a few 1e-3 (peaked)."""
    for L in (64, 700):
        ref16, emu, emu_run, fused = AR.refs_f16(L, inputs, "none")
        assert rel_err(fused.numpy(), ref16.numpy()) < 1e-3         # q rounded once: a few elements, one fp16 unit each
        ref32, ref64 = AR.refs(L, inputs, "none")
        for e in (rel_err(emu.numpy(), ref16.numpy()), rel_err(emu_run.numpy(), ref16.numpy())):
            assert lo < e < hi, (L, inputs, e)
        r = rel_err(ref16.numpy(), ref64.numpy())
        assert (1e-4 < r < 1e-3) if inputs == "unit" else (1e-3 < r < 1e-2), (L, inputs, r)
        assert rel_err(ref32.numpy(), ref64.numpy()) < BAR_RED / 2


def test_f16_emulation_with_masks_is_finite_and_tight():
    for mask in AR.MASKS:
        ref16, emu, emu_run, _ = AR.refs_f16(129, "late_max", mask)
        assert bool(torch.isfinite(emu).all()) and bool(torch.isfinite(emu_run).all())
        assert rel_err(emu.numpy(), ref16.numpy()) < 1e-3 and rel_err(emu_run.numpy(), ref16.numpy()) < 1e-3


@pytest.mark.parametrize("L,w", [(1, 4), (5, 4), (40, 0), (40, 4), (40, 8)])
def test_rel_attention_pieces_are_the_restatement(L, w):
    g = gen(L + w)
    B, H, D = 2, 2, 128
    qkv = torch.randn(B, 3 * H * D, L, generator=g, dtype=torch.float64)
    ek, ev = torch.randn(2 * w + 1, D, generator=g, dtype=torch.float64), torch.randn(2 * w + 1, D, generator=g, dtype=torch.float64)
    valid = GF.ragged_valid(B, L, g)
    P = LT.rel_attention_probs(qkv, valid, ek, H, w)
    assert rel_err(LT.rel_attention_apply(P, qkv, ev, H, w).numpy(), LT.rel_attention(qkv, valid, ek, ev, H, w).numpy()) < 1e-13
    assert float((P.sum(-1) - 1).abs().max()) < 1e-12
    keep = (torch.rand(B, H, L, L, generator=g) > 0.3).to(torch.uint8)
    a = LT.rel_attention_apply(P, qkv, ev, H, w, keep, 2.0)
    b = LT.rel_attention_apply(P * keep * 2.0, qkv, ev, H, w)
    assert torch.equal(a, b)


def test_glue_restatements_are_torch_operators():
    g = gen(3)
    ids = torch.randint(0, 9, (2, 30), generator=g)
    table = torch.randn(9, 5, generator=g)
    ones = torch.ones(2, 30, dtype=torch.uint8)
    assert torch.equal(LT.embed_cm(ids, table, ones), F.embedding(ids, table).transpose(1, 2))
    h = torch.randn(2, 6, 30, generator=g, dtype=torch.float64)
    w, b = torch.randn(1, 6, generator=g, dtype=torch.float64), torch.randn(1, generator=g, dtype=torch.float64)
    bins = torch.tensor([-1.0, 0.25, 1.5])
    tgt = torch.randn(2, 30, generator=g)
    tgt[0, :3] = bins
    pred, bucket = LT.variance_head(h, w, b, ones, 1.0, tgt, bins)
    assert torch.equal(bucket, torch.bucketize(tgt, bins)) and int(bucket[0, 1]) == 1
    assert rel_err(pred.numpy(), F.linear(h.transpose(1, 2), w, b).squeeze(-1).numpy()) < 1e-14
    pred, bucket = LT.variance_head(h, w, b, ones, 0.5, None, bins)
    assert torch.equal(bucket, torch.bucketize(pred, bins.double()))


@pytest.mark.parametrize("L", [1, 256, 257, 700])
def test_variance_head_inputs_keep_off_the_bin_edges(L):
    h, weight, bias, valid, control, target, bins, emb, x, redrawn = GF.variance_inputs(L, False)
    assert redrawn <= KINK_SHARE * valid.numel(), (redrawn, valid.numel())
    pred, _ = LT.variance_head(h.double(), weight.double(), bias.double(), valid, control, None, bins)
    dist = (pred[:, :, None] - bins.double()).abs().amin(-1)[valid.bool()]
    assert float(dist.min()) > KINK_BAND * float(bins[-1] - bins[0])
    # the float32 restatement lands in the same bucket everywhere, so may a float32 kernel
    b64 = LT.variance_head(h.double(), weight.double(), bias.double(), valid, control, None, bins)[1]
    assert torch.equal(LT.variance_head(h, weight, bias, valid, control, None, bins)[1], b64)
    t = GF.variance_inputs(L, True)[5]
    on = (t[:, :, None] == bins).any(-1)
    assert int(on.sum()) >= min(3, t.numel()) and (L == 1 or (float(t.min()) < float(bins[0]) and float(t.max()) > float(bins[-1])))


@pytest.mark.parametrize("W", [1, 256, 257, 300])
def test_duration_head_inputs_keep_off_the_half_integers(W):
    logp, target, wb, swl = GF.duration_inputs(W)
    assert logp.shape[1] == int(wb.sum(1).max()) and int(swl[0]) == W
    for c in (1.0, 0.5, 1.25):
        lw64, dur = LT.duration_head(logp.double(), None, wb, swl, c, W)
        lw32, dur32 = LT.duration_head(logp, None, wb, swl, c, W)
        s = lw64.exp()[torch.isfinite(lw64)]
        assert float((s - s.floor() - 0.5).abs().min()) > 0.04
        assert torch.equal(dur, dur32) and int(dur.min()) >= 0
    if W > 2:
        assert math.isinf(float(lw64[0, W // 2])) and math.isinf(float(lw64[1, W - 1]))
