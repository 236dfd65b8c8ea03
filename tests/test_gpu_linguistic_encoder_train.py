"""Training the native LinguisticEncoder on the GPU (linguistic_encoder.py train path, csrc/lingenc_train.hip):
the whole encoder in train mode against the REAL reference (tests/golden/make_golden_lingenc_train.py, dropout masks
replayed through DROPOUT_FN) -- outputs, LinguisticEncoderLoss terms and parameter gradients; both attention backward
passes against fp64 autograd of tests/lingenc_torch.py over short, window-sized, ragged and long shapes; the
per-token glue backward passes against torch autograd; run-to-run bit identity; the no_grad train forward; ABI errors;
and a get_model(..., train=True, linguistic_encoder="native") model trained by step_from_model."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lingenc_torch as LT
from helpers import golden, assert_close, assert_digest, T
from lingenc_helpers import configs, load_weights, encoder_inputs, assert_outputs
from lingenc_train_helpers import (TRAIN_CASES, train_manifest, fixture_masks, MaskReplay, model_slots,
                                   fixture_batch, loss_terms_close)

pytestmark = pytest.mark.gpu
TOL = 1e-3


def _native(tmp_path, name):
    import mixgan_tts_amd as mg
    man = train_manifest()
    cfg = configs(man, name, tmp_path)
    enc = mg.LinguisticEncoder(*cfg)
    load_weights(enc, man, name)
    return enc.cuda().train(), cfg


def _run(enc, cfg, g, masks):
    """Train-mode forward with the fixture's masks, LinguisticEncoderLoss + the fixture's functional, backward."""
    import mixgan_tts_amd as mg
    args = encoder_inputs(g, "cuda")
    rep = MaskReplay(masks)
    mg.transformer.DROPOUT_FN = rep
    try:
        out = enc(*args)
    finally:
        mg.transformer.DROPOUT_FN = None
    assert rep.i == len(masks)
    loss = mg.LinguisticEncoderLoss(*cfg)
    slots = model_slots(out, args[3], args[1], args[5])
    total = loss(fixture_batch(g, "cuda"), slots, 1)
    enc.zero_grad(set_to_none=True)
    (total + (T(g["coef"]).cuda() * out[0]).sum()).backward()
    torch.cuda.synchronize()
    return out, loss.last


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_encoder_train_matches_reference_fixture(tmp_path, name):
    enc, cfg = _native(tmp_path, name)
    g = golden(name)
    out, terms = _run(enc, cfg, g, fixture_masks(g))
    assert_outputs(out, g, TOL)
    loss_terms_close(terms, g, TOL)
    for k, p in enc.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if k.endswith("conv_k.bias"):
            # a key bias shifts every score of a query row by the same amount: softmax-invariant, so its gradient is
            # zero up to rounding on both sides; bound it against the same layer's value-bias gradient instead
            scale = float(np.abs(g["grad/" + k.replace("conv_k", "conv_v")]).max())
            assert float((p.grad.cpu() - T(g["grad/" + k])).abs().max()) <= TOL * scale, k
        elif "grad/" + k in g:
            assert_close(p.grad, g["grad/" + k], TOL, k)
        else:
            assert_digest(p.grad, g, k, TOL)


def test_backward_is_bit_identical_and_no_grad_train_forward_matches(tmp_path):
    name = "lingenc_train_ctc"
    enc, cfg = _native(tmp_path, name)
    g = golden(name)
    masks = fixture_masks(g)
    out1, _ = _run(enc, cfg, g, masks)
    g1 = {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    out2, _ = _run(enc, cfg, g, masks)
    for k, p in enc.named_parameters():
        if k in g1:
            assert torch.equal(g1[k], p.grad), k
    import mixgan_tts_amd as mg
    mg.transformer.DROPOUT_FN = MaskReplay(masks)
    try:
        with torch.no_grad():
            out3 = enc(*encoder_inputs(g, "cuda"))
    finally:
        mg.transformer.DROPOUT_FN = None
    for a, b in zip(LT_flat(out1), LT_flat(out3)):
        assert torch.equal(a.detach(), b), "no_grad train forward differs"


def LT_flat(out):
    r = []
    for o in out:
        r.extend(o if isinstance(o, (list, tuple)) else [o])
    return r


# ------------------------------------------------------------------------------------ attention backward passes
def _rel_attention_drop(qkv, valid, emb_k, emb_v, n_head, w, keep, scale):
    """tests/lingenc_torch.py's rel_attention with dropout(p_attn) applied (model/blocks.py:1059)."""
    B, C3, L = qkv.shape
    HD = C3 // 3
    d = HD // n_head
    q, k, v = [t.reshape(B, n_head, d, L).transpose(2, 3) for t in qkv.split(HD, 1)]
    scores = q @ k.transpose(-1, -2) / math.sqrt(d)
    i = torch.arange(L, device=qkv.device)
    rel = i[None, :] - i[:, None] + w
    band = (rel >= 0) & (rel <= 2 * w)
    idx = rel.clamp(0, 2 * w)
    rk = (q @ emb_k.t()) / math.sqrt(d)
    scores = scores + torch.where(band, rk.gather(3, idx.expand(B, n_head, L, L)), torch.zeros((), device=qkv.device,
                                                                                                dtype=rk.dtype))
    m = valid.to(scores.dtype)
    scores = scores.masked_fill((m[:, None, :, None] * m[:, None, None, :]) == 0, -1e4)
    p = F.softmax(scores, -1) * keep.to(scores.dtype) * scale
    out = p @ v
    pb = torch.zeros(B, n_head, L, 2 * w + 1, device=qkv.device, dtype=p.dtype)
    pb.scatter_add_(3, idx.expand(B, n_head, L, L), p * band)
    out = out + pb @ emb_v
    return out.transpose(2, 3).reshape(B, HD, L)


def _ragged_valid(B, L, gen):
    lens = [L] + [int(torch.randint(1, L + 1, (1,), generator=gen)) for _ in range(B - 1)]
    return (torch.arange(L)[None] < torch.tensor(lens)[:, None]).to(torch.uint8)


@pytest.mark.parametrize("L", [1, 4, 5, 9, 64, 65, 200])
def test_rel_attention_backward(L):
    import mixgan_tts_amd as mg
    LE = mg.linguistic_encoder
    gen = torch.Generator().manual_seed(100 + L)
    B, H, D, w, p = 3, 2, 128, 4, 0.2
    qkv = torch.randn(B, 3 * H * D, L, generator=gen)
    ek = torch.randn(2 * w + 1, D, generator=gen) * D ** -0.5
    ev = torch.randn(2 * w + 1, D, generator=gen) * D ** -0.5
    valid = _ragged_valid(B, L, gen)
    keep = (torch.rand(B, H, L, L, generator=gen) >= p).to(torch.uint8)
    gout = torch.randn(B, H * D, L, generator=gen)
    ref_in = [t.double().cuda().requires_grad_() for t in (qkv, ek, ev)]
    ref = _rel_attention_drop(ref_in[0], valid.cuda(), ref_in[1], ref_in[2], H, w, keep.cuda(), 1 / (1 - p))
    ref.backward(gout.double().cuda())
    c = [t.cuda() for t in (qkv, valid, ek, ev, keep, gout)]
    out, P = LE.rel_attention_train(c[0], c[1], c[2], c[3], H, w, c[4], 1 / (1 - p))
    dqkv, dek, dev_ = LE.rel_attention_bwd(c[0], c[1], P, c[4], 1 / (1 - p), c[5], c[2], c[3], H, w)
    torch.cuda.synchronize()
    assert_close(out, ref.detach(), 1e-4, "out")
    for got, r, what in ((dqkv, ref_in[0], "dqkv"), (dek, ref_in[1], "d emb_k"), (dev_, ref_in[2], "d emb_v")):
        assert torch.isfinite(got).all(), what
        assert_close(got, r.grad, TOL, what)
    again = LE.rel_attention_bwd(c[0], c[1], P, c[4], 1 / (1 - p), c[5], c[2], c[3], H, w)
    assert all(torch.equal(a, b) for a, b in zip((dqkv, dek, dev_), again))


@pytest.mark.parametrize("Lq,Lk", [(7, 3), (150, 37), (2000, 300)])
@pytest.mark.parametrize("with_prior", [False, True])
def test_w2p_attention_backward(Lq, Lk, with_prior):
    import mixgan_tts_amd as mg
    LE = mg.linguistic_encoder
    gen = torch.Generator().manual_seed(Lq * 7 + Lk + int(with_prior))
    B, H, D = 2, 2, 128
    q = torch.randn(B, H * D, Lq, generator=gen)
    kv = torch.randn(B, 2 * H * D, Lk, generator=gen)
    kvalid = _ragged_valid(B, Lk, gen)
    qvalid = _ragged_valid(B, Lq, gen)
    mapping = (torch.rand(B, Lq, Lk, generator=gen) < 0.5).to(torch.uint8)
    prior = torch.rand(B, Lk, Lq, generator=gen) * 0.99 + 0.01 if with_prior else None
    gs = [torch.randn(B, H * D, Lq, generator=gen)] + [torch.randn(H, B, Lq, Lk, generator=gen) for _ in range(2)] + \
        [torch.randn(H, B, 1, Lq, Lk, generator=gen)]
    rq, rkv = q.double().cuda().requires_grad_(), kv.double().cuda().requires_grad_()
    ref = LT.w2p_attention(rq, rkv, kvalid.cuda(), qvalid.cuda(), mapping.cuda(),
                           None if prior is None else prior.double().cuda(), H)
    torch.autograd.backward(list(ref), [t.double().cuda() for t in gs])
    c = lambda t: None if t is None else t.cuda()  # noqa: E731
    qc, kvc = q.cuda(), kv.cuda()
    out, attn, raw, logp = LE.w2p_attention(qc, kvc, c(kvalid), c(qvalid), c(mapping), c(prior), H)
    dq, dkv = LE.w2p_attention_bwd(qc, kvc, c(kvalid), c(qvalid), c(mapping), c(prior), attn, raw, logp, c(gs[0]),
                                   c(gs[1]), c(gs[2]), c(gs[3]), H)
    torch.cuda.synchronize()
    assert torch.isfinite(dq).all() and torch.isfinite(dkv).all()
    assert_close(dq, rq.grad, TOL, "dq")
    assert_close(dkv, rkv.grad, TOL, "dkv")
    kpad = ~kvalid.bool().cuda()
    assert float(dkv[:, :H * D].permute(0, 2, 1)[kpad].abs().sum()) == 0.0      # padded keys get nothing
    # only the output's gradient (the three probability tensors unused): NULL upstream pointers
    dq2, dkv2 = LE.w2p_attention_bwd(qc, kvc, c(kvalid), c(qvalid), c(mapping), c(prior), attn, raw, logp, c(gs[0]),
                                     None, None, None, H)
    rq.grad = rkv.grad = None
    ref = LT.w2p_attention(rq, rkv, kvalid.cuda(), qvalid.cuda(), mapping.cuda(),
                           None if prior is None else prior.double().cuda(), H)
    ref[0].backward(gs[0].double().cuda())
    assert_close(dq2, rq.grad, TOL, "dq (out only)")
    assert_close(dkv2, rkv.grad, TOL, "dkv (out only)")


# ------------------------------------------------------------------------------------ glue
def test_glue_backward_passes():
    import mixgan_tts_amd as mg
    LE = mg.linguistic_encoder
    gen = torch.Generator().manual_seed(5)
    B, C, L, n = 3, 256, 37, 40
    dev = "cuda"
    # embedding, padding row 0, pads skipped
    ids = torch.randint(0, n, (B, L), generator=gen)
    valid = _ragged_valid(B, L, gen)
    g = torch.randn(B, C, L, generator=gen)
    table = torch.randn(n, C, generator=gen).requires_grad_()
    ref = F.embedding(ids, table, padding_idx=0) * valid[:, :, None]
    ref.backward(g.transpose(1, 2))
    got = LE.embed_cm_bwd(ids.cuda(), g.cuda(), valid.cuda(), n, 0)
    assert_close(got, table.grad, 1e-5, "embedding")
    assert float(got[0].abs().sum()) == 0.0
    # variance head: pred = (w . h + b) * valid * control
    h = torch.randn(B, C, L, generator=gen).requires_grad_()
    w = torch.randn(1, C, generator=gen).requires_grad_()
    bb = torch.randn(1, generator=gen).requires_grad_()
    dpred = torch.randn(B, L, generator=gen)
    ((torch.einsum("c,bcl->bl", w[0], h) + bb) * valid * 1.5).backward(dpred)
    dh, dw, db = LE.variance_head_bwd(h.detach().cuda(), w.detach().cuda(), valid.cuda(), 1.5, dpred.cuda())
    assert_close(dh, h.grad, 1e-5, "dh")
    assert_close(dw, w.grad[0], 1e-5, "dw")
    assert_close(db, bb.grad, 1e-5, "db")
    # duration head: logw = log(word sum of exp(logp))
    wb = torch.tensor([[3, 2, 4, 0], [1, 1, 1, 5]])
    swl = torch.tensor([3, 4])
    Tp, W = 9, 4
    logp = torch.randn(2, Tp, generator=gen, dtype=torch.float64).requires_grad_()
    ref = LT.word_pool(logp.exp()[:, :, None], wb, swl, W, False).log().squeeze(-1)
    dlw = torch.randn(2, W, generator=gen, dtype=torch.float64) * torch.isfinite(ref)
    ref.backward(torch.where(torch.isfinite(ref), dlw, 0.))
    logw, _ = LE.duration_head(logp.detach().float().cuda(), None, wb.cuda(), swl.cuda(), 1.0, W)
    got = LE.duration_head_bwd(logp.detach().float().cuda(), logw, dlw.float().cuda(), wb.cuda(), swl.cuda())
    assert torch.isfinite(got).all()
    assert_close(got, logp.grad, 1e-5, "duration head")
    # position encoding: d table[l] = sum_b coef[b, l] dOut[b, :, l]
    coef = torch.rand(B, L, generator=gen)
    tab = torch.randn(L + 5, C, generator=gen).requires_grad_()
    (coef[:, None, :] * tab[:L].t()[None]).backward(g)
    got = LE.posenc_add_bwd(g.cuda(), coef.cuda())
    assert_close(got, tab.grad[:L], 1e-5, "posenc table")
    # the Function: gradient to x in both layouts and to the parameter's first L rows
    param = torch.randn(1, L + 5, C, device=dev, requires_grad=True)
    x = torch.randn(B, L, C, device=dev, requires_grad=True)
    y = LE._PosencAddFn.apply(x, param, True, coef.to(dev))
    y.backward(g.to(dev))
    assert_close(x.grad, g.transpose(1, 2), 0, "posenc dx")
    assert float(param.grad[0, L:].abs().sum()) == 0.0


def test_entry_points_reject_bad_arguments():
    import mixgan_tts_amd as mg
    L = mg._lib.lib()
    ARG, SHAPE, WS = -1, -2, -3
    x = torch.zeros(4096, device="cuda")
    u = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    p, pu = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(u.data_ptr())
    s = mg._lib.stream_ptr()
    assert L.mg_rel_attention_train_fwd(None, pu, p, p, None, 1.0, p, None, 1, 4, 2, 128, 4, s) == ARG
    assert L.mg_rel_attention_train_fwd(p, pu, p, p, None, 1.0, p, None, 1, 4, 2, 64, 4, s) == SHAPE
    assert L.mg_rel_attention_train_fwd(p, pu, p, p, None, 1.0, p, None, 1, 4, 2, 128, 9, s) == SHAPE
    assert L.mg_rel_attention_bwd_ws_floats(1, 4, 2, 9) == 0
    n = L.mg_rel_attention_bwd_ws_floats(1, 4, 2, 4)
    args = [p, pu, p, None, 1.0, p, p, p, p, p, p, p]
    assert L.mg_rel_attention_bwd(*([None] + args[1:]), n, 1, 4, 2, 128, 4, s) == ARG
    assert L.mg_rel_attention_bwd(*args, n, 0, 4, 2, 128, 4, s) == SHAPE
    assert L.mg_rel_attention_bwd(*args, n - 1, 1, 4, 2, 128, 4, s) == WS
    wargs = [p, p, pu, pu, pu, None, p, p, p, p, None, None, None, p, p, p]
    n = L.mg_w2p_attention_bwd_ws_floats(1, 3, 2, 2)
    assert L.mg_w2p_attention_bwd(*(wargs[:6] + [None] + wargs[7:]), n, 1, 3, 2, 2, 128, s) == ARG
    assert L.mg_w2p_attention_bwd(*wargs, n, 1, 3, 2, 2, 96, s) == SHAPE
    assert L.mg_w2p_attention_bwd(*wargs, n - 1, 1, 3, 2, 2, 128, s) == WS
    assert L.mg_embed_cm_bwd(None, p, None, p, 1, 4, 8, 4, 0, s) == ARG
    assert L.mg_embed_cm_bwd(p, p, None, p, 1, 0, 8, 4, 0, s) == SHAPE
    assert L.mg_variance_head_bwd(p, p, pu, 1.0, p, None, p, p, 1, 8, 4, s) == ARG
    assert L.mg_variance_head_bwd(p, p, pu, 1.0, p, p, p, p, 1, 8, 0, s) == SHAPE
    assert L.mg_duration_head_bwd(p, p, None, p, p, p, 1, 4, 2, 2, s) == ARG
    assert L.mg_duration_head_bwd(p, p, p, p, p, p, 1, 4, 0, 2, s) == SHAPE
    assert L.mg_posenc_add_bwd(p, None, p, 1, 8, 4, s) == ARG
    assert L.mg_posenc_add_bwd(p, p, p, 1, 0, 4, s) == SHAPE
    assert L.mg_dropout_apply(p, None, 1.0, p, 16, s) == ARG
    assert L.mg_dropout_apply(p, pu, 1.0, p, 0, s) == SHAPE
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ end to end
def test_get_model_native_trains_through_step_from_model(tmp_path):
    """get_model(..., train=True, linguistic_encoder="native"), naive model, a synthetic batch: step_from_model with
    LinguisticEncoderLoss gives every trainable encoder parameter a finite gradient, and over 30 steps on the one
    batch the encoder loss falls."""
    import mixgan_tts_amd as mg
    name = "lingenc_train_dga"
    g = golden(name)
    pre, mc, tr = configs(train_manifest(), name, tmp_path)
    tr["optimizer"]["init_lr_G"] = 1e-3
    args = types.SimpleNamespace(model="naive", restore_step=0)
    model, D, *_ = mg.get_model(args, (pre, mc, tr), "cuda", train=True, linguistic_encoder="native")
    assert model.training and model.linguistic_encoder.training
    enc_names = [n for n, p in model.named_parameters() if n.startswith("linguistic_encoder.")]
    assert enc_names
    others = [p for n, p in model.named_parameters() if not n.startswith("diffusion.")]
    trainer = mg.HotPathTrainer(model.diffusion, D, tr, mc, extra_g_params=others,
                                g_param_order=list(model.parameters()))
    ein = encoder_inputs(g, "cuda")
    texts, src_lens, wb, _, src_w_lens = ein[0], ein[1], ein[2], ein[3], ein[4]
    dur = ein[11]
    mel_lens = dur.sum(1)
    Lm = int(mel_lens.max())
    gen = torch.Generator().manual_seed(3)
    mels = ((torch.rand(len(mel_lens), Lm, 80, generator=gen) * 13.5 - 11.5).cuda() *
            (torch.arange(Lm, device="cuda")[None] < mel_lens[:, None]).unsqueeze(-1))
    batch = [["a"] * len(mel_lens), ["t"] * len(mel_lens), torch.zeros(len(mel_lens), dtype=torch.long, device="cuda"),
             texts, src_lens, texts.shape[1], wb, src_w_lens, int(src_w_lens.max()), None, None, mels, mel_lens, Lm,
             ein[9], ein[10], dur]
    loss = mg.LinguisticEncoderLoss(pre, mc, tr)
    seen = {}

    def hook(bname, bucket):
        if bname == "G":
            seen.update({k: bucket.flat[bucket.offsets[id(p)]:bucket.offsets[id(p)] + p.numel()].detach().clone()
                         for k, p in model.named_parameters() if id(p) in bucket.offsets})
    trainer.grad_hook = hook
    totals = []
    for step in range(30):
        trainer.step_from_model(model, list(batch), upstream_loss=loss)
        totals.append(float(loss.last["total"]))
        if step == 0:
            for k in enc_names:
                p = dict(model.named_parameters())[k]
                if not p.requires_grad:
                    continue
                assert k in seen and torch.isfinite(seen[k]).all(), k
            assert sum(float(seen[k].abs().sum()) for k in enc_names if k in seen) > 0
            trainer.grad_hook = None
    assert all(np.isfinite(totals))
    assert np.mean(totals[-5:]) < 0.8 * np.mean(totals[:5]), totals
