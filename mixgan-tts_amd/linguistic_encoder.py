"""Native LinguisticEncoder (model/linguistic_encoder.py:41-380, model/blocks.py:695-768,915-1123).

Same class names, constructor arguments, forward signature (14 arguments, nine outputs) and state_dict keys,
shapes and order as the reference, so a reference checkpoint loads with strict=True.

One forward per module, run in the mode LinguisticEncoder.forward chooses once per call; each op picks its kernel or
autograd Function for the mode in one place (_conv, _block_norm, _rel_attention, ...).  _INFER (eval mode, unless
grad is enabled and a parameter requires it): the inference kernels only.  _RECORD (any other call with grad
enabled): every op a torch.autograd.Function whose forward and backward are library calls (lingenc_train.hip for the
two attentions and the per-token glue, the conv / LayerNorm / word-pooling / length-regulator Functions otherwise),
with dropout in train mode and p = 0 in eval mode.  _NOGRAD (train mode under no_grad, the D phase of a training
step): the same kernels and dropout, nothing saved.  Dropout keep-masks come from transformer._keep_mask (so
DROPOUT_FN / a module's `dropout_fn` can replay the reference's), requested in the reference's call order and with
its shapes; where the native layout differs the mask is transposed here.

Internally everything is channel-major [B, C, L] like transformer.py's forward_cm: k=1 / k=3 / k=9 convolutions
are the generic conv kernel, LayerNorms are mg_layernorm_cm_fwd, the two attentions and the per-token glue
(embedding gather, pitch / energy / duration heads, position encodings) are lingenc.hip, and word pooling, the
length regulator, the mapping mask and the relative coefficients are lingops.  Every [B, ., 256] tensor is made
by a library kernel; only [B, T] integer bookkeeping (masks) stays in torch.
"""
import json
import os

import numpy as np
import torch
from torch import nn

from . import ops, lingops, _lib, autograd as ag
from ._lib import fptr, iptr, check, stream_ptr
from .blocks import ConvNorm, LinearNorm
from .transformer import get_sinusoid_encoding_table, _keep_mask

# len(text.symbols.symbols) + 1 of the reference (text/symbols.py: pad, punctuation, letters, the ARPAbet set with
# its "@" prefix, pinyin and the silences), the vocabulary of src_emb.  A constant: the text front end is not ours.
N_SRC_VOCAB = 361


def _u8(t):
    return t.to(torch.uint8).contiguous()


# ------------------------------------------------------------------------------------ kernel wrappers
def rel_attention(qkv, valid8, emb_k, emb_v, n_head, window):
    """qkv [B, 3*H*D, L], valid8 uint8 [B, L] (1 = valid), emb_k / emb_v [2w+1, D] -> [B, H*D, L]."""
    B, C3, L = qkv.shape
    d = C3 // (3 * n_head)
    out = torch.empty(B, n_head * d, L, device=qkv.device, dtype=torch.float32)
    check(_lib.lib().mg_rel_attention_fwd(fptr(qkv), iptr(valid8, torch.uint8), fptr(emb_k.contiguous()),
                                          fptr(emb_v.contiguous()), fptr(out), B, L, n_head, d, int(window),
                                          stream_ptr()))
    return out


def w2p_attention(q, kv, key_valid8, query_valid8, mapping8, prior, n_head):
    """q [B, H*D, Lq], kv [B, 2*H*D, Lk] -> (out [B, H*D, Lq], attn, attn_raw [H, B, Lq, Lk], logprob [H, B, 1, Lq, Lk])."""
    B, HD, Lq = q.shape
    Lk = kv.shape[2]
    dev = q.device
    out = torch.empty(B, HD, Lq, device=dev, dtype=torch.float32)
    attn = torch.empty(n_head, B, Lq, Lk, device=dev, dtype=torch.float32)
    raw = torch.empty_like(attn)
    logp = torch.empty(n_head, B, 1, Lq, Lk, device=dev, dtype=torch.float32)
    check(_lib.lib().mg_w2p_attention_fwd(fptr(q), fptr(kv), iptr(key_valid8, torch.uint8),
                                          iptr(query_valid8, torch.uint8), iptr(mapping8, torch.uint8),
                                          fptr(prior, True), fptr(out), fptr(attn), fptr(raw), fptr(logp), B, Lq, Lk,
                                          n_head, HD // n_head, stream_ptr()))
    return out, attn, raw, logp


def embed_cm(ids, table, valid8):
    B, L = ids.shape
    n, C = table.shape
    out = torch.empty(B, C, L, device=table.device, dtype=torch.float32)
    check(_lib.lib().mg_embed_cm(iptr(ids.to(torch.int64).contiguous(), torch.int64), fptr(table), iptr(valid8, torch.uint8),
                                 fptr(out), B, L, C, n, stream_ptr()))
    return out


def variance_head(h, weight, bias, valid8, control, target=None, bins=None, emb=None, x=None):
    """pred [B, L]; with `emb`, also adds the bucketized embedding rows into x [B, C, L] in place."""
    B, C, L = h.shape
    pred = torch.empty(B, L, device=h.device, dtype=torch.float32)
    tgt = None if target is None else target.to(torch.float32).contiguous()
    check(_lib.lib().mg_variance_head(fptr(h), fptr(weight.reshape(-1).contiguous()), fptr(bias), iptr(valid8, torch.uint8),
                                      float(control), fptr(tgt, True), fptr(bins, True),
                                      0 if bins is None else bins.numel(), fptr(emb, True), fptr(pred), fptr(x, True),
                                      B, C, L, stream_ptr()))
    return pred


def duration_head(logp, target, wb, src_w_len, d_control, W):
    B, Tp = logp.shape
    logw = torch.empty(B, W, device=logp.device, dtype=torch.float32)
    dur = torch.empty(B, W, device=logp.device, dtype=torch.int64)
    tgt = None if target is None else target.to(torch.int64).contiguous()
    check(_lib.lib().mg_duration_head(fptr(logp), iptr(tgt, torch.int64, True), iptr(wb.to(torch.int64).contiguous(), torch.int64),
                                      iptr(src_w_len.to(torch.int64).contiguous(), torch.int64), float(d_control),
                                      fptr(logw), iptr(dur, torch.int64), B, Tp, wb.shape[1], W, stream_ptr()))
    return logw, dur


def posenc_add(x, rowmajor, coef, table):
    """-> [B, C, L] channel-major = x + coef[:, :, None] * table[:L] (x [B, L, C] when rowmajor else [B, C, L])."""
    if rowmajor:
        B, L, C = x.shape
    else:
        B, C, L = x.shape
    out = torch.empty(B, C, L, device=x.device, dtype=torch.float32)
    check(_lib.lib().mg_posenc_add(fptr(x), int(rowmajor), fptr(coef), fptr(table), fptr(out), B, C, L, stream_ptr()))
    return out


# ------------------------------------------------------------------------------------ training (lingenc_train.hip)
def _ws(n):
    return torch.empty(max(int(n), 1), device="cuda", dtype=torch.float32)


def rel_attention_train(qkv, valid8, emb_k, emb_v, n_head, window, keep=None, keep_scale=1.0, save=True):
    """Train-mode rel_attention: dropout(P) with the uint8 keep-mask [B, H, L, L] -> (out, P or None)."""
    B, C3, L = qkv.shape
    d = C3 // (3 * n_head)
    out = torch.empty(B, n_head * d, L, device=qkv.device, dtype=torch.float32)
    P = torch.empty(B, n_head, L, L, device=qkv.device, dtype=torch.float32) if save else None
    check(_lib.lib().mg_rel_attention_train_fwd(fptr(qkv), iptr(valid8, torch.uint8), fptr(emb_k.contiguous()),
                                                fptr(emb_v.contiguous()), iptr(keep, torch.uint8, True),
                                                float(keep_scale), fptr(out), fptr(P, True), B, L, n_head, d,
                                                int(window), stream_ptr()))
    return out, P


def rel_attention_bwd(qkv, valid8, P, keep, keep_scale, d_out, emb_k, emb_v, n_head, window):
    """-> (d_qkv [B, 3HD, L], d_emb_k, d_emb_v [2w+1, D])."""
    B, C3, L = qkv.shape
    d = C3 // (3 * n_head)
    Lb = _lib.lib()
    n = Lb.mg_rel_attention_bwd_ws_floats(B, L, n_head, int(window))
    ws = _ws(n)
    dqkv = torch.empty_like(qkv)
    dek = torch.empty_like(emb_k)
    dev_ = torch.empty_like(emb_v)
    check(Lb.mg_rel_attention_bwd(fptr(qkv), iptr(valid8, torch.uint8), fptr(P), iptr(keep, torch.uint8, True),
                                  float(keep_scale), fptr(d_out), fptr(emb_k.contiguous()), fptr(emb_v.contiguous()),
                                  fptr(dqkv), fptr(dek), fptr(dev_), fptr(ws), ws.numel(), B, L, n_head, d, int(window),
                                  stream_ptr()))
    return dqkv, dek, dev_


def w2p_attention_bwd(q, kv, key_valid8, query_valid8, mapping8, prior, attn, raw, logp, d_out, d_attn, d_raw, d_logp,
                      n_head):
    """-> (dq [B, HD, Lq], dkv [B, 2HD, Lk]); d_attn / d_raw / d_logp may be None."""
    B, HD, Lq = q.shape
    Lk = kv.shape[2]
    Lb = _lib.lib()
    ws = _ws(Lb.mg_w2p_attention_bwd_ws_floats(B, Lq, Lk, n_head))
    dq = torch.empty_like(q)
    dkv = torch.empty_like(kv)
    c = lambda t: None if t is None else t.contiguous()  # noqa: E731
    check(Lb.mg_w2p_attention_bwd(fptr(q), fptr(kv), iptr(key_valid8, torch.uint8), iptr(query_valid8, torch.uint8),
                                  iptr(mapping8, torch.uint8), fptr(prior, True), fptr(attn), fptr(raw), fptr(logp),
                                  fptr(d_out), fptr(c(d_attn), True), fptr(c(d_raw), True), fptr(c(d_logp), True),
                                  fptr(dq), fptr(dkv), fptr(ws), ws.numel(), B, Lq, Lk, n_head, HD // n_head,
                                  stream_ptr()))
    return dq, dkv


def embed_cm_bwd(ids, d_out, valid8, n_rows, skip_row=-1):
    """nn.Embedding's weight gradient [n_rows, C] from a channel-major output gradient [B, C, L]."""
    B, C, L = d_out.shape
    dt = torch.empty(n_rows, C, device=d_out.device, dtype=torch.float32)
    check(_lib.lib().mg_embed_cm_bwd(iptr(ids.to(torch.int64).contiguous(), torch.int64), fptr(d_out),
                                     iptr(valid8, torch.uint8, True), fptr(dt), B, L, C, n_rows, int(skip_row),
                                     stream_ptr()))
    return dt


def variance_head_bwd(h, weight, valid8, scale, d_pred):
    B, C, L = h.shape
    dh = torch.empty_like(h)
    dw = torch.empty(C, device=h.device, dtype=torch.float32)
    db = torch.empty(1, device=h.device, dtype=torch.float32)
    check(_lib.lib().mg_variance_head_bwd(fptr(h), fptr(weight.reshape(-1).contiguous()), iptr(valid8, torch.uint8),
                                          float(scale), fptr(d_pred), fptr(dh), fptr(dw), fptr(db), B, C, L,
                                          stream_ptr()))
    return dh, dw, db


def duration_head_bwd(logp, logw, d_logw, wb, src_w_len):
    B, Tp = logp.shape
    d = torch.empty_like(logp)
    check(_lib.lib().mg_duration_head_bwd(fptr(logp), fptr(logw), fptr(d_logw), iptr(wb, torch.int64),
                                          iptr(src_w_len, torch.int64), fptr(d), B, Tp, wb.shape[1], logw.shape[1],
                                          stream_ptr()))
    return d


def posenc_add_bwd(d_out, coef):
    """-> d table[:L] [L, C] = sum_b coef[b, l] * d_out[b, :, l]."""
    B, C, L = d_out.shape
    dt = torch.empty(L, C, device=d_out.device, dtype=torch.float32)
    check(_lib.lib().mg_posenc_add_bwd(fptr(d_out), fptr(coef), fptr(dt), B, C, L, stream_ptr()))
    return dt


def dropout_apply(x, keep, scale):
    out = torch.empty_like(x)
    check(_lib.lib().mg_dropout_apply(fptr(x), iptr(keep, torch.uint8), float(scale), fptr(out), x.numel(),
                                      stream_ptr()))
    return out


class _RelAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, emb_k, emb_v, valid8, keep, scale, n_head, window):
        qkv = qkv.contiguous()
        out, P = rel_attention_train(qkv, valid8, emb_k.detach(), emb_v.detach(), n_head, window, keep, scale)
        ctx.save_for_backward(qkv, emb_k, emb_v, valid8, P, keep if keep is not None else P.new_empty(0, dtype=torch.uint8))
        ctx.cfg = (keep is not None, scale, n_head, window)
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, emb_k, emb_v, valid8, P, keep = ctx.saved_tensors
        has_keep, scale, n_head, window = ctx.cfg
        dqkv, dek, dev_ = rel_attention_bwd(qkv, valid8, P, keep if has_keep else None, scale, g.contiguous(),
                                            emb_k.detach(), emb_v.detach(), n_head, window)
        return dqkv, dek, dev_, None, None, None, None, None


class _W2PAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, kv, key_valid8, query_valid8, mapping8, prior, n_head):
        ctx.set_materialize_grads(False)
        q, kv = q.contiguous(), kv.contiguous()
        out, attn, raw, logp = w2p_attention(q, kv, key_valid8, query_valid8, mapping8, prior, n_head)
        ctx.save_for_backward(q, kv, key_valid8, query_valid8, mapping8,
                              prior if prior is not None else q.new_empty(0), attn, raw, logp)
        ctx.cfg = (prior is not None, n_head)
        return out, attn, raw, logp

    @staticmethod
    def backward(ctx, d_out, d_attn, d_raw, d_logp):
        q, kv, kvalid, qvalid, mapping, prior, attn, raw, logp = ctx.saved_tensors
        has_prior, n_head = ctx.cfg
        if d_out is None:
            d_out = torch.zeros_like(q)
        dq, dkv = w2p_attention_bwd(q, kv, kvalid, qvalid, mapping, prior if has_prior else None, attn, raw, logp,
                                    d_out.contiguous(), d_attn, d_raw, d_logp, n_head)
        return dq, dkv, None, None, None, None, None


class _EmbedFn(torch.autograd.Function):
    """src_emb gather into [B, C, L] (pads zeroed); the padding_idx row gets no gradient."""

    @staticmethod
    def forward(ctx, table, ids, valid8, padding_idx):
        ctx.save_for_backward(ids, valid8)
        ctx.cfg = (table.shape[0], -1 if padding_idx is None else padding_idx)
        return embed_cm(ids, table.detach().contiguous(), valid8)

    @staticmethod
    def backward(ctx, g):
        ids, valid8 = ctx.saved_tensors
        n, skip = ctx.cfg
        return embed_cm_bwd(ids, g.contiguous(), valid8, n, skip), None, None, None


class _VarianceHeadFn(torch.autograd.Function):
    """(pred [B, L], x + emb[bucket] [B, C, L]) = mg_variance_head on a copy of x; without `emb` only pred.
    `bucket` ([B, L] int64, bucketize of the target or of the detached prediction) routes the embedding gradient."""

    @staticmethod
    def forward(ctx, h, weight, bias, x, emb, valid8, control, target, bins):
        h = h.contiguous()
        x2 = None if x is None else x.detach().clone()
        pred = variance_head(h, weight.detach(), bias.detach(), valid8, control, target, bins,
                             None if emb is None else emb.detach().contiguous(), x2)
        bucket = None
        if emb is not None:
            bucket = torch.bucketize(target if target is not None else pred, bins)
        ctx.save_for_backward(h, weight, valid8, bucket if bucket is not None else valid8.new_empty(0, dtype=torch.int64))
        ctx.cfg = (1.0 if target is not None else float(control), None if emb is None else emb.shape[0])
        if x2 is None:
            return pred
        return pred, x2

    @staticmethod
    def backward(ctx, d_pred, d_x2=None):
        h, weight, valid8, bucket = ctx.saved_tensors
        scale, n_emb = ctx.cfg
        if d_pred is None:
            d_pred = torch.zeros(h.shape[0], h.shape[2], device=h.device)
        dh, dw, db = variance_head_bwd(h, weight.detach(), valid8, scale, d_pred.contiguous())
        dx = demb = None
        if n_emb is not None and d_x2 is not None:
            dx = d_x2
            demb = embed_cm_bwd(bucket, d_x2.contiguous(), None, n_emb)
        return dh, dw.reshape(weight.shape), db, dx, demb, None, None, None, None


class _DurationHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, target, wb, src_w_len, d_control, W):
        logp = logp.contiguous()
        logw, dur = duration_head(logp, target, wb, src_w_len, d_control, W)
        ctx.save_for_backward(logp, logw, wb, src_w_len)
        ctx.mark_non_differentiable(dur)
        return logw, dur

    @staticmethod
    def backward(ctx, d_logw, _):
        logp, logw, wb, src_w_len = ctx.saved_tensors
        return duration_head_bwd(logp, logw, d_logw.contiguous(), wb, src_w_len), None, None, None, None, None


class _PosencAddFn(torch.autograd.Function):
    """posenc_add with gradients to x and to the position-encoding parameter's first L rows."""

    @staticmethod
    def forward(ctx, x, param, rowmajor, coef):
        L = x.shape[1] if rowmajor else x.shape[2]
        ctx.save_for_backward(coef)
        ctx.cfg = (rowmajor, tuple(param.shape), L)
        return posenc_add(x.contiguous(), rowmajor, coef, param.detach()[0])

    @staticmethod
    def backward(ctx, g):
        (coef,) = ctx.saved_tensors
        rowmajor, pshape, L = ctx.cfg
        g = g.contiguous()
        dx = ops.transpose_bml(g, True) if rowmajor else g
        dp = None
        if ctx.needs_input_grad[1]:
            dp = torch.zeros(pshape, device=g.device, dtype=torch.float32)
            dp[0, :L] = posenc_add_bwd(g, coef)
        return dx, dp, None, None


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, keep, scale):
        ctx.save_for_backward(keep)
        ctx.scale = scale
        return dropout_apply(x.contiguous(), keep, scale)

    @staticmethod
    def backward(ctx, g):
        (keep,) = ctx.saved_tensors
        return dropout_apply(g.contiguous(), keep, ctx.scale), None, None


class _LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the channels of [B, C, L] (the VariancePredictor's), no residual, no pad."""

    @staticmethod
    def forward(ctx, a, gamma, beta, eps):
        out, pre = ops.layernorm_cm_train(a.contiguous(), None, 1.0, None, gamma.detach(), beta.detach(), None, eps)
        ctx.save_for_backward(pre, gamma)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, g):
        pre, gamma = ctx.saved_tensors
        d_pre, _, dg, db = ops.layernorm_cm_bwd(pre, g.contiguous(), gamma.detach(), None, None, 1.0, ctx.eps)
        return d_pre, dg, db, None


class _LinearAddFn(torch.autograd.Function):
    """y = W x + res on [B, C, L] (a bias-free k=1 conv with the residual added in its epilogue)."""

    @staticmethod
    def forward(ctx, x, weight, res):
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        return ops.conv1d_packed(x, ops.pack_cached(weight[:, :, None]), None, weight.shape[0], 1,
                                 add=res.contiguous())

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        dx = ops.conv1d_packed(g, ops.pack_cached(weight[:, :, None], ops.PACK_DGRAD), None, weight.shape[1], 1,
                               split=True)
        dw = ops.conv1d_wgrad(g, x, 1)[:, :, 0] if ctx.needs_input_grad[1] else None
        return dx, dw, g


class _MaskedToCmFn(torch.autograd.Function):
    """[B, L, C] -> [B, C, L] with the padded frames zeroed (the block's x * x_mask)."""

    @staticmethod
    def forward(ctx, x, keep8):
        return ops.transpose_bml(x.contiguous(), False, keep=keep8)

    @staticmethod
    def backward(ctx, g):
        return ops.transpose_bml(g.contiguous(), True), None


class CpuTrainingError(_lib.MixganHipError, NotImplementedError):
    """A train-mode or grad-enabled forward on CPU tensors: training runs on the HIP path only.  Both a library
    error (no CPU fallback) and NotImplementedError (the native encoder does not train on the CPU)."""


# ------------------------------------------------------------------------------------ per-op choice by mode
_INFER, _RECORD, _NOGRAD = "infer", "record", "no_grad"


def _stack(ts):
    return ts[0] if len(ts) == 1 else torch.cat(ts)


def _packed(*weights):
    """Inference pack of `weights` stacked along Co (k=1 ones may be [Co, Ci]), each packed once per parameter
    version; a single Conv1d weight's pack is used as it is."""
    if len(weights) == 1 and weights[0].dim() == 3:
        return ops.pack_cached(weights[0])
    return torch.cat([ops.pack_cached(w[:, :, None] if w.dim() == 2 else w) for w in weights])


def _keep(mode, module, shape, p, device):
    """Keep-mask and scale of `module`'s dropout(p): none in inference, p = 0 in eval mode (grad enabled)."""
    if mode == _INFER:
        return None, 1.0
    return _keep_mask(module, tuple(shape), p if module.training else 0.0, device)


def _conv(mode, x, weights, biases=(), padding=0, act=None, add=None):
    """Stride-1 convolution of x [B, Ci, L] by `weights` (Conv1d [Co, Ci, k] or k=1 Linear [Co, Ci]) stacked along Co
    plus their stacked `biases`, then `act`; `add` (one bias-free k=1 weight) is a residual added in the epilogue.
    Inference: the conv kernel on the cached packs, no split.  Training: ag.conv1d (split reduction), or _LinearAddFn
    with `add`."""
    w = weights[0]
    if mode == _INFER:
        packed = _packed(*weights)
        b = _stack(biases).detach() if biases else None
        return ops.conv1d_packed(x, packed, b, w.shape[0] * len(weights), w.shape[2] if w.dim() == 3 else 1, 1,
                                 padding, act, add=add)
    if add is not None:
        return _LinearAddFn.apply(x, w, add)
    w = _stack(weights)
    return ag.conv1d(x, w if w.dim() == 3 else w[:, :, None], _stack(biases) if biases else None, 1, padding, act)


def _block_norm(mode, y, x, norm, pad8, keep, scale):
    """LayerNorm(dropout(y) + x) of a RelativeFFTBlock, pads zeroed."""
    if mode == _INFER:
        return ops.layernorm_cm(y, x, norm.gamma.detach(), norm.beta.detach(), pad8, norm.eps)
    return ag.layernorm_train(y, x, norm.gamma, norm.beta, pad8, keep, scale, norm.eps)


def _norm_drop(mode, module, h, norm):
    """dropout(nn.LayerNorm(h)) of a VariancePredictor; the keep-mask is drawn [B, L, F] (the reference's channel-last
    layout) and transposed."""
    if mode == _INFER:
        return ops.layernorm_cm(h, None, norm.weight.detach(), norm.bias.detach(), None, norm.eps)
    h = _LayerNormFn.apply(h, norm.weight, norm.bias, norm.eps)
    B, F, L = h.shape
    keep, scale = _keep(mode, module, (B, L, F), module.dropout_p, h.device)
    return h if keep is None else _DropoutFn.apply(h, keep.transpose(1, 2).contiguous(), scale)


def _rel_attention(mode, qkv, valid8, emb_k, emb_v, keep, scale, n_head, window):
    if mode == _INFER:
        return rel_attention(qkv, valid8, emb_k.detach(), emb_v.detach(), n_head, window)
    if mode == _RECORD:
        return _RelAttentionFn.apply(qkv, emb_k, emb_v, valid8, keep, scale, n_head, window)
    return rel_attention_train(qkv, valid8, emb_k, emb_v, n_head, window, keep, scale, save=False)[0]


def _to_rm(mode, x):
    """[B, C, L] -> [B, L, C]."""
    return ops.transpose_bml(x, True) if mode == _INFER else ag.transpose_to_blm(x)


# ------------------------------------------------------------------------------------ modules
class LayerNorm(nn.Module):
    """model/blocks.py:258-276: channel LayerNorm with `gamma` / `beta`, eps 1e-4."""

    def __init__(self, channels, eps=1e-4):
        super().__init__()
        self.channels, self.eps = channels, eps
        self.gamma = nn.Parameter(torch.ones(channels))
        self.beta = nn.Parameter(torch.zeros(channels))


class _Conv1d(nn.Module):
    """nn.Conv1d parameter holder (`weight`, `bias`)."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        c = nn.Conv1d(in_channels, out_channels, kernel_size)
        self.weight, self.bias = c.weight, c.bias


class RelativeSelfAttention(nn.Module):
    """model/blocks.py:978-1061 (heads_share=True, no block_length / proximal bias)."""

    def __init__(self, channels, out_channels, n_heads, window_size=None, heads_share=True, p_dropout=0.):
        super().__init__()
        if window_size is None or not heads_share:
            raise NotImplementedError("the native encoder implements the reference's windowed, head-shared form")
        self.channels, self.n_heads, self.window_size = channels, n_heads, window_size
        self.k_channels = channels // n_heads
        self.conv_q = _Conv1d(channels, channels, 1)
        self.conv_k = _Conv1d(channels, channels, 1)
        self.conv_v = _Conv1d(channels, channels, 1)
        rel_stddev = self.k_channels ** -0.5
        self.emb_rel_k = nn.Parameter(torch.randn(1, window_size * 2 + 1, self.k_channels) * rel_stddev)
        self.emb_rel_v = nn.Parameter(torch.randn(1, window_size * 2 + 1, self.k_channels) * rel_stddev)
        self.conv_o = _Conv1d(channels, out_channels, 1)
        self.p_dropout = p_dropout

    def forward_cm(self, x, valid8, mode):
        """conv_o(attention, with dropout on p_attn in training) (before the block's drop(y))."""
        B, C, L = x.shape
        keep, scale = _keep(mode, self, (B, self.n_heads, L, L), self.p_dropout, x.device)
        qkv = _conv(mode, x, (self.conv_q.weight, self.conv_k.weight, self.conv_v.weight),
                    (self.conv_q.bias, self.conv_k.bias, self.conv_v.bias))
        att = _rel_attention(mode, qkv, valid8, self.emb_rel_k[0], self.emb_rel_v[0], keep, scale, self.n_heads,
                             self.window_size)
        return _conv(mode, att, (self.conv_o.weight,), (self.conv_o.bias,))


class FFN(nn.Module):
    """model/blocks.py:956-976: one Conv1d(k) + ReLU (the reference's default activation)."""

    def __init__(self, in_channels, out_channels, kernel_size, p_dropout=0., activation=None):
        super().__init__()
        if activation is not None:
            raise NotImplementedError("RelativeFFTBlock builds its FFN with the ReLU activation")
        self.kernel_size = kernel_size
        self.p_dropout = p_dropout
        self.conv = _Conv1d(in_channels, out_channels, kernel_size)

    def forward_cm(self, x, mode):
        return _conv(mode, x, (self.conv.weight,), (self.conv.bias,), self.kernel_size // 2, "relu")


class RelativeFFTBlock(nn.Module):
    """model/blocks.py:915-954."""

    def __init__(self, hidden_channels, filter_channels, n_heads, n_layers, kernel_size=1, p_dropout=0.,
                 window_size=None):
        super().__init__()
        self.n_layers = n_layers
        self.p_dropout = p_dropout
        self.attn_layers = nn.ModuleList()
        self.norm_layers_1 = nn.ModuleList()
        self.ffn_layers = nn.ModuleList()
        self.norm_layers_2 = nn.ModuleList()
        for _ in range(n_layers):
            self.attn_layers.append(RelativeSelfAttention(hidden_channels, hidden_channels, n_heads,
                                                          window_size=window_size, p_dropout=p_dropout))
            self.norm_layers_1.append(LayerNorm(hidden_channels))
            self.ffn_layers.append(FFN(hidden_channels, hidden_channels, kernel_size, p_dropout=p_dropout))
            self.norm_layers_2.append(LayerNorm(hidden_channels))

    def forward_cm(self, x, valid8, pad8, mode):
        """x [B, C, L] with zeros at the pads -> the block's output (zeros at the pads).

        The reference masks x at the top of every layer, the FFN's input and output, and the block's output.  Every
        LayerNorm here zeroes its padded frames instead: a frame's LayerNorm reads only that frame, the convolutions
        and the attention read the pads only through those masks, so the valid frames and the (zero) pads of the
        block's output are the reference's.

        In training (model/blocks.py:941-954) the keep-masks are requested per layer in the reference's order: p_attn,
        drop(y) after the attention, the FFN's inner drop and drop(y) after the FFN.  The FFN's two dropouts act on the
        same tensor one after the other, so they enter the LayerNorm kernel as one mask (keep1 * keep2, s1 * s2)."""
        for i in range(self.n_layers):
            n1, n2, ffn = self.norm_layers_1[i], self.norm_layers_2[i], self.ffn_layers[i]
            y = self.attn_layers[i].forward_cm(x, valid8, mode)
            keep, scale = _keep(mode, self, y.shape, self.p_dropout, y.device)
            x = _block_norm(mode, y, x, n1, pad8, keep, scale)
            y = ffn.forward_cm(x, mode)
            keep1, s1 = _keep(mode, ffn, y.shape, ffn.p_dropout, y.device)
            keep2, s2 = _keep(mode, self, y.shape, self.p_dropout, y.device)
            if keep1 is not None and keep2 is not None:
                keep1, keep2 = (keep1 & keep2).contiguous(), None
            x = _block_norm(mode, y, x, n2, pad8, keep1 if keep1 is not None else keep2, s1 * s2)
        return x


class VariancePredictor(nn.Module):
    """model/linguistic_encoder.py:419-478: (ConvNorm k -> ReLU -> LayerNorm) x 2 -> Linear(., 1) -> * mask."""

    def __init__(self, model_config):
        super().__init__()
        from collections import OrderedDict
        self.input_size = model_config["transformer"]["encoder_hidden"]
        self.filter_size = model_config["variance_predictor"]["filter_size"]
        self.kernel = model_config["variance_predictor"]["kernel_size"]
        self.conv_output_size = self.filter_size
        self.conv_layer = nn.Sequential(OrderedDict([
            ("conv1d_1", ConvNorm(self.input_size, self.filter_size, kernel_size=self.kernel, padding=(self.kernel - 1) // 2)),
            ("layer_norm_1", nn.LayerNorm(self.filter_size)),
            ("conv1d_2", ConvNorm(self.filter_size, self.filter_size, kernel_size=self.kernel, padding=1)),
            ("layer_norm_2", nn.LayerNorm(self.filter_size)),
        ]))
        self.linear_layer = nn.Linear(self.conv_output_size, 1)
        self.dropout_p = model_config["variance_predictor"]["dropout"]

    def hidden_cm(self, x, mode):
        """(conv -> ReLU -> LayerNorm -> dropout in training) x 2 on x [B, C, L] (pads are read as they are, like the
        reference) -> [B, filter, L]."""
        cl = self.conv_layer
        for conv, norm in ((cl.conv1d_1, cl.layer_norm_1), (cl.conv1d_2, cl.layer_norm_2)):
            x = _conv(mode, x, (conv.conv.weight,), (conv.conv.bias,), conv.padding, "relu")
            x = _norm_drop(mode, self, x, norm)
        return x

    def head(self, h, valid8, mode, control=1.0, target=None, bins=None, emb=None, x=None):
        """-> pred, or (pred, x + emb[bucket]) with `emb`: inference adds into x in place, training into a copy."""
        lin = self.linear_layer
        if mode == _INFER:
            pred = variance_head(h, lin.weight.detach(), lin.bias.detach(), valid8, control, target, bins,
                                 None if emb is None else emb.detach(), x)
            return pred if emb is None else (pred, x)
        return _VarianceHeadFn.apply(h, lin.weight, lin.bias, x, emb, valid8, control,
                                     None if target is None else target.to(torch.float32).contiguous(), bins)


class WordToPhonemeAttention(nn.Module):
    """model/blocks.py:673-739 (bias-free LinearNorm projections and fc)."""

    def __init__(self, n_head, d_model, d_k, d_v, dropout=0.0):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.w_qs = LinearNorm(d_model, n_head * d_k)
        self.w_ks = LinearNorm(d_model, n_head * d_k)
        self.w_vs = LinearNorm(d_model, n_head * d_v)
        self.fc = LinearNorm(n_head * d_v, d_model)

    def forward_cm(self, q_in, kv_in, key_valid8, query_valid8, mapping8, attn_prior, mode):
        """q_in [B, D, Lq], kv_in [B, D, Lk] (k and v are the same tensor in the encoder) ->
        (fc(attention) + q_in [B, D, Lq], (attn, attn_raw) [H, B, Lq, Lk], attn_logprob [H, B, 1, Lq, Lk])."""
        q = _conv(mode, q_in, (self.w_qs.linear.weight,))
        kv = _conv(mode, kv_in, (self.w_ks.linear.weight, self.w_vs.linear.weight))
        prior = None if attn_prior is None else attn_prior.to(torch.float32).contiguous()
        attend = _W2PAttentionFn.apply if mode == _RECORD else w2p_attention
        out, attn, raw, logp = attend(q, kv, key_valid8, query_valid8, mapping8, prior, self.n_head)
        y = _conv(mode, out, (self.fc.linear.weight,), add=q_in)
        return y, (attn, raw), logp


class LinguisticEncoder(nn.Module):
    """model/linguistic_encoder.py:41-380."""

    def __init__(self, preprocess_config, model_config, train_config):
        super().__init__()
        tc = model_config["transformer"]
        n_position = model_config["max_seq_len"] + 1
        d_model = tc["encoder_hidden"]
        n_head = tc["encoder_head"]
        d_k = d_v = d_model // n_head
        n_layers, kernel_size = tc["encoder_layer"], tc["conv_kernel_size"]
        dropout, window_size = tc["encoder_dropout"], tc["encoder_window_size"]
        self.helper_type = train_config["aligner"]["helper_type"]
        self.max_seq_len = model_config["max_seq_len"]
        self.d_model, self.n_head = d_model, n_head

        self.pitch_feature_level = preprocess_config["preprocessing"]["pitch"]["feature"]
        self.energy_feature_level = preprocess_config["preprocessing"]["energy"]["feature"]
        for lvl in (self.pitch_feature_level, self.energy_feature_level):
            if lvl == "frame_level":
                raise NotImplementedError("frame_level pitch / energy: the reference's own forward cannot broadcast "
                                          "frame-level predictions against phoneme-level encoder output")
            if lvl != "phoneme_level":
                raise ValueError("unknown variance feature level %r" % (lvl,))

        self.src_emb = nn.Embedding(N_SRC_VOCAB, d_model, padding_idx=0)
        table = get_sinusoid_encoding_table(n_position, d_model).unsqueeze(0)
        self.abs_position_enc = nn.Parameter(table.clone(), requires_grad=False)
        self.kv_position_enc = nn.Parameter(table.clone(), requires_grad=True)
        self.q_position_enc = nn.Parameter(table.clone(), requires_grad=True)
        self.phoneme_encoder = RelativeFFTBlock(d_model, tc["conv_filter_size"], n_head, n_layers, kernel_size,
                                                dropout, window_size)
        self.word_encoder = RelativeFFTBlock(d_model, tc["conv_filter_size"], n_head, n_layers, kernel_size,
                                             dropout, window_size)
        self.length_regulator = lingops.LengthRegulator()
        self.duration_predictor = VariancePredictor(model_config)
        self.pitch_predictor = VariancePredictor(model_config)
        self.energy_predictor = VariancePredictor(model_config)
        self.w2p_attn = WordToPhonemeAttention(n_head, d_model, d_k, d_v)

        ve = model_config["variance_embedding"]
        n_bins = ve["n_bins"]
        with open(os.path.join(preprocess_config["path"]["preprocessed_path"], "stats.json")) as f:
            stats = json.load(f)
        pitch_min, pitch_max = stats["pitch"][:2]
        energy_min, energy_max = stats["energy"][:2]

        def bins(quant, lo, hi):
            if quant == "log":
                return torch.exp(torch.linspace(np.log(lo), np.log(hi), n_bins - 1))
            if quant == "linear":
                return torch.linspace(lo, hi, n_bins - 1)
            raise ValueError("quantization must be 'linear' or 'log', got %r" % (quant,))
        self.pitch_bins = nn.Parameter(bins(ve["pitch_quantization"], pitch_min, pitch_max), requires_grad=False)
        self.energy_bins = nn.Parameter(bins(ve["energy_quantization"], energy_min, energy_max), requires_grad=False)
        self.pitch_embedding = nn.Embedding(n_bins, d_model)
        self.energy_embedding = nn.Embedding(n_bins, d_model)
        self._tables = {}
        self.record = False     # True: keep enc_p_out / the word encoder's output in self.recorded (tests)
        self.recorded = None

    def _table(self, position_enc, L, device):
        """add_position_enc's table (linguistic_encoder.py:201-220): the parameter's first L rows, or in eval a fresh
        sinusoid table when the sequence is longer than max_seq_len."""
        if L > self.max_seq_len:
            key = (L, str(device))
            t = self._tables.get(key)
            if t is None:
                t = get_sinusoid_encoding_table(L, self.d_model).to(device).contiguous()
                self._tables[key] = t
            return t
        return position_enc.detach()[0]

    def _posenc(self, x, rowmajor, coef, position_enc, mode):
        """x + coef * position_enc -> [B, C, L]; training has no table past max_seq_len (_check_len)."""
        if mode == _INFER:
            L = x.shape[1] if rowmajor else x.shape[2]
            return posenc_add(x, rowmajor, coef, self._table(position_enc, L, x.device))
        return _PosencAddFn.apply(x, position_enc, rowmajor, coef)

    def _check_len(self, n, what):
        if n > self.max_seq_len:
            raise ValueError("LinguisticEncoder training: %d %s exceed max_seq_len %d (the position-encoding tables "
                             "have max_seq_len + 1 rows)" % (n, what, self.max_seq_len))

    def forward(self, src_p_seq, src_p_len, word_boundary, src_p_mask, src_w_len, src_w_mask, mel_mask=None,
                max_len=None, attn_prior=None, pitch_target=None, energy_target=None, duration_target=None,
                p_control=1.0, duration_control=1.0):
        """model/linguistic_encoder.py:238-380 in the mode of this call (module docstring).  In training the keep-masks
        are requested in the reference's order: phoneme encoder, pitch predictor, energy predictor, word encoder,
        duration predictor."""
        grad = torch.is_grad_enabled()
        train = self.training or (grad and any(p.requires_grad for p in self.parameters()))
        mode = (_RECORD if grad else _NOGRAD) if train else _INFER
        B, Tp = src_p_mask.shape
        if mode != _INFER:
            self._check_len(Tp, "phonemes")
        if not src_p_seq.is_cuda:
            if mode == _INFER:
                raise _lib.MixganHipError("LinguisticEncoder on %s: the HIP path has no CPU fallback"
                                          % src_p_seq.device)
            raise CpuTrainingError(
                "LinguisticEncoder training on %s: the HIP path has no CPU fallback (move the inputs to the GPU, or "
                "inject the reference's model.linguistic_encoder.LinguisticEncoder to train on the CPU)"
                % src_p_seq.device)
        dev = src_p_seq.device
        W = src_w_mask.shape[1]
        pv8, pp8 = _u8(src_p_mask), _u8(~src_p_mask.bool())
        wv8, wp8 = _u8(src_w_mask), _u8(~src_w_mask.bool())
        wb = word_boundary.to(torch.int64).contiguous()
        src_w_len = src_w_len.to(torch.int64).contiguous()

        # phoneme encoder (:318-320), pitch / energy embeddings added at every phoneme, pads included (:322-333)
        if mode == _INFER:
            x = embed_cm(src_p_seq[:, :Tp], self.src_emb.weight.detach(), pv8)
        else:
            x = _EmbedFn.apply(self.src_emb.weight, src_p_seq[:, :Tp].to(torch.int64).contiguous(), pv8,
                               self.src_emb.padding_idx)
        enc_p = self.phoneme_encoder.forward_cm(x, pv8, pp8, mode)
        pp, ep = self.pitch_predictor, self.energy_predictor
        pitch_prediction, enc_p = pp.head(pp.hidden_cm(enc_p, mode), pv8, mode, p_control, pitch_target,
                                          self.pitch_bins.detach(), self.pitch_embedding.weight, enc_p)
        energy_prediction, enc_p = ep.head(ep.hidden_cm(enc_p, mode), pv8, mode, p_control, energy_target,
                                           self.energy_bins.detach(), self.energy_embedding.weight, enc_p)

        # word pooling -> word encoder (:347-353)
        enc_p_rm = _to_rm(mode, enc_p)
        src_w_seq = lingops.word_level_pooling(enc_p_rm, src_p_len, wb, src_w_len, "mean", max_words=W)
        if mode == _INFER:
            src_w_seq = ops.transpose_bml(src_w_seq, False, keep=wv8)
        else:
            src_w_seq = _MaskedToCmFn.apply(src_w_seq, wv8)
        enc_w = self.word_encoder.forward_cm(src_w_seq, wv8, wp8, mode)
        enc_w_rm = _to_rm(mode, enc_w)
        if self.record:
            self.recorded = {"enc_p_out": enc_p_rm, "enc_w_out": enc_w_rm}

        # durations (:355-376)
        dp = self.duration_predictor
        log_d_p = dp.head(dp.hidden_cm(enc_p, mode), pv8, mode)
        log_duration_w_prediction, duration_w_rounded = (duration_head if mode == _INFER else _DurationHeadFn.apply)(
            log_d_p, duration_target, wb, src_w_len, duration_control, W)
        xr, mel_len = self.length_regulator(enc_w_rm, duration_w_rounded, max_len)
        if duration_target is None:
            ids = torch.arange(xr.shape[1], device=dev)
            mel_mask = ids[None, :] < mel_len[:, None]
        if mode != _INFER:
            self._check_len(xr.shape[1], "frames")

        # word-to-phoneme attention (:378-407); k and v share one input, and their rel coefficients are one tensor
        mapping = lingops.get_mapping_mask(xr, enc_p_rm, duration_w_rounded, wb, src_w_len)
        coef_q = lingops.get_rel_coef(duration_w_rounded, src_w_len, mel_mask)
        coef_kv = lingops.get_rel_coef(wb, src_p_len, src_p_mask)
        q_in = self._posenc(xr, True, coef_q, self.q_position_enc, mode)
        kv_in = self._posenc(enc_p, False, coef_kv, self.kv_position_enc, mode)
        y, attns, attn_logprob = self.w2p_attn.forward_cm(
            q_in, kv_in, pv8, _u8(mel_mask), _u8(mapping), attn_prior if self.helper_type == "ctc" else None, mode)
        out = _to_rm(mode, y)
        return (out, pitch_prediction, energy_prediction, log_duration_w_prediction, duration_w_rounded, mel_len,
                mel_mask, attns, attn_logprob)
