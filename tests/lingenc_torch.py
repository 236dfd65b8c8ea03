"""Plain-PyTorch restatement of the reference's LinguisticEncoder forward in eval mode, written from its semantics
(like oracle/refmath.py), for the kernel and full-encoder tests of tests/test_gpu_linguistic_encoder.py and the
stock-eager comparison of tools/lingenc_bench.py.  Works on a state dict with the reference's keys.  Vectorised: no
per-phoneme Python loop, so it also runs at B=16 / 1000 frames on the GPU.

Citations are to the reference: model/linguistic_encoder.py (LE), model/blocks.py (BL), utils/tools.py (UT).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def sinusoid(n, d):
    """LE:19-38 (float64, cast to fp32)."""
    pos = np.arange(n, dtype=np.float64)[:, None]
    j = np.arange(d)[None, :]
    t = pos / np.power(10000, 2 * (j // 2) / d)
    t[:, 0::2] = np.sin(t[:, 0::2])
    t[:, 1::2] = np.cos(t[:, 1::2])
    return torch.from_numpy(t).float()


def rel_attention_probs(qkv, valid, emb_k, n_head, w):
    """The softmax of rel_attention, [B, H, L, L]: what mg_rel_attention_train_fwd saves.  Follows qkv's dtype."""
    B, C3, L = qkv.shape
    HD = C3 // 3
    d = HD // n_head
    q, k = [t.reshape(B, n_head, d, L).transpose(2, 3) for t in qkv.split(HD, 1)[:2]]
    scores = q @ k.transpose(-1, -2) / math.sqrt(d)
    i = torch.arange(L, device=qkv.device)
    rel = i[None, :] - i[:, None] + w
    rk = F.pad((q @ emb_k.t()) / math.sqrt(d), (0, 1))              # one more column of zeros: outside the band
    scores += rk.gather(3, torch.where((rel >= 0) & (rel <= 2 * w), rel, 2 * w + 1).expand(B, n_head, L, L))
    m = valid.bool()
    scores.masked_fill_(~(m[:, None, :, None] & m[:, None, None, :]), -1e4)
    return F.softmax(scores, -1)


def rel_attention_apply(p, qkv, emb_v, n_head, w, keep=None, scale=1.0):
    """P.V + sum over the band of P[i,j] E_v[j-i+w] with P = dropout(p) (BL:1059: keep [B, H, L, L] 1 = kept, times
    scale) -> [B, HD, L]."""
    B, C3, L = qkv.shape
    HD = C3 // 3
    v = qkv[:, 2 * HD:].reshape(B, n_head, HD // n_head, L).transpose(2, 3)
    if keep is not None:
        p = p * keep.to(p.dtype) * scale
    out = p @ v
    i = torch.arange(L, device=qkv.device)
    for m in range(2 * w + 1):                                       # diagonal j = i + m - w of P, times E_v[m]
        lo, hi = max(0, w - m), min(L, L + w - m)
        if lo < hi:
            out[:, :, lo:hi] += p[:, :, i[lo:hi], i[lo:hi] + m - w][..., None] * emb_v[m]
    return out.transpose(2, 3).reshape(B, HD, L)


def rel_attention(qkv, valid, emb_k, emb_v, n_head, w):
    """BL:1016-1061 on qkv [B, 3HD, L]: scores q.k/sqrt(d) + q.E_k[j-i+w]/sqrt(d) inside the band, -1e4 where
    valid[i]*valid[j] == 0, softmax over all keys, P.V + sum over the band of P[i,j] E_v[j-i+w]."""
    B, C3, L = qkv.shape
    HD = C3 // 3
    d = HD // n_head
    q, k, v = [t.reshape(B, n_head, d, L).transpose(2, 3) for t in qkv.split(HD, 1)]     # [B, H, L, d]
    scores = q @ k.transpose(-1, -2) / math.sqrt(d)
    i = torch.arange(L, device=qkv.device)
    rel = i[None, :] - i[:, None] + w                   # [L(i), L(j)]
    band = (rel >= 0) & (rel <= 2 * w)
    idx = rel.clamp(0, 2 * w)
    rk = (q @ emb_k.t()) / math.sqrt(d)                 # [B, H, L, 2w+1]
    scores = scores + torch.where(band, rk.gather(3, idx.expand(B, n_head, L, L)), torch.zeros((), device=qkv.device, dtype=rk.dtype))
    m = valid.float()
    scores = scores.masked_fill((m[:, None, :, None] * m[:, None, None, :]) == 0, -1e4)
    p = F.softmax(scores, -1)
    out = p @ v
    pb = torch.zeros(B, n_head, L, 2 * w + 1, device=qkv.device, dtype=p.dtype)
    pb.scatter_add_(3, idx.expand(B, n_head, L, L), p * band)
    out = out + pb @ emb_v
    return out.transpose(2, 3).reshape(B, HD, L)


def w2p_attention(q, kv, key_valid, query_valid, mapping, prior, n_head):
    """BL:741-768 on q [B, HD, Lq], kv [B, 2HD, Lk] -> (out [B, HD, Lq], attn, attn_raw [H, B, Lq, Lk],
    logprob [H, B, 1, Lq, Lk])."""
    B, HD, Lq = q.shape
    Lk = kv.shape[2]
    d = HD // n_head
    qh = q.reshape(B, n_head, d, Lq).permute(1, 0, 3, 2)            # [H, B, Lq, d]
    kh = kv[:, :HD].reshape(B, n_head, d, Lk).permute(1, 0, 3, 2)
    vh = kv[:, HD:].reshape(B, n_head, d, Lk).permute(1, 0, 3, 2)
    s = qh @ kh.transpose(-1, -2) / np.power(d, 0.5)
    s = s.masked_fill(~key_valid.bool()[None, :, None, :], -np.inf)
    if prior is not None:
        s = F.log_softmax(s, -1) + torch.log(prior.transpose(1, 2)[None] + 1e-8)
    logp = s.unsqueeze(2).clone()
    a = F.softmax(s, -1) * query_valid.bool()[None, :, :, None]
    raw = a.clone()
    a = a * mapping.bool()[None]
    out = a @ vh                                                     # [H, B, Lq, d]
    return out.permute(1, 0, 3, 2).reshape(B, HD, Lq), a, raw, logp


def _conv(x, sd, key, k, act=True):
    y = F.conv1d(x, sd[key + ".weight"], sd.get(key + ".bias"), padding=k // 2)
    return torch.relu(y) if act else y


def _ln_c(x, g, b, eps):
    """BL:258-276: LayerNorm over channels of [B, C, L]."""
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * g[None, :, None] + b[None, :, None]


def fft_block(sd, p, x, mask, n_layers, n_head, w, k):
    """BL:915-976 (RelativeFFTBlock with RelativeSelfAttention and a ReLU FFN), x [B, C, L], mask [B, L] bool."""
    m = mask.float()[:, None, :]
    for i in range(n_layers):
        a = "%sattn_layers.%d." % (p, i)
        x = x * m
        qkv = torch.cat([_conv(x, sd, a + c, 1, False) for c in ("conv_q", "conv_k", "conv_v")], 1)
        y = rel_attention(qkv, mask, sd[a + "emb_rel_k"][0], sd[a + "emb_rel_v"][0], n_head, w)
        y = _conv(y, sd, a + "conv_o", 1, False)
        x = _ln_c(x + y, sd["%snorm_layers_1.%d.gamma" % (p, i)], sd["%snorm_layers_1.%d.beta" % (p, i)], 1e-4)
        y = _conv(x * m, sd, "%sffn_layers.%d.conv" % (p, i), k) * m
        x = _ln_c(x + y, sd["%snorm_layers_2.%d.gamma" % (p, i)], sd["%snorm_layers_2.%d.beta" % (p, i)], 1e-4)
    return x * m


def variance_predictor(sd, p, x, mask):
    """LE:419-478 on x [B, C, L] -> [B, L]."""
    c = p + "conv_layer."
    h = _conv(x, sd, c + "conv1d_1.conv", 3)
    h = F.layer_norm(h.transpose(1, 2), (h.shape[1],), sd[c + "layer_norm_1.weight"], sd[c + "layer_norm_1.bias"])
    h = _conv(h.transpose(1, 2), sd, c + "conv1d_2.conv", 3)
    h = F.layer_norm(h.transpose(1, 2), (h.shape[1],), sd[c + "layer_norm_2.weight"], sd[c + "layer_norm_2.bias"])
    return F.linear(h, sd[p + "linear_layer.weight"], sd[p + "linear_layer.bias"]).squeeze(-1) * mask


# ---- the per-token glue kernels of csrc/lingenc.hip, one restatement each; every one follows its input's dtype
def embed_cm(ids, table, valid, skip_row=-1):
    """mg_embed_cm: [B, C, L] = table[ids] where valid and 0 <= id < n_rows, else zero rows (and, for the gradient of
    mg_embed_cm_bwd, nothing through row skip_row: nn.Embedding's padding_idx)."""
    n = table.shape[0]
    ok = valid.bool() & (ids >= 0) & (ids < n) & (ids != skip_row)
    rows = table[ids.clamp(0, n - 1)]
    return torch.where(ok[:, :, None], rows, torch.zeros((), dtype=table.dtype)).transpose(1, 2)


def variance_head(h, weight, bias, valid, control, target, bins):
    """mg_variance_head (LE:163-183, 473-478) on h [B, C, L] -> (pred [B, L], bucket [B, L]): pred = (w . h + b) * valid
    (* control without a target); bucket = torch.bucketize(target or pred, bins), right=False: the number of bins strictly
    below the value."""
    pred = (torch.einsum("c,bcl->bl", weight.reshape(-1), h) + bias) * valid.to(h.dtype)
    if target is None:
        pred = pred * control
    val = pred if target is None else target.to(h.dtype)
    return pred, (bins.to(h.dtype)[None, None, :] < val[:, :, None]).sum(-1)


def duration_head(logp, target, wb, src_w_len, d_control, W):
    """mg_duration_head (LE:294-316) -> (log_w [B, W], dur int64 [B, W]): log of the word sum of exp(logp) (-inf for
    words with no phoneme or past src_w_len); dur the word sum of the integer target, or
    long(clamp(round(exp(log_w) - 1) * d_control, min=0))."""
    logw = word_pool(logp.exp()[:, :, None], wb, src_w_len, W, False).log().squeeze(-1)
    if target is not None:
        return logw, word_pool(target.double()[:, :, None], wb, src_w_len, W, False).squeeze(-1).round().long()
    return logw, torch.clamp(torch.round(torch.exp(logw) - 1) * d_control, min=0).long()


def posenc_add(x, rowmajor, coef, table):
    """mg_posenc_add (LE:201-220) -> [B, C, L] = x + coef[:, :, None] * table[:L]; x [B, L, C] when rowmajor."""
    L = coef.shape[1]
    y = x if rowmajor else x.transpose(1, 2)
    return (y + coef[:, :, None] * table[:L]).transpose(1, 2)


def dropout_apply(x, keep, scale):
    return torch.where(keep.bool(), x * scale, torch.zeros((), dtype=x.dtype))


def word_index(wb, Tp):
    """[B, Tp] word of every phoneme (past the last word: len(words))."""
    ends = wb.long().cumsum(1)
    return torch.searchsorted(ends, torch.arange(Tp, device=wb.device).expand(wb.shape[0], Tp).contiguous(), right=True)


def word_pool(x, wb, src_w_len, W, mean):
    """UT:394-413 on x [B, Tp, C] -> [B, W, C]."""
    B, Tp, C = x.shape
    wi = word_index(wb, Tp)
    valid = wi < src_w_len[:, None]
    out = torch.zeros(B, W + 1, C, device=x.device, dtype=x.dtype)
    out.scatter_add_(1, torch.where(valid, wi, W).clamp(max=W)[:, :, None].expand(B, Tp, C), x)
    out = out[:, :W]
    if mean:
        cnt = wb[:, :W].to(x.dtype).clamp(min=1)[:, :, None]
        out = out / cnt
    return out


def expand_index(dur, L):
    """frame -> word index for durations [B, W] (past the end: W), and the cumulative ends."""
    ends = dur.clamp(min=0).cumsum(1)
    f = torch.arange(L, device=dur.device).expand(dur.shape[0], L).contiguous()
    return torch.searchsorted(ends, f, right=True), ends


def rel_coef(dur, n, mask):
    """LE:222-236: position inside the segment / segment length, 1 where mask is False as the divisor."""
    B, L = mask.shape
    dur = dur.long() * (torch.arange(dur.shape[1], device=dur.device)[None] < n[:, None])
    wi, ends = expand_index(dur, L)
    wic = wi.clamp(max=dur.shape[1] - 1)
    start = ends.gather(1, wic) - dur.gather(1, wic)
    pos = torch.arange(L, device=dur.device)[None] - start
    seg = dur.gather(1, wic)
    inside = wi < dur.shape[1]
    num = torch.where(inside, pos, 0).float()
    den = torch.where(mask.bool(), torch.where(inside, seg, 0).float(), 1.0)
    return num / den


def encoder_forward(sd, cfg, texts, src_lens, wb, src_mask, src_w_lens, src_w_mask, mel_mask=None, max_len=None,
                    attn_prior=None, pitch_target=None, energy_target=None, duration_target=None, p_control=1.0,
                    d_control=1.0):
    """LE:238-380 in eval mode -> the nine outputs plus (enc_p_out, enc_w_out)."""
    pre, mc, tr = cfg
    tc = mc["transformer"]
    H, w, k, nl = tc["encoder_head"], tc["encoder_window_size"], tc["conv_kernel_size"], tc["encoder_layer"]
    D = tc["encoder_hidden"]
    dev = texts.device
    B, Tp = src_mask.shape
    W = src_w_mask.shape[1]
    x = F.embedding(texts, sd["src_emb.weight"]).transpose(1, 2)
    enc = fft_block(sd, "phoneme_encoder.", x, src_mask, nl, H, w, k)
    pm = src_mask.float()

    def vemb(name, x, target, control):
        pred = variance_predictor(sd, name + "_predictor.", x, pm)
        if target is None:
            pred = pred * control
        val = pred if target is None else target
        e = F.embedding(torch.bucketize(val, sd[name + "_bins"]), sd[name + "_embedding.weight"])
        return pred, x + e.transpose(1, 2)
    pitch, enc = vemb("pitch", enc, pitch_target, p_control)
    energy, enc = vemb("energy", enc, energy_target, p_control)
    enc_p = enc.transpose(1, 2)
    wseq = word_pool(enc_p, wb, src_w_lens, W, True)
    enc_w = fft_block(sd, "word_encoder.", wseq.transpose(1, 2), src_w_mask, nl, H, w, k).transpose(1, 2)
    logd_p = variance_predictor(sd, "duration_predictor.", enc, pm)
    logd_w = word_pool(logd_p.exp()[:, :, None], wb, src_w_lens, W, False).log().squeeze(-1)
    if duration_target is not None:
        dur = word_pool(duration_target.double()[:, :, None], wb, src_w_lens, W, False).squeeze(-1).round().long()
    else:
        dur = torch.clamp(torch.round(torch.exp(logd_w) - 1) * d_control, min=0).long()
    mel_len = dur.clamp(min=0).sum(1)
    Lq = int(max_len) if max_len else int(mel_len.max())
    wi, _ = expand_index(dur, Lq)
    fr_ok = wi < W
    xr = enc_w.gather(1, wi.clamp(max=W - 1)[:, :, None].expand(B, Lq, D)) * fr_ok[:, :, None]
    if duration_target is None:
        mel_mask = torch.arange(Lq, device=dev)[None] < mel_len[:, None]
    # LE:185-199: frames of word i attend to phonemes of word i
    pwi = word_index(wb, Tp)
    mapping = (wi[:, :, None] == pwi[:, None, :]) & fr_ok[:, :, None] & (pwi < src_w_lens[:, None])[:, None, :]

    def table(name, L):
        return sinusoid(L, D).to(dev) if L > mc["max_seq_len"] else sd[name][0, :L]
    cq = rel_coef(dur, src_w_lens, mel_mask)
    ckv = rel_coef(wb, src_w_lens, src_mask)
    q = xr + cq[:, :, None] * table("q_position_enc", Lq)
    kvin = enc_p + ckv[:, :, None] * table("kv_position_enc", Tp)
    a = "w2p_attn."
    qp = F.linear(q, sd[a + "w_qs.linear.weight"]).transpose(1, 2)
    kvp = torch.cat([F.linear(kvin, sd[a + "w_ks.linear.weight"]), F.linear(kvin, sd[a + "w_vs.linear.weight"])],
                    2).transpose(1, 2)
    prior = attn_prior if tr["aligner"]["helper_type"] == "ctc" else None
    o, attn, raw, logp = w2p_attention(qp, kvp, src_mask, mel_mask, mapping, prior, H)
    out = F.linear(o.transpose(1, 2), sd[a + "fc.linear.weight"]) + q
    return (out, pitch, energy, logd_w, dur, mel_len, mel_mask, (attn, raw), logp), (enc_p, enc_w)
