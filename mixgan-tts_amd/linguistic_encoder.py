"""Native LinguisticEncoder for inference (model/linguistic_encoder.py:41-380, model/blocks.py:695-768,915-1123).

Same class names, constructor arguments, forward signature (14 arguments, nine outputs) and state_dict keys,
shapes and order as the reference, so a reference checkpoint loads with strict=True.  Eval-mode forward only:
training the encoder needs backward passes this module does not have, so a forward with grad enabled on
trainable parameters raises instead of returning outputs that silently lack gradients.

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

from . import ops, lingops, _lib
from ._lib import fptr, iptr, check, stream_ptr
from .blocks import ConvNorm, LinearNorm
from .transformer import get_sinusoid_encoding_table

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


def _packed(*weights):
    """k=1 weights [Co, Ci] stacked along Co, packed once per parameter version."""
    return torch.cat([ops.pack_cached(w[:, :, None] if w.dim() == 2 else w) for w in weights])


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

    def forward_cm(self, x, valid8):
        C = self.channels
        qkv = ops.conv1d_packed(x, _packed(self.conv_q.weight, self.conv_k.weight, self.conv_v.weight),
                                torch.cat([self.conv_q.bias, self.conv_k.bias, self.conv_v.bias]).detach(), 3 * C, 1)
        att = rel_attention(qkv, valid8, self.emb_rel_k.detach()[0], self.emb_rel_v.detach()[0], self.n_heads,
                            self.window_size)
        return ops.conv1d_packed(att, ops.pack_cached(self.conv_o.weight), self.conv_o.bias.detach(),
                                 self.conv_o.weight.shape[0], 1)


class FFN(nn.Module):
    """model/blocks.py:956-976: one Conv1d(k) + ReLU (the reference's default activation)."""

    def __init__(self, in_channels, out_channels, kernel_size, p_dropout=0., activation=None):
        super().__init__()
        if activation is not None:
            raise NotImplementedError("RelativeFFTBlock builds its FFN with the ReLU activation")
        self.kernel_size = kernel_size
        self.conv = _Conv1d(in_channels, out_channels, kernel_size)

    def forward_cm(self, x):
        k = self.kernel_size
        return ops.conv1d_packed(x, ops.pack_cached(self.conv.weight), self.conv.bias.detach(),
                                 self.conv.weight.shape[0], k, 1, k // 2, "relu")


class RelativeFFTBlock(nn.Module):
    """model/blocks.py:915-954."""

    def __init__(self, hidden_channels, filter_channels, n_heads, n_layers, kernel_size=1, p_dropout=0.,
                 window_size=None):
        super().__init__()
        self.n_layers = n_layers
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

    def forward_cm(self, x, valid8, pad8):
        """x [B, C, L] with zeros at the pads -> the block's output (zeros at the pads).

        The reference masks x at the top of every layer, the FFN's input and output, and the block's output.  Every
        LayerNorm here zeroes its padded frames instead: a frame's LayerNorm reads only that frame, the convolutions
        and the attention read the pads only through those masks, so the valid frames and the (zero) pads of the
        block's output are the reference's."""
        for i in range(self.n_layers):
            n1, n2 = self.norm_layers_1[i], self.norm_layers_2[i]
            y = self.attn_layers[i].forward_cm(x, valid8)
            x = ops.layernorm_cm(y, x, n1.gamma.detach(), n1.beta.detach(), pad8, n1.eps)
            y = self.ffn_layers[i].forward_cm(x)
            x = ops.layernorm_cm(y, x, n2.gamma.detach(), n2.beta.detach(), pad8, n2.eps)
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

    def hidden_cm(self, x):
        """The conv stack on x [B, C, L] (pads are read as they are, like the reference) -> [B, filter, L]."""
        c1, c2 = self.conv_layer.conv1d_1, self.conv_layer.conv1d_2
        n1, n2 = self.conv_layer.layer_norm_1, self.conv_layer.layer_norm_2
        F = self.filter_size
        h = ops.conv1d_packed(x, ops.pack_cached(c1.conv.weight), c1.conv.bias.detach(), F, self.kernel, 1,
                              (self.kernel - 1) // 2, "relu")
        h = ops.layernorm_cm(h, None, n1.weight.detach(), n1.bias.detach(), None, n1.eps)
        h = ops.conv1d_packed(h, ops.pack_cached(c2.conv.weight), c2.conv.bias.detach(), F, self.kernel, 1, 1, "relu")
        return ops.layernorm_cm(h, None, n2.weight.detach(), n2.bias.detach(), None, n2.eps)

    def head(self, h, valid8, control=1.0, target=None, bins=None, emb=None, x=None):
        return variance_head(h, self.linear_layer.weight.detach(), self.linear_layer.bias.detach(), valid8, control,
                             target, bins, emb, x)


class WordToPhonemeAttention(nn.Module):
    """model/blocks.py:673-739 (bias-free LinearNorm projections and fc)."""

    def __init__(self, n_head, d_model, d_k, d_v, dropout=0.0):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.w_qs = LinearNorm(d_model, n_head * d_k)
        self.w_ks = LinearNorm(d_model, n_head * d_k)
        self.w_vs = LinearNorm(d_model, n_head * d_v)
        self.fc = LinearNorm(n_head * d_v, d_model)

    def forward_cm(self, q_in, kv_in, key_valid8, query_valid8, mapping8, attn_prior=None):
        """q_in [B, D, Lq], kv_in [B, D, Lk] (k and v are the same tensor in the encoder) ->
        (fc(attention) + q_in [B, D, Lq], (attn, attn_raw) [H, B, Lq, Lk], attn_logprob [H, B, 1, Lq, Lk])."""
        HD = self.n_head * self.d_k
        D = self.fc.linear.weight.shape[0]
        q = ops.conv1d_packed(q_in, _packed(self.w_qs.linear.weight), None, HD, 1)
        kv = ops.conv1d_packed(kv_in, _packed(self.w_ks.linear.weight, self.w_vs.linear.weight), None, 2 * HD, 1)
        prior = None if attn_prior is None else attn_prior.to(torch.float32).contiguous()
        out, attn, raw, logp = w2p_attention(q, kv, key_valid8, query_valid8, mapping8, prior, self.n_head)
        y = ops.conv1d_packed(out, _packed(self.fc.linear.weight), None, D, 1, add=q_in)
        return y, (attn, raw), logp


class LinguisticEncoder(nn.Module):
    """model/linguistic_encoder.py:41-380, inference."""

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

    def forward(self, src_p_seq, src_p_len, word_boundary, src_p_mask, src_w_len, src_w_mask, mel_mask=None,
                max_len=None, attn_prior=None, pitch_target=None, energy_target=None, duration_target=None,
                p_control=1.0, duration_control=1.0):
        if self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(
                "the native LinguisticEncoder is inference-only (eval() under torch.no_grad(), or parameters with "
                "requires_grad=False): for training, inject the reference's model.linguistic_encoder.LinguisticEncoder")
        if not src_p_seq.is_cuda:
            raise _lib.MixganHipError("LinguisticEncoder on %s: the HIP path has no CPU fallback" % src_p_seq.device)
        dev = src_p_seq.device
        B, Tp = src_p_mask.shape
        W = src_w_mask.shape[1]
        pv8, pp8 = _u8(src_p_mask), _u8(~src_p_mask.bool())
        wv8, wp8 = _u8(src_w_mask), _u8(~src_w_mask.bool())
        wb = word_boundary.to(torch.int64).contiguous()
        src_w_len = src_w_len.to(torch.int64).contiguous()

        # phoneme encoder (:318-320), pitch / energy embeddings added at every phoneme, pads included (:322-333)
        x = embed_cm(src_p_seq[:, :Tp], self.src_emb.weight.detach(), pv8)
        enc_p = self.phoneme_encoder.forward_cm(x, pv8, pp8)
        pitch_prediction = self.pitch_predictor.head(
            self.pitch_predictor.hidden_cm(enc_p), pv8, p_control, pitch_target, self.pitch_bins.detach(),
            self.pitch_embedding.weight.detach(), enc_p)
        energy_prediction = self.energy_predictor.head(
            self.energy_predictor.hidden_cm(enc_p), pv8, p_control, energy_target, self.energy_bins.detach(),
            self.energy_embedding.weight.detach(), enc_p)

        # word pooling -> word encoder (:347-353)
        enc_p_rm = ops.transpose_bml(enc_p, True)
        src_w_seq = lingops.word_level_pooling(enc_p_rm, src_p_len, wb, src_w_len, "mean", max_words=W)
        enc_w = self.word_encoder.forward_cm(ops.transpose_bml(src_w_seq, False, keep=wv8), wv8, wp8)
        enc_w_rm = ops.transpose_bml(enc_w, True)
        if self.record:
            self.recorded = {"enc_p_out": enc_p_rm, "enc_w_out": enc_w_rm}

        # durations (:355-376)
        log_d_p = self.duration_predictor.head(self.duration_predictor.hidden_cm(enc_p), pv8)
        log_duration_w_prediction, duration_w_rounded = duration_head(
            log_d_p, duration_target, wb, src_w_len, duration_control, W)
        xr, mel_len = self.length_regulator(enc_w_rm, duration_w_rounded, max_len)
        if duration_target is None:
            ids = torch.arange(xr.shape[1], device=dev)
            mel_mask = ids[None, :] < mel_len[:, None]
        Lq = xr.shape[1]

        # word-to-phoneme attention (:378-407); k and v share one input, and their rel coefficients are one tensor
        mapping = lingops.get_mapping_mask(xr, enc_p_rm, duration_w_rounded, wb, src_w_len)
        coef_q = lingops.get_rel_coef(duration_w_rounded, src_w_len, mel_mask)
        coef_kv = lingops.get_rel_coef(wb, src_p_len, src_p_mask)
        q_in = posenc_add(xr, True, coef_q, self._table(self.q_position_enc, Lq, dev))
        kv_in = posenc_add(enc_p, False, coef_kv, self._table(self.kv_position_enc, Tp, dev))
        y, attns, attn_logprob = self.w2p_attn.forward_cm(
            q_in, kv_in, pv8, _u8(mel_mask), _u8(mapping),
            attn_prior if self.helper_type == "ctc" else None)
        out = ops.transpose_bml(y, True)
        return (out, pitch_prediction, energy_prediction, log_duration_w_prediction, duration_w_rounded, mel_len,
                mel_mask, attns, attn_logprob)
