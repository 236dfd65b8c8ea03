"""torch.autograd.Function wrappers: forward and backward both run in the HIP library."""
import torch

from . import ops, _lib


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.MixganHipError("tensor on %s: the HIP path has no CPU fallback" % t.device)


class _TransposeFn(torch.autograd.Function):
    """[B,L,C] <-> [B,C,L] through mg_transpose_bml; the gradient is the opposite transpose."""

    @staticmethod
    def forward(ctx, x, to_blm):
        ctx.to_blm = to_blm
        return ops.transpose_bml(x.contiguous(), to_blm)

    @staticmethod
    def backward(ctx, g):
        return ops.transpose_bml(g.contiguous(), not ctx.to_blm), None


def transpose_to_bml(x):
    _require_cuda(x)
    return _TransposeFn.apply(x, False)


def transpose_to_blm(x):
    _require_cuda(x)
    return _TransposeFn.apply(x, True)


class _SpecAffineFn(torch.autograd.Function):
    """norm_spec / denorm_spec (model/diffusion.py:228-232) on [..., M] tensors."""

    @staticmethod
    def forward(ctx, x, spec_min, spec_max, norm):
        ctx.save_for_backward(spec_min, spec_max)
        ctx.norm = norm
        return ops.spec_affine(x.contiguous(), spec_min, spec_max, 1 if norm else 2)

    @staticmethod
    def backward(ctx, g):
        spec_min, spec_max = ctx.saved_tensors
        return ops.spec_affine(g.contiguous(), spec_min, spec_max, 3 if ctx.norm else 4), None, None, None


def spec_affine(x, spec_min, spec_max, norm):
    _require_cuda(x)
    return _SpecAffineFn.apply(x, spec_min, spec_max, norm)


class DenoiserFn(torch.autograd.Function):
    """Denoiser.forward with the layer activations saved in a workspace that this node keeps alive (a later forward
    of the module at any shape, or a cache eviction, cannot take it away); backward = mg_denoiser_bwd."""

    @staticmethod
    def forward(ctx, module, x, t, cond, spk, pre, *params):
        """pre: None, or (out, ws) of a forward that already ran on exactly these inputs (Denoiser.run_pair): the node
        then only adopts its output and saved activations."""
        _require_cuda(x, cond)
        if pre is None:
            out = module.run(x, t, cond, spk, save=True)
            ctx.ws = module.last_ws
        else:
            out, ctx.ws = pre
        ctx.module = module
        ctx.gen = ctx.ws._mg_gen
        ctx.save_for_backward(x, t, cond, spk if spk is not None else x.new_empty(0))
        ctx.has_spk = spk is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, t, cond, spk = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_x, d_cond, d_spk, pg = ctx.module.run_backward(g.contiguous(), x, t, cond, spk if ctx.has_spk else None,
                                                         ctx.ws, ctx.gen, need[1], need[3], need[4])
        return (None, d_x, None, d_cond, d_spk, None) + tuple(pg)


def denoise_and_posterior(diff, x_t, t, cond_t, spk, post_noise, keep, clip, coarse_mel, pre=None):
    """Training branch of GaussianDiffusion.forward with autograd (model/diffusion.py:210-220)."""
    den = diff.denoise_fn
    x0 = DenoiserFn.apply(den, x_t, t, cond_t, spk, pre, *[p for p in den._weight_table() if p is not None])
    buf = diff._buf()
    if coarse_mel is None:
        x0c, xpp = _PosteriorFn.apply(x0, x_t, t, post_noise, keep, buf["posterior_mean_coef1"],
                                      buf["posterior_mean_coef2"], buf["posterior_log_variance_clipped"], clip, True)
        return x0c, xpp
    # shallow: x_{t-1} is sampled around the detached coarse mel; only x0c carries gradient
    start = ops.transpose_bml(coarse_mel.detach().contiguous(), False, 1, diff.spec_min, diff.spec_max)
    xpp = ops.posterior_sample(start, x_t, t, post_noise, keep, buf, clip=False)
    x0c, _ = _PosteriorFn.apply(x0, x_t, t, post_noise, keep, buf["posterior_mean_coef1"],
                                buf["posterior_mean_coef2"], buf["posterior_log_variance_clipped"], clip, False)
    return x0c, xpp


class _PosteriorFn(torch.autograd.Function):
    """(x0c, x_{t-1}) = mg_posterior_sample_fwd(x0, ...); d/dx0 only (everything else is data)."""

    @staticmethod
    def forward(ctx, x0, x_t, t, noise, keep, c1, c2, lv, clip, through_posterior):
        buf = {"posterior_mean_coef1": c1, "posterior_mean_coef2": c2, "posterior_log_variance_clipped": lv}
        xpp, x0c = ops.posterior_sample(x0.contiguous(), x_t, t, noise, keep, buf, clip=clip, want_x0c=True)
        ctx.save_for_backward(x0, t, keep, c1)
        ctx.clip = clip
        ctx.through = through_posterior
        ctx.mark_non_differentiable(xpp) if not through_posterior else None
        return x0c, xpp

    @staticmethod
    def backward(ctx, g_x0c, g_xpp):
        x0, t, keep, c1 = ctx.saved_tensors
        g = ops.posterior_sample_bwd(x0, t, keep, c1, g_x0c.contiguous(),
                                     g_xpp.contiguous() if ctx.through else None, ctx.clip)
        return (g,) + (None,) * 9


# --------------------------------------------------------------------------------------------------
# differentiable building blocks for the JCU discriminator and the FFT blocks: every forward and
# backward below is a call into the HIP library; torch.autograd only chains them.
# --------------------------------------------------------------------------------------------------
def _pack(w, mode=ops.PACK_PLAIN):
    """MFMA pack of a convolution weight.  A module parameter (or a view of one) keeps its pack in ops.pack_cached,
    refreshed in place so that a captured graph goes on reading the same address; anything else -- an effective weight,
    or several weights stacked by torch.cat (the attention's q/k/v, the linguistic encoder's stacked convolutions), is a
    fresh tensor every step -- is packed here and the pack dies with its use."""
    owner = w._base if w._base is not None else w
    return ops.pack_cached(w, mode) if isinstance(owner, torch.nn.Parameter) else ops.pack_conv_weight(w, mode)


class _Conv1dFn(torch.autograd.Function):
    """y = act(conv1d(x (+ in_vec), W, b)); x [B,Ci,L] channel-major.  act "lrelu_s" is leaky ReLU with the runtime
    slope act_slope, differentiated through the activated y (slope > 0 keeps the sign)."""

    @staticmethod
    def forward(ctx, x, weight, bias, in_vec, stride, padding, act, act_slope):
        _require_cuda(x)
        x = x.contiguous()
        Co, Ci, K = weight.shape
        y = ops.conv1d_packed(x, _pack(weight), None if bias is None else bias.detach(), Co, K, stride, padding, act,
                              in_vec=None if in_vec is None else in_vec.detach().contiguous(), act_slope=act_slope,
                              split=True)
        ctx.save_for_backward(x, weight, y if act else None, in_vec)
        ctx.cfg = (stride, padding, act, act_slope, bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y, in_vec = ctx.saved_tensors
        stride, padding, act, act_slope, has_bias = ctx.cfg
        Co, Ci, K = weight.shape
        gy = gy.contiguous()
        dpre = gy
        if act:
            dpre = ops.lrelu_bwd(gy, y, act_slope) if act == "lrelu_s" else ops.act_bwd(gy, y, act)
        need = ctx.needs_input_grad
        vec = None if in_vec is None else in_vec.detach().contiguous()
        dw = ops.conv1d_wgrad(dpre, x, K, stride, padding, x_vec=vec) if need[1] else None
        db = ops.rowsum(dpre) if (has_bias and need[2]) else None
        dx = dvec = None
        if need[0] or (in_vec is not None and need[3]):
            Lin = x.shape[2]
            src = dpre
            if stride > 1:
                src = ops.upsample_zero(dpre, stride, (dpre.shape[2] - 1) * stride + 1)
            dx = ops.conv1d_packed(src, _pack(weight, ops.PACK_DGRAD), None, Ci, K, 1, K - 1 - padding, Lout=Lin,
                                   split=True)
            if in_vec is not None and need[3]:
                dvec = ops.rowsum(dx, per_batch=True)
        return dx if need[0] else None, dw, db, dvec, None, None, None, None


def conv1d(x, weight, bias=None, stride=1, padding=0, act=None, in_vec=None, act_slope=0.0):
    return _Conv1dFn.apply(x, weight, bias, in_vec, stride, padding, act, act_slope)


class _StepMlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, freq, W0, W2):
        out, emb, pre, h = ops.step_mlp_fwd(t.contiguous(), freq, W0.detach().contiguous(), W2.detach().contiguous())
        ctx.save_for_backward(emb, pre, h, W2)
        return out

    @staticmethod
    def backward(ctx, g):
        emb, pre, h, W2 = ctx.saved_tensors
        dW0, dW2 = ops.step_mlp_bwd(g.contiguous(), emb, pre, h, W2.detach().contiguous())
        return None, None, dW0, dW2


def step_mlp(t, freq, W0, W2):
    _require_cuda(W0)
    return _StepMlpFn.apply(t, freq, W0, W2)


class _LinearSmallFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W):
        ctx.save_for_backward(x, W)
        return ops.linear_small_fwd(x.contiguous(), W.detach().contiguous())

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        dx, dW = ops.linear_small_bwd(g.contiguous(), x.contiguous(), W.detach().contiguous(), ctx.needs_input_grad[0])
        return dx, dW


def linear_small(x, W):
    _require_cuda(x)
    return _LinearSmallFn.apply(x, W)


class _CatTransposeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.M = a.shape[-1]
        return ops.cat_transpose(a.contiguous(), b.contiguous())

    @staticmethod
    def backward(ctx, g):
        da, db = ops.split_transpose(g.contiguous(), ctx.M)
        return da, db


def cat_transpose(a, b):
    _require_cuda(a, b)
    return _CatTransposeFn.apply(a, b)


class _ResBlockFn(torch.autograd.Function):
    """One gated residual block (model/blocks.py:1157-1176) stand-alone: forward = the fused layer kernel the Denoiser
    launches per layer (mg_resblock_fwd), backward = the same data-gradient / weight-gradient GEMMs mg_denoiser_bwd
    uses, one layer's worth.  hvec = Wd s (+ Wp spk) and dvec = Wd s are inputs (their Linear layers are separate
    autograd nodes)."""

    @staticmethod
    def forward(ctx, x, cond, hvec, dvec, Wc, bc, W3, b3, Wo, bo):
        _require_cuda(x, cond)
        x, cond = x.contiguous(), cond.contiguous()
        save = any(ctx.needs_input_grad)
        x_out, skip, saves = ops.resblock_fwd(
            x, cond, ops.pack_cached(Wc), ops.pack_cached(W3, ops.PACK_GATE), ops.pack_cached(Wo), bc.detach(),
            b3.detach(), bo.detach(), hvec.detach().contiguous(), dvec.detach().contiguous(), save)
        if save:
            ctx.save_for_backward(cond, Wc, W3, Wo, *saves)
        return x_out, skip

    @staticmethod
    def backward(ctx, g_x, g_skip):
        cond, Wc, W3, Wo, h, g, sig, tnh = ctx.saved_tensors
        C, H = Wc.shape[0], Wc.shape[1]
        rs2 = 0.70710678118654752440
        g_xs = (g_x * rs2).contiguous()                     # d/d(x + Wd s) through the residual
        dout = torch.cat([g_xs, g_skip.contiguous()], 1)   # gradient of o = Wo g + bo, [B, 2C, L]
        dg = ops.conv1d_packed(dout, ops.pack_cached(Wo, ops.PACK_DGRAD), None, C, 1)
        dz = ops.gate_bwd(dg, sig, tnh)
        dh = ops.conv1d_packed(dz, ops.pack_cached(W3, ops.PACK_DGRAD), None, C, 3, 1, 1)
        need = ctx.needs_input_grad
        dx = ops.conv1d_packed(dz, ops.pack_cached(W3, ops.PACK_DGRAD), None, C, 3, 1, 1, add=g_xs) if need[0] else None
        dcond = ops.conv1d_packed(dh, ops.pack_cached(Wc, ops.PACK_DGRAD), None, H, 1) if need[1] else None
        return (dx, dcond,
                ops.rowsum(dh, per_batch=True) if need[2] else None,
                ops.rowsum(g_xs, per_batch=True) if need[3] else None,
                ops.conv1d_wgrad(dh, cond, 1) if need[4] else None, ops.rowsum(dh) if need[5] else None,
                ops.conv1d_wgrad(dz, h, 3, 1, 1) if need[6] else None, ops.rowsum(dz) if need[7] else None,
                ops.conv1d_wgrad(dout, g, 1) if need[8] else None, ops.rowsum(dout) if need[9] else None)


def residual_block(x, cond, hvec, dvec, Wc, bc, W3, b3, Wo, bo):
    return _ResBlockFn.apply(x, cond, hvec, dvec, Wc, bc, W3, b3, Wo, bo)


class _MishFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_cuda(x)
        x = x.contiguous()
        ctx.save_for_backward(x)
        return ops.mish_fwd(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.mish_bwd(g.contiguous(), x)


def mish(x):
    return _MishFn.apply(x)


# --------------------------------------------------------------------------------------------------
# aux pre-training: train-mode FFT-block / PostNet pieces with their backward
# --------------------------------------------------------------------------------------------------
class _AttentionTrainFn(torch.autograd.Function):
    """softmax(QK^T / sqrt(d) | key mask) V on channel-major qkv [B, 3HD, L], probabilities kept for the backward."""

    @staticmethod
    def forward(ctx, qkv, key_pad, n_head, d):
        _require_cuda(qkv)
        qkv = qkv.contiguous()
        out, P = ops.attention_train_fwd(qkv, key_pad, n_head, d)
        ctx.save_for_backward(qkv, P)
        ctx.cfg = (n_head, d)
        return out

    @staticmethod
    def backward(ctx, g):
        qkv, P = ctx.saved_tensors
        return ops.attention_train_bwd(qkv, P, g.contiguous(), *ctx.cfg), None, None, None


def attention_train(qkv, key_pad, n_head, d):
    return _AttentionTrainFn.apply(qkv, key_pad, n_head, d)


class _LayerNormTrainFn(torch.autograd.Function):
    """out = pad ? 0 : LayerNorm_c(dropout(a) + res) on [B, C, L]; keep: uint8 keep-mask or None."""

    @staticmethod
    def forward(ctx, a, res, gamma, beta, pad, keep, drop_scale, eps):
        _require_cuda(a, res)
        out, pre = ops.layernorm_cm_train(a.contiguous(), keep, drop_scale, res.contiguous(), gamma.detach(),
                                          beta.detach(), pad, eps)
        ctx.save_for_backward(pre, gamma, pad if pad is not None else pre.new_empty(0, dtype=torch.uint8),
                              keep if keep is not None else pre.new_empty(0, dtype=torch.uint8))
        ctx.cfg = (pad is not None, keep is not None, drop_scale, eps)
        return out

    @staticmethod
    def backward(ctx, g):
        pre, gamma, pad, keep = ctx.saved_tensors
        has_pad, has_keep, scale, eps = ctx.cfg
        d_pre, d_a, dg, db = ops.layernorm_cm_bwd(pre, g.contiguous(), gamma.detach(), pad if has_pad else None,
                                                  keep if has_keep else None, scale, eps)
        return d_a, d_pre, dg, db, None, None, None, None


def layernorm_train(a, res, gamma, beta, pad, keep, drop_scale, eps):
    return _LayerNormTrainFn.apply(a, res, gamma, beta, pad, keep, drop_scale, eps)


class _BatchNormActFn(torch.autograd.Function):
    """dropout(act(BatchNorm1d(x))) with batch statistics on [B, C, L].  Returns (out, mean, biased var); with a
    process group the statistics -- and in the backward the two per-channel sums -- are all-reduced (SyncBN)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, keep, drop_scale, act, eps, group):
        _require_cuda(x)
        x = x.contiguous()
        mean, var = ops.bn_stats(x)
        count = x.shape[0] * x.shape[2]
        if group is not None:
            import torch.distributed as dist
            world = dist.get_world_size(group)
            packed = torch.stack([mean, var + mean * mean])          # E[x], E[x^2]; equal counts per rank
            dist.all_reduce(packed, group=group)
            mean = packed[0] / world
            var = (packed[1] / world - mean * mean).clamp_min_(0.0)
            count *= world
        invstd = torch.rsqrt(var + eps)
        out, y = ops.bn_act_fwd(x, mean, invstd, gamma.detach(), beta.detach(), keep, drop_scale, act)
        ctx.save_for_backward(x, mean, invstd, gamma, y if y is not None else x.new_empty(0),
                              keep if keep is not None else x.new_empty(0, dtype=torch.uint8))
        ctx.cfg = (keep is not None, drop_scale, act, count, group)
        ctx.mark_non_differentiable(mean, var)
        return out, mean, var

    @staticmethod
    def backward(ctx, g, _gm, _gv):
        x, mean, invstd, gamma, y, keep = ctx.saved_tensors
        has_keep, scale, act, count, group = ctx.cfg
        g = g.contiguous()
        keep = keep if has_keep else None
        y = y if act == "tanh" else None
        dg, db = ops.bn_act_bwd_reduce(g, keep, scale, y, x, mean, invstd, act)
        dg_all, db_all = dg, db
        if group is not None:
            import torch.distributed as dist
            packed = torch.stack([dg, db])
            dist.all_reduce(packed, group=group)
            dg_all, db_all = packed[0], packed[1]
        dx = ops.bn_act_bwd_apply(g, keep, scale, y, x, mean, invstd, gamma.detach(), dg_all, db_all, 1.0 / count, act)
        return dx, dg, db, None, None, None, None, None


def batchnorm_act(x, gamma, beta, keep, drop_scale, act, eps, group=None):
    return _BatchNormActFn.apply(x, gamma, beta, keep, drop_scale, act, eps, group)


# --------------------------------------------------------------------------------------------------
# Differentiable log-mel (audio.TacotronSTFT.mel_spectrogram_diff) and the HiFi-GAN generator's training ops
# (vocoder.Generator.forward_train).  The HIP side differentiates with respect to the EFFECTIVE weight; weight norm is
# a torch expression in front of these functions.
# --------------------------------------------------------------------------------------------------
def weight_norm(v, g):
    """The effective weight of torch.nn.utils.weight_norm(dim=0): g v / |v| per output row."""
    return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))


class _MelDiffFn(torch.autograd.Function):
    """log-mel of x [B, N] (mg_stft_mel); the gradient recomputes each frame's spectrum (mg_stft_mel_bwd)."""

    @staticmethod
    def forward(ctx, x, stft):
        _require_cuda(x)
        B, L = x.shape
        hop, win, tw, band, band_w = stft._mel_args(x)
        T = 1 + L // hop
        mel = torch.empty(B, stft.n_mel_channels, T, device=x.device, dtype=torch.float32)
        energy = torch.empty(B, T, device=x.device, dtype=torch.float32)
        _lib.check(_lib.lib().mg_stft_mel(_lib.fptr(x), L, None, B, L, hop, _lib.fptr(win), _lib.fptr(tw),
                                          _lib.iptr(band, torch.int32), _lib.fptr(band_w), stft.n_mel_channels,
                                          _lib.fptr(mel), _lib.fptr(energy), T, _lib.stream_ptr()))
        ctx.save_for_backward(x)
        ctx.stft = stft
        return mel

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        stft = ctx.stft
        B, L = x.shape
        hop, win, tw, band, band_w = stft._mel_args(x)
        T = g.shape[2]
        g = g.contiguous()
        L_ = _lib.lib()
        nbytes = L_.mg_stft_mel_bwd_workspace_bytes(B, T)
        ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x)
        _lib.check(L_.mg_stft_mel_bwd(_lib.fptr(x), L, None, B, L, hop, _lib.fptr(win), _lib.fptr(tw),
                                      _lib.iptr(band, torch.int32), _lib.fptr(band_w), stft.n_mel_channels, _lib.fptr(g),
                                      T, _lib.fptr(dx), L, _lib.fptr(ws), nbytes, _lib.stream_ptr()))
        return dx, None


def mel_diff(x, stft):
    return _MelDiffFn.apply(x, stft)


REFLECT = "reflect"   # voc_conv's `pad`: ReflectionPad1d(dil (K - 1) / 2) in front of the convolution (MelGAN)


def _voc_conv_bwd(g, x, w, dil, pad, in_slope, alpha, need=(True, True, True), add=None, x_bs=0, add_bs=0, C=None):
    """(dw, db, dx), each where `need` asks for it, of alpha * conv1d(leaky_relu(x, in_slope), w [Co,Ci,K], dilation dil,
    padding pad) + b, from the output's gradient g and the saved pre-activation x.  The data gradient is the forward
    kernel on the transposed, tap-flipped pack with pad' = dil (K-1) - pad, then masked in place; `add` (a residual
    branch's gradient) joins in the mask's pass.  pad = REFLECT: the reflect-padded kernels (csrc/melgan_train.hip), which
    also take x / add as channels [0, C) of buffers with batch strides x_bs / add_bs."""
    Ci, K = w.shape[1], w.shape[2]
    dw = dx = None
    if need[0] and pad == REFLECT:
        dw = ops.conv1d_reflect_wgrad(g, x, K, dil, in_slope, alpha, x_bs=x_bs, C=C)
    elif need[0]:
        dw = ops.conv1d_wgrad_ex(g, x, K, dil, pad, in_slope, alpha)
    db = ops.rowsum(g) if need[1] else None
    if need[2] and pad == REFLECT:
        dx = ops.conv1d_reflect_dgrad(g, w, x, dil, in_slope, alpha, add=add, x_bs=x_bs, add_bs=add_bs, C=C)
    elif need[2]:
        dx = ops.conv1d_packed(g, ops.pack_conv_weight(w, ops.PACK_DGRAD), None, Ci, K, 1, dil * (K - 1) - pad,
                               alpha=alpha, Lout=x.shape[2], dilation=dil)
        if in_slope != 1.0 or add is not None:
            ops.lrelu_bwd(dx, x, in_slope, add=add, out=dx)
    return dw, db, dx


class _VocConvFn(torch.autograd.Function):
    """y = act(alpha * conv1d(leaky_relu(x, in_slope), w, dilation, padding) + b), act None or "tanh" (conv_pre and
    conv_post; with pad = REFLECT, MelGAN's first conv -- in_slope 1, alpha the mel scale -- and its last).  Saves x, w
    (and y for tanh)."""

    @staticmethod
    def forward(ctx, x, w, b, dil, pad, in_slope, alpha, act):
        Co, Ci, K = w.shape
        packed = ops.pack_conv_weight(w, ops.PACK_PLAIN)
        if pad == REFLECT:
            y = ops.conv1d_reflect_packed(x, packed, b, Co, K, dil, in_slope, act, 0.0, alpha)
        else:
            y = ops.conv1d_packed(x, packed, b, Co, K, 1, pad, act=act, alpha=alpha, dilation=dil, in_slope=in_slope)
        ctx.save_for_backward(x, w, y if act else None)
        ctx.cfg = (dil, pad, in_slope, alpha, act)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, y = ctx.saved_tensors
        dil, pad, in_slope, alpha, act = ctx.cfg
        g = g.contiguous()
        if act:
            g = ops.act_bwd(g, y, act)
        need = ctx.needs_input_grad
        dw, db, dx = _voc_conv_bwd(g, x, w, dil, pad, in_slope, alpha, (need[1], need[2], need[0]))
        return dx, dw, db, None, None, None, None, None


class _VocPairFn(torch.autograd.Function):
    """One (convs1[m], convs2[m]) pair of a ResBlock: t = conv1(lrelu(r)) + b1 (dilation dil, padding pad1),
    out = conv2(lrelu(t)) + b2 + r (padding pad2).  Saves the two PRE-activations r and t; both leaky ReLUs are applied
    while the kernels stage their input."""

    @staticmethod
    def forward(ctx, r, w1, b1, w2, b2, dil, pad1, pad2, slope):
        C, _, K = w1.shape
        t = ops.conv1d_packed(r, ops.pack_conv_weight(w1, ops.PACK_PLAIN), b1, C, K, 1, pad1, dilation=dil,
                              in_slope=slope)
        out = ops.conv1d_packed(t, ops.pack_conv_weight(w2, ops.PACK_PLAIN), b2, C, K, 1, pad2, add=r, in_slope=slope)
        ctx.save_for_backward(r, t, w1, w2)
        ctx.cfg = (dil, pad1, pad2, slope)
        ctx.mark_non_differentiable(t)
        return out, t

    @staticmethod
    def backward(ctx, g, _gt):
        r, t, w1, w2 = ctx.saved_tensors
        dil, pad1, pad2, slope = ctx.cfg
        g = g.contiguous()
        dw2, db2, dt = _voc_conv_bwd(g, t, w2, 1, pad2, slope, 1.0)
        dw1, db1, dr = _voc_conv_bwd(dt, r, w1, dil, pad1, slope, 1.0, add=g)    # + the residual branch's gradient
        return dr, dw1, db1, dw2, db2, None, None, None, None


class _VocUpFn(torch.autograd.Function):
    """y = alpha * conv_transpose1d(leaky_relu(x, slope), w [Ci,Co,2u], stride u, padding u/2) + b, polyphase."""

    @staticmethod
    def forward(ctx, x, w, b, u, slope, alpha):
        Co = w.shape[1]
        y = ops.conv_transpose1d_packed(x, ops.pack_conv_transpose_weight(w), b, Co, u, in_slope=slope, alpha=alpha)
        ctx.save_for_backward(x, w)
        ctx.cfg = (u, slope, alpha)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        u, slope, alpha = ctx.cfg
        g = g.contiguous()
        dw = ops.conv_transpose1d_wgrad(g, x, w.shape[1], u, slope, alpha)
        db = ops.rowsum(g)
        dx = ops.conv_transpose1d_dgrad(g, w, x, slope, alpha)
        return dx, dw, db, None, None, None


def voc_conv(x, w, b, dil, pad, in_slope=1.0, alpha=1.0, act=None):
    """pad: zero padding per side, or REFLECT."""
    _require_cuda(x, w, b)
    return _VocConvFn.apply(x.contiguous(), w.contiguous(), b, dil, pad, in_slope, alpha, act)


def voc_pair(r, w1, b1, w2, b2, dil, pad1, pad2, slope):
    return _VocPairFn.apply(r, w1.contiguous(), b1, w2.contiguous(), b2, dil, pad1, pad2, slope)


def voc_up(x, w, b, u, slope, alpha):
    return _VocUpFn.apply(x, w.contiguous(), b, u, slope, alpha)


# --------------------------------------------------------------------------------------------------
# MelGAN generator (melgan.MelGANGenerator._walk; csrc/melgan_train.hip).  Effective weights, as above.
# --------------------------------------------------------------------------------------------------
def melgan_block_fwd(buf, pack1, b1, mix, C, dil, slope, out=None, out_bs=0):
    """General-form MelGAN ResnetBlock(C, dil) on buf [B, 2C, L], x in channels [0, C): t = lrelu(conv3(reflection_pad(
    lrelu(x)), dil) + b1) -> channels [C, 2C), then y = [Ws | W2] [x ; t] + bs + b2, one K = 1 GEMM; mix() gives that pack
    and bias, after the conv as both callers always did.  out None: a new y (training); else into `out`, batch stride
    out_bs (inference).  Two entry points on purpose: only mg_conv1x1_fwd_strided writes a strided output, and its case
    list is not mg_conv1d_fwd_split's, so moving either side could change its bits."""
    L = buf.shape[2]
    ops.conv1d_reflect_packed(buf, pack1, b1, C, 3, dil, slope, "lrelu_s", slope, x_bs=2 * C * L, C=C, out=buf,
                              out_bs=2 * C * L, out_off=C * L)
    pack_mix, b_mix = mix()
    if out is None:
        return ops.conv1d_packed(buf, pack_mix, b_mix, C, 1)
    _lib.check(_lib.lib().mg_conv1x1_fwd_strided(_lib.fptr(buf), 2 * C * L, _lib.fptr(pack_mix), _lib.fptr(b_mix),
                                                 _lib.fptr(out), out_bs, buf.shape[0], 2 * C, L, C, _lib.stream_ptr()))
    return out


class _MelResBlockFn(torch.autograd.Function):
    """melgan_block_fwd on a fresh [B, 2C, L] buffer [x ; t] and fresh packs.  Saves that buffer -- x is the first leaky
    ReLU's input, t the second's OUTPUT, whose sign is its input's -- and the weights; returns (y, buffer)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, ws, bs, dil, slope):
        B, C, L = x.shape
        buf = torch.empty(B, 2 * C, L, device=x.device, dtype=torch.float32)
        buf[:, :C].copy_(x)
        mixed = []

        def mix():
            mixed.append(torch.cat([ws, w2], 1))
            return ops.pack_conv_weight(mixed[0], ops.PACK_PLAIN), bs + b2

        y = melgan_block_fwd(buf, ops.pack_conv_weight(w1, ops.PACK_PLAIN), b1, mix, C, dil, slope)
        ctx.save_for_backward(buf, w1, mixed[0])
        ctx.cfg = (dil, slope)
        ctx.mark_non_differentiable(buf)
        return y, buf

    @staticmethod
    def backward(ctx, g, _gbuf):
        buf, w1, wmix = ctx.saved_tensors
        dil, slope = ctx.cfg
        B, C2, L = buf.shape
        C = C2 // 2
        g = g.contiguous()
        db = ops.rowsum(g)                                                        # db_s = db_2
        dmix = ops.conv1d_wgrad(g, buf, 1)                                        # d[Ws | W2]  [C, 2C, 1]
        dbuf = ops.conv1d_packed(g, ops.pack_conv_weight(wmix, ops.PACK_DGRAD), None, C2, 1)   # [d x (shortcut) ; d t]
        dt = ops.lrelu_bwd_strided(dbuf, C * L, C2 * L, buf, C * L, C2 * L, B, C, L, slope)
        dw1, db1, dx = _voc_conv_bwd(dt, buf, w1, dil, REFLECT, slope, 1.0, add=dbuf, x_bs=C2 * L, add_bs=C2 * L, C=C)
        return dx, dw1, db1, dmix[:, C:], db, dmix[:, :C], db, None, None


def melgan_resblock(x, w1, b1, w2, b2, ws, bs, dil, slope):
    """-> (y [B, C, L], [x ; t] [B, 2C, L] detached: the two leaky ReLUs' sign carriers)."""
    _require_cuda(x, w1, w2, ws)
    return _MelResBlockFn.apply(x.contiguous(), w1.contiguous(), b1, w2.contiguous(), b2, ws.contiguous(), bs, dil, slope)


# --------------------------------------------------------------------------------------------------
# Discriminator stacks: a chain of convolutions as ONE node f(x, <two non-tensor arguments>, w0, b0, w1, b1, ...) that
# returns every layer's map, so that a map's outside gradient (feature matching) and the leaky-ReLU mask of the layer
# below (from the stored activated map: slope > 0 keeps the sign) ride in the data-gradient kernel's epilogue.
# --------------------------------------------------------------------------------------------------
def _stack_backward(need, gs, start, wgrad, dgrad, bottom):
    """-> (dx, None, None, dw0, db0, ...), each only where `need` (needs_input_grad) asks.  gs[j]: the outside gradient of
    layer j's map or None.  Walks from the highest map that has one down to `lowest`, the lowest layer with anything to
    compute at or below it.  d = gradient of layer j's PRE-activation: start(j, gs[j]) -> d; wgrad(j, d, want_w,
    want_b) -> (dw, db); dgrad(j, d, gs[j - 1]) -> d of layer j - 1, masked by layer j's input; bottom(d) -> dx."""
    n = len(gs)
    need_w = [need[3 + 2 * j] for j in range(n)]
    need_b = [need[4 + 2 * j] for j in range(n)]
    lowest = 0 if need[0] else min([j for j in range(n) if need_w[j] or need_b[j]], default=n)
    grads = [None] * (3 + 2 * n)
    d = None
    for j in range(n - 1, lowest - 1, -1):
        if d is None:
            if gs[j] is None:
                continue
            d = start(j, gs[j].contiguous())
        if need_w[j] or need_b[j]:
            dw, db = wgrad(j, d, need_w[j], need_b[j])
            grads[3 + 2 * j], grads[4 + 2 * j] = (dw if need_w[j] else None), (db if need_b[j] else None)
        if j > lowest:
            add = gs[j - 1]
            d = dgrad(j, d, None if add is None else add.contiguous())
        elif need[0]:
            grads[0] = bottom(d)
    return tuple(grads)


# --------------------------------------------------------------------------------------------------
# HiFi-GAN multi-scale discriminator (csrc/msd.hip; hifigan_discriminators.py)
# --------------------------------------------------------------------------------------------------
class _ScaleStackFn(torch.autograd.Function):
    """DiscriminatorS' one-channel first layer and the grouped layers above it as ONE node, every layer followed by
    leaky_relu(slope): x [N, 1, T] -> the activated maps.  params = (w0, b0, w1, b1, ...), effective weights;
    layers[j] = (stride, groups, padding)."""

    @staticmethod
    def forward(ctx, x, slope, layers, *params):
        _require_cuda(x)
        x = x.contiguous()
        ws = [w.detach().contiguous() for w in params[0::2]]
        bs = [b.detach() for b in params[1::2]]
        maps = [ops.conv1d_c1_fwd(x, ws[0], bs[0], layers[0][2], slope)]
        for j in range(1, len(layers)):
            s, g, pad = layers[j]
            Co, _, K = ws[j].shape
            maps.append(ops.gconv1d_fwd(maps[-1], ops.gconv_pack(ws[j], s, g), bs[j], Co, K, s, pad, g, slope))
        ctx.save_for_backward(x, *maps, *ws)
        ctx.cfg = (slope, layers)
        ctx.set_materialize_grads(False)
        return tuple(maps)

    @staticmethod
    def backward(ctx, *gs):
        slope, layers = ctx.cfg
        n = len(layers)
        saved = ctx.saved_tensors
        x, maps, ws = saved[0], saved[1:1 + n], saved[1 + n:]

        def wgrad(j, d, want_w, want_b):
            s, g, pad = layers[j]
            K = ws[j].shape[2]
            if j == 0:                             # the one-channel kernel gives both in one launch
                return ops.conv1d_c1_wgrad(d, x, K, pad)
            return (ops.gconv1d_wgrad(d, maps[j - 1], K, s, pad, g) if want_w else None,
                    ops.rowsum(d) if want_b else None)

        def dgrad(j, d, add):
            s, g, pad = layers[j]
            below = maps[j - 1]
            return ops.gconv1d_dgrad(d, ops.gconv_pack(ws[j], s, g, ops.GCONV_DGRAD), below.shape[1], below.shape[2],
                                     ws[j].shape[2], s, pad, g, map=below, add=add, slope=slope)

        return _stack_backward(ctx.needs_input_grad, gs, lambda j, g: ops.lrelu_bwd(g, maps[j], slope), wgrad, dgrad,
                               lambda d: ops.conv1d_c1_dgrad(d, ws[0], x.shape[2], layers[0][2]))


def scale_stack(x, slope, layers, *params):
    return _ScaleStackFn.apply(x, slope, tuple(layers), *params)


class _AvgPool4s2Fn(torch.autograd.Function):
    """AvgPool1d(4, 2, padding, count_include_pad=...): (2, True) is HiFi-GAN's MeanPool, (1, False) MelGAN's
    Downsample."""

    @staticmethod
    def forward(ctx, x, padding, count_include_pad):
        _require_cuda(x)
        ctx.cfg = (x.shape[2], padding, count_include_pad)
        return ops.avgpool4s2_fwd(x.contiguous(), padding, count_include_pad)

    @staticmethod
    def backward(ctx, g):
        return ops.avgpool4s2_bwd(g.contiguous(), *ctx.cfg), None, None


def avgpool4s2(x, padding=2, count_include_pad=True):
    return _AvgPool4s2Fn.apply(x, padding, count_include_pad)


# --------------------------------------------------------------------------------------------------
# MelGAN's discriminator (melgan_discriminators.py): the reflection pad in front of layer 0.  The grouped layers are
# scale_stack's, on the four-channel-group kernels of csrc/gconv_c4.h; the pool is avgpool4s2(x, 1, False).
# --------------------------------------------------------------------------------------------------
class _ReflectPad1dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        _require_cuda(x)
        ctx.p = p
        return ops.reflect_pad1d_fwd(x.contiguous(), p)

    @staticmethod
    def backward(ctx, g):
        return ops.reflect_pad1d_bwd(g.contiguous(), ctx.p), None


def reflect_pad1d(x, p):
    return _ReflectPad1dFn.apply(x, p)


# --------------------------------------------------------------------------------------------------
# HiFi-GAN multi-period discriminator (csrc/mpd.hip; hifigan_discriminators.py)
# --------------------------------------------------------------------------------------------------
class _PeriodStackFn(torch.autograd.Function):
    """DiscriminatorP(p) as ONE node: the fold of x [N, 1, T] onto the slotted axis, the five leaky-ReLU layers and
    conv_post; returns the six slotted maps [1, C, N p S[j]] (slack exactly 0).  params = (w0, b0, ..., w5, b5),
    effective [Co, Ci, K] weights."""

    @staticmethod
    def forward(ctx, x, p, slope, *params):
        _require_cuda(x)
        if x.dim() != 3 or x.shape[1] != 1:
            raise _lib.MixganHipError("period_stack: expected a waveform [N, 1, T], got %s" % (tuple(x.shape),))
        x = x.contiguous()
        N, _, T = x.shape
        H, S = ops.period_geometry(T, p)
        ws = [w.detach().contiguous() for w in params[0::2]]
        bs = [b.detach() for b in params[1::2]]
        n = len(ws)
        bufs = [ops.period_fold_fwd(x, p)]
        for j in range(n):
            bufs.append(ops.period_conv_fwd(bufs[-1], ws[j], bs[j], N * p, S[j], S[j + 1], H[j + 1], S[j] // S[j + 1],
                                            slope if j < n - 1 else None))
        ctx.save_for_backward(*bufs[:-1], *ws)
        ctx.cfg = (N, T, p, slope, H, S)
        ctx.set_materialize_grads(False)
        return tuple(bufs[1:])

    @staticmethod
    def backward(ctx, *gs):
        N, T, p, slope, H, S = ctx.cfg
        n = len(gs)
        saved = ctx.saved_tensors
        bufs, ws = saved[:n], saved[n:]        # bufs[j]: the input of layer j (the fold, then the activated maps)
        R = N * p

        def start(j, g):                           # conv_post's map is raw; the others are activated
            return g if j == n - 1 else ops.lrelu_bwd(g, bufs[j + 1], slope)

        def wgrad(j, d, want_w, want_b):
            K = ws[j].shape[2]
            return (ops.conv1d_wgrad(d, bufs[j], K, S[j] // S[j + 1], (K - 1) // 2) if want_w else None,
                    ops.rowsum(d) if want_b else None)

        def dgrad(j, d, add):
            return ops.period_conv_dgrad(d, ws[j], R, S[j], H[j], S[j + 1], S[j] // S[j + 1], map=bufs[j], add=add,
                                         slope=slope)

        def bottom(d):                             # no mask below layer 0: the fold is linear
            return ops.period_fold_bwd(ops.period_conv_dgrad(d, ws[0], R, S[0], H[0], S[1], S[0] // S[1]), N, T, p)

        return _stack_backward(ctx.needs_input_grad, gs, start, wgrad, dgrad, bottom)


def period_stack(x, p, slope, *params):
    return _PeriodStackFn.apply(x, p, slope, *params)
