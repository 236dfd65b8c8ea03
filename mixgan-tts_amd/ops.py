"""Thin tensor-level wrappers over the C ABI (include/mixgan_hip.h).  Forward only here;
differentiable entry points live next to the modules that own the parameters."""
import ctypes
import os

import torch

from . import _lib
from ._lib import fptr, iptr, check, stream_ptr

ACT = {None: _lib.MG_ACT_NONE, "none": _lib.MG_ACT_NONE, "relu": _lib.MG_ACT_RELU, "lrelu": _lib.MG_ACT_LRELU02,
       "tanh": _lib.MG_ACT_TANH, "lrelu_s": _lib.MG_ACT_LRELU}
PACK_PLAIN, PACK_GATE, PACK_DGRAD = _lib.MG_PACK_PLAIN, _lib.MG_PACK_GATE, _lib.MG_PACK_DGRAD


def pack_conv_weight(w, mode=PACK_PLAIN, out=None):
    """[Co, Ci, K] (or [Co, Ci]) fp32 -> MFMA-fragment-ordered cache tensor (into `out` when it fits)."""
    L = _lib.lib()
    if w.dim() == 2:
        w = w[:, :, None]
    w = w.detach().contiguous()
    Co, Ci, K = w.shape
    n = L.mg_conv_packed_floats(Co, Ci, K, mode)
    if n == 0:
        raise _lib.MixganHipError("unsupported conv weight shape %s" % (tuple(w.shape),))
    if out is None or out.numel() != n or out.device != w.device:
        out = torch.empty(n, device=w.device, dtype=torch.float32)
    check(L.mg_conv_pack(fptr(w), fptr(out), Co, Ci, K, mode, stream_ptr()))
    return out


def pack_cached(w, mode=PACK_PLAIN):
    """pack_conv_weight with the result cached ON the owning parameter object (so its lifetime is the
    parameter's: an address-keyed cache goes stale when the allocator reuses freed storage).  The
    packed form is a derived cache, rebuilt when the parameter's version changes (optimizer step,
    load_state_dict)."""
    owner = w._base if w._base is not None else w
    cache = owner.__dict__.setdefault("_mg_pack", {})
    key = (mode, tuple(w.shape), owner.data_ptr())
    hit = cache.get(key)
    if hit is not None and hit[0] == owner._version:
        return hit[1]
    # refreshed IN PLACE when the buffer exists: launches captured in a hipGraph keep reading the same address
    p = pack_conv_weight(w, mode, out=None if hit is None else hit[1])
    cache[key] = (owner._version, p)
    return p


PACK_TPOSE = "tpose"   # polyphase ConvTranspose1d pack (pack_conv_transpose_weight)


def pack_conv_transpose_weight(w):
    """ConvTranspose1d weight [Ci, Co, 2u] (stride u, padding u/2) -> polyphase MFMA pack."""
    L = _lib.lib()
    w = w.detach().contiguous()
    Ci, Co, K = w.shape
    u = K // 2
    n = L.mg_conv_transpose_packed_floats(Ci, Co, u) if K == 2 * u else 0
    if n == 0:
        raise _lib.MixganHipError("unsupported transposed-conv weight shape %s" % (tuple(w.shape),))
    out = torch.empty(n, device=w.device, dtype=torch.float32)
    check(L.mg_conv_transpose_pack(fptr(w), fptr(out), Ci, Co, u, stream_ptr()))
    return out


def conv_transpose1d_packed(x, packed, bias, Co, u, in_slope=1.0, alpha=1.0):
    """alpha * conv_transpose1d(leaky_relu(x, in_slope), w, stride=u, padding=u/2) + bias; x [B,Ci,L] -> [B,Co,u*L]."""
    L = _lib.lib()
    B, Ci, Lin = x.shape
    out = torch.empty(B, Co, u * Lin, device=x.device, dtype=torch.float32)
    check(L.mg_conv_transpose1d_fwd(fptr(x), fptr(packed), fptr(bias, True), fptr(out), B, Ci, Lin, Co, u,
                                    float(in_slope), float(alpha), stream_ptr()))
    return out


_SPLIT_SCRATCH = {}
SPLIT_SCRATCH_FLOATS = 12 << 20


def split_scratch(dev):
    """The split-reduction scratch of mg_conv1d_fwd_split for the current stream.  One per (device, stream): launches
    on one stream are ordered, launches on different streams must not share partial tiles."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    buf = _SPLIT_SCRATCH.get(key)
    if buf is None:
        buf = _SPLIT_SCRATCH[key] = torch.empty(SPLIT_SCRATCH_FLOATS, device=dev, dtype=torch.float32)
    return buf


def conv1d_packed(x, packed, bias, Co, K, stride=1, padding=0, act=None, alpha=1.0, add=None, in_vec=None,
                  out=None, accumulate=False, Lout=None, dilation=1, in_slope=1.0, act_slope=0.0, split=False):
    """act: None | "relu" | "lrelu" (0.2) | "tanh" | "lrelu_s" (slope act_slope); in_slope: leaky ReLU
    applied to the input while staging (1 = identity).  split=True: let the library split a deep reduction over
    workgroups when the output is only a few tiles (mg_conv1d_fwd_split; same result up to summation order)."""
    L = _lib.lib()
    B, Ci, Lin = x.shape
    if Lout is None:
        Lout = (Lin + 2 * padding - dilation * (K - 1) - 1) // stride + 1
    if out is None:
        out = torch.empty(B, Co, Lout, device=x.device, dtype=torch.float32)
    scratch = None
    if split and os.environ.get("MG_CONV_SPLIT", "1") != "0" and not torch.cuda.is_current_stream_capturing():
        scratch = split_scratch(x.device)
    check(L.mg_conv1d_fwd_split(fptr(x), fptr(in_vec, True), fptr(packed), fptr(bias, True), fptr(add, True), fptr(out),
                                B, Ci, Lin, Co, Lout, K, stride, padding, dilation, float(in_slope), ACT[act],
                                float(act_slope), float(alpha), int(accumulate), fptr(scratch, True),
                                0 if scratch is None else scratch.numel(), stream_ptr()))
    return out


def conv1d(x, weight, bias=None, stride=1, padding=0, act=None):
    Co, _, K = weight.shape
    return conv1d_packed(x, pack_conv_weight(weight), None if bias is None else bias.detach(), Co, K, stride,
                         padding, act)


def linear(x, weight, bias=None):
    """x [..., in] -> [..., out] through the k=1 conv kernel (frames = flattened leading dims)."""
    shp = x.shape
    x2 = x.reshape(1, -1, shp[-1]).transpose(1, 2).contiguous()
    y = conv1d(x2, weight[:, :, None], bias)
    return y.transpose(1, 2).reshape(*shp[:-1], weight.shape[0])


def diffuse(mel, t, noise, keep, buf):
    """mg_diffuse_fwd: mel [B,L,M], noise [B,M,L] -> x_t [B,M,L]."""
    L = _lib.lib()
    B, Lf, M = mel.shape
    out = torch.empty(B, M, Lf, device=mel.device, dtype=torch.float32)
    check(L.mg_diffuse_fwd(fptr(mel), iptr(t, torch.int64), fptr(noise), iptr(keep, torch.uint8, True),
                           fptr(buf["spec_min"]), fptr(buf["spec_max"]), fptr(buf["sqrt_alphas_cumprod"]),
                           fptr(buf["sqrt_one_minus_alphas_cumprod"]), fptr(out), B, Lf, M,
                           buf["sqrt_alphas_cumprod"].numel(), stream_ptr()))
    return out


def posterior_sample(x0, x_t, t, noise, keep, buf, clip=True, want_x0c=False, out=None):
    L = _lib.lib()
    B, M, Lf = x_t.shape
    if out is None:
        out = torch.empty_like(x_t)
    x0c = torch.empty_like(x_t) if want_x0c else None
    check(L.mg_posterior_sample_fwd(fptr(x0), fptr(x_t), iptr(t, torch.int64), fptr(noise),
                                    iptr(keep, torch.uint8, True), fptr(buf["posterior_mean_coef1"]),
                                    fptr(buf["posterior_mean_coef2"]), fptr(buf["posterior_log_variance_clipped"]),
                                    fptr(out), fptr(x0c, True), int(clip), B, Lf, M,
                                    buf["posterior_mean_coef1"].numel(), stream_ptr()))
    return (out, x0c) if want_x0c else out


def transpose_bml(x, to_blm, mode=0, spec_min=None, spec_max=None, keep=None):
    """to_blm: [B,M,L] -> [B,L,M] (mode 2 = denorm_spec); else [B,L,M] -> [B,M,L] (mode 1 = norm_spec)."""
    L = _lib.lib()
    if to_blm:
        B, M, Lf = x.shape
        out = torch.empty(B, Lf, M, device=x.device, dtype=torch.float32)
    else:
        B, Lf, M = x.shape
        out = torch.empty(B, M, Lf, device=x.device, dtype=torch.float32)
    check(L.mg_transpose_bml(fptr(x), fptr(out), fptr(spec_min, True), fptr(spec_max, True),
                             iptr(keep, torch.uint8, True), int(to_blm), mode, B, Lf, M, stream_ptr()))
    return out


def posterior_sample_bwd(x0, t, keep, coef1, g_x0c, g_xpp, clip):
    L = _lib.lib()
    B, M, Lf = x0.shape
    out = torch.empty_like(x0)
    check(L.mg_posterior_sample_bwd(fptr(x0), iptr(t, torch.int64), iptr(keep, torch.uint8, True), fptr(coef1),
                                    fptr(g_x0c, True), fptr(g_xpp, True), fptr(out), int(clip), B, Lf, M,
                                    coef1.numel(), stream_ptr()))
    return out


def spec_affine(x, spec_min, spec_max, mode):
    L = _lib.lib()
    M = x.shape[-1]
    out = torch.empty_like(x)
    check(L.mg_spec_affine(fptr(x), fptr(out), fptr(spec_min.reshape(-1)), fptr(spec_max.reshape(-1)), mode,
                           x.numel(), M, stream_ptr()))
    return out


def conv1d_wgrad(dy, x, K, stride=1, padding=0, x_vec=None, alpha=1.0):
    """dW [Co, Ci, K] of conv1d(x, W): dy [B,Co,Ldy], x [B,Ci,Lx]."""
    L = _lib.lib()
    B, Co, Ldy = dy.shape
    _, Ci, Lx = x.shape
    dw = torch.empty(Co, Ci, K, device=x.device, dtype=torch.float32)
    scratch = torch.empty(L.mg_conv1d_wgrad_scratch_floats(Co, Ci, K), device=x.device, dtype=torch.float32)
    check(L.mg_conv1d_wgrad(fptr(dy), fptr(x), fptr(x_vec, True), fptr(dw), fptr(scratch), B, Co, Ci, Ldy, Lx, K,
                            stride, padding, float(alpha), 0, stream_ptr()))
    return dw


def rowsum(x, per_batch=False, alpha=1.0):
    """x [B,R,L] -> [R] (sum over b,l) or [B,R] (sum over l)."""
    L = _lib.lib()
    B, R, Lf = x.shape
    out = torch.empty((B, R) if per_batch else (R,), device=x.device, dtype=torch.float32)
    check(L.mg_rowsum(fptr(x), 0, B, R, Lf, fptr(None if per_batch else out, True), fptr(out if per_batch else None, True),
                      float(alpha), 0, stream_ptr()))
    return out


def conv1d_wgrad_ex(dy, x, K, dilation=1, padding=0, in_slope=1.0, alpha=1.0, out=None, accumulate=False):
    """dW [Co, Ci, K] of alpha * conv1d(leaky_relu(x, in_slope), W, dilation, padding) through the saved
    pre-activation x [B,Ci,Lx]; dy [B,Co,Ldy].  accumulate adds into `out`."""
    L = _lib.lib()
    B, Co, Ldy = dy.shape
    _, Ci, Lx = x.shape
    dw = out if out is not None else torch.empty(Co, Ci, K, device=x.device, dtype=torch.float32)
    scratch = torch.empty(L.mg_conv1d_wgrad_scratch_floats(Co, Ci, K), device=x.device, dtype=torch.float32)
    check(L.mg_conv1d_wgrad_ex(fptr(dy), 0, fptr(x), 0, fptr(dw), fptr(scratch), B, Co, Ci, Ldy, Lx, K, dilation, padding,
                               float(in_slope), float(alpha), int(accumulate), stream_ptr()))
    return dw


def lrelu_bwd(dy, x, slope, add=None, out=None):
    """dy * (x > 0 ? 1 : slope) (+ add): leaky ReLU backward through its saved input, residual gradient added."""
    L = _lib.lib()
    if out is None:
        out = torch.empty_like(dy)
    check(L.mg_lrelu_bwd(fptr(dy), fptr(x), fptr(add, True), fptr(out), float(slope), dy.numel(), stream_ptr()))
    return out


def _at(t, float_offset):
    fptr(t)
    return ctypes.c_void_p(t.data_ptr() + 4 * float_offset)


def conv1d_reflect_packed(x, packed, bias, Co, K, dilation=1, in_slope=1.0, act=None, act_slope=0.0, alpha=1.0, x_bs=0,
                          C=None, out=None, out_bs=0, out_off=0):
    """act(alpha * conv1d(reflection_pad(leaky_relu(x, in_slope), dilation (K-1)/2), w, dilation) + bias) on the
    MG_PACK_PLAIN pack.  x_bs / C: x is channels [0, C) of a buffer with that batch stride; out / out_bs / out_off:
    write into a buffer at that float offset and batch stride."""
    L = _lib.lib()
    B, Lf = x.shape[0], x.shape[2]
    Ci = x.shape[1] if C is None else C
    if out is None:
        out = torch.empty(B, Co, Lf, device=x.device, dtype=torch.float32)
    check(L.mg_conv1d_reflect_fwd(fptr(x), x_bs, fptr(packed), fptr(bias, True), _at(out, out_off), out_bs, B, Ci, Lf,
                                  Co, K, dilation, float(in_slope), ACT[act], float(act_slope), float(alpha),
                                  stream_ptr()))
    return out


def conv1d_reflect_wgrad(dy, x, K, dilation=1, in_slope=1.0, alpha=1.0, out=None, accumulate=False, x_bs=0, C=None,
                         dy_bs=0, Co=None):
    """dW [Co, Ci, K] of conv1d_reflect_packed through the saved pre-activation x (channels [0, C) of a buffer with
    batch stride x_bs when those are given); dy [B, Co, L], or channels [0, Co) of a buffer with batch stride dy_bs.
    accumulate adds into `out`."""
    L = _lib.lib()
    B, Lf = dy.shape[0], dy.shape[2]
    Co = dy.shape[1] if Co is None else Co
    Ci = x.shape[1] if C is None else C
    dw = out if out is not None else torch.empty(Co, Ci, K, device=x.device, dtype=torch.float32)
    scratch = torch.empty(L.mg_conv1d_wgrad_scratch_floats(Co, Ci, K), device=x.device, dtype=torch.float32)
    check(L.mg_conv1d_reflect_wgrad(fptr(dy), dy_bs, fptr(x), x_bs, fptr(dw), fptr(scratch), B, Co, Ci, Lf, K, dilation,
                                    float(in_slope), float(alpha), int(accumulate), stream_ptr()))
    return dw


def conv1d_reflect_dgrad(dy, w, x, dilation=1, in_slope=1.0, alpha=1.0, add=None, out=None, x_bs=0, add_bs=0, C=None):
    """dx [B, Ci, L] of conv1d_reflect_packed: the zero-padded correlation of dy with the MG_PACK_DGRAD pack of
    w [Co, Ci, K] over the padded length, folded back through the reflection, masked by the saved pre-activation x,
    plus `add` (a residual gradient).  x / add may be channels [0, C) of buffers with batch strides x_bs / add_bs;
    `out` may be a dense `add`."""
    L = _lib.lib()
    B, Co, Lf = dy.shape
    K = w.shape[2]
    Ci = x.shape[1] if C is None else C
    n = L.mg_conv1d_reflect_dgrad_workspace_floats(B, Ci, Lf, K, dilation)
    if n == 0:
        raise _lib.MixganHipError("reflect-padded conv: K = %d at dilation %d has no HIP backward" % (K, dilation))
    ws = torch.empty(n, device=dy.device, dtype=torch.float32)
    dx = out if out is not None else torch.empty(B, Ci, Lf, device=dy.device, dtype=torch.float32)
    check(L.mg_conv1d_reflect_dgrad(fptr(dy), fptr(pack_conv_weight(w, PACK_DGRAD)), fptr(x), x_bs, fptr(add, True),
                                    add_bs, fptr(dx), fptr(ws), n, B, Co, Ci, Lf, K, dilation, float(in_slope),
                                    float(alpha), stream_ptr()))
    return dx


def lrelu_bwd_strided(dy, dy_off, dy_bs, x, x_off, x_bs, B, C, Lf, slope, out=None):
    """lrelu_bwd on channel slices: dy and x start dy_off / x_off floats into buffers with batch strides dy_bs / x_bs
    (mg_reflect_fold_bwd with no padding); out [B, C, L] dense."""
    if out is None:
        out = torch.empty(B, C, Lf, device=dy.device, dtype=torch.float32)
    check(_lib.lib().mg_reflect_fold_bwd(_at(dy, dy_off), dy_bs, _at(x, x_off), x_bs, None, 0, fptr(out), B, C, Lf, 0,
                                         float(slope), stream_ptr()))
    return out


def conv_transpose1d_dgrad(dy, w, x, in_slope=1.0, alpha=1.0):
    """dx of alpha * conv_transpose1d(leaky_relu(x, in_slope), w [Ci,Co,2u], stride u, padding u/2); dy [B,Co,u*L]."""
    L = _lib.lib()
    B, Ci, Lin = x.shape
    _, Co, K = w.shape
    u = K // 2
    n = L.mg_conv_transpose1d_dgrad_workspace_floats(B, Ci, Lin, Co, u) if K == 2 * u else 0
    if n == 0:
        raise _lib.MixganHipError("unsupported transposed-conv weight shape %s" % (tuple(w.shape),))
    ws = torch.empty(n, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    check(L.mg_conv_transpose1d_dgrad(fptr(dy), fptr(w), fptr(x), fptr(dx), fptr(ws), n, B, Ci, Lin, Co, u,
                                      float(in_slope), float(alpha), stream_ptr()))
    return dx


def conv_transpose1d_wgrad(dy, x, Co, u, in_slope=1.0, alpha=1.0, out=None, accumulate=False):
    """dW [Ci, Co, 2u] of alpha * conv_transpose1d(leaky_relu(x, in_slope), W, stride u, padding u/2)."""
    L = _lib.lib()
    B, Ci, Lin = x.shape
    n = L.mg_conv_transpose1d_wgrad_scratch_floats(Ci, Co, u)
    if n == 0:
        raise _lib.MixganHipError("unsupported transposed-conv shape Ci=%d Co=%d u=%d" % (Ci, Co, u))
    dw = out if out is not None else torch.empty(Ci, Co, 2 * u, device=x.device, dtype=torch.float32)
    scratch = torch.empty(n, device=x.device, dtype=torch.float32)
    check(L.mg_conv_transpose1d_wgrad(fptr(dy), fptr(x), fptr(dw), fptr(scratch), B, Ci, Lin, Co, u, float(in_slope),
                                      float(alpha), int(accumulate), stream_ptr()))
    return dw


def act_bwd(dy, y, act):
    L = _lib.lib()
    out = torch.empty_like(dy)
    check(L.mg_act_bwd(fptr(dy), fptr(y), fptr(out), ACT[act], dy.numel(), stream_ptr()))
    return out


def upsample_zero(x, stride, Lup, slope=1.0):
    L = _lib.lib()
    B, C, Lin = x.shape
    out = torch.empty(B, C, Lup, device=x.device, dtype=torch.float32)
    check(L.mg_upsample_zero_act(fptr(x), fptr(out), B * C, Lin, stride, Lup, float(slope), stream_ptr()))
    return out


def cat_transpose(a, b):
    """torch.cat([a, b], -1).transpose(1, 2) for a, b [B,L,M] -> [B,2M,L] (model/mixgantts.py:262-264)."""
    L = _lib.lib()
    B, Lf, M = a.shape
    out = torch.empty(B, 2 * M, Lf, device=a.device, dtype=torch.float32)
    for i, src in enumerate((a, b)):
        dst = ctypes.c_void_p(out.data_ptr() + i * M * Lf * 4)
        check(L.mg_transpose_bml_strided(fptr(src), dst, None, None, None, 0, 0, B, Lf, M, 2 * M * Lf, stream_ptr()))
    return out


def split_transpose(g, M):
    """inverse of cat_transpose for gradients: g [B,2M,L] -> two [B,L,M]."""
    L = _lib.lib()
    B, M2, Lf = g.shape
    outs = []
    for i in range(2):
        o = torch.empty(B, Lf, M, device=g.device, dtype=torch.float32)
        src = ctypes.c_void_p(g.data_ptr() + i * M * Lf * 4)
        check(L.mg_transpose_bml_strided(src, fptr(o), None, None, None, 1, 0, B, Lf, M, M2 * Lf, stream_ptr()))
        outs.append(o)
    return outs


def transpose_max_m():
    """Largest M of transpose_bml / cat_transpose / split_transpose / diffuse on the current device."""
    return _lib.lib().mg_transpose_max_m()


def _aligned16(t, K):
    """t, or a fresh copy of it when the 16-byte loads of the small linears (K % 256 == 0) would read it misaligned:
    a view that starts a few floats into its storage."""
    return t.clone() if K % 256 == 0 and t.data_ptr() % 16 else t


def step_mlp_fwd(t, freq, W0, W2):
    L = _lib.lib()
    B = t.shape[0]
    D1, D0 = W0.shape
    D2 = W2.shape[0]
    dev = W0.device
    W0, W2 = _aligned16(W0, D0), _aligned16(W2, D1)
    emb, pre, h = (torch.empty(B, d, device=dev) for d in (D0, D1, D1))
    out = torch.empty(B, D2, device=dev)
    check(L.mg_step_mlp_fwd(iptr(t, torch.int64), fptr(freq), fptr(W0), fptr(W2), fptr(emb), fptr(pre), fptr(h),
                            fptr(out), B, D0, D1, D2, stream_ptr()))
    return out, emb, pre, h


def step_mlp_bwd(g, emb, pre, h, W2):
    L = _lib.lib()
    B, D2 = g.shape
    D0, D1 = emb.shape[1], pre.shape[1]
    dW0 = torch.empty(D1, D0, device=g.device)
    dW2 = torch.empty(D2, D1, device=g.device)
    scratch = torch.empty(2 * B * D1, device=g.device)
    check(L.mg_step_mlp_bwd(fptr(g), fptr(emb), fptr(pre), fptr(h), fptr(W2), fptr(dW0), fptr(dW2), fptr(scratch),
                            B, D0, D1, D2, stream_ptr()))
    return dW0, dW2


def linear_small_fwd(x, W):
    L = _lib.lib()
    B, K = x.shape
    N = W.shape[0]
    out = torch.empty(B, N, device=x.device)
    x, W = _aligned16(x, K), _aligned16(W, K)
    check(L.mg_linear_small_fwd(fptr(x), fptr(W), fptr(out), B, N, K, stream_ptr()))
    return out


def linear_small_bwd(g, x, W, want_dx=True):
    L = _lib.lib()
    B, N = g.shape
    K = x.shape[1]
    dx = torch.empty_like(x) if want_dx else None
    dW = torch.empty_like(W)
    check(L.mg_linear_small_bwd(fptr(g), fptr(x), fptr(W), fptr(dx, True), fptr(dW), B, N, K, stream_ptr()))
    return dx, dW


def attention(qkv, key_pad, n_head, d_head, precision="fp32"):
    """qkv [B, 3*n_head*d_head, L] -> [B, n_head*d_head, L] (mg_attention_fwd; precision "f16": fp16 MFMA operands)."""
    L = _lib.lib()
    B, _, Lf = qkv.shape
    out = torch.empty(B, n_head * d_head, Lf, device=qkv.device, dtype=torch.float32)
    if precision not in ("fp32", "f16"):
        raise ValueError("attention precision must be 'fp32' or 'f16', got %r" % (precision,))
    fn = L.mg_attention_fwd if precision == "fp32" else L.mg_attention_fwd_f16
    check(fn(fptr(qkv), iptr(key_pad, torch.uint8, True), fptr(out), B, Lf, n_head, d_head,
                             float(d_head) ** -0.5, stream_ptr()))
    return out


def layernorm_cm(a, res, gamma, beta, pad, eps=1e-5):
    L = _lib.lib()
    B, C, Lf = a.shape
    out = torch.empty_like(a)
    check(L.mg_layernorm_cm_fwd(fptr(a), fptr(res, True), fptr(gamma), fptr(beta), iptr(pad, torch.uint8, True),
                                fptr(out), B, C, Lf, float(eps), stream_ptr()))
    return out


# ------------------------------------------------------------------ aux pre-training (train_ops.hip, bgemm.hip)
def _u8(t, allow_none=True):
    return iptr(t, torch.uint8, allow_none)


def attention_train_fwd(qkv, key_pad, n_head, d):
    """Train-mode attention keeping the probabilities: qkv [B,3HD,L] -> (out [B,HD,L], P [B*H,L,L])."""
    Lb = _lib.lib()
    B, _, L = qkv.shape
    HD, scale, st = n_head * d, float(d) ** -0.5, stream_ptr()
    P = torch.empty(B * n_head, L, L, device=qkv.device, dtype=torch.float32)
    q, k, v = qkv, qkv[:, HD:], qkv[:, 2 * HD:]
    bs, hs = 3 * HD * L, d * L
    # S[q,k] = sum_d Q[d,q] K[d,k]
    check(Lb.mg_bgemm(ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(k.data_ptr()), fptr(P), L, L, d, B, n_head,
                      1, L, bs, hs, L, 1, bs, hs, L, n_head * L * L, L * L, 1.0, 0, st))
    check(Lb.mg_softmax_rows_fwd(fptr(P), _u8(key_pad), B, n_head, L, scale, st))
    out = torch.empty(B, HD, L, device=qkv.device, dtype=torch.float32)
    # O[d,q] = sum_k V[d,k] P[q,k]
    check(Lb.mg_bgemm(ctypes.c_void_p(v.data_ptr()), fptr(P), fptr(out), d, L, L, B, n_head,
                      L, 1, bs, hs, 1, L, n_head * L * L, L * L, L, HD * L, d * L, 1.0, 0, st))
    return out, P


def attention_train_bwd(qkv, P, d_out, n_head, d):
    """-> d_qkv [B,3HD,L]."""
    Lb = _lib.lib()
    B, _, L = qkv.shape
    HD, scale, st = n_head * d, float(d) ** -0.5, stream_ptr()
    q, k, v = qkv, qkv[:, HD:], qkv[:, 2 * HD:]
    bs, hs = 3 * HD * L, d * L
    pbs, phs = n_head * L * L, L * L
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = dqkv, dqkv[:, HD:], dqkv[:, 2 * HD:]
    cp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    # dV[d,k] = sum_q dO[d,q] P[q,k]
    check(Lb.mg_bgemm(fptr(d_out), fptr(P), cp(dv), d, L, L, B, n_head, L, 1, HD * L, d * L, L, 1, pbs, phs,
                      L, bs, hs, 1.0, 0, st))
    # dP[q,k] = sum_d dO[d,q] V[d,k]
    dS = torch.empty_like(P)
    check(Lb.mg_bgemm(fptr(d_out), cp(v), fptr(dS), L, L, d, B, n_head, 1, L, HD * L, d * L, L, 1, bs, hs,
                      L, pbs, phs, 1.0, 0, st))
    check(Lb.mg_softmax_rows_bwd(fptr(P), fptr(dS), B, n_head, L, scale, st))
    # dQ[d,q] = sum_k K[d,k] dS[q,k];  dK[d,k] = sum_q Q[d,q] dS[q,k]
    check(Lb.mg_bgemm(cp(k), fptr(dS), cp(dq), d, L, L, B, n_head, L, 1, bs, hs, 1, L, pbs, phs, L, bs, hs, 1.0, 0, st))
    check(Lb.mg_bgemm(cp(q), fptr(dS), cp(dk), d, L, L, B, n_head, L, 1, bs, hs, L, 1, pbs, phs, L, bs, hs, 1.0, 0, st))
    return dqkv


def layernorm_cm_train(a, keep, drop_scale, res, gamma, beta, pad, eps=1e-5):
    Lb = _lib.lib()
    B, C, L = a.shape
    pre, out = torch.empty_like(a), torch.empty_like(a)
    check(Lb.mg_layernorm_cm_train_fwd(fptr(a), _u8(keep), float(drop_scale), fptr(res, True), fptr(gamma), fptr(beta),
                                       _u8(pad), fptr(pre), fptr(out), B, C, L, float(eps), stream_ptr()))
    return out, pre


def layernorm_cm_bwd(pre, dy, gamma, pad, keep, drop_scale, eps=1e-5):
    """-> (d_pre, d_a, dgamma, dbeta)."""
    Lb = _lib.lib()
    B, C, L = pre.shape
    d_pre = torch.empty_like(pre)
    d_a = torch.empty_like(pre) if keep is not None else None
    part = torch.zeros(2, 32, C, device=pre.device, dtype=torch.float32)     # 32 partial-sum slots per vector
    check(Lb.mg_layernorm_cm_bwd(fptr(pre), fptr(dy), fptr(gamma), _u8(pad), _u8(keep), float(drop_scale), fptr(d_pre),
                                 fptr(d_a, True), fptr(part[0]), fptr(part[1]), B, C, L, float(eps), stream_ptr()))
    dgb = part.sum(1)
    return d_pre, (d_a if d_a is not None else d_pre), dgb[0], dgb[1]


def bn_stats(x):
    Lb = _lib.lib()
    B, C, L = x.shape
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    var = torch.empty(C, device=x.device, dtype=torch.float32)
    check(Lb.mg_bn_stats(fptr(x), fptr(mean), fptr(var), B, C, L, stream_ptr()))
    return mean, var


def bn_act_fwd(x, mean, invstd, gamma, beta, keep, drop_scale, act):
    Lb = _lib.lib()
    B, C, L = x.shape
    y = torch.empty_like(x) if act == "tanh" else None
    out = torch.empty_like(x)
    check(Lb.mg_bn_act_fwd(fptr(x), fptr(mean), fptr(invstd), fptr(gamma), fptr(beta), _u8(keep), float(drop_scale),
                           ACT[act], fptr(y, True), fptr(out), B, C, L, stream_ptr()))
    return out, y


def bn_act_bwd_reduce(dout, keep, drop_scale, y, x, mean, invstd, act):
    Lb = _lib.lib()
    B, C, L = x.shape
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty(C, device=x.device, dtype=torch.float32)
    check(Lb.mg_bn_act_bwd_reduce(fptr(dout), _u8(keep), float(drop_scale), fptr(y, True), fptr(x), fptr(mean),
                                  fptr(invstd), ACT[act], fptr(dg), fptr(db), B, C, L, stream_ptr()))
    return dg, db


def bn_act_bwd_apply(dout, keep, drop_scale, y, x, mean, invstd, gamma, dg, db, inv_count, act):
    Lb = _lib.lib()
    B, C, L = x.shape
    dx = torch.empty_like(x)
    check(Lb.mg_bn_act_bwd_apply(fptr(dout), _u8(keep), float(drop_scale), fptr(y, True), fptr(x), fptr(mean),
                                 fptr(invstd), fptr(gamma), fptr(dg), fptr(db), float(inv_count), ACT[act], fptr(dx),
                                 B, C, L, stream_ptr()))
    return dx


def resblock_fwd(x, cond, wc_p, w3_p, wo_p, bc, b3, bo, hvec, dvec, save):
    """mg_resblock_fwd: one fused residual layer.  Returns (x_out, skip, saves) with saves = (h, g, sig, tnh) | None."""
    L = _lib.lib()
    B, C, Lf = x.shape
    H = cond.shape[1]
    x_out, skip = torch.empty_like(x), torch.empty_like(x)
    saves = tuple(torch.empty_like(x) for _ in range(4)) if save else None
    sp = [fptr(t) for t in saves] if save else [fptr(None, True)] * 4
    check(L.mg_resblock_fwd(fptr(x), fptr(cond), fptr(wc_p), fptr(w3_p), fptr(wo_p), fptr(bc), fptr(b3), fptr(bo),
                            fptr(hvec), fptr(dvec), fptr(x_out), fptr(skip), *sp, B, C, H, Lf, stream_ptr()))
    return x_out, skip, saves


def gate_bwd(dg, sig, tnh):
    L = _lib.lib()
    B, C, Lf = dg.shape
    dz = torch.empty(B, 2 * C, Lf, device=dg.device, dtype=torch.float32)
    check(L.mg_gate_bwd(fptr(dg), fptr(sig), fptr(tnh), fptr(dz), B, C, Lf, stream_ptr()))
    return dz


def mish_fwd(x):
    y = torch.empty_like(x)
    check(_lib.lib().mg_mish_fwd(fptr(x), fptr(y), x.numel(), stream_ptr()))
    return y


def mish_bwd(gy, x):
    gx = torch.empty_like(x)
    check(_lib.lib().mg_mish_bwd(fptr(gy), fptr(x), fptr(gx), x.numel(), stream_ptr()))
    return gx


def step_embed(t, freq):
    """DiffusionEmbedding: t int64 [B], freq [D/2] -> [B, D]."""
    B, D = t.shape[0], 2 * freq.shape[0]
    emb = torch.empty(B, D, device=t.device, dtype=torch.float32)
    check(_lib.lib().mg_step_embed(iptr(t, torch.int64), fptr(freq), fptr(emb), B, D, stream_ptr()))
    return emb


def grad_norm(flat, max_norm, out=None, scratch=None):
    """(||flat||_2, clip factor min(1, max_norm / (norm + 1e-6))) as a 2-element device tensor (no host sync)."""
    L = _lib.lib()
    if out is None:
        out = torch.empty(2, device=flat.device, dtype=torch.float32)
    if scratch is None:
        scratch = torch.empty(L.mg_grad_norm_scratch_floats(), device=flat.device, dtype=torch.float32)
    check(L.mg_grad_norm(fptr(flat), flat.numel(), float(max_norm), fptr(scratch), fptr(out), stream_ptr()))
    return out


def adam_flat(p, g, m, v, lr, betas, eps, weight_decay, step, grad_scale=None, hyper=None):
    """One torch.optim.Adam step on flat buffers, in place on p, m, v; g * grad_scale[0] is the gradient used.
    hyper: device pair {lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)} read by the kernel instead of lr / step (graphs)."""
    L = _lib.lib()
    check(L.mg_adam_flat_dev(fptr(p), fptr(g), fptr(m), fptr(v), p.numel(), float(lr), float(betas[0]), float(betas[1]),
                             float(eps), float(weight_decay), int(step), fptr(grad_scale, True), fptr(hyper, True),
                             stream_ptr()))


# ---- HiFi-GAN multi-scale discriminator (csrc/msd.hip)
GCONV_FWD, GCONV_DGRAD = _lib.MG_GCONV_FWD, _lib.MG_GCONV_DGRAD


def gconv_pack(w, stride, groups, mode=GCONV_FWD):
    """Grouped Conv1d weight [Co, Ci / groups, K] -> the fragment-ordered pack of mg_gconv1d_fwd (GCONV_FWD) or of
    mg_gconv1d_dgrad (GCONV_DGRAD); raises for a (Ci / G, Co / G, K, stride) the library does not instantiate."""
    L = _lib.lib()
    w = w.detach().contiguous()
    Co, Cig, K = w.shape
    n = L.mg_gconv_packed_floats(Cig * groups, Co, K, stride, groups, mode)
    if n == 0:
        raise _lib.MixganHipError("unsupported grouped conv: weight %s, stride %d, groups %d" % (tuple(w.shape), stride,
                                                                                                groups))
    out = torch.empty(n, device=w.device, dtype=torch.float32)
    check(L.mg_gconv_pack(fptr(w), fptr(out), Cig * groups, Co, K, stride, groups, mode, stream_ptr()))
    return out


def gconv1d_fwd(x, packed, bias, Co, K, stride, padding, groups, slope=None):
    """act(conv1d(x, w, bias, stride, padding, groups)), act = leaky ReLU with `slope` (None: no activation)."""
    N, Ci, Lin = x.shape
    Lout = (Lin + 2 * padding - K) // stride + 1
    out = torch.empty(N, Co, max(Lout, 0), device=x.device, dtype=torch.float32)
    check(_lib.lib().mg_gconv1d_fwd(fptr(x), fptr(packed), fptr(bias, True), fptr(out), N, Ci, Lin, Co, Lout, K, stride,
                                    padding, groups, _lib.MG_ACT_NONE if slope is None else _lib.MG_ACT_LRELU,
                                    0.0 if slope is None else float(slope), stream_ptr()))
    return out


def gconv1d_dgrad(dy, packed, Ci, Lin, K, stride, padding, groups, map=None, add=None, slope=1.0):
    """(data gradient of gconv1d_fwd + add) * (map > 0 ? 1 : slope); packed is the GCONV_DGRAD form."""
    N, Co, Lout = dy.shape
    dx = torch.empty(N, Ci, Lin, device=dy.device, dtype=torch.float32)
    check(_lib.lib().mg_gconv1d_dgrad(fptr(dy), fptr(packed), fptr(map, True), fptr(add, True), fptr(dx), N, Ci, Lin, Co,
                                      Lout, K, stride, padding, groups, float(slope), stream_ptr()))
    return dx


def gconv1d_wgrad(dy, x, K, stride, padding, groups):
    """dW [Co, Ci / groups, K] of gconv1d_fwd: dy [N, Co, Lout], x [N, Ci, Lin]."""
    L = _lib.lib()
    N, Co, Lout = dy.shape
    _, Ci, Lin = x.shape
    n = L.mg_gconv1d_wgrad_scratch_floats(N, Ci, Co, Lout, K, stride, groups)
    if n == 0:
        raise _lib.MixganHipError("unsupported grouped conv: Ci %d Co %d K %d stride %d groups %d" % (Ci, Co, K, stride,
                                                                                                      groups))
    dw = torch.empty(Co, Ci // groups, K, device=x.device, dtype=torch.float32)
    scratch = torch.empty(n, device=x.device, dtype=torch.float32)
    check(L.mg_gconv1d_wgrad(fptr(dy), fptr(x), fptr(dw), fptr(scratch), n, N, Ci, Lin, Co, Lout, K, stride, padding,
                             groups, stream_ptr()))
    return dw


def conv1d_c1_fwd(x, w, bias, padding, slope=None):
    """act(conv1d(x [N, 1, L], w [Co, 1, K], bias, padding)): the one-input-channel first layer."""
    N, _, Lin = x.shape
    Co, _, K = w.shape
    out = torch.empty(N, Co, Lin + 2 * padding - K + 1, device=x.device, dtype=torch.float32)
    check(_lib.lib().mg_conv1d_c1_fwd(fptr(x), fptr(w), fptr(bias, True), fptr(out), N, Lin, Co, K, padding,
                                      _lib.MG_ACT_NONE if slope is None else _lib.MG_ACT_LRELU,
                                      0.0 if slope is None else float(slope), stream_ptr()))
    return out


def conv1d_c1_dgrad(dy, w, Lin, padding):
    N, Co, _ = dy.shape
    dx = torch.empty(N, 1, Lin, device=dy.device, dtype=torch.float32)
    check(_lib.lib().mg_conv1d_c1_dgrad(fptr(dy), fptr(w), fptr(dx), N, Lin, Co, w.shape[2], padding, stream_ptr()))
    return dx


def conv1d_c1_wgrad(dy, x, K, padding):
    """(dW [Co, 1, K], db [Co]) of conv1d_c1_fwd."""
    L = _lib.lib()
    N, Co, _ = dy.shape
    Lin = x.shape[2]
    n = L.mg_conv1d_c1_wgrad_scratch_floats(N, Lin, Co, K)
    if n == 0:
        raise _lib.MixganHipError("unsupported first-layer conv: Co %d K %d" % (Co, K))
    dw = torch.empty(Co, 1, K, device=x.device, dtype=torch.float32)
    db = torch.empty(Co, device=x.device, dtype=torch.float32)
    scratch = torch.empty(n, device=x.device, dtype=torch.float32)
    check(L.mg_conv1d_c1_wgrad(fptr(dy), fptr(x), fptr(dw), fptr(db), fptr(scratch), n, N, Lin, Co, K, padding,
                               stream_ptr()))
    return dw, db


def _avgpool4s2_export(padding, count_include_pad, which):
    if (padding, bool(count_include_pad)) not in ((2, True), (1, False)):
        raise ValueError("avgpool4s2: the library has (padding 2, count_include_pad True) and (1, False), got (%r, %r)"
                         % (padding, count_include_pad))
    return getattr(_lib.lib(), "mg_avgpool4s2%s_%s" % ("" if padding == 2 else "p1", which))


def avgpool4s2_fwd(x, padding=2, count_include_pad=True):
    """AvgPool1d(4, 2, padding, count_include_pad=...) of x [N, C, L] -> [N, C, (L + 2 padding - 4) / 2 + 1]:
    (2, True) is HiFi-GAN's, (1, False) MelGAN's, whose windows divide by their in-range count."""
    export = _avgpool4s2_export(padding, count_include_pad, "fwd")
    N, C, Lin = x.shape
    out = torch.empty(N, C, max((Lin + 2 * padding - 4) // 2 + 1, 0), device=x.device, dtype=torch.float32)
    check(export(fptr(x), fptr(out), N * C, Lin, stream_ptr()))
    return out


def avgpool4s2_bwd(dy, Lin, padding=2, count_include_pad=True):
    export = _avgpool4s2_export(padding, count_include_pad, "bwd")
    N, C, _ = dy.shape
    dx = torch.empty(N, C, Lin, device=dy.device, dtype=torch.float32)
    check(export(fptr(dy), fptr(dx), N * C, Lin, stream_ptr()))
    return dx


# ---- MelGAN's discriminator (csrc/msd.hip): the reflection pad in front of layer 0
def reflect_pad1d_fwd(x, p):
    """ReflectionPad1d(p) of x [N, C, T] -> [N, C, T + 2 p]."""
    N, C, T = x.shape
    out = torch.empty(N, C, T + 2 * p, device=x.device, dtype=torch.float32)
    check(_lib.lib().mg_reflect_pad1d_fwd(fptr(x), fptr(out), N * C, T, p, stream_ptr()))
    return out


def reflect_pad1d_bwd(dy, p):
    """The fold-back: dy [N, C, T + 2 p] -> [N, C, T], the mirrored pad samples added into the positions they read."""
    N, C, Tp = dy.shape
    dx = torch.empty(N, C, max(Tp - 2 * p, 0), device=dy.device, dtype=torch.float32)
    check(_lib.lib().mg_reflect_pad1d_bwd(fptr(dy), fptr(dx), N * C, Tp - 2 * p, p, stream_ptr()))
    return dx


# ---- HiFi-GAN multi-period discriminator (csrc/mpd.hip): one layer at a time on the slotted flat axis
def period_geometry(T, p):
    """(H[0..6], S[0..6]) of DiscriminatorP(p) on T samples (mg_period_geometry, the one source of these numbers)."""
    H, S = (ctypes.c_int * 7)(), (ctypes.c_int * 7)()
    rc = _lib.lib().mg_period_geometry(int(T), int(p), H, S)
    if rc != 0:
        raise _lib.MixganHipError("DiscriminatorP(%d): %d samples do not fold (the reflect pad needs T > p - 1 - (T - 1) %% p)"
                                  % (p, T))
    return list(H), list(S)


def period_fold_fwd(y, p):
    """y [N, 1, T] -> the slotted layer-0 input [1, 1, N p S0]."""
    N, _, T = y.shape
    _, S = period_geometry(T, p)
    out = torch.empty(1, 1, N * p * S[0], device=y.device, dtype=torch.float32)
    check(_lib.lib().mg_period_fold_fwd(fptr(y), fptr(out), N, T, p, stream_ptr()))
    return out


def period_fold_bwd(din0, N, T, p):
    dy = torch.empty(N, 1, T, device=din0.device, dtype=torch.float32)
    check(_lib.lib().mg_period_fold_bwd(fptr(din0), fptr(dy), N, T, p, stream_ptr()))
    return dy


def _period_scratch(x, split):
    if split and os.environ.get("MG_CONV_SPLIT", "1") != "0" and not torch.cuda.is_current_stream_capturing():
        return split_scratch(x.device)
    return None


def period_conv_fwd(x, w, bias, R, S_in, S_out, H_out, stride, slope=None, split=True):
    """One layer: x [1, Ci, R S_in] slotted, w [Co, Ci, K] -> [1, Co, R S_out] slotted (slack exactly 0), leaky ReLU with
    `slope` (None: no activation)."""
    Co, Ci, K = w.shape
    Lin = x.shape[2]
    out = torch.empty(1, Co, R * S_out, device=x.device, dtype=torch.float32)
    scratch = _period_scratch(x, split)
    check(_lib.lib().mg_period_conv_fwd(fptr(x), fptr(pack_conv_weight(w, PACK_PLAIN)), fptr(bias, True), fptr(out), R, Ci,
                                        Lin, S_in, Co, R * S_out, S_out, H_out, K, stride,
                                        _lib.MG_ACT_NONE if slope is None else _lib.MG_ACT_LRELU,
                                        0.0 if slope is None else float(slope), fptr(scratch, True),
                                        0 if scratch is None else scratch.numel(), stream_ptr()))
    return out


def period_dgrad3_pack(w):
    """[Co, Ci, 5] -> the two-tap polyphase pack of the stride-3 data gradient."""
    L = _lib.lib()
    w = w.detach().contiguous()
    Co, Ci, K = w.shape
    n = L.mg_period_dgrad3_packed_floats(Co, Ci) if K == 5 else 0
    if n == 0:
        raise _lib.MixganHipError("unsupported period conv weight shape %s" % (tuple(w.shape),))
    out = torch.empty(n, device=w.device, dtype=torch.float32)
    check(L.mg_period_dgrad3_pack(fptr(w), fptr(out), Co, Ci, stream_ptr()))
    return out


def period_conv_dgrad(d, w, R, S_in, H_in, S_out, stride, map=None, add=None, slope=1.0, split=True):
    """(data gradient of period_conv_fwd + add) * (map > 0 ? 1 : slope), slack exactly 0: d [1, Co, R S_out] ->
    [1, Ci, R S_in]."""
    Co, Ci, K = w.shape
    packed = period_dgrad3_pack(w) if stride == 3 else pack_conv_weight(w, PACK_DGRAD)
    dx = torch.empty(1, Ci, R * S_in, device=d.device, dtype=torch.float32)
    scratch = _period_scratch(d, split)
    check(_lib.lib().mg_period_conv_dgrad(fptr(d), fptr(packed), fptr(map, True), fptr(add, True), fptr(dx), R, Ci,
                                          R * S_in, S_in, H_in, Co, d.shape[2], S_out, K, stride, float(slope),
                                          fptr(scratch, True), 0 if scratch is None else scratch.numel(), stream_ptr()))
    return dx
