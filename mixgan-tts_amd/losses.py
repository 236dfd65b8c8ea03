"""Losses that enter the hot path's backward (model/loss.py:12-30, 221-242, 255-259): LSGAN
on the last feature map of the JCU discriminator, feature matching over the first four maps and
the masked mel L1.  Reductions and their gradients run in the HIP library."""
import collections
import ctypes

import torch

from . import _lib
from ._lib import fptr, iptr, check, stream_ptr


class _MseConstFn(torch.autograd.Function):
    """F.mse_loss(x, full_like(x, c)) -- mean (x - c)^2."""

    @staticmethod
    def forward(ctx, x, c):
        x = x.contiguous()
        out = torch.empty(1, device=x.device)
        check(_lib.lib().mg_loss_sum(fptr(x), None, float(c), 0, x.numel(), fptr(out), stream_ptr()))
        ctx.save_for_backward(x)
        ctx.c = float(c)
        return out[0] / x.numel()

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        check(_lib.lib().mg_loss_grad(fptr(x), None, ctx.c, 0, fptr(g.reshape(1).contiguous()), 1.0 / x.numel(),
                                      x.numel(), fptr(dx), stream_ptr()))
        return dx, None


class _L1Fn(torch.autograd.Function):
    """F.l1_loss(target, pred) with gradient to `pred` only (the reference detaches the real maps).
    den (host number, optional): the divisor in place of pred.numel() -- the element count of the WHOLE batch when
    `pred` is one rank's shard of it."""

    @staticmethod
    def forward(ctx, pred, target, den=None):
        pred, target = pred.contiguous(), target.detach().contiguous()
        if den is not None and not den > 0:
            raise ValueError("den must be positive")
        out = torch.empty(1, device=pred.device)
        check(_lib.lib().mg_loss_sum(fptr(pred), fptr(target), 0.0, 1, pred.numel(), fptr(out), stream_ptr()))
        ctx.save_for_backward(pred, target)
        ctx.den = pred.numel() if den is None else den
        return out[0] / ctx.den

    @staticmethod
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        d = torch.empty_like(pred)
        check(_lib.lib().mg_loss_grad(fptr(pred), fptr(target), 0.0, 1, fptr(g.reshape(1).contiguous()),
                                      1.0 / ctx.den, pred.numel(), fptr(d), stream_ptr()))
        return d, None, None


_SCRATCH = {}


def _multi_scratch(dev):
    """Zero-initialised once per (device, stream): the kernel keeps its ticket there and re-arms it."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    if key not in _SCRATCH:
        _SCRATCH[key] = torch.zeros(_lib.lib().mg_multi_loss_scratch_floats(), device=dev, dtype=torch.float32)
    return _SCRATCH[key]


# One entry of a loss table (MgLossTerm): mode (_lib.MG_LOSSMODE_*), c, weight, group; x: which tensor, rows [lo, hi) of
# it (hi None: the whole tensor); y: which tensor holds the L1 target (x itself, or another one: it gets no gradient), from
# row y_lo on; den: a host denominator in place of the term's element count.
_Term = collections.namedtuple("_Term", "mode c weight group x lo hi y y_lo den", defaults=(0, None, None, 0, None))


def _loss_table(spec, ts, grads=None):
    """(MgLossTerm array of `spec` over the contiguous tensors `ts`, its denominators as a double array or None).
    grads: per tensor the gradient buffer its terms write into, or None (the forward)."""
    nt = len(spec)
    terms = (_lib.LossTerm * nt)()
    for k, s in enumerate(spec):
        x, y = ts[s.x], None if s.y is None else ts[s.y]
        if s.hi is None:            # the whole tensor, as one row
            lo, rows, per = 0, 1, x.numel()
            if y is not None and (y.shape != x.shape or s.y_lo != 0):
                raise ValueError("term %d: shapes %s vs %s" % (k, tuple(x.shape), tuple(y.shape)))
        else:
            lo, rows, per = s.lo, s.hi - s.lo, x.numel() // max(1, x.shape[0])
            if not (0 <= lo < s.hi <= x.shape[0]) or (y is not None and not (
                    0 <= s.y_lo and s.y_lo + rows <= y.shape[0] and (y is x or y.shape[1:] == x.shape[1:]))):
                raise ValueError("term %d: batch range outside the tensor" % k)
        d = grads[s.x] if grads is not None else None
        terms[k] = _lib.LossTerm(fptr(x).value + 4 * lo * per, None if y is None else fptr(y).value + 4 * s.y_lo * per,
                                 None if d is None else fptr(d).value + 4 * lo * per, rows * per, float(s.c),
                                 float(s.weight), int(s.mode), int(s.group))
    den = [float(s.den) for s in spec if s.den is not None]
    if den and len(den) != nt:
        raise ValueError("a denominator for every term or for none")
    return terms, (ctypes.c_double * nt)(*den) if den else None


_ENTRY = {("fwd", False): "mg_multi_loss_fwd", ("fwd", True): "mg_multi_loss_fwd_den",
          ("bwd", False): "mg_multi_loss_bwd", ("bwd", True): "mg_multi_loss_bwd_den"}


def _launch_means(which, table, *args):
    """The plain entry point, or the _den one when the table carries denominators: the one place that chooses."""
    terms, den = table
    fn = getattr(_lib.lib(), _ENTRY[which, den is not None])
    check(fn(terms, len(terms), *(() if den is None else (den,)), *args, stream_ptr()))


class _MeansFn(torch.autograd.Function):
    """total = sum_k weight_k * mean_k in ONE launch (mg_multi_loss_fwd), gradients of all terms in one more.
    spec: tuple of _Term over `tensors` -- MSE = mean (x - c)^2, L1 = mean |x - y| with gradient to x only, HINGE = mean
    max(0, 1 + c x), MEAN = mean x, each over rows [lo, hi) of its x.  Returns the [1 + groups + nterms] result vector
    (total, group subtotals, per-term means); differentiate [0].
    The trainer runs D(fake) and D(real) as one pass over 2B items; slicing the maps apart for the losses made autograd
    rebuild every map's gradient from two zero-padded halves (a fill, a copy and an add per half and map: ~55 launches per
    step).  Here the maps go in whole and the terms name their rows: a tensor that one term writes over all of its rows
    gets an empty gradient buffer, every other one a view into ONE zero-filled flat buffer (rows no term writes: zero).
    No two terms may write the same rows."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        nt = len(spec)
        if nt < 1 or nt > _lib.MG_LOSS_MAX_TERMS:
            raise ValueError("1..%d terms per call" % _lib.MG_LOSS_MAX_TERMS)
        ts = [t.contiguous() for t in tensors]
        table = _loss_table(spec, ts)            # refuses a tensor off the GPU before anything is allocated there
        dev = ts[0].device
        out = torch.empty(1 + _lib.MG_LOSS_GROUPS + nt, device=dev, dtype=torch.float32)
        _launch_means("fwd", table, fptr(_multi_scratch(dev)), fptr(out))
        ctx.spec = spec
        ctx.save_for_backward(*ts)
        return out

    @staticmethod
    def backward(ctx, g):
        spec, ts = ctx.spec, ctx.saved_tensors
        writers = [[] for _ in ts]
        for s in spec:
            if ctx.needs_input_grad[1 + s.x]:
                writers[s.x].append(s)
        whole = [len(w) == 1 and (w[0].hi is None or (w[0].lo == 0 and w[0].hi == t.shape[0]))
                 for w, t in zip(writers, ts)]
        sizes = [t.numel() if w and not wh else 0 for w, wh, t in zip(writers, whole, ts)]
        flat = torch.zeros(sum(sizes), device=ts[0].device, dtype=torch.float32) if any(sizes) else None
        grads, at = [], 0
        for w, wh, n, t in zip(writers, whole, sizes, ts):
            grads.append(None if not w else torch.empty_like(t) if wh else flat[at:at + n].view_as(t))
            at += n
        # only the total (element 0) is a loss; the subtotals and means are read-outs of the same numbers
        _launch_means("bwd", _loss_table(spec, ts, grads), fptr(g[:1].contiguous()))
        return (None, *grads)


_KINDS = {"mse": _lib.MG_LOSSMODE_MSE, "l1": _lib.MG_LOSSMODE_L1, "hinge": _lib.MG_LOSSMODE_HINGE,
          "mean": _lib.MG_LOSSMODE_MEAN}


def weighted_means(terms):
    """terms: list of ("mse", x, c, weight[, group]) / ("l1", x, y, weight[, group]) / ("hinge", x, sign, weight[, group])
    = weight * mean(max(0, 1 + sign * x)) / ("mean", x, None, weight[, group]).  Returns the result vector of
    _MeansFn: [0] total (differentiable w.r.t. every x), [1:1+4] group subtotals, then per-term means."""
    spec, ys = [], []
    for k, t in enumerate(terms):
        kind, x, other, w = t[:4]
        if kind not in _KINDS:
            raise ValueError(kind)
        l1 = kind == "l1"
        spec.append(_Term(_KINDS[kind], 0.0 if l1 or other is None else float(other), float(w),
                          t[4] if len(t) > 4 else 0, k, y=len(terms) + len(ys) if l1 else None))
        if l1:
            ys.append(other)
    return _MeansFn.apply(tuple(spec), *[t[1] for t in terms], *ys)


# --------------------------------------------------------------------------------------------------
# HiFi-GAN's GAN terms (Kong et al. 2020: discriminator_loss, generator_loss, feature_loss) over the outputs of
# discriminators with the published calling convention (vocoder_train.VocoderGANTrainer).
# --------------------------------------------------------------------------------------------------
def _means_in_calls(terms):
    """weighted_means over any number of terms, MG_LOSS_MAX_TERMS per launch: (total, [detached per-term means])."""
    total, means = None, []
    for at in range(0, len(terms), _lib.MG_LOSS_MAX_TERMS):
        part = terms[at:at + _lib.MG_LOSS_MAX_TERMS]
        out = weighted_means(part)
        total = out[0] if total is None else total + out[0]
        means.extend(out.detach()[1 + _lib.MG_LOSS_GROUPS:1 + _lib.MG_LOSS_GROUPS + len(part)].unbind(0))
    return total, means


def hifigan_discriminator_loss(disc_real, disc_gen):
    """sum over the discriminators of mean((1 - dr)^2) + mean(dg^2).  Returns (total, r_losses, g_losses); the lists
    hold device scalars (upstream's hold host floats)."""
    if len(disc_real) != len(disc_gen) or not disc_real:
        raise ValueError("one real and one generated output per discriminator")
    terms = []
    for dr, dg in zip(disc_real, disc_gen):
        terms += [("mse", dr, 1.0, 1.0), ("mse", dg, 0.0, 1.0)]
    total, means = _means_in_calls(terms)
    return total, means[0::2], means[1::2]


def hifigan_generator_loss(disc_gen):
    """sum of mean((1 - dg)^2).  Returns (total, gen_losses)."""
    if not disc_gen:
        raise ValueError("no discriminator outputs")
    return _means_in_calls([("mse", dg, 1.0, 1.0) for dg in disc_gen])


def hifigan_feature_loss(fmap_r, fmap_g):
    """2 sum over the discriminators and their maps of mean|fr - fg|, the real maps as targets (gradient to fmap_g)."""
    terms = [("l1", g, r, 2.0) for dr, dg in zip(fmap_r, fmap_g) for r, g in zip(dr, dg)]
    if not terms:
        raise ValueError("no feature maps")
    return _means_in_calls(terms)[0]


# --------------------------------------------------------------------------------------------------
# MelGAN's objective (Kumar et al. 2019, scripts/train.py) over melgan_discriminators.Discriminator's outputs: one list of
# maps per scale, the last map the raw logits.
# --------------------------------------------------------------------------------------------------
def melgan_discriminator_loss(D_real, D_fake):
    """sum over the scales of mean(relu(1 - real[-1])) + mean(relu(1 + fake[-1]))."""
    if len(D_real) != len(D_fake) or not D_real:
        raise ValueError("one real and one generated list of maps per scale")
    terms = []
    for r, f in zip(D_real, D_fake):
        terms += [("hinge", r[-1], -1.0, 1.0), ("hinge", f[-1], 1.0, 1.0)]
    return _means_in_calls(terms)[0]


def melgan_generator_loss(D_fake):
    """sum over the scales of -mean(fake[-1])."""
    if not D_fake:
        raise ValueError("no discriminator outputs")
    return _means_in_calls([("mean", f[-1], None, -1.0) for f in D_fake])[0]


def melgan_feature_loss(D_real, D_fake):
    """sum over the scales and over every map but the last of wt * mean|fake - real.detach()|,
    wt = (1 / num_D) * 4 / (n_layers + 1), n_layers + 3 maps per scale."""
    if len(D_real) != len(D_fake) or not D_real:
        raise ValueError("one real and one generated list of maps per scale")
    terms = []
    for r, f in zip(D_real, D_fake):
        if len(r) != len(f) or len(f) < 4:
            raise ValueError("a scale returns n_layers + 3 maps")
        wt = (1.0 / len(D_fake)) * 4.0 / (len(f) - 2)
        terms += [("l1", fm, rm, wt) for rm, fm in zip(r[:-1], f[:-1])]
    return _means_in_calls(terms)[0]


def _range_means(spec, tensors, den=None):
    """_MeansFn over BATCH RANGES of whole feature maps.  spec entries (tensor index, mode, c, weight, group, a_lo, a_hi,
    b_lo): the term reads rows [a_lo, a_hi) of its tensor, L1 against rows [b_lo, b_lo + a_hi - a_lo) of the same tensor.
    den: one host denominator per term (mg_multi_loss_fwd_den); None = each term's own element count (a mean)."""
    if den is not None and len(den) != len(spec):
        raise ValueError("one denominator per term: %d for %d terms" % (len(den), len(spec)))
    return _MeansFn.apply(tuple(
        _Term(mode, c, w, grp, ti, a_lo, a_hi, ti if mode == _lib.MG_LOSSMODE_L1 else None, b_lo,
              None if den is None else den[k])
        for k, (ti, mode, c, w, grp, a_lo, a_hi, b_lo) in enumerate(spec)), *tensors)


def _global_den(spec, tensors, B, n_total):
    """The denominators of the whole batch for terms that each cover B of its n_total items: the term's element count
    per item times n_total."""
    if n_total is None:
        return None
    return [tensors[e[0]][0].numel() * (e[6] - e[5]) // B * n_total for e in spec]


def d_loss_total_2b(logit_cond, logit_uncond, B, n_total=None):
    """d_loss_total on the last maps of ONE discriminator pass over [fake (rows 0..B-1); real (rows B..2B-1)].
    n_total: the item count of the whole batch when these B items are one rank's shard of it -- every mean then divides
    by the whole batch's element count (the maps of all ranks have the same length), and the result is the rank's share."""
    MSE = _lib.MG_LOSSMODE_MSE
    spec = [(0, MSE, 1.0, 0.5, 0, B, 2 * B, 0), (1, MSE, 1.0, 0.5, 0, B, 2 * B, 0),
            (0, MSE, 0.0, 0.5, 1, 0, B, 0), (1, MSE, 0.0, 0.5, 1, 0, B, 0)]
    tensors = [logit_cond, logit_uncond]
    out = _range_means(spec, tensors, _global_den(spec, tensors, B, n_total))
    return out[0], out[1], out[2]


def g_adv_fm_total_2b(cond_maps, uncond_maps, B, lambda_fm, n_layers=5, n_total=None):
    """g_adv_fm_total on the maps of ONE discriminator pass over [fake; real]: LSGAN on the fake rows of the last maps,
    feature matching |fake - real| on the others (gradient to the fake rows only, as model/loss.py:221-227 with the real
    maps as targets).  n_total: as in d_loss_total_2b."""
    w = lambda_fm * (4.0 / (n_layers + 1)) * 0.5
    nm = len(cond_maps)
    tensors = list(cond_maps) + list(uncond_maps)
    MSE, L1 = _lib.MG_LOSSMODE_MSE, _lib.MG_LOSSMODE_L1
    spec = [(nm - 1, MSE, 1.0, 0.5, 0, 0, B, 0), (2 * nm - 1, MSE, 1.0, 0.5, 0, 0, B, 0)]
    for j in range(nm - 1):
        spec.append((j, L1, 0.0, w, 1, 0, B, B))
        spec.append((nm + j, L1, 0.0, w, 1, 0, B, B))
    out = _range_means(spec, tensors, _global_den(spec, tensors, B, n_total))
    return out[0], out[1], out[2]


def d_loss_total(r_logit_cond, r_logit_uncond, f_logit_cond, f_logit_uncond):
    """d_real + d_fake of get_lsgan_losses_fn()'s d_loss_fn (model/loss.py:12-30, train.py:142-143) as one fused sum.
    Returns (total, d_real, d_fake); differentiate total."""
    out = weighted_means([("mse", r_logit_cond, 1.0, 0.5, 0), ("mse", r_logit_uncond, 1.0, 0.5, 0),
                          ("mse", f_logit_cond, 0.0, 0.5, 1), ("mse", f_logit_uncond, 0.0, 0.5, 1)])
    return out[0], out[1], out[2]


def g_adv_fm_total(D_real_cond, D_real_uncond, D_fake_cond, D_fake_uncond, lambda_fm, n_layers=5):
    """adv + lambda_fm * fm of the generator loss (train.py:162-170: g_loss_fn on the last maps, get_fm_loss on the
    others) as one fused sum.  Returns (total, adv, lambda_fm * fm); differentiate total."""
    w = lambda_fm * (4.0 / (n_layers + 1)) * 0.5
    terms = [("mse", D_fake_cond[-1], 1.0, 0.5, 0), ("mse", D_fake_uncond[-1], 1.0, 0.5, 0)]
    for j in range(len(D_fake_cond) - 1):
        terms.append(("l1", D_fake_cond[j], D_real_cond[j], w, 1))
        terms.append(("l1", D_fake_uncond[j], D_real_uncond[j], w, 1))
    out = weighted_means(terms)
    return out[0], out[1], out[2]


def _jcu_loss(logit_cond, logit_uncond, label, mask=None):
    if mask is not None:
        raise NotImplementedError("train.py never passes a mask to the adversarial losses (train.py:142,162)")
    return 0.5 * (_MseConstFn.apply(logit_cond, label) + _MseConstFn.apply(logit_uncond, label))


def get_lsgan_losses_fn():
    """model/loss.py:12-30."""

    def d_loss_fn(r_logit_cond, r_logit_uncond, f_logit_cond, f_logit_uncond, mask=None):
        return _jcu_loss(r_logit_cond, r_logit_uncond, 1.0, mask), _jcu_loss(f_logit_cond, f_logit_uncond, 0.0, mask)

    def g_loss_fn(f_logit_cond, f_logit_uncond, mask=None):
        return _jcu_loss(f_logit_cond, f_logit_uncond, 1.0, mask)

    return d_loss_fn, g_loss_fn


def get_adversarial_losses_fn(mode):
    if mode == "lsgan":
        return get_lsgan_losses_fn()
    raise NotImplementedError(mode)


def get_fm_loss(D_real_cond, D_real_uncond, D_fake_cond, D_fake_uncond, n_layers=5):
    """model/loss.py:221-227 (unscaled by lambda_fm)."""
    w = 4.0 / (n_layers + 1)
    tot = 0
    for j in range(len(D_fake_cond) - 1):
        tot = tot + w * 0.5 * (_L1Fn.apply(D_fake_cond[j], D_real_cond[j]) + _L1Fn.apply(D_fake_uncond[j], D_real_uncond[j]))
    return tot


class _MelL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, pad, den=None):
        pred, target = pred.contiguous(), target.detach().contiguous()
        B, L, M = pred.shape
        pad8 = pad.to(torch.uint8).contiguous()
        out = torch.empty(2, device=pred.device)
        check(_lib.lib().mg_mel_l1_fwd(fptr(pred), fptr(target), iptr(pad8, torch.uint8), B * L, M, fptr(out),
                                       stream_ptr()))
        if den is not None:      # the whole batch's M * counted rows: out[1] is this shard's
            out = torch.stack([out[0], den.detach().to(torch.float32).reshape(())])
        ctx.save_for_backward(pred, target, pad8, out)
        return out[0] / out[1]

    @staticmethod
    def backward(ctx, g):
        pred, target, pad8, out = ctx.saved_tensors
        B, L, M = pred.shape
        d = torch.empty_like(pred)
        check(_lib.lib().mg_mel_l1_bwd(fptr(pred), fptr(target), iptr(pad8, torch.uint8), B * L, M,
                                       fptr(g.reshape(1).contiguous()), fptr(out[1:2].contiguous()), fptr(d),
                                       stream_ptr()))
        return d, None, None, None


def get_mel_loss(mel_predictions, mel_targets, mel_masks_fill, den=None):
    """model/loss.py:229-242: masked_fill(pad, 0) on both, L1 weighted by non-zero target rows.
    mel_masks_fill: bool [B, L], True = pad.  den: a device scalar that replaces the denominator (M * the counted rows
    of THIS tensor) -- M * the counted rows of the whole batch (mel_count_rows, summed over the ranks) when the tensors
    are one rank's shard; both the value and the gradient divide by it, without a host read."""
    if den is None:
        return _MelL1Fn.apply(mel_predictions, mel_targets, mel_masks_fill)
    return _MelL1Fn.apply(mel_predictions, mel_targets, mel_masks_fill, den)


def mel_count_rows(mel_targets, mel_masks_fill, out=None):
    """The number of rows get_mel_loss counts in mel_targets [B, L, M] (unpadded, with a non-zero entry), as a
    one-element int64 device tensor (`out`, e.g. ShardCounts.slot("mel_rows"), or a new one)."""
    target = mel_targets.detach().contiguous()
    B, L, M = target.shape
    pad8 = mel_masks_fill.to(torch.uint8).contiguous() if mel_masks_fill is not None else None
    if out is None:
        out = torch.empty(1, dtype=torch.int64, device=target.device)
    check(_lib.lib().mg_mel_count_rows(fptr(target), iptr(pad8, torch.uint8, True), B * L, M, iptr(out, torch.int64),
                                       stream_ptr()))
    return out


# --------------------------------------------------------------------------------------------------
# the linguistic encoder's terms of recon_loss (model/loss.py:128-195): small masked means, a guided-attention mask
# and a CTC dynamic program -- device-side torch, vectorised over the batch (no per-utterance host loop).
# --------------------------------------------------------------------------------------------------
def guided_attention_loss(att, ilens, olens, sigma, alpha, den=None):
    """GuidedAttentionLoss (model/loss.py:261-352) on att [B, T_out, T_in]: alpha * mean over the valid (out, in)
    cells of att * (1 - exp(-(in/ilen - out/olen)^2 / (2 sigma^2))).  den: the number of valid cells of the whole
    batch (sum of ilen * olen) when att is one rank's shard: the sum over this shard's cells divided by it."""
    B, To, Ti = att.shape
    il = ilens.to(att.device, torch.float32)[:, None, None]
    ol = olens.to(att.device, torch.float32)[:, None, None]
    o = torch.arange(To, device=att.device, dtype=torch.float32)[None, :, None]
    i = torch.arange(Ti, device=att.device, dtype=torch.float32)[None, None, :]
    mask = (o < ol) & (i < il)
    g = 1.0 - torch.exp(-((i / il - o / ol) ** 2) / (2 * sigma ** 2))
    cells = (g * att).masked_select(mask)
    return alpha * (cells.mean() if den is None else cells.sum() / den)


def forward_sum_loss(attn_logprob, in_lens, out_lens, blank_logprob=-1.0, den=None):
    """ForwardSumLoss (model/loss.py:420-447) on attn_logprob [B, 1, T_out, T_in]: a blank column of `blank_logprob`
    in front, log_softmax over the first in_len + 1 columns, CTC against 1..in_len (zero_infinity, mean over the
    target length), then the batch mean.  Columns past in_len + 1 are filled with -1e4 rather than cut (one batched
    call): exp(-1e4 - max) is exactly 0 in fp32, so the value is the reference's, and unlike -inf the filler gives
    the CTC backward finite gradients there (at -inf it returns NaN, which the log_softmax backward would spread over
    the whole row).  The padded keys' -inf scores all lie in those columns.  den: the item count of the whole batch
    when these B items are one rank's shard (sum / den instead of the mean)."""
    B, _, To, Ti = attn_logprob.shape
    dev = attn_logprob.device
    il = in_lens.to(dev, torch.int64)
    ol = out_lens.to(dev, torch.int64)
    lp = torch.nn.functional.pad(attn_logprob[:, 0], (1, 0), value=blank_logprob)          # [B, To, Ti + 1]
    cols = torch.arange(Ti + 1, device=dev)
    lp = lp.masked_fill(cols[None, None, :] > il[:, None, None], -1e4)
    lp = torch.log_softmax(lp, -1).transpose(0, 1)                                       # [To, B, Ti + 1]
    targets = (torch.arange(1, Ti + 1, device=dev)[None, :].expand(B, Ti) * (cols[None, 1:] <= il[:, None]))
    per = torch.nn.functional.ctc_loss(lp, targets, ol, il, blank=0, reduction="none", zero_infinity=True)
    per = per / il.clamp(min=1).to(per.dtype)
    return per.mean() if den is None else per.sum() / den


class LinguisticEncoderLoss:
    """model/loss.py:128-195's linguistic-encoder terms: lambda_d * duration + lambda_p * pitch + lambda_e * energy +
    helper (dga: guided attention on alignments[1], one term per head; ctc: the forward-sum loss per head, weight
    switched at ctc_step).  Zero for `shallow`.  Callable as `upstream_loss(batch, output, step)` of
    HotPathTrainer.step_from_model; `terms(...)` returns every term for logging, and the last call's terms stay in
    `self.last`."""

    def __init__(self, preprocess_config, model_config, train_config, model="naive"):
        for lvl in (preprocess_config["preprocessing"]["pitch"]["feature"],
                    preprocess_config["preprocessing"]["energy"]["feature"]):
            if lvl != "phoneme_level":
                raise NotImplementedError("LinguisticEncoderLoss: phoneme_level pitch / energy only")
        self.model = model
        lc = train_config["loss"]
        self.lambda_d, self.lambda_p, self.lambda_e = lc["lambda_d"], lc["lambda_p"], lc["lambda_e"]
        al = train_config["aligner"]
        self.helper_type = al["helper_type"]
        if self.helper_type == "dga":
            self.guided_sigma, self.guided_lambda = al["guided_sigma"], al["guided_lambda"]
            self.guided_weight = al["guided_weight"]
        elif self.helper_type == "ctc":
            self.ctc_step = train_config["step"]["ctc_step"]
            self.ctc_weight_start, self.ctc_weight_end = al["ctc_weight_start"], al["ctc_weight_end"]
        self.last = None

    @staticmethod
    def local_counts(output):
        """This shard's data-dependent denominators, as 0-dim int64 tensors: what goes into distributed.ShardCounts
        (slots "words", "phonemes", "attn_cells") before its all-reduce."""
        src_masks, src_lens, mel_lens, src_w_masks = output[8], output[10], output[11], output[14]
        return {"words": src_w_masks.sum(), "phonemes": src_masks.sum(),
                "attn_cells": (src_lens.to(torch.int64) * mel_lens.to(torch.int64).to(src_lens.device)).sum()}

    def terms(self, batch, output, step, counts=None):
        """batch: the reference's batch list (pitch / energy targets at 14 / 15); output: MixGANTTS.forward's 16 slots.
        counts: the denominators of the WHOLE batch when `batch` is one rank's shard of it -- a mapping (a
        distributed.ShardCounts after its all-reduce, or a dict) with "n_items", "words", "phonemes" and "attn_cells"
        (the sum of ilen * olen).  Every masked mean then becomes masked sum / global count, the CTC batch mean sum / N,
        and the returned terms are this rank's SHARES: summed over the ranks they are `terms` on the whole batch."""
        p_pred, e_pred, logd_pred, d_rounded = output[4], output[5], output[6], output[7]
        src_masks, src_lens, mel_lens = output[8], output[10], output[11]
        alignments, logprobs, src_w_masks = output[12], output[13], output[14]
        dev = logd_pred.device
        zero = torch.zeros((), device=dev)
        t = {"duration_loss": zero, "pitch_loss": zero, "energy_loss": zero, "helper_loss": zero}
        if self.model != "shallow":
            if counts is None:
                mse = lambda a, b, key: torch.nn.functional.mse_loss(a, b)  # noqa: E731
            else:
                mse = lambda a, b, key: (a - b).pow(2).sum() / counts[key]  # noqa: E731
            ga_den = None if counts is None else counts["attn_cells"]
            n_items = None if counts is None else counts["n_items"]
            logd_tgt = torch.log(d_rounded.to(logd_pred.dtype) + 1)
            t["duration_loss"] = mse(logd_pred.masked_select(src_w_masks), logd_tgt.masked_select(src_w_masks),
                                     "words")
            t["pitch_loss"] = mse(p_pred.masked_select(src_masks), batch[14].to(dev).masked_select(src_masks),
                                  "phonemes")
            t["energy_loss"] = mse(e_pred.masked_select(src_masks), batch[15].to(dev).masked_select(src_masks),
                                   "phonemes")
            if self.helper_type == "dga":
                attn = sum(guided_attention_loss(a, src_lens, mel_lens, self.guided_sigma, self.guided_lambda, ga_den)
                           for a in alignments[1])
                t["attn_loss"] = attn
                t["helper_loss"] = self.guided_weight * attn
            elif self.helper_type == "ctc":
                ctc = sum(forward_sum_loss(lp, src_lens, mel_lens, den=n_items) for lp in logprobs)
                t["ctc_loss"] = ctc
                w = self.ctc_weight_start if step <= self.ctc_step else self.ctc_weight_end
                t["helper_loss"] = w * ctc
        t["total"] = (self.lambda_d * t["duration_loss"] + self.lambda_p * t["pitch_loss"] +
                      self.lambda_e * t["energy_loss"] + t["helper_loss"])
        return t

    def __call__(self, batch, output, step, counts=None):
        t = self.terms(batch, output, step, counts)
        self.last = {k: v.detach() for k, v in t.items()}
        return t["total"]
