"""Plain torch restatements of the small diffusion, step-MLP, loss and index operations (include/mixgan_hip.h:
elementwise.hip, misc_api.hip, the small_* kernels, the scalar part of losses.hip, lingops.hip), and the input sets of
tests/test_gpu_small_ops.py.  Every function follows the dtype of what it is given, so one body serves as the float64
reference and as the float32 restatement whose own error feeds helpers.bar_for.  Gradients are torch.autograd through
these functions (grads()); no gradient formula is written down a second time.  tests/test_small_ops_cpu.py pins the
restatements to torch's own operators and to oracle/refmath.py, and checks every input set below for the kink margin,
the float32 restatement's error and the share of redrawn elements, with no GPU involved."""
import numpy as np
import torch
import torch.nn.functional as F

from helpers import rel_err
from oracle import refmath as R

KINK_BAND = 1e-4        # "away from a kink": farther than this share of the tensor's max-abs (hifigan_disc_ref.kink_masks)
KINK_SHARE = 1e-3       # at most this share of a tensor may be redrawn to get there
BAR_MOVE, BAR_ELEM, BAR_RED, BAR_DGRAD, BAR_WGRAD = 0.0, 2e-6, 2e-5, 5e-5, 1e-4
T_STEPS = 4


def gen(seed):
    return torch.Generator().manual_seed(seed)


def as_dtype(x, dtype):
    """Tensors (and containers of them) widened / narrowed to `dtype`; integer and bool tensors pass through."""
    if isinstance(x, torch.Tensor):
        return x.to(dtype) if x.is_floating_point() else x
    if isinstance(x, dict):
        return {k: as_dtype(v, dtype) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(as_dtype(v, dtype) for v in x)
    return x


def grads(fn, inputs, cots, dtype=torch.float64):
    """d sum_i <fn(*inputs)_i, cots_i> / d inputs by autograd, everything in `dtype`.  A None cotangent leaves that
    output out of the sum."""
    leaves = [x.detach().to(dtype).requires_grad_() for x in inputs]
    outs = fn(*leaves)
    if isinstance(outs, torch.Tensor):
        outs = (outs,)
    loss = sum((o * c.to(dtype)).sum() for o, c in zip(outs, cots) if c is not None)
    return torch.autograd.grad(loss, leaves, allow_unused=True)


# ------------------------------------------------------------------------------------------------ comparison
def tile_errors(got, ref, dim, block):
    """(max-abs error, max-abs reference) of every `block`-wide slice along `dim`, the last partial one included."""
    d = (got.detach().cpu().double() - ref.double()).abs().movedim(dim, -1)
    r = ref.double().abs().movedim(dim, -1)
    pad = (-d.shape[-1]) % block
    d, r = F.pad(d, (0, pad)), F.pad(r, (0, pad))
    nt = d.shape[-1] // block
    return d.reshape(-1, nt, block).amax((0, 2)), r.reshape(-1, nt, block).amax((0, 2))


WORST = {}      # group -> (worst error / bar ratio, error, bar, what): the rows of the table in DESIGN.md


def _note(group, e, bar, what):
    if group is not None and (group not in WORST or e / bar > WORST[group][0]):
        WORST[group] = (e / bar, e, bar, what)


def check(got, ref32, ref64, bar, what, dim=None, block=64, group=None):
    """The project's measure (max-abs error / max-abs reference, helpers.assert_close) under the project's fallback rule
    (helpers.bar_for: 8 x the float32 restatement's own error where that exceeds bar / 8), on the whole tensor and then,
    with `dim`, on every `block`-wide slice along it against that slice's own reference maximum.  Prints what it
    measured before it asserts."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), what + ": non-finite values"
    e32 = rel_err(ref32.detach().double().numpy(), ref64.numpy())
    b = bar if e32 <= bar / 8 else 8 * e32
    e = rel_err(got.double().numpy(), ref64.numpy())
    line = "%-58s err %.3e  bar %.1e" % (what, e, b)
    worst_tile = None
    if dim is not None and got.numel():
        d, r = tile_errors(got, ref64, dim, block)
        d32, _ = tile_errors(ref32, ref64, dim, block)
        et, e32t = d / (r + 1e-30), d32 / (r + 1e-30)
        bt = torch.where(e32t <= bar / 8, torch.full_like(et, bar), 8 * e32t)
        k = int((et / bt).argmax())
        worst_tile = (k, float(et[k]), float(bt[k]))
        line += "  worst %d-block %d of %d: err %.3e  bar %.1e" % (block, k, len(et), worst_tile[1], worst_tile[2])
    print(line)
    _note(group, e, b, what)
    assert e <= b, "%s: max-abs err / max-abs ref = %.3e > %.1e" % (what, e, b)
    if worst_tile is not None:
        _note(group, worst_tile[1], worst_tile[2], what + " (block)")
        assert worst_tile[1] <= worst_tile[2], "%s: %d-block %d along dim %d: err %.3e > %.1e" % (
            what, block, worst_tile[0], dim, worst_tile[1], worst_tile[2])


def check_equal(got, ref, what, group=None):
    got = got.detach().cpu()
    same = got.shape == ref.shape and torch.equal(got, ref)
    print("%-58s %s" % (what, "bit-equal" if same else "DIFFERS"))
    _note(group, 0.0, 1.0, what)
    assert same, what + ": not bit-equal"


# ------------------------------------------------------------------------------------------------ kinks
def away_from(x, kinks, g, on=0, scale=None):
    """In place: every element of x within KINK_BAND * max|x| (or * scale) of a value in `kinks` is drawn again until
    none is; then the first `on` elements per kink value, at scattered places, are set exactly ON it.  Returns the
    number of elements redrawn (the ones set on a kink are placed on purpose and not counted)."""
    flat = x.view(-1)
    redrawn = 0
    while True:
        band = KINK_BAND * float(x.abs().max() if scale is None else scale)
        bad = torch.zeros_like(flat, dtype=torch.bool)
        for k in kinks:
            bad |= (flat.double() - k).abs() <= band
        n = int(bad.sum())
        if n == 0:
            break
        redrawn += n
        flat[bad] = torch.randn(n, generator=g) * float(flat.std() if flat.numel() > 1 else 1.0)
    if on:
        idx = torch.randperm(flat.numel(), generator=g)[: on * len(kinks)]
        for j, k in enumerate(kinks):
            flat[idx[j * on:(j + 1) * on]] = k
    return redrawn


def kink_report(x, kinks, scale=None):
    """(elements exactly on a kink, smallest distance of the others from any kink / max|x| (or / scale)).  The distance
    is taken in float64 on the float32 values."""
    v = x.detach().double().reshape(-1)
    dist = torch.full_like(v, float("inf"))
    for k in kinks:
        dist = torch.minimum(dist, (v - k).abs())
    on = dist == 0
    rest = dist[~on]
    m = float(x.abs().max() if scale is None else scale)
    return int(on.sum()), (float(rest.min()) / m if rest.numel() else float("inf"))


# ------------------------------------------------------------------------------------------------ schedule and masks
def spec(M):
    """Per-channel spec_min / spec_max that all differ."""
    return torch.linspace(-11.5, -9.0, M) - 0.01 * torch.arange(M) % 0.07, torch.linspace(1.0, 2.0, M) + 0.003 * torch.arange(M)


def schedule(T=T_STEPS, M=80):
    """The float32 buffers of GaussianDiffusion (vpsde) plus spec_min / spec_max, as CPU tensors."""
    import mixgan_tts_amd as mg
    buf = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in
           mg.diffusion_buffers(mg.beta_schedule("vpsde", T, 0.1, 40, 0.008)).items()}
    buf["spec_min"], buf["spec_max"] = spec(M)
    return buf


def keep_mask(B, L, seed=0, zero_row=False):
    """uint8 [B, L], 1 = valid: zeros in the middle and at the end of rows; with zero_row the last row is all zero."""
    k = torch.ones(B, L, dtype=torch.uint8)
    if L >= 2:
        k[:, L - max(1, L // 4):] = 0
    if L >= 3:
        k[:, L // 2] = 0
    if B > 1:
        k[1] = (torch.rand(L, generator=gen(seed)) > 0.3).to(torch.uint8)
        if L >= 2:
            k[1, -1] = 0
    if zero_row or (L == 1 and B > 1):
        k[-1] = 0
    return k


# ------------------------------------------------------------------------------------------------ restatements
norm_spec, denorm_spec, mish, step_embedding = R.norm_spec, R.denorm_spec, R.mish, R.step_embedding


def transpose(x, to_blm, mode, spec_min=None, spec_max=None, keep=None):
    """mg_transpose_bml: [B,M,L] -> [B,L,M] (mode 2: denorm_spec on the way out) or [B,L,M] -> [B,M,L] (mode 1:
    norm_spec on the way in), times keep [B,L]."""
    if to_blm:
        y = x.transpose(1, 2)
        if mode == 2:
            y = denorm_spec(y, spec_min.to(x.dtype), spec_max.to(x.dtype))
        if keep is not None:
            y = y * keep[:, :, None].to(x.dtype)
    else:
        y = norm_spec(x, spec_min.to(x.dtype), spec_max.to(x.dtype)) if mode == 1 else x
        y = y.transpose(1, 2)
        if keep is not None:
            y = y * keep[:, None, :].to(x.dtype)
    return y.contiguous()


def diffuse_fn(buf, mel, t, noise, keep=None):
    """mg_diffuse_fwd on refmath.diffuse_fn: mel [B,L,M], noise [B,M,L] -> [B,M,L]; t < 0 gives the clean normalised mel,
    t >= T is clamped to T - 1; times keep."""
    b = as_dtype(buf, mel.dtype)
    T = b["sqrt_alphas_cumprod"].numel()
    out = R.diffuse_fn(b, mel, t.clamp(max=T - 1), noise[:, None])[:, 0]
    return out if keep is None else out * keep[:, None, :].to(mel.dtype)


def q_posterior_sample(buf, x0, x_t, t, noise, keep=None, clip=True):
    """mg_posterior_sample_fwd on refmath.q_posterior_sample: (x0 clamped, x_{t-1}), all [B,M,L]; t clamped to
    [0, T - 1]."""
    b = as_dtype(buf, x0.dtype)
    T = b["posterior_mean_coef1"].numel()
    k = 1 if keep is None else keep[:, None, :].to(x0.dtype)
    x0c = x0 * k
    if clip:
        x0c = x0c.clamp(-1.0, 1.0)
    out = R.q_posterior_sample(b, x0c[:, None], x_t[:, None], t.clamp(0, T - 1), noise[:, None])[:, 0]
    return x0c, out * k


def diffuse_trace(buf, x_start, keep, noises):
    """refmath.diffuse_trace stacked: [T+1, B, L, M]; keep uint8 [B, L] or None; noises: T tensors [B,1,M,L]."""
    b = as_dtype(buf, x_start.dtype)
    B, L, _ = x_start.shape
    mask = torch.zeros(B, L, dtype=torch.bool) if keep is None else keep == 0
    it = iter(noises)
    return torch.stack(R.diffuse_trace(b, x_start, mask, len(noises), lambda shape: next(it).to(x_start.dtype)))


def spec_affine(x, spec_min, spec_max, mode):
    """mg_spec_affine: 1 norm_spec, 2 denorm_spec, 3 / 4 their gradients (by autograd) for the cotangent x."""
    mn, mx = spec_min.to(x.dtype), spec_max.to(x.dtype)
    if mode in (1, 2):
        return (norm_spec if mode == 1 else denorm_spec)(x, mn, mx)
    f = norm_spec if mode == 3 else denorm_spec
    return grads(lambda a: f(a, mn, mx), [torch.zeros_like(x)], [x], x.dtype)[0]


def act(x, name):
    return {"relu": F.relu, "lrelu": lambda v: F.leaky_relu(v, 0.2), "tanh": torch.tanh, "none": lambda v: v}[name](x)


def gate(z):
    """sigmoid(z[:, :C]) * tanh(z[:, C:]) (model/blocks.py:1170-1171)."""
    C = z.shape[1] // 2
    return torch.sigmoid(z[:, :C]) * torch.tanh(z[:, C:])


def upsample_zero(x, s, Lup, slope=1.0):
    """mg_upsample_zero_act: out[..., q s] = leaky_relu(x[..., q], slope) for q s < Lup, zeros elsewhere."""
    y = x if slope == 1.0 else F.leaky_relu(x, slope)
    out = x.new_zeros(*x.shape[:-1], Lup)
    n = min(x.shape[-1], (Lup + s - 1) // s)
    out[..., 0:(n - 1) * s + 1:s] = y[..., :n]
    return out


def loss_sum(a, b, c, mode):
    """mg_loss_sum: mode 0 sum (a - c)^2, mode 1 sum |a - b|."""
    return ((a - c) ** 2).sum() if mode == 0 else (a - b).abs().sum()


def mel_l1_terms(pred, target, pad):
    """(numerator, denominator) of refmath.mel_l1: what mg_mel_l1_fwd writes."""
    p = pred.masked_fill(pad.unsqueeze(-1), 0)
    t = target.masked_fill(pad.unsqueeze(-1), 0)
    w = t.abs().sum(-1, keepdim=True).ne(0).to(pred.dtype).repeat(1, 1, target.size(-1))
    return ((p - t).abs() * w).sum(), w.sum()


def linear(x, W):
    return x @ W.t()


def step_mlp(t, W0, W2):
    """out = W2 mish(W0 emb(t)), emb the fp32-rounded step embedding widened to the weights' dtype."""
    emb = step_embedding(t, W0.shape[1], W0.dtype)
    pre = linear(emb, W0)
    h = mish(pre)
    return linear(h, W2), emb, pre, h


def frequencies(D):
    import mixgan_tts_amd as mg
    return mg.blocks.DiffusionEmbedding(D).frequencies()


word_level_pooling, length_regulate, mapping_mask, rel_coef = R.word_level_pooling, R.length_regulate, R.mapping_mask, R.rel_coef


# ------------------------------------------------------------------------------------------------ input sets
TRANSPOSE_L = (1, 3, 4, 63, 64, 65, 130, 260)
TRANSPOSE_M = (1, 3, 4, 80, 81)
TRANSPOSE_B = (1, 3)


def transpose_inputs(B, L, M, to_blm, seed=0):
    """x in the source layout; for mode 2 it is a normalised mel (about +-1.5), for mode 1 a mel between the stats."""
    g = gen(1000 * L + 10 * M + B + seed)
    if to_blm:
        return torch.randn(B, M, L, generator=g)
    mn, mx = spec(M)
    return mn + (mx - mn) * (0.5 + 0.4 * torch.randn(B, L, M, generator=g))


# (L, M, what a 1-float storage offset is applied to): vector form needs L % 4 == M % 4 == 0 and aligned bases
DIFFUSE_CASES = [(1, 80, None), (63, 80, None), (64, 80, None), (65, 80, None), (132, 80, None), (64, 81, None),
                 (64, 3, None), (132, 4, None), (64, 80, "mel"), (64, 80, "noise")]
DIFFUSE_T = (-1, 0, T_STEPS - 1, T_STEPS, T_STEPS + 5)


def diffuse_inputs(L, M):
    g = gen(77 * L + M)
    B = len(DIFFUSE_T)
    mn, mx = spec(M)
    mel = mn + (mx - mn) * (0.5 + 0.4 * torch.randn(B, L, M, generator=g))
    return mel, torch.tensor(DIFFUSE_T), torch.randn(B, M, L, generator=g)


# (M, L, storage offset): 80 x 1639 = 131 120 scalars and 80 x 6556 / 4 = 131 120 vectors are just past the 512 x 256 cap
POSTERIOR_CASES = [(3, 5, 0), (4, 8, 0), (4, 8, 1), (80, 1639, 0), (80, 6556, 0)]
POSTERIOR_T = (0, 1, T_STEPS - 1, T_STEPS + 3)


def posterior_inputs(M, L):
    """x0 (about 1.5 sigma, so a third clamps) whose kept part is either exactly on -1 / +1 or farther than the band
    from them; x_t, two noises, keep with an all-zero last row, and the number of elements redrawn."""
    g = gen(31 * M + L)
    B = len(POSTERIOR_T)
    x0 = torch.randn(B, M, L, generator=g) * 1.5
    redrawn = away_from(x0, (-1.0, 1.0), g, on=max(1, min(40, x0.numel() // 8)))
    x_t, nz, nz2 = (torch.randn(B, M, L, generator=g) for _ in range(3))
    keep = keep_mask(B, L, seed=L, zero_row=False)
    keep[2] = 0                                        # an all-zero row (not the t = 0 one)
    return dict(x0=x0, x_t=x_t, noise=nz, noise2=nz2, t=torch.tensor(POSTERIOR_T), keep=keep, redrawn=redrawn,
                g_x0c=torch.randn(B, M, L, generator=g), g_xpp=torch.randn(B, M, L, generator=g))


CAP_ACT, CAP_AFFINE, CAP_GATE, CAP_MISH, CAP_UPS, CAP_TRACE = 524288, 524288, 1048576, 1048576, 2097152, 1048576
CAP_LOSS_SUM, CAP_LOSS_GRAD = 262144, 524288
ACT_N = (200, CAP_ACT + 300)
AFFINE_ROWS = (3, 6554)                              # x 80: 240 and 524 320
GATE_SHAPES = ((1, 3, 5), (2, 255, 2057))            # 15 and 1 049 070 (with C = 256 every n is a multiple of 256)
MISH_N = (100, CAP_MISH + 300)
UPS_CASES = [(6, 7, 3, 19), (6, 7, 3, 15), (6, 7, 3, 25), (5, 1, 4, 1), (8, 66000, 4, 263997)]   # rows, Lin, s, Lup
TRACE_SHAPES = ((1, 3, 80), (2, 6556, 80))           # 240 and 1 048 960
LOSS_N = (200, CAP_LOSS_GRAD + 300)
MEL_CASES = [(7, 1171, 80), (7, 1171, 1), (7, 1171, 65), (2, 3, 80)]   # 8197 rows: past 2048 (forward) and 8192 (backward)


def act_inputs(n, name):
    """(pre-activation, dy); relu / lrelu: pre is exactly 0 at 16 places and farther than the band from 0 elsewhere."""
    g = gen(n + len(name))
    pre, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    redrawn = away_from(pre, (0.0,), g, on=16) if name != "none" else 0
    return pre, dy, redrawn


def trace_inputs(B, L, M):
    """x_start whose normalised value is exactly +-1 at 32 places (x = spec_max / spec_min there) and farther than the
    band from +-1 elsewhere; about a fifth lies outside [-1, 1]."""
    g = gen(B * L + M)
    mn, mx = spec(M)
    x = mn + (mx - mn) * (0.5 + 0.4 * torch.randn(B, L, M, generator=g))
    redrawn = 0
    while True:
        nv = norm_spec(x.double(), mn.double(), mx.double())
        bad = ((nv.abs() - 1).abs() <= KINK_BAND * float(nv.abs().max()))
        n = int(bad.sum())
        if n == 0:
            break
        redrawn += n
        fresh = mn + (mx - mn) * (0.5 + 0.4 * torch.randn(B, L, M, generator=g))
        x = torch.where(bad, fresh, x)
    idx = torch.randperm(B * L, generator=g)[:32]
    for j, r in enumerate(idx.tolist()):
        m = j % M
        x.view(-1, M)[r, m] = (mx if j % 2 else mn)[m]
    return dict(x=x, g=torch.randn(T_STEPS + 1, B, L, M, generator=g), keep=keep_mask(B, L, seed=M), redrawn=redrawn,
                noises=[torch.randn(B, 1, M, L, generator=g) for _ in range(T_STEPS)])


def loss_inputs(n):
    """a, b with 16 exact ties and every other |a - b| farther than the band from 0."""
    g = gen(n)
    a, d = torch.randn(n, generator=g), torch.randn(n, generator=g)
    redrawn = away_from(d, (0.0,), g, on=16)
    b = a - d
    tie = d == 0
    # a - b must round back onto the side d is on, and onto exactly 0 at the ties
    assert bool(((a - b) == 0)[tie].all()) and bool((torch.sign(a - b) == torch.sign(d)).all())
    return a, b, redrawn


def mel_inputs(B, L, M):
    """pred, target, pad (True = padded): padded rows keep non-zero data, one unpadded target row is all zero, 16
    exact ties pred == target, every other difference farther than the band from 0."""
    g = gen(B * L * M)
    target, d = torch.randn(B, L, M, generator=g), torch.randn(B, L, M, generator=g)
    redrawn = away_from(d, (0.0,), g, on=min(16, d.numel() // 4))
    pad = torch.arange(L)[None, :] >= torch.randint(L // 2, L + 1, (B, 1), generator=g)
    pad[0, L // 3] = True                               # a padded row in the middle, data left in place
    target[-1, 0] = 0                                   # unpadded, all-zero target: not counted
    pad[-1, 0] = False
    pred = target + d
    pred[-1, 0] = torch.randn(M, generator=g) + 3.0
    return pred, target, pad, redrawn


LIN_B, LIN_N, LIN_K = (1, 8, 9), (1, 5, 256), (1, 63, 64, 65, 256, 320, 512)
MLP_DIMS = ((256, 1024, 256), (6, 10, 3))
MLP_T = (0, 1, 99, 999)


def linear_inputs(B, N, K):
    g = gen(10000 * B + 100 * N + K)
    return (torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(B, N, generator=g))


def mlp_inputs(D0, D1, D2, B):
    g = gen(D0 + D1 + D2 + B)
    t = torch.tensor([MLP_T[i % len(MLP_T)] for i in range(B)])
    return (t, torch.randn(D1, D0, generator=g) / D0 ** 0.5, torch.randn(D2, D1, generator=g) / D1 ** 0.5,
            torch.randn(B, D2, generator=g))


# lingops: name -> dict(B, Tw, H, ...) (see lingops_inputs)
LING_CASES = {
    "ragged_h1": dict(B=3, Tw=9, H=1, seed=1),
    "ragged_h256": dict(B=3, Tw=9, H=256, seed=2),
    "ragged_h300": dict(B=4, Tw=12, H=300, seed=3),
    "limit_4096": dict(B=1, Tw=4096, H=4, seed=4),
}


def lingops_inputs(B, Tw, H, seed):
    """Ragged word / phoneme counts with zero and negative durations, one zero-length word inside a row, a src_w_len
    above Tw (clamped by both sides) and a row whose phoneme counts add up to more than Tp."""
    g = gen(seed)
    swl = torch.randint(max(1, Tw // 2), Tw + 1, (B,), generator=g)
    swl[0] = Tw
    if B > 1:
        swl[-1] = Tw + 3                                    # larger than Tw: both sides count Tw words
    wb =torch.randint(1, 4, (B, Tw), generator=g)
    dur = torch.randint(-1, 4, (B, Tw), generator=g)        # -1: clamped to 0 by the regulator, like the reference
    dur[:, 1 % Tw] = 0
    wb[0, 2 % Tw] = 0                                       # a zero-length word: NaN under reduce="mean"
    for b in range(B):
        wb[b, int(swl[b]):] = 0
    Tp = int(wb.sum(1).max())
    if B > 1:
        wb[1, 0] += Tp - int(wb[1].sum()) + 3               # sum(wb[1]) = Tp + 3: the last words run past the phonemes
    src = torch.randn(B, Tp, H, generator=g)
    xw = torch.randn(B, Tw, H, generator=g)
    return dict(src=src, xw=xw, wb=wb, dur=dur, swl=swl, src_len=wb.sum(1).clamp(max=Tp), Tp=Tp)
