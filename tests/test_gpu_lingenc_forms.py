"""The encoder's attention kernel in all six instantiations and its per-token glue kernels past their first workgroup
(csrc/lingenc.hip, csrc/lingenc_train.hip), each against the float64 restatement of tests/lingenc_torch.py at the
project's bars.

le_attention_kernel<REL, ROWS, TRAIN> takes 16 query rows per workgroup up to 615 keys and 4 up to 2895; at 615 and at
2895 the dynamic LDS request is exactly 64 KiB.  Every attention case first asserts mg_le_attention_rows(Lk) -- the function
the launcher switches on -- so the lengths below select <false, 16>, <false, 4> (word-to-phoneme), <true, 16>, <true, 4>
(inference) and <true, 16, true>, <true, 4, true> (train) on both sides of both thresholds.  The glue kernels run at sizes
whose second workgroup, strided-loop trip or partial tile the whole-encoder tests never reach.

Inputs are built on the CPU by the functions at the top (tests/test_attention_forms_cpu.py checks their margins with no
GPU); references are computed once per shape and shared."""
import ctypes
import functools

import pytest
import torch

import lingenc_torch as LT
from small_ops_ref import (BAR_MOVE, BAR_ELEM, BAR_RED, BAR_DGRAD, BAR_WGRAD, KINK_BAND, KINK_SHARE, check, check_equal,
                           gen, grads)

pytestmark = pytest.mark.gpu

H, D, W_DEFAULT, P_DROP = 2, 128, 4, 0.2
assert BAR_MOVE == 0.0


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd as m
    return m


def cuda(*ts):
    return [None if t is None else t.cuda() for t in ts]


def ragged_valid(B, L, g, full_first=True):
    lens = [L if full_first else max(1, (2 * L) // 3)] + [int(torch.randint(1, L + 1, (1,), generator=g)) for _ in range(B - 1)]
    return (torch.arange(L)[None] < torch.tensor(lens)[:, None]).to(torch.uint8)


def assert_rows(mg, Lk, rows):
    assert mg.lib().mg_le_attention_rows(Lk) == rows, "Lk = %d is no longer a %d-row case" % (Lk, rows)


def check_masked(got, ref32, ref64, bar, what, dim, group):
    """Non-finite positions of the reference must match exactly; the finite ones are held to `bar`."""
    got = got.detach().cpu()
    fin = torch.isfinite(ref64)
    assert torch.equal(torch.isfinite(got), fin) and torch.equal(got[~fin].double(), ref64[~fin]), what + ": non-finite"
    assert torch.equal(torch.isfinite(ref32), fin), what
    z = lambda t: torch.where(fin, t, torch.zeros((), dtype=t.dtype))  # noqa: E731
    check(z(got), z(ref32), z(ref64), bar, what, dim=dim, block=64, group=group)


# ------------------------------------------------------------------------------------ word-to-phoneme attention
W2P_SHAPES = [(9, 615, 16), (9, 616, 4), (40, 1500, 4), (9, 2895, 4)]


@functools.lru_cache(maxsize=None)
def w2p_inputs(Lq, Lk, ctc, B=2):
    g = gen(Lq + Lk)
    q = torch.randn(B, H * D, Lq, generator=g)
    kv = torch.randn(B, 2 * H * D, Lk, generator=g)
    kvalid = ragged_valid(B, Lk, g)
    qvalid = ragged_valid(B, Lq, g, full_first=False)
    mapping = (torch.rand(B, Lq, Lk, generator=g) < 0.3).to(torch.uint8)
    prior = torch.rand(B, Lk, Lq, generator=g) + 1e-3 if ctc else None
    return q, kv, kvalid, qvalid, mapping, prior


def w2p_ref(inp, dtype):
    q, kv, kvalid, qvalid, mapping, prior = inp
    return LT.w2p_attention(q.to(dtype), kv.to(dtype), kvalid, qvalid, mapping, None if prior is None else prior.to(dtype), H)


@pytest.mark.parametrize("ctc", [False, True], ids=["plain", "ctc"])
@pytest.mark.parametrize("Lq,Lk,rows", W2P_SHAPES)
def test_w2p_attention_forms(mg, Lq, Lk, rows, ctc):
    assert_rows(mg, Lk, rows)
    inp = w2p_inputs(Lq, Lk, ctc)
    ref32, ref64 = w2p_ref(inp, torch.float32), w2p_ref(inp, torch.float64)
    c = cuda(*inp)
    got = mg.linguistic_encoder.w2p_attention(*c, H)
    torch.cuda.synchronize()
    for name, dim, a, r32, r64 in zip(("out", "attn", "attn_raw", "logprob"), (2, 2, 2, 3), got, ref32, ref64):
        check_masked(a, r32, r64, BAR_RED, "w2p %dx%d %s %s" % (Lq, Lk, "ctc" if ctc else "plain", name), dim,
                     "w2p_attention fwd, %d rows" % rows)
    for name, a, b in zip(("out", "attn", "attn_raw", "logprob"), got, mg.linguistic_encoder.w2p_attention(*c, H)):
        assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32)), name + ": run 2 differs"


# ------------------------------------------------------------------------------------ relative self-attention
REL_SHAPES = [(615, 2, 16), (616, 2, 4), (1500, 2, 4), (2895, 1, 4)]


@functools.lru_cache(maxsize=None)
def rel_inputs(L, B, w):
    g = gen(L + 31 * w)
    qkv = torch.randn(B, 3 * H * D, L, generator=g)
    ek = torch.randn(2 * w + 1, D, generator=g) * D ** -0.5
    ev = torch.randn(2 * w + 1, D, generator=g) * D ** -0.5
    valid = ragged_valid(B, L, g)
    if B == 1:
        valid[0, L - L // 5:] = 0             # one item: full length for the kernel's loops, its tail padded
    keep = (torch.rand(B, H, L, L, generator=g) >= P_DROP).to(torch.uint8)
    return qkv, ek, ev, valid, keep


def rel_ref(L, B, w, dtype):
    """(out, out under dropout, P) of the restatement in `dtype`."""
    qkv, ek, ev, valid, keep = rel_inputs(L, B, w)
    qkv, ek, ev = qkv.to(dtype), ek.to(dtype), ev.to(dtype)
    P = LT.rel_attention_probs(qkv, valid, ek, H, w)
    return (LT.rel_attention_apply(P, qkv, ev, H, w), LT.rel_attention_apply(P, qkv, ev, H, w, keep, 1 / (1 - P_DROP)), P)


def _rel_case(mg, L, B, w, rows):
    assert_rows(mg, L, rows)
    LE = mg.linguistic_encoder
    qkv, ek, ev, valid, keep = cuda(*rel_inputs(L, B, w))
    ref64 = rel_ref(L, B, w, torch.float64)
    ref32 = rel_ref(L, B, w, torch.float32)
    what = "rel L=%d w=%d " % (L, w)
    out = LE.rel_attention(qkv, valid, ek, ev, H, w)
    check(out, ref32[0], ref64[0], BAR_RED, what + "inference", dim=2, block=64, group="rel_attention fwd, %d rows" % rows)
    check_equal(LE.rel_attention(qkv, valid, ek, ev, H, w), out.cpu(), what + "inference run 2")
    same, none = LE.rel_attention_train(qkv, valid, ek, ev, H, w, None, 1.0, save=False)
    assert none is None
    check_equal(same, out.cpu(), what + "train entry, no keep, nothing saved")
    del same
    tout, P = LE.rel_attention_train(qkv, valid, ek, ev, H, w, keep, 1 / (1 - P_DROP), save=True)
    group = "rel_attention train fwd, %d rows" % rows
    check(tout, ref32[1], ref64[1], BAR_RED, what + "train out", dim=2, block=64, group=group)
    check(P, ref32[2], ref64[2], BAR_RED, what + "train P", dim=2, block=64, group=group)
    tout2, P2 = LE.rel_attention_train(qkv, valid, ek, ev, H, w, keep, 1 / (1 - P_DROP), save=True)
    assert torch.equal(tout2, tout) and torch.equal(P2, P), what + "train run 2 differs"


@pytest.mark.parametrize("L,B,rows", REL_SHAPES)
def test_rel_attention_forms(mg, L, B, rows):
    _rel_case(mg, L, B, W_DEFAULT, rows)


@pytest.mark.parametrize("w", [0, 8])       # 4 is the case above; 8 = LE_WMAX
def test_rel_attention_window_widths(mg, w):
    _rel_case(mg, 616, 2, w, 4)


def test_le_attention_refuses_2896_keys(mg):
    """One key past the 4-row form: MG_ERR_SHAPE from all three entry points, the wrappers raise, nothing is written."""
    LE, L = mg.linguistic_encoder, 2896
    assert_rows(mg, L, 0)
    lib, s = mg.lib(), mg._lib.stream_ptr()
    qkv = torch.zeros(1, 3 * H * D, L, device="cuda")
    valid = torch.ones(1, L, device="cuda", dtype=torch.uint8)
    ek = torch.zeros(2 * W_DEFAULT + 1, D, device="cuda")
    out = torch.full((1, H * D, L), -7.25, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    SHAPE = mg._lib.MG_ERR_SHAPE
    assert lib.mg_rel_attention_fwd(p(qkv), p(valid), p(ek), p(ek), p(out), 1, L, H, D, W_DEFAULT, s) == SHAPE
    assert lib.mg_rel_attention_train_fwd(p(qkv), p(valid), p(ek), p(ek), None, 1.0, p(out), None, 1, L, H, D, W_DEFAULT,
                                          s) == SHAPE
    q = torch.zeros(1, H * D, 4, device="cuda")
    small = torch.full((H, 1, 4, L), -7.25, device="cuda")
    mapping = torch.ones(1, 4, L, device="cuda", dtype=torch.uint8)
    assert lib.mg_w2p_attention_fwd(p(q), p(qkv), p(valid), p(valid), p(mapping), None, p(out), p(small), p(small),
                                    p(small), 1, 4, L, H, D, s) == SHAPE
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()) and bool((small == -7.25).all())
    with pytest.raises(mg.MixganHipError):
        LE.rel_attention(qkv, valid, ek, ek, H, W_DEFAULT)
    with pytest.raises(mg.MixganHipError):
        LE.rel_attention_train(qkv, valid, ek, ek, H, W_DEFAULT, None, 1.0, save=False)
    with pytest.raises(mg.MixganHipError):
        LE.w2p_attention(q, qkv[:, :2 * H * D].contiguous(), valid, valid[:, :4].contiguous(), mapping, None, H)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ through the backward
def test_w2p_attention_bwd_from_the_4_row_forward(mg):
    LE, Lq, Lk, B = mg.linguistic_encoder, 40, 700, 2
    assert_rows(mg, Lk, 4)
    g = gen(4700)
    inp = w2p_inputs(Lq, Lk, True)
    q, kv, kvalid, qvalid, mapping, prior = inp
    cots = [torch.randn(B, H * D, Lq, generator=g)] + [torch.randn(H, B, Lq, Lk, generator=g) for _ in range(2)] + \
        [torch.randn(H, B, 1, Lq, Lk, generator=g)]

    def fn(a, b):
        return LT.w2p_attention(a, b, kvalid, qvalid, mapping, prior.to(a.dtype), H)
    ref64 = grads(fn, [q, kv], cots)
    ref32 = grads(fn, [q, kv], cots, torch.float32)
    c = cuda(*inp)
    out, attn, raw, logp = LE.w2p_attention(*c, H)
    args = c + [attn, raw, logp] + cuda(*cots) + [H]
    dq, dkv = LE.w2p_attention_bwd(*args)
    check(dq, ref32[0], ref64[0], BAR_DGRAD, "w2p bwd 40x700 dq", dim=2, block=64, group="w2p_attention bwd")
    check(dkv, ref32[1], ref64[1], BAR_DGRAD, "w2p bwd 40x700 dkv", dim=2, block=64, group="w2p_attention bwd")
    again = LE.w2p_attention_bwd(*args)
    assert torch.equal(again[0], dq) and torch.equal(again[1], dkv)


def test_rel_attention_bwd_from_the_4_row_train_forward(mg):
    LE, L, B, w = mg.linguistic_encoder, 700, 2, W_DEFAULT
    assert_rows(mg, L, 4)
    qkv, ek, ev, valid, keep = rel_inputs(L, B, w)
    gout = torch.randn(B, H * D, L, generator=gen(5700))
    scale = 1 / (1 - P_DROP)

    def fn(a, k, v):
        return LT.rel_attention_apply(LT.rel_attention_probs(a, valid, k, H, w), a, v, H, w, keep, scale)
    ref64 = grads(fn, [qkv, ek, ev], [gout])
    ref32 = grads(fn, [qkv, ek, ev], [gout], torch.float32)
    c = cuda(qkv, valid, ek, ev, keep, gout)
    out, P = LE.rel_attention_train(c[0], c[1], c[2], c[3], H, w, c[4], scale)
    got = LE.rel_attention_bwd(c[0], c[1], P, c[4], scale, c[5], c[2], c[3], H, w)
    group = "rel_attention bwd"
    check(got[0], ref32[0], ref64[0], BAR_DGRAD, "rel bwd L=700 dqkv", dim=2, block=64, group=group)
    check(got[1], ref32[1], ref64[1], BAR_WGRAD, "rel bwd L=700 d emb_k", group=group)
    check(got[2], ref32[2], ref64[2], BAR_WGRAD, "rel bwd L=700 d emb_v", group=group)
    again = LE.rel_attention_bwd(c[0], c[1], P, c[4], scale, c[5], c[2], c[3], H, w)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


# ------------------------------------------------------------------------------------ glue: forward
def scattered_valid(B, L, g):
    v = (torch.rand(B, L, generator=g) > 0.25).to(torch.uint8)
    v[0, 0] = 1
    if L > 1:
        v[0, L - 1] = 0
    return v


@pytest.mark.parametrize("C", [256, 40])
def test_embed_cm(mg, C):
    B, L, n = 3, 300, 23
    g = gen(C)
    ids = torch.randint(0, n, (B, L), generator=g)
    ids[0, :4] = torch.tensor([0, n - 1, -1, n])
    ids[2, L - 4:] = torch.tensor([n, -1, n - 1, 0])
    valid = scattered_valid(B, L, g)
    valid[0, :4] = 1
    valid[2, L - 4:] = 1
    table = torch.randn(n, C, generator=g)
    ref = LT.embed_cm(ids, table, valid)
    bad = ~(valid.bool() & (ids >= 0) & (ids < n))
    assert int(bad.sum()) > 10 and float(ref.transpose(1, 2)[bad].abs().sum()) == 0.0
    got = mg.linguistic_encoder.embed_cm(*cuda(ids, table, valid))
    check_equal(got, ref.contiguous(), "embed_cm C=%d" % C, group="embed_cm")
    check_equal(mg.linguistic_encoder.embed_cm(*cuda(ids, table, valid)), got.cpu(), "embed_cm C=%d run 2" % C)


VH_BINS = torch.tensor([-1.0, 0.25, 1.5])      # none at 0: the prediction of a masked frame is exactly 0


@functools.lru_cache(maxsize=None)
def variance_inputs(L, with_target, B=3, C=256):
    """h, weight, bias, valid, control, target, bins, emb, x, frames redrawn.  Without a target every valid frame's
    float64 prediction is farther than KINK_BAND of the bin span from every bin edge (frames inside it get a fresh
    column of h); with one, the target holds values exactly on every edge, below the first and above the last."""
    g = gen(10 * L + int(with_target))
    h = torch.randn(B, C, L, generator=g)
    weight = torch.randn(1, C, generator=g) * 2 / C ** 0.5
    bias = torch.randn(1, generator=g) * 0.1
    valid = scattered_valid(B, L, g)
    control = 1.0 if with_target else 1.25
    nb = VH_BINS.numel()
    emb = torch.randn(nb + 1, C, generator=g)
    x = torch.randn(B, C, L, generator=g)
    target, redrawn = None, 0
    if with_target:
        target = torch.randn(B, L, generator=g)
        special = torch.cat([VH_BINS, VH_BINS[:1] - 1, VH_BINS[-1:] + 1])
        idx = torch.randperm(B * L, generator=g)[:min(B * L, 3 * special.numel())]
        target.view(-1)[idx] = special.repeat(3)[:idx.numel()]
    else:
        band = KINK_BAND * float(VH_BINS[-1] - VH_BINS[0])
        while True:
            pred, _ = LT.variance_head(h.double(), weight.double(), bias.double(), valid, control, None, VH_BINS)
            near = ((pred[:, :, None] - VH_BINS.double()).abs() <= band).any(-1) & valid.bool()
            n = int(near.sum())
            if n == 0:
                break
            redrawn += n
            b, l = near.nonzero(as_tuple=True)
            h[b, :, l] = torch.randn(n, C, generator=g)
    return h, weight, bias, valid, control, target, VH_BINS, emb, x, redrawn


@pytest.mark.parametrize("add", [True, False], ids=["embed", "pred_only"])
@pytest.mark.parametrize("with_target", [True, False], ids=["target", "no_target"])
@pytest.mark.parametrize("L", [1, 256, 257, 700])
def test_variance_head(mg, L, with_target, add):
    h, weight, bias, valid, control, target, bins, emb, x, redrawn = variance_inputs(L, with_target)
    assert redrawn <= KINK_SHARE * valid.numel(), "%d of %d frames redrawn" % (redrawn, valid.numel())
    p64, bucket = LT.variance_head(h.double(), weight.double(), bias.double(), valid, control, target, bins)
    p32, _ = LT.variance_head(h, weight, bias, valid, control, target, bins)
    what = "variance_head L=%d %s " % (L, "target" if with_target else "no target")
    xg = x.cuda()
    dev = cuda(h, weight, bias, valid)
    kw = dict(target=None if target is None else target.cuda(), bins=bins.cuda() if add else None,
              emb=emb.cuda() if add else None, x=xg if add else None)
    pred = mg.linguistic_encoder.variance_head(*dev, control, **kw)
    check(pred, p32, p64, BAR_RED, what + "pred", dim=1, block=64, group="variance_head")
    if add:
        e = emb[bucket].transpose(1, 2)
        check(xg, x + e, x.double() + e.double(), BAR_ELEM, what + "x", dim=2, block=64, group="variance_head")
        x2 = x.cuda()
        kw["x"] = x2
        again = mg.linguistic_encoder.variance_head(*dev, control, **kw)
        assert torch.equal(again, pred) and torch.equal(x2, xg), what + "run 2 differs"
    else:
        assert torch.equal(xg.cpu(), x)


@functools.lru_cache(maxsize=None)
def duration_inputs(W, B=2, Tp=None):
    """logp [B, Tp], integer target, wb [B, W], src_w_len.  Words have 0 to 5 phonemes; item 0 counts all W words, the
    others fewer; every counted word's sum of exp(logp) is farther than 0.05 from a half-integer."""
    g = gen(W)
    wb = torch.randint(1, 6, (B, W), generator=g)
    if W > 2:
        wb[:, W // 2] = 0
        wb[0, W - 1] = 0
    swl = torch.tensor([W] + [max(1, W - 1 - 3 * b) for b in range(1, B)])
    need = int(wb.sum(1).max())
    Tp = need if Tp is None else Tp
    assert Tp >= need
    sums = torch.rand(B, W, generator=g, dtype=torch.float64) * 6.8 + 0.2
    frac = sums - sums.floor()
    sums = torch.where((frac - 0.5).abs() < 0.05, sums + 0.2, sums)
    share = torch.rand(B, Tp, generator=g, dtype=torch.float64) + 0.1
    wi = LT.word_index(wb, Tp)                                        # [B, Tp], W past the last word
    tot = torch.zeros(B, W + 1, dtype=torch.float64).scatter_add_(1, wi, share)
    val = F_pad1(sums).gather(1, wi) * share / tot.gather(1, wi)
    logp = val.log().float()
    target = torch.randint(0, 9, (B, Tp), generator=g)
    return logp, target, wb, swl


def F_pad1(t):
    return torch.nn.functional.pad(t, (0, 1), value=1.0)


@pytest.mark.parametrize("d_control", [1.0, 0.5, 1.25])
@pytest.mark.parametrize("with_target", [True, False], ids=["target", "no_target"])
@pytest.mark.parametrize("W", [1, 256, 257, 300])
def test_duration_head(mg, W, with_target, d_control):
    logp, target, wb, swl = duration_inputs(W)
    tgt = target if with_target else None
    lw64, dur = LT.duration_head(logp.double(), tgt, wb, swl, d_control, W)
    lw32, dur32 = LT.duration_head(logp, tgt, wb, swl, d_control, W)
    s = lw64.exp()
    counted = torch.isfinite(lw64)
    assert int((~counted).sum()) >= 1 or W == 1
    assert float(((s - s.floor() - 0.5).abs())[counted].min()) > 1e-3, "a word sum within 1e-3 of a half-integer"
    assert torch.equal(dur, dur32)
    what = "duration_head W=%d %s x%.2f " % (W, "target" if with_target else "no target", d_control)
    dev = cuda(logp, tgt, wb, swl)
    logw, d = mg.linguistic_encoder.duration_head(*dev, d_control, W)
    check_masked(logw, lw32, lw64, BAR_RED, what + "log_w", 1, "duration_head")
    check_equal(d, dur, what + "durations", group="duration_head")
    assert int(d.cpu()[~counted].abs().sum()) == 0
    logw2, d2 = mg.linguistic_encoder.duration_head(*dev, d_control, W)
    assert torch.equal(logw2.view(torch.int32), logw.view(torch.int32)) and torch.equal(d2, d)


@pytest.mark.parametrize("rowmajor", [True, False], ids=["rowmajor", "channelmajor"])
@pytest.mark.parametrize("C", [256, 40])
@pytest.mark.parametrize("L", [1, 31, 33, 300])
def test_posenc_add(mg, L, C, rowmajor):
    B = 2
    g = gen(L + C)
    x = torch.randn(B, L, C, generator=g) if rowmajor else torch.randn(B, C, L, generator=g)
    coef = torch.rand(B, L, generator=g)
    table = torch.randn(L + 7, C, generator=g)
    ref32, ref64 = LT.posenc_add(x, rowmajor, coef, table), LT.posenc_add(x.double(), rowmajor, coef.double(), table.double())
    dev = cuda(x, coef, table)
    got = mg.linguistic_encoder.posenc_add(dev[0], rowmajor, dev[1], dev[2])
    check(got, ref32, ref64, BAR_ELEM, "posenc_add L=%d C=%d %s" % (L, C, "rowmajor" if rowmajor else "channel-major"), dim=2,
          block=64, group="posenc_add")
    assert torch.equal(mg.linguistic_encoder.posenc_add(dev[0], rowmajor, dev[1], dev[2]), got)


# ------------------------------------------------------------------------------------ glue: backward
@pytest.mark.parametrize("B,L", [(3, 37), (4, 300), (1, 257)])
def test_variance_head_bwd(mg, B, L):
    C, scale = 256, 1.5
    g = gen(B * L)
    h = torch.randn(B, C, L, generator=g)
    weight = torch.randn(1, C, generator=g) / C ** 0.5
    bias = torch.randn(1, generator=g)
    valid = scattered_valid(B, L, g)
    valid[:, L - 1] = 1                        # at (1, 257) frame 256 is the whole second trip of the strided sum
    dpred = torch.randn(B, L, generator=g)

    def fn(a, w, b):
        return LT.variance_head(a, w, b, valid, scale, None, VH_BINS)[0]
    ref64 = grads(fn, [h, weight, bias], [dpred])
    ref32 = grads(fn, [h, weight, bias], [dpred], torch.float32)
    dev = cuda(h, weight, valid)
    got = mg.linguistic_encoder.variance_head_bwd(*dev, scale, dpred.cuda())
    what = "variance_head_bwd B=%d L=%d " % (B, L)
    check(got[0], ref32[0], ref64[0], BAR_DGRAD, what + "dh", dim=2, block=64, group="variance_head_bwd")
    check(got[1], ref32[1].reshape(-1), ref64[1].reshape(-1), BAR_WGRAD, what + "dw", group="variance_head_bwd")
    check(got[2], ref32[2], ref64[2], BAR_WGRAD, what + "db", group="variance_head_bwd")
    again = mg.linguistic_encoder.variance_head_bwd(*dev, scale, dpred.cuda())
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("C", [256, 40])
def test_embed_cm_bwd(mg, C):
    B, L, n = 3, 300, 11                       # 900 tokens on 11 rows: every id repeats within and across items
    g = gen(50 + C)
    ids = torch.randint(0, n, (B, L), generator=g)
    ids[:, 5] = 7
    ids[1, :40] = 3
    valid = scattered_valid(B, L, g)
    table = torch.randn(n, C, generator=g)
    dout = torch.randn(B, C, L, generator=g)
    fn = lambda t: LT.embed_cm(ids, t, valid, skip_row=0)  # noqa: E731
    ref64, ref32 = grads(fn, [table], [dout])[0], grads(fn, [table], [dout], torch.float32)[0]
    assert float(ref64[0].abs().sum()) == 0.0
    dev = cuda(ids, dout, valid)
    got = mg.linguistic_encoder.embed_cm_bwd(*dev, n, 0)
    check(got, ref32, ref64, BAR_WGRAD, "embed_cm_bwd C=%d" % C, group="embed_cm_bwd")
    assert float(got[0].abs().sum()) == 0.0
    assert torch.equal(mg.linguistic_encoder.embed_cm_bwd(*dev, n, 0), got)


@pytest.mark.parametrize("Tp", [257, 700])
def test_duration_head_bwd(mg, Tp):
    W, B = Tp // 4, 2                          # about 3 phonemes a word: the last quarter belongs to no word
    logp, _, wb, swl = duration_inputs(W, B, Tp)
    assert logp.shape == (B, Tp)
    lw64, _ = LT.duration_head(logp.double(), None, wb, swl, 1.0, W)
    fin = torch.isfinite(lw64)
    dlw = torch.randn(B, W, generator=gen(Tp)) * fin
    fn = lambda a: torch.where(fin, LT.duration_head(a, None, wb, swl, 1.0, W)[0], torch.zeros((), dtype=a.dtype))  # noqa: E731
    ref64, ref32 = grads(fn, [logp], [dlw])[0], grads(fn, [logp], [dlw], torch.float32)[0]
    assert bool(torch.isfinite(ref64).all())
    dev = cuda(logp, wb, swl)
    logw, _ = mg.linguistic_encoder.duration_head(dev[0], None, dev[1], dev[2], 1.0, W)
    got = mg.linguistic_encoder.duration_head_bwd(dev[0], logw, dlw.cuda(), dev[1], dev[2])
    check(got, ref32, ref64, BAR_DGRAD, "duration_head_bwd Tp=%d" % Tp, dim=1, block=64, group="duration_head_bwd")
    assert torch.equal(mg.linguistic_encoder.duration_head_bwd(dev[0], logw, dlw.cuda(), dev[1], dev[2]), got)


@pytest.mark.parametrize("L", [33, 300])
def test_posenc_add_bwd(mg, L):
    B, C = 3, 40
    g = gen(900 + L)
    coef = torch.rand(B, L, generator=g)
    dout = torch.randn(B, C, L, generator=g)
    table = torch.randn(L, C, generator=g)
    x = torch.zeros(B, C, L)
    fn = lambda t: LT.posenc_add(x.to(t.dtype), False, coef.to(t.dtype), t)  # noqa: E731
    ref64, ref32 = grads(fn, [table], [dout])[0], grads(fn, [table], [dout], torch.float32)[0]
    dev = cuda(dout, coef)
    got = mg.linguistic_encoder.posenc_add_bwd(*dev)
    check(got, ref32, ref64, BAR_WGRAD, "posenc_add_bwd L=%d C=%d" % (L, C), dim=0, block=64, group="posenc_add_bwd")
    assert torch.equal(mg.linguistic_encoder.posenc_add_bwd(*dev), got)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_dropout_apply(mg, n):
    g = gen(n)
    x = torch.randn(n, generator=g)
    keep = (torch.rand(n, generator=g) >= P_DROP).to(torch.uint8)
    keep[0] = 1
    scale = 1 / (1 - P_DROP)
    dev = cuda(x, keep)
    got = mg.linguistic_encoder.dropout_apply(*dev, scale)
    check(got, LT.dropout_apply(x, keep, scale), LT.dropout_apply(x.double(), keep, scale), BAR_ELEM, "dropout_apply n=%d" % n,
          group="dropout_apply")
    assert torch.equal(mg.linguistic_encoder.dropout_apply(*dev, scale), got)
