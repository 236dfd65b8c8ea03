"""GPU parity of the aux pre-training kernels (bgemm.hip, train_ops.hip and the attention_train / layernorm_train /
batchnorm_act Functions) against float64 CPU computations of the same operations, at the shapes where the launchers
change form: both workgroup tiles of mg_bgemm in its four layouts (MG_BGEMM_TILE), attention at lengths that take the
128 x 128 tile by default, the LayerNorm backward's partial-sum slots wrapping, the BatchNorm loops at more than one
trip and more than one grid pass.

Error measure: max-abs error over max-abs reference (helpers.assert_close).  Bars: 2e-5 maps,
5e-5 data gradients, 1e-4 parameter gradients; where the float32 CPU restatement's own error against float64 exceeds
bar / 8 on a tensor, that tensor's bar is 8 x that error (helpers.check).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from helpers import check

pytestmark = pytest.mark.gpu
BAR_MAP, BAR_DATA, BAR_PARAM = 2e-5, 5e-5, 1e-4
DTYPES = (torch.float64, torch.float32)


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def pin_tile(monkeypatch, tile):
    if tile is None:
        monkeypatch.delenv("MG_BGEMM_TILE", raising=False)
    else:
        monkeypatch.setenv("MG_BGEMM_TILE", str(tile))


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------
# a. mg_bgemm, direct
# ------------------------------------------------------------------------------------------------------------------
BGEMM_SHAPES = [(1, 1, 1, 1, 1), (64, 128, 16, 1, 1), (129, 257, 17, 1, 2), (130, 70, 300, 2, 3), (37, 53, 15, 2, 1)]
LAYOUTS = [(False, False), (True, False), (False, True), (True, True)]      # (A k-contiguous, B k-contiguous)
LAYOUT_IDS = ["Am_Bn", "Ak_Bn", "Am_Bk", "Ak_Bk"]
_bgemm_ref = {}


def bgemm_case(shape):
    """A [batch, heads, M, K], B [batch, heads, K, N], C0 [batch, heads, M, N] and the float64 / float32 CPU A @ B."""
    if shape not in _bgemm_ref:
        M, N, K, batch, heads = shape
        gen = torch.Generator().manual_seed(M * 7 + N * 3 + K)
        A = torch.randn(batch, heads, M, K, generator=gen)
        B = torch.randn(batch, heads, K, N, generator=gen)
        C0 = torch.randn(batch, heads, M, N, generator=gen)
        _bgemm_ref[shape] = {"A": A, "B": B, "C0": C0, torch.float64: A.double() @ B.double(), torch.float32: A @ B}
    return _bgemm_ref[shape]


def launch_bgemm(mg, A_ptr, B_ptr, C_ptr, shape, sa, sb, sc, alpha, accumulate):
    """sa = (a_ms, a_ks, a_bs, a_hs), sb = (b_ks, b_ns, b_bs, b_hs), sc = (c_ms, c_bs, c_hs); pointers in bytes."""
    M, N, K, batch, heads = shape
    vp = ctypes.c_void_p
    mg._lib.check(mg._lib.lib().mg_bgemm(vp(A_ptr), vp(B_ptr), vp(C_ptr), M, N, K, batch, heads, *sa, *sb, *sc,
                                         float(alpha), int(accumulate), None))
    torch.cuda.synchronize()


def packed_operands(c, shape, a_kc, b_kc):
    """Device copies of A and B in the asked layout, with their stride tuples."""
    M, N, K, batch, heads = shape
    Ad = (c["A"] if a_kc else c["A"].transpose(2, 3)).contiguous().cuda()
    Bd = (c["B"].transpose(2, 3) if b_kc else c["B"]).contiguous().cuda()
    a_ms, a_ks = (K, 1) if a_kc else (1, M)
    b_ks, b_ns = (1, K) if b_kc else (N, 1)
    return Ad, Bd, (a_ms, a_ks, heads * M * K, M * K), (b_ks, b_ns, heads * K * N, K * N)


def run_packed(mg, c, shape, a_kc, b_kc, alpha, accumulate, prefill):
    M, N, K, batch, heads = shape
    Ad, Bd, sa, sb = packed_operands(c, shape, a_kc, b_kc)
    Cd = prefill.clone().cuda()
    launch_bgemm(mg, Ad.data_ptr(), Bd.data_ptr(), Cd.data_ptr(), shape, sa, sb, (N, heads * M * N, M * N), alpha, accumulate)
    return Cd


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("shape", BGEMM_SHAPES, ids=lambda s: "M%d_N%d_K%d_b%d_h%d" % s)
def test_bgemm_both_tiles(mg, monkeypatch, shape, a_kc, b_kc):
    """Each tile form, accumulating onto random C and overwriting a NaN-filled C (accumulate = 0 must not read C);
    a second run gives the same bits (no atomics), and the two forms give the same bits (same k order, same MFMA)."""
    c = bgemm_case(shape)
    nan = torch.full_like(c["C0"], float("nan"))
    got = {}
    for tile in (64, 128):
        pin_tile(monkeypatch, tile)
        assert mg._lib.lib().mg_bgemm_tile(*shape[:2], *shape[3:]) == tile
        acc = run_packed(mg, c, shape, a_kc, b_kc, 0.5, 1, c["C0"])
        check(acc, 0.5 * c[torch.float32] + c["C0"], 0.5 * c[torch.float64] + c["C0"].double(), BAR_MAP,
              "tile %d: 0.5 A B + C" % tile)
        over = run_packed(mg, c, shape, a_kc, b_kc, 1.0, 0, nan)
        assert bool(torch.isfinite(over).all()), "accumulate = 0 read the old C"
        check(over, c[torch.float32], c[torch.float64], BAR_MAP, "tile %d: A B over NaN" % tile)
        assert torch.equal(acc, run_packed(mg, c, shape, a_kc, b_kc, 0.5, 1, c["C0"])), "accumulating run not reproducible"
        assert torch.equal(over, run_packed(mg, c, shape, a_kc, b_kc, 1.0, 0, nan)), "overwriting run not reproducible"
        got[tile] = (acc, over)
    assert torch.equal(got[64][0], got[128][0]) and torch.equal(got[64][1], got[128][1]), "the two tile forms differ in bits"


SENTINEL = 7777.25


def strided_buffer(logical, strides, offset, fill):
    """A flat CPU buffer filled with `fill` that holds `logical` at `offset` with `strides`; returns (flat, view)."""
    size = offset + sum((n - 1) * s for n, s in zip(logical.shape, strides)) + 1 + 9
    flat = torch.full((size,), fill, dtype=torch.float32)
    view = flat.as_strided(tuple(logical.shape), strides, offset)
    view.copy_(logical)
    return flat, view


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS, ids=LAYOUT_IDS)
def test_bgemm_strided_views(mg, monkeypatch, tile, a_kc, b_kc):
    """A and B as views into larger buffers with gaps between heads and batches (NaN in the gaps: a read of one poisons
    the result), C as a column window of a wider buffer (c_ms = N + 5) whose guard columns and gaps stay bit-unchanged."""
    shape = M, N, K, batch, heads = (130, 70, 300, 2, 3)
    c = bgemm_case(shape)
    pin_tile(monkeypatch, tile)
    a_ms, a_ks = (K, 1) if a_kc else (1, M)
    b_ks, b_ns = (1, K) if b_kc else (N, 1)
    a_hs, b_hs = M * K + 7, 2 * K * N + 3            # a head stride of its own for each operand, neither the packed one
    a_bs, b_bs = heads * a_hs + 11, heads * b_hs + 5
    nan = float("nan")
    Af, _ = strided_buffer(c["A"], (a_bs, a_hs, a_ms, a_ks), 3, nan)
    Bf, _ = strided_buffer(c["B"], (b_bs, b_hs, b_ks, b_ns), 6, nan)
    c_ms = N + 5
    c_hs = M * c_ms + 13
    c_bs = heads * c_hs + 17
    c_off = 2                                         # the window starts two columns into the wider rows
    Ad, Bd = Af.cuda(), Bf.cuda()
    for alpha, accumulate, window, r32, r64 in (
            (0.5, 1, c["C0"], 0.5 * c[torch.float32] + c["C0"], 0.5 * c[torch.float64] + c["C0"].double()),
            (1.0, 0, torch.full_like(c["C0"], nan), c[torch.float32], c[torch.float64])):
        Cf, Cview = strided_buffer(window, (c_bs, c_hs, c_ms, 1), c_off, SENTINEL)
        outside = torch.ones_like(Cf, dtype=torch.bool)
        outside.as_strided(tuple(window.shape), (c_bs, c_hs, c_ms, 1), c_off).fill_(False)
        assert int(outside.sum()) == Cf.numel() - window.numel()
        Cd = Cf.cuda()
        launch_bgemm(mg, Ad.data_ptr() + 4 * 3, Bd.data_ptr() + 4 * 6, Cd.data_ptr() + 4 * c_off, shape,
                     (a_ms, a_ks, a_bs, a_hs), (b_ks, b_ns, b_bs, b_hs), (c_ms, c_bs, c_hs), alpha, accumulate)
        back = Cd.cpu()
        assert torch.equal(bits(back[outside]), bits(Cf[outside])), "wrote outside the C window"
        got = back.as_strided(tuple(window.shape), (c_bs, c_hs, c_ms, 1), c_off)
        assert bool(torch.isfinite(got).all()), "read a gap of A or B, or the old C"
        check(got, r32, r64, BAR_MAP, "strided, tile %d, accumulate %d" % (tile, accumulate))
        # the same bits as the packed call of the same form
        assert torch.equal(got, run_packed(mg, c, shape, a_kc, b_kc, alpha, accumulate, window).cpu())


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS, ids=LAYOUT_IDS)
def test_bgemm_default_form_at_the_threshold(mg, monkeypatch, a_kc, b_kc):
    """2 x 2 x 128 = 512 tiles of 128 x 128: the first size that takes the 128 form by itself."""
    shape = (200, 200, 20, 16, 8)
    c = bgemm_case(shape)
    zero = torch.zeros_like(c["C0"])
    pin_tile(monkeypatch, None)
    assert mg._lib.lib().mg_bgemm_tile(200, 200, 16, 8) == 128
    default = run_packed(mg, c, shape, a_kc, b_kc, 1.0, 0, zero)
    check(default, c[torch.float32], c[torch.float64], BAR_MAP, "default form")
    pin_tile(monkeypatch, 128)
    assert torch.equal(default, run_packed(mg, c, shape, a_kc, b_kc, 1.0, 0, zero)), "default is not the pinned 128 form"
    pin_tile(monkeypatch, 64)
    assert torch.equal(default, run_packed(mg, c, shape, a_kc, b_kc, 1.0, 0, zero)), "the two tile forms differ in bits"


# ------------------------------------------------------------------------------------------------------------------
# b. softmax_rows_fwd / _bwd, direct
# ------------------------------------------------------------------------------------------------------------------
def scattered_pad(B, L, gen, lens=None):
    """[B, L] bool, True = padded: about a third of the keys, scattered (not a suffix), key 0 always live; with `lens`
    the frames from lens[b] on are padded as well."""
    pad = torch.rand(B, L, generator=gen) < 0.3
    pad[:, 0] = False
    if lens is not None:
        pad |= torch.arange(L)[None, :] >= torch.tensor(lens)[:, None]
    return pad


@pytest.mark.parametrize("wide", [False, True], ids=["unit", "pm60"])
@pytest.mark.parametrize("B,H,L", [(2, 2, 1), (2, 2, 63), (1, 2, 64), (1, 3, 65), (2, 2, 1500)])
def test_softmax_rows(mg, B, H, L, wide):
    """B H L = 195 rows at (1, 3, 65): the last workgroup has one live wave.  `wide`: scale * S uniform in +-60."""
    gen = torch.Generator().manual_seed(L * 2 + int(wide))
    scale = 128 ** -0.5
    if wide:
        S = (torch.rand(B * H, L, L, generator=gen) * 2 - 1) * (60.0 / scale)
    else:
        S = torch.randn(B * H, L, L, generator=gen) / scale
    pad = scattered_pad(B, L, gen)
    dP = torch.randn(B * H, L, L, generator=gen)
    keymask = pad[:, None, None, :].expand(B, H, L, L).reshape(B * H, L, L)
    ref = {dt: torch.softmax((S.to(dt) * scale).masked_fill(keymask, float("-inf")), dim=-1) for dt in DTYPES}
    lib, vp = mg._lib.lib(), ctypes.c_void_p
    Sd, padd = S.cuda(), pad.to(torch.uint8).cuda()
    mg._lib.check(lib.mg_softmax_rows_fwd(vp(Sd.data_ptr()), vp(padd.data_ptr()), B, H, L, scale, None))
    P = Sd.cpu()
    check(P, ref[torch.float32], ref[torch.float64], BAR_MAP, "softmax rows L=%d" % L)
    assert bool((P[keymask] == 0).all()), "a masked key has weight"
    rows = float((P.double().sum(-1) - 1).abs().max())
    print("%-40s err %.3e  bar %.1e" % ("row sums", rows, BAR_MAP))
    assert rows <= BAR_MAP
    # backward on the kernel's own P, in place on dP
    dref = {dt: scale * P.to(dt) * (dP.to(dt) - (P.to(dt) * dP.to(dt)).sum(-1, keepdim=True)) for dt in DTYPES}
    dPd = dP.cuda()
    mg._lib.check(lib.mg_softmax_rows_bwd(vp(Sd.data_ptr()), vp(dPd.data_ptr()), B, H, L, scale, None))
    check(dPd, dref[torch.float32], dref[torch.float64], BAR_DATA, "softmax rows backward L=%d" % L)
    assert torch.equal(Sd.cpu(), P), "the backward wrote P"


# ------------------------------------------------------------------------------------------------------------------
# c. attention_train through the Function
# ------------------------------------------------------------------------------------------------------------------
H_, D_ = 2, 128
ATT_CASES = {"B8_L650": (8, 650, [650, 1, 333, 640, 641, 129, 64, 500], 1.0),
             "B32_L259": (32, 259, [259, 1] + [1 + (37 * i) % 259 for i in range(30)], 1.0),
             "B8_L650_peaked": (8, 650, [650, 1, 333, 640, 641, 129, 64, 500], 3.0)}


def attention_case(name):
    B, L, lens, gain = ATT_CASES[name]
    gen = torch.Generator().manual_seed(L + B)
    qkv = torch.randn(B, 3 * H_ * D_, L, generator=gen) * gain
    go = torch.randn(B, H_ * D_, L, generator=gen)
    pad = torch.arange(L)[None, :] >= torch.tensor(lens)[:, None]
    out = {"qkv": qkv, "go": go, "pad": pad}
    for dt in DTYPES:
        x = qkv.to(dt, copy=True).requires_grad_()
        q, k, v = [t.view(B, H_, D_, L) for t in x.split(H_ * D_, dim=1)]
        att = torch.einsum("bhdq,bhdk->bhqk", q, k) * (float(D_) ** -0.5)
        att = torch.softmax(att.masked_fill(pad[:, None, None, :], float("-inf")), dim=-1)
        o = torch.einsum("bhqk,bhdk->bhdq", att, v).reshape(B, H_ * D_, L)
        (o * go.to(dt)).sum().backward()
        out[dt] = {"out": o.detach(), "P": att.detach().reshape(B * H_, L, L), "d_qkv": x.grad}
    return out


@pytest.mark.parametrize("name", list(ATT_CASES))
def test_attention_train(mg, monkeypatch, name):
    B, L, lens, _ = ATT_CASES[name]
    c = attention_case(name)
    r64, r32 = c[torch.float64], c[torch.float32]
    pin_tile(monkeypatch, None)
    tile = mg._lib.lib().mg_bgemm_tile
    print("tiles: L x L GEMMs %d, d-row GEMMs %d" % (tile(L, L, B, H_), tile(D_, L, B, H_)))
    if L == 650:
        assert tile(L, L, B, H_) == 128 and tile(D_, L, B, H_) == 64       # S, dP  |  O, dV, dQ, dK
    padd = c["pad"].to(torch.uint8).cuda()
    xg = c["qkv"].cuda().requires_grad_()
    out = mg.autograd.attention_train(xg, padd, H_, D_)
    check(out, r32["out"], r64["out"], BAR_MAP, "attention_train out")
    (out * c["go"].cuda()).sum().backward()
    check(xg.grad, r32["d_qkv"], r64["d_qkv"], BAR_DATA, "attention_train d_qkv")
    # the kept probabilities
    out2, P = mg.ops.attention_train_fwd(c["qkv"].cuda(), padd, H_, D_)
    assert torch.equal(out2, out.detach()), "the forward gives other bits the second time"
    check(P, r32["P"], r64["P"], BAR_MAP, "kept P")
    keymask = c["pad"][:, None, None, :].expand(B, H_, L, L).reshape(B * H_, L, L)
    assert bool((P.cpu()[keymask] == 0).all()), "a padded key has weight"
    del P
    # the streaming-softmax inference kernel computes the same function
    check(mg.ops.attention(c["qkv"].cuda(), padd, H_, D_), r32["out"], r64["out"], BAR_MAP, "eval kernel")
    x2 = c["qkv"].cuda().requires_grad_()
    (mg.autograd.attention_train(x2, padd, H_, D_) * c["go"].cuda()).sum().backward()
    assert torch.equal(x2.grad, xg.grad), "the backward gives other bits the second time"


# ------------------------------------------------------------------------------------------------------------------
# d. LayerNorm, train forward and backward
# ------------------------------------------------------------------------------------------------------------------
LN_CASES = [(3, 1100, 0.0), (40, 33, 0.0), (1, 1, 0.0), (3, 1100, 50.0)]


def layernorm_case(B, L, mean, drop):
    C = 256
    gen = torch.Generator().manual_seed(B * 10000 + L)
    s = 0.7 if mean else 1.0                 # a + res: per-frame mean `mean`, spread about 1
    a, res = torch.randn(B, C, L, generator=gen) * s, torch.randn(B, C, L, generator=gen) * s + mean
    go = torch.randn(B, C, L, generator=gen)
    gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    pad = scattered_pad(B, L, gen)
    keep = (torch.rand(B, C, L, generator=gen) >= 0.2) if drop else None
    out = {"a": a, "res": res, "go": go, "gamma": gamma, "beta": beta, "pad": pad, "keep": keep}
    for dt in DTYPES:
        ar, rr, gr, br = (t.to(dt, copy=True).requires_grad_() for t in (a, res, gamma, beta))
        pre = (ar * keep.to(dt) * (1 / 0.8) if drop else ar) + rr
        y = F.layer_norm(pre.transpose(1, 2), (C,), gr, br, 1e-5).transpose(1, 2).masked_fill(pad[:, None, :], 0)
        (y * go.to(dt)).sum().backward()
        out[dt] = {"out": y.detach(), "d_a": ar.grad, "d_res": rr.grad, "dgamma": gr.grad, "dbeta": br.grad}
    return out


@pytest.mark.parametrize("drop", [False, True], ids=["nokeep", "keep"])
@pytest.mark.parametrize("B,L,mean", LN_CASES, ids=lambda v: str(v))
def test_layernorm_train(mg, B, L, mean, drop):
    """(3, 1100): blockIdx.x reaches 34 and the slot index (blockIdx.x + blockIdx.y) % 32 wraps; (40, 33): it wraps
    through blockIdx.y and the second frame tile has one live frame; mean 50: the two-pass variance."""
    c = layernorm_case(B, L, mean, drop)
    r64, r32 = c[torch.float64], c[torch.float32]
    padd = c["pad"].to(torch.uint8).cuda()
    keepd = c["keep"].to(torch.uint8).cuda() if drop else None
    scale = 1 / 0.8 if drop else 1.0
    runs = []
    for _ in range(2):
        ag, rg, gg, bg = (c[k].cuda().requires_grad_() for k in ("a", "res", "gamma", "beta"))
        out = mg.autograd.layernorm_train(ag, rg, gg, bg, padd, keepd, scale, 1e-5)
        (out * c["go"].cuda()).sum().backward()
        check(out, r32["out"], r64["out"], BAR_MAP, "LN out")
        check(ag.grad, r32["d_a"], r64["d_a"], BAR_DATA, "LN d_a")
        check(rg.grad, r32["d_res"], r64["d_res"], BAR_DATA, "LN d_res")
        check(gg.grad, r32["dgamma"], r64["dgamma"], BAR_PARAM, "LN dgamma")       # atomics: each run against float64
        check(bg.grad, r32["dbeta"], r64["dbeta"], BAR_PARAM, "LN dbeta")
        runs.append((out.detach(), ag.grad, rg.grad))
    for x, y in zip(*runs):
        assert torch.equal(x, y), "out / d_a / d_res have no atomics and must reproduce"
    if not drop:       # the inference kernel runs the same arithmetic
        same = mg.ops.layernorm_cm(c["a"].cuda(), c["res"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), padd, 1e-5)
        assert torch.equal(same, runs[0][0]), "train forward and inference LayerNorm differ in bits"


# ------------------------------------------------------------------------------------------------------------------
# e. BatchNorm + act + dropout
# ------------------------------------------------------------------------------------------------------------------
def batchnorm_ref(x, gamma, beta, keep, scale, act, go, dt):
    """From the definition (F.batch_norm refuses one value per channel): biased batch statistics over (B, L)."""
    xr, gr, br = (t.to(dt, copy=True).requires_grad_() for t in (x, gamma, beta))
    mean = xr.mean((0, 2), keepdim=True)
    var = ((xr - mean) ** 2).mean((0, 2), keepdim=True)
    y = (xr - mean) * torch.rsqrt(var + 1e-5) * gr[None, :, None] + br[None, :, None]
    if act == "tanh":
        y = torch.tanh(y)
    if keep is not None:
        y = y * keep.to(dt) * scale
    (y * go.to(dt)).sum().backward()
    return {"mean": mean.detach().reshape(-1), "var": var.detach().reshape(-1), "out": y.detach(), "dx": xr.grad,
            "dgamma": gr.grad, "dbeta": br.grad}


@pytest.mark.parametrize("B,C,L,act,drop", [(6, 512, 700, "tanh", True), (2, 3, 257, None, False), (1, 1, 1, "tanh", False)])
def test_batchnorm_act(mg, B, C, L, act, drop):
    """(6, 512, 700): 2 150 400 elements, more than the 8192 x 256 one grid pass covers, and L > 256 (a second trip of
    the per-channel loops); its data has mean 30, sigma 0.5 and every channel's first sample -- the shift the statistics
    kernel subtracts -- 6 sigma out.  (1, 1, 1): variance exactly 0."""
    gen = torch.Generator().manual_seed(C + L)
    if B == 6:
        x = 30.0 + 0.5 * torch.randn(B, C, L, generator=gen)
        x[0, :, 0] = 30.0 + 6 * 0.5
    else:
        x = torch.randn(B, C, L, generator=gen) * 2 + 0.7
    go = torch.randn(B, C, L, generator=gen)
    gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    keep = (torch.rand(B, C, L, generator=gen) >= 0.5) if drop else None
    scale = 2.0 if drop else 1.0
    r64, r32 = (batchnorm_ref(x, gamma, beta, keep, scale, act, go, dt) for dt in DTYPES)
    xg, gg, bg = (t.clone().cuda().requires_grad_() for t in (x, gamma, beta))
    out, mean, var = mg.autograd.batchnorm_act(xg, gg, bg, keep.to(torch.uint8).cuda() if drop else None, scale, act, 1e-5)
    check(mean, r32["mean"], r64["mean"], BAR_MAP, "BN mean")
    check(var, r32["var"], r64["var"], BAR_MAP, "BN var")
    if B * L == 1:
        assert float(var.abs().max()) == 0.0
    check(out, r32["out"], r64["out"], BAR_MAP, "BN out")
    (out * go.cuda()).sum().backward()
    check(xg.grad, r32["dx"], r64["dx"], BAR_DATA, "BN dx")
    check(gg.grad, r32["dgamma"], r64["dgamma"], BAR_PARAM, "BN dgamma")
    check(bg.grad, r32["dbeta"], r64["dbeta"], BAR_PARAM, "BN dbeta")
