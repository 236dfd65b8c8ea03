"""The references and the inputs of tests/test_gpu_small_ops.py, proven without a GPU: every restatement of
tests/small_ops_ref.py is pinned to torch's own operator where there is one and to oracle/refmath.py where that is the
authority, the conventions on a kink (clamp at +-1, ReLU / leaky ReLU at 0, L1 at a == b) are torch's, and every input
set the GPU file draws keeps its distance from the kinks, leaves out at most 1e-3 of a tensor, and is computed by the
float32 restatement to within bar / 8 of float64, so that the bars of DESIGN.md section 7 apply as stated."""
import pytest
import torch
import torch.nn.functional as F

import small_ops_ref as S
from helpers import rel_err
from oracle import refmath as R

f64 = torch.float64


def close(a, b, tol=1e-12):
    assert a.shape == b.shape and rel_err(a.detach().numpy(), b.detach().numpy()) <= tol


def own_error(fn, args, bar, what):
    """The float32 restatement against the float64 one on the same float32 inputs: within bar / 8."""
    o32, o64 = fn(*S.as_dtype(args, torch.float32)), fn(*S.as_dtype(args, f64))
    if isinstance(o32, torch.Tensor):
        o32, o64 = (o32,), (o64,)
    for i, (a, b) in enumerate(zip(o32, o64)):
        if a is None:
            continue
        e = rel_err(a.detach().double().numpy(), b.detach().numpy())
        print("%-52s float32 restatement %.3e  bar / 8 %.1e" % ("%s[%d]" % (what, i), e, bar / 8))
        assert e <= bar / 8, (what, i, e)


def away(x, kinks, redrawn, what, on=None, scale=None, total=None):
    n_on, dist = S.kink_report(x, kinks, scale)
    print("%-52s on a kink %d  nearest other %.2e of max  redrawn %d of %d" % (what, n_on, dist, redrawn, x.numel()))
    assert dist > S.KINK_BAND, (what, dist)
    total = x.numel() if total is None else total           # the tensor the elements were redrawn in
    assert redrawn <= S.KINK_SHARE * total or total < 1000 and redrawn <= 1, (what, redrawn, total)
    if on is not None:
        assert n_on >= on, (what, n_on)


# ------------------------------------------------------------------------------------------------ pins
def test_linear_mish_losses_are_torchs():
    g = S.gen(0)
    x, W = torch.randn(9, 65, generator=g, dtype=f64), torch.randn(5, 65, generator=g, dtype=f64)
    close(S.linear(x, W), F.linear(x, W))
    close(S.mish(x), F.mish(x))
    a, b = torch.randn(1000, generator=g, dtype=f64), torch.randn(1000, generator=g, dtype=f64)
    close(S.loss_sum(a, b, 0.0, 1), F.l1_loss(a, b, reduction="sum"))
    close(S.loss_sum(a, None, 0.7, 0), F.mse_loss(a, torch.full_like(a, 0.7), reduction="sum"))
    t = torch.tensor([0, 1, 99, 999])
    W0, W2 = torch.randn(10, 6, generator=g, dtype=f64), torch.randn(3, 10, generator=g, dtype=f64)
    out, emb, pre, h = S.step_mlp(t, W0, W2)
    assert torch.equal(emb, R.step_embedding(t, 6, f64)) and emb.dtype == f64
    close(out, F.linear(F.mish(F.linear(emb, W0)), W2))
    assert torch.equal(R.step_embedding(t, 256).double(), R.step_embedding(t, 256, f64))     # the fp32-rounded values
    import mixgan_tts_amd as mg
    for D in (6, 256):
        ang = (t[:, None].float() * S.frequencies(D)[None, :]).double()
        assert torch.equal(torch.cat((ang.sin(), ang.cos()), -1).float(), R.step_embedding(t, D)), D
    assert mg.ops.ACT["lrelu"] == mg._lib.MG_ACT_LRELU02


def test_kink_conventions_are_torchs():
    """What the kernels do ON a kink is what torch.autograd does there."""
    x = torch.tensor([-1.5, -1.0, -0.3, 1.0, 1.5], dtype=f64)
    g = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=f64)
    assert S.grads(lambda v: v.clamp(-1.0, 1.0), [x], [g])[0].tolist() == [0.0, 2.0, 3.0, 4.0, 0.0]
    z = torch.tensor([-2.0, 0.0, 2.0], dtype=f64)
    one = torch.ones(3, dtype=f64)
    assert S.grads(lambda v: S.act(v, "relu"), [z], [one])[0].tolist() == [0.0, 0.0, 1.0]
    assert S.grads(lambda v: S.act(v, "lrelu"), [z], [one])[0].tolist() == [0.2, 0.2, 1.0]
    assert S.grads(lambda v: S.act(v, "tanh"), [z], [one])[0][1].item() == 1.0
    assert S.grads(lambda v: S.loss_sum(v, torch.zeros(3, dtype=f64), 0.0, 1), [z], [torch.ones((), dtype=f64)])[0].tolist() \
        == [-1.0, 0.0, 1.0]
    # the posterior passes the gradient where x0 * keep sits exactly on +-1
    buf = S.schedule()
    x0 = torch.tensor([-1.5, -1.0, 1.0, 1.5]).reshape(1, 1, 4)
    t = torch.tensor([2])
    fn = lambda a: S.q_posterior_sample(buf, a, torch.zeros_like(a), t, torch.zeros_like(a), None, True)   # noqa: E731
    d = S.grads(fn, [x0], [torch.ones(1, 1, 4), None])[0]
    assert d.reshape(-1).tolist() == [0.0, 1.0, 1.0, 0.0]


@pytest.mark.parametrize("rows,Lin,s,Lup", S.UPS_CASES[:4] + [(3, 50, 4, 197), (3, 50, 4, 150), (3, 50, 4, 230)])
@pytest.mark.parametrize("slope", [1.0, 0.1])
def test_upsample_zero_is_conv_transpose_with_a_unit_weight(rows, Lin, s, Lup, slope):
    x = torch.randn(rows, 1, Lin, generator=S.gen(Lin), dtype=f64)
    y = F.conv_transpose1d(F.leaky_relu(x, slope), torch.ones(1, 1, 1, dtype=f64), stride=s)[:, 0]
    y = F.pad(y, (0, Lup - y.shape[-1])) if Lup >= y.shape[-1] else y[:, :Lup]
    assert torch.equal(S.upsample_zero(x[:, 0], s, Lup, slope), y)


def test_diffusion_restatements_are_refmaths():
    buf = S.schedule()
    b64 = S.as_dtype(buf, f64)
    mel, t, nz = S.diffuse_inputs(65, 80)
    mel, nz = mel.double(), nz.double()
    keep = S.keep_mask(len(t), 65)
    inside = torch.tensor([0, 1, 2, 3, 0])
    assert torch.equal(S.diffuse_fn(buf, mel, inside, nz), R.diffuse_fn(b64, mel, inside, nz[:, None])[:, 0])
    out = S.diffuse_fn(buf, mel, t, nz, keep)
    clamped = S.diffuse_fn(buf, mel, torch.tensor([-1, 0, 3, 3, 3]), nz, keep)
    assert torch.equal(out, clamped)                                                      # t >= T is T - 1
    clean = S.transpose(mel, False, 1, buf["spec_min"], buf["spec_max"], keep)
    assert torch.equal(out[0], clean[0]) and not torch.equal(out[1], clean[1])            # t < 0 is the clean mel
    assert bool((out[:, :, keep[0] == 0][0] == 0).all())
    x = torch.randn(3, 80, 65, generator=S.gen(1), dtype=f64)
    assert torch.equal(S.transpose(x, True, 2, buf["spec_min"], buf["spec_max"]),
                       R.denorm_spec(x.transpose(1, 2), b64["spec_min"], b64["spec_max"]))
    assert torch.equal(S.transpose(x, True, 0), x.transpose(1, 2).contiguous())
    p = S.posterior_inputs(3, 5)
    x0c, xpp = S.q_posterior_sample(buf, p["x0"].double(), p["x_t"].double(), torch.tensor([0, 1, 3, 3]),
                                    p["noise"].double(), None, False)
    assert torch.equal(xpp, R.q_posterior_sample(b64, p["x0"].double()[:, None], p["x_t"].double()[:, None],
                                                 torch.tensor([0, 1, 3, 3]), p["noise"].double()[:, None])[:, 0])
    same = S.q_posterior_sample(buf, p["x0"].double(), p["x_t"].double(), p["t"], p["noise"].double(), None, False)[1]
    assert torch.equal(xpp, same)                                                         # t = T + 3 is T - 1
    other = S.q_posterior_sample(buf, p["x0"].double(), p["x_t"].double(), p["t"], p["noise2"].double(), None, False)[1]
    assert torch.equal(other[0], xpp[0]) and not torch.equal(other[1], xpp[1])            # no noise at t = 0
    mn, mx = S.spec(80)
    assert len(set(mn.tolist())) == 80 and len(set(mx.tolist())) == 80 and bool((mx - mn > 1).all())
    pred, target, pad, _ = S.mel_inputs(2, 3, 80)
    num, den = S.mel_l1_terms(pred.double(), target.double(), pad)
    close(num / den, R.mel_l1(pred.double(), target.double(), pad))


# ------------------------------------------------------------------------------------------------ input sets
def test_transpose_inputs():
    for M in S.TRANSPOSE_M:
        mn, mx = S.spec(M)
        for L in (1, 65, 260):
            for to_blm, mode in ((0, 1), (1, 2)):
                x = S.transpose_inputs(3, L, M, to_blm)
                own_error(lambda a: S.transpose(a, to_blm, mode, mn, mx, S.keep_mask(3, L)), [x], S.BAR_ELEM,
                          "transpose L %d M %d mode %d" % (L, M, mode))
    for L in S.TRANSPOSE_L:
        k = S.keep_mask(3, L)
        assert k.dtype == torch.uint8 and (L < 2 or int(k[0, -1]) == 0) and (L < 3 or int(k[0, L // 2]) == 0)
        assert L < 4 or int(k[0].sum()) > 0


@pytest.mark.parametrize("L,M,_off", S.DIFFUSE_CASES[:8])
def test_diffuse_inputs(L, M, _off):
    buf = S.schedule(M=M)
    mel, t, nz = S.diffuse_inputs(L, M)
    assert t.tolist() == [-1, 0, S.T_STEPS - 1, S.T_STEPS, S.T_STEPS + 5]
    own_error(lambda a, b: S.diffuse_fn(buf, a, t, b, S.keep_mask(len(t), L)), [mel, nz], S.BAR_ELEM, "diffuse")


@pytest.mark.parametrize("M,L,_off", [c for c in S.POSTERIOR_CASES if c[2] == 0])
def test_posterior_inputs(M, L, _off):
    buf = S.schedule(M=M)
    p = S.posterior_inputs(M, L)
    kept = p["x0"] * p["keep"][:, None, :]
    live = kept[p["keep"][:, None, :].expand_as(kept) != 0]
    away(live, (-1.0, 1.0), p["redrawn"], "posterior x0 * keep", on=2 if M * L > 100 else 0, scale=float(p["x0"].abs().max()),
         total=p["x0"].numel())
    assert int(p["keep"][2].sum()) == 0 and int(p["keep"][0].sum()) > 0 and p["t"].tolist() == list(S.POSTERIOR_T)
    if M == 80:                                              # just past the 512 x 256 cap of its form
        assert 512 * 256 < (M * L if L % 4 else M * L // 4) < 512 * 256 + 256
    for clip in (True, False):
        fwd = lambda a: S.q_posterior_sample(buf, a, p["x_t"], p["t"], p["noise"], p["keep"], clip)   # noqa: E731
        own_error(lambda a: fwd(a.to(a.dtype)), [p["x0"]], S.BAR_ELEM, "posterior clip %d" % clip)
        for cots in ((p["g_x0c"], None), (None, p["g_xpp"]), (p["g_x0c"], p["g_xpp"])):
            g32 = S.grads(lambda a: S.q_posterior_sample(buf, a, p["x_t"], p["t"], p["noise"], p["keep"], clip),
                          [p["x0"]], cots, torch.float32)[0]
            g64 = S.grads(lambda a: S.q_posterior_sample(buf, a, p["x_t"].double(), p["t"], p["noise"].double(), p["keep"],
                                                         clip), [p["x0"]], cots)[0]
            assert rel_err(g32.double().numpy(), g64.numpy()) <= S.BAR_DGRAD / 8


def test_capped_kernel_inputs():
    for name in ("relu", "lrelu", "tanh"):
        for n in S.ACT_N:
            pre, dy, redrawn = S.act_inputs(n, name)
            away(pre, (0.0,), redrawn, "act_bwd %s n %d" % (name, n), on=16)
            assert int((S.act(pre, name) == 0).sum()) >= 16                  # saved outputs that are exactly 0
            g32 = S.grads(lambda a: S.act(a, name), [pre], [dy], torch.float32)[0]
            g64 = S.grads(lambda a: S.act(a, name), [pre], [dy])[0]
            assert rel_err(g32.double().numpy(), g64.numpy()) <= S.BAR_DGRAD / 8
    assert S.ACT_N[0] < 256 < S.CAP_ACT < S.ACT_N[1] and S.ACT_N[1] % 256
    assert S.AFFINE_ROWS[0] * 80 < 256 and S.AFFINE_ROWS[1] * 80 > S.CAP_AFFINE and (S.AFFINE_ROWS[1] * 80) % 256
    n = [b * c * l for b, c, l in S.GATE_SHAPES]
    assert n[0] < 256 and n[1] > S.CAP_GATE and n[1] % 256
    assert S.MISH_N[0] < 256 and S.MISH_N[1] > S.CAP_MISH and S.MISH_N[1] % 256
    rows, Lin, s, Lup = S.UPS_CASES[-1]
    assert rows * Lup > S.CAP_UPS and (rows * Lup) % 256 and Lup == (Lin - 1) * s + 1
    assert {(c[3] > (c[1] - 1) * c[2] + 1) - (c[3] < (c[1] - 1) * c[2] + 1) for c in S.UPS_CASES} == {-1, 0, 1}
    n = [b * l * m for b, l, m in S.TRACE_SHAPES]
    assert n[0] < 256 and n[1] > S.CAP_TRACE and n[1] % 256
    assert S.LOSS_N[0] < 256 and S.LOSS_N[1] > max(S.CAP_LOSS_SUM, S.CAP_LOSS_GRAD) and S.LOSS_N[1] % 256
    rows = [b * l for b, l, _ in S.MEL_CASES]
    assert rows[0] > 8192 and {m for _, _, m in S.MEL_CASES} >= {80, 1, 65}
    mn, mx = S.spec(80)
    x = torch.randn(S.AFFINE_ROWS[1], 80, generator=S.gen(5))
    for mode in (1, 2, 3, 4):
        own_error(lambda a: S.spec_affine(a, mn, mx, mode), [x], S.BAR_ELEM, "spec_affine mode %d" % mode)
    x = torch.randn(S.MISH_N[1], generator=S.gen(6)) * 3
    own_error(S.mish, [x], S.BAR_ELEM, "mish")


def test_trace_loss_and_mel_inputs():
    B, L, M = S.TRACE_SHAPES[0]
    for B, L, M in (S.TRACE_SHAPES[0], (2, 700, 80)):                # the large shape is drawn by the same function
        buf = S.schedule(M=M)
        p = S.trace_inputs(B, L, M)
        nv = S.norm_spec(p["x"].double(), buf["spec_min"].double(), buf["spec_max"].double())
        away(nv.abs(), (1.0,), p["redrawn"], "diffuse_trace |norm(x)|", on=8 if B * L > 100 else 1)
        assert bool((S.norm_spec(p["x"], buf["spec_min"], buf["spec_max"]).abs() == 1).sum() >= (8 if B * L > 100 else 1))
        fn = lambda a: S.diffuse_trace(buf, a, p["keep"], p["noises"])                # noqa: E731
        g32, g64 = S.grads(fn, [p["x"]], [p["g"]], torch.float32)[0], S.grads(fn, [p["x"]], [p["g"]])[0]
        assert rel_err(g32.double().numpy(), g64.numpy()) <= S.BAR_DGRAD / 8
    for n in S.LOSS_N:
        a, b, redrawn = S.loss_inputs(n)
        away(a - b, (0.0,), redrawn, "loss a - b, n %d" % n, on=16)
        own_error(lambda u, v: S.loss_sum(u, v, 0.0, 1), [a, b], S.BAR_RED, "l1 sum")
        own_error(lambda u: S.loss_sum(u, None, 0.7, 0), [a], S.BAR_RED, "mse sum")
    for B, L, M in S.MEL_CASES:
        pred, target, pad, redrawn = S.mel_inputs(B, L, M)
        live = (pred - target)[~pad & (target.abs().sum(-1) != 0)]
        away(live, (0.0,), redrawn, "mel pred - target %s" % ((B, L, M),), on=1)
        assert bool(pad.any()) and bool((pred[pad] != 0).any()) and bool((target[pad] != 0).any())
        assert bool((target[-1, 0] == 0).all()) and not bool(pad[-1, 0]) and bool((pred[-1, 0] != 0).all())
        own_error(lambda u, v: S.mel_l1_terms(u, v, pad), [pred, target], S.BAR_RED, "mel_l1")


def test_linear_and_mlp_inputs():
    for B in S.LIN_B:
        for N in S.LIN_N:
            for K in S.LIN_K:
                x, W, g = S.linear_inputs(B, N, K)
                own_error(S.linear, [x, W], S.BAR_RED, "linear %s" % ((B, N, K),))
                g32, g64 = S.grads(S.linear, [x, W], [g], torch.float32), S.grads(S.linear, [x, W], [g])
                assert rel_err(g32[0].double().numpy(), g64[0].numpy()) <= S.BAR_DGRAD / 8
                assert rel_err(g32[1].double().numpy(), g64[1].numpy()) <= S.BAR_WGRAD / 8
    for D0, D1, D2 in S.MLP_DIMS:
        for B in (8, 9):
            t, W0, W2, g = S.mlp_inputs(D0, D1, D2, B)
            assert set(t.tolist()) == set(S.MLP_T)
            own_error(lambda a, b: S.step_mlp(t, a, b)[0], [W0, W2], S.BAR_RED, "step_mlp %s" % ((D0, D1, D2, B),))
            g32 = S.grads(lambda a, b: S.step_mlp(t, a, b)[0], [W0, W2], [g], torch.float32)
            g64 = S.grads(lambda a, b: S.step_mlp(t, a, b)[0], [W0, W2], [g])
            for a, b in zip(g32, g64):
                assert rel_err(a.double().numpy(), b.numpy()) <= S.BAR_WGRAD / 8


@pytest.mark.parametrize("name", [k for k in S.LING_CASES if not k.startswith("limit")])
def test_lingops_inputs(name):
    c = S.LING_CASES[name]
    p = S.lingops_inputs(**c)
    assert bool((p["dur"] < 0).any()) and bool((p["dur"] == 0).any())
    assert int(p["wb"][0, 2]) == 0 and int(p["swl"][0]) > 2                  # a zero-length word that is counted
    assert int(p["swl"][-1]) > c["Tw"] and int(p["wb"][1].sum()) > p["Tp"]
    ref = S.word_level_pooling(p["src"].double(), p["src_len"], p["wb"], p["swl"], "mean")
    nan = torch.isnan(ref)
    assert bool(nan[0, 2].all()) and int(nan.sum()) == c["H"]                # NaN there and nowhere else
    own = S.word_level_pooling(p["src"], p["src_len"], p["wb"], p["swl"], "sum")
    assert rel_err(own.double().numpy(), S.word_level_pooling(p["src"].double(), p["src_len"], p["wb"], p["swl"]).numpy()) \
        <= S.BAR_RED / 8
