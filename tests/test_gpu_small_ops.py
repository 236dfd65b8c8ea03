"""The small diffusion, step-MLP, loss and index kernels (elementwise.hip, misc_api.hip, the small_* kernels of
denoiser_common.h, the scalar part of losses.hip, lingops.hip forward and backward) called directly, against the float64
restatements of tests/small_ops_ref.py, at the sizes where each picks another form: 16-byte or scalar access (L % 4,
M % 4, K % 256, a 1-float storage offset), a grid at its cap with the stride loop behind it, a clamped t, batch chunks
of 8, rows in fours, K tiles of 64, and the LDS limits.  Data movement and masking are held to bit equality;
elementwise forwards to 2e-6, reductions and linears to 2e-5, data gradients to 5e-5, weight gradients to 1e-4
(helpers.bar_for's fallback rule), on the whole tensor and on every 64-frame block of L / every 8
rows of B against that block's own maximum.  tests/test_small_ops_cpu.py proves the references and the inputs."""
import pytest
import torch

import small_ops_ref as S
from small_ops_ref import check, check_equal

pytestmark = pytest.mark.gpu
f64 = torch.float64


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd as m
    assert torch.cuda.is_available()
    m.lib()
    return m


@pytest.fixture(scope="module", autouse=True)
def worst_errors():
    """After the file's last test: the worst measured error of every group next to its bar."""
    yield
    for grp, (_, e, bar, what) in sorted(S.WORST.items()):
        print("WORST | %-28s | %.1e | %s | %s" % (grp, e, "bit-equal" if bar == 1.0 and e == 0 else "%.0e" % bar, what.strip()))


def dev(x):
    return None if x is None else x.cuda()


def dbuf(buf):
    return {k: v.cuda() for k, v in buf.items()}


def offset_view(x):
    """x on the device, starting 1 float into its storage: contiguous, 4-byte aligned only."""
    store = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
    v = store[1:].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def both(fn, args):
    """(float32 restatement, float64 reference) of fn on the same float32 inputs."""
    return fn(*S.as_dtype(args, torch.float32)), fn(*S.as_dtype(args, f64))


# ------------------------------------------------------------------------------------------------ transposes
@pytest.mark.parametrize("to_blm,mode", [(0, 0), (0, 1), (1, 0), (1, 2)])
def test_transpose_bml(mg, to_blm, mode):
    grp = "transpose mode %d" % mode
    for M in S.TRANSPOSE_M:
        mn, mx = S.spec(M)
        for L in S.TRANSPOSE_L:
            for B in S.TRANSPOSE_B:
                x = S.transpose_inputs(B, L, M, to_blm)
                for keep in (None, S.keep_mask(B, L)):
                    what = "transpose to_blm %d mode %d B %d L %d M %d keep %d" % (to_blm, mode, B, L, M, keep is not None)
                    got = mg.ops.transpose_bml(dev(x), bool(to_blm), mode, dev(mn), dev(mx), dev(keep))
                    r32, r64 = both(lambda a: S.transpose(a, to_blm, mode, mn, mx, keep), [x])
                    if mode == 0:
                        check_equal(got, r32, what, grp)
                    else:
                        check(got, r32, r64, S.BAR_ELEM, what, dim=1 if to_blm else 2, group=grp)
                    if keep is not None:
                        dead = (keep == 0)[:, :, None].expand(B, L, M) if to_blm else (keep == 0)[:, None, :].expand(B, M, L)
                        assert bool((got.cpu()[dead] == 0).all()), what + ": masked positions not 0"


@pytest.mark.parametrize("M", [80, 4])
def test_transpose_offset_source_takes_the_scalar_form(mg, M):
    """L = 64, M % 4 == 0: the vector form but for the source's base, 1 float into its storage."""
    mn, mx = S.spec(M)
    for to_blm, mode in ((0, 0), (0, 1), (1, 0), (1, 2)):
        x = S.transpose_inputs(3, 64, M, to_blm)
        keep = S.keep_mask(3, 64)
        aligned = mg.ops.transpose_bml(dev(x), bool(to_blm), mode, dev(mn), dev(mx), dev(keep))
        got = mg.ops.transpose_bml(offset_view(x), bool(to_blm), mode, dev(mn), dev(mx), dev(keep))
        check_equal(got, aligned.cpu(), "transpose offset source to_blm %d mode %d M %d" % (to_blm, mode, M), "transpose mode %d" % mode)
        r32, r64 = both(lambda a: S.transpose(a, to_blm, mode, mn, mx, keep), [x])
        if mode == 0:
            check_equal(got, r32, "  against torch", "transpose mode 0")
        else:
            check(got, r32, r64, S.BAR_ELEM, "  against float64", dim=1 if to_blm else 2, group="transpose mode %d" % mode)


@pytest.mark.parametrize("M", [80, 3])
def test_cat_and_split_transpose(mg, M):
    from mixgan_tts_amd import autograd as A
    for L in S.TRANSPOSE_L:
        for B in S.TRANSPOSE_B:
            g = S.gen(L * M + B)
            a, b = torch.randn(B, L, M, generator=g), torch.randn(B, L, M, generator=g)
            ref = torch.cat([a, b], -1).transpose(1, 2).contiguous()
            what = "B %d L %d M %d" % (B, L, M)
            check_equal(mg.ops.cat_transpose(dev(a), dev(b)), ref, "cat_transpose " + what, "cat / split transpose")
            da, db = mg.ops.split_transpose(dev(ref), M)
            check_equal(da, a, "split_transpose a " + what, "cat / split transpose")
            check_equal(db, b, "split_transpose b " + what, "cat / split transpose")
            ag, bg = dev(a).requires_grad_(), dev(b).requires_grad_()
            out = A.cat_transpose(ag, bg)
            cot = torch.randn(B, 2 * M, L, generator=g)
            (out * dev(cot)).sum().backward()
            check_equal(out, ref, "autograd.cat_transpose " + what, "cat / split transpose")
            check_equal(ag.grad, cot[:, :M].transpose(1, 2).contiguous(), "  d a", "cat / split transpose")
            check_equal(bg.grad, cot[:, M:].transpose(1, 2).contiguous(), "  d b", "cat / split transpose")


def test_lds_limit_transposes_and_the_next_m_is_refused(mg):
    """The widest M the [64][M + 1] LDS tile allows launches and is bit-exact in both directions at L = 65 (two tiles, the
    second of one frame); one more is MG_ERR_SHAPE before any launch, for the transposes and for diffuse."""
    lim = mg.ops.transpose_max_m()
    print("mg_transpose_max_m() = %d" % lim)
    assert 255 <= lim <= 1024
    L = 65
    x = torch.randn(1, lim, L, generator=S.gen(lim))
    check_equal(mg.ops.transpose_bml(dev(x), True), x.transpose(1, 2).contiguous(), "transpose to_blm at M = %d" % lim, "LDS limit")
    check_equal(mg.ops.transpose_bml(dev(x.transpose(1, 2).contiguous()), False), x, "transpose to_bml at M = %d" % lim, "LDS limit")
    buf = S.schedule(M=lim)
    mel, nz = S.transpose_inputs(1, L, lim, 0), torch.randn(1, lim, L, generator=S.gen(1))
    for t in (-1, 2):
        tt = torch.tensor([t])
        got = mg.ops.diffuse(dev(mel), dev(tt), dev(nz), None, dbuf(buf))
        r32, r64 = both(lambda a, b: S.diffuse_fn(buf, a, tt, b), [mel, nz])
        check(got, r32, r64, S.BAR_ELEM, "diffuse at M = %d, t = %d" % (lim, t), dim=2, group="LDS limit")
    M = lim + 1
    Lb, s = mg.lib(), mg._lib.stream_ptr()
    x = torch.randn(1, M, L).cuda()
    out = torch.full((1, L, M), 7.0).cuda()
    mn = torch.zeros(M).cuda()
    fp = mg._lib.fptr
    assert Lb.mg_transpose_bml(fp(x), fp(out), None, None, None, 1, 0, 1, L, M, s) == mg._lib.MG_ERR_SHAPE
    assert Lb.mg_transpose_bml(fp(out), fp(x), None, None, None, 0, 0, 1, L, M, s) == mg._lib.MG_ERR_SHAPE
    assert Lb.mg_transpose_bml_strided(fp(x), fp(out), None, None, None, 1, 0, 1, L, M, M * L, s) == mg._lib.MG_ERR_SHAPE
    t = torch.zeros(1, dtype=torch.int64).cuda()
    tab = torch.ones(4).cuda()
    assert Lb.mg_diffuse_fwd(fp(out), mg._lib.iptr(t, torch.int64), fp(x), None, fp(mn), fp(mn), fp(tab), fp(tab), fp(out),
                             1, L, M, 4, s) == mg._lib.MG_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(mg.MixganHipError):
        mg.ops.transpose_bml(x, True)


# ------------------------------------------------------------------------------------------------ diffuse
@pytest.mark.parametrize("L,M,off", S.DIFFUSE_CASES)
def test_diffuse(mg, L, M, off):
    buf = S.schedule(M=M)
    db = dbuf(buf)
    mel, t, nz = S.diffuse_inputs(L, M)
    T = S.T_STEPS
    for keep in (None, S.keep_mask(len(t), L)):
        what = "diffuse L %d M %d offset %s keep %d" % (L, M, off, keep is not None)
        dm = offset_view(mel) if off == "mel" else dev(mel)
        dn = offset_view(nz) if off == "noise" else dev(nz)
        got = mg.ops.diffuse(dm, dev(t), dn, dev(keep), db)
        r32, r64 = both(lambda a, b: S.diffuse_fn(buf, a, t, b, keep), [mel, nz])
        check(got, r32, r64, S.BAR_ELEM, what, dim=2, group="diffuse")
        clean = mg.ops.transpose_bml(dm, False, 1, db["spec_min"], db["spec_max"], dev(keep))
        check_equal(got[0], clean[0].cpu(), "  t = -1 is the mode-1 transpose", "diffuse")
        clamped = mg.ops.diffuse(dm, dev(t.clamp(max=T - 1)), dn, dev(keep), db)
        check_equal(got[3:], clamped[3:].cpu(), "  t = T, T + 5 are t = T - 1", "diffuse")
        assert not torch.equal(got[1].cpu(), got[2].cpu())
        if off:
            check_equal(got, mg.ops.diffuse(dev(mel), dev(t), dev(nz), dev(keep), db).cpu(), "  equals the aligned call", "diffuse")
        if keep is not None:
            assert bool((got.cpu()[(keep == 0)[:, None, :].expand_as(got)] == 0).all()), what + ": masked positions not 0"


# ------------------------------------------------------------------------------------------------ posterior
@pytest.mark.parametrize("M,L,off", S.POSTERIOR_CASES)
def test_posterior_sample_forward_and_backward(mg, M, L, off):
    buf = S.schedule(M=M)
    db = dbuf(buf)
    p = S.posterior_inputs(M, L)
    place = offset_view if off else dev
    for keep in (p["keep"], None):
        for clip in (True, False):
            what = "posterior M %d L %d offset %d keep %d clip %d" % (M, L, off, keep is not None, clip)
            x0d = place(p["x0"])
            out, x0c = mg.ops.posterior_sample(x0d, dev(p["x_t"]), dev(p["t"]), dev(p["noise"]), dev(keep), db, clip=clip,
                                               want_x0c=True)
            fn = lambda a, b, c: S.q_posterior_sample(buf, a, b, p["t"], c, keep, clip)     # noqa: E731
            r32, r64 = both(fn, [p["x0"], p["x_t"], p["noise"]])
            check_equal(x0c, r32[0], what + ": x0 masked and clamped", "posterior forward")
            check(out, r32[1], r64[1], S.BAR_ELEM, what, dim=2, group="posterior forward")
            out2 = mg.ops.posterior_sample(x0d, dev(p["x_t"]), dev(p["t"]), dev(p["noise2"]), dev(keep), db, clip=clip)
            check_equal(out2[0], out[0].cpu(), "  t = 0: the noise does not contribute", "posterior forward")
            assert not torch.equal(out2[1].cpu(), out[1].cpu())
            if keep is not None:
                assert bool((out.cpu()[(keep == 0)[:, None, :].expand_as(out)] == 0).all()), what
            for name, cots in (("g_x0c", (p["g_x0c"], None)), ("g_xpp", (None, p["g_xpp"])), ("both", (p["g_x0c"], p["g_xpp"]))):
                got = mg.ops.posterior_sample_bwd(x0d, dev(p["t"]), dev(keep), db["posterior_mean_coef1"], dev(cots[0]),
                                                  dev(cots[1]), clip)
                g32 = S.grads(lambda a: fn(a, p["x_t"], p["noise"]), [p["x0"]], cots, torch.float32)[0]
                g64 = S.grads(lambda a: fn(a, p["x_t"].double(), p["noise"].double()), [p["x0"]], cots)[0]
                check(got, g32, g64, S.BAR_DGRAD, "  d x0 from " + name, dim=2, group="posterior backward")
                if clip and cots[0] is not None and cots[1] is None and keep is None:
                    on = (p["x0"].abs() == 1)
                    assert int(on.sum()) >= 2 and torch.equal(got.cpu()[on], p["g_x0c"][on])      # passes on +-1
                    assert bool((got.cpu()[p["x0"].abs() > 1] == 0).all())


@pytest.mark.parametrize("through", [True, False])
def test_posterior_fn_autograd(mg, through):
    from mixgan_tts_amd.autograd import _PosteriorFn
    M, L = 80, 132
    buf = S.schedule(M=M)
    db = dbuf(buf)
    p = S.posterior_inputs(M, L)
    x0 = dev(p["x0"]).requires_grad_()
    x0c, xpp = _PosteriorFn.apply(x0, dev(p["x_t"]), dev(p["t"]), dev(p["noise"]), dev(p["keep"]), db["posterior_mean_coef1"],
                                  db["posterior_mean_coef2"], db["posterior_log_variance_clipped"], True, through)
    assert x0c.requires_grad and xpp.requires_grad == through
    loss = (x0c * dev(p["g_x0c"])).sum()
    if through:
        loss = loss + (xpp * dev(p["g_xpp"])).sum()
    loss.backward()
    cots = (p["g_x0c"], p["g_xpp"] if through else None)
    fn = lambda a, b, c: S.q_posterior_sample(buf, a, b, p["t"], c, p["keep"], True)        # noqa: E731
    r32, r64 = both(fn, [p["x0"], p["x_t"], p["noise"]])
    check(xpp, r32[1], r64[1], S.BAR_ELEM, "_PosteriorFn x_{t-1}", dim=2, group="posterior forward")
    g32 = S.grads(lambda a: fn(a, p["x_t"], p["noise"]), [p["x0"]], cots, torch.float32)[0]
    g64 = S.grads(lambda a: fn(a, p["x_t"].double(), p["noise"].double()), [p["x0"]], cots)[0]
    check(x0.grad, g32, g64, S.BAR_DGRAD, "_PosteriorFn d x0, through_posterior %d" % through, dim=2, group="posterior backward")


# ------------------------------------------------------------------------------------------------ capped grid-stride kernels
@pytest.mark.parametrize("name", ["relu", "lrelu", "tanh"])
@pytest.mark.parametrize("n", S.ACT_N)
def test_act_bwd(mg, name, n):
    pre, dy, _ = S.act_inputs(n, name)
    y = S.act(pre, name)                                  # the saved output, as float32 rounds it
    got = mg.ops.act_bwd(dev(dy), dev(y), name)
    g32, g64 = (S.grads(lambda a: S.act(a, name), [pre], [dy], d)[0] for d in (torch.float32, f64))
    check(got, g32, g64, S.BAR_DGRAD, "act_bwd %s n %d" % (name, n), dim=0, block=256 * 64, group="act_bwd")
    zero = y == 0
    assert int(zero.sum()) >= 16
    expect = {"relu": 0.0, "lrelu": 0.2, "tanh": 1.0}[name]
    assert torch.equal(got.cpu()[zero & (pre == 0)], (dy * expect)[zero & (pre == 0)])


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("rows", S.AFFINE_ROWS)
def test_spec_affine(mg, mode, rows):
    M = 80
    mn, mx = S.spec(M)
    x = torch.randn(rows, M, generator=S.gen(rows + mode))
    got = mg.ops.spec_affine(dev(x), dev(mn), dev(mx), mode)
    r32, r64 = both(lambda a: S.spec_affine(a, mn, mx, mode), [x])
    check(got, r32, r64, S.BAR_ELEM if mode < 3 else S.BAR_DGRAD, "spec_affine mode %d rows %d" % (mode, rows), dim=0, block=512,
          group="spec_affine")
    from mixgan_tts_amd import autograd as A
    xa = dev(x).requires_grad_()
    y = A.spec_affine(xa, dev(mn), dev(mx), mode % 2 == 1)
    y.sum().backward()
    r, r64 = both(lambda a: S.spec_affine(a, mn, mx, 3 if mode % 2 else 4), [torch.ones_like(x)])
    check(xa.grad, r, r64, S.BAR_DGRAD, "  autograd.spec_affine norm %d" % (mode % 2), group="spec_affine")


@pytest.mark.parametrize("B,C,L", S.GATE_SHAPES)
def test_gate_bwd(mg, B, C, L):
    g = S.gen(B * C * L)
    z, dg = torch.randn(B, 2 * C, L, generator=g) * 2, torch.randn(B, C, L, generator=g)
    sig, tnh = torch.sigmoid(z[:, :C].double()).float(), torch.tanh(z[:, C:].double()).float()
    got = mg.ops.gate_bwd(dev(dg), dev(sig), dev(tnh))
    g32, g64 = (S.grads(S.gate, [z], [dg], d)[0] for d in (torch.float32, f64))
    check(got, g32, g64, S.BAR_DGRAD, "gate_bwd %s" % ((B, C, L),), dim=2, group="gate_bwd")


@pytest.mark.parametrize("n", S.MISH_N)
def test_mish_forward_and_backward(mg, n):
    g = S.gen(n)
    x, gy = torch.randn(n, generator=g) * 4, torch.randn(n, generator=g)
    x[:4] = torch.tensor([0.0, 19.99, 20.01, -30.0])      # softplus switches form at 20
    got = mg.ops.mish_fwd(dev(x))
    r32, r64 = both(S.mish, [x])
    check(got, r32, r64, S.BAR_ELEM, "mish_fwd n %d" % n, dim=0, block=256 * 64, group="mish")
    gx = mg.ops.mish_bwd(dev(gy), dev(x))
    g32, g64 = (S.grads(S.mish, [x], [gy], d)[0] for d in (torch.float32, f64))
    check(gx, g32, g64, S.BAR_DGRAD, "mish_bwd n %d" % n, dim=0, block=256 * 64, group="mish")
    from mixgan_tts_amd import autograd as A
    xa = dev(x).requires_grad_()
    (A.mish(xa) * dev(gy)).sum().backward()
    check_equal(xa.grad, gx.cpu(), "  autograd.mish is mish_bwd", "mish")


@pytest.mark.parametrize("rows,Lin,s,Lup", S.UPS_CASES)
@pytest.mark.parametrize("slope", [1.0, 0.1])
def test_upsample_zero(mg, rows, Lin, s, Lup, slope):
    x = torch.randn(1, rows, Lin, generator=S.gen(Lin + s))
    x[0, 0, 0] = 0.0
    got = mg.ops.upsample_zero(dev(x), s, Lup, slope)
    r32, r64 = both(lambda a: S.upsample_zero(a, s, Lup, slope), [x])
    what = "upsample_zero rows %d Lin %d s %d Lup %d slope %g" % (rows, Lin, s, Lup, slope)
    if slope == 1.0:
        check_equal(got, r32, what, "upsample_zero")
    else:
        check(got, r32, r64, S.BAR_ELEM, what, dim=2, block=64 * s, group="upsample_zero")
        assert torch.equal(got.cpu() == 0, r32 == 0), what + ": zeros are not where the reference has them"


@pytest.mark.parametrize("B,L,M", S.TRACE_SHAPES)
def test_diffuse_trace_bwd(mg, B, L, M):
    buf = S.schedule(M=M)
    p = S.trace_inputs(B, L, M)
    fp, Lb = mg._lib.fptr, mg.lib()
    gd, xd, mn, mx, sac = (dev(v) for v in (p["g"], p["x"], buf["spec_min"], buf["spec_max"], buf["sqrt_alphas_cumprod"]))
    for keep in (p["keep"], None):
        dx = torch.empty(B, L, M, device="cuda")
        kd = dev(keep)
        rc = Lb.mg_diffuse_trace_bwd(fp(gd), fp(xd), fp(mn), fp(mx), mg._lib.iptr(kd, torch.uint8, True), fp(sac), fp(dx),
                                     S.T_STEPS, B, L, M, mg._lib.stream_ptr())
        assert rc == 0
        fn = lambda a: S.diffuse_trace(buf, a, keep, p["noises"])            # noqa: E731
        g32, g64 = (S.grads(fn, [p["x"]], [p["g"]], d)[0] for d in (torch.float32, f64))
        check(dx, g32, g64, S.BAR_DGRAD, "diffuse_trace_bwd %s keep %d" % ((B, L, M), keep is not None), dim=1, group="diffuse_trace_bwd")
        if keep is not None:
            assert bool((dx.cpu()[(keep == 0)[:, :, None].expand(B, L, M)] == 0).all())


@pytest.mark.parametrize("n", S.LOSS_N)
def test_loss_sum_and_grad(mg, n):
    from mixgan_tts_amd.losses import _MseConstFn, _L1Fn
    a, b, _ = S.loss_inputs(n)
    up = torch.tensor(0.7)
    for mode, c in ((0, 0.7), (1, 0.0)):
        ad = dev(a).requires_grad_()
        val = _MseConstFn.apply(ad, c) if mode == 0 else _L1Fn.apply(ad, dev(b))
        (val * dev(up)).backward()
        fn = lambda u: S.loss_sum(u, None if mode == 0 else b.to(u.dtype), c, mode) / n     # noqa: E731
        r32, r64 = both(fn, [a])
        check(val.reshape(1), r32.reshape(1), r64.reshape(1), S.BAR_RED, "loss_sum mode %d n %d" % (mode, n), group="loss_sum / loss_grad")
        g32, g64 = (S.grads(fn, [a], [up], d)[0] for d in (torch.float32, f64))
        check(ad.grad, g32, g64, S.BAR_DGRAD, "loss_grad mode %d n %d" % (mode, n), dim=0, block=256 * 64, group="loss_sum / loss_grad")
        if mode == 1:
            tie = a == b
            assert int(tie.sum()) >= 16 and bool((ad.grad.cpu()[tie] == 0).all())


@pytest.mark.parametrize("B,L,M", S.MEL_CASES)
def test_mel_l1(mg, B, L, M):
    from mixgan_tts_amd import losses
    pred, target, pad, _ = S.mel_inputs(B, L, M)
    up = torch.tensor(1.3)
    num64, den64 = S.mel_l1_terms(pred.double(), target.double(), pad)
    rows = losses.mel_count_rows(dev(target), dev(pad))
    assert int(rows.item()) * M == int(den64.item()), (int(rows.item()), int(den64.item()))
    assert int(losses.mel_count_rows(dev(target), None).item()) == int((target.abs().sum(-1) != 0).sum())
    for den in (None, torch.tensor(3.0 * float(den64))):
        pd = dev(pred).requires_grad_()
        val = losses.get_mel_loss(pd, dev(target), dev(pad), None if den is None else dev(den))
        (val * dev(up)).backward()

        def fn(u):
            nu, de = S.mel_l1_terms(u, target.to(u.dtype), pad)
            return nu / (de if den is None else den.to(u.dtype))
        r32, r64 = both(fn, [pred])
        what = "mel_l1 %s den %s" % ((B, L, M), "given" if den is not None else "own")
        check(val.reshape(1), r32.reshape(1), r64.reshape(1), S.BAR_RED, what, group="mel_l1")
        g32, g64 = (S.grads(fn, [pred], [up], d)[0] for d in (torch.float32, f64))
        check(pd.grad, g32, g64, S.BAR_DGRAD, "  d pred", dim=1, group="mel_l1")
        got = pd.grad.cpu()
        assert bool((got[pad] == 0).all()) and bool((got[-1, 0] == 0).all()) and bool((got[pred == target] == 0).all())


@pytest.mark.parametrize("B,C,L", [(2, 3, 5), (2, 33, 31800)])
def test_lrelu_bwd_strided(mg, B, C, L):
    """Channel slices of wider buffers (mg_reflect_fold_bwd with no padding): 2 098 800 elements are past its 8192 x 256
    grid; x is exactly 0 at 16 places, where the slope applies as in torch."""
    Cx, Cy = C + 2, C + 3
    xb, _, _ = S.act_inputs(B * Cx * L, "lrelu")
    xb = xb.view(B, Cx, L)
    dyb = torch.randn(B, Cy, L, generator=S.gen(L))
    got = mg.ops.lrelu_bwd_strided(dev(dyb), 2 * L, Cy * L, dev(xb), L, Cx * L, B, C, L, 0.1)
    x, dy = xb[:, 1:1 + C].contiguous(), dyb[:, 2:2 + C].contiguous()
    fn = lambda a: torch.nn.functional.leaky_relu(a, 0.1)                    # noqa: E731
    g32, g64 = (S.grads(fn, [x], [dy], d)[0] for d in (torch.float32, f64))
    check(got, g32, g64, S.BAR_DGRAD, "lrelu_bwd_strided %s" % ((B, C, L),), dim=2, group="lrelu_bwd_strided")
    assert torch.equal(got.cpu()[x == 0], (dy * 0.1)[x == 0])


# ------------------------------------------------------------------------------------------------ step MLP and small linears
def test_linear_small(mg):
    from mixgan_tts_amd import autograd as A
    for B in S.LIN_B:
        for N in S.LIN_N:
            for K in S.LIN_K:
                x, W, g = S.linear_inputs(B, N, K)
                what = "linear_small B %d N %d K %d" % (B, N, K)
                out = mg.ops.linear_small_fwd(dev(x), dev(W))
                r32, r64 = both(S.linear, [x, W])
                check(out, r32, r64, S.BAR_RED, what, dim=0, block=8, group="linear_small forward")
                check_equal(mg.ops.linear_small_fwd(dev(x), dev(W)), out.cpu(), "  second run", "linear_small forward")
                dx, dW = mg.ops.linear_small_bwd(dev(g), dev(x), dev(W))
                g32, g64 = (S.grads(S.linear, [x, W], [g], d) for d in (torch.float32, f64))
                check(dx, g32[0], g64[0], S.BAR_DGRAD, "  d x", dim=0, block=8, group="linear_small backward")
                check(dW, g32[1], g64[1], S.BAR_WGRAD, "  d W", dim=1, block=64, group="linear_small backward")
                none, dW2 = mg.ops.linear_small_bwd(dev(g), dev(x), dev(W), want_dx=False)
                assert none is None
                check_equal(dW2, dW.cpu(), "  d W with want_dx=False", "linear_small backward")
                xa, Wa = dev(x).requires_grad_(), dev(W).requires_grad_()
                oa = A.linear_small(xa, Wa)
                (oa * dev(g)).sum().backward()
                check_equal(oa, out.cpu(), "  autograd.linear_small", "linear_small forward")
                check_equal(xa.grad, dx.cpu(), "  autograd d x", "linear_small backward")
                check_equal(Wa.grad, dW.cpu(), "  autograd d W", "linear_small backward")


@pytest.mark.parametrize("K", [256, 320])
def test_linear_small_rows_do_not_depend_on_the_batch(mg, K):
    """Row b alone gives the bits of row b inside a batch of 9 (chunks of 8 + 1), on the 16-byte form and the scalar one."""
    x, W, _ = S.linear_inputs(9, 5, K)
    xd, Wd = dev(x), dev(W)
    full = mg.ops.linear_small_fwd(xd, Wd).cpu()
    for b in range(9):
        check_equal(mg.ops.linear_small_fwd(xd[b:b + 1], Wd)[0], full[b], "linear_small K %d row %d alone" % (K, b), "linear_small forward")
    check_equal(mg.ops.linear_small_fwd(xd[:8], Wd), full[:8], "  first 8 rows", "linear_small forward")


@pytest.mark.parametrize("which", ["W", "x", "both"])
def test_linear_small_misaligned_views_are_realigned(mg, which):
    """K % 256 == 0 reads 16 bytes at a time: a weight or an input 1 float into its storage gives the bits of its aligned
    copy through ops (which copies), and the entry point itself refuses it."""
    x, W, _ = S.linear_inputs(9, 5, 256)
    aligned = mg.ops.linear_small_fwd(dev(x), dev(W)).cpu()
    xv = offset_view(x) if which in ("x", "both") else dev(x)
    Wv = offset_view(W) if which in ("W", "both") else dev(W)
    check_equal(mg.ops.linear_small_fwd(xv, Wv), aligned, "linear_small, %s 1 float into its storage" % which, "linear_small forward")
    out = torch.full((9, 5), 7.0).cuda()
    fp = mg._lib.fptr
    assert mg.lib().mg_linear_small_fwd(fp(xv), fp(Wv), fp(out), 9, 5, 256, mg._lib.stream_ptr()) == mg._lib.MG_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    x2, W2, _ = S.linear_inputs(9, 5, 320)                 # the scalar form takes any 4-byte aligned pointer
    check_equal(mg.ops.linear_small_fwd(offset_view(x2), offset_view(W2)), mg.ops.linear_small_fwd(dev(x2), dev(W2)).cpu(),
                "linear_small K 320 from offset views", "linear_small forward")


@pytest.mark.parametrize("D", [256, 6])
def test_step_embed(mg, D):
    t = torch.tensor(S.MLP_T + (0, 1, 99, 999, 500))
    got = mg.ops.step_embed(dev(t), dev(S.frequencies(D)))
    ref = S.step_embedding(t, D, f64)
    check(got, ref.float(), ref, S.BAR_ELEM, "step_embed D %d" % D, dim=0, block=8, group="step_embed / step_mlp")


@pytest.mark.parametrize("D0,D1,D2", S.MLP_DIMS)
@pytest.mark.parametrize("B", [1, 8, 9])
def test_step_mlp(mg, D0, D1, D2, B):
    from mixgan_tts_amd import autograd as A
    t, W0, W2, g = S.mlp_inputs(D0, D1, D2, B)
    freq = dev(S.frequencies(D0))
    out, emb, pre, h = mg.ops.step_mlp_fwd(dev(t), freq, dev(W0), dev(W2))
    what = "step_mlp %s B %d" % ((D0, D1, D2), B)
    r32, r64 = both(lambda a, b: S.step_mlp(t, a, b), [W0, W2])
    for name, got, i, bar in (("out", out, 0, S.BAR_RED), ("emb", emb, 1, S.BAR_ELEM), ("pre", pre, 2, S.BAR_RED), ("h", h, 3, S.BAR_RED)):
        check(got, r32[i], r64[i], bar, "%s %s" % (what, name), dim=0, block=8, group="step_embed / step_mlp")
    dW0, dW2 = mg.ops.step_mlp_bwd(dev(g), emb, pre, h, dev(W2))
    g32, g64 = (S.grads(lambda a, b: S.step_mlp(t, a, b)[0], [W0, W2], [g], d) for d in (torch.float32, f64))
    check(dW0, g32[0], g64[0], S.BAR_WGRAD, "  d W0", dim=1, block=64, group="step_embed / step_mlp")
    check(dW2, g32[1], g64[1], S.BAR_WGRAD, "  d W2", dim=1, block=64, group="step_embed / step_mlp")
    Wa, Wb = dev(W0).requires_grad_(), dev(W2).requires_grad_()
    oa = A.step_mlp(dev(t), freq, Wa, Wb)
    (oa * dev(g)).sum().backward()
    check_equal(oa, out.cpu(), "  autograd.step_mlp", "step_embed / step_mlp")
    check_equal(Wa.grad, dW0.cpu(), "  autograd d W0", "step_embed / step_mlp")
    check_equal(Wb.grad, dW2.cpu(), "  autograd d W2", "step_embed / step_mlp")
    check_equal(mg.ops.step_mlp_fwd(dev(t), freq, dev(W0), dev(W2))[0], out.cpu(), "  second run", "step_embed / step_mlp")
    if B == 9:
        for b in (0, 7, 8):
            alone = mg.ops.step_mlp_fwd(dev(t[b:b + 1]), freq, dev(W0), dev(W2))[0]
            check_equal(alone[0], out[b].cpu(), "  row %d alone" % b, "step_embed / step_mlp")
    if D0 % 256 == 0:
        off = mg.ops.step_mlp_fwd(dev(t), freq, offset_view(W0), offset_view(W2))[0]
        check_equal(off, out.cpu(), "  weights 1 float into their storage", "step_embed / step_mlp")


# ------------------------------------------------------------------------------------------------ lingops
def _nan_equal(got, ref, what):
    got = got.detach().cpu()
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), what + ": NaN not exactly where the reference has it"
    return torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(ref), ref)


@pytest.mark.parametrize("name", list(S.LING_CASES))
def test_length_regulator(mg, name):
    c = S.LING_CASES[name]
    p = S.lingops_inputs(**c)
    total = int(p["dur"].clamp(min=0).sum(1).max())
    lr = mg.lingops.LengthRegulator()
    for max_len in (None, max(1, total - 3), total + 5):
        what = "LengthRegulator %s max_len %s" % (name, max_len)
        xd = dev(p["xw"]).requires_grad_()
        out, lens = lr(xd, dev(p["dur"]), max_len)
        ref, ref_len = S.length_regulate(p["xw"], p["dur"], max_len)
        check_equal(out, ref, what, "lingops forward")
        assert torch.equal(lens.cpu(), ref_len), what
        cot = torch.randn(ref.shape, generator=S.gen(7))
        (out * dev(cot)).sum().backward()
        fn = lambda a: S.length_regulate(a, p["dur"], max_len)[0]            # noqa: E731
        g32, g64 = (S.grads(fn, [p["xw"]], [cot], d)[0] for d in (torch.float32, f64))
        check(xd.grad, g32, g64, S.BAR_DGRAD, "  d x", group="lingops backward")


@pytest.mark.parametrize("name", list(S.LING_CASES))
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_word_level_pooling(mg, name, reduce):
    c = S.LING_CASES[name]
    p = S.lingops_inputs(**c)
    w_all = int(p["swl"].clamp(max=c["Tw"]).max())
    fn = lambda a: S.word_level_pooling(a, p["src_len"], p["wb"], p["swl"], reduce)          # noqa: E731
    r32, r64 = both(fn, [p["src"]])
    assert reduce == "sum" or bool(torch.isnan(r64[0, 2]).all())
    for max_words in (None, w_all, max(1, w_all - 2)):
        what = "word_level_pooling %s %s max_words %s" % (name, reduce, max_words)
        sd = dev(p["src"]).requires_grad_()
        out = mg.lingops.word_level_pooling(sd, dev(p["src_len"]), dev(p["wb"]), dev(p["swl"]), reduce=reduce, max_words=max_words)
        W = out.shape[1]
        assert W == (w_all if max_words is None else max_words)
        got, ref = _nan_equal(out, r64[:, :W], what)
        check(got, torch.nan_to_num(r32[:, :W]), ref, S.BAR_RED, what, group="lingops forward")
        cot = torch.randn(out.shape, generator=S.gen(11))
        (out * dev(cot)).sum().backward()
        g32, g64 = (S.grads(lambda a: torch.nan_to_num(fn(a)[:, :W]), [p["src"]], [cot], d)[0] for d in (torch.float32, f64))
        check(sd.grad, g32, g64, S.BAR_DGRAD, "  d src", group="lingops backward")
        if W < w_all:                                       # phonemes of the dropped words get exactly 0
            first = p["wb"][0, :W].sum()
            assert bool((sd.grad.cpu()[0, int(first):] == 0).all()), what


@pytest.mark.parametrize("name", list(S.LING_CASES))
def test_rel_coef_and_mapping_mask(mg, name):
    c = S.LING_CASES[name]
    p = S.lingops_inputs(**c)
    dur = p["dur"].clamp(min=0)
    swl = p["swl"].clamp(max=c["Tw"])
    lens = torch.stack([dur[b, :int(swl[b])].sum() for b in range(c["B"])])
    for d, n in ((dur, lens), (p["wb"], torch.stack([p["wb"][b, :int(swl[b])].sum() for b in range(c["B"])]))):
        mask = torch.arange(int(n.max()))[None, :] < n[:, None]
        got, ref = _nan_equal(mg.lingops.get_rel_coef(dev(d), dev(swl), dev(mask)), S.rel_coef(d, swl, mask), "rel_coef " + name)
        check_equal(got, ref, "rel_coef %s T %d" % (name, c["Tw"]), "lingops forward")
    Tw = min(c["Tw"], 2048)                                 # the mask holds two prefix sums in LDS
    dw, wb, sw = dur[:, :Tw].contiguous(), p["wb"][:, :Tw].contiguous(), swl.clamp(max=Tw)
    Lq, Lkv = int(dw.sum(1).max()) + 3, int(wb.sum(1).max()) + 2
    got = mg.lingops.get_mapping_mask(torch.zeros(c["B"], Lq, 1, device="cuda"), torch.zeros(c["B"], Lkv, 1, device="cuda"),
                                      dev(dw), dev(wb), dev(sw))
    check_equal(got, S.mapping_mask(Lq, Lkv, dw, wb, sw), "mapping_mask %s Tw %d" % (name, Tw), "lingops forward")
