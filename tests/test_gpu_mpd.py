"""GPU parity of the native HiFi-GAN multi-period discriminator (csrc/mpd.hip, hifigan_discriminators.py) against float64
torch on the CPU: the kernels one layer at a time against F.conv2d on the published [N, C, H, p] layout, the fold, each
DiscriminatorP at full width against hifigan_disc_ref.disc_p_forward, and the module inside VocoderGANTrainer.

Error measure: max-abs error over max-abs reference through helpers.check.  Bars: 2e-5 maps and
values, 5e-5 data gradients, 1e-4 parameter gradients and parameters; where the float32 CPU restatement's own error
against float64 exceeds bar / 8 on a tensor, that tensor's bar is 8 x that error.

Leaky-ReLU kinks: the float64 restatement adopts the GPU run's sign pattern, and hifigan_disc_ref.kink_masks asserts
what makes that sound (a flipped element has |pre64| <= 1e-4 max, flips are <= 1e-3 of a tensor).

Kernel shapes: the five real layer widths, R = N p rows with N = 3 and p in {2, 11} (row and phase stride mistakes need
more than two rows).  H_in for the stride-3 layers: 1, 4, 27, 28, 29, 190 (every residue mod 3, the one-column row, rows
that span a 64-column tile edge); for the stride-1 layers 1, 2, 20, 62.  A flat output axis of exactly 64, 65 and 129
columns (a launch ending on a tile edge; a one-column tail after a 64- and a 128-column tile) needs another R than 6 or 33:
the *_at_tile_edges cases, forward and data gradient, stride 3 (polyphase epilogue) and stride 1.  Slots are the narrowest the construction allows
(S_out = H_out + 2, S_in = stride S_out): the neighbour's live columns then sit exactly two columns from a row's edge.
With K = 5, stride 3 and padding 2 every input column is read by some output, so "positions no output reads" has no
instance at these layers; the slack columns, which must come out as exactly 0 whatever `add` holds there, do.
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import check
import hifigan_train_ref as HR
import hifigan_disc_ref as DR
import hifigan_msd_ref as MR
import test_gpu_vocoder_gan as VG      # its helpers: seeded_weights, trainer_batch, _h

pytestmark = pytest.mark.gpu
BAR_MAP, BAR_DATA, BAR_PARAM = 2e-5, 5e-5, 1e-4
SLOPE = 0.1
N = 3
LAYERS = [(32, 128, 5, 3), (128, 512, 5, 3), (512, 1024, 5, 3), (1024, 1024, 5, 1), (1024, 1, 3, 1)]   # (Ci, Co, K, stride)
H_INS = {3: [1, 4, 27, 28, 29, 190], 1: [1, 2, 20, 62]}


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def to_slots(x, S, fill=0.0):
    """Published [N, C, H, p] -> slotted [1, C, N p S]; the slack holds `fill`."""
    n, c, h, p = x.shape
    out = torch.full((c, n, p, S), fill, dtype=x.dtype)
    out[:, :, :, :h] = x.permute(1, 0, 3, 2)
    return out.reshape(1, c, n * p * S)


def from_slots(buf, n, p, S, H):
    c = buf.shape[1]
    return buf.reshape(c, n, p, S).permute(1, 0, 3, 2)[:, :, :H]


def slack_of(buf, n, p, S, H):
    return buf.reshape(buf.shape[1], n, p, S)[:, :, :, H:]


def lrelu_like(pre, product):
    masks = DR.kink_masks({"x": product}, {"x": pre.double()})
    return DR.lrelu(pre, SLOPE, "x", None, masks)


# ------------------------------------------------------------------------------------------------------------------
# 1: one layer at a time.  One float64 / float32 reference per case, shared by the forward and the backward test.
# ------------------------------------------------------------------------------------------------------------------
_cases = {}


def layer_case(layer, p, H_in, n=N):
    key = (layer, p, H_in, n)
    if key in _cases:
        return _cases[key]
    ci, co, K, s = layer
    H_out = (H_in - 1) // s + 1
    S_out = H_out + 2
    S_in = s * S_out
    gen = torch.Generator().manual_seed(100000 * ci + 1000 * p + 10 * H_in + s)
    x = torch.randn(n, ci, H_in, p, generator=gen)
    w = torch.randn(co, ci, K, generator=gen) / (ci * K) ** 0.5
    b = 0.1 * torch.randn(co, generator=gen)
    cot = torch.randn(n, co, H_out, p, generator=gen)
    below = torch.randn(n, ci, H_in, p, generator=gen)       # the layer below's stored map: only its signs matter
    add = torch.randn(n, ci, H_in, p, generator=gen)
    res = {"in": (x, w, b, cot, below, add), "geo": (H_out, S_in, S_out)}
    for dt in (torch.float64, torch.float32):
        x_, w_, b_ = (t.to(dt).requires_grad_() for t in (x, w, b))
        pre = F.conv2d(x_, w_[..., None], b_, stride=(s, 1), padding=((K - 1) // 2, 0))
        assert pre.shape[2] == H_out
        (pre * cot.to(dt)).sum().backward()
        mask = torch.where(below > 0, 1.0, SLOPE).to(dt)
        res[dt] = {"pre": pre.detach(), "dx": x_.grad, "dx_masked": (x_.grad + add.to(dt)) * mask, "dw": w_.grad,
                   "db": b_.grad}
    _cases[key] = res
    return res


CASES = [(l, p, h) for l in LAYERS for p in (2, 11) for h in H_INS[l[3]]]
IDS = ["%dto%d_k%ds%d-p%d-H%d" % (l + (p, h)) for l, p, h in CASES]


def run_layer_forward(mg, layer, p, H_in, n=N):
    ci, co, K, s = layer
    c = layer_case(layer, p, H_in, n)
    H_out, S_in, S_out = c["geo"]
    x, w, b = c["in"][:3]
    R = n * p
    xs, wc, bc = to_slots(x, S_in).cuda(), w.cuda(), b.cuda()
    r64, r32 = c[torch.float64], c[torch.float32]
    pre = mg.ops.period_conv_fwd(xs, wc, bc, R, S_in, S_out, H_out, s)
    assert tuple(pre.shape) == (1, co, R * S_out)
    check(from_slots(pre, n, p, S_out, H_out), r32["pre"], r64["pre"], BAR_MAP, "forward, no activation")
    assert bool((slack_of(pre, n, p, S_out, H_out) == 0.0).all()), "slack columns must be exactly 0"
    act = mg.ops.period_conv_fwd(xs, wc, bc, R, S_in, S_out, H_out, s, slope=SLOPE)
    got = from_slots(act, n, p, S_out, H_out)
    check(got, lrelu_like(r32["pre"], got), lrelu_like(r64["pre"], got), BAR_MAP, "forward + leaky ReLU")
    assert bool((slack_of(act, n, p, S_out, H_out) == 0.0).all())
    nob = mg.ops.period_conv_fwd(xs, wc, None, R, S_in, S_out, H_out, s)
    check(from_slots(nob, n, p, S_out, H_out), r32["pre"] - b.view(1, -1, 1, 1), r64["pre"] - b.double().view(1, -1, 1, 1),
          BAR_MAP, "forward, no bias")
    assert bool((slack_of(nob, n, p, S_out, H_out) == 0.0).all())
    # unsplit reduction: same values up to summation order; a second run of each gives the same bits
    uns = mg.ops.period_conv_fwd(xs, wc, bc, R, S_in, S_out, H_out, s, split=False)
    check(from_slots(uns, n, p, S_out, H_out), r32["pre"], r64["pre"], BAR_MAP, "forward, reduction not split")
    assert torch.equal(mg.ops.period_conv_fwd(xs, wc, bc, R, S_in, S_out, H_out, s), pre)
    assert torch.equal(mg.ops.period_conv_fwd(xs, wc, bc, R, S_in, S_out, H_out, s, split=False), uns)


def run_layer_backward(mg, layer, p, H_in, n=N):
    ci, co, K, s = layer
    c = layer_case(layer, p, H_in, n)
    H_out, S_in, S_out = c["geo"]
    x, w, b, cot, below, add = c["in"]
    R = n * p
    r64, r32 = c[torch.float64], c[torch.float32]
    xs, wc, ds = to_slots(x, S_in).cuda(), w.cuda(), to_slots(cot, S_out).cuda()
    dx = mg.ops.period_conv_dgrad(ds, wc, R, S_in, H_in, S_out, s)
    assert tuple(dx.shape) == (1, ci, R * S_in)
    check(from_slots(dx, n, p, S_in, H_in), r32["dx"], r64["dx"], BAR_DATA, "dx")
    assert bool((slack_of(dx, n, p, S_in, H_in) == 0.0).all()), "slack columns must be exactly 0"
    ms, as_ = to_slots(below, S_in).cuda(), to_slots(add, S_in, fill=3.0).cuda()      # add's slack must not leak through
    dxm = mg.ops.period_conv_dgrad(ds, wc, R, S_in, H_in, S_out, s, map=ms, add=as_, slope=SLOPE)
    check(from_slots(dxm, n, p, S_in, H_in), r32["dx_masked"], r64["dx_masked"], BAR_DATA, "(dx + add) * mask")
    assert bool((slack_of(dxm, n, p, S_in, H_in) == 0.0).all())
    uns = mg.ops.period_conv_dgrad(ds, wc, R, S_in, H_in, S_out, s, map=ms, add=as_, slope=SLOPE, split=False)
    check(from_slots(uns, n, p, S_in, H_in), r32["dx_masked"], r64["dx_masked"], BAR_DATA, "(dx + add) * mask, not split")
    pad = (K - 1) // 2
    dw = mg.ops.conv1d_wgrad(ds, xs, K, s, pad)
    check(dw, r32["dw"], r64["dw"], BAR_PARAM, "dw on slotted operands")
    db = mg.ops.rowsum(ds)
    check(db, r32["db"], r64["db"], BAR_PARAM, "db on slotted operands")
    # fixed summation order: a second run gives the same bits
    assert torch.equal(mg.ops.conv1d_wgrad(ds, xs, K, s, pad), dw)
    assert torch.equal(mg.ops.rowsum(ds), db)
    assert torch.equal(mg.ops.period_conv_dgrad(ds, wc, R, S_in, H_in, S_out, s, map=ms, add=as_, slope=SLOPE), dxm)
    assert torch.equal(mg.ops.period_conv_dgrad(ds, wc, R, S_in, H_in, S_out, s), dx)


@pytest.mark.parametrize("layer,p,H_in", CASES, ids=IDS)
def test_layer_forward(mg, layer, p, H_in):
    run_layer_forward(mg, layer, p, H_in)


@pytest.mark.parametrize("layer,p,H_in", CASES, ids=IDS)
def test_layer_backward(mg, layer, p, H_in):
    run_layer_backward(mg, layer, p, H_in)


# A flat output axis of exactly 64, 65 and 129 columns: a launch that ends on a tile edge, and launches with a one-column
# tail after a 64- and after a 128-column tile.  R = 6 or 33 cannot give these (6 S and 33 S never equal them), so these
# cases take another R = n p: (n, p, H_out) = (2, 2, 14): 4 x 16; (1, 5, 11): 5 x 13; (1, 3, 41): 3 x 43.  At stride 3 the
# polyphase data gradient's GEMM has that same column count (its u = 3 epilogue writes 192, 195 and 387 columns); at
# stride 1 input and output axes are equal.
EDGE_GEO = [(2, 2, 14, 40), (1, 5, 11, 32), (1, 3, 41, 123)]      # (n, p, H_out, an H_in that gives it at stride 3)
EDGE_LAYERS = [(32, 128, 5, 3), (128, 512, 5, 3), (1024, 1024, 5, 1), (1024, 1, 3, 1)]
EDGE = [(l, n, p, (h3 if l[3] == 3 else ho), n * p * (ho + 2)) for l in EDGE_LAYERS for n, p, ho, h3 in EDGE_GEO]
EDGE_IDS = ["%dto%d_k%ds%d-Lout%d" % (l + (lout,)) for l, n, p, h, lout in EDGE]


@pytest.mark.parametrize("layer,n,p,H_in,Lout", EDGE, ids=EDGE_IDS)
def test_layer_forward_at_tile_edges(mg, layer, n, p, H_in, Lout):
    assert Lout in (64, 65, 129) and layer_case(layer, p, H_in, n)["geo"][2] * n * p == Lout
    run_layer_forward(mg, layer, p, H_in, n)


@pytest.mark.parametrize("layer,n,p,H_in,Lout", EDGE, ids=EDGE_IDS)
def test_layer_backward_at_tile_edges(mg, layer, n, p, H_in, Lout):
    assert Lout in (64, 65, 129) and layer_case(layer, p, H_in, n)["geo"][2] * n * p == Lout
    run_layer_backward(mg, layer, p, H_in, n)


def test_first_layer_through_the_generic_kernel(mg):
    """1 -> 32 at stride 3, the layer the fold feeds: one input channel padded to a 16-channel chunk, three GEMM rows in
    the polyphase data gradient."""
    layer = (1, 32, 5, 3)
    for p, H_in in ((2, 190), (11, 29)):
        c = layer_case(layer, p, H_in)
        H_out, S_in, S_out = c["geo"]
        x, w, b, cot, _, _ = c["in"]
        R = N * p
        r64, r32 = c[torch.float64], c[torch.float32]
        xs, ds = to_slots(x, S_in).cuda(), to_slots(cot, S_out).cuda()
        pre = mg.ops.period_conv_fwd(xs, w.cuda(), b.cuda(), R, S_in, S_out, H_out, 3)
        check(from_slots(pre, N, p, S_out, H_out), r32["pre"], r64["pre"], BAR_MAP, "first layer forward")
        dx = mg.ops.period_conv_dgrad(ds, w.cuda(), R, S_in, H_in, S_out, 3)
        check(from_slots(dx, N, p, S_in, H_in), r32["dx"], r64["dx"], BAR_DATA, "first layer dx")
        assert bool((slack_of(dx, N, p, S_in, H_in) == 0.0).all())
        check(mg.ops.conv1d_wgrad(ds, xs, 5, 3, 2), r32["dw"], r64["dw"], BAR_PARAM, "first layer dw")


# ------------------------------------------------------------------------------------------------------------------
# 2: the fold
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", DR.PERIODS)
def test_fold(mg, p):
    for T in (p, 2 * p + 1, 3 * p, 81 * p + 1, 700):
        gen = torch.Generator().manual_seed(1000 * p + T)
        y = torch.randn(N, 1, T, generator=gen)
        H, S = mg.ops.period_geometry(T, p)
        ref = {}
        for dt in (torch.float64, torch.float32):
            y_ = y.to(dt).requires_grad_()
            v = F.pad(y_, (0, p - T % p), "reflect") if T % p else y_
            v = v.view(N, 1, v.shape[2] // p, p)
            assert v.shape[2] == H[0]
            cot = torch.randn(v.shape, generator=torch.Generator().manual_seed(T)).to(dt)
            (v * cot).sum().backward()
            ref[dt] = (v.detach(), y_.grad, cot)
        in0 = mg.ops.period_fold_fwd(y.cuda(), p)
        assert tuple(in0.shape) == (1, 1, N * p * S[0])
        assert torch.equal(from_slots(in0, N, p, S[0], H[0]).cpu(), ref[torch.float32][0]), (p, T)
        assert bool((slack_of(in0, N, p, S[0], H[0]) == 0.0).all())
        cs = to_slots(ref[torch.float32][2], S[0], fill=5.0).cuda()       # the backward reads live columns only
        dy = mg.ops.period_fold_bwd(cs, N, T, p)
        assert tuple(dy.shape) == (N, 1, T)
        check(dy, ref[torch.float32][1], ref[torch.float64][1], BAR_DATA, "fold backward p %d T %d" % (p, T))
        assert torch.equal(mg.ops.period_fold_bwd(cs, N, T, p), dy)


# ------------------------------------------------------------------------------------------------------------------
# 3: DiscriminatorP at full width, N = 2 + 2
# ------------------------------------------------------------------------------------------------------------------
_full = {}


def full_case(mg, pi, T):
    """The product's two runs (D phase: parameters trainable, y_hat detached, discriminator_loss; G phase: parameters
    frozen, generator_loss + feature_loss to y_hat) from one state, and ONE float64 and one float32 reference forward
    under the product's sign pattern, differentiated twice."""
    key = (pi, T)
    if key in _full:
        return _full[key]
    p = DR.PERIODS[pi]
    prefix = "discriminators.%d." % pi
    W = {k: v for k, v in DR.mpd_init(40 + pi).items() if k.startswith(prefix)}
    gen = torch.Generator().manual_seed(100 * p + T)
    y, y_hat = torch.randn(2, 1, T, generator=gen), torch.randn(2, 1, T, generator=gen)
    runs = {}
    for name in ("d_phase", "g_phase"):
        net = mg.DiscriminatorP(p)
        net.load_state_dict({k[len(prefix):]: v.clone() for k, v in W.items()}, strict=True)
        net = net.cuda().train()
        yh = y_hat.cuda()
        if name == "g_phase":
            for q in net.parameters():
                q.requires_grad_(False)
            yh.requires_grad_()
        logits, fmap = net(torch.cat([y.cuda(), yh], 0))
        if name == "d_phase":
            loss = mg.hifigan_discriminator_loss([logits[:2]], [logits[2:]])[0]
        else:
            loss = mg.hifigan_generator_loss([logits[2:]])[0] + mg.hifigan_feature_loss([[f[:2] for f in fmap]],
                                                                                        [[f[2:] for f in fmap]])
        loss.backward()
        runs[name] = {"net": net, "logits": logits.detach().cpu(), "fmap": [f.detach().cpu() for f in fmap], "y_hat": yh,
                      "loss": loss.detach().cpu()}
    taps = {prefix + "convs.%d" % j: runs["d_phase"]["fmap"][j] for j in range(5)}
    ref, masks = {}, None
    for dt in (torch.float64, torch.float32):
        Wd = {k: v.to(dt, copy=True).requires_grad_() for k, v in W.items()}
        yh_ = y_hat.to(dt).requires_grad_()
        x = torch.cat([y.to(dt), yh_], 0)
        if masks is None:
            own = {}
            with torch.no_grad():
                DR.disc_p_forward(Wd, prefix, x, p, taps=own)
            masks = DR.kink_masks(taps, own)
        logits, fmap = DR.disc_p_forward(Wd, prefix, x, p, masks=masks)
        loss_d = DR.discriminator_loss([logits[:2]], [logits[2:]])[0]
        loss_g = DR.generator_loss([logits[2:]])[0] + DR.feature_loss([[f[:2] for f in fmap]], [[f[2:] for f in fmap]])
        names = list(Wd)
        dW = dict(zip(names, torch.autograd.grad(loss_d, [Wd[k] for k in names], retain_graph=True)))
        dy_hat, = torch.autograd.grad(loss_g, [yh_])
        ref[dt] = {"logits": logits.detach(), "fmap": [f.detach() for f in fmap], "dW": dW, "dy_hat": dy_hat,
                   "loss_d": loss_d.detach(), "loss_g": loss_g.detach()}
    _full[key] = {"runs": runs, "ref": ref, "prefix": prefix, "p": p}
    return _full[key]


FULL = [(pi, T) for pi in range(5) for T in (700, 2083)]
FULL_IDS = ["p%d-T%d" % (DR.PERIODS[pi], T) for pi, T in FULL]


@pytest.mark.parametrize("pi,T", FULL, ids=FULL_IDS)
def test_discriminator_p_forward(mg, pi, T):
    c = full_case(mg, pi, T)
    r64, r32 = c["ref"][torch.float64], c["ref"][torch.float32]
    H, _ = mg.ops.period_geometry(T, c["p"])
    for name in ("d_phase", "g_phase"):
        run = c["runs"][name]
        assert tuple(run["logits"].shape) == (4, H[6] * c["p"]) and len(run["fmap"]) == 6
        check(run["logits"], r32["logits"], r64["logits"], BAR_MAP, "%s: logits" % name)
        for j, (got, a32, a64) in enumerate(zip(run["fmap"], r32["fmap"], r64["fmap"])):
            assert tuple(got.shape) == tuple(a64.shape) == (4, DR.MPD_CHANNELS[j + 1] if j < 5 else 1, H[j + 1], c["p"])
            check(got, a32, a64, BAR_MAP, "%s: map %d" % (name, j))
    check(c["runs"]["d_phase"]["loss"].reshape(1), r32["loss_d"].reshape(1), r64["loss_d"].reshape(1), BAR_MAP, "D loss")
    check(c["runs"]["g_phase"]["loss"].reshape(1), r32["loss_g"].reshape(1), r64["loss_g"].reshape(1), BAR_MAP, "G loss")
    # the two runs saw the same inputs and state: same bits
    assert torch.equal(c["runs"]["d_phase"]["logits"], c["runs"]["g_phase"]["logits"])
    for a, b in zip(c["runs"]["d_phase"]["fmap"], c["runs"]["g_phase"]["fmap"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("pi,T", FULL, ids=FULL_IDS)
def test_discriminator_p_parameter_gradients(mg, pi, T):
    c = full_case(mg, pi, T)
    r64, r32 = c["ref"][torch.float64], c["ref"][torch.float32]
    run = c["runs"]["d_phase"]
    assert run["y_hat"].grad is None
    names = [k for k, _ in run["net"].named_parameters()]
    assert len(names) == 18
    for k, q in run["net"].named_parameters():
        assert q.grad is not None, k
        check(q.grad, r32["dW"][c["prefix"] + k], r64["dW"][c["prefix"] + k], BAR_PARAM, "d / d " + k)


@pytest.mark.parametrize("pi,T", FULL, ids=FULL_IDS)
def test_discriminator_p_input_gradient_with_frozen_parameters(mg, pi, T):
    c = full_case(mg, pi, T)
    r64, r32 = c["ref"][torch.float64], c["ref"][torch.float32]
    run = c["runs"]["g_phase"]
    assert all(q.grad is None for q in run["net"].parameters()), "frozen parameters get no gradient"
    check(run["y_hat"].grad, r32["dy_hat"], r64["dy_hat"], BAR_DATA, "d / d y_hat")


def test_discriminator_p_partly_frozen_backward_stops_above_layer_0(mg):
    """DiscriminatorP(2) at the shortest FULL case with convs.0 and convs.1 frozen, an input that does not require grad
    and a loss on one middle map plus the logits: the walk down the stack starts at a map with an outside gradient and
    stops at layer 2.  The layers above run the same kernels on the same data as with nothing frozen, and those kernels
    have fixed summation orders, so their parameter gradients are the same bits."""
    pi, T = FULL[0]
    p, prefix = DR.PERIODS[pi], "discriminators.%d." % pi
    W = {k[len(prefix):]: v for k, v in DR.mpd_init(40 + pi).items() if k.startswith(prefix)}
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(4, 1, T, generator=gen).cuda()
    cots = None
    nets = {}
    for name in ("all", "frozen"):
        net = mg.DiscriminatorP(p)
        net.load_state_dict({k: v.clone() for k, v in W.items()}, strict=True)
        net = net.cuda().train()
        if name == "frozen":
            for q in [*net.convs[0].parameters(), *net.convs[1].parameters()]:
                q.requires_grad_(False)
        logits, fmap = net(x)
        if cots is None:
            cots = [torch.randn(t.shape, generator=gen).cuda() for t in (fmap[3], logits)]
        ((fmap[3] * cots[0]).sum() + (logits * cots[1]).sum()).backward()
        nets[name] = net
    assert x.grad is None
    full = dict(nets["all"].named_parameters())
    for k, q in nets["frozen"].named_parameters():
        if k.startswith(("convs.0.", "convs.1.")):
            assert q.grad is None, "frozen %s got a gradient" % k
        else:
            assert q.grad is not None and torch.equal(q.grad, full[k].grad), k
    assert all(q.grad is not None for q in full.values())


# ------------------------------------------------------------------------------------------------------------------
# 4: MultiPeriodDiscriminator
# ------------------------------------------------------------------------------------------------------------------
def test_multi_period_structure_and_state_dict_round_trip(mg):
    W = DR.mpd_init(51)
    net = mg.MultiPeriodDiscriminator()
    net.load_state_dict({k: v.clone() for k, v in W.items()}, strict=True)
    net = net.cuda()
    T = 700
    gen = torch.Generator().manual_seed(52)
    y, y_hat = torch.randn(2, 1, T, generator=gen).cuda(), torch.randn(2, 1, T, generator=gen).cuda()
    with torch.no_grad():
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = net(y, y_hat)
    assert len(y_d_rs) == len(y_d_gs) == len(fmap_rs) == len(fmap_gs) == 5
    for i, p in enumerate(DR.PERIODS):
        H, _ = mg.ops.period_geometry(T, p)
        assert tuple(y_d_rs[i].shape) == tuple(y_d_gs[i].shape) == (2, H[6] * p)
        assert len(fmap_rs[i]) == len(fmap_gs[i]) == 6
        for j in range(6):
            shape = (2, DR.MPD_CHANNELS[j + 1] if j < 5 else 1, H[j + 1], p)
            assert tuple(fmap_rs[i][j].shape) == tuple(fmap_gs[i][j].shape) == shape
    # the halves are the two halves of one batch: period 3 alone on [y; y_hat] gives the same bits
    logits, _ = net.discriminators[1](torch.cat([y, y_hat], 0))
    assert torch.equal(logits[:2], y_d_rs[1]) and torch.equal(logits[2:], y_d_gs[1])
    sd = net.state_dict()
    assert set(sd) == set(DR.mpd_keys()) and all(v.is_cuda for v in sd.values())
    for k, v in W.items():
        assert torch.equal(sd[k].cpu(), v), k
    other = mg.MultiPeriodDiscriminator().cuda()
    other.load_state_dict(sd, strict=True)
    with torch.no_grad():
        again = other(y, y_hat)
    for a, b in zip(again[0] + again[1], y_d_rs + y_d_gs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------
# 5: in the trainer, beside the native generator and the native multi-scale discriminator
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stft(mg):
    return mg.audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)


def test_trainer_sgd_two_steps_match_float64(mg, manifest, stft):
    """VocoderGANTrainer over the native generator, the native MPD and the native MSD against the float64 chain
    (hifigan_train_ref + hifigan_disc_ref + hifigan_msd_ref), with the batch and learning rates of
    test_gpu_vocoder_gan's trainer test: the five scalars of two SGD steps and the post-step parameters of all three."""
    LR, LR_D = 1e-5, 1e-3
    Wg, Wp, Wm = VG.seeded_weights(manifest), DR.mpd_init(61), MR.msd_init(62)
    Gn = mg.vocoder.Generator(VG._h())
    Gn.load_state_dict({k: v.detach().clone() for k, v in Wg.items()})
    mpd, msd = mg.MultiPeriodDiscriminator(), mg.MultiScaleDiscriminator()
    mpd.load_state_dict({k: v.clone() for k, v in Wp.items()}, strict=True)
    msd.load_state_dict({k: v.clone() for k, v in Wm.items()}, strict=True)
    tr = mg.VocoderGANTrainer(Gn.cuda(), stft, {"mpd": mpd.cuda(), "msd": msd.cuda()}, optimizer=torch.optim.SGD, lr=LR)
    for group in tr.optim_d.param_groups:
        group["lr"] = LR_D
    mel, wav = VG.trainer_batch()
    win, basis = stft.stft_fn._tables.window.double(), stft.mel_basis.double().cpu()
    bufs = {"mpd": set(), "msd": set(MR.buffer_names())}      # scale 0's u / v; the MPD has parameters of the same names
    fwd = {"mpd": DR.mpd_forward, "msd": MR.msd_forward}

    def to_state(Wd, dt, n):
        return {k: (v.to(dt, copy=True) if k in bufs[n] else v.detach().to(dt, copy=True).requires_grad_())
                for k, v in Wd.items()}

    state = {dt: {"g": {k: v.detach().to(dt, copy=True).requires_grad_() for k, v in Wg.items()},
                  "mpd": to_state(Wp, dt, "mpd"), "msd": to_state(Wm, dt, "msd")} for dt in (torch.float64, torch.float32)}
    got, ref = [], {torch.float64: [], torch.float32: []}
    for step in range(2):
        taps = {}
        got.append(tr.step(mel.cuda(), wav.cuda(), taps=taps))
        for dt, st in state.items():
            y = wav.to(dt)[:, None, :]
            first = dt == torch.float64
            discs = {n: (fwd[n], st[n]) for n in ("mpd", "msd")}
            params = [v for n in discs for k, v in st[n].items() if k not in bufs[n]]

            def dry(st=st):      # the sign-finding passes must not advance the spectral-norm buffers
                return {"mpd": (fwd["mpd"], st["mpd"]), "msd": (fwd["msd"], MR.clone_buffers(st["msd"]))}

            if first:
                own_g, own_d = {}, {}
                with torch.no_grad():
                    y_own = HR.generator_forward(st["g"], mel.to(dt), taps=own_g)
                    DR.d_phase_loss(dry(), y, y_own, taps=own_d)
                masks = {"generator": DR.kink_masks(taps["generator"], own_g),
                         "d": {n: DR.kink_masks(DR.taps_of_fmaps("discriminators", *taps["d"][n]), own_d[n]) for n in discs}}
            y_hat = HR.generator_forward(st["g"], mel.to(dt), masks=masks["generator"])
            for v in params:
                v.grad = None
            loss_d = DR.d_phase_loss(discs, y, y_hat, masks=masks["d"])
            loss_d.backward()
            with torch.no_grad():
                for v in params:
                    v -= LR_D * v.grad
            if first:
                own_gp = {}
                with torch.no_grad():
                    DR.g_phase_loss(dry(), y, y_hat.detach(), taps=own_gp)
                masks["g"] = {n: DR.kink_masks(DR.taps_of_fmaps("discriminators", *taps["g"][n]), own_gp[n]) for n in discs}
            for v in st["g"].values():
                v.grad = None
            for v in params:
                v.requires_grad_(False)
            adv, fm = DR.g_phase_loss(discs, y, y_hat, masks=masks["g"])
            mel_l1 = (HR.log_mel(y_hat[:, 0], win, basis) - HR.log_mel(wav.to(dt), win, basis)).abs().mean()
            loss_g = adv + fm + 45.0 * mel_l1
            loss_g.backward()
            for v in params:
                v.requires_grad_(True)
            with torch.no_grad():
                for v in st["g"].values():
                    v -= LR * v.grad
            ref[dt].append({"loss_d": loss_d.detach(), "loss_g": loss_g.detach(), "mel_l1": mel_l1.detach(),
                            "adv": adv.detach(), "fm": fm.detach()})
    r64 = ref[torch.float64]
    for i in range(2):
        assert set(got[i]) == {"loss_d", "loss_g", "mel_l1", "adv", "fm"}
        for k, v in got[i].items():
            check(v.reshape(1), ref[torch.float32][i][k].reshape(1), r64[i][k].reshape(1), BAR_MAP, "%s of step %d" % (k, i))
    for k, q in tr.generator.named_parameters():
        check(q, state[torch.float32]["g"][k], state[torch.float64]["g"][k].detach(), BAR_PARAM, "post-step G " + k)
    for n in ("mpd", "msd"):
        for k, q in tr.discriminators[n].state_dict().items():
            check(q, state[torch.float32][n][k].detach(), state[torch.float64][n][k].detach(), BAR_PARAM,
                  "post-step %s %s" % (n, k))
    assert tr.steps == 2 and all(q.requires_grad for d in tr.discriminators.values() for q in d.parameters())


def test_trainer_checkpoint_round_trip(mg, manifest, stft, tmp_path):
    """save / load go through state_dict(): a second trainer loaded from the checkpoint holds the same MPD bits and
    takes the same third step."""
    def build(seed):
        Gn = mg.vocoder.Generator(VG._h())
        Gn.load_state_dict({k: v.detach().clone() for k, v in VG.seeded_weights(manifest).items()})
        mpd = mg.MultiPeriodDiscriminator()
        mpd.load_state_dict(DR.mpd_init(seed), strict=True)
        return mg.VocoderGANTrainer(Gn.cuda(), stft, {"mpd": mpd.cuda()})

    tr = build(71)
    mel, wav = VG.trainer_batch()
    tr.step(mel.cuda(), wav.cuda())
    ck = tmp_path / "do_00000001"
    tr.save(str(ck))
    tr2 = build(72)
    assert tr2.load(str(ck)).steps == 1
    for (ka, a), (kb, b) in zip(tr.discriminators["mpd"].state_dict().items(),
                                tr2.discriminators["mpd"].state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    a, b = tr.step(mel.cuda(), wav.cuda()), tr2.step(mel.cuda(), wav.cuda())
    for k in a:
        assert torch.equal(a[k], b[k]), "second step, " + k
