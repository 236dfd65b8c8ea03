"""GPU parity of the native HiFi-GAN multi-scale discriminator (csrc/msd.hip, hifigan_discriminators.py) against float64
torch on the CPU (tests/hifigan_msd_ref.py): the kernels one shape at a time, the whole module at full width, and the
module inside VocoderGANTrainer.

Error measure: max-abs error over max-abs reference through helpers.check.  Bars: 2e-5 maps and
values, 5e-5 data gradients, 1e-4 parameter gradients and parameters; where the float32 CPU restatement's own error
against float64 exceeds bar / 8 on a tensor, that tensor's bar is 8 x that error.

Leaky-ReLU kinks: the float64 restatement adopts the GPU run's sign pattern, and hifigan_disc_ref.kink_masks asserts
what makes that sound (a flipped element has |pre64| <= 1e-4 max, flips are <= 1e-3 of a tensor).

Kernel shapes: each of the five grouped forms (Cig, Cog, K = 41, s) with G = 3 groups and N = 3 -- group and batch
stride errors need more than two of each, full G buys nothing.  Lengths: 7 (shorter than the filter: every tap partly in
padding); 64 s and 64 s + 1 (the weight gradient's 64-frame chunk; (Lin - 1) mod s zero and not); 128 s and 128 s + 1
(the forward's 128-frame tile and the data gradient's 128-sample tile); 150 s - 1 (ragged last tile, and trailing
inputs that no output reads, whose data gradient must be exactly 0).
"""
import pytest
import torch
import torch.nn.functional as F

from helpers import check
import hifigan_train_ref as HR
import hifigan_msd_ref as MR
import test_gpu_vocoder_gan as VG      # its helpers: seeded_weights, trainer_batch, _h

pytestmark = pytest.mark.gpu
BAR_MAP, BAR_DATA, BAR_PARAM = 2e-5, 5e-5, 1e-4
SLOPE = 0.1
FORMS = [(32, 32, 2), (8, 16, 2), (16, 32, 4), (32, 64, 4), (64, 64, 1)]      # (Cig, Cog, stride); K = 41, padding 20
G, N, K, PAD = 3, 3, 41, 20


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def lengths(s):
    return [7, 64 * s, 64 * s + 1, 128 * s, 128 * s + 1, 150 * s - 1]


def lrelu_like(pre, product):
    """leaky_relu(pre) with the side of every element taken from the product's activated map (slope > 0 keeps the sign)."""
    masks = MR.kink_masks({"x": product}, {"x": pre.double()})
    return MR.lrelu(pre, SLOPE, "x", None, masks)


# ------------------------------------------------------------------------------------------------------------------
# 1: the grouped kernels.  One float64 / float32 reference per (form, length), shared by the tests.
# ------------------------------------------------------------------------------------------------------------------
_cases = {}


def gconv_case(form, Lin):
    key = (form, Lin)
    if key in _cases:
        return _cases[key]
    cig, cog, s = form
    gen = torch.Generator().manual_seed(1000 * cig + 10 * s + Lin)
    x = torch.randn(N, cig * G, Lin, generator=gen)
    w = torch.randn(cog * G, cig, K, generator=gen) / (cig * K) ** 0.5
    b = 0.1 * torch.randn(cog * G, generator=gen)
    Lout = (Lin + 2 * PAD - K) // s + 1
    cot = torch.randn(N, cog * G, Lout, generator=gen)
    below = torch.randn(N, cig * G, Lin, generator=gen)       # the layer below's stored map: only its signs matter
    add = torch.randn(N, cig * G, Lin, generator=gen)
    res = {"in": (x, w, b, cot, below, add), "Lout": Lout}
    for dt in (torch.float64, torch.float32):
        x_, w_, b_ = (t.to(dt).requires_grad_() for t in (x, w, b))
        pre = F.conv1d(x_, w_, b_, stride=s, padding=PAD, groups=G)
        (pre * cot.to(dt)).sum().backward()
        mask = torch.where(below > 0, 1.0, SLOPE).to(dt)
        res[dt] = {"pre": pre.detach(), "dx": x_.grad, "dx_masked": (x_.grad + add.to(dt)) * mask, "dw": w_.grad,
                   "db": b_.grad}
    _cases[key] = res
    return res


CASES = [(f, L) for f in FORMS for L in lengths(f[2])]
IDS = ["%dx%d_s%d-L%d" % (f + (L,)) for f, L in CASES]


@pytest.mark.parametrize("form,Lin", CASES, ids=IDS)
def test_grouped_forward(mg, form, Lin):
    cig, cog, s = form
    c = gconv_case(form, Lin)
    x, w, b = (t.cuda() for t in c["in"][:3])
    packed = mg.ops.gconv_pack(w, s, G)
    r64, r32 = c[torch.float64], c[torch.float32]
    pre = mg.ops.gconv1d_fwd(x, packed, b, cog * G, K, s, PAD, G)
    assert tuple(pre.shape) == (N, cog * G, c["Lout"])
    check(pre, r32["pre"], r64["pre"], BAR_MAP, "forward, no activation")
    act = mg.ops.gconv1d_fwd(x, packed, b, cog * G, K, s, PAD, G, slope=SLOPE)
    check(act, lrelu_like(r32["pre"], act), lrelu_like(r64["pre"], act), BAR_MAP, "forward + leaky ReLU")
    nob = mg.ops.gconv1d_fwd(x, packed, None, cog * G, K, s, PAD, G)
    check(nob, r32["pre"] - c["in"][2].view(1, -1, 1), r64["pre"] - c["in"][2].double().view(1, -1, 1), BAR_MAP,
          "forward, no bias")


@pytest.mark.parametrize("form,Lin", CASES, ids=IDS)
def test_grouped_backward(mg, form, Lin):
    cig, cog, s = form
    c = gconv_case(form, Lin)
    x, w, b, cot, below, add = (t.cuda() for t in c["in"])
    r64, r32 = c[torch.float64], c[torch.float32]
    pd = mg.ops.gconv_pack(w, s, G, mg.ops.GCONV_DGRAD)
    dx = mg.ops.gconv1d_dgrad(cot, pd, cig * G, Lin, K, s, PAD, G)
    check(dx, r32["dx"], r64["dx"], BAR_DATA, "dx")
    read_to = (c["Lout"] - 1) * s + K - PAD           # inputs from here on were read by no output
    if read_to < Lin:
        assert float(r64["dx"][:, :, read_to:].abs().max()) == 0.0
        assert float(dx[:, :, read_to:].abs().max()) == 0.0, "unread trailing inputs must get exactly 0"
    dxm = mg.ops.gconv1d_dgrad(cot, pd, cig * G, Lin, K, s, PAD, G, map=below, add=add, slope=SLOPE)
    check(dxm, r32["dx_masked"], r64["dx_masked"], BAR_DATA, "(dx + add) * mask")
    dw = mg.ops.gconv1d_wgrad(cot, x, K, s, PAD, G)
    check(dw, r32["dw"], r64["dw"], BAR_PARAM, "dw")
    check(mg.ops.rowsum(cot), r32["db"], r64["db"], BAR_PARAM, "db")
    # fixed summation order: a second run gives the same bits
    assert torch.equal(mg.ops.gconv1d_wgrad(cot, x, K, s, PAD, G), dw)
    assert torch.equal(mg.ops.gconv1d_dgrad(cot, pd, cig * G, Lin, K, s, PAD, G, map=below, add=add, slope=SLOPE), dxm)


# ------------------------------------------------------------------------------------------------------------------
# 2: the first layer and the pool
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lin", [5, 64, 333, 1100])      # 1100: five 256-sample tiles of the data gradient, the last ragged
def test_first_layer(mg, Lin):
    gen = torch.Generator().manual_seed(Lin)
    x = torch.randn(N, 1, Lin, generator=gen)
    w = torch.randn(128, 1, 15, generator=gen) / 15 ** 0.5
    b = 0.1 * torch.randn(128, generator=gen)
    cot = torch.randn(N, 128, Lin, generator=gen)
    ref = {}
    for dt in (torch.float64, torch.float32):
        x_, w_, b_ = (t.to(dt).requires_grad_() for t in (x, w, b))
        pre = F.conv1d(x_, w_, b_, padding=7)
        (pre * cot.to(dt)).sum().backward()
        ref[dt] = (pre.detach(), x_.grad, w_.grad, b_.grad)
    r64, r32 = ref[torch.float64], ref[torch.float32]
    xc, wc, bc, cc = x.cuda(), w.cuda(), b.cuda(), cot.cuda()
    check(mg.ops.conv1d_c1_fwd(xc, wc, bc, 7), r32[0], r64[0], BAR_MAP, "first layer, no activation")
    act = mg.ops.conv1d_c1_fwd(xc, wc, bc, 7, slope=SLOPE)
    check(act, lrelu_like(r32[0], act), lrelu_like(r64[0], act), BAR_MAP, "first layer + leaky ReLU")
    dx = mg.ops.conv1d_c1_dgrad(cc, wc, Lin, 7)
    check(dx, r32[1], r64[1], BAR_DATA, "first layer dx")
    dw, db = mg.ops.conv1d_c1_wgrad(cc, xc, 15, 7)
    check(dw, r32[2], r64[2], BAR_PARAM, "first layer dw")
    check(db, r32[3], r64[3], BAR_PARAM, "first layer db")
    dw2, db2 = mg.ops.conv1d_c1_wgrad(cc, xc, 15, 7)
    assert torch.equal(dw2, dw) and torch.equal(db2, db) and torch.equal(mg.ops.conv1d_c1_dgrad(cc, wc, Lin, 7), dx)


@pytest.mark.parametrize("L", [1, 2, 7, 128, 333])
def test_average_pool(mg, L):
    gen = torch.Generator().manual_seed(L)
    x = torch.randn(N, 5, L, generator=gen)
    cot = torch.randn(N, 5, L // 2 + 1, generator=gen)
    ref = {}
    for dt in (torch.float64, torch.float32):
        x_ = x.to(dt).requires_grad_()
        y = F.avg_pool1d(x_, 4, 2, padding=2)
        (y * cot.to(dt)).sum().backward()
        ref[dt] = (y.detach(), x_.grad)
    y = mg.ops.avgpool4s2_fwd(x.cuda())
    assert tuple(y.shape) == (N, 5, L // 2 + 1)
    check(y, ref[torch.float32][0], ref[torch.float64][0], BAR_MAP, "pool")
    check(mg.ops.avgpool4s2_bwd(cot.cuda(), L), ref[torch.float32][1], ref[torch.float64][1], BAR_DATA, "pool backward")


# ------------------------------------------------------------------------------------------------------------------
# 3: the whole module at full width.  B = 1 (N = 2), T = 2083: scale-0 lengths 2083, 1042, 521, 131, 33, 33, 33, 33.
# ------------------------------------------------------------------------------------------------------------------
T_FULL = 2083


def flat_outputs(out):
    """The returned tensors in a fixed order: logits real, logits generated, maps real, maps generated."""
    y_d_rs, y_d_gs, fmap_rs, fmap_gs = out
    return list(y_d_rs) + list(y_d_gs) + [f for d in fmap_rs for f in d] + [f for d in fmap_gs for f in d]


def output_names():
    names = ["logits real %d" % i for i in range(3)] + ["logits gen %d" % i for i in range(3)]
    for half in ("real", "gen"):
        names += ["map %s %d.%d" % (half, i, j) for i in range(3) for j in range(8)]
    return names


@pytest.fixture(scope="module")
def full(mg):
    """The product's two runs (parameters trainable / y_hat detached; parameters frozen / y_hat requires grad) from the
    same state, and ONE float64 and one float32 reference forward + backward under the product's sign pattern: the
    loss sum(map . cotangent) over every returned tensor gives the parameter gradients of the first run and the y_hat
    gradient of the second."""
    W = MR.msd_init(21)
    gen = torch.Generator().manual_seed(22)
    y, y_hat = torch.randn(1, 1, T_FULL, generator=gen), torch.randn(1, 1, T_FULL, generator=gen)
    runs = {}
    cots = None
    for name in ("d_phase", "g_phase"):
        net = mg.MultiScaleDiscriminator()
        net.load_state_dict({k: v.clone() for k, v in W.items()}, strict=True)
        net = net.cuda().train()
        yh = y_hat.cuda()
        if name == "g_phase":
            for p in net.parameters():
                p.requires_grad_(False)
            yh.requires_grad_()
        out = net(y.cuda(), yh)
        flat = flat_outputs(out)
        if cots is None:
            cots = [torch.randn(f.shape, generator=gen) for f in flat]
        sum((f * c.cuda()).sum() for f, c in zip(flat, cots)).backward()
        runs[name] = {"net": net, "out": out, "flat": [f.detach().cpu() for f in flat], "y_hat": yh}
    product_taps = MR.taps_of_fmaps("discriminators", runs["d_phase"]["out"][2], runs["d_phase"]["out"][3])
    ref = {}
    masks = None
    for dt in (torch.float64, torch.float32):
        Wd = {k: v.to(dt, copy=True) for k, v in W.items()}
        for k in Wd:
            if k not in MR.buffer_names():
                Wd[k].requires_grad_()
        y_, yh_ = y.to(dt), y_hat.to(dt).requires_grad_()
        if masks is None:
            own = {}
            with torch.no_grad():
                MR.msd_forward(MR.clone_buffers(Wd), y_, yh_, taps=own)
            masks = MR.kink_masks(product_taps, own)
        flat = flat_outputs(MR.msd_forward(Wd, y_, yh_, masks=masks))
        sum((f * c.to(dt)).sum() for f, c in zip(flat, cots)).backward()
        ref[dt] = {"flat": [f.detach() for f in flat], "W": Wd, "dy_hat": yh_.grad}
    return {"runs": runs, "ref": ref, "W": W}


def test_module_forward(full):
    r64, r32 = full["ref"][torch.float64], full["ref"][torch.float32]
    for name in ("d_phase", "g_phase"):
        run = full["runs"][name]
        assert len(run["flat"]) == 6 + 2 * 24
        for what, got, a32, a64 in zip(output_names(), run["flat"], r32["flat"], r64["flat"]):
            assert got.shape == a64.shape, what
            check(got, a32, a64, BAR_MAP, "%s: %s" % (name, what))
        for k in MR.buffer_names():       # two power iterations on scale 0, none elsewhere
            check(run["net"].state_dict()[k], r32["W"][k], r64["W"][k], BAR_MAP, "%s: %s" % (name, k))
            if r64["W"][k].numel() > 1:
                assert not torch.equal(r64["W"][k].float(), full["W"][k])
    # the two runs saw the same inputs and state: same bits
    for a, b in zip(full["runs"]["d_phase"]["flat"], full["runs"]["g_phase"]["flat"]):
        assert torch.equal(a, b)


def test_module_parameter_gradients(full):
    r64, r32 = full["ref"][torch.float64], full["ref"][torch.float32]
    run = full["runs"]["d_phase"]
    assert run["y_hat"].grad is None
    names = [k for k, _ in run["net"].named_parameters()]
    assert len(names) == 8 * 2 + 2 * 8 * 3
    for k, p in run["net"].named_parameters():
        assert p.grad is not None, k
        check(p.grad, r32["W"][k].grad, r64["W"][k].grad, BAR_PARAM, "d / d " + k)


def test_module_input_gradient_with_frozen_parameters(full):
    r64, r32 = full["ref"][torch.float64], full["ref"][torch.float32]
    run = full["runs"]["g_phase"]
    assert all(p.grad is None for p in run["net"].parameters()), "frozen parameters get no gradient"
    check(run["y_hat"].grad, r32["dy_hat"], r64["dy_hat"], BAR_DATA, "d / d y_hat")


def test_module_eval_leaves_u_and_v(mg):
    W = MR.msd_init(23)
    net = mg.MultiScaleDiscriminator()
    net.load_state_dict(W, strict=True)
    net = net.cuda().eval()
    gen = torch.Generator().manual_seed(24)
    y, y_hat = torch.randn(1, 1, 300, generator=gen), torch.randn(1, 1, 300, generator=gen)
    with torch.no_grad():
        out = net(y.cuda(), y_hat.cuda())
        W64 = {k: v.double() for k, v in W.items()}
        own = {}
        MR.msd_forward(W64, y.double(), y_hat.double(), taps=own, train=False)
        masks = MR.kink_masks(MR.taps_of_fmaps("discriminators", out[2], out[3]), own)
        r64 = MR.msd_forward(W64, y.double(), y_hat.double(), masks=masks, train=False)
        r32 = MR.msd_forward({k: v.clone() for k, v in W.items()}, y, y_hat, masks=masks, train=False)
    for k in MR.buffer_names():
        assert torch.equal(net.state_dict()[k].cpu(), W[k]), k
        assert torch.equal(W64[k], W[k].double()), k
    for what, got, a32, a64 in zip(output_names(), flat_outputs(out), flat_outputs(r32), flat_outputs(r64)):
        check(got, a32, a64, BAR_MAP, "eval: " + what)


def test_discriminator_s_partly_frozen_backward_stops_above_layer_0(mg):
    """A weight-norm DiscriminatorS at T = 300 with convs.0 and convs.1 frozen, an input that does not require grad and
    a loss on one middle map plus the logits: the walk down the stack starts at a map with an outside gradient and stops
    at layer 2.  The layers above run the same kernels on the same data as with nothing frozen, and those kernels have
    fixed summation orders, so their parameter gradients are the same bits."""
    prefix = "discriminators.1."
    W = {k[len(prefix):]: v for k, v in MR.msd_init(25).items() if k.startswith(prefix)}
    gen = torch.Generator().manual_seed(26)
    x = torch.randn(2, 1, 300, generator=gen).cuda()
    cots = None
    nets = {}
    for name in ("all", "frozen"):
        net = mg.DiscriminatorS()
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
# 4: in the trainer
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stft(mg):
    return mg.audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)


def build_trainer(mg, manifest, stft, seed, **kw):
    Wg, Wm = VG.seeded_weights(manifest), MR.msd_init(seed)
    Gn = mg.vocoder.Generator(VG._h())
    Gn.load_state_dict({k: v.detach().clone() for k, v in Wg.items()})
    msd = mg.MultiScaleDiscriminator()
    msd.load_state_dict({k: v.clone() for k, v in Wm.items()}, strict=True)
    return mg.VocoderGANTrainer(Gn.cuda(), stft, {"msd": msd.cuda()}, **kw), Wg, Wm


def test_trainer_sgd_two_steps_match_float64(mg, manifest, stft):
    """VocoderGANTrainer over the native generator and the native MSD against the float64 chain (hifigan_train_ref +
    hifigan_msd_ref): losses of two SGD steps, post-step parameters of both sides, and scale 0's u / v after the eight
    power iterations (two per forward, two forwards a step)."""
    LR, LR_D = 1e-5, 1e-3
    tr, Wg, Wm = build_trainer(mg, manifest, stft, 31, optimizer=torch.optim.SGD, lr=LR)
    for group in tr.optim_d.param_groups:
        group["lr"] = LR_D
    mel, wav = VG.trainer_batch()
    win, basis = stft.stft_fn._tables.window.double(), stft.mel_basis.double().cpu()
    bufs = set(MR.buffer_names())

    def to_state(Wd, dt):
        return {k: (v.to(dt, copy=True) if k in bufs else v.detach().to(dt, copy=True).requires_grad_()) for k, v in Wd.items()}

    state = {dt: {"g": {k: v.detach().to(dt, copy=True).requires_grad_() for k, v in Wg.items()}, "msd": to_state(Wm, dt)}
             for dt in (torch.float64, torch.float32)}
    got, ref = [], {torch.float64: [], torch.float32: []}
    for step in range(2):
        taps = {}
        got.append(tr.step(mel.cuda(), wav.cuda(), taps=taps))
        for dt, st in state.items():
            y = wav.to(dt)[:, None, :]
            first = dt == torch.float64
            discs = {"msd": (MR.msd_forward, st["msd"])}
            params = [v for k, v in st["msd"].items() if k not in bufs]
            if first:       # the float64 run's own signs against the GPU run's, phase by phase; u / v must not advance
                own_g, own_d = {}, {}
                with torch.no_grad():
                    y_own = HR.generator_forward(st["g"], mel.to(dt), taps=own_g)
                    MR.d_phase_loss({"msd": (MR.msd_forward, MR.clone_buffers(st["msd"]))}, y, y_own, taps=own_d)
                masks = {"generator": MR.kink_masks(taps["generator"], own_g),
                         "d": {"msd": MR.kink_masks(MR.taps_of_fmaps("discriminators", *taps["d"]["msd"]), own_d["msd"])}}
            y_hat = HR.generator_forward(st["g"], mel.to(dt), masks=masks["generator"])
            for v in params:
                v.grad = None
            loss_d = MR.d_phase_loss(discs, y, y_hat, masks=masks["d"])
            loss_d.backward()
            with torch.no_grad():
                for v in params:
                    v -= LR_D * v.grad
            if first:
                own_gp = {}
                with torch.no_grad():
                    MR.g_phase_loss({"msd": (MR.msd_forward, MR.clone_buffers(st["msd"]))}, y, y_hat.detach(), taps=own_gp)
                masks["g"] = {"msd": MR.kink_masks(MR.taps_of_fmaps("discriminators", *taps["g"]["msd"]), own_gp["msd"])}
            for v in st["g"].values():
                v.grad = None
            for v in params:
                v.requires_grad_(False)
            adv, fm = MR.g_phase_loss(discs, y, y_hat, masks=masks["g"])
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
    for k, p in tr.generator.named_parameters():
        check(p, state[torch.float32]["g"][k], state[torch.float64]["g"][k].detach(), BAR_PARAM, "post-step G " + k)
    for k, p in tr.discriminators["msd"].state_dict().items():
        check(p, state[torch.float32]["msd"][k].detach(), state[torch.float64]["msd"][k].detach(), BAR_PARAM,
              "post-step msd " + k)
    assert tr.steps == 2 and all(p.requires_grad for p in tr.discriminators["msd"].parameters())


def test_trainer_checkpoint_reproduces_the_third_step(mg, manifest, stft, tmp_path):
    tr, _, Wm = build_trainer(mg, manifest, stft, 32)
    mel, wav = VG.trainer_batch()
    for _ in range(2):
        tr.step(mel.cuda(), wav.cuda())
    k = "discriminators.0.convs.3.weight_u"
    assert not torch.equal(tr.discriminators["msd"].state_dict()[k].cpu(), Wm[k])
    ck = tmp_path / "do_00000002"
    tr.save(str(ck))
    tr2, _, _ = build_trainer(mg, manifest, stft, 33)
    assert tr2.load(str(ck)).steps == 2
    for (ka, a), (kb, b) in zip(tr.discriminators["msd"].state_dict().items(),
                                tr2.discriminators["msd"].state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka      # parameters and the spectral-norm buffers
    a, b = tr.step(mel.cuda(), wav.cuda()), tr2.step(mel.cuda(), wav.cuda())
    for k in a:
        assert torch.equal(a[k], b[k]), "third step, " + k
