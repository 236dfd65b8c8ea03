"""GPU parity of the native MelGAN discriminator (csrc/gconv_c4.h, csrc/msd.hip, melgan_discriminators.py) and of the
hinge GAN step against float64 torch on the CPU (tests/melgan_disc_ref.py): the kernels one shape at a time, the whole
module at full width, and the module inside VocoderGANTrainer.

Error measure and bars as tests/test_gpu_msd.py: max-abs error over max-abs reference through helpers.check; 2e-5 maps
and values, 5e-5 data gradients, 1e-4 parameter gradients and parameters.  Leaky-ReLU kinks: the float64 restatement
adopts the GPU run's sign pattern, and kink_masks asserts what makes that sound.

Kernel shapes: both four-channel-group forms (Cig 4, Cog 16 | 4, K = 41, s = 4) at N = 2.  Groups: the kernels put 16
(Cog = 4) or 4 (Cog = 16) groups in a workgroup, so G = 5 is a ragged pack for the one and a full pack plus a ragged one
for the other, G = 19 a full plus a ragged pack for both (four full packs and a ragged one for Cog = 16), and G = 16
exactly one pack (four).  Lengths: 7 (shorter than the filter), 256 / 257 and 512 / 513 (the forward's 32-frame tile, the
weight gradient's 16-frame chunk and the data gradient's 128- and 512-sample tiles, (Lin - 1) mod 4 zero and not), 599
(ragged last tile, and trailing inputs that no output reads).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import check
import hifigan_train_ref as HR
import melgan_disc_ref as DR
import melgan_train_ref as GR
import test_gpu_melgan_train as TM      # its helpers: seeded_weights, seeded_vocoder, trainer_batch
from test_gpu_vocoder_train import assert_kinks_sound, mel_tables

pytestmark = pytest.mark.gpu
BAR_MAP, BAR_DATA, BAR_PARAM = 2e-5, 5e-5, 1e-4
SLOPE = 0.2
FORMS = [(4, 16, 4), (4, 4, 4)]
GROUPS = [5, 19, 16]
LENGTHS = [7, 256, 257, 512, 513, 599]
N, K, PAD = 2, 41, 20


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


def leaf(t, dt=None):
    """A fresh copy of t in dtype dt that requires grad (t.to(t.dtype) would be t itself); without dt a detached copy."""
    if dt is None:
        return t.detach().clone()
    return t.detach().to(dt, copy=True).requires_grad_()


def lrelu_like(pre, product):
    masks = DR.kink_masks({"x": product}, {"x": pre.double()})
    return DR.lrelu(pre, SLOPE, "x", None, masks)


# ------------------------------------------------------------------------------------------------------------------
# 1: the grouped kernels.  One float64 / float32 reference per (form, G, length), shared by the tests.
# ------------------------------------------------------------------------------------------------------------------
_cases = {}


def gconv_case(form, G, Lin, n=N):
    key = (form, G, Lin, n)
    if key in _cases:
        return _cases[key]
    cig, cog, s = form
    gen = torch.Generator().manual_seed(100000 * cog + 1000 * G + Lin)
    x = torch.randn(n, cig * G, Lin, generator=gen)
    w = torch.randn(cog * G, cig, K, generator=gen) / (cig * K) ** 0.5
    b = 0.1 * torch.randn(cog * G, generator=gen)
    Lout = (Lin + 2 * PAD - K) // s + 1
    cot = torch.randn(n, cog * G, Lout, generator=gen)
    below = torch.randn(n, cig * G, Lin, generator=gen)
    add = torch.randn(n, cig * G, Lin, generator=gen)
    res = {"in": (x, w, b, cot, below, add), "Lout": Lout}
    for dt in (torch.float64, torch.float32):
        x_, w_, b_ = (leaf(t, dt) for t in (x, w, b))
        pre = F.conv1d(x_, w_, b_, stride=s, padding=PAD, groups=G)
        (pre * cot.to(dt)).sum().backward()
        mask = torch.where(below > 0, 1.0, SLOPE).to(dt)
        res[dt] = {"pre": pre.detach(), "dx": x_.grad, "dx_masked": (x_.grad + add.to(dt)) * mask, "dw": w_.grad,
                   "db": b_.grad}
    _cases[key] = res
    return res


CASES = [(f, g, L) for f in FORMS for g in GROUPS for L in LENGTHS]
IDS = ["%dx%d_s%d-G%d-L%d" % (f + (g, L)) for f, g, L in CASES]


@pytest.mark.parametrize("form,G,Lin", CASES, ids=IDS)
def test_grouped_forward(mg, form, G, Lin):
    cig, cog, s = form
    c = gconv_case(form, G, Lin)
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


@pytest.mark.parametrize("form,G,Lin", CASES, ids=IDS)
def test_grouped_backward(mg, form, G, Lin):
    cig, cog, s = form
    c = gconv_case(form, G, Lin)
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
    if read_to < Lin:
        want = add[:, :, read_to:] * torch.where(below[:, :, read_to:] > 0, 1.0, SLOPE)
        assert torch.equal(dxm[:, :, read_to:], want), "unread trailing inputs must get exactly add * mask"
    dw = mg.ops.gconv1d_wgrad(cot, x, K, s, PAD, G)
    check(dw, r32["dw"], r64["dw"], BAR_PARAM, "dw")
    check(mg.ops.rowsum(cot), r32["db"], r64["db"], BAR_PARAM, "db")
    # fixed summation order: a second run gives the same bits
    assert torch.equal(mg.ops.gconv1d_wgrad(cot, x, K, s, PAD, G), dw)
    assert torch.equal(mg.ops.gconv1d_dgrad(cot, pd, cig * G, Lin, K, s, PAD, G, map=below, add=add, slope=SLOPE), dxm)


def test_weight_gradient_over_many_splits(mg):
    """N = 5 and 70 frames: 25 (n, 16-frame) chunks, every one its own partial tile, the last of each n ragged."""
    for form in FORMS:
        cig, cog, s = form
        c = gconv_case(form, 3, 277, n=5)
        x, w, b, cot, below, add = (t.cuda() for t in c["in"])
        dw = mg.ops.gconv1d_wgrad(cot, x, K, s, PAD, 3)
        check(dw, c[torch.float32]["dw"], c[torch.float64]["dw"], BAR_PARAM, "dw, 25 chunks")
        assert torch.equal(mg.ops.gconv1d_wgrad(cot, x, K, s, PAD, 3), dw)


def test_an_existing_form_through_the_shared_dispatcher(mg):
    cig, cog, s, G, Lin = 8, 16, 2, 3, 257
    gen = torch.Generator().manual_seed(77)
    x = torch.randn(N, cig * G, Lin, generator=gen)
    w = torch.randn(cog * G, cig, K, generator=gen) / (cig * K) ** 0.5
    b = 0.1 * torch.randn(cog * G, generator=gen)
    ref = F.conv1d(x.double(), w.double(), b.double(), stride=s, padding=PAD, groups=G)
    cot = torch.randn(ref.shape, generator=gen).cuda()
    xc, wc, bc = x.cuda(), w.cuda(), b.cuda()
    runs = []
    for _ in range(2):
        out = mg.ops.gconv1d_fwd(xc, mg.ops.gconv_pack(wc, s, G), bc, cog * G, K, s, PAD, G)
        dx = mg.ops.gconv1d_dgrad(cot, mg.ops.gconv_pack(wc, s, G, mg.ops.GCONV_DGRAD), cig * G, Lin, K, s, PAD, G)
        runs.append((out, dx, mg.ops.gconv1d_wgrad(cot, xc, K, s, PAD, G)))
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)
    check(runs[0][0], F.conv1d(x, w, b, stride=s, padding=PAD, groups=G), ref, BAR_MAP, "(8, 16, 2) forward")


# ------------------------------------------------------------------------------------------------------------------
# 2: the pool, the reflection pad with the first layer, the two loss modes
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 3, 7, 128, 333])
def test_average_pool_without_counted_padding(mg, L):
    gen = torch.Generator().manual_seed(L)
    x = torch.randn(N, 5, L, generator=gen)
    Lout = (L - 2) // 2 + 1
    cot = torch.randn(N, 5, Lout, generator=gen)
    ref = {}
    for dt in (torch.float64, torch.float32):
        x_ = leaf(x, dt)
        y = F.avg_pool1d(x_, 4, 2, padding=1, count_include_pad=False)
        (y * cot.to(dt)).sum().backward()
        ref[dt] = (y.detach(), x_.grad)
    xc = leaf(x).cuda().requires_grad_()
    y = mg.autograd.avgpool4s2(xc, padding=1, count_include_pad=False)
    assert tuple(y.shape) == (N, 5, Lout)
    check(y, ref[torch.float32][0], ref[torch.float64][0], BAR_MAP, "pool")
    (y * cot.cuda()).sum().backward()
    check(xc.grad, ref[torch.float32][1], ref[torch.float64][1], BAR_DATA, "pool backward")


@pytest.mark.parametrize("T", [8, 64, 333, 1100])
def test_reflect_pad_and_first_layer(mg, T):
    gen = torch.Generator().manual_seed(T)
    x = torch.randn(N, 1, T, generator=gen)
    w = torch.randn(16, 1, 15, generator=gen) / 15 ** 0.5
    b = 0.1 * torch.randn(16, generator=gen)
    cot = torch.randn(N, 16, T, generator=gen)
    ref = {}
    xc, wc, bc = (leaf(t).cuda().requires_grad_() for t in (x, w, b))
    (act,) = mg.autograd.scale_stack(mg.autograd.reflect_pad1d(xc, 7), SLOPE, [(1, 1, 0)], wc, bc)
    assert tuple(act.shape) == (N, 16, T)
    (act * cot.cuda()).sum().backward()
    for dt in (torch.float64, torch.float32):
        x_, w_, b_ = (leaf(t, dt) for t in (x, w, b))
        out = lrelu_like(F.conv1d(F.pad(x_, (7, 7), mode="reflect"), w_, b_), act)
        (out * cot.to(dt)).sum().backward()
        ref[dt] = [out.detach(), x_.grad, w_.grad, b_.grad]
    r64, r32 = ref[torch.float64], ref[torch.float32]
    check(act, r32[0], r64[0], BAR_MAP, "reflect pad + first layer")
    check(xc.grad, r32[1], r64[1], BAR_DATA, "dx through the fold-back")
    check(wc.grad, r32[2], r64[2], BAR_PARAM, "dw")
    check(bc.grad, r32[3], r64[3], BAR_PARAM, "db")
    padded = mg.ops.reflect_pad1d_fwd(x.cuda(), 7)
    assert torch.equal(padded.cpu(), F.pad(x, (7, 7), mode="reflect"))


@pytest.mark.parametrize("n", [1, 255, 70001])
def test_hinge_and_mean_loss_modes(mg, n):
    gen = torch.Generator().manual_seed(n)
    logits = [2.0 * torch.randn(n, generator=gen) for _ in range(3)]
    for sign, x in zip((-1.0, 1.0), logits):      # keep every logit away from the hinge's kink at 1 + sign x = 0
        near = (1 + sign * x.double()).abs() < 1e-3
        x[near] += 0.01
        assert float((1 + sign * x.double()).abs().min()) >= 1e-4
    a, t = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    ref = {}
    for dt in (torch.float64, torch.float32):
        r, f, m, a_ = (leaf(v, dt) for v in (*logits, a))
        terms = [F.relu(1 - r).mean(), F.relu(1 + f).mean(), m.mean(), (a_ - 0.5).pow(2).mean(), (a_ - t.to(dt)).abs().mean()]
        total = 1.0 * terms[0] + 1.5 * terms[1] - 0.7 * terms[2] + 0.3 * terms[3] + 2.0 * terms[4]
        total.backward()
        ref[dt] = (total.detach(), [v.detach() for v in terms], [r.grad, f.grad, m.grad, a_.grad])
    r, f, m, a1, a2 = (v.detach().cuda().requires_grad_() for v in (*logits, a, a))
    out = mg.losses.weighted_means([("hinge", r, -1.0, 1.0), ("hinge", f, 1.0, 1.5), ("mean", m, None, -0.7),
                                    ("mse", a1, 0.5, 0.3), ("l1", a2, t.cuda(), 2.0)])
    out[0].backward()
    r64, r32 = ref[torch.float64], ref[torch.float32]
    check(out[:1], r32[0].reshape(1), r64[0].reshape(1), BAR_MAP, "total")
    means = out.detach()[1 + mg._lib.MG_LOSS_GROUPS:]
    for k in range(5):
        check(means[k:k + 1], r32[1][k].reshape(1), r64[1][k].reshape(1), BAR_MAP, "term %d" % k)
    for k, g in enumerate((r.grad, f.grad, m.grad)):
        check(g, r32[2][k], r64[2][k], BAR_DATA, "gradient of term %d" % k)
    check(a1.grad + a2.grad, r32[2][3], r64[2][3], BAR_DATA, "gradient of the mse and l1 terms")


# ------------------------------------------------------------------------------------------------------------------
# 3: the whole module at full width.  B = 1 (N = 2 in forward_pair), T = 2083: scale 2 runs on 520 samples and its
# deepest grouped map is 3 frames long.
# ------------------------------------------------------------------------------------------------------------------
T_FULL = 2083


def flat_maps(D_real, D_fake):
    return [m for maps in D_real for m in maps] + [m for maps in D_fake for m in maps]


@pytest.fixture(scope="module")
def full(mg):
    """The product's two runs (parameters trainable / y_hat detached; parameters frozen / y_hat requires grad) from the
    same state, and one float64 and one float32 reference forward + backward under the product's sign pattern."""
    W = DR.disc_init(41)
    gen = torch.Generator().manual_seed(42)
    y, y_hat = torch.randn(1, 1, T_FULL, generator=gen), torch.randn(1, 1, T_FULL, generator=gen)
    runs, cots = {}, None
    for name in ("d_phase", "g_phase"):
        net = mg.melgan_discriminators.Discriminator()
        net.load_state_dict({k: v.clone() for k, v in W.items()}, strict=True)
        net = net.cuda().train()
        yh = y_hat.cuda()
        if name == "g_phase":
            for p in net.parameters():
                p.requires_grad_(False)
            yh.requires_grad_()
        D_real, D_fake = net.forward_pair(y.cuda(), yh)
        flat = flat_maps(D_real, D_fake)
        if cots is None:
            cots = [torch.randn(f.shape, generator=gen) for f in flat]
        sum((f * c.cuda()).sum() for f, c in zip(flat, cots)).backward()
        runs[name] = {"net": net, "out": (D_real, D_fake), "flat": [f.detach().cpu() for f in flat], "y_hat": yh}
    with torch.no_grad():
        runs["single"] = [m.cpu() for maps in runs["d_phase"]["net"](y.cuda()) for m in maps]
    product_taps = DR.taps_of_maps(*runs["d_phase"]["out"])
    ref, masks = {}, None
    for dt in (torch.float64, torch.float32):
        Wd = {k: v.to(dt, copy=True).requires_grad_() for k, v in W.items()}
        y_, yh_ = y.to(dt), leaf(y_hat, dt)
        if masks is None:
            own = {}
            with torch.no_grad():
                DR.disc_forward_pair(Wd, y_, yh_, taps=own)
            masks = DR.kink_masks(product_taps, own)
        flat = flat_maps(*DR.disc_forward_pair(Wd, y_, yh_, masks=masks))
        sum((f * c.to(dt)).sum() for f, c in zip(flat, cots)).backward()
        ref[dt] = {"flat": [f.detach() for f in flat], "W": Wd, "dy_hat": yh_.grad}
    return {"runs": runs, "ref": ref, "W": W}


def test_module_forward(full):
    r64, r32 = full["ref"][torch.float64], full["ref"][torch.float32]
    for name in ("d_phase", "g_phase"):
        run = full["runs"][name]
        assert len(run["flat"]) == 2 * 3 * 7
        for i, (got, a32, a64) in enumerate(zip(run["flat"], r32["flat"], r64["flat"])):
            assert got.shape == a64.shape, i
            check(got, a32, a64, BAR_MAP, "%s: %s scale %d map %d" % (name, "real" if i < 21 else "gen", i % 21 // 7, i % 7))
    assert tuple(full["runs"]["d_phase"]["out"][0][2][4].shape) == (1, 1024, 3)
    for a, b in zip(full["runs"]["d_phase"]["flat"], full["runs"]["g_phase"]["flat"]):
        assert torch.equal(a, b)
    # forward(x) is the real half of forward_pair: the kernels treat batch items independently
    for a, b in zip(full["runs"]["single"], full["runs"]["d_phase"]["flat"][:21]):
        assert torch.equal(a, b)


def test_module_parameter_gradients(full):
    r64, r32 = full["ref"][torch.float64], full["ref"][torch.float32]
    run = full["runs"]["d_phase"]
    assert run["y_hat"].grad is None
    assert len(list(run["net"].named_parameters())) == 3 * 7 * 3
    for k, p in run["net"].named_parameters():
        assert p.grad is not None, k
        check(p.grad, r32["W"][k].grad, r64["W"][k].grad, BAR_PARAM, "d / d " + k)


def test_module_input_gradient_with_frozen_parameters(full):
    r64, r32 = full["ref"][torch.float64], full["ref"][torch.float32]
    run = full["runs"]["g_phase"]
    assert all(p.grad is None for p in run["net"].parameters()), "frozen parameters get no gradient"
    check(run["y_hat"].grad, r32["dy_hat"], r64["dy_hat"], BAR_DATA, "d / d y_hat")


def test_fused_losses_on_module_outputs(mg, full):
    D_real, D_fake = full["runs"]["g_phase"]["out"]
    n = len(full["ref"][torch.float64]["flat"]) // 2

    def split(flat):
        return ([flat[7 * i:7 * i + 7] for i in range(3)], [flat[n + 7 * i:n + 7 * i + 7] for i in range(3)])

    r64, r32 = split(full["ref"][torch.float64]["flat"]), split(full["ref"][torch.float32]["flat"])
    for name, got, fn in (("discriminator", mg.losses.melgan_discriminator_loss(D_real, D_fake), DR.discriminator_loss),
                          ("feature", mg.losses.melgan_feature_loss(D_real, D_fake), DR.feature_loss)):
        check(got.reshape(1), fn(*r32).reshape(1), fn(*r64).reshape(1), BAR_MAP, name + " loss")
    check(mg.losses.melgan_generator_loss(D_fake).reshape(1), DR.generator_loss(r32[1]).reshape(1),
          DR.generator_loss(r64[1]).reshape(1), BAR_MAP, "generator loss")


# ------------------------------------------------------------------------------------------------------------------
# 4: in the trainer
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stft(mg):
    return mg.audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000)


NUM_D = 2


def build_trainer(mg, stft, seed, **kw):
    Wg, Wd = TM.seeded_weights(), DR.disc_init(seed, NUM_D)
    voc = TM.seeded_vocoder(mg, Wg)
    disc = mg.melgan_discriminators.Discriminator(NUM_D)
    disc.load_state_dict({k: v.clone() for k, v in Wd.items()}, strict=True)
    return mg.VocoderGANTrainer(voc, stft, {"melgan_d": disc.cuda()}, objective="melgan", **kw), Wg, Wd


def reference_steps(stft, Wg, Wd, mel, wav, all_taps, lr_g, lr_d, lambda_mel, lambda_feat=10.0):
    """The float64 and float32 chains of len(all_taps) SGD steps under the product's sign patterns."""
    win, basis = mel_tables(stft)
    scale = 1.0 / math.log(10.0)
    state = {dt: {"g": {k: v.detach().to(dt, copy=True).requires_grad_() for k, v in Wg.items()},
                  "d": {k: v.detach().to(dt, copy=True).requires_grad_() for k, v in Wd.items()}}
             for dt in (torch.float64, torch.float32)}
    ref = {torch.float64: [], torch.float32: []}
    for taps in all_taps:
        for dt, st in state.items():
            y = wav.to(dt)[:, None, :]
            first = dt == torch.float64
            params = list(st["d"].values())
            if first:
                own_g, own_d = {}, {}
                with torch.no_grad():
                    y_own = GR.generator_forward(st["g"], mel.to(dt), taps=own_g, scale=scale)
                    DR.disc_forward_pair(st["d"], y, y_own, NUM_D, taps=own_d)
                masks = {"generator": assert_kinks_sound(taps["generator"], own_g),
                         "d": DR.kink_masks(DR.taps_of_maps(*taps["d"]["melgan_d"]), own_d)}
            y_hat = GR.generator_forward(st["g"], mel.to(dt), masks=masks["generator"], scale=scale)
            for v in params:
                v.grad = None
            loss_d = DR.discriminator_loss(*DR.disc_forward_pair(st["d"], y, y_hat.detach(), NUM_D, masks=masks["d"]))
            loss_d.backward()
            with torch.no_grad():
                for v in params:
                    v -= lr_d * v.grad
            if first:
                own_gp = {}
                with torch.no_grad():
                    DR.disc_forward_pair(st["d"], y, y_hat.detach(), NUM_D, taps=own_gp)
                masks["g"] = DR.kink_masks(DR.taps_of_maps(*taps["g"]["melgan_d"]), own_gp)
            for v in st["g"].values():
                v.grad = None
            for v in params:
                v.requires_grad_(False)
            D_real, D_fake = DR.disc_forward_pair(st["d"], y, y_hat, NUM_D, masks=masks["g"])
            adv, fm = DR.generator_loss(D_fake), DR.feature_loss(D_real, D_fake)
            loss_g = adv + lambda_feat * fm
            mel_l1 = torch.zeros((), dtype=dt)
            if lambda_mel:
                mel_l1 = (HR.log_mel(y_hat[:, 0], win, basis) - HR.log_mel(wav.to(dt), win, basis)).abs().mean()
                loss_g = loss_g + lambda_mel * mel_l1
            loss_g.backward()
            for v in params:
                v.requires_grad_(True)
            with torch.no_grad():
                for v in st["g"].values():
                    v -= lr_g * v.grad
            ref[dt].append({"loss_d": loss_d.detach(), "loss_g": loss_g.detach(), "mel_l1": mel_l1.detach(),
                            "adv": adv.detach(), "fm": fm.detach()})
    return ref, state


@pytest.mark.parametrize("lambda_mel,steps", [(45.0, 2), (0.0, 1)], ids=["with_mel-2_steps", "lambda_mel_0-1_step"])
def test_trainer_sgd_steps_match_float64(mg, stft, lambda_mel, steps):
    LR, LR_D = 1e-5, 1e-3
    tr, Wg, Wd = build_trainer(mg, stft, 51, optimizer=torch.optim.SGD, lr=LR, lambda_mel=lambda_mel)
    for group in tr.optim_d.param_groups:
        group["lr"] = LR_D
    mel, wav = TM.trainer_batch()
    got, all_taps = [], []
    for _ in range(steps):
        taps = {}
        got.append(tr.step(mel.cuda(), wav.cuda(), taps=taps))
        all_taps.append(taps)
    ref, state = reference_steps(stft, Wg, Wd, mel, wav, all_taps, LR, LR_D, lambda_mel)
    for i in range(steps):
        assert set(got[i]) == {"loss_d", "loss_g", "mel_l1", "adv", "fm"}
        for k, v in got[i].items():
            assert v.is_cuda
            if k == "mel_l1" and not lambda_mel:
                assert float(v) == 0.0
                continue
            check(v.reshape(1), ref[torch.float32][i][k].reshape(1), ref[torch.float64][i][k].reshape(1), BAR_MAP,
                  "%s of step %d" % (k, i))
    for k, p in tr.generator.mel2wav.named_parameters():
        check(p, state[torch.float32]["g"][k].detach(), state[torch.float64]["g"][k].detach(), BAR_PARAM, "post-step G " + k)
        assert not torch.equal(p.detach().cpu(), Wg[k]), k + " did not move"
    for k, p in tr.discriminators["melgan_d"].state_dict().items():
        check(p, state[torch.float32]["d"][k].detach(), state[torch.float64]["d"][k].detach(), BAR_PARAM, "post-step D " + k)
    assert tr.steps == steps and all(p.requires_grad for p in tr.discriminators["melgan_d"].parameters())


def test_trainer_checkpoint_reproduces_the_third_step(mg, stft, tmp_path):
    tr, _, _ = build_trainer(mg, stft, 52)
    mel, wav = TM.trainer_batch()
    for _ in range(2):
        tr.step(mel.cuda(), wav.cuda())
    tr.end_epoch()
    ck = tmp_path / "melgan_00000002"
    tr.save(str(ck))
    tr2, _, _ = build_trainer(mg, stft, 53)
    assert tr2.load(str(ck)).steps == 2
    for (ka, a), (kb, b) in zip(tr.discriminators["melgan_d"].state_dict().items(),
                                tr2.discriminators["melgan_d"].state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    a, b = tr.step(mel.cuda(), wav.cuda()), tr2.step(mel.cuda(), wav.cuda())
    for k in a:
        assert torch.equal(a[k], b[k]), "third step, " + k
    path = tmp_path / "generator.pt"
    mg.vocoder_train.export_melgan_generator(tr.generator, str(path))
    sd = torch.load(path, map_location="cpu", weights_only=True)
    for k, p in tr.generator.mel2wav.state_dict().items():
        assert torch.equal(sd[k], p.cpu()), k


def test_default_objective_is_unchanged(mg, stft):
    """objective="hifigan" spelled out and the constructor without the new arguments: the same bits."""
    mel, wav = TM.trainer_batch()
    outs = []
    for kw in ({}, {"objective": "hifigan", "lambda_feat": 10.0}):
        voc = TM.seeded_vocoder(mg, TM.seeded_weights())
        torch.manual_seed(11)
        msd = mg.MultiScaleDiscriminator().cuda()
        tr = mg.VocoderGANTrainer(voc, stft, {"msd": msd}, **kw)
        out = tr.step(mel.cuda(), wav.cuda())
        outs.append((out, [p.detach().clone() for p in voc.mel2wav.parameters()]))
    for k in outs[0][0]:
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)
