"""JCUDiscriminator, its autograd chain and the fused LSGAN / feature-matching sums at lengths where the three resolutions
(L, L/2, L/4 frames) span several tiles, against float64 torch.autograd through the CPU oracle (oracle/refmath.py:jcu_forward)
-- elementwise, every map, every input gradient, every parameter gradient.  Until this file the discriminator met a
reference only at L <= 64: one tile per utterance in every convolution and data gradient, one chunk per weight gradient.

1. Shapes (CASES): the smallest lengths at which the resolutions cross tiles in different ways.  Before each case
   mg_conv1d_fwd_plan -- the function the launcher switches on -- is asked for the form of every forward and data-gradient
   convolution with the scratch the wrappers pass (ops.SPLIT_SCRATCH_FLOATS); the case asserts that the plan answers, and
   test_cases_reach_a_split_tail_and_several_tiles that the cases together still reach a split 512 -> 128 tail and more than
   one frame tile, so a change of the dispatch thresholds fails here instead of silently moving the coverage.
2. Leaky-ReLU kinks.  An input that fp32 and float64 put on different sides of zero changes the gradient through that
   element by a factor of 5 with no kernel at fault.  Every activation output is one of the ten returned maps, so the
   product's own sign pattern `map > 0` is handed to the reference (jcu_forward(masks=)).  That cannot hide a failure: per
   map, every element whose product mask differs from the float64 run's own has |pre64| <= 1e-4 max|pre64| (a flip means
   |y_gpu - y_ref| >= 0.2 |pre_ref|, and the forward bar is 2e-5), and such elements number at most 1e-3 of the map.  The
   maps themselves are compared with the float64 run that applies its own leaky ReLU.
3. Two streams against one (B = 16, L = 1000, the trainer's 2B rows): the unconditional tail on the side stream, each
   backward replayed on its forward's stream, against both tails on the caller's stream.
4. The fused range losses at sizes that reach their workgroup caps (64 per term forward above 131 072 elements, 256 per
   term backward above 524 288) and at ragged row sizes, on synthetic maps.

Bars (max-abs error / max-abs reference per tensor): the project's own, 2e-5 maps, 5e-5 data gradients, 1e-4 parameter
gradients, 2e-6 max(1, |ref|) loss scalars, 1e-6 loss gradients.  A tensor that misses its bar is judged by the rule of
test_gpu_denoiser_backward_shapes.py: against 8 x the float32 CPU oracle's own error versus float64 at the same shape, seed
and masks, and only where that figure is above the project bar.

Run to run.  Every reduction of the chain has a fixed order: the convolutions sum along the reduction in program order and a
split reduction is combined from scratch in split order (conv_split_finalize_kernel); conv1d_wgrad writes per-split partial
tiles and wgrad_finalize_kernel adds them in index order; rowsum is one workgroup per row with a tree of fixed shape; the
step MLP's and speaker projection's backward (small_outer_kernel, small_linear_t_kernel with Z = 1) use no atomics; the
multi-term loss adds per-workgroup partials in index order.  torch.autograd adds the gradients that meet at a map in the
order their nodes were recorded, which JCUDiscriminator.forward keeps the same on both stream paths.  So two runs must agree
bit for bit in EVERY gradient, and so must the two stream paths: asserted for all of them, no tolerance.

Measured on an MI355X (the table is in DESIGN.md section 7.2): no tensor missed a project bar, so the fallback rule never
applied; worst map 3.1e-6, worst data gradient 6.2e-7, worst parameter gradient 1.2e-6, worst loss scalar 8.2e-8, worst
loss gradient 1.0e-7; no sign decision differed from float64 in any map.  Each test prints its figures on `JCUERR` lines (-s)."""
import ctypes
import json
import os

import pytest
import torch

from helpers import GOLDEN, hot_path_configs, load_seeded, seeded, jcu_oracle_grads
from oracle import refmath as R

pytestmark = pytest.mark.gpu
FT, GT, PT = 2e-5, 5e-5, 1e-4
LOSS_T, LOSS_GT = 2e-6, 1e-6
BAND, FLIP_SHARE = 1e-4, 1e-3
SEED = {0: 41, 1: 42}

# (multi-speaker, B, L) -> L, L/2, L/4
CASES = [
    (0, 4, 517),     # 517, 259, 130: odd, odd, even; the tail is one 128-frame tile + 2; stride-2 dgrads from odd lengths
    (1, 3, 1000),    # 1000, 500, 250: the trained length; L % 4 == 0; zero-inserted length 999 / 499 against Lout 1000 / 500
    (0, 2, 262),     # 262, 131, 66: even, odd, even; 64 + 2 frames at the tail, 2 * 65 + 1 in the middle
    (1, 2, 129),     # 129, 65, 33: one frame past a tile at two resolutions
]
SMALLEST = (1, 2, 129)
# name, Ci, Co, K, stride: the input projection (a k = 1 convolution), the three shared layers, one tail (both tails have
# the same shapes)
LAYERS = [("input_projection", 160, 160, 1, 1), ("conv_block.0", 160, 64, 3, 1), ("conv_block.1", 64, 128, 5, 2),
          ("conv_block.2", 128, 512, 5, 2), ("tail.0", 512, 128, 5, 1), ("tail.1", 128, 1, 3, 1)]


def _cid(c):
    return "ms%d-B%d-L%d" % c


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd as m
    assert torch.cuda.is_available()
    m.lib()
    return m


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for k in ("MG_JCU_OVERLAP", "MG_CONV_SPLIT"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------ plans
def _plan(mg, B, Ci, Lout, rows, K, stride):
    from mixgan_tts_amd import _lib, ops
    p = _lib.ConvPlan()
    rc = mg.lib().mg_conv1d_fwd_plan(B, Ci, Lout, rows, K, stride, 1, ops.SPLIT_SCRATCH_FLOATS, _lib.MG_CONV_EPI_PLAIN,
                                     ctypes.byref(p))
    assert rc == 0, "mg_conv1d_fwd_plan has no answer for B=%d Ci=%d Lout=%d rows=%d K=%d stride=%d: %d" % (
        B, Ci, Lout, rows, K, stride, rc)
    assert (p.kw, p.stride) == (K, stride) and p.ksplit >= 1
    return p


def _plans(mg, B, L):
    """{(layer, "fwd" | "dgrad"): (plan, frame tiles per utterance)} as autograd._Conv1dFn launches them: the data
    gradient is a stride-1 convolution over the (zero-inserted) output gradient with the layer's input length forced."""
    out = {}
    Lin = L
    for name, Ci, Co, K, stride in LAYERS:
        Lout = (Lin - 1) // stride + 1
        for kind, p, frames in (("fwd", _plan(mg, B, Ci, Lout, Co, K, stride), Lout),
                                ("dgrad", _plan(mg, B, Co, Lin, Ci, K, 1), Lin)):
            out[(name, kind)] = (p, -(-frames // (32 * (4 // p.mw) * p.nnb)))
        Lin = Lout
    return out


def test_cases_reach_a_split_tail_and_several_tiles(mg):
    split_tail, multi_tile = [], []
    for c in CASES:
        pl = _plans(mg, c[1], c[2])
        if pl[("tail.0", "fwd")][0].ksplit > 1:
            split_tail.append(c)
        if any(tiles > 1 for _, tiles in pl.values()):
            multi_tile.append(c)
        for (name, kind), (p, tiles) in sorted(pl.items()):
            print("JCUERR %-16s plan %-16s %-5s form (%d,%d,%d) ksplit %d frame tiles %d" % (
                _cid(c), name, kind, p.mw, p.wm, p.nnb, p.ksplit, tiles))
    assert split_tail, "no case runs the 512 -> 128 tail with a split reduction any more"
    assert multi_tile, "no case gives any convolution more than one frame tile any more"


# ------------------------------------------------------------------------------------------ models, inputs, references
_MODELS, _CASES = {}, {}


def _manifest():
    with open(os.path.join(GOLDEN, "manifest.json")) as f:
        return json.load(f)


def _new_D(mg, ms):
    _, pre, mc, tr = hot_path_configs(multi_speaker=bool(ms), stats_dir=".")
    D = mg.JCUDiscriminator(pre, mc, tr)
    load_seeded(D, _manifest(), "jcu_ms%d" % ms, SEED[ms])
    return D.cuda()


def _model(mg, ms):
    """(product discriminator with the seeded jcu_ms<ms> weights, the same weights as float32 tensors)."""
    if ms not in _MODELS:
        W32, _ = seeded(_manifest(), "jcu_ms%d" % ms, SEED[ms])
        D = _new_D(mg, ms)
        assert sorted(k for k, _ in D.named_parameters()) == sorted(W32), "parameters differ from the weight recipe"
        _MODELS[ms] = (D, W32)
    return _MODELS[ms]


def _map_shapes(B, L):
    L2 = (L - 1) // 2 + 1
    L4 = (L2 - 1) // 2 + 1
    return [(B, 64, L), (B, 128, L2), (B, 512, L4), (B, 128, L4), (B, 1, L4)]


def _err(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-30))


MAPS = ["cond%d" % i for i in range(5)] + ["uncond%d" % i for i in range(5)]


def _bar(key):
    return FT if key in MAPS else PT if key.startswith("param/") else GT


def _kind(key):
    return "maps" if key in MAPS else "param" if key.startswith("param/") else key


class Case:
    """Fixed inputs and cotangents of one (ms, B, L); the float64 references are computed once, from the first product
    run's masks, and never changed."""

    def __init__(self, mg, ms, B, L):
        self.ms, self.B, self.L = ms, B, L
        self.D, self.W32 = _model(mg, ms)
        gen = torch.Generator().manual_seed(100003 * ms + 1009 * B + L)
        self.x_ts = torch.randn(B, L, 80, generator=gen)
        self.x_t_prevs = torch.randn(B, L, 80, generator=gen)
        self.s = torch.randn(B, 256, generator=gen) if ms else None
        self.t = torch.tensor([0, 3, 1, 2][:B])                      # 0..3, both ends in every batch
        assert 0 in self.t.tolist() and 3 in self.t.tolist()
        self.cot = [[torch.randn(*sh, generator=gen) for sh in _map_shapes(B, L)] for _ in range(2)]
        self.cot_gpu = [[g.cuda() for g in side] for side in self.cot]
        self.masks = self._plain = self._ref = self._f32 = None

    def plain(self):
        """The float64 forward with its own leaky ReLU: the maps' reference, and the pre-activations the flips are judged by."""
        if self._plain is None:
            W = {k: v.double() for k, v in self.W32.items()}
            taps = {}
            with torch.no_grad():
                c, u = R.jcu_forward(W, self.x_ts.double(), self.x_t_prevs.double(), None if self.s is None else self.s.double(),
                                     self.t, taps=taps)
            self._plain = {"cond%d" % i: c[i] for i in range(5)}
            self._plain.update({"uncond%d" % i: u[i] for i in range(5)})
            self._plain.update({"pre/" + k: v for k, v in taps.items()})
        return self._plain

    def adopt_masks(self, got):
        if self.masks is None:
            self.masks = ([(got["cond%d" % i] > 0).cpu() for i in range(5)], [(got["uncond%d" % i] > 0).cpu() for i in range(5)])
        return self.masks

    def ref(self):
        """float64 autograd with the product's sign pattern."""
        if self._ref is None:
            W = {k: v.double().requires_grad_() for k, v in self.W32.items()}
            self._ref = jcu_oracle_grads(W, self.x_ts, self.x_t_prevs, self.s, self.t, self.cot, torch.float64, self.masks)
        return self._ref

    def f32_cpu_error(self, kind):
        """The yardstick for a missed bar: the float32 CPU oracle's error against the float64 one at this shape, seed and
        masks, worst tensor of the kind."""
        if self._f32 is None:
            W = {k: v.clone().requires_grad_() for k, v in self.W32.items()}
            got = jcu_oracle_grads(W, self.x_ts, self.x_t_prevs, self.s, self.t, self.cot, torch.float32, self.masks)
            self._f32 = {}
            for k, v in got.items():
                if not k.startswith("pre/"):
                    self._f32[_kind(k)] = max(self._f32.get(_kind(k), 0.0), _err(v, self.ref()[k]))
        return self._f32[kind]


def _case(mg, c):
    if c not in _CASES:
        _CASES[c] = Case(mg, *c)
    return _CASES[c]


def _run(D, x_ts, x_t_prevs, s, t, cot, overlap=True):
    """One product forward + backward of sum_i <cond_i, cot[0][i]> + <uncond_i, cot[1][i]>; every result cloned on the GPU."""
    D.branch_overlap = overlap
    D.zero_grad(set_to_none=True)
    a, b = x_ts.cuda().requires_grad_(), x_t_prevs.cuda().requires_grad_()
    ss = None if s is None else s.cuda().requires_grad_()
    c, u = D(a, b, ss, t.cuda())
    assert all(c[i] is u[i] for i in range(3))
    loss = sum((m * g).sum() for m, g in zip(c, cot[0])) + sum((m * g).sum() for m, g in zip(u, cot[1]))
    loss.backward()
    got = {"d_x_ts": a.grad, "d_x_t_prevs": b.grad}
    if ss is not None:
        got["d_s"] = ss.grad
    for i in range(5):
        got["cond%d" % i], got["uncond%d" % i] = c[i].detach(), u[i].detach()
    for k, p in D.named_parameters():
        assert p.grad is not None, k
        got["param/" + k] = p.grad.clone()
    D.zero_grad(set_to_none=True)
    D.branch_overlap = True
    return got


def _run_case(case, overlap=True):
    return _run(case.D, case.x_ts, case.x_t_prevs, case.s, case.t, case.cot_gpu, overlap)


def _judge(case, label, got, fails):
    """Maps against the float64 run with its own activations, gradients against float64 autograd with the adopted masks."""
    worst = {}
    for k in sorted(got):
        ref = case.plain()[k] if k in MAPS else case.ref()[k]
        e = _err(got[k].cpu(), ref)
        kind, bar = _kind(k), _bar(k)
        if e >= worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (e, k)
        if not e <= bar:
            f32 = case.f32_cpu_error(kind)
            if 8 * f32 > bar and e <= 8 * f32:
                print("JCUERR-WIDENED %s %s: %.3e > %.1e, within 8 x the float32 CPU oracle's %.3e" % (label, k, e, bar, f32))
            else:
                fails.append("%s %s: %.3e > %.1e (float32 CPU oracle: %.3e)" % (label, k, e, bar, f32))
    for kind in sorted(worst):
        print("JCUERR %-24s %-12s %.3e  (%s)" % (label, kind, worst[kind][0], worst[kind][1]))
    return worst


def _check_flips(case, label, fails):
    """The condition under which adopting the product's masks cannot hide a failure, per map."""
    plain = case.plain()
    for side, lst in zip(("cond", "uncond"), case.masks):
        for i, m in enumerate(lst):
            pre = plain["pre/%s%d" % (side, i)]
            flips = m != (pre > 0)
            n = int(flips.sum())
            top = float(pre.abs().max())
            far = float(pre[flips].abs().max()) / top if n else 0.0
            print("JCUERR %-24s flips %s%d %d of %d, largest |pre| / max|pre| %.2e" % (label, side, i, n, pre.numel(), far))
            if far > BAND:
                fails.append("%s %s%d: a flipped element has |pre| = %.2e of the map's largest (> %.0e)" % (label, side, i, far, BAND))
            if n > FLIP_SHARE * pre.numel():
                fails.append("%s %s%d: %d flips in %d elements (> %.0e)" % (label, side, i, n, pre.numel(), FLIP_SHARE))


# ------------------------------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("c", CASES, ids=_cid)
def test_forward_and_every_gradient_vs_float64(mg, c):
    """The ten maps, d_x_ts, d_x_t_prevs, d_s and every parameter gradient elementwise against float64, on the default
    (two-stream) path; a second forward + backward gives the same bits in every tensor."""
    ms, B, L = c
    _plans(mg, B, L)                                   # the plan answers for all twelve convolutions of this shape
    case = _case(mg, c)
    label = _cid(c)
    a = _run_case(case)
    assert case.D._side is not None and case.D._side != torch.cuda.current_stream(), "the default path did not take the side stream"
    assert [tuple(a["cond%d" % i].shape) for i in range(5)] == _map_shapes(B, L)
    case.adopt_masks(a)
    fails = []
    _check_flips(case, label, fails)
    _judge(case, label, a, fails)
    b = _run_case(case)
    assert sorted(a) == sorted(b)
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    print("JCUERR %-24s bit-identical run to run: %d of %d tensors" % (label, len(a) - len(differ), len(a)))
    if differ:
        fails.append("%s: two runs differ in %s (every reduction has a fixed order)" % (label, differ))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ 3. two streams against one
def test_one_stream_path_vs_float64_at_the_smallest_case(mg):
    """branch_overlap = False: the same maps bit for bit, and the same float64 comparison as the default path."""
    case = _case(mg, SMALLEST)
    label = _cid(SMALLEST) + "/one-stream"
    ref_run = _run_case(case)
    case.adopt_masks(ref_run)
    a = _run_case(case, overlap=False)
    fails = []
    for k in MAPS:
        if not torch.equal(a[k], ref_run[k]):
            fails.append("%s %s: differs from the two-stream path" % (label, k))
    _check_flips(case, label, fails)
    _judge(case, label, a, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("ms", [0, 1])
def test_two_streams_equal_one_stream_at_the_training_shape(mg, monkeypatch, ms):
    """B = 16 rows (the trainer's 2B at B = 8), L = 1000: the one shape at which the tails' kernels last long enough to
    coexist.  Alternating one-stream / two-stream runs, three rounds: every map, input gradient and parameter gradient
    bit-identical between the paths and between the rounds (every reduction has a fixed order -- see the module docstring --
    so no tensor is left to a tolerance); the two-stream run really has a side stream; MG_JCU_OVERLAP=0 gives the
    one-stream path."""
    B, L = 16, 1000
    gen = torch.Generator().manual_seed(7700 + ms)
    x_ts, x_prev = torch.randn(B, L, 80, generator=gen), torch.randn(B, L, 80, generator=gen)
    s = torch.randn(B, 256, generator=gen) if ms else None
    t = torch.arange(B) % 4
    cot = [[torch.randn(*sh, generator=gen).cuda() for sh in _map_shapes(B, L)] for _ in range(2)]
    D = _new_D(mg, ms)
    assert D._side is None and D.branch_overlap
    runs = []
    for rnd in range(3):
        runs.append(("one-stream/%d" % rnd, _run(D, x_ts, x_prev, s, t, cot, overlap=False)))
        if rnd == 0:
            assert D._side is None, "branch_overlap = False opened the side stream"
        runs.append(("two-stream/%d" % rnd, _run(D, x_ts, x_prev, s, t, cot, overlap=True)))
        assert D._side is not None and D._side != torch.cuda.current_stream(), "the overlapped run has no side stream"
    E = _new_D(mg, ms)
    monkeypatch.setenv("MG_JCU_OVERLAP", "0")
    runs.append(("MG_JCU_OVERLAP=0", _run(E, x_ts, x_prev, s, t, cot, overlap=True)))
    assert E._side is None, "MG_JCU_OVERLAP=0 still opened the side stream"
    torch.cuda.synchronize()
    first = runs[0][1]
    fails = []
    worst = 0.0
    for name, r in runs[1:]:
        assert sorted(r) == sorted(first)
        for k in first:
            assert torch.isfinite(r[k]).all(), (name, k)
            if not torch.equal(r[k], first[k]):
                e = _err(r[k], first[k])
                worst = max(worst, e)
                fails.append("ms%d %s vs %s: %s differs (%.3e of its largest)" % (ms, name, runs[0][0], k, e))
    print("JCUERR ms%d-B16-L1000 two-stream vs one-stream, 3 rounds + MG_JCU_OVERLAP=0: %d tensors x %d runs, %d differ (worst %.3e)" % (
        ms, len(first), len(runs) - 1, len(fails), worst))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ 4. fused range losses
LAMBDA_FM = 10.0
LOSS_SETS = {
    # the JCU's maps at B = 5, L = 1000: per-term n = 320 000 (cond0, cond1: the forward cap of 64 workgroups) and
    # 640 000 (cond2: also the backward cap of 256)
    "jcu-B5-L1000": (5, [(64, 1000), (128, 500), (512, 250), (128, 250), (1, 250)]),
    # ragged rows at B = 3, L = 131: the real rows of the logit maps start 99 floats into the tensor
    "ragged-B3-L131": (3, [(64, 131), (128, 66), (512, 33), (128, 33), (1, 33)]),
}
_LOSS_DATA = {}


def _loss_data(name):
    """Synthetic whole maps [2B, C, L'] (cond list, uncond list) and the float64 losses and gradients on their slices,
    fake = rows [0, B), real = rows [B, 2B); computed once."""
    if name not in _LOSS_DATA:
        B, shapes = LOSS_SETS[name]
        gen = torch.Generator().manual_seed(len(name) + 31 * B)
        maps = [[torch.randn(2 * B, C, Lm, generator=gen) for C, Lm in shapes] for _ in range(2)]
        ref = {}
        for phase in ("d", "g"):
            c, u = ([m.double().requires_grad_() for m in side] for side in maps)
            fc, fu, rc, ru = [m[:B] for m in c], [m[:B] for m in u], [m[B:] for m in c], [m[B:] for m in u]
            if phase == "d":
                first, second = R.d_loss(rc[-1], ru[-1], fc[-1], fu[-1])            # d_real, d_fake
            else:
                first, second = R.g_loss(fc[-1], fu[-1]), LAMBDA_FM * R.fm_loss(rc, ru, fc, fu)   # adv, lambda_fm * fm
            total = first + second
            total.backward()
            ref[phase] = ([total.item(), first.item(), second.item()], [[m.grad for m in c], [m.grad for m in u]])
        _LOSS_DATA[name] = (B, maps, ref)
    return _LOSS_DATA[name]


def _leaves(maps):
    return [[m.cuda().requires_grad_() for m in side] for side in maps]


def _scalars(label, got, ref, fails):
    vals = [float(v) for v in got]
    for nm, a, b in zip(("total", "first subtotal", "second subtotal"), vals, ref):
        e = abs(a - b) / max(1.0, abs(b))
        print("JCUERR %-28s %-16s %.3e  (%.9g vs %.9g)" % (label, nm, e, a, b))
        if not e <= LOSS_T:
            fails.append("%s %s: %.9g vs %.9g, %.3e > %.1e" % (label, nm, a, b, e, LOSS_T))
    return vals


def _loss_grads(label, leaves, ref_grads, fails, only_last=False):
    worst = 0.0
    for side, lst, refs in zip(("cond", "uncond"), leaves, ref_grads):
        for i, (m, r) in enumerate(zip(lst, refs)):
            if only_last and i < len(lst) - 1:
                if m.grad is not None:
                    fails.append("%s %s%d: the D phase wrote a gradient to a map that is no logit map" % (label, side, i))
                continue
            if m.grad is None:
                fails.append("%s %s%d: no gradient" % (label, side, i))
                continue
            e = _err(m.grad.cpu(), r)
            worst = max(worst, e)
            if not e <= LOSS_GT:
                fails.append("%s d_%s%d: %.3e > %.1e" % (label, side, i, e, LOSS_GT))
    print("JCUERR %-28s %-16s %.3e" % (label, "gradients", worst))


@pytest.mark.parametrize("name", sorted(LOSS_SETS))
def test_g_adv_fm_total_2b_vs_float64(mg, name):
    from mixgan_tts_amd import losses
    B, maps, ref = _loss_data(name)
    if name.startswith("jcu"):
        n = [B * C * Lm for C, Lm in LOSS_SETS[name][1]]
        assert n[0] > 131072 and n[1] > 131072 and n[2] > 524288, "the set no longer reaches the workgroup caps"
    else:
        assert (B * LOSS_SETS[name][1][-1][0] * LOSS_SETS[name][1][-1][1]) % 2 == 1, "the real rows no longer start at an odd offset"
    fails = []
    runs = []
    for _ in range(2):
        lv = _leaves(maps)
        out = losses.g_adv_fm_total_2b(lv[0], lv[1], B, LAMBDA_FM)
        out[0].backward()
        runs.append((lv, torch.stack([o.detach() for o in out])))
    lv, vals = runs[0]
    _scalars(name + "/g-2b", vals, ref["g"][0], fails)
    _loss_grads(name + "/g-2b", lv, ref["g"][1], fails)
    for side in lv:
        for i, m in enumerate(side):
            if m.grad is not None and not bool((m.grad[B:] == 0).all()):
                fails.append("%s map %d: a real row has a gradient in the G phase" % (name, i))
    # a second call: the same bits
    assert torch.equal(runs[0][1], runs[1][1]), "two calls give different sums"
    for sa, sb in zip(runs[0][0], runs[1][0]):
        for i, (ma, mb) in enumerate(zip(sa, sb)):
            assert torch.equal(ma.grad, mb.grad), "two calls give different gradients for map %d" % i
    # the sliced form reads the same rows through the same kernel with the same per-term sizes: the same bits
    sl = _leaves(maps)
    out = losses.g_adv_fm_total([m[B:] for m in sl[0]], [m[B:] for m in sl[1]], [m[:B] for m in sl[0]], [m[:B] for m in sl[1]],
                                LAMBDA_FM)
    out[0].backward()
    if not torch.equal(torch.stack([o.detach() for o in out]), vals):
        fails.append("%s: g_adv_fm_total on slices %s vs the range form %s" % (name, [float(o) for o in out], vals.tolist()))
    for side_s, side_r in zip(sl, lv):
        for i, (ms_, mr) in enumerate(zip(side_s, side_r)):
            if not torch.equal(ms_.grad, mr.grad):
                fails.append("%s map %d: gradient of the sliced form differs from the range form (%.3e)" % (
                    name, i, _err(ms_.grad, mr.grad)))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", sorted(LOSS_SETS))
def test_d_loss_total_2b_vs_float64(mg, name):
    from mixgan_tts_amd import losses
    B, maps, ref = _loss_data(name)
    fails = []
    runs = []
    for _ in range(2):
        lv = _leaves(maps)
        out = losses.d_loss_total_2b(lv[0][-1], lv[1][-1], B)
        out[0].backward()
        runs.append((lv, torch.stack([o.detach() for o in out])))
    lv, vals = runs[0]
    _scalars(name + "/d-2b", vals, ref["d"][0], fails)
    _loss_grads(name + "/d-2b", lv, ref["d"][1], fails, only_last=True)
    assert torch.equal(runs[0][1], runs[1][1]), "two calls give different sums"
    for k in range(2):
        assert torch.equal(runs[0][0][k][-1].grad, runs[1][0][k][-1].grad), "two calls give different gradients"
    sl = _leaves(maps)
    out = losses.d_loss_total(sl[0][-1][B:], sl[1][-1][B:], sl[0][-1][:B], sl[1][-1][:B])
    out[0].backward()
    if not torch.equal(torch.stack([o.detach() for o in out]), vals):
        fails.append("%s: d_loss_total on slices %s vs the range form %s" % (name, [float(o) for o in out], vals.tolist()))
    for k in range(2):
        if not torch.equal(sl[k][-1].grad, lv[k][-1].grad):
            fails.append("%s: logit gradient %d of the sliced form differs from the range form" % (name, k))
    assert not fails, "\n".join(fails)
