"""The denoiser at model sizes other than residual_channels = encoder_hidden = 256, n_mel_channels <= 96, against float64
autograd through the CPU oracle.  The hand-tuned kernels cover that one point; every other model
takes the paths chosen in den_fwd_plan / den_fwd_layers (csrc/denoiser.hip), which no other test runs:

  C != 256 or H != 256   generic layers -- three conv_launch calls per layer with the epilogues EpiCond, EpiGate (on the
                         gate / filter block pairs of MG_PACK_GATE) and EpiResSkip -- and generic 1x1 head and tail
  C = H = 256, 96 < M <= 128   fused layers, generic head, fused tail
  C = H = 256, M > 128         fused layers, generic head, generic tail
  MG_DENOISER_GENERIC          the generic layers at 256 / 256 (read once per process: run in a child process)

and behind them the generic saving layout (h / g / sig / tnh per layer, ws.x0 != ws.x) feeding mg_denoiser_bwd_staged's
launch-per-layer data gradients (EpiGateBwd / EpiDhBwd), the grouped weight gradients at other row counts, wc_allT
with H <= 64 and H = 192, small_linear's scalar branch (K % 256 != 0) and small_linear_t_kernel with K < 64, and
psample_tail_kernel behind both tails.  The sizes and shapes are helpers.DEN_SIZES / DEN_SMALL_SHAPES;
test_denoiser_plan_cpu.py pins that A to F launch per layer and G takes the single launch.

Weights: the module's own initialisation under a fixed seed (no fixture recipe exists for these sizes), with a live
output projection.  Bars: the project's own (helpers.den_judge) -- 2e-5 output, 5e-5 data gradients, 1e-4 parameter
gradients, max-abs error over max-abs reference, and the one fallback of 8 x the float32 CPU oracle's error where that
exceeds the bar.  Inputs are conditioned (helpers.condition_relu_kinks, band 2e-5) so that the float64 gradient is
single-valued.  Every case prints its worst error per tensor kind (`DIMERR` lines, -s).  Measured on an MI355X (the
table is in DESIGN.md section 7.6): no case needed the fallback; the worst error of any case is 1.0e-6 on the output,
1.1e-6 d_x, 2.3e-6 d_cond (120 layers), 1.1e-6 d_spk, 1.3e-6 on a parameter gradient."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import (DEN_SIZES, DEN_SMALL_SHAPES, DEN_LARGE_SHAPE, DEN_FT, den_size_model, den_size_configs, den_run, den_judge,
                     den_err, den_bar, den_f32_cpu_errors, oracle_grads, condition_relu_kinks, hot_path_configs, write_stats,
                     live_output_projection, Tape)
from oracle import refmath as R
from mixgan_tts_amd import _lib

pytestmark = pytest.mark.gpu
PINS = ("MG_DENOISER_PERSIST", "MG_PERSIST_NT", "MG_PERSIST_SOLO", "MG_PERSIST_TEAM")
GENERIC_SHAPES = [(3, 129), (2, 260)]       # what the MG_DENOISER_GENERIC child runs
T_STEPS = 4


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd as m
    assert torch.cuda.is_available()
    m.lib()
    return m


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for k in PINS:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------ models, inputs, references
_MODELS, _CASES = {}, {}
SIZES = dict(DEN_SIZES, P=(120, 64, 32, 20, 1))      # P: more layers than one pack table holds (test_pack_in_several_launches)


def _model(mg, name):
    if name not in _MODELS:
        den, W64, W32 = den_size_model(mg, name, SIZES[name])
        _MODELS[name] = (den.cuda(), W64, W32)
    return _MODELS[name]


class Case:
    """Fixed inputs of one (size, B, L) and their float64 reference, computed once."""

    def __init__(self, mg, name, B, L):
        NL, C, H, M, ms = SIZES[name]
        self.name, self.B, self.L, self.ms = name, B, L, ms
        self.den, self.W64, self.W32 = _model(mg, name)
        gen = torch.Generator().manual_seed(1000 * B + L + 100003 * ord(name))
        self.x = torch.randn(B, 1, M, L, generator=gen)
        self.cond = torch.randn(B, H, L, generator=gen)
        self.go = torch.randn(B, 1, M, L, generator=gen)
        self.spk = torch.randn(B, H, generator=gen) if ms else None
        t = torch.randint(1, 999, (B,), generator=gen)      # both ends of the schedule in every batch
        t[0] = 999
        if B > 1:
            t[B - 1] = 0
        self.t = t
        self.conditioned = condition_relu_kinks(self.W64, self.x, self.t, self.cond, self.spk, self.go, DEN_FT, gen)
        self._ref = self._ref_gpu = self._f32 = None

    def ref(self):
        if self._ref is None:
            self._ref = oracle_grads(self.W64, self.x, self.t, self.cond, self.spk, self.go, torch.float64)
        return self._ref

    def ref_gpu(self, key):
        if self._ref_gpu is None:
            self._ref_gpu = {k: v.cuda() for k, v in self.ref().items()}
        return self._ref_gpu[key]

    def f32_cpu_error(self, kind):
        if self._f32 is None:
            self._f32 = den_f32_cpu_errors(self.W32, self.x, self.t, self.cond, self.spk, self.go, self.ref())
        return self._f32[kind]

    def batch_of_one(self, b):
        c = Case.__new__(Case)
        c.name, c.B, c.L, c.ms = self.name, 1, self.L, self.ms
        c.den, c.W64, c.W32 = self.den, self.W64, self.W32
        c.x, c.cond, c.go, c.t = self.x[b:b + 1], self.cond[b:b + 1], self.go[b:b + 1], self.t[b:b + 1]
        c.spk = None if self.spk is None else self.spk[b:b + 1]
        c._ref = c._ref_gpu = c._f32 = None
        return c


def _case(mg, name, B, L):
    key = (name, B, L)
    if key not in _CASES:
        _CASES[key] = Case(mg, name, B, L)
    return _CASES[key]


def _conv_plan(B, Ci, L, rows, K, epi):
    """The form conv_launch picks for a denoiser conv (no scratch: the denoiser passes none)."""
    p = _lib.ConvPlan()
    rc = _lib.lib().mg_conv1d_fwd_plan(B, Ci, L, rows, K, 1, 1, 0, epi, ctypes.byref(p))
    assert rc == 0, rc
    assert p.ksplit == 1
    return p.mw, p.wm, p.nnb


def _layer_forms(name, B, L):
    """(EpiCond, EpiGate, EpiResSkip) forms of one generic layer: den_fwd_layers' three ConvShapes."""
    NL, C, H, M, ms = DEN_SIZES[name]
    return (_conv_plan(B, H, L, C, 1, _lib.MG_CONV_EPI_PLAIN), _conv_plan(B, C, L, 2 * C, 3, _lib.MG_CONV_EPI_NEEDS_WM2),
            _conv_plan(B, C, L, 2 * C, 1, _lib.MG_CONV_EPI_PLAIN))


def _fwd_path(case, mode):
    p = _lib.FwdPlan()
    dims = case.den._dims
    assert _lib.lib().mg_denoiser_fwd_plan(ctypes.byref(dims), case.B, case.L, mode, 0, 0, ctypes.byref(p)) == 0
    return p.path


# ------------------------------------------------------------------------------------------ the forms the cases reach
def test_conv_forms_reached():
    """A change of conv_plan's thresholds must fail here instead of silently moving the coverage: over the cases of
    this file whose layers are generic, EpiGate is reached with one and with two 32-frame blocks per wave, EpiCond and
    EpiResSkip each with one and with two 32-row blocks per wave; the small shapes keep the small forms and the
    large-form case is what adds the others."""
    generic = [n for n, (NL, C, H, M, ms) in DEN_SIZES.items() if (C, H) != (256, 256)]
    small = {(n, B, L): _layer_forms(n, B, L) for n in generic for B, L in DEN_SMALL_SHAPES}
    for n, B, L in [("G", B, L) for B, L in GENERIC_SHAPES]:       # under MG_DENOISER_GENERIC
        small[(n, B, L)] = _layer_forms(n, B, L)
    for key, (cond, gate, out) in small.items():
        print("DIMFORM %-14s cond %s gate %s out %s" % (key, cond, gate, out))
        assert gate == (2, 2, 1) and cond[1:] == (1, 1) and out[1:] == (1, 1), key
    big = _layer_forms(*DEN_LARGE_SHAPE)
    print("DIMFORM %-14s cond %s gate %s out %s" % (DEN_LARGE_SHAPE, *big))
    forms = list(small.values()) + [big]
    assert {g[2] for _, g, _ in forms} == {1, 2}, "EpiGate: one and two frame blocks per wave"
    assert all(g[1] == 2 for _, g, _ in forms), "EpiGate pairs two row blocks in every form"
    assert {c[1] for c, _, _ in forms} == {1, 2}, "EpiCond: one and two row blocks per wave"
    assert {o[1] for _, _, o in forms} == {1, 2}, "EpiResSkip: one and two row blocks per wave"


# ------------------------------------------------------------------------------------------ a. forward and backward
@pytest.mark.parametrize("B,L", DEN_SMALL_SHAPES, ids=["%dx%d" % s for s in DEN_SMALL_SHAPES])
@pytest.mark.parametrize("name", sorted(DEN_SIZES))
def test_forward_backward_vs_float64(mg, monkeypatch, name, B, L):
    """out, d_x, d_cond, d_spk and every parameter gradient elementwise against float64, on the default path and under
    MG_DENOISER_PERSIST=0, and the two against each other."""
    assert "MG_DENOISER_GENERIC" not in os.environ, "this file's parent process runs the default kernels"
    case = _case(mg, name, B, L)
    ts = case.t.tolist()
    assert 999 in ts and (B == 1 or 0 in ts)
    single = 1 if name == "G" else 0
    assert _fwd_path(case, _lib.MG_FWD_SAVE) == single and _fwd_path(case, 0) == single
    label = "%s %dx%d" % (name, B, L)
    fails = []
    a, _ = den_run(case)
    den_judge(case, label + "/default", a, fails, tag="DIMERR")
    monkeypatch.setenv("MG_DENOISER_PERSIST", "0")
    assert _fwd_path(case, _lib.MG_FWD_SAVE) == 0
    b, adv = den_run(case)
    assert adv == 0, "MG_DENOISER_PERSIST=0 still ran the single-launch backward"
    den_judge(case, label + "/per-layer", b, fails, tag="DIMERR")
    assert sorted(a) == sorted(b) and ("d_spk" in a) == bool(case.ms)
    for k in a:
        e = den_err(a[k], b[k])
        if not e <= den_bar(k):
            fails.append("%s default vs per-layer %s: %.3e > %.1e" % (label, k, e, den_bar(k)))
    assert not fails, "\n".join(fails)


def test_run_pair_declines_other_sizes(mg):
    """train_step.py and diffusion.py fall back to two forwards when run_pair returns None."""
    case = _case(mg, "A", 2, 63)
    x, t, cond = case.x[:, 0].contiguous().cuda(), case.t.cuda(), case.cond.cuda()
    assert case.den.run_pair(x, t, x.clone(), t.clone(), cond, None) is None
    case.den.check()


# ------------------------------------------------------------------------------------------ b. the large forms
def test_large_forms_size_c(mg):
    """Size C at B = 16, L = 700: head, cond and skip convs with two row blocks per wave, gate and out convs with two
    frame blocks too (test_conv_forms_reached).  Utterances 0 and 15 against float64 (utterances are independent);
    every utterance's out / d_x / d_cond against its single-utterance run and the parameter gradients against the sum
    of the 16 single-utterance runs' -- those take the small forms, which test_forward_backward_vs_float64 ties to
    float64."""
    name, B, L = DEN_LARGE_SHAPE
    case = _case(mg, name, B, L)
    fails = []
    got, _ = den_run(case)
    data = ("out", "d_x", "d_cond")
    total = None
    assert _layer_forms(name, 1, L) == ((2, 1, 1), (2, 2, 1), (2, 1, 1)), "a single utterance takes the small forms"
    for b in range(B):
        one = case.batch_of_one(b)
        o, _ = den_run(one)
        for k in data:
            e = den_err(got[k][b:b + 1], o[k])
            if not e <= den_bar(k):
                fails.append("%s[%d] in the batch vs alone: %.3e > %.1e" % (k, b, e, den_bar(k)))
        params = {k: v.clone() for k, v in o.items() if k.startswith("param/")}
        total = params if total is None else {k: total[k] + v for k, v in params.items()}
        if b in (0, B - 1):
            den_judge(one, "C 16x700 utterance %d" % b, {k: got[k][b:b + 1] for k in data}, fails, tag="DIMERR")
    worst = {}
    for k, v in total.items():
        e = den_err(got[k], v)
        worst[k] = e
        if not e <= den_bar(k):
            fails.append("%s vs the sum over single-utterance runs: %.3e > %.1e" % (k, e, den_bar(k)))
    print("DIMERR %-28s %-52s %.3e" % ("C 16x700 vs sum of singles", "param/* (worst)", max(worst.values())))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ c. inference and p_sample
_DIFFUSIONS = {}


def _diffusion(mg, name, tmp_path_factory):
    """GaussianDiffusion of a size (T = 4) with seeded weights; its weights and buffers as float64 for the oracle."""
    if name not in _DIFFUSIONS:
        NL, C, H, M, ms = DEN_SIZES[name]
        stats = write_stats(tmp_path_factory.mktemp("stats" + name), np.linspace(-11.5, -9.0, M), np.linspace(1.0, 2.0, M))
        args, _, _, tr = hot_path_configs("naive", T_STEPS, stats_dir=stats)
        pre, mc = den_size_configs(name)
        pre["path"] = {"preprocessed_path": stats}
        torch.manual_seed(4300 + ord(name))
        gd = mg.GaussianDiffusion(args, pre, mc, tr)
        live_output_projection(gd.denoise_fn, 4400 + ord(name))
        W = {k: v.detach().clone().double() for k, v in gd.state_dict().items() if k.startswith("denoise_fn.")}
        buf = {k: v.detach().clone().double() for k, v in gd._buf().items()}
        assert gd.num_timesteps == T_STEPS
        _DIFFUSIONS[name] = (gd.cuda().eval(), W, buf)
    return _DIFFUSIONS[name]


def _infer_inputs(name, B, L):
    NL, C, H, M, ms = DEN_SIZES[name]
    gen = torch.Generator().manual_seed(77 * B + L + 100003 * ord(name))
    x = torch.randn(B, 1, M, L, generator=gen)
    cond = torch.randn(B, H, L, generator=gen)
    spk = torch.randn(B, H, generator=gen) if ms else None
    noise = [torch.randn(B, 1, M, L, generator=gen) for _ in range(T_STEPS)]
    t = torch.tensor([T_STEPS - 1 if b % 2 == 0 else 0 for b in range(B)])      # both ends of the schedule
    return x, cond, spk, noise, t


@pytest.mark.parametrize("B,L", GENERIC_SHAPES, ids=["%dx%d" % s for s in GENERIC_SHAPES])
@pytest.mark.parametrize("name", ["A", "D", "E"])
def test_inference_and_p_sample(mg, tmp_path_factory, name, B, L):
    """The non-saving workspace (ws.x0 aliases ws.x) and psample_tail_kernel behind the fused (D) and the generic (A, E)
    tail, against the float64 oracle; a sampling loop equals its explicit steps bit for bit."""
    gd, W, buf = _diffusion(mg, name, tmp_path_factory)
    den = gd.denoise_fn
    x, cond, spk, noise, t = _infer_inputs(name, B, L)
    assert 0 in t.tolist() and T_STEPS - 1 in t.tolist()
    xg, cg, tg = x.cuda(), cond.cuda(), t.cuda()
    sg = None if spk is None else spk.cuda()
    sd = None if spk is None else spk.double()
    label = "%s %dx%d" % (name, B, L)
    fails = []

    def judge(what, got, ref):
        e = den_err(got.cpu(), ref)
        print("DIMERR %-28s %-52s %.3e" % (label, what, e))
        if not e <= DEN_FT:
            fails.append("%s %s: %.3e > %.1e" % (label, what, e, DEN_FT))

    # big t for the bare forward: the step embedding at both ends of the training schedule
    t_fwd = torch.tensor([999 if b % 2 == 0 else 0 for b in range(B)])
    with torch.no_grad():
        out = den(xg, t_fwd.cuda(), cg, sg)
        ref = R.denoiser_forward(W, "denoise_fn.", x.double(), t_fwd, cond.double(), sd)
    judge("out (no_grad)", out, ref)
    for clip in (True, False):
        gd.noise_fn = Tape([noise[0].numpy()])
        got = gd.p_sample(xg, tg, cg, sg, clip_denoised=clip)
        ref = R.p_sample(W, buf, x.double(), t, cond.double(), sd, noise[0].double(), clip=clip)
        judge("p_sample clip=%s" % clip, got, ref)
    packed = den.packed_weights()
    if name == "A":
        assert den.has_cond_projection() is False
        assert gd._loop_cond_buffer(cg, packed) is None
    else:
        assert den.has_cond_projection() is True
    # sampling(keep_trace=False) = T explicit p_sample steps under the same tape, bit for bit
    gd.cond, gd.spk_emb = cg, sg
    gd.noise_fn = Tape([x.numpy()] + [n.numpy() for n in noise])
    mel = gd.sampling(keep_trace=False)[-1]
    gd.noise_fn = Tape([n.numpy() for n in noise])
    xs = xg
    for i in reversed(range(T_STEPS)):
        xs = gd.p_sample(xs, torch.full((B,), i, dtype=torch.long, device="cuda"), cg, sg)
    from mixgan_tts_amd import ops
    explicit = ops.transpose_bml(xs[:, 0].contiguous(), True, 2, gd.spec_min, gd.spec_max)
    gd.noise_fn = None
    gd.cond = gd.spk_emb = None
    den.check()
    assert mel.shape == (B, L, DEN_SIZES[name][3])
    assert torch.equal(mel, explicit), "sampling() differs from its explicit steps: %.3e" % den_err(mel, explicit)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ d. MG_DENOISER_GENERIC
def _child(out_path):
    """Runs in a fresh process with MG_DENOISER_GENERIC set: size G, grad-mode forward and backward at GENERIC_SHAPES,
    everything into one .npz; nothing else on the GPU."""
    import mixgan_tts_amd as m
    assert os.environ.get("MG_DENOISER_GENERIC") and torch.cuda.is_available()
    res = {}
    for B, L in GENERIC_SHAPES:
        case = _case(m, "G", B, L)
        res["path/%dx%d" % (B, L)] = np.array([_fwd_path(case, _lib.MG_FWD_SAVE), _fwd_path(case, 0)])
        got, _ = den_run(case)
        for k, v in got.items():
            res["%dx%d/%s" % (B, L, k)] = v.cpu().numpy()
    torch.cuda.synchronize()
    np.savez(out_path, **res)


def test_generic_layers_at_the_default_size(mg, tmp_path):
    """MG_DENOISER_GENERIC at C = H = 256, M = 80 (the leg bench.py prices): the generic layers, head and tail and the
    generic saving layout feeding the backward, in a child process because the flag is read once per process.  The
    child's results against float64 and against this process's default-path results, at the same bars."""
    out = str(tmp_path / "generic.npz")
    env = dict(os.environ, MG_DENOISER_GENERIC="1")
    for k in PINS:
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, "the MG_DENOISER_GENERIC child failed (%d):\n%s" % (r.returncode, r.stderr[-4000:])
    child = np.load(out)
    fails = []
    for B, L in GENERIC_SHAPES:
        case = _case(mg, "G", B, L)
        assert child["path/%dx%d" % (B, L)].tolist() == [0, 0], "the child did not leave the single launch"
        assert _fwd_path(case, _lib.MG_FWD_SAVE) == 1
        pre = "%dx%d/" % (B, L)
        got = {k[len(pre):]: torch.from_numpy(child[k]).cuda() for k in child.files if k.startswith(pre)}
        mine, _ = den_run(case)
        assert sorted(got) == sorted(mine)
        den_judge(case, "G %dx%d/generic" % (B, L), got, fails, tag="DIMERR")
        for k in got:
            e = den_err(got[k], mine[k])
            if not e <= den_bar(k):
                fails.append("G %dx%d generic vs default %s: %.3e > %.1e" % (B, L, k, e, den_bar(k)))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ the chunked pack
def test_pack_in_several_launches(mg):
    """120 layers at C = 64, multi-speaker: 9 + 8 * 120 jobs for the forward packs and 3 + 3 * 120 more for the backward
    packs, two launches of the 768-entry job table each way (tests/test_denoiser_pack_cpu.py has the counts).  A wrong
    table offset in the second launch would leave layers unpacked: forward, data and parameter gradients against
    float64, again after a repack of the same tensors (MG_DEN_JOBS_RESIDENT is passed then, and must be ignored)."""
    NL = SIZES["P"][0]
    case = _case(mg, "P", 2, 63)
    den = case.den
    jobs, launches = ctypes.c_int(), ctypes.c_int()
    table = den._weight_table()
    ptrs = (ctypes.c_void_p * len(table))(*[None if p is None else p.data_ptr() for p in table])
    for flags, want in ((0, 9 + 8 * NL), (_lib.MG_DEN_BACKWARD, 12 + 11 * NL)):
        assert _lib.lib().mg_denoiser_pack_plan(ctypes.byref(den._dims), ptrs, ptrs[0], ptrs[0], flags, ctypes.byref(jobs),
                                                ctypes.byref(launches)) == 0
        assert (jobs.value, launches.value) == (want, 2)
    fails = []
    x, t, cond, spk = case.x.cuda(), case.t.cuda(), case.cond.cuda(), case.spk.cuda()
    with torch.no_grad():
        out = den(x, t, cond, spk)                      # the inference packs
    den.check()
    den_judge(case, "P 2x63/inference packs", {"out": out}, fails, tag="DIMERR")
    got, _ = den_run(case)                              # the training packs
    den_judge(case, "P 2x63/training packs", got, fails, tag="DIMERR")
    with torch.no_grad():
        den.output_projection.conv.bias.add_(0.0)       # a new version of one tensor: the next call repacks in place
    resident = []
    pack = _lib.lib().mg_denoiser_pack
    try:
        _lib.lib().mg_denoiser_pack = lambda d, w, f, p, flags, st: (resident.append(flags), pack(d, w, f, p, flags, st))[1]
        again, _ = den_run(case)
    finally:
        _lib.lib().mg_denoiser_pack = pack
    assert resident and all(f & _lib.MG_DEN_JOBS_RESIDENT for f in resident), "the repack did not pass MG_DEN_JOBS_RESIDENT"
    den_judge(case, "P 2x63/repacked", again, fails, tag="DIMERR")
    assert not fails, "\n".join(fails)


if __name__ == "__main__":
    _child(sys.argv[1])
