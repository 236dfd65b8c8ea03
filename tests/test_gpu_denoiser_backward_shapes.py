"""The denoiser backward (mg_denoiser_bwd behind autograd.DenoiserFn) at the shapes it trains at, against float64
autograd through the CPU oracle, elementwise, on both data-gradient paths: the single persistent launch
(denoiser_bwd_persist.h) and the two launches per layer (MG_DENOISER_PERSIST=0, more tiles per utterance than a quarter
of the CUs, fewer than 3 layers).  Which path ran is read from the backward workspace's counters
(Denoiser.backward_status), so "both paths agree" cannot pass on one path run twice.

Bars (max-abs error / max-abs reference, per tensor): the project's own, 2e-5 forward, 5e-5 data gradients, 1e-4
parameter gradients -- here against a float64 reference, which has no rounding of its own to hide behind.  A tensor
that misses its bar is judged against the float32 CPU oracle's autograd error at the same shape and seed instead: 8 x
that error (another summation order over the same number of fp32 terms, not another algorithm), and only where that is
above the project bar.  Measured on an MI355X (the table is in DESIGN.md section 7.1): no case needed that rule; the
worst error of any case is 2.0e-6 forward, 1.4e-6 d_x, 3.7e-6 d_cond, 1.4e-6 d_spk, 5.1e-6 on a parameter gradient
(a conv_layer weight at B=16, L=1000).  Each test prints its worst error per tensor kind (`BWDERR` lines, -s).

Inputs are standard normal from fixed generators, then conditioned (helpers.condition_relu_kinks): the gradient is
discontinuous where a ReLU input is zero, and with plain inputs every case of 8 000 frames or more had one 32-frame
tile whose d_x was off by 2e-2 -- a ReLU input that fp32 and fp64 put on different sides of zero (which one depended on
the forward form, not on the backward path), not a kernel fault.  The conditioning keeps those elements out of the
gradient; the product computes on the inputs as given."""
import ctypes
import json
import os

import pytest
import torch

from helpers import GOLDEN, hot_path_configs, seeded, oracle_grads, condition_relu_kinks
# shared with test_gpu_denoiser_dims.py: the bars, the error measure, the one run and the judgement with its fallback
from helpers import DEN_FT as FT
from helpers import den_bar as _bar, den_err as _err, den_run as _run, den_judge as _judge
from helpers import den_f32_cpu_errors
from oracle import weights as WR
from mixgan_tts_amd import _lib

pytestmark = pytest.mark.gpu
SEED = {0: 78, 1: 79}
# Reduced with fp32 atomics, so not bit-reproducible run to run: small_linear_t_kernel with Z = n_layers adds every
# layer's product into the step-vector gradient (bws.ds), which the two mlp weight gradients are computed from, and in
# multi-speaker into d_spk.  Every other reduction of mg_denoiser_bwd has a fixed order (split-K through scratch).
ATOMIC = ("d_spk", "param/mlp.0.linear.weight", "param/mlp.2.linear.weight")


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd as m
    assert torch.cuda.is_available()
    m.lib()
    return m


@pytest.fixture(autouse=True)
def _default_paths(monkeypatch):
    for k in ("MG_DENOISER_PERSIST", "MG_PERSIST_NT", "MG_PERSIST_SOLO", "MG_PERSIST_TEAM"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------ models, inputs, references
_MODELS, _CASES = {}, {}


def _model(mg, ms, n_layers=20):
    """(product Denoiser on the GPU, the same seeded weights as float64 leaves for the oracle), one per configuration."""
    key = (ms, n_layers)
    if key not in _MODELS:
        with open(os.path.join(GOLDEN, "manifest.json")) as f:
            manifest = json.load(f)
        name = "denoiser_ms%d" % ms
        if n_layers == 20:
            W32, _ = seeded(manifest, name, SEED[ms])
        else:   # the manifest entry cut to the first n_layers layers, drawn by the same recipe
            cut = {k: v for k, v in manifest[name]["seeded"].items()
                   if not k.startswith("residual_layers.") or int(k.split(".")[1]) < n_layers}
            W32 = {k: torch.from_numpy(a) for k, a in WR.draw(cut, SEED[ms]).items()}
        _, pre, mc, _ = hot_path_configs(multi_speaker=bool(ms), stats_dir=None)
        mc["denoiser"]["residual_layers"] = n_layers
        den = mg.Denoiser(pre, mc)
        sd = den.state_dict()
        assert sorted(sd) == sorted(W32), "state_dict keys differ from the weight recipe"
        den.load_state_dict({k: W32[k].clone() for k in sd})
        W64 = {k: v.double().requires_grad_() for k, v in W32.items()}
        _MODELS[key] = (den.cuda(), W64, W32)
    return _MODELS[key]


class Case:
    """Fixed inputs of one (B, L, speakers, layers) and their float64 reference, computed once."""

    def __init__(self, mg, B, L, ms, n_layers=20, t_one=999, salt=0):
        self.B, self.L, self.ms, self.n_layers = B, L, ms, n_layers
        self.den, self.W64, self.W32 = _model(mg, ms, n_layers)
        gen = torch.Generator().manual_seed(1000 * B + L + 7 * ms + n_layers + 100003 * salt)
        self.x = torch.randn(B, 1, 80, L, generator=gen)
        self.cond = torch.randn(B, 256, L, generator=gen)
        self.go = torch.randn(B, 1, 80, L, generator=gen)
        self.spk = torch.randn(B, 256, generator=gen) if ms else None
        # both ends of the schedule in every batch; a batch of one takes the end its case names
        t = torch.randint(1, 999, (B,), generator=gen)
        if B == 1:
            t[0] = t_one
        else:
            t[0], t[B - 1] = 999, 0
        self.t = t
        # keep every ReLU input of the float64 forward further from zero than the forward's own bar, where it matters
        self.conditioned = condition_relu_kinks(self.W64, self.x, self.t, self.cond, self.spk, self.go, FT, gen)
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
        """The yardstick for a missed bar: the float32 CPU oracle's autograd error against the float64 one at this
        shape and seed, worst tensor of the kind."""
        if self._f32 is None:
            self._f32 = den_f32_cpu_errors(self.W32, self.x, self.t, self.cond, self.spk, self.go, self.ref())
        return self._f32[kind]

    def batch_of_one(self, mg, b):
        c = Case.__new__(Case)
        c.B, c.L, c.ms, c.n_layers = 1, self.L, self.ms, self.n_layers
        c.den, c.W64, c.W32 = self.den, self.W64, self.W32
        c.x, c.cond, c.go, c.t = self.x[b:b + 1], self.cond[b:b + 1], self.go[b:b + 1], self.t[b:b + 1]
        c.spk = None if self.spk is None else self.spk[b:b + 1]
        c._ref = c._ref_gpu = c._f32 = None
        return c


def _case(mg, B, L, ms, n_layers=20, t_one=999, salt=0):
    key = (B, L, ms, n_layers, t_one, salt)
    if key not in _CASES:
        _CASES[key] = Case(mg, B, L, ms, n_layers, t_one, salt)
    return _CASES[key]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _single_launch_expected(case):
    """mg_denoiser_bwd's own condition: at least 3 layers, an utterance's chain of 32-frame tiles within a quarter of
    the CUs, and no MG_DENOISER_PERSIST=0."""
    return (os.environ.get("MG_DENOISER_PERSIST", "1")[:1] != "0" and case.n_layers >= 3
            and -(-case.L // 32) <= _cus() // 4)


# ------------------------------------------------------------------------------------------ 2. shapes x paths
# L "cap" = the longest utterance the single launch takes on this device (32 frames x a quarter of the CUs: 2048 on 256
# CUs), "cap+4" the first float4-aligned one that falls back by itself.
SHAPES = [
    ("bench", 8, 1000, 1, 20, 999),          # the benchmark's training shape: 256 tiles on 256 one-per-CU slots
    ("2x-slots", 16, 1000, 0, 20, 999),      # 512 tiles on 256 slots; 64-frame save forward
    ("2x-slots-ms", 16, 1000, 1, 20, 999),
    ("scalar-staging", 5, 1001, 0, 20, 999),  # L % 4 != 0: VEC4 = false, 9 valid frames in the last tile, unaligned rows
    ("one-frame", 3, 1, 0, 20, 999),
    ("partial-tile", 2, 31, 1, 20, 999),
    ("exact-tile", 1, 32, 0, 20, 999),
    ("one-over", 3, 33, 1, 20, 999),
    ("smallest-float4", 2, 4, 0, 20, 999),
    ("longest-chain", 2, "cap", 0, 20, 999),
    ("first-fallback", 2, "cap+4", 0, 20, 999),
    ("per-layer-by-shape", 1, 4000, 0, 20, 0),
    ("two-layers", 3, 131, 1, 2, 999),       # NL < 3: the hand-off tags need three layers
]


@pytest.mark.parametrize("label,B,L,ms,n_layers,t_one", SHAPES, ids=[s[0] for s in SHAPES])
def test_backward_vs_float64_on_both_paths(mg, monkeypatch, label, B, L, ms, n_layers, t_one):
    """Output (the save-mode forward forms), d_x, d_cond, d_spk and every parameter gradient elementwise against
    float64, on the default path and under MG_DENOISER_PERSIST=0 (forward and backward launch per layer), and the two
    paths against each other; `launches` advances exactly where the single launch is expected."""
    if isinstance(L, str):
        L = 32 * (_cus() // 4) + (4 if L.endswith("+4") else 0)
    case = _case(mg, B, L, ms, n_layers, t_one)
    ts = case.t.tolist()
    assert (0 in ts and 999 in ts) if B > 1 else ts[0] in (0, 999)
    fails = []
    expect = _single_launch_expected(case)
    if label in ("bench", "2x-slots", "2x-slots-ms", "scalar-staging", "longest-chain"):
        assert expect, "this case is here for the single launch"
    if label in ("first-fallback", "per-layer-by-shape", "two-layers"):
        assert not expect, "this case is here for the fallback"
    a, adv = _run(case)
    assert adv == (1 if expect else 0), "default path: launches advanced by %d, single launch expected: %s" % (adv, expect)
    _judge(case, label + "/default", a, fails)
    monkeypatch.setenv("MG_DENOISER_PERSIST", "0")
    b, adv = _run(case)
    assert adv == 0, "MG_DENOISER_PERSIST=0 still ran the single launch"
    _judge(case, label + "/per-layer", b, fails)
    for k in a:
        e = _err(a[k], b[k])
        if not e <= _bar(k):
            fails.append("%s default vs per-layer %s: %.3e > %.1e" % (label, k, e, _bar(k)))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ 4. hand-offs, full occupancy
@pytest.mark.parametrize("B,ms", [(16, 1), (40, 0)])
def test_backward_handoffs_under_full_occupancy(mg, monkeypatch, B, ms):
    """B=16 / B=40 at L=1000: 512 / 1280 tiles on one-per-CU slots, later tiles taking their ticket as earlier utterances
    finish, every tile waiting on both neighbours' dz columns in every layer.  Two backwards on the same inputs are
    bit-identical in everything but the atomically reduced tensors (ATOMIC); d_x[b] and d_cond[b] equal bit for bit what
    the utterance gives in a batch of one.  mg_denoiser_bwd has no batch-dependent reduction order on that path (the
    data-gradient GEMMs take no split-K scratch, the persistent kernel works per tile), but the SAVING FORWARD has: it
    picks 32-frame 8-wave tiles at B=1 and 64-frame 4-wave tiles from B=16 on (test_denoiser_plan_cpu.py), so the
    forward form is pinned to 64 -- the default at B=16 and B=40 -- for the batches of one to save the same bits."""
    monkeypatch.setenv("MG_PERSIST_NT", "64")
    L = 1000
    case = _case(mg, B, L, ms)
    assert _single_launch_expected(case)
    r1, adv1 = _run(case)
    r2, adv2 = _run(case)
    assert (adv1, adv2) == (1, 1)
    fails = []
    for k in r1:
        if k in ATOMIC:
            continue
        if not torch.equal(r1[k], r2[k]):
            fails.append("%s differs between two runs: %.3e" % (k, _err(r1[k], r2[k])))
    atomic = [k for k in r1 if k in ATOMIC]
    assert len(atomic) == (3 if ms else 2)
    if B == 16:      # the full float64 reference is the shape matrix's (cached)
        _judge(case, "handoff B=16 run 1", r1, fails)
        _judge(case, "handoff B=16 run 2", r2, fails, keys=atomic)
    else:            # no full reference at B=40 (CPU time): the atomically reduced tensors of the two runs at their bar
        for k in atomic:
            e = _err(r1[k], r2[k])
            if not e <= _bar(k):
                fails.append("%s run 1 vs run 2: %.3e > %.1e" % (k, e, _bar(k)))
    for b in sorted({0, 7, 15, B - 1}):
        one = case.batch_of_one(mg, b)
        o, adv = _run(one)
        assert adv == 1
        for k in ("out", "d_x", "d_cond"):
            if not torch.equal(o[k][0], r1[k][b]):
                fails.append("%s[%d] in the batch differs from the batch of one: %.3e" % (k, b, _err(r1[k][b], o[k][0])))
        if B == 40 and b in (0, B - 1):
            _judge(one, "handoff B=40 utterance %d" % b, {k: r1[k][b:b + 1] for k in ("out", "d_x", "d_cond")}, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------ 5. NULL gradient pointers
SENTINEL = 12345.0


def _abi_backward(mg, case, ws, want_head, want_kind, want_dx, want_dcond, want_dspk, break_layer_major=False):
    """mg_denoiser_bwd through ctypes.  Every buffer exists and is pre-filled with SENTINEL; the ones not wanted are
    passed as NULL.  Returns ({name: tensor} of all buffers, set of the requested names, return code)."""
    den = case.den
    lib = _lib.lib()
    d = den._dims
    B, L, NL = case.B, case.L, d.n_layers
    table = den._weight_table()
    HEAD, PER_LAYER = _lib.MG_DEN_HEAD_PTRS, _lib.MG_DEN_LAYER_PTRS
    slot = lambda l, j: HEAD + PER_LAYER * l + j  # noqa: E731
    names = {id(p): "param/" + k for k, p in den.named_parameters()}
    full = lambda *shape: torch.full(shape, SENTINEL, device="cuda")  # noqa: E731
    head = [full(*p.shape) for p in table[:HEAD]]
    kinds = [None if table[slot(0, j)] is None else full(NL, *table[slot(0, j)].shape) for j in range(PER_LAYER)]
    bufs, asked, ptrs = {}, set(), []
    for i in range(HEAD):
        bufs[names[id(table[i])]] = head[i]
        if want_head(i):
            asked.add(names[id(table[i])])
        ptrs.append(head[i].data_ptr() if want_head(i) else None)
    for l in range(NL):
        for j in range(PER_LAYER):
            if kinds[j] is None:
                ptrs.append(None)
                continue
            bufs[names[id(table[slot(l, j)])]] = kinds[j][l]
            if want_kind(j):
                asked.add(names[id(table[slot(l, j)])])
            ptrs.append(kinds[j][l].data_ptr() if want_kind(j) else None)
    if break_layer_major:      # layer 1's conv_layer weight is not layer 0's plus one layer
        ptrs[slot(1, _lib.MG_DEN_L_CONV_W)] = kinds[_lib.MG_DEN_L_CONV_W][2].data_ptr()
    x, cond, go = case.x[:, 0].contiguous().cuda(), case.cond.cuda(), case.go[:, 0].contiguous().cuda()
    spk = case.spk.cuda() if case.ms else None
    bufs["d_x"], bufs["d_cond"] = full(*x.shape), full(*cond.shape)
    if case.ms:
        bufs["d_spk"] = full(*spk.shape)
    for k, w in (("d_x", want_dx), ("d_cond", want_dcond), ("d_spk", want_dspk and case.ms)):
        if w:
            asked.add(k)
    bws = torch.zeros(lib.mg_denoiser_bwd_workspace_floats(ctypes.byref(d), B, L), device="cuda")
    opt = lambda k: _lib.fptr(bufs[k] if k in asked else None, True)  # noqa: E731
    rc = lib.mg_denoiser_bwd(ctypes.byref(d), _lib.fptr(den.packed_weights(with_backward=True)), _lib.fptr(go), _lib.fptr(x),
                             _lib.fptr(cond), _lib.fptr(spk, True), _lib.fptr(ws), _lib.fptr(bws), bws.numel(),
                             (ctypes.c_void_p * len(ptrs))(*ptrs), opt("d_x"), opt("d_cond"), opt("d_spk"), B, L,
                             _lib.stream_ptr())
    torch.cuda.synchronize()
    bufs["d_x"] = bufs["d_x"][:, None]      # [B, 1, M, L] like the reference's
    return bufs, asked, rc


# every head slot / every per-layer kind (the header's MG_DEN_L_* names) but one
_all, _but = (lambda i: True), (lambda kind: lambda j: j != kind)
POINTER_SETS = [
    ("conv3 weights, no conv3 biases (fold3 false)", _all, _but(_lib.MG_DEN_L_CONV_B), True, True, True),
    ("conv3 biases, no conv3 weights (mg_rowsum over dz)", _all, _but(_lib.MG_DEN_L_CONV_W), True, True, True),
    ("output-conv weights, no biases (foldo false)", _all, _but(_lib.MG_DEN_L_OUT_B), True, True, True),
    ("output-conv biases, no weights (mg_rowsum + bias_scatter_kernel)", _all, _but(_lib.MG_DEN_L_OUT_W), True, True, True),
    ("conditioner weights, no biases (foldc false)", _all, _but(_lib.MG_DEN_L_COND_B), True, True, True),
    ("conditioner biases, no weights", _all, _but(_lib.MG_DEN_L_COND_W), True, True, True),
    ("no parameter gradients, only d_x_t", lambda i: False, lambda j: False, True, False, False),
    ("no d_x_t, no d_cond", _all, _all, False, False, True),
]


@pytest.mark.parametrize("B,L,ms", [(3, 131, 0), (2, 64, 1)])
def test_null_gradient_pointers_through_the_c_abi(mg, B, L, ms):
    """include/mixgan_hip.h: any gradient pointer may be NULL.  That selects the unfolded reductions of
    mg_denoiser_bwd_staged (separate mg_rowsum launches, bias_scatter_kernel), which the Python wrapper never asks for.
    Every requested tensor equals the all-requested run's within GT / 1e-4 and meets the float64 bars; buffers that
    were not requested keep their sentinel."""
    case = _case(mg, B, L, ms)
    den = case.den
    den.run(case.x[:, 0].contiguous().cuda(), case.t.cuda(), case.cond.cuda(), case.spk.cuda() if ms else None, save=True)
    ws = den.last_ws
    fails = []
    try:
        base, asked, rc = _abi_backward(mg, case, ws, lambda i: True, lambda j: True, True, True, True)
        assert rc == 0
        assert asked == set(base), "the baseline requests everything"
        _judge(case, "abi B=%d L=%d all" % (B, L), base, fails, keys=sorted(asked))
        for what, want_head, want_kind, dx, dcond, dspk in POINTER_SETS:
            got, asked, rc = _abi_backward(mg, case, ws, want_head, want_kind, dx, dcond, dspk)
            assert rc == 0, (what, rc)
            assert asked and asked != set(got), what
            for k, v in got.items():
                if k not in asked:
                    if not bool((v == SENTINEL).all()):
                        fails.append("%s: %s was not requested and was written" % (what, k))
                    continue
                e = _err(v, base[k])
                if not e <= _bar(k):
                    fails.append("%s: %s vs the all-requested run %.3e > %.1e" % (what, k, e, _bar(k)))
            _judge(case, "abi B=%d L=%d %s" % (B, L, what.split(" (")[0]), got, fails, keys=sorted(asked))
        again, asked, rc = _abi_backward(mg, case, ws, lambda i: True, lambda j: True, True, True, True)
        assert rc == 0
        for k in sorted(set(again) - set(ATOMIC)):
            assert torch.equal(again[k], base[k]), "the backward changed the saved activations: " + k
    finally:
        ws._mg_busy = False
    assert not fails, "\n".join(fails)


def test_layer_major_pointer_check(mg):
    """Per-layer gradients must be slices of one [n_layers, ...] buffer: MG_ERR_ARG when layer 1's pointer is not
    layer 0's plus one layer, and nothing is written."""
    case = _case(mg, 2, 64, 1)
    den = case.den
    den.run(case.x[:, 0].contiguous().cuda(), case.t.cuda(), case.cond.cuda(), case.spk.cuda(), save=True)
    ws = den.last_ws
    try:
        got, _, rc = _abi_backward(mg, case, ws, lambda i: True, lambda j: True, True, True, True, break_layer_major=True)
    finally:
        ws._mg_busy = False
    assert rc == _lib.MG_ERR_ARG
    for k, v in got.items():
        assert bool((v == SENTINEL).all()), k + " was written by a call that returned an error"
    with pytest.raises(mg.MixganHipError):
        mg._lib.check(rc)


# ------------------------------------------------------------------------------------------ 6. workspace lifetime
def _forward(case):
    x, cond = case.x.cuda().requires_grad_(), case.cond.cuda().requires_grad_()
    spk = case.spk.cuda().requires_grad_() if case.ms else None
    out = case.den(x, case.t.cuda(), cond, spk)
    return x, cond, spk, out


def _collect(case, x, cond, spk, out):
    got = {"out": out.detach(), "d_x": x.grad, "d_cond": cond.grad}
    if case.ms:
        got["d_spk"] = spk.grad
    for k, p in case.den.named_parameters():
        got["param/" + k] = p.grad
    return got


def test_saved_activations_outlive_a_second_forward_and_the_guard(mg):
    """Two grad-mode forwards of one shape before either backward: the second gets a workspace of its own (a saving
    workspace whose backward is pending is not handed out again, Denoiser._workspace), so BOTH backwards are valid and
    both are held to the float64 bars here.  run_backward's guard is for the case that is left: a backward that has run
    releases its workspace, a later forward of the shape overwrites it, and a second backward through the first graph
    (retain_graph) must raise rather than differentiate through the other forward's activations -- while the later
    forward's own backward still matches the reference."""
    a, b = _case(mg, 3, 131, 0), _case(mg, 3, 131, 0, salt=1)      # same shape, other inputs
    den = a.den
    fails = []
    den.zero_grad(set_to_none=True)
    fa, fb = _forward(a), _forward(b)
    (fa[3] * a.go.cuda()).sum().backward()
    _judge(a, "lifetime A, B pending", _collect(a, *fa), fails)
    den.zero_grad(set_to_none=True)
    (fb[3] * b.go.cuda()).sum().backward()
    _judge(b, "lifetime B after A", _collect(b, *fb), fails)
    den.zero_grad(set_to_none=True)
    # the guard
    fa = _forward(a)
    loss = (fa[3] * a.go.cuda()).sum()
    loss.backward(retain_graph=True)
    fb = _forward(b)                  # A's workspace is free again: this forward saves into it
    with pytest.raises(mg.MixganHipError, match="saved activations were overwritten"):
        loss.backward()
    den.zero_grad(set_to_none=True)
    (fb[3] * b.go.cuda()).sum().backward()
    _judge(b, "lifetime B after the guard", _collect(b, *fb), fails)
    den.zero_grad(set_to_none=True)
    den.check()
    assert not fails, "\n".join(fails)


def test_backward_workspace_cache_eviction(mg):
    """Five other shapes evict the first one's backward workspace from the four-entry cache; the first shape again gets
    a new zero-filled one (its counters start over) and still meets the bars."""
    first = _case(mg, 2, 40, 1)
    den = first.den
    den._bws.clear()
    fails = []
    got, adv = _run(first)
    assert adv == 1 and den.backward_status(2, 40)["launches"] == 1
    _judge(first, "cache first", got, fails)
    got, adv = _run(first)
    assert adv == 1 and den.backward_status(2, 40)["launches"] == 2, "a cached workspace keeps counting"
    for B, L in [(1, 64), (2, 33), (1, 100), (3, 20), (2, 70)]:
        _, adv = _run(_case(mg, B, L, 1))
        assert adv == 1
    assert len(den._bws) == 4 and not any(k[:2] == (2, 40) for k in den._bws)
    assert den.backward_status(2, 40) == {"ticket": 0, "error": 0, "launches": 0, "done": 0}
    got, adv = _run(first)
    assert adv == 1 and den.backward_status(2, 40)["launches"] == 1, "the recreated workspace starts from zero"
    _judge(first, "cache after eviction", got, fails)
    assert not fails, "\n".join(fails)
