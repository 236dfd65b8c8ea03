"""Every workgroup form (MW, WM, NNB) of the implicit-GEMM convolution kernel (csrc/conv_mfma.h) against a float64
torch.nn.functional reference on the CPU, through each C entry point that launches it: mg_conv1d_fwd_ex,
mg_conv_transpose1d_fwd, mg_conv_transpose1d_fwd_slice, mg_conv1d_reflect_fwd and mg_conv1x1_fwd_strided.

Each case (1) asks mg_conv1d_fwd_plan -- the function the launcher switches on -- for the form and asserts it is the one
the case was written for, so a change of the dispatch thresholds fails here instead of silently moving the coverage,
(2) runs the kernel, (3) compares with the reference at 1e-5 (max-abs error over max-abs reference: the figure
test_gpu_parity.py holds this kernel to at reductions five times deeper), (4) runs it again and requires the same bits (the
unsplit kernel sums in a fixed order), and (5) checks that the floats around the output, and between its rows where the
output is a slice of a wider buffer, are untouched.

Shapes are the smallest that select each form (FORMS); every length leaves a ragged last tile, and the second length of
the NNB = 2 forms ends inside the second 32-frame block of a wave.  Reductions are two chunks with the second part
filled: 40 channels where CK = 32, 24 where CK = 16."""
import ctypes
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
GUARD = 4096            # floats on each side of an output buffer (a multiple of 4: keeps the 16-byte alignment)
SENTINEL = 70001.5

# form -> GEMM rows, B, output frames, second length (tail of 40 frames: both 32-frame blocks of a wave's NNB = 2 pair)
FORMS = {
    (1, 1, 1): (5, 2, 300, None),
    (1, 1, 2): (5, 2, 65300, 65320),      # 255 tiles of 256 frames + 20 / + 40
    (2, 1, 1): (40, 3, 300, None),
    (2, 1, 2): (40, 16, 4100, 4136),      # 32 tiles of 128 + 4 / + 40
    (2, 2, 1): (130, 8, 2053, None),
    (2, 2, 2): (130, 16, 2053, 2088),     # 16 tiles of 128 + 5 / + 40; the second 128-row tile holds 2 live rows
}
ALL = tuple(FORMS)
NO_256 = tuple(f for f in ALL if f != (1, 1, 2))      # K = 3 and K = 5 / stride 2: the slab of a 256-frame tile is too large
PLAIN, REFLECT, SLICE = 0, 1, 2
ACTS = {"none": 0, "relu": 1, "lrelu": 2, "tanh": 3, "lrelu_s": 4}


def _fid(form):
    return "f%d%d%d" % form


def _lib():
    import mixgan_tts_amd as mg
    from mixgan_tts_amd import _lib as L
    assert L.MG_CONV_EPI_PLAIN == PLAIN and L.MG_CONV_EPI_REFLECT == REFLECT and L.MG_CONV_EPI_PHASES_SLICE == SLICE
    return mg.lib(), L


def _assert_form(form, B, Ci, Lout, rows, K, stride=1, dil=1, epi=PLAIN):
    lib, L = _lib()
    p = L.ConvPlan()
    rc = lib.mg_conv1d_fwd_plan(B, Ci, Lout, rows, K, stride, dil, 0, epi, ctypes.byref(p))
    assert rc == 0, rc
    assert (p.mw, p.wm, p.nnb) == form and p.ksplit == 1, "the plan gives (%d,%d,%d) x %d for a case written for %s" % (
        p.mw, p.wm, p.nnb, p.ksplit, form)
    assert (p.kw, p.stride) == (K, stride) and p.dilmax >= dil and p.ck == (32 if K <= 3 else 16)
    return p


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ci(K):
    return 40 if K <= 3 else 24


def _guarded(n, fill=None):
    """A flat CUDA buffer of n floats between two guards; returns (whole buffer, the n floats)."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda", dtype=torch.float32)
    body = buf[GUARD:GUARD + n]
    if fill is not None:
        body.copy_(fill.reshape(-1))
    return buf, body


def _check_guards(buf, what):
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), what + ": wrote outside the output"


def _twice(launch, n, prefill=None):
    """Run `launch(out_flat)` on two fresh guarded buffers; require equal bits and clean guards; return the first body."""
    bodies = []
    for _ in range(2):
        buf, body = _guarded(n, prefill)
        launch(body)
        torch.cuda.synchronize()
        _check_guards(buf, "launch")
        bodies.append(body)
    assert torch.equal(bodies[0], bodies[1]), "two launches differ: the unsplit kernel has a fixed summation order"
    return bodies[0].cpu()


def _report(what, got, ref):
    e = rel_err(got.numpy(), ref.numpy())
    print("conv-forms %s err %.3e" % (what, e))
    assert_close(got, ref, TOL, what)


def _pack(w, mode=0):
    from mixgan_tts_amd import ops
    return ops.pack_conv_weight(w.cuda(), mode)


# ---------------------------------------------------------------------------------------------
# mg_conv1d_fwd_ex
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _conv_problem(form, K, stride, dil, Lout, Lextra=0):
    """Inputs and the float64 convolution without bias of one (form, case): shared by the cases that differ only in
    the epilogue.  Lextra lengthens the input so that the natural output is longer than Lout."""
    rows, B, _, _ = FORMS[form]
    Ci = _ci(K)
    pad = dil * (K - 1) // 2
    Lin = (Lout - 1) * stride + 1 + dil * (K - 1) - 2 * pad + (stride - 1) + Lextra     # stride 2: Lin = 2 Lout
    g = _gen(form, K, stride, dil, Lout, Lextra)
    x = torch.randn(B, Ci, Lin, generator=g)
    w = torch.randn(rows, Ci, K, generator=g) * (Ci * K) ** -0.5
    bias = torch.randn(rows, generator=g)
    lin = F.conv1d(x.double(), w.double(), None, stride, pad, dil)[:, :, :Lout]
    assert lin.shape[2] == Lout
    return x, w, bias, lin, pad


def _run_ex(x, packed, rows, Lout, K, stride, pad, dil, bias=None, add=None, in_vec=None, in_slope=1.0, act="none",
            act_slope=0.0, alpha=1.0, prefill=None):
    lib, L = _lib()
    B, Ci, Lin = x.shape
    xd = x.cuda()
    bd = None if bias is None else bias.cuda()
    ad = None if add is None else add.cuda().contiguous()
    vd = None if in_vec is None else in_vec.cuda()

    def launch(out):
        L.check(lib.mg_conv1d_fwd_ex(L.fptr(xd), L.fptr(vd, True), L.fptr(packed), L.fptr(bd, True), L.fptr(ad, True),
                                     L.fptr(out), B, Ci, Lin, rows, Lout, K, stride, pad, dil, float(in_slope), ACTS[act],
                                     float(act_slope), float(alpha), int(prefill is not None), L.stream_ptr()))
    return _twice(launch, B * rows * Lout, prefill).view(B, rows, Lout)


# every instantiated (K, stride, dilation) of the plain/wide set; dilation 3 runs the DILMAX = 5 kernels below their maximum
CASES = [(1, 1, 1), (3, 1, 1), (5, 1, 1), (9, 1, 1), (5, 2, 1), (3, 1, 5), (3, 1, 3), (7, 1, 5), (7, 1, 3), (11, 1, 5),
         (11, 1, 3), (16, 1, 1), (4, 1, 1)]
TAIL40 = [(1, 1, 1), (5, 1, 1), (5, 2, 1), (3, 1, 3), (7, 1, 3), (16, 1, 1)]


def _admitted(K, stride):
    return NO_256 if K == 3 or (K, stride) == (5, 2) else ALL


def _matrix():
    out = []
    for K, stride, dil in CASES:
        for form in _admitted(K, stride):
            out.append(pytest.param(form, K, stride, dil, False, id="%s-k%ds%dd%d" % (_fid(form), K, stride, dil)))
            if FORMS[form][3] and (K, stride, dil) in TAIL40:
                out.append(pytest.param(form, K, stride, dil, True, id="%s-k%ds%dd%d-tail40" % (_fid(form), K, stride, dil)))
    return out


@pytest.mark.parametrize("form,K,stride,dil,tail40", _matrix())
def test_conv1d_ex_form_by_case(form, K, stride, dil, tail40):
    rows, B, L0, L1 = FORMS[form]
    Lout = L1 if tail40 else L0
    _assert_form(form, B, _ci(K), Lout, rows, K, stride, dil)
    x, w, bias, lin, pad = _conv_problem(form, K, stride, dil, Lout)
    got = _run_ex(x, _pack(w), rows, Lout, K, stride, pad, dil, bias=bias)
    _report("ex %s k%d s%d d%d L%d" % (_fid(form), K, stride, dil, Lout), got, lin + bias.double()[None, :, None])


@pytest.mark.parametrize("K,stride,dil", [(3, 1, 1), (3, 1, 3), (3, 1, 5), (5, 2, 1)])
def test_big_slab_cases_do_not_get_256_frame_tiles(K, stride, dil):
    """The shape that selects (1,1,2) gets (1,1,1) where the slab of a 256-frame tile exceeds the staging registers."""
    rows, B, L0, _ = FORMS[(1, 1, 2)]
    _assert_form((1, 1, 1), B, _ci(K), L0, rows, K, stride, dil)


OPTIONS = ["relu", "lrelu", "tanh", "lrelu_s", "alpha", "add", "accumulate", "in_vec", "in_slope", "no_bias", "short_lout",
           "dgrad"]


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("form", ALL, ids=_fid)
def test_conv1d_ex_epilogue_and_staging_options(form, option):
    rows, B, Lout, _ = FORMS[form]
    K, stride, dil = 5, 1, 1
    Ci = _ci(K)
    _assert_form(form, B, Ci, Lout, rows, K, stride, dil)
    x, w, bias, lin, pad = _conv_problem(form, K, stride, dil, Lout, 7 if option == "short_lout" else 0)
    g = _gen(form, option)
    b64 = bias.double()[None, :, None]
    kw = dict(bias=bias)
    packed = None
    if option in ("relu", "lrelu", "tanh", "lrelu_s"):
        kw.update(act=option, act_slope=0.37 if option == "lrelu_s" else 0.0)
        pre = lin + b64
        ref = {"relu": F.relu, "lrelu": lambda t: F.leaky_relu(t, 0.2), "tanh": torch.tanh,
               "lrelu_s": lambda t: F.leaky_relu(t, 0.37)}[option](pre)
    elif option == "alpha":
        kw.update(alpha=-0.75)
        ref = -0.75 * lin + b64
    elif option == "add":
        add = torch.randn(B, rows, Lout, generator=g)
        kw.update(add=add, act="relu")                      # the residual joins after the activation
        ref = F.relu(lin + b64) + add.double()
    elif option == "accumulate":
        base = torch.randn(B, rows, Lout, generator=g)
        kw.update(prefill=base, alpha=0.5)
        ref = base.double() + 0.5 * lin + b64
    elif option == "in_vec":
        vec = torch.randn(B, Ci, generator=g)
        kw.update(in_vec=vec)
        xp = F.pad(x.double() + vec.double()[:, :, None], (pad, pad))      # added to in-range samples only
        ref = F.conv1d(xp, w.double(), bias.double())
    elif option == "in_slope":
        kw.update(in_slope=0.1)
        ref = F.conv1d(F.leaky_relu(x.double(), 0.1), w.double(), bias.double(), stride, pad, dil)
    elif option == "no_bias":
        kw.update(bias=None)
        ref = lin
    elif option == "short_lout":
        assert x.shape[2] == Lout + 7                       # the natural output is 7 frames longer
        ref = lin + b64
    else:   # a data-gradient pack: rows = the source's input channels, taps flipped
        ws = torch.randn(Ci, rows, K, generator=g) * (Ci * K) ** -0.5          # the source weight [Co', Ci', K]
        packed = _pack(ws, 2)
        ref = F.conv1d(x.double(), ws.double().permute(1, 0, 2).flip(2), bias.double(), stride, pad, dil)
    got = _run_ex(x, _pack(w) if packed is None else packed, rows, Lout, K, stride, pad, dil, **kw)
    _report("ex-option %s %s" % (_fid(form), option), got, ref)


# ---------------------------------------------------------------------------------------------
# polyphase transposed convolution: rows = Co * u, K = 3 -- five forms
# ---------------------------------------------------------------------------------------------
def _tpose_rows(form, u):
    if form == (1, 1, 1):
        return 24
    if form[1] == 1:
        return 40
    return 136 if u == 8 else 132       # a multiple of u just over 128


@functools.lru_cache(maxsize=16)      # both transposed-conv tests use each problem
def _tpose_problem(form, u):
    _, B, L, _ = FORMS[form]
    Co = _tpose_rows(form, u) // u
    Ci = _ci(3)
    g = _gen("tpose", form, u)
    x = torch.randn(B, Ci, L, generator=g)
    w = torch.randn(Ci, Co, 2 * u, generator=g) * (Ci * 2) ** -0.5       # two taps reach each output sample
    bias = torch.randn(Co, generator=g)
    ref = 0.5 * F.conv_transpose1d(F.leaky_relu(x.double(), 0.1), w.double(), None, stride=u, padding=u // 2) \
        + bias.double()[None, :, None]
    assert ref.shape == (B, Co, u * L)
    return x, w, bias, ref, Co


def _pack_tpose(w):
    from mixgan_tts_amd import ops
    return ops.pack_conv_transpose_weight(w.cuda())


@pytest.mark.parametrize("u", [2, 4, 8])
@pytest.mark.parametrize("form", NO_256, ids=_fid)
def test_conv_transpose1d(form, u):
    lib, L = _lib()
    _, B, Lin, _ = FORMS[form]
    x, w, bias, ref, Co = _tpose_problem(form, u)
    Ci = x.shape[1]
    _assert_form(form, B, Ci, Lin, Co * u, 3)
    xd, bd, packed = x.cuda(), bias.cuda(), _pack_tpose(w)

    def launch(out):
        L.check(lib.mg_conv_transpose1d_fwd(L.fptr(xd), L.fptr(packed), L.fptr(bd), L.fptr(out), B, Ci, Lin, Co, u, 0.1, 0.5,
                                            L.stream_ptr()))
    got = _twice(launch, B * Co * u * Lin).view(B, Co, u * Lin)
    _report("tpose %s u%d" % (_fid(form), u), got, ref)


@pytest.mark.parametrize("u", [2, 4, 8])
@pytest.mark.parametrize("form", NO_256, ids=_fid)
def test_conv_transpose1d_slice(form, u):
    """The same into channels [0, Co) of a [B, Co + 3, u L] buffer: the other channels keep their sentinel."""
    lib, L = _lib()
    _, B, Lin, _ = FORMS[form]
    x, w, bias, ref, Co = _tpose_problem(form, u)
    Ci = x.shape[1]
    _assert_form(form, B, Ci, Lin, Co * u, 3, epi=SLICE)
    xd, bd, packed = x.cuda(), bias.cuda(), _pack_tpose(w)
    Ctot = Co + 3

    def launch(out):
        L.check(lib.mg_conv_transpose1d_fwd_slice(L.fptr(xd), L.fptr(packed), L.fptr(bd), L.fptr(out), Ctot * u * Lin, B, Ci,
                                                  Lin, Co, u, 0.1, 0.5, L.stream_ptr()))
    got = _twice(launch, B * Ctot * u * Lin).view(B, Ctot, u * Lin)
    assert bool((got[:, Co:] == SENTINEL).all()), "wrote outside the channel slice"
    _report("tpose-slice %s u%d" % (_fid(form), u), got[:, :Co], ref)


def test_transposed_conv_has_no_256_frame_tiles():
    rows, B, L0, _ = FORMS[(1, 1, 2)]
    _assert_form((1, 1, 1), B, _ci(3), L0, 24, 3)
    _assert_form((1, 1, 1), B, _ci(3), L0, 24, 3, epi=SLICE)


# ---------------------------------------------------------------------------------------------
# reflect-padded convolution, input and output as channel slices of wider buffers
# ---------------------------------------------------------------------------------------------
def _reflect_cases():
    out = []
    for K, dil in [(3, 1), (3, 3), (3, 9), (7, 1)]:
        for form in (NO_256 if K == 3 else ALL):
            out.append(pytest.param(form, K, dil, id="%s-k%dd%d" % (_fid(form), K, dil)))
    return out


@pytest.mark.parametrize("form,K,dil", _reflect_cases())
def test_conv1d_reflect(form, K, dil):
    lib, L = _lib()
    rows, B, Lf, _ = FORMS[form]
    Ci = _ci(K)
    _assert_form(form, B, Ci, Lf, rows, K, 1, dil, epi=REFLECT)
    pad = dil * (K - 1) // 2
    g = _gen("reflect", form, K, dil)
    x = torch.randn(B, Ci, Lf, generator=g)
    w = torch.randn(rows, Ci, K, generator=g) * (Ci * K) ** -0.5
    bias = torch.randn(rows, generator=g)
    ref = F.leaky_relu(F.conv1d(F.pad(F.leaky_relu(x.double(), 0.2), (pad, pad), mode="reflect"), w.double(), bias.double(),
                                dilation=dil), 0.3)
    Cin_tot, Cout_tot = Ci + 2, rows + 3
    xw = torch.full((B, Cin_tot, Lf), SENTINEL)           # a sentinel read from the gap would wreck the result
    xw[:, :Ci] = x
    xd, bd, packed = xw.cuda(), bias.cuda(), _pack(w)

    def launch(out):
        L.check(lib.mg_conv1d_reflect_fwd(L.fptr(xd), Cin_tot * Lf, L.fptr(packed), L.fptr(bd), L.fptr(out), Cout_tot * Lf, B,
                                          Ci, Lf, rows, K, dil, 0.2, ACTS["lrelu_s"], 0.3, 1.0, L.stream_ptr()))
    got = _twice(launch, B * Cout_tot * Lf).view(B, Cout_tot, Lf)
    assert bool((got[:, rows:] == SENTINEL).all()), "wrote outside the channel slice"
    _report("reflect %s k%d d%d" % (_fid(form), K, dil), got[:, :rows], ref)


def test_reflect_k3_has_no_256_frame_tiles():
    rows, B, L0, _ = FORMS[(1, 1, 2)]
    for dil in (1, 3, 9):
        _assert_form((1, 1, 1), B, _ci(3), L0, rows, 3, 1, dil, epi=REFLECT)


# ---------------------------------------------------------------------------------------------
# K = 1 with batch strides
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL, ids=_fid)
def test_conv1x1_strided(form):
    lib, L = _lib()
    rows, B, Lf, _ = FORMS[form]
    Ci = _ci(1)
    _assert_form(form, B, Ci, Lf, rows, 1)
    g = _gen("1x1", form)
    x = torch.randn(B, Ci, Lf, generator=g)
    w = torch.randn(rows, Ci, 1, generator=g) * Ci ** -0.5
    bias = torch.randn(rows, generator=g)
    ref = F.conv1d(x.double(), w.double(), bias.double())
    Cin_tot, Cout_tot = Ci + 2, rows + 3
    xw = torch.full((B, Cin_tot, Lf), SENTINEL)
    xw[:, :Ci] = x
    xd, bd, packed = xw.cuda(), bias.cuda(), _pack(w)

    def launch(out):
        L.check(lib.mg_conv1x1_fwd_strided(L.fptr(xd), Cin_tot * Lf, L.fptr(packed), L.fptr(bd), L.fptr(out), Cout_tot * Lf, B,
                                           Ci, Lf, rows, L.stream_ptr()))
    got = _twice(launch, B * Cout_tot * Lf).view(B, Cout_tot, Lf)
    assert bool((got[:, rows:] == SENTINEL).all()), "wrote outside the channel slice"
    _report("1x1-strided %s" % _fid(form), got[:, :rows], ref)
