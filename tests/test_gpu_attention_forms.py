"""Every form of the decoder's streaming-softmax attention (csrc/attention.hip) directly against float64, at the project's
bars.

fp32: the four forms (plain 128-query, 64-query key split, 128-query key split, 256-query) x the two staging paths
(16-byte loads at L % 4 == 0, scalar otherwise); fp16 operands: the two forms x the two staging paths.  Each case pins its
form with MG_ATTENTION_KSPLIT / MG_ATTENTION_WIDE and first asserts, through mg_attention_form -- the function the
launchers switch on -- that it is the form the case was written for.  Lengths sit on the key-tile edges (63, 64, 65), on
the form's own query-tile edges, below one vector (1, 3) and at several tiles with a remainder (700); B = 2 and three heads,
so a wrong head or batch stride shows.  Inputs and masks: tests/attention_ref.py.

fp32 outputs are held to BAR_RED under the fallback rule, on the whole tensor and on every 64-frame block against that
block's own maximum.  The fp16-operand outputs are held to 8 x the error of a CPU emulation of the kernel's arithmetic
against the rounded-operand float64 reference (measured per case, never taken from the kernel); their distance from
true float64 is printed, and asserted only for unit-variance inputs: with a peaked softmax the rounding of the operands
alone is several 1e-3 of the tensor maximum, whatever the kernel does.

Measured on an MI355X: with unit-variance inputs the kernel is within 1.1 x the emulation (and equal to the
running-maximum emulation to three digits at L = 700); with the two other input sets a handful of query rows reach
6.7 x (wide, L = 256, late maximum) and 5.0 x (L = 33, peaked).  Those rows are a property of the compiled rounding of q,
not of the softmax: for 16 of a lane's 64 q elements the compiler folds `q * (scale * log2 e)` and the conversion to
fp16 into one v_fma_mixlo_f16 (one rounding), for the other 48 it multiplies in float32 and converts (two, as the source
states and as the reference above does).  About 1e-4 of the products round differently the two ways, by one fp16 unit of
q, which moves every score of that query by up to 2^-10 |k| -- visible only where |k| is large.  Against the reference
with every q rounded once (printed beside each case) the two worst rows drop to 1.0 x and others rise, as a mixture
must.  The asserted reference stays the two-rounding one: it is what the source states and what the issue set."""
import ctypes

import pytest
import torch

import attention_ref as AR
from helpers import rel_err
from small_ops_ref import BAR_RED, check, check_equal, tile_errors

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -7.25

# form -> (MG_ATTENTION_KSPLIT, MG_ATTENTION_WIDE, the form's own query-tile edges)
FP32_FORMS = {"plain128": ("0", "0", (127, 128, 129)), "ksplit64": ("1", "0", ()),
              "ksplit128": ("2", "0", (127, 128, 129)), "wide256": ("0", "1", (255, 256, 257))}
F16_FORMS = {"plain128": ("0", "0", (127, 128, 129)), "wide256": ("0", "1", (255, 256, 257))}


def _cases(forms):
    return [pytest.param(f, L, id="%s-L%d" % (f, L)) for f, (_, _, edges) in forms.items()
            for L in sorted(AR.COMMON_L + edges)]


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd as m
    return m


def _pin(mg, monkeypatch, forms, form, L, f16):
    ks, wide, _ = forms[form]
    monkeypatch.setenv("MG_ATTENTION_KSPLIT", ks)
    monkeypatch.setenv("MG_ATTENTION_WIDE", wide)
    want = {"plain128": mg._lib.MG_ATTN_PLAIN128, "ksplit64": mg._lib.MG_ATTN_KSPLIT64,
            "ksplit128": mg._lib.MG_ATTN_KSPLIT128, "wide256": mg._lib.MG_ATTN_WIDE256}[form]
    assert mg.lib().mg_attention_form(AR.B, L, AR.N_HEAD, int(f16)) == want, (form, L)


def offset_view(t):
    """t's values as a contiguous GPU tensor one float into a larger buffer: never 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _guarded(mg, qkv, pad, precision):
    """The entry point on an output buffer with GUARD sentinel floats on each side -> (out, the two guards)."""
    Bn, C3, L = qkv.shape
    n = Bn * (C3 // 3) * L
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    out = buf[GUARD:GUARD + n].view(Bn, C3 // 3, L)
    fn = mg.lib().mg_attention_fwd if precision == "fp32" else mg.lib().mg_attention_fwd_f16
    mg._lib.check(fn(mg._lib.fptr(qkv), ctypes.c_void_p(0 if pad is None else pad.data_ptr()), mg._lib.fptr(out), Bn, L,
                     AR.N_HEAD, AR.D_HEAD, float(AR.D_HEAD) ** -0.5, mg._lib.stream_ptr()))
    torch.cuda.synchronize()
    return out, buf[:GUARD], buf[GUARD + n:]


def _run(mg, L, inputs, mask, precision, what):
    """The kernel on case (L, inputs, mask): the result, after asserting that a second run on a guarded buffer and a
    run from a qkv that is one float off 16-byte alignment (scalar staging at every L) give the same bits and that the
    guards are untouched."""
    qkv, pad = AR.case(L, inputs, mask)
    dq, dp = qkv.cuda(), None if pad is None else pad.cuda()
    assert dq.data_ptr() % 16 == 0
    out = mg.ops.attention(dq, dp, AR.N_HEAD, AR.D_HEAD, precision)
    torch.cuda.synchronize()
    again, lo, hi = _guarded(mg, dq, dp, precision)
    assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), what + ": wrote outside out"
    ref = out.cpu()
    check_equal(again, ref, what + " run 2")
    check_equal(mg.ops.attention(offset_view(dq), dp, AR.N_HEAD, AR.D_HEAD, precision), ref, what + " unaligned qkv")
    return out


@pytest.mark.parametrize("form,L", _cases(FP32_FORMS))
def test_attention_fp32_form(mg, monkeypatch, form, L):
    _pin(mg, monkeypatch, FP32_FORMS, form, L, False)
    for inputs in AR.INPUTS:
        for mask in AR.MASKS:
            what = "%s L=%d %s/%s" % (form, L, inputs, mask)
            out = _run(mg, L, inputs, mask, "fp32", what)
            ref32, ref64 = AR.refs(L, inputs, mask)
            check(out, ref32, ref64, BAR_RED, what, dim=2, block=64, group="attention fp32 " + form)


def _f16_errors(got, ref, L):
    """(whole-tensor error, worst 64-frame block error) relative to the reference maxima."""
    d, r = tile_errors(got, ref, 2, 64)
    return rel_err(got.double().numpy(), ref.numpy()), float((d / (r + 1e-30)).max())


F16_WORST = {}      # form -> per input set the worst (kernel vs rounded ref, emulation vs rounded ref, kernel vs float64)


@pytest.mark.parametrize("form,L", _cases(F16_FORMS))
def test_attention_f16_form(mg, monkeypatch, form, L):
    _pin(mg, monkeypatch, F16_FORMS, form, L, True)
    for inputs in AR.INPUTS:
        for mask in AR.MASKS:
            what = "f16 %s L=%d %s/%s" % (form, L, inputs, mask)
            out = _run(mg, L, inputs, mask, "f16", what).cpu()
            assert bool(torch.isfinite(out).all()), what
            ref16, emu, emu_run, ref16_fused = AR.refs_f16(L, inputs, mask)
            _, ref64 = AR.refs(L, inputs, mask)
            e, et = _f16_errors(out, ref16, L)
            ee, eet = _f16_errors(emu, ref16, L)
            er, ert = _f16_errors(emu_run, ref16, L)
            ef, _ = _f16_errors(out, ref16_fused, L)
            e64 = rel_err(out.double().numpy(), ref64.numpy())
            r64 = rel_err(ref16.numpy(), ref64.numpy())
            print("%-44s kernel %.2e (block %.2e)  emulation %.2e (block %.2e)  with running max %.2e (block %.2e)  "
                  "| kernel vs q rounded once %.2e | vs float64: kernel %.2e, rounded operands alone %.2e"
                  % (what, e, et, ee, eet, er, ert, ef, e64, r64))
            w = F16_WORST.setdefault((form, inputs), [0.0, 0.0, 0.0])
            w[:] = [max(w[0], e), max(w[1], ee), max(w[2], e64)]
            assert e <= 8 * ee, "%s: %.3e against the rounded-operand reference > 8 x the emulation's %.3e" % (what, e, ee)
            assert et <= 8 * eet, "%s: worst 64-frame block %.3e > 8 x the emulation's %.3e" % (what, et, eet)
            if inputs == "unit":
                assert e64 <= 2 * r64, "%s: %.3e from float64, the rounded operands alone %.3e" % (what, e64, r64)
