"""mg_denoiser_pack's host half, on the CPU: what it accepts must be what den_check / mg_denoiser_packed_floats promised.

The pack runs from a job table of 768 entries in the packed blob's tail.  A model has 9 + 7 jobs per layer (8 with a
speaker projection), 3 + 3 per layer more for the backward packs and 3 + 5 per layer more for the 16-row packs, so one
table overflows above 108 layers for the plain inference packs, above 75 / 68 (single / multi-speaker) for the training
packs and above 63 / 58 for the 256/256 inference packs -- while the library accepts up to 256 layers and
mg_denoiser_packed_floats sizes a blob for them.  The pack used to answer MG_ERR_ARG there; it now runs the list 768
jobs at a time.

Nothing here touches a device: mg_denoiser_pack_plan is mg_denoiser_pack's own code up to its first upload (every
check, the whole job list) and stops there, and the calls of mg_denoiser_pack itself are restricted to refusals that
return before any device call -- which is what the second half of this file asserts about them: the weight pointers
are dummies, so a refusal that came after a launch would not be survivable on a machine that has a GPU."""
import ctypes

import pytest

import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib
from helpers import den_size_configs

BWD, SPLIT, P16, RESIDENT = _lib.MG_DEN_BACKWARD, _lib.MG_DEN_SPLIT, _lib.MG_DEN_P16, _lib.MG_DEN_JOBS_RESIDENT
TABLE = 768
# both sides of every overflow point of one table, and the largest model den_check admits
LAYERS = [58, 59, 63, 64, 68, 69, 75, 76, 108, 109, 256]
FLAG_SETS = [0, BWD, P16, BWD | P16, SPLIT, SPLIT | P16, BWD | SPLIT, RESIDENT, BWD | RESIDENT]

_DUMMY = (ctypes.c_float * 16)()      # every pointer names this; nothing may read through one


def _table(NL, ms, missing=()):
    n = _lib.MG_DEN_HEAD_PTRS + _lib.MG_DEN_LAYER_PTRS * NL
    p = ctypes.addressof(_DUMMY)
    t = (ctypes.c_void_p * n)(*[p] * n)
    for l in range(NL):
        base = _lib.MG_DEN_HEAD_PTRS + _lib.MG_DEN_LAYER_PTRS * l
        t[base + _lib.MG_DEN_L_RESERVED] = None
        if not ms:
            t[base + _lib.MG_DEN_L_SPK_W] = None
    for i in missing:
        t[i] = None
    return t


def _expected_jobs(NL, ms, flags):
    n = 9 + (8 if ms else 7) * NL
    if flags & BWD:
        n += 3 + 3 * NL
    if flags & P16:
        n += 3 + 5 * NL
    return n


def _plan(dims, flags, table=None):
    L = mg.lib()
    jobs, launches = ctypes.c_int(-1), ctypes.c_int(-1)
    dummy = ctypes.cast(_DUMMY, ctypes.c_void_p)
    rc = L.mg_denoiser_pack_plan(ctypes.byref(dims), table if table is not None else _table(dims.n_layers, dims.multi_speaker),
                                 dummy, dummy, flags, ctypes.byref(jobs), ctypes.byref(launches))
    return rc, jobs.value, launches.value


@pytest.mark.parametrize("C,H,M", [(64, 32, 8), (256, 256, 80)])
@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("NL", LAYERS)
def test_pack_accepts_what_the_size_query_promised(NL, ms, C, H, M):
    L = mg.lib()
    dims = _lib.DenoiserDims(NL, C, H, M, ms)
    for flags in FLAG_SETS:
        promised = L.mg_denoiser_packed_floats(ctypes.byref(dims), flags & ~RESIDENT)
        rc, jobs, launches = _plan(dims, flags)
        small_only = bool(flags & (SPLIT | P16)) and (C, H) != (256, 256)
        assert (promised == 0) == small_only, (flags, promised)
        if promised == 0:
            assert (rc, jobs, launches) == (_lib.MG_ERR_SHAPE, 0, 0), (flags, rc)
            continue
        assert rc == _lib.MG_OK, "NL=%d ms=%d flags=%d: packed_floats promised %d floats, the pack answers %d" % (
            NL, ms, flags, promised, rc)
        assert jobs == _expected_jobs(NL, ms, flags), (flags, jobs)
        assert launches == -(-jobs // TABLE), (flags, jobs, launches)


def test_overflow_points_are_where_the_issue_counted_them():
    """The last NL of one launch and the first of two, per pack kind: the cases above straddle each."""
    for C, ms, flags, last in [(64, 0, 0, 108), (64, 0, BWD, 75), (64, 1, BWD, 68), (256, 0, P16, 63), (256, 1, P16, 58)]:
        H = 32 if C == 64 else 256
        for NL, want in ((last, 1), (last + 1, 2)):
            rc, _, launches = _plan(_lib.DenoiserDims(NL, C, H, 8, ms), flags)
            assert (rc, launches) == (_lib.MG_OK, want), (C, ms, flags, NL, rc, launches)
    rc, jobs, launches = _plan(_lib.DenoiserDims(256, 256, 256, 80, 1), P16)
    assert (rc, jobs, launches) == (_lib.MG_OK, 9 + 8 * 256 + 3 + 5 * 256, 5)
    assert _plan(_lib.DenoiserDims(20, 256, 256, 80, 1), BWD)[1:] == (9 + 8 * 20 + 3 + 3 * 20, 1)      # the model as shipped


def test_plan_refuses_what_den_check_refuses():
    L = mg.lib()
    for dims in (_lib.DenoiserDims(257, 64, 32, 8, 0), _lib.DenoiserDims(0, 64, 32, 8, 0), _lib.DenoiserDims(3, 96, 32, 8, 0),
                 _lib.DenoiserDims(3, 64, 48, 8, 0), _lib.DenoiserDims(3, 64, 32, 0, 0)):
        assert L.mg_denoiser_packed_floats(ctypes.byref(dims), 0) == 0
        assert _plan(dims, 0, _table(max(1, min(dims.n_layers, 257)), 0))[0] == _lib.MG_ERR_SHAPE


# ------------------------------------------------------------------------------------------ refusals of the real call
# mg_denoiser_pack itself, with the same dummy pointers: every case below must return before it queues, uploads or
# launches anything, and the plan must name the same code.
def _pack(dims, flags, table):
    dummy = ctypes.cast(_DUMMY, ctypes.c_void_p)
    return mg.lib().mg_denoiser_pack(ctypes.byref(dims), table, dummy, dummy, flags, None)


@pytest.mark.parametrize("flags", [SPLIT, P16, SPLIT | P16, BWD | SPLIT])
@pytest.mark.parametrize("C,H", [(64, 32), (128, 256), (256, 384), (384, 256)])
def test_split_and_p16_are_refused_before_anything_runs(C, H, flags):
    """The 256/256-only packs at another size: MG_ERR_SHAPE from the top of the function (they used to be refused after
    the job pushes, MG_DEN_SPLIT after the table launch too, in a blob mg_denoiser_packed_floats had sized as 0)."""
    dims = _lib.DenoiserDims(3, C, H, 20, 0)
    assert mg.lib().mg_denoiser_packed_floats(ctypes.byref(dims), flags) == 0
    t = _table(3, 0)
    assert _plan(dims, flags, t)[0] == _lib.MG_ERR_SHAPE
    assert _pack(dims, flags, t) == _lib.MG_ERR_SHAPE


def test_a_missing_weight_is_refused_before_anything_runs():
    """A NULL weight of the LAST layer of a model that packs in several launches (9 + 7 * 200 jobs): MG_ERR_ARG before
    the first chunk goes out, also for the speaker projection of a multi-speaker model."""
    NL = 200
    last = _lib.MG_DEN_HEAD_PTRS + _lib.MG_DEN_LAYER_PTRS * (NL - 1)
    for ms, slot in ((0, _lib.MG_DEN_L_OUT_B), (0, _lib.MG_DEN_L_CONV_W), (1, _lib.MG_DEN_L_SPK_W)):
        dims = _lib.DenoiserDims(NL, 64, 32, 8, ms)
        assert _plan(dims, 0)[0] == _lib.MG_OK
        t = _table(NL, ms, missing=(last + slot,))
        assert _plan(dims, 0, t)[0] == _lib.MG_ERR_ARG
        assert _pack(dims, 0, t) == _lib.MG_ERR_ARG
    dims = _lib.DenoiserDims(3, 64, 32, 8, 0)
    assert _pack(dims, 0, _table(3, 0, missing=(_lib.MG_DEN_OUT_B,))) == _lib.MG_ERR_ARG
    assert _pack(dims, 0, None) == _lib.MG_ERR_ARG


@pytest.mark.parametrize("name", ["A", "B", "C", "F"])
def test_bf16x3_names_its_reason_at_other_sizes(name):
    """Denoiser.packed_weights refuses precision = "bf16x3" for a model that is not 256 / 256 by name, before it looks
    at the device (the parameters are on the CPU here) and before the library is asked for a size."""
    den = mg.Denoiser(*den_size_configs(name))
    den.precision = "bf16x3"
    with pytest.raises(mg.MixganHipError, match=r"bf16x3.*channels = cond channels = 256"):
        den.packed_weights()
    with pytest.raises(mg.MixganHipError, match=r"bf16x3"):
        den.packed_weights(with_backward=True)
    den.precision = "fp32"
    with pytest.raises(mg.MixganHipError, match="needs them on the GPU"):
        den.packed_weights()      # the next refusal in line: CPU parameters
