"""The generic convolution's kernel choice (mg_conv1d_fwd_plan: the function conv_launch itself switches on, csrc/conv_mfma.h),
on the CPU: the (K, stride, DILMAX) case and the workgroup form (MW, WM, NNB) for the shapes the project trains and benchmarks
at, the split reduction, the grid, and the shapes without an instantiation.  tests/test_gpu_conv_forms.py asks the same
query before each of its cases, so its coverage of the six forms cannot drift; this file holds the defaults.

The expected forms are written out from the rule, not computed: with tiles(wm, nnb) = ceil(rows / 64 wm) ceil(L / 64 nnb) B,
  rows <= 32: (1,1,2) when 256-frame tiles number >= 512 and the slab fits the staging registers, else (1,1,1);
  otherwise start at wm = 2 (1 when rows <= 64), nnb = 2; with scratch and tiles < 256 split the reduction
  min(ceil(384 / tiles), chunks / 4, 8) ways when that is >= 2; else halve nnb, then wm, while tiles < 512."""
import ctypes

import pytest

import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib

PLAIN, REFLECT, SLICE, NEEDS_WM2 = (_lib.MG_CONV_EPI_PLAIN, _lib.MG_CONV_EPI_REFLECT, _lib.MG_CONV_EPI_PHASES_SLICE,
                                    _lib.MG_CONV_EPI_NEEDS_WM2)
SCRATCH = 12 << 20      # ops.SPLIT_SCRATCH_FLOATS


def _query(B, Ci, Lout, rows, K, stride=1, dil=1, scratch=0, epi=PLAIN):
    p = _lib.ConvPlan()
    rc = mg.lib().mg_conv1d_fwd_plan(B, Ci, Lout, rows, K, stride, dil, scratch, epi, ctypes.byref(p))
    return rc, p


def _plan(*a, **k):
    rc, p = _query(*a, **k)
    assert rc == 0, rc
    return p


def _form(p):
    return p.mw, p.wm, p.nnb


def _tiles(p, B, Lout, rows):
    return -(-rows // (32 * p.mw * p.wm)) * -(-Lout // (32 * (4 // p.mw) * p.nnb)) * B


# B, Ci, Co, K, stride, dil, L (input frames), scratch -> (kw, stride, ck, dilmax), (mw, wm, nnb), ksplit
WORKLOAD = [
    (16, 256, 1024, 9, 1, 1, 1000, 0, (9, 1, 16, 1), (2, 2, 2), 1),       # FFN conv
    (16, 80, 512, 5, 1, 1, 1000, 0, (5, 1, 16, 1), (2, 2, 2), 1),         # PostNet
    (16, 256, 80, 1, 1, 1, 1000, 0, (1, 1, 32, 1), (2, 1, 1), 1),         # mel_linear: 256 tiles at (2,2,1)
    (16, 64, 128, 5, 2, 1, 1000, 0, (5, 2, 16, 1), (2, 1, 1), 1),         # JCU stride 2: Lout 500
    (1, 32, 1, 7, 1, 1, 256000, 0, (7, 1, 16, 5), (1, 1, 2), 1),          # HiFi-GAN conv_post: 1000 tiles of 256
    (1, 32, 32, 11, 1, 5, 256000, 0, (11, 1, 16, 5), (1, 1, 2), 1),       # HiFi-GAN residual conv
    (16, 128, 1, 3, 1, 1, 250, 0, (3, 1, 32, 1), (1, 1, 1), 1),           # JCU head: K = 3 slab too large for (1,1,2)
    (16, 512, 128, 5, 1, 1, 250, SCRATCH, (5, 1, 16, 1), (2, 2, 2), 8),   # JCU tail: 32 tiles, 32 chunks
    (16, 512, 128, 5, 1, 1, 250, 0, (5, 1, 16, 1), (2, 1, 1), 1),
    (4, 256, 256, 3, 1, 1, 100, SCRATCH, (3, 1, 32, 1), (2, 2, 2), 2),    # 8 tiles, 8 chunks: 2 splits of 4
    (4, 256, 256, 3, 1, 1, 100, 0, (3, 1, 32, 1), (2, 1, 1), 1),
    (16, 256, 512, 3, 1, 1, 1000, 0, (3, 1, 32, 1), (2, 2, 2), 1),        # the denoiser's k = 3 rows
    (1, 512, 256, 3, 1, 3, 8000, 0, (3, 1, 32, 5), (2, 1, 1), 1),         # a dilated vocoder conv: 250 tiles at (2,2,1)
]


@pytest.mark.parametrize("B,Ci,Co,K,stride,dil,L,scratch,case,form,ksplit", WORKLOAD)
def test_default_choice(B, Ci, Co, K, stride, dil, L, scratch, case, form, ksplit):
    Lout = (L - 1) // stride + 1      # padding dil (K - 1) / 2
    p = _plan(B, Ci, Lout, Co, K, stride, dil, scratch)
    assert (p.kw, p.stride, p.ck, p.dilmax) == case
    assert _form(p) == form
    assert p.ksplit == ksplit
    assert p.grid == _tiles(p, B, Lout, Co) * ksplit


def test_grid():
    assert _plan(16, 256, 1000, 1024, 9).grid == 8 * 8 * 16
    assert _plan(1, 32, 256000, 1, 7).grid == 1000
    assert _plan(16, 512, 250, 128, 5, scratch=SCRATCH).grid == 32 * 8
    assert _plan(3, 40, 300, 40, 5).grid == 5 * 3                # (2,1,1): one 64-row tile, 64-frame tiles
    assert _plan(2, 40, 300, 5, 5).grid == 3 * 2                 # (1,1,1): 128-frame tiles


def test_thresholds():
    """Both sides of each count the rule compares with."""
    # rows <= 32: 512 tiles of 256 frames
    assert _form(_plan(2, 40, 65300, 5, 5)) == (1, 1, 2)         # 256 x 2
    assert _form(_plan(2, 40, 65280, 5, 5)) == (1, 1, 1)         # 255 x 2
    assert _form(_plan(2, 40, 65300, 33, 5)) == (2, 1, 2)        # 33 rows: the two-block forms
    # 512 workgroups: nnb, then wm
    assert _form(_plan(16, 24, 4100, 40, 5)) == (2, 1, 2)        # 33 x 16 = 528
    assert _form(_plan(16, 24, 4096, 40, 5)) == (2, 1, 2)        # 32 x 16 = 512: not below
    assert _form(_plan(16, 24, 3968, 40, 5)) == (2, 1, 1)        # 31 x 16 = 496
    assert _form(_plan(16, 24, 2053, 130, 5)) == (2, 2, 2)       # 2 x 17 x 16 = 544
    assert _form(_plan(8, 24, 2053, 130, 5)) == (2, 2, 1)        # 272, then 2 x 33 x 8 = 528
    assert _form(_plan(4, 24, 2053, 130, 5)) == (2, 1, 1)        # 264 at (2,2,1), so wm = 1 too
    assert _form(_plan(16, 24, 4100, 64, 5)) == (2, 1, 2)        # 64 rows: the pack holds two blocks, WM = 1 only
    assert _form(_plan(16, 24, 4100, 65, 5)) == (2, 2, 2)


def test_big_slab_cases_have_no_256_frame_tiles():
    """CK (256 stride + (K - 1) DILMAX) > 8192 floats: K = 3 (CK = 32, either DILMAX) and K = 5 at stride 2; K = 1 fits
    exactly."""
    for K, stride, dil, big in [(1, 1, 1, False), (3, 1, 1, True), (3, 1, 3, True), (5, 1, 1, False), (9, 1, 1, False),
                                (5, 2, 1, True), (7, 1, 1, False), (7, 1, 5, False), (11, 1, 5, False), (16, 1, 1, False),
                                (4, 1, 1, False)]:
        assert _form(_plan(2, 40, 65300, 5, K, stride, dil)) == ((1, 1, 1) if big else (1, 1, 2)), (K, stride, dil)
    assert _form(_plan(2, 40, 65300, 5, 3, 1, 9, epi=REFLECT)) == (1, 1, 1)
    assert _form(_plan(2, 40, 65300, 5, 7, 1, 1, epi=REFLECT)) == (1, 1, 2)
    assert _form(_plan(2, 40, 65300, 24, 3, epi=SLICE)) == (1, 1, 1)


def test_cases_and_dilmax():
    assert (lambda p: (p.kw, p.ck, p.dilmax))(_plan(1, 8, 64, 8, 3, 1, 1)) == (3, 32, 1)      # first match: DILMAX 1
    assert (lambda p: (p.kw, p.ck, p.dilmax))(_plan(1, 8, 64, 8, 3, 1, 2)) == (3, 32, 5)
    assert (lambda p: (p.kw, p.ck, p.dilmax))(_plan(1, 8, 64, 8, 7, 1, 1)) == (7, 16, 5)
    assert (lambda p: (p.kw, p.ck, p.dilmax))(_plan(1, 8, 64, 8, 3, 1, 1, epi=REFLECT)) == (3, 32, 9)
    assert (lambda p: (p.kw, p.ck, p.dilmax))(_plan(1, 8, 64, 8, 7, 1, 1, epi=REFLECT)) == (7, 16, 1)
    assert (lambda p: (p.kw, p.ck, p.dilmax))(_plan(1, 8, 64, 8, 3, 1, 1, epi=SLICE)) == (3, 32, 1)
    for K in (1, 3, 4, 5, 7, 9, 11, 16):
        assert _plan(1, 8, 64, 8, K).ck == (32 if K <= 3 else 16)


def test_split_adjustments():
    # no empty split: 33 chunks 8 ways is 5 per split, which 7 splits cover
    p = _plan(16, 33 * 16, 250, 128, 5, scratch=SCRATCH)
    assert (_form(p), p.ksplit, p.grid) == ((2, 2, 2), 7, 32 * 7)
    # fewer than 4 chunks per split: no split, the unsplit choice
    p = _plan(16, 7 * 16, 250, 128, 5, scratch=SCRATCH)
    assert (_form(p), p.ksplit) == ((2, 1, 1), 1)
    # 256 tiles or more: no split
    p = _plan(16, 512, 2048, 128, 5, scratch=SCRATCH)
    assert (_form(p), p.ksplit) == ((2, 2, 1), 1)
    # the partial tiles (tiles x ksplit x WM NNB 16 x 256 floats) must fit: else the large tile, unsplit
    need = 32 * 8 * 2 * 2 * 16 * 256
    p = _plan(16, 512, 250, 128, 5, scratch=need)
    assert (_form(p), p.ksplit) == ((2, 2, 2), 8)
    p = _plan(16, 512, 250, 128, 5, scratch=need - 1)
    assert (_form(p), p.ksplit, p.grid) == ((2, 2, 2), 1, 32)
    # <= 64 rows split on the (2,1,2) tile; <= 32 rows never split
    p = _plan(2, 128, 1000, 64, 5, scratch=SCRATCH)
    assert (_form(p), p.ksplit) == ((2, 1, 2), 2)
    p = _plan(16, 512, 250, 32, 5, scratch=SCRATCH)
    assert (_form(p), p.ksplit) == ((1, 1, 1), 1)


def test_needs_wm2_never_gets_one_block_per_wave():
    for rows in (8, 32, 33, 64, 65, 128, 512):
        for B, L in ((1, 16), (1, 100), (2, 1000), (16, 1000), (16, 250), (2, 65300)):
            for K in (1, 3, 5, 9):
                for scratch in (0, SCRATCH):
                    p = _plan(B, 256, L, rows, K, scratch=scratch, epi=NEEDS_WM2)
                    assert (p.mw, p.wm) == (2, 2), (rows, B, L, K, scratch)
                    assert p.grid == _tiles(p, B, L, rows) * p.ksplit
    assert _form(_plan(1, 256, 100, 512, 3, epi=NEEDS_WM2)) == (2, 2, 1)
    assert _form(_plan(1, 256, 100, 512, 3)) == (2, 1, 1)


@pytest.mark.parametrize("K,stride,dil,epi", [
    (2, 1, 1, PLAIN), (6, 1, 1, PLAIN), (13, 1, 1, PLAIN), (0, 1, 1, PLAIN),      # K without an instantiation
    (3, 2, 1, PLAIN), (9, 2, 1, PLAIN), (1, 2, 1, PLAIN), (7, 2, 1, PLAIN),       # stride 2 is K = 5 only
    (5, 3, 1, PLAIN), (5, 0, 1, PLAIN),
    (3, 1, 6, PLAIN), (7, 1, 6, PLAIN), (11, 1, 6, PLAIN),                        # dilation <= 5 ...
    (1, 1, 2, PLAIN), (5, 1, 2, PLAIN), (9, 1, 2, PLAIN), (16, 1, 2, PLAIN), (4, 1, 2, PLAIN), (5, 2, 2, PLAIN),  # ... K 3/7/11
    (3, 1, 0, PLAIN),
    (3, 1, 10, REFLECT), (5, 1, 1, REFLECT), (7, 1, 2, REFLECT), (1, 1, 1, REFLECT), (9, 1, 1, REFLECT),
    (1, 1, 1, SLICE), (5, 1, 1, SLICE), (3, 1, 2, SLICE),
    (7, 1, 1, NEEDS_WM2), (3, 1, 2, NEEDS_WM2), (16, 1, 1, NEEDS_WM2),            # the vocoder cases are EpiBiasAct's
])
def test_rejected_shapes(K, stride, dil, epi):
    rc, _ = _query(2, 40, 300, 40, K, stride, dil, 0, epi)
    assert rc == _lib.MG_ERR_SHAPE


def test_argument_checks():
    L = mg.lib()
    p = _lib.ConvPlan()
    assert L.mg_conv1d_fwd_plan(2, 40, 300, 40, 5, 1, 1, 0, PLAIN, None) == _lib.MG_ERR_ARG
    assert L.mg_conv1d_fwd_plan(2, 40, 300, 40, 5, 1, 1, 0, 4, ctypes.byref(p)) == _lib.MG_ERR_ARG
    assert L.mg_conv1d_fwd_plan(2, 40, 300, 40, 5, 1, 1, 0, -1, ctypes.byref(p)) == _lib.MG_ERR_ARG
    for bad in ((0, 40, 300, 40), (2, 0, 300, 40), (2, 40, 0, 40), (2, 40, 300, 0)):
        assert L.mg_conv1d_fwd_plan(*bad, 5, 1, 1, 0, PLAIN, ctypes.byref(p)) == _lib.MG_ERR_SHAPE
