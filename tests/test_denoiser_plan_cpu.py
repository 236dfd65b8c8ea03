"""The denoiser forward's kernel choice (mg_denoiser_fwd_plan: the same function mg_denoiser_fwd / _psample use), on the
CPU: the default form for the shapes that matter and every MG_PERSIST_* / MG_DENOISER_PERSIST pin.  The GPU tests pin each
form and check its numbers; this checks that an unpinned launch gets the form it is meant to get."""
import ctypes

import pytest

import mixgan_tts_amd as mg
from mixgan_tts_amd import _lib
from helpers import DEN_SIZES, DEN_SMALL_SHAPES, DEN_LARGE_SHAPE

CUS = 256
SAVE, SPLIT, P16 = 1, 2, 4
INFER = P16   # inference: the packs carry the 16-row forms
PINS = ("MG_DENOISER_PERSIST", "MG_PERSIST_NT", "MG_PERSIST_SOLO", "MG_PERSIST_TEAM")

PERSIST, PERSIST16, TEAM16 = 0, 1, 2


def _dims(n_layers=20, channels=256, cond_channels=256, mel_bins=80):
    return _lib.DenoiserDims(n_layers, channels, cond_channels, mel_bins, 0)


def _plan(B, L, mode, cproj_mode=0, dims=None, cus=CUS):
    p = _lib.FwdPlan()
    rc = mg.lib().mg_denoiser_fwd_plan(ctypes.byref(dims or _dims()), B, L, mode, cproj_mode, cus, ctypes.byref(p))
    assert rc == 0, rc
    return p


def _form(p):
    """(family, tile width, waves, solo, team), or None for the launch-per-layer path"""
    if p.path == 0:
        assert (p.family, p.nt, p.waves, p.grid, p.block) == (0, 0, 0, 0, 0)
        return None
    assert p.block == 64 * p.waves
    return p.family, p.nt, p.waves, p.solo, p.team


@pytest.fixture(autouse=True)
def _no_pins(monkeypatch):
    for k in PINS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("B,L,mode,form", [
    (16, 1000, INFER, (PERSIST, 64, 4, 1, 0)),
    (16, 1000, SAVE, (PERSIST, 64, 4, 1, 0)),
    (8, 1000, SAVE, (PERSIST, 32, 8, 0, 0)),
    (8, 1000, INFER, (PERSIST, 32, 4, 1, 0)),
    (8, 1000, 0, (PERSIST, 32, 4, 1, 0)),
    (4, 1000, INFER, (PERSIST16, 16, 4, 1, 0)),
    (4, 1000, 0, (PERSIST, 32, 4, 1, 0)),          # no 16-row packs: no 16-frame tiles
    (2, 1000, INFER, (TEAM16, 16, 8, 0, 2)),
    (1, 1000, INFER, (TEAM16, 16, 4, 1, 4)),
    (4, 256, INFER, (TEAM16, 16, 4, 1, 4)),
    (1, 256, INFER, (TEAM16, 16, 4, 1, 4)),
    (2, 2000, INFER, (PERSIST16, 16, 4, 0, 0)),
    (1, 4000, INFER, (PERSIST, 32, 4, 0, 0)),
    (1, 4100, INFER, None),
    (1, 9000, INFER, None),
    (16, 1000, SPLIT, None),
    (16, 1000, SPLIT | P16, None),
])
def test_default_choice(B, L, mode, form):
    assert _form(_plan(B, L, mode)) == form


def test_grid_and_block():
    p = _plan(16, 1000, INFER)
    assert (p.grid, p.block) == (16 * 16, 256)
    p = _plan(8, 1000, SAVE)
    assert (p.grid, p.block) == (8 * 32, 512)
    p = _plan(2, 1000, INFER)
    assert (p.grid, p.block) == (2 * 63 * 2, 512)
    p = _plan(1, 1000, INFER)
    assert (p.grid, p.block) == (63 * 4, 256)


def test_cproj_mode():
    for cpm in (0, 1, 2):
        assert _plan(16, 1000, INFER, cpm).cproj_mode == cpm
        assert _plan(1, 1000, INFER, cpm).cproj_mode == cpm
        assert _plan(16, 1000, SAVE, cpm).cproj_mode == 0       # the saving forward has no loop buffers
        assert _plan(1, 9000, INFER, cpm).cproj_mode == 0       # per layer: the projections come from the GEMM


def test_shape_conditions():
    assert _form(_plan(16, 1000, INFER, dims=_dims(n_layers=2))) is None        # the tag scheme needs >= 3 layers
    assert _form(_plan(16, 1000, INFER, dims=_dims(n_layers=3))) == (PERSIST, 64, 4, 1, 0)
    assert _form(_plan(16, 1000, INFER, dims=_dims(mel_bins=97))) is None
    assert _form(_plan(16, 1000, INFER, dims=_dims(channels=128))) is None
    assert _form(_plan(16, 1000, INFER, dims=_dims(cond_channels=192))) is None


@pytest.mark.parametrize("name", sorted(DEN_SIZES))
def test_other_model_sizes_launch_per_layer(name):
    """The sizes test_gpu_denoiser_dims.py runs (helpers.DEN_SIZES): A to F launch per layer in inference and in save
    mode at every shape of that test, so its default and MG_DENOISER_PERSIST=0 runs are the same code there; G, the
    control, takes the single launch."""
    NL, C, H, M, ms = DEN_SIZES[name]
    dims = _lib.DenoiserDims(NL, C, H, M, ms)
    modes = [0, SAVE] + ([INFER] if C == 256 and H == 256 else [])      # the 16-row packs exist at 256 / 256 only
    for B, L in DEN_SMALL_SHAPES + [DEN_LARGE_SHAPE[1:]]:
        for mode in modes:
            p = _plan(B, L, mode, dims=dims)
            assert p.path == (1 if name == "G" else 0), (name, B, L, mode)
            if p.path == 0:
                assert _form(p) is None


def test_chain_capacity_follows_cus():
    # 32-frame tiles, two per CU: an utterance's chain within half the CUs
    assert _form(_plan(1, 4000, INFER, cus=256)) == (PERSIST, 32, 4, 0, 0)
    assert _form(_plan(1, 4000, INFER, cus=248)) is None
    # teams need tiles x team <= CUs
    assert _form(_plan(1, 1000, INFER, cus=128)) == (TEAM16, 16, 8, 0, 2)


@pytest.mark.parametrize("env,B,L,mode,form", [
    ({"MG_DENOISER_PERSIST": "0"}, 16, 1000, INFER, None),
    ({"MG_DENOISER_PERSIST": "0"}, 1, 1000, INFER, None),
    ({"MG_DENOISER_PERSIST": "1"}, 16, 1000, INFER, (PERSIST, 64, 4, 1, 0)),
    ({"MG_PERSIST_NT": "32"}, 16, 1000, INFER, (PERSIST, 32, 4, 0, 0)),
    ({"MG_PERSIST_NT": "64"}, 8, 1000, INFER, (PERSIST, 64, 4, 1, 0)),
    ({"MG_PERSIST_NT": "64"}, 8, 1000, SAVE, (PERSIST, 64, 4, 1, 0)),
    ({"MG_PERSIST_NT": "328"}, 16, 1000, INFER, (PERSIST, 32, 8, 0, 0)),
    ({"MG_PERSIST_NT": "328"}, 16, 1000, SAVE, (PERSIST, 32, 8, 0, 0)),
    ({"MG_PERSIST_NT": "864"}, 16, 1000, INFER, (PERSIST, 64, 8, 0, 0)),
    ({"MG_PERSIST_NT": "864"}, 1, 1000, INFER, (PERSIST, 64, 8, 0, 0)),
    ({"MG_PERSIST_NT": "16"}, 16, 1000, INFER, (PERSIST16, 16, 4, 0, 0)),
    ({"MG_PERSIST_NT": "16"}, 16, 1000, 0, (PERSIST, 64, 4, 1, 0)),          # 16 needs the 16-row packs ...
    ({"MG_PERSIST_NT": "16"}, 8, 1000, SAVE, (PERSIST, 32, 8, 0, 0)),        # ... and no save
    ({"MG_PERSIST_NT": "16"}, 1, 4000, INFER, (PERSIST, 32, 4, 0, 0)),       # > 128 tiles of 16: 32 after the pin
    ({"MG_PERSIST_NT": "7"}, 16, 1000, INFER, (PERSIST, 64, 4, 1, 0)),       # not a width: ignored
    ({"MG_PERSIST_SOLO": "0"}, 8, 1000, INFER, (PERSIST, 32, 4, 0, 0)),
    ({"MG_PERSIST_SOLO": "0"}, 4, 1000, INFER, (PERSIST16, 16, 4, 0, 0)),
    ({"MG_PERSIST_SOLO": "1"}, 8, 1000, INFER, (PERSIST, 32, 4, 1, 0)),
    ({"MG_PERSIST_TEAM": "0"}, 1, 1000, INFER, (PERSIST16, 16, 4, 1, 0)),
    ({"MG_PERSIST_TEAM": "0", "MG_PERSIST_SOLO": "0"}, 1, 1000, INFER, (PERSIST16, 16, 4, 0, 0)),
    ({"MG_PERSIST_TEAM": "2"}, 1, 1000, INFER, (TEAM16, 16, 8, 0, 2)),
    ({"MG_PERSIST_TEAM": "4"}, 1, 1000, INFER, (TEAM16, 16, 4, 1, 4)),
    ({"MG_PERSIST_TEAM": "4"}, 2, 1000, INFER, (PERSIST16, 16, 4, 1, 0)),    # a team of 4 does not fit; 2 is excluded
])
def test_pins(monkeypatch, env, B, L, mode, form):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _form(_plan(B, L, mode)) == form


def test_argument_checks():
    L = mg.lib()
    p = _lib.FwdPlan()
    d = _dims()
    assert L.mg_denoiser_fwd_plan(ctypes.byref(d), 1, 100, 0, 0, CUS, None) == -1
    assert L.mg_denoiser_fwd_plan(ctypes.byref(d), 1, 100, SAVE | SPLIT, 0, CUS, ctypes.byref(p)) == -1
    assert L.mg_denoiser_fwd_plan(ctypes.byref(d), 1, 100, 0, 3, CUS, ctypes.byref(p)) == -1
    assert L.mg_denoiser_fwd_plan(ctypes.byref(d), 0, 100, 0, 0, CUS, ctypes.byref(p)) == -2
    assert L.mg_denoiser_fwd_plan(ctypes.byref(d), 1, 0, 0, 0, CUS, ctypes.byref(p)) == -2
    assert L.mg_denoiser_fwd_plan(None, 1, 100, 0, 0, CUS, ctypes.byref(p)) == -1
