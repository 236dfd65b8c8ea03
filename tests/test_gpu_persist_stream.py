"""The 64-frame, four-wave single-launch denoiser (csrc/denoiser_persist.h) at the edge shapes of its tiling.  Its k
loops address the weight streams as scalar base + lane offset + immediate; the order of every floating-point operation
is the other forms'.

What each comparison can catch: the eight-wave and the 32-frame form run the same k loops with the same addressing, so
the bitwise comparisons with them guard what differs between the forms -- the tiling, the row blocks a wave owns, the
halo hand-off, the masks and the dealing of the output projection's tasks -- not an addressing error
common to all forms.  That one is caught by the comparison with the launch-per-layer kernels (other kernels, other
weight packs) within the suite's tolerance.

Shapes: B = 2, L = 136 with 64-frame tiles pinned = a left, an interior and a right tile per utterance, the last with 8
live frames (both halo sides, the f < L masks, a nearly empty column block); B = 1, L = 64 = one tile without a
neighbour.  The model's own 20 layers, the seeded fixture weights."""
import pytest
import torch

from helpers import golden, hot_path_configs, write_stats, load_seeded, assert_close, pin_width

pytestmark = pytest.mark.gpu
TOL = 2e-5                      # the suite's parity tolerance (test_gpu_persist.py, test_gpu_cond_project.py)
SHAPES = [(2, 136), (1, 64)]
FORMS = (64, 864, 32)           # four waves x 64 frames (the form under test), eight waves x 64 frames, 32 frames


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd as m
    assert torch.cuda.is_available()
    return m


@pytest.fixture(scope="module")
def models(mg, manifest, tmp_path_factory):
    """One seeded GaussianDiffusion per form (each keeps its own workspaces) and one for the launch-per-layer kernels."""
    e = golden("elementwise")
    stats = write_stats(tmp_path_factory.mktemp("stats"), e["spec_min"], e["spec_max"])
    out = {}
    for key in FORMS + ("layers",):
        gd = mg.GaussianDiffusion(*hot_path_configs("naive", 4, stats_dir=stats))
        load_seeded(gd, manifest, "diffusion_naive_ms0", 31)
        _live_output(gd.denoise_fn)
        out[key] = gd.cuda().eval()
    return out


def _live_output(den, seed=3):
    """Denoiser.__init__ zeroes output_projection's weight and the fixture recipe leaves it so: with it the output would
    be the bias broadcast over the frames whatever the layers and the projection compute.  Seeded weight and bias."""
    gen = torch.Generator().manual_seed(seed)
    conv = den.output_projection.conv
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * 0.05)
        conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen) * 0.1)


def _inputs(B, L, M=80):
    gen = torch.Generator().manual_seed(1000 * B + L)
    x, cond, nz = (torch.randn(B, c, L, generator=gen).cuda() for c in (M, 256, M))
    return x, cond, nz


def _on(monkeypatch, models, key, fn):
    """fn(model) on the form `key` (or the launch-per-layer kernels); a hand-off timeout raises"""
    if key == "layers":
        monkeypatch.setenv("MG_DENOISER_PERSIST", "0")
    else:
        monkeypatch.delenv("MG_DENOISER_PERSIST", raising=False)
        pin_width(monkeypatch, key)
    with torch.no_grad():
        r = fn(models[key])
    models[key].denoise_fn.check(sync=True)
    monkeypatch.delenv("MG_DENOISER_PERSIST", raising=False)
    return r


@pytest.mark.parametrize("B,L", SHAPES)
def test_forward_is_bitwise_the_other_forms(models, monkeypatch, B, L):
    x, cond, _ = _inputs(B, L)
    t = torch.tensor([7, 900][:B]).cuda()
    outs = {k: _on(monkeypatch, models, k, lambda gd: gd.denoise_fn(x[:, None], t, cond, None).clone())
            for k in FORMS + ("layers",)}
    assert torch.isfinite(outs[64]).all()
    for k in FORMS[1:]:
        assert torch.equal(outs[64], outs[k]), "form %d: %g" % (k, (outs[64] - outs[k]).abs().max().item())
    assert_close(outs[64].cpu(), outs["layers"].cpu(), TOL, "vs the launch-per-layer kernels B=%d L=%d" % (B, L))


@pytest.mark.parametrize("tval", [0, 2])            # t = 0: the posterior mean alone; t > 0: + sigma * noise
@pytest.mark.parametrize("B,L", SHAPES)
def test_p_sample_is_bitwise_the_other_forms(models, monkeypatch, B, L, tval):
    x, cond, nz = _inputs(B, L)
    t = torch.full((B,), tval).cuda()
    outs = {k: _on(monkeypatch, models, k, lambda gd: gd._p_sample_bml(x, t, cond, None, nz).clone())
            for k in FORMS + ("layers",)}
    assert torch.isfinite(outs[64]).all()
    for k in FORMS[1:]:
        assert torch.equal(outs[64], outs[k]), "form %d: %g" % (k, (outs[64] - outs[k]).abs().max().item())
    assert_close(outs[64].cpu(), outs["layers"].cpu(), TOL, "vs the launch-per-layer kernels B=%d L=%d t=%d" % (B, L, tval))


@pytest.mark.parametrize("B,L", SHAPES)
def test_writing_step_and_two_reading_steps_equal_three_plain_steps(models, monkeypatch, B, L):
    """The property of test_gpu_cond_project.py at these shapes: a step that leaves its conditioner projections behind and
    two steps that read them, against three steps that project for themselves, each step fed the one before."""
    x, cond, _ = _inputs(B, L)
    gen = torch.Generator().manual_seed(77)
    draws = [torch.randn(B, 80, L, generator=gen).cuda() for _ in range(3)]

    def loop(gd, hoist):
        left = torch.full((B, 20 * 256, L), float("nan"), device="cuda")
        cur, trace = x, []
        for k, tv in enumerate((3, 2, 1)):
            t = torch.full((B,), tv).cuda()
            kw = {} if not hoist else {"cproj_out": left} if k == 0 else {"cproj": left}
            cur = gd._p_sample_bml(cur, t, cond, None, draws[k], **kw).clone()
            trace.append(cur)
        return trace

    plain = _on(monkeypatch, models, 64, lambda gd: loop(gd, False))
    hoisted = _on(monkeypatch, models, 64, lambda gd: loop(gd, True))
    for k, (a, b) in enumerate(zip(plain, hoisted)):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), "step %d: %g" % (k, (a - b).abs().max().item())


@pytest.mark.parametrize("M", [80, 75])             # 75: the output projection's last 32-row block has 11 live rows
def test_forward_with_a_ragged_last_row_block(mg, monkeypatch, tmp_path, M):
    """Mel bins that do not fill the output projection's last row block.  No seeded fixture has M != 80: the module's own
    initialisation under a fixed seed, with a live output projection."""
    B, L = 2, 136
    pre, mc = hot_path_configs(stats_dir=str(tmp_path))[1:3]
    pre["preprocessing"]["mel"]["n_mel_channels"] = M
    torch.manual_seed(5)
    den = mg.Denoiser(pre, mc)
    _live_output(den)
    den = den.cuda().eval()
    x, cond, _ = _inputs(B, L, M)
    t = torch.tensor([7, 900]).cuda()
    outs = {}
    for k in FORMS + ("layers",):
        if k == "layers":
            monkeypatch.setenv("MG_DENOISER_PERSIST", "0")
        else:
            pin_width(monkeypatch, k)
        den._ws.clear()                             # a workspace per form
        with torch.no_grad():
            outs[k] = den(x[:, None], t, cond, None).clone()
        den.check(sync=True)
    assert outs[64].shape == (B, 1, M, L) and torch.isfinite(outs[64]).all()
    assert outs[64].std(dim=-1).min().item() > 1e-3, "every mel row varies over the frames: the projection is live"
    for k in FORMS[1:]:
        assert torch.equal(outs[64], outs[k]), "form %d: %g" % (k, (outs[64] - outs[k]).abs().max().item())
    assert_close(outs[64].cpu(), outs["layers"].cpu(), TOL, "vs the launch-per-layer kernels M=%d" % M)
