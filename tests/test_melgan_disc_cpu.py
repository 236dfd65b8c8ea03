"""MelGAN discriminator, the parts that need no GPU: the float64 restatement the GPU tests compare against
(tests/melgan_disc_ref.py) is pinned to the same network built from torch's own modules, the product classes carry the
torch construction's state-dict keys, unsupported constructor arguments raise, and the library exports the new entry
points."""
import ctypes

import pytest
import torch

import melgan_disc_ref as DR


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


@pytest.mark.parametrize("num_D,n_layers,T", [(3, 4, 2083), (2, 5, 700), (1, 4, 8)])
def test_restatement_equals_the_torch_modules(num_D, n_layers, T):
    torch.manual_seed(3)
    net = DR.TorchDiscriminator(num_D, n_layers=n_layers).double()
    W = DR.disc_init(5, num_D, n_layers)
    assert list(net.state_dict().keys()) == list(W.keys())
    net.load_state_dict({k: v.double() for k, v in W.items()}, strict=True)
    x = torch.randn(2, 1, T, dtype=torch.float64, generator=torch.Generator().manual_seed(T))
    with torch.no_grad():
        want = net(x)
        got = DR.disc_forward({k: v.double() for k, v in W.items()}, x, num_D, n_layers)
    assert len(got) == num_D
    for i, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b) == n_layers + 3
        for j, (u, v) in enumerate(zip(a, b)):
            assert u.shape == v.shape, (i, j)
            assert float((u - v).abs().max()) <= 1e-10 * max(1.0, float(v.abs().max())), (i, j)


def test_restated_losses():
    gen = torch.Generator().manual_seed(9)
    D_real = [[torch.randn(2, 3, 5, generator=gen, dtype=torch.float64) for _ in range(7)] for _ in range(3)]
    D_fake = [[torch.randn(2, 3, 5, generator=gen, dtype=torch.float64) for _ in range(7)] for _ in range(3)]
    d = sum(torch.clamp(1 - r[-1], min=0).mean() + torch.clamp(1 + f[-1], min=0).mean() for r, f in zip(D_real, D_fake))
    assert float((DR.discriminator_loss(D_real, D_fake) - d).abs()) <= 1e-14
    assert float((DR.generator_loss(D_fake) + sum(f[-1].mean() for f in D_fake)).abs()) <= 1e-14
    fm = sum((1 / 3) * (4 / 5) * torch.nn.functional.l1_loss(f[j], r[j]) for r, f in zip(D_real, D_fake) for j in range(6))
    assert float((DR.feature_loss(D_real, D_fake) - fm).abs()) <= 1e-14


@pytest.mark.parametrize("num_D,n_layers", [(3, 4), (1, 5)])
def test_state_dict_loads_strictly_both_ways(mg, num_D, n_layers):
    torch.manual_seed(4)
    ref = DR.TorchDiscriminator(num_D, n_layers=n_layers)
    net = mg.melgan_discriminators.Discriminator(num_D, n_layers=n_layers)
    a, b = ref.state_dict(), net.state_dict()
    assert list(a.keys()) == list(b.keys())
    assert "model.disc_0.model.layer_0.1.weight_g" in b and "model.disc_0.model.layer_1.0.weight_v" in b
    assert "model.disc_0.model.layer_%d.bias" % (n_layers + 2) in b
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
    net.load_state_dict(a, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, a[k]), k
    fresh = mg.melgan_discriminators.Discriminator(num_D, n_layers=n_layers)
    ref.load_state_dict(fresh.state_dict(), strict=True)
    # initialised as Conv1d + weight_norm: g = |v| per output row
    for k, v in fresh.state_dict().items():
        if k.endswith("weight_g"):
            assert torch.equal(v, fresh.state_dict()[k[:-1] + "v"].flatten(1).norm(dim=1).view(-1, 1, 1)), k


def test_upstream_weights_init_changes_no_parameter():
    """Upstream's weights_init draws N(0, 0.02) into `m.weight` of every Conv module.  Under weight_norm that attribute is
    derived: parameters keep their bits and the next forward is unchanged."""
    torch.manual_seed(6)
    net = DR.TorchDiscriminator(2).double()
    x = torch.randn(1, 1, 300, dtype=torch.float64)
    with torch.no_grad():
        before_out = [m.clone() for maps in net(x) for m in maps]
    before = {k: v.clone() for k, v in net.state_dict().items()}

    def weights_init(m):
        if m.__class__.__name__.find("Conv") != -1:
            m.weight.data.normal_(0.0, 0.02)

    net.apply(weights_init)
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k
    with torch.no_grad():
        after = [m for maps in net(x) for m in maps]
    assert all(torch.equal(a, b) for a, b in zip(after, before_out))


@pytest.mark.parametrize("kw", [dict(ndf=32), dict(downsampling_factor=2), dict(n_layers=3), dict(n_layers=0),
                                dict(num_D=0)])
def test_unsupported_configurations_raise(mg, kw):
    with pytest.raises(ValueError):
        mg.melgan_discriminators.Discriminator(**kw)


def test_cpu_tensors_raise(mg):
    net = mg.melgan_discriminators.Discriminator(1)
    with pytest.raises(mg.MixganHipError):
        net(torch.zeros(1, 1, 64))
    with pytest.raises(mg.MixganHipError):
        net.model["disc_0"](torch.zeros(1, 1, 64))


def test_trainer_rejects_an_unknown_objective(mg):
    with pytest.raises(ValueError):
        mg.VocoderGANTrainer(torch.nn.Linear(1, 1), None, {"d": torch.nn.Linear(1, 1)}, objective="wgan")


def test_new_symbols_exported(mg):
    L = ctypes.CDLL(mg.library_path())
    for name in ("mg_avgpool4s2p1_fwd", "mg_avgpool4s2p1_bwd", "mg_reflect_pad1d_fwd", "mg_reflect_pad1d_bwd"):
        assert hasattr(L, name), name
        assert name in mg._lib.EXPORTS
    # the size queries know the two four-channel-group forms (host-only calls) and still refuse their neighbours
    lib = mg.lib()
    for cog, G in ((16, 4), (4, 256), (16, 5)):
        for mode in (mg._lib.MG_GCONV_FWD, mg._lib.MG_GCONV_DGRAD):
            assert lib.mg_gconv_packed_floats(4 * G, cog * G, 41, 4, G, mode) == cog * G * 4 * 41
        assert lib.mg_gconv1d_wgrad_scratch_floats(2, 4 * G, cog * G, 100, 41, 4, G) % (cog * G * 4 * 41) == 0
        assert lib.mg_gconv1d_wgrad_scratch_floats(2, 4 * G, cog * G, 100, 41, 4, G) > 0
    assert lib.mg_gconv_packed_floats(16, 32, 41, 4, 4, 0) == 0       # (4, 8, 4)
    assert lib.mg_gconv_packed_floats(16, 64, 40, 4, 4, 0) == 0       # K = 40
    assert lib.mg_gconv_packed_floats(16, 64, 41, 2, 4, 0) == 0       # stride 2 with Cig = 4
    assert (mg._lib.MG_LOSSMODE_MSE, mg._lib.MG_LOSSMODE_L1, mg._lib.MG_LOSSMODE_HINGE, mg._lib.MG_LOSSMODE_MEAN) == (0, 1, 2, 3)
