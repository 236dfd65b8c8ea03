"""The oracle's JCU discriminator in float64 with adopted activation masks (the reference of
test_gpu_discriminator_shapes.py), on the CPU: it follows the dtype of its weights and still meets the recorded
reference fixtures; `masks=` taken from a run's own output changes no bit of the maps or of any gradient; `taps=`
receives the ten pre-activations; and a mask that differs flips exactly the elements it names."""
import pytest
import torch
import torch.nn.functional as F

from helpers import golden, T, assert_close, seeded, jcu_oracle_grads
from oracle import refmath as R


def _own_masks(c, u):
    return [m > 0 for m in c], [m > 0 for m in u]


@pytest.mark.parametrize("ms", [0, 1])
@pytest.mark.parametrize("L", [37, 64])
def test_float64_jcu_forward_meets_the_fixtures(manifest, ms, L):
    g = golden("jcu_ms%d_L%d" % (ms, L))
    W32, _ = seeded(manifest, "jcu_ms%d" % ms, 41 + ms)
    W = {k: v.double() for k, v in W32.items()}
    s = T(g["s"]).double() if ms else None
    t = T(g["t"])
    for pair, (nc, nu) in ((T(g["fake"]), ("fc", "fu")), (T(g["real"]), ("rc", "ru"))):
        c, u = R.jcu_forward(W, T(g["x_ts"]).double(), pair.double(), s, t)
        for i in range(5):
            assert c[i].dtype == torch.float64 and u[i].dtype == torch.float64
            assert_close(c[i], g["%s%d" % (nc, i)], 5e-6, "%s%d" % (nc, i))
            assert_close(u[i], g["%s%d" % (nu, i)], 5e-6, "%s%d" % (nu, i))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("ms", [0, 1])
def test_own_masks_reproduce_the_unmasked_run_bit_for_bit(manifest, ms, dtype):
    W32, _ = seeded(manifest, "jcu_ms%d" % ms, 41 + ms)
    W = {k: v.to(dtype).requires_grad_() for k, v in W32.items()}
    gen = torch.Generator().manual_seed(5 + ms)
    B, L = 2, 131
    x_ts, x_prev = torch.randn(B, L, 80, generator=gen), torch.randn(B, L, 80, generator=gen)
    s = torch.randn(B, 256, generator=gen) if ms else None
    t = torch.tensor([0, 3])
    shapes = [(B, 64, 131), (B, 128, 66), (B, 512, 33), (B, 128, 33), (B, 1, 33)]
    cot = [[torch.randn(*sh, generator=gen) for sh in shapes] for _ in range(2)]
    plain = jcu_oracle_grads(W, x_ts, x_prev, s, t, cot, dtype)
    assert [tuple(plain["cond%d" % i].shape) for i in range(5)] == shapes
    masks = _own_masks([plain["cond%d" % i] for i in range(5)], [plain["uncond%d" % i] for i in range(5)])
    masked = jcu_oracle_grads(W, x_ts, x_prev, s, t, cot, dtype, masks=masks)
    assert sorted(plain) == sorted(masked)
    for k in plain:
        assert plain[k].dtype == dtype, k
        assert torch.equal(plain[k], masked[k]), k
    # the taps are the pre-activations of the maps, the shared three under both names
    for i in range(5):
        for side in ("cond", "uncond"):
            assert torch.equal(F.leaky_relu(plain["pre/%s%d" % (side, i)], 0.2), plain["%s%d" % (side, i)]), (side, i)
    for i in range(3):
        assert torch.equal(plain["pre/cond%d" % i], plain["pre/uncond%d" % i])


def test_a_foreign_mask_changes_exactly_the_elements_it_flips(manifest):
    W32, _ = seeded(manifest, "jcu_ms0", 41)
    W = {k: v.double() for k, v in W32.items()}
    gen = torch.Generator().manual_seed(9)
    x_ts, x_prev = torch.randn(1, 40, 80, generator=gen).double(), torch.randn(1, 40, 80, generator=gen).double()
    t = torch.tensor([2])
    taps = {}
    c, u = R.jcu_forward(W, x_ts, x_prev, None, t, taps=taps)
    mc, mu = _own_masks(c, u)
    mu[4] = ~mu[4]                      # the unconditional logit map with every sign decision inverted
    c2, u2 = R.jcu_forward(W, x_ts, x_prev, None, t, masks=(mc, mu))
    for i in range(5):
        assert torch.equal(c[i], c2[i])
    for i in range(4):
        assert torch.equal(u[i], u2[i])
    pre = taps["uncond4"]
    one = torch.ones((), dtype=torch.float64)
    assert torch.equal(u2[4], pre * torch.where(pre > 0, 0.2 * one, one))
