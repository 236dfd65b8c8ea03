"""The oracle's denoiser in float64 (the reference of test_gpu_denoiser_backward_shapes.py), on the CPU: it runs, the
step embedding it sees is the fp32-rounded one, and the float32 oracle's own forward / autograd error against it at
B=2, L=1000 -- the part of the project's bars (2e-5 forward, 5e-5 data gradients, 1e-4 parameter gradients) that was
reference rounding while the float32 oracle was the reference.  Those bars only meant something if that part is small:
asserted here at a tenth of each bar (measured: 6.6e-7 d_x, 6.4e-7 d_cond, at most 3.3e-6 on a parameter gradient)."""
import torch

from helpers import seeded, oracle_grads, rel_err, condition_relu_kinks
from oracle import refmath as R


def test_step_embedding_follows_dtype_with_fp32_values():
    t = torch.tensor([0, 1, 17, 500, 999])
    e32 = R.step_embedding(t)
    e64 = R.step_embedding(t, 256, torch.float64)
    assert e32.dtype == torch.float32 and e64.dtype == torch.float64
    assert torch.equal(e64, e32.double()), "the float64 run must see the fp32-rounded embedding, widened"


def test_float32_oracle_error_against_float64(manifest):
    W32, _ = seeded(manifest, "denoiser_ms1", 79, requires_grad=True)
    W64 = {k: v.detach().double().requires_grad_() for k, v in W32.items()}
    gen = torch.Generator().manual_seed(2)
    B, L = 2, 1000
    x, cond = torch.randn(B, 1, 80, L, generator=gen), torch.randn(B, 256, L, generator=gen)
    go, spk = torch.randn(B, 1, 80, L, generator=gen), torch.randn(B, 256, generator=gen)
    t = torch.tensor([999, 0])
    # a ReLU input that float32 puts on the other side of zero would cost O(1) in the gradient of its frames
    print("frames of x redrawn, of go projected:", condition_relu_kinks(W64, x, t, cond, spk, go, 2e-5, gen))
    ref = oracle_grads(W64, x, t, cond, spk, go, torch.float64)
    got = oracle_grads(W32, x, t, cond, spk, go, torch.float32)
    assert sorted(ref) == sorted(got) and all(v.dtype == torch.float64 for v in ref.values())
    worst = {}
    for k in ref:
        kind = "param" if k.startswith("param/") else k
        worst[kind] = max(worst.get(kind, 0.0), rel_err(got[k].numpy(), ref[k].numpy()))
    print("float32 oracle vs float64 oracle at (2, 1000):", {k: "%.2e" % v for k, v in worst.items()})
    assert worst["out"] <= 2e-6 and worst["d_x"] <= 5e-6 and worst["d_cond"] <= 5e-6 and worst["d_spk"] <= 5e-6
    assert worst["param"] <= 1e-5
