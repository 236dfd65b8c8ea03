"""Adam steps that the host queues ahead of the GPU (mixgan-tts_amd/optimizer.py FlatAdam, csrc/train_ops.hip
adam_flat_kernel).

HotPathTrainer.capture hands each optimizer's step-dependent scalars, lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t), to
the Adam kernel through device memory (FlatAdam.enable_device_hyper), so the host can queue replays -- and eager steps
-- without waiting for the GPU.  The FlatAdam and trainer tests queue their steps behind a GPU-busy prologue, check that
it is still running once the last step is queued (the host really was ahead), and only then read anything back: a step
that picked up another step's scalars changes the result, because every step gets its own gradient and its own bias
correction, and the learning rate changes half-way.

The yardstick is `adam64`, a float64 restatement of torch.optim.Adam (L2 weight decay, lerp first moment) after
clip_grad_norm_, fed the kernel's own float32 clip factor and the float32 hyper-parameters the kernel receives, so that
what it measures is the kernel's arithmetic (see `assert_adam64` for the bars)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PROLOGUE_MS = 200.0      # GPU time queued ahead of the steps; queueing six steps or four replays takes a few ms
U = 2.0 ** -24           # half an ulp of float32, relative
EPS = 1e-8
SCALES = (0.3, 1.0, 10.0, 0.05, 0.3, 2.0)       # gradient scale of step 1..6: every step differs


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd as m
    assert torch.cuda.is_available()
    m.lib()
    return m


@pytest.fixture(scope="module")
def prologue():
    """Returns a callable that queues ~PROLOGUE_MS of GPU work (torch.cuda._sleep) on the current stream and an event
    behind it.  Sized once from a timed call; the scale-up is bounded, so a bad timing cannot queue a long spin."""
    probe = 1 << 22
    torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    b.synchronize()
    cycles = int(probe * min(PROLOGUE_MS / max(a.elapsed_time(b), 1e-3), 1000.0))

    def run():
        torch.cuda._sleep(cycles)
        ev = torch.cuda.Event()
        ev.record()
        return ev
    return run


def assert_host_was_ahead(ev):
    assert not ev.query(), ("the GPU prologue had finished before the last step was queued, so this run never let the "
                            "host run ahead of the GPU: lengthen the prologue (PROLOGUE_MS)")


def f32(x):
    return float(np.float32(x))


def launch_scalars(lr, betas, t):
    """The pair mg_adam_flat_dev derives from its float arguments: float32 of the double expressions over the float32
    lr and betas."""
    lr, b1, b2 = f32(lr), f32(betas[0]), f32(betas[1])
    return np.float32(lr / (1.0 - b1 ** t)), np.float32(1.0 / math.sqrt(1.0 - b2 ** t))


def adam64(p, m, v, g, clip, lr, betas, eps, wd, t):
    """One torch.optim.Adam step after clip_grad_norm_, in float64 (p, m, v, g: float64 tensors; clip: the factor)."""
    b1, b2 = betas
    g = g * clip
    if wd:
        g = g + wd * p                                   # L2 weight decay, torch.optim.Adam's default
    m = m + (1.0 - b1) * (g - m)                         # torch.lerp(m, g, 1 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr / (1.0 - b1 ** t) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v


def step1_cancels(p0, g1, clip1, wd):
    """With weight decay: the elements whose first effective gradient g * clip + wd * p lies within 1e-5 of zero."""
    return (g1 * clip1 + wd * p0).abs() < 1e-5 if wd else torch.zeros(p0.shape, dtype=torch.bool)


def _within(what, got, ref, rtol, atol):
    err = (got - ref).abs()
    over = err > rtol * ref.abs() + atol
    if bool(over.any()):
        i = int((err - rtol * ref.abs() - atol).argmax())
        raise AssertionError("%s: %d of %d elements beyond the bar; worst at %d: %.9e vs float64 %.9e" % (
            what, int(over.sum()), over.numel(), i, float(got[i]), float(ref[i])))


def assert_adam64(what, p, m, v, ref, lr0, wd, cancels, gmax):
    """p, m, v (device float32) against the float64 state `ref` after six steps (lr0: the learning rate of step 1).
    Bars, in U = 2^-24, with what the MI355X needed at n = 8.4M, the largest case, in parentheses:
    - v is a sum of non-negative terms: relative only, 16 U (<= 7.7 U).
    - p: every step rounds p once, 8 U of |p| covers six of them.  The updates themselves are accurate to a few U of
      their size, lr0 ~ 2e-3: atol 4e-9 (<= 1e-9).  One exception: with weight decay, g * clip + wd * p can cancel to
      near zero in step 1, where the update lr * g / (|g| + eps) has slope lr * eps / (|g| + eps)^2 -- up to 2e5 -- in
      g, so the last bit of the float32 g * clip moves p by up to micro-units (5.5e-6 measured).  Bounded by the step-1
      update itself, lr0: the elements with |g * clip + wd * p| < 1e-5 in step 1 (`cancels`, where the slope is still
      above 0.2; a few hundred of 8.4M) get atol 2 lr0 instead.
      The suite's earlier bar was rtol 2e-6 (34 U), atol 1e-5 on every element.
    - m = lerp(m, g, 1 - beta1) can cancel to near zero: relative 8 U, plus one U of the largest effective
      gradient seen, gmax = max |g * clip| + wd max |p| (<= 0.22 of that).
    - Through wd * p, the p of a `cancels` element feeds its error into every later gradient: up to dg = wd * 2 lr0,
      which m may carry as is and v as 2 gmax dg (needed where g * clip is small next to wd * p, as in the FlatAdam
      tests)."""
    P, M, V = ref
    got = [x.detach().double().cpu() for x in (p, m, v)]
    at_p = torch.where(cancels, 2.0 * lr0, 4e-9)
    print("%s: p needs atol %.2e outside the %d step-1 cancellations; m needs %.3f U*gmax; v max rel %.1f U" % (
        what, float((got[0] - P).abs().sub(8 * U * P.abs()).masked_fill(cancels, 0).max().clamp(min=0)),
        int(cancels.sum()), float(((got[1] - M).abs() - 8 * U * M.abs()).max().clamp(min=0)) / (U * gmax),
        float(((got[2] - V).abs() / V).max()) / U))
    _within(what + " p", got[0], P, 8 * U, at_p)
    dg = wd * 2.0 * lr0
    _within(what + " m", got[1], M, 8 * U, torch.where(cancels, U * gmax + dg, U * gmax))
    _within(what + " v", got[2], V, 16 * U, torch.where(cancels, 2.0 * gmax * dg, 0.0))


# --------------------------------------------------------------------------------------------------------------------
# (a) the kernel: launch-argument scalars vs device scalars, both against float64


@pytest.mark.parametrize("clipped", [False, True], ids=["clip1", "clip<1"])
@pytest.mark.parametrize("betas,wd", [((0.5, 0.9), 0.0), ((0.5, 0.9), 0.01), ((0.9, 0.999), 0.0), ((0.9, 0.999), 0.01)])
@pytest.mark.parametrize("n", [1, 3, 5, 1021, 2 * 4096 * 256 * 4 + 3])    # last: two grid-stride sweeps plus a tail
def test_adam_kernel_transports_agree_and_match_float64(mg, n, betas, wd, clipped):
    gen = torch.Generator().manual_seed(n % 9973 + 17)
    p0 = torch.randn(n, generator=gen)
    arg = [p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    dev = [x.clone() for x in arg]
    ref = (p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64))
    b32 = (f32(betas[0]), f32(betas[1]))
    gmax = 0.0
    for t in range(1, 7):
        lr = 2e-3 if t <= 3 else 5e-4
        g = torch.randn(n, generator=gen) * SCALES[t - 1]
        gd = g.cuda()
        max_norm = 0.37 * float(torch.linalg.vector_norm(g.double())) if clipped else 1e9
        norm = mg.ops.grad_norm(gd, max_norm)
        clip = float(norm[1])
        assert (clip < 1.0) if clipped else (clip == 1.0)
        hyper = torch.tensor(launch_scalars(lr, betas, t), dtype=torch.float32).cuda()     # synchronous fill
        mg.ops.adam_flat(arg[0], gd, arg[1], arg[2], lr, betas, EPS, wd, t, norm[1:])
        # lr = 0 at step 1 in the launch arguments: only the device pair can move p
        mg.ops.adam_flat(dev[0], gd, dev[1], dev[2], 0.0, betas, EPS, wd, 1, norm[1:], hyper=hyper)
        for name, a, d in zip("pmv", arg, dev):
            assert torch.equal(a, d), "step %d: %s differs between launch-argument and device scalars" % (t, name)
        if t == 1:
            cancels = step1_cancels(ref[0], g.double(), clip, f32(wd))
        ref = adam64(*ref, g.double(), clip, f32(lr), b32, f32(EPS), f32(wd), t)
        gmax = max(gmax, float(g.abs().max()) * clip + f32(wd) * float(ref[0].abs().max()))
    torch.cuda.synchronize()
    assert_adam64("n=%d betas=%s wd=%g clip<1=%s" % (n, betas, wd, clipped), *arg, ref, 2e-3, f32(wd), cancels, gmax)


# --------------------------------------------------------------------------------------------------------------------
# (b), (c) FlatAdam steps queued eagerly and as graph replays, against a synced twin on the launch-argument path

# lr and betas exactly representable in float32, so that the pair write_hyper stages (float32 of double expressions
# over the Python floats) and the pair the launcher derives from float32 arguments are the same numbers, and the two
# paths must agree bit for bit
LR, BETAS, GAMMA, WD, CLIP = 2.0 ** -9, (0.5, 0.875), 0.5, 0.01, 1.0
SHAPES = [(256, 80, 1), (256,), (512, 256, 3), (7,), (3, 5), (1,), (128, 33)]     # 418 199 floats: n & 3 = 3


def _bucket(mg):
    g = torch.Generator().manual_seed(5)
    return mg.GradBucket([torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in SHAPES])


def _grads(n):
    g = torch.Generator().manual_seed(6)
    return [(torch.randn(n, generator=g) * (s * 1e-3 if i == 1 else s)).cuda() for i, s in enumerate(SCALES)]


def _synced_twin(mg, grads):
    """Six steps on the launch-argument path, each followed by a synchronisation; returns the optimizer and the float64
    state of the same six steps (with the twin's clip factors)."""
    bucket = _bucket(mg)
    opt = mg.FlatAdam(bucket, lr=LR, betas=BETAS, weight_decay=WD)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=GAMMA)
    ref = (opt.flat_p.double().cpu(), torch.zeros(opt.flat_p.numel(), dtype=torch.float64),
           torch.zeros(opt.flat_p.numel(), dtype=torch.float64))
    clips, gmax = [], 0.0
    for i, g in enumerate(grads):
        if i == 3:
            sched.step()
        lr = opt.param_groups[0]["lr"]
        b1, b2 = BETAS
        t = i + 1
        staged = (np.float32(lr / (1.0 - b1 ** t)), np.float32(1.0 / (1.0 - b2 ** t) ** 0.5))
        assert staged == launch_scalars(lr, BETAS, t), "lr / betas must be exact in float32 for a bitwise comparison"
        bucket.flat.copy_(g)
        out = opt.step(max_grad_norm=CLIP)
        torch.cuda.synchronize()
        clips.append(float(out[1]))
        if t == 1:
            cancels = step1_cancels(ref[0], g.double().cpu(), clips[0], f32(WD))
        gmax = max(gmax, float(g.abs().max()) * clips[-1] + f32(WD) * float(ref[0].abs().max()))
        ref = adam64(*ref, g.double().cpu(), clips[-1], lr, BETAS, f32(EPS), f32(WD), t)
    assert min(clips) < 1.0 == max(clips), "the steps should cover clipped and unclipped gradients"
    return opt, ref, cancels, gmax


def _assert_equal_to_twin(opt, twin):
    for name in ("flat_p", "flat_m", "flat_v"):
        a, b = getattr(opt, name), getattr(twin, name)
        assert torch.equal(a, b), "%s differs from the synced twin in %d of %d elements" % (
            name, int((a != b).sum()), a.numel())
    assert float(opt._steps) == float(twin._steps) == 6


def test_queued_eager_steps_equal_synced_steps(mg, prologue):
    bucket = _bucket(mg)
    grads = _grads(bucket.flat.numel())
    twin, ref, cancels, gmax = _synced_twin(mg, grads)
    opt = mg.FlatAdam(bucket, lr=LR, betas=BETAS, weight_decay=WD).enable_device_hyper()
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=GAMMA)
    torch.cuda.synchronize()
    ev = prologue()
    for i, g in enumerate(grads):
        if i == 3:
            sched.step()
        bucket.flat.copy_(g)
        opt.step(max_grad_norm=CLIP)
    assert_host_was_ahead(ev)
    torch.cuda.synchronize()
    _assert_equal_to_twin(opt, twin)
    assert_adam64("queued eager steps", opt.flat_p, opt.flat_m, opt.flat_v, ref, LR, f32(WD), cancels, gmax)


def test_queued_graph_replays_equal_synced_steps(mg, prologue):
    bucket = _bucket(mg)
    grads = _grads(bucket.flat.numel())
    twin, ref, cancels, gmax = _synced_twin(mg, grads)
    opt = mg.FlatAdam(bucket, lr=LR, betas=BETAS, weight_decay=WD).enable_device_hyper()
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=GAMMA)
    static_grad = torch.zeros_like(bucket.flat)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bucket.flat.copy_(static_grad)
        opt.step(max_grad_norm=CLIP)
    opt._steps -= 1                  # the capture ran nothing (HotPathTrainer.capture undoes its count the same way)
    assert float(opt._steps) == 0 and torch.count_nonzero(opt.flat_m) == 0
    torch.cuda.synchronize()
    ev = prologue()
    for i, g in enumerate(grads):
        if i == 3:
            sched.step()
        static_grad.copy_(g)
        opt.prepare_replay()         # what the trainer's captured step does before every replay
        graph.replay()
    assert_host_was_ahead(ev)
    torch.cuda.synchronize()
    _assert_equal_to_twin(opt, twin)
    assert_adam64("queued graph replays", opt.flat_p, opt.flat_m, opt.flat_v, ref, LR, f32(WD), cancels, gmax)


# --------------------------------------------------------------------------------------------------------------------
# (d) the captured GAN step: replays queued behind the prologue vs replays read back one by one


def _replayed_trainer(mg, manifest, tmp_path, queued, prologue):
    from test_gpu_trainer_boundary import _setup
    G, D, _, _, _, mel, conds, pad, _, tr, mc = _setup(mg, manifest, tmp_path, B=3, L=64)
    trainer = mg.HotPathTrainer(G, D, tr, mc)
    batch = (mel.cuda(), conds[0].cuda(), None, pad.cuda())
    torch.cuda.manual_seed(1234)                 # same t / noise in the capture's warm-up steps ...
    step = trainer.capture(*batch)
    torch.cuda.manual_seed(4321)                 # ... and in the replays
    ev = prologue() if queued else None
    for i in range(4):
        if i == 2:
            trainer.end_epoch()
        out = step(*batch)
        if not queued:
            losses = {k: float(v) for k, v in out.items()}
    if queued:
        assert_host_was_ahead(ev)
        losses = {k: float(v) for k, v in out.items()}
    trainer.check()
    return {"moments": [x.clone() for o in (trainer.optG, trainer.optD) for x in (o.flat_m, o.flat_v)],
            "losses": losses, "steps": (float(trainer.optG._steps), float(trainer.optD._steps))}


def test_queued_trainer_replays_match_synced_replays(mg, manifest, tmp_path, prologue):
    """Four replays queued behind the prologue against four read back one by one, same weights, data and t / noise.

    Not bitwise: two captured trainers that both read back after every replay already differ.  The step is not
    run-to-run deterministic -- mg_denoiser_bwd sums the diffusion-step gradient over the residual layers with one
    fp32 atomicAdd per layer (small_linear_t_kernel, Z > 1), so the step MLP's weight gradients (mlp.0 / mlp.2) differ
    in the last bits between runs, and the mel L1 loss value is summed with atomics (mel_l1 forward) -- and Adam's
    normalised updates carry such differences into every weight after a few steps.  Measured on the MI355X at this
    size, synced against synced (worst of the runs seen) and, with the earlier pinned staging copy put back, queued
    against synced: relative loss differences mel 2.3e-5 / 4.5e-3, fm 2.7e-6 / 2.6e-3, adv 5e-4 / 4.3e-2; relative
    difference of the discriminator's moments m 6.1e-3 / 8.8e-2, v 5.2e-4 / 4.1e-2.  The bars sit between the two:
    5x to 70x above the run-to-run spread, 3x to 20x below what replays reading other steps' Adam scalars did."""
    synced = _replayed_trainer(mg, manifest, tmp_path, False, prologue)
    queued = _replayed_trainer(mg, manifest, tmp_path, True, prologue)
    assert synced["steps"] == queued["steps"]
    assert all(np.isfinite(v) for v in synced["losses"].values())
    for k, bar in (("mel_loss", 2e-4), ("fm_loss", 2e-4), ("adv_loss", 5e-3)):
        a, b = queued["losses"][k], synced["losses"][k]
        assert abs(a - b) <= bar * abs(b), "%s: queued %.9g, synced %.9g" % (k, a, b)
    for i, (name, bar) in enumerate((("D m", 3e-2), ("D v", 5e-3)), start=2):
        a, b = queued["moments"][i], synced["moments"][i]
        rel = float((a - b).norm() / b.norm())
        assert rel <= bar, "%s: queued differs from synced by %.3g of its norm" % (name, rel)
