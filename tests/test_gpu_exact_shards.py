"""Exact multi-rank training steps on ragged shards (HotPathTrainer(exact_shards=True)).

Kernels: mg_multi_loss_fwd_den / _bwd_den against float64 torch (bars of tests/test_gpu_discriminator_shapes.py: loss
scalars 2e-6 max(1, |ref|), loss gradients 1e-6 max-abs / max-ref) and bit for bit against the plain entry points when
den == n; mg_mel_count_rows against torch, as integers; the argument errors.

Trainer: two processes share the one test GPU (gloo carries the collectives, as in tests/test_gpu_distributed_trainer.py,
whose scaffolding and tolerances are copied here because the situation is the same).  The global batch has N = 4 items of
64, 40, 23 and 9 frames; every rank gets its rows cut to ITS OWN longest item -- rank 1 of the (2, 2) split holds 23
frames, rank 1 of (3, 1) one item of 9 -- and must reproduce the single process stepping on the whole batch: reduced
gradients of all four updates (2e-4 in step 1, 2e-3 in step 2, which starts from weights that already differ in the last
bits), the weight update within 2e-2 in L2, identical weights on both ranks, loss shares that add up to the single-process
losses at 2e-6 max(1, |ref|).  A guard runs the (2, 2) split WITHOUT exact_shards on hand-padded tensors: its first G
update must miss the single-process one by more than ten times the bar, or the inputs would prove nothing (rank 0 counts
104 mel rows, rank 1 counts 32: the mean of means weighs rank 1's mel gradient about 2.1 times too heavily).

Loader: PrefetchLoader(shape_group=...) on two ranks pads every sub-batch to the longer rank's length and attaches the
same BatchShape on both.

Workers report exceptions through the queue and every wait carries a timeout; at most three processes hold the GPU."""
import ctypes
import json
import os
import queue as queue_mod
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import golden, hot_path_configs, write_stats, load_seeded, Tape
from test_data_path import tree  # noqa: F401  (fixture: rebuilds the synthetic preprocessed tree from dataset.npz)

pytestmark = pytest.mark.gpu
LOSS_T, LOSS_GT = 2e-6, 1e-6
LENS = [64, 40, 23, 9]
N, L, STEPS = 4, 64, 2
WAIT = 240


@pytest.fixture(scope="module")
def mg():
    import mixgan_tts_amd
    return mixgan_tts_amd


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "manifest.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------ mg_multi_loss_fwd_den / _bwd_den
SIZES = [1, 255, 257, 4099, 300001]       # 300001: 147 blocks wanted, 64 (forward) / 147 (backward) granted


def _terms_data(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for k, n in enumerate(sizes):
        mode = k % 2
        a = torch.randn(n, generator=gen).cuda()
        b = torch.randn(n, generator=gen).cuda() if mode == 1 else None
        out.append((mode, a, b, 0.5 + 0.25 * k, 0.3 + 0.1 * k, k % 4))     # mode, a, b, c, weight, group
    return out


def _launch(mg, data, den, g, with_den):
    """Forward + backward through the C ABI; den: list of host doubles (with_den) or ignored."""
    from mixgan_tts_amd import _lib
    from mixgan_tts_amd._lib import fptr, stream_ptr
    nt = len(data)
    L_ = _lib.lib()
    grads = [torch.full_like(a, 7.0) for _, a, *_ in data]
    terms = (_lib.LossTerm * nt)()
    for k, ((mode, a, b, c, w, grp), d) in enumerate(zip(data, grads)):
        terms[k] = _lib.LossTerm(fptr(a).value, fptr(b).value if b is not None else None, fptr(d).value, a.numel(), c, w,
                                 mode, grp)
    scratch = torch.zeros(L_.mg_multi_loss_scratch_floats(), device="cuda")
    out = torch.empty(1 + _lib.MG_LOSS_GROUPS + nt, device="cuda")
    gd = torch.tensor([g], device="cuda")
    if with_den:
        dens = (ctypes.c_double * nt)(*den)
        _lib.check(L_.mg_multi_loss_fwd_den(terms, nt, dens, fptr(scratch), fptr(out), stream_ptr()))
        _lib.check(L_.mg_multi_loss_bwd_den(terms, nt, dens, fptr(gd), stream_ptr()))
    else:
        _lib.check(L_.mg_multi_loss_fwd(terms, nt, fptr(scratch), fptr(out), stream_ptr()))
        _lib.check(L_.mg_multi_loss_bwd(terms, nt, fptr(gd), stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu(), [d.cpu() for d in grads]


# ------------------------------------------------------------------ the Python loss table against one built by hand
# The multi-loss kernels sum in a fixed order, so the spec builders of losses.py must return the bits of a table written
# out here: whole result vector and every gradient, torch.equal.
G_OUT = 0.625        # the cotangent of the total


def _through_python(out, inputs):
    grads = torch.autograd.grad(out[0] * G_OUT, inputs)
    torch.cuda.synchronize()
    return out.detach().cpu(), [d.cpu() for d in grads]


@pytest.mark.parametrize("n", [1, 257, 4099, 12306])          # 12306: several 2048-element blocks per term
def test_weighted_means_is_the_hand_built_table(mg, n):
    from mixgan_tts_amd import _lib
    gen = torch.Generator().manual_seed(n)
    xs = [torch.randn(n, generator=gen).cuda().requires_grad_() for _ in range(4)]
    y = torch.randn(n, generator=gen).cuda()                  # the "l1" term's target: a tensor of its own
    out, grads = _through_python(
        mg.losses.weighted_means([("mse", xs[0], 0.75, 0.5, 0), ("l1", xs[1], y, 1.25, 1), ("hinge", xs[2], -1.0, 0.3, 2),
                                  ("mean", xs[3], None, -1.0, 3)]), xs)
    data = [(_lib.MG_LOSSMODE_MSE, xs[0].detach(), None, 0.75, 0.5, 0), (_lib.MG_LOSSMODE_L1, xs[1].detach(), y, 0.0, 1.25, 1),
            (_lib.MG_LOSSMODE_HINGE, xs[2].detach(), None, -1.0, 0.3, 2), (_lib.MG_LOSSMODE_MEAN, xs[3].detach(), None, 0.0, -1.0, 3)]
    ref_out, ref_grads = _launch(mg, data, None, G_OUT, False)
    assert torch.equal(out, ref_out)
    for k, (d, r) in enumerate(zip(grads, ref_grads)):
        assert torch.equal(d, r), "gradient of term %d" % k


@pytest.mark.parametrize("n_total", [None, 7])
def test_2b_totals_are_the_hand_built_tables(mg, n_total):
    from mixgan_tts_amd import _lib
    MSE, L1 = _lib.MG_LOSSMODE_MSE, _lib.MG_LOSSMODE_L1
    gen = torch.Generator().manual_seed(9)
    B, lam, n_layers = 3, 10.0, 5
    shapes = [(5, 33), (4, 17), (7, 293), (1, 9)]
    cm, um = ([torch.randn(2 * B, c, l, generator=gen).cuda().requires_grad_() for c, l in shapes] for _ in range(2))
    rows = lambda m, lo: m.detach()[lo:lo + B].reshape(-1)  # noqa: E731  (views: the table points into the maps)
    den = lambda data: [float(a.numel() // B * n_total) for _, a, *_ in data]  # noqa: E731
    # discriminator: real rows against 1, fake rows against 0, on the last maps
    tot, d_real, d_fake = mg.losses.d_loss_total_2b(cm[-1], um[-1], B, n_total=n_total)
    out, grads = _through_python(tot._base, [cm[-1], um[-1]])        # the result vector the three are views of
    assert torch.equal(torch.stack([tot, d_real, d_fake]).detach().cpu(), out[:3])
    data = [(MSE, rows(cm[-1], B), None, 1.0, 0.5, 0), (MSE, rows(um[-1], B), None, 1.0, 0.5, 0),
            (MSE, rows(cm[-1], 0), None, 0.0, 0.5, 1), (MSE, rows(um[-1], 0), None, 0.0, 0.5, 1)]
    ref_out, ref = _launch(mg, data, den(data) if n_total else None, G_OUT, n_total is not None)
    assert torch.equal(out, ref_out)
    for m, real, fake in zip(grads, ref[:2], ref[2:]):
        assert torch.equal(m, torch.cat([fake, real]).view_as(m))
    # generator: fake rows of the last maps against 1, fake rows of the others against their real rows
    maps = cm + um
    tot, adv, fm = mg.losses.g_adv_fm_total_2b(cm, um, B, lam, n_layers, n_total=n_total)
    out, grads = _through_python(tot._base, maps)
    assert torch.equal(torch.stack([tot, adv, fm]).detach().cpu(), out[:3])
    w = lam * (4.0 / (n_layers + 1)) * 0.5
    data = [(MSE, rows(cm[-1], 0), None, 1.0, 0.5, 0), (MSE, rows(um[-1], 0), None, 1.0, 0.5, 0)]
    for j in range(len(shapes) - 1):
        data += [(L1, rows(cm[j], 0), rows(cm[j], B), 0.0, w, 1), (L1, rows(um[j], 0), rows(um[j], B), 0.0, w, 1)]
    ref_out, ref = _launch(mg, data, den(data) if n_total else None, G_OUT, n_total is not None)
    assert torch.equal(out, ref_out)
    order = [cm[-1], um[-1]] + [m for j in range(len(shapes) - 1) for m in (cm[j], um[j])]     # the terms' maps
    for m, r in zip(order, ref):
        d = grads[[id(x) for x in maps].index(id(m))]
        assert torch.equal(d[:B].reshape(-1), r), "fake rows"
        assert not d[B:].any(), "the real rows are targets: exactly zero"


def _reference(data, den, g):
    """float64: [total, 4 group subtotals, per-term sum / den] and every term's gradient."""
    total, groups, means, grads = 0.0, [0.0] * 4, [], []
    for (mode, a, b, c, w, grp), dk in zip(data, den):
        a64 = a.double().cpu().requires_grad_()
        s = (a64 - c).pow(2).sum() if mode == 0 else (a64 - b.double().cpu()).abs().sum()
        term = s / dk
        (ga,) = torch.autograd.grad(g * w * term, a64)
        grads.append(ga)
        term = float(term.detach())
        means.append(term)
        total += w * term
        groups[grp] += w * term
    return torch.tensor([total] + groups + means, dtype=torch.float64), grads


def _judge(out, grads, ref_out, ref_grads):
    fails = []
    for i, (v, r) in enumerate(zip(out.double().tolist(), ref_out.tolist())):
        err = abs(v - r) / max(1.0, abs(r))
        print("EXACTERR scalar %d: %.3e (ref %.6g)" % (i, err, r))
        if not err <= LOSS_T:
            fails.append(("scalar", i, err))
    for k, (d, r) in enumerate(zip(grads, ref_grads)):
        err = float((d.double() - r).abs().max() / (r.abs().max() + 1e-30))
        print("EXACTERR grad %d (n=%d): %.3e" % (k, d.numel(), err))
        if not err <= LOSS_GT:
            fails.append(("grad", k, err))
    assert not fails, fails


@pytest.mark.parametrize("case", ["sizes", "max_terms"])
def test_den_kernels_vs_float64(mg, case):
    from mixgan_tts_amd import _lib
    if case == "sizes":      # every size in both modes
        sizes = [n for n in SIZES for _ in (0, 1)]
    else:
        sizes = [SIZES[k % 4] + 3 * k for k in range(_lib.MG_LOSS_MAX_TERMS)]
        assert len(sizes) == 16
    data = _terms_data(sizes, 21)
    den = [1.7 * n + 3.0 for n in sizes]                   # den != n: what the ranks of a sharded batch pass
    out, grads = _launch(mg, data, den, 0.75, True)
    ref_out, ref_grads = _reference(data, den, 0.75)
    _judge(out, grads, ref_out, ref_grads)


def test_den_equal_n_returns_the_bits_of_the_plain_entry_points(mg):
    sizes = [n for n in SIZES for _ in (0, 1)]
    data = _terms_data(sizes, 22)
    out_d, grads_d = _launch(mg, data, [float(n) for n in sizes], 1.25, True)
    out_p, grads_p = _launch(mg, data, None, 1.25, False)
    assert torch.equal(out_d, out_p)
    for a, b in zip(grads_d, grads_p):
        assert torch.equal(a, b)
    ref_out, ref_grads = _reference(data, [float(n) for n in sizes], 1.25)
    _judge(out_d, grads_d, ref_out, ref_grads)


def test_range_means_and_l1_take_denominators(mg):
    """The Python layer on top: d_loss_total_2b / g_adv_fm_total_2b with n_total, _L1Fn with a host denominator."""
    gen = torch.Generator().manual_seed(4)
    B, n_total = 3, 7
    maps = [torch.randn(2 * B, c, l, generator=gen).cuda().requires_grad_() for c, l in ((5, 33), (4, 17), (1, 9))]
    umaps = [torch.randn(2 * B, c, l, generator=gen).cuda().requires_grad_() for c, l in ((5, 33), (4, 17), (1, 9))]
    tot, adv, fm = mg.losses.g_adv_fm_total_2b(maps, umaps, B, 10.0, 5, n_total=n_total)
    tot_p, adv_p, fm_p = mg.losses.g_adv_fm_total_2b(maps, umaps, B, 10.0, 5)
    for v, p in ((tot, tot_p), (adv, adv_p), (fm, fm_p)):     # every term's denominator grows by n_total / B
        v, p = float(v.detach()), float(p.detach())
        assert abs(v - p * B / n_total) <= LOSS_T * max(1.0, abs(p))
    (g_d,) = torch.autograd.grad(tot, maps[0])
    (g_p,) = torch.autograd.grad(tot_p, maps[0])
    assert float((g_d.double() * n_total / B - g_p.double()).abs().max() / g_p.abs().max()) <= LOSS_GT
    d, _, _ = mg.losses.d_loss_total_2b(maps[-1], umaps[-1], B, n_total=n_total)
    d_p, _, _ = mg.losses.d_loss_total_2b(maps[-1], umaps[-1], B)
    d, d_p = float(d.detach()), float(d_p.detach())
    assert abs(d - d_p * B / n_total) <= LOSS_T * max(1.0, abs(d_p))
    x = torch.randn(2, 11, 80, generator=gen).cuda().requires_grad_()
    y = torch.randn(2, 11, 80, generator=gen).cuda()
    l1 = mg.losses._L1Fn.apply(x, y, 5 * 11 * 80)
    ref = (x.detach().double() - y.double()).abs().sum() / (5 * 11 * 80)
    (gx,) = torch.autograd.grad(l1, x)
    assert abs(float(l1.detach()) - float(ref)) <= LOSS_T * max(1.0, abs(float(ref)))
    ref_g = torch.sign(x.detach().double() - y.double()) / (5 * 11 * 80)
    assert float((gx.double() - ref_g).abs().max() / ref_g.abs().max()) <= LOSS_GT


# ------------------------------------------------------------------ mg_mel_count_rows
@pytest.mark.parametrize("M", [3, 80, 130])
@pytest.mark.parametrize("rows", [1, 5, 2051])          # 2051: past one grid sweep of 512 blocks x 4 rows
def test_mel_count_rows_equals_torch(mg, rows, M):
    gen = torch.Generator().manual_seed(rows * 1000 + M)
    targ = torch.randn(1, rows, M, generator=gen)
    zero = torch.rand(rows, generator=gen) < 0.3          # unpadded all-zero rows: not counted
    pad = torch.rand(rows, generator=gen) < 0.3           # padded rows, most of them non-zero: not counted
    if rows >= 5:
        zero[0], pad[0], zero[1], pad[1], zero[2], pad[2] = True, False, False, True, True, True
        assert (zero & ~pad).any() and (pad & ~zero).any()
    targ[0, zero] = 0.0
    targ[0, ~zero, :-1] *= (torch.rand(int((~zero).sum()), M - 1, generator=gen) < 0.5)     # rows with few non-zeros
    want = int(((targ[0] != 0).any(-1) & ~pad).sum())
    got = mg.losses.mel_count_rows(targ.cuda(), pad[None].cuda())
    assert got.dtype == torch.int64 and got.shape == (1,) and int(got) == want
    counts = mg.ShardCounts("cuda")
    mg.losses.mel_count_rows(targ.cuda(), pad[None].cuda(), out=counts.slot("mel_rows"))
    counts.all_reduce_async()
    assert int(counts["mel_rows"]) == want and counts.vec.tolist()[1:] == [0, 0, 0]
    assert int(mg.losses.mel_count_rows(targ.cuda(), None)) == int((targ[0] != 0).any(-1).sum())
    # ... and it is the count the mel L1 divides by
    out2 = torch.empty(2, device="cuda")
    from mixgan_tts_amd import _lib
    pad8 = pad[None].to(torch.uint8).cuda()
    t = targ.cuda()
    _lib.check(_lib.lib().mg_mel_l1_fwd(_lib.fptr(t), _lib.fptr(t), _lib.iptr(pad8, torch.uint8), rows, M, _lib.fptr(out2),
                                        _lib.stream_ptr()))
    assert float(out2[1]) == want * M


def test_argument_errors_come_back_without_a_launch(mg):
    from mixgan_tts_amd import _lib
    from mixgan_tts_amd._lib import fptr, iptr, stream_ptr, MG_ERR_ARG, MG_ERR_SHAPE
    L_ = _lib.lib()
    t = torch.ones(4, 80, device="cuda")
    out = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    o = iptr(out, torch.int64)
    assert L_.mg_mel_count_rows(None, None, 4, 80, o, stream_ptr()) == MG_ERR_ARG
    assert L_.mg_mel_count_rows(fptr(t), None, 4, 80, None, stream_ptr()) == MG_ERR_ARG
    assert L_.mg_mel_count_rows(fptr(t), None, 0, 80, o, stream_ptr()) == MG_ERR_SHAPE
    assert L_.mg_mel_count_rows(fptr(t), None, -1, 80, o, stream_ptr()) == MG_ERR_SHAPE
    assert L_.mg_mel_count_rows(fptr(t), None, 4, 0, o, stream_ptr()) == MG_ERR_SHAPE
    a = torch.ones(100, device="cuda")
    da = torch.full((100,), 7.0, device="cuda")
    terms = (_lib.LossTerm * 1)(_lib.LossTerm(fptr(a).value, None, fptr(da).value, 100, 0.0, 1.0, 0, 0))
    scratch = torch.zeros(L_.mg_multi_loss_scratch_floats(), device="cuda")
    res = torch.full((1 + _lib.MG_LOSS_GROUPS + 1,), -5.0, device="cuda")
    g = torch.ones(1, device="cuda")
    for bad in (0.0, -3.0, float("nan")):
        den = (ctypes.c_double * 1)(bad)
        assert L_.mg_multi_loss_fwd_den(terms, 1, den, fptr(scratch), fptr(res), stream_ptr()) == MG_ERR_ARG
        assert L_.mg_multi_loss_bwd_den(terms, 1, den, fptr(g), stream_ptr()) == MG_ERR_ARG
    assert L_.mg_multi_loss_fwd_den(terms, 1, None, fptr(scratch), fptr(res), stream_ptr()) == MG_ERR_ARG
    assert L_.mg_multi_loss_bwd_den(terms, 1, None, fptr(g), stream_ptr()) == MG_ERR_ARG
    torch.cuda.synchronize()
    assert int(out) == -5 and (res == -5.0).all() and (da == 7.0).all() and not scratch.any()      # nothing ran
    with pytest.raises(mg.MixganHipError):
        mg.losses._range_means([(0, 0, 1.0, 0.5, 0, 0, 1, 0)], [a.view(1, 100)], den=[0.0])


# ------------------------------------------------------------------ processes
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(body, world, *args):
    """Run the module-level function named `body` as body(rank, world, *args) in `world` fresh processes (_worker);
    their results in rank order.  A worker that raises reports through the queue, one that dies silently is noticed by
    its exit code: the parent never waits out a hang, and nothing is tried twice."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, body) + args) for r in range(world)]
    for p in procs:
        p.start()
    got, problem, waited = [], None, 0
    try:
        while len(got) < world and problem is None and waited < WAIT:
            try:
                item = q.get(timeout=2)
            except queue_mod.Empty:
                waited += 2
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                if dead:
                    problem = "a worker died with exit code %s" % dead
                continue
            if item[1] != "ok":
                problem = "rank %d: %s" % (item[0], item[2])
            got.append(item)
        if problem is None and len(got) < world:
            problem = "no result within %d s" % WAIT
    finally:
        for p in procs:
            p.join(30 if problem is None else 2)
            if p.is_alive():
                p.kill()
                p.join(10)
    assert problem is None, problem
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [item[2] for item in sorted(got, key=lambda t_: t_[0])]


def _worker(rank, world, port, q, body, *args):
    """Worker: a gloo process group around globals()[body](rank, world, *args) -> picklable result; errors go through
    the queue."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            q.put((rank, "ok", globals()[body](rank, world, *args)))
        finally:
            dist.destroy_process_group()
    except BaseException as exc:
        q.put((rank, "error", repr(exc)))
        raise


# ------------------------------------------------------------------ the trainer across two ranks
def _data(kind):
    gen = torch.Generator().manual_seed(78)
    keep = (torch.arange(L)[None, :] < torch.tensor(LENS)[:, None])
    mel = (torch.rand(N, L, 80, generator=gen) * 13.5 - 11.5) * keep[..., None]       # zero past each length
    cond = torch.randn(N, L, 256, generator=gen) * keep[..., None]
    spk = torch.randn(N, 256, generator=gen) if kind == "naive" else None
    coarse = (mel + 0.3 * torch.randn(N, L, 80, generator=gen)) * keep[..., None] if kind == "shallow" else None
    # per step: D-phase forward (t, 3 noises) then G-phase forward (t, 3 noises), pinned per sample at L = 64
    ts = [torch.randint(0, 4, (N,), generator=gen) for _ in range(2 * STEPS)]
    noises = [torch.randn(N, 1, 80, L, generator=gen) for _ in range(6 * STEPS)]
    return mel, cond, spk, coarse, ~keep, ts, noises


def _models(mg_, manifest_, stats_dir, kind):
    ms = kind == "naive"
    args, pre, mc, tr = hot_path_configs(kind, 4, multi_speaker=ms, stats_dir=stats_dir)
    G = mg_.GaussianDiffusion(args, pre, mc, tr)
    D = mg_.JCUDiscriminator(pre, mc, tr)
    load_seeded(G, manifest_, "diffusion_%s_ms%d" % (kind, ms), 32)
    load_seeded(D, manifest_, "jcu_ms%d" % ms, 42)
    with torch.no_grad():   # the fixture recipe leaves output_projection at its zero init: make the path live
        G.denoise_fn.output_projection.conv.weight.normal_(0, 0.05, generator=torch.Generator().manual_seed(3))
    return G, D, tr, mc


def _run(mg_, manifest_, stats_dir, kind, lo, hi, cut, exact, steps):
    """`steps` trainer steps on samples [lo, hi) cut to `cut` frames.  Returns the reduced gradients per update, the
    final weights, the returned losses per step and (shallow) the coarse mel's gradient."""
    G, D, tr, mc = _models(mg_, manifest_, stats_dir, kind)
    G, D = G.cuda(), D.cuda()
    mel, cond, spk, coarse, pad, ts, noises = _data(kind)
    G.t_fn = Tape([t[lo:hi].numpy() for t in ts])
    G.noise_fn = Tape([n[lo:hi].numpy() for n in noises])
    trainer = mg_.HotPathTrainer(G, D, tr, mc, exact_shards=exact)
    seen = []
    trainer.grad_hook = lambda name, bucket: seen.append((name, bucket.flat.detach().cpu().numpy().copy()))
    sl = lambda x: None if x is None else x[lo:hi, :cut].contiguous().cuda()  # noqa: E731
    leaf = None
    outs = []
    for _ in range(steps):
        if coarse is not None:
            leaf = sl(coarse).requires_grad_()
        out = trainer.step(sl(mel), sl(cond), None if spk is None else spk[lo:hi].cuda(), sl(pad), leaf)
        assert all(torch.isfinite(v).all() for v in out.values())
        outs.append({k: float(v) for k, v in out.items()})
    assert G.t_fn.i == 2 * steps and G.noise_fn.i == 6 * steps
    weights = {"G." + k: v.detach().cpu().numpy() for k, v in G.named_parameters()}
    weights.update({"D." + k: v.detach().cpu().numpy() for k, v in D.named_parameters()})
    return {"seen": seen, "weights": weights, "outs": outs,
            "coarse_grad": None if leaf is None else leaf.grad.cpu().numpy()}


def _trainer_rank(rank, world, stats_dir, kind, split, exact, steps):
    import mixgan_tts_amd as mg_
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "manifest.json")) as f:
        manifest_ = json.load(f)
    lo = sum(split[:rank])
    hi = lo + split[rank]
    cut = max(LENS[lo:hi]) if exact else L        # exact: the rank's own longest item; the guard pads to 64 by hand
    return _run(mg_, manifest_, stats_dir, kind, lo, hi, cut, exact, steps)


_SINGLE = {}


def _stats(tmp_path_factory, kind):
    e = golden("elementwise")
    return write_stats(tmp_path_factory.mktemp("stats_" + kind), e["spec_min"], e["spec_max"],
                       n_speakers=5 if kind == "naive" else 0)


def _single(mg, manifest, tmp_path_factory, kind, steps):
    """One process stepping on the whole batch (computed once per model kind and shared)."""
    if kind not in _SINGLE:
        _SINGLE[kind] = _run(mg, manifest, _stats(tmp_path_factory, kind), kind, 0, N, L, False, steps)
    return _SINGLE[kind]


def _grad_err(flat, ref):
    return float(np.abs(flat - ref).max()) / (float(np.abs(ref).max()) + 1e-30)


def _update_distance(mg, manifest, stats_dir, kind, weights, ref_w):
    G, D, _, _ = _models(mg, manifest, stats_dir, kind)
    init = {"G." + k: v.detach().numpy() for k, v in G.named_parameters()}
    init.update({"D." + k: v.detach().numpy() for k, v in D.named_parameters()})
    num = den = 0.0
    for k, w in weights.items():
        d_ref = (ref_w[k] - init[k]).astype(np.float64)
        d_got = (w - init[k]).astype(np.float64)
        num += float(((d_got - d_ref) ** 2).sum())
        den += float((d_ref ** 2).sum())
    return num, den


def _share_errors(ranks, ref, step):
    errs = {}
    for k, r in ref["outs"][step].items():
        got = sum(res["outs"][step][k] for res in ranks)
        errs[k] = (abs(got - r) / max(1.0, abs(r)), got, r)
    return errs


@pytest.mark.parametrize("split", [(2, 2), (3, 1)], ids=["2+2", "3+1"])
def test_two_ragged_ranks_equal_single_process(mg, manifest, tmp_path_factory, split):
    stats = _stats(tmp_path_factory, "naive")
    ranks = _spawn("_trainer_rank", 2, stats, "naive", split, True, STEPS)
    ref = _single(mg, manifest, tmp_path_factory, "naive", STEPS)
    assert [n for n, _ in ref["seen"]] == ["D", "G"] * STEPS
    fails = []
    for r, res in enumerate(ranks):
        assert [n for n, _ in res["seen"]] == ["D", "G"] * STEPS
        for i, ((name, flat), (_, rflat)) in enumerate(zip(res["seen"], ref["seen"])):
            tol = 2e-4 if i < 2 else 2e-3
            err = _grad_err(flat, rflat)
            print("EXACTERR split %s rank %d update %d (%s): reduced gradient %.3e (bar %.0e)" % (split, r, i, name, err, tol))
            if not err <= tol:
                fails.append(("grad", r, i, name, err))
        num, den = _update_distance(mg, manifest, stats, "naive", res["weights"], ref["weights"])
        print("EXACTERR split %s rank %d: weight update L2 %.3e" % (split, r, (num / max(den, 1e-300)) ** 0.5))
        if not (den > 0 and (num / den) ** 0.5 <= 2e-2):
            fails.append(("update", r, (num / max(den, 1e-300)) ** 0.5))
    for k in ranks[0]["weights"]:
        if not np.array_equal(ranks[0]["weights"][k], ranks[1]["weights"][k]):
            fails.append(("ranks differ", k))
    for step in range(STEPS):
        for k, (err, got, r) in _share_errors(ranks, ref, step).items():
            print("EXACTERR split %s step %d %s: shares sum %.8g, single process %.8g, err %.3e" % (split, step, k, got, r, err))
            if not err <= LOSS_T:
                fails.append(("loss", step, k, err))
    assert not fails, fails


def test_guard_mean_of_means_misses_on_these_inputs(mg, manifest, tmp_path_factory):
    """The same (2, 2) split, padded to 64 frames by hand, through the default mean exchange: the first G update must be
    off by more than ten times the bar of the exact test, or that test's inputs would not tell the two apart."""
    stats = _stats(tmp_path_factory, "naive")
    ranks = _spawn("_trainer_rank", 2, stats, "naive", (2, 2), False, 1)
    ref = _single(mg, manifest, tmp_path_factory, "naive", STEPS)
    for res in ranks:
        name, flat = res["seen"][1]
        assert name == "G" and ref["seen"][1][0] == "G"
        err = _grad_err(flat, ref["seen"][1][1])
        print("EXACTERR guard: first G update, mean of means vs single process %.3e" % err)
        assert err > 2e-3, err


def test_shallow_coarse_mel_gradient_and_postnet_share(mg, manifest, tmp_path_factory):
    """shallow: the mel L1 counts rows of the coarse mel, and postnet_loss = L1(coarse_mel, mel) is a mean over the
    padded mel of the WHOLE batch; coarse_mel is a leaf, and its gradient on each rank is the single process's rows."""
    stats = _stats(tmp_path_factory, "shallow")
    ranks = _spawn("_trainer_rank", 2, stats, "shallow", (2, 2), True, 1)
    ref = _single(mg, manifest, tmp_path_factory, "shallow", 1)
    fails = []
    lo = 0
    for r, res in enumerate(ranks):
        for i, ((name, flat), (_, rflat)) in enumerate(zip(res["seen"], ref["seen"])):
            err = _grad_err(flat, rflat)
            print("EXACTERR shallow rank %d update %d (%s): reduced gradient %.3e" % (r, i, name, err))
            if not err <= 2e-4:
                fails.append(("grad", r, i, err))
        cg = res["coarse_grad"]
        want = ref["coarse_grad"][lo:lo + cg.shape[0], :cg.shape[1]]
        assert cg.shape[1] == max(LENS[lo:lo + cg.shape[0]])
        err = float(np.abs(cg - want).max()) / float(np.abs(ref["coarse_grad"]).max())
        print("EXACTERR shallow rank %d: coarse mel gradient %.3e" % (r, err))
        if not err <= 2e-4:
            fails.append(("coarse", r, err))
        # what the single process has past this rank's cut is zero: pad frames carry no gradient
        assert not ref["coarse_grad"][lo:lo + cg.shape[0], cg.shape[1]:].any()
        lo += cg.shape[0]
    errs = _share_errors(ranks, ref, 0)
    assert "postnet_loss" in errs and errs["postnet_loss"][2] > 0
    for k, (err, got, r_) in errs.items():
        print("EXACTERR shallow %s: shares sum %.8g, single process %.8g, err %.3e" % (k, got, r_, err))
        if not err <= LOSS_T:
            fails.append(("loss", k, err))
    assert not fails, fails


def test_exact_mode_refuses_capture_and_plain_mode_refuses_a_shape(mg, manifest, tmp_path_factory):
    G, D, tr, mc = _models(mg, manifest, _stats(tmp_path_factory, "naive"), "naive")
    G, D = G.cuda(), D.cuda()
    mel, cond, spk, _, pad, _, _ = _data("naive")
    with pytest.raises(RuntimeError, match="exact_shards"):
        mg.HotPathTrainer(G, D, tr, mc, exact_shards=True).capture(mel.cuda(), cond.cuda(), spk.cuda(), pad.cuda())
    with pytest.raises(ValueError, match="exact_shards"):
        mg.HotPathTrainer(G, D, tr, mc).step(mel.cuda(), cond.cuda(), spk.cuda(), pad.cuda(), shape=mg.BatchShape(4, 64, 1))


# ------------------------------------------------------------------ the loader
def _dataset(d, pre, train):
    from mixgan_tts_amd import data as D
    g = golden("dataset")
    ids = {}
    for i, ln in enumerate(str(x) for x in g["meta_lines"]):
        ids[ln.split("|")[2]] = g["item%02d/phone_ids" % i]
    return D.Dataset("train.txt", types.SimpleNamespace(model="naive"), pre, {"multi_speaker": False}, train,
                     sort=True, drop_last=False, text_to_sequence=lambda text, cleaners: ids[text].tolist())


def _loader_rank(rank, world, d, pre, train):
    from mixgan_tts_amd import data as D
    ds = _dataset(d, pre, train)
    grp = dist.new_group(backend="gloo")          # the loader's own: nothing else runs collectives on it
    smp = D.RankShardSampler(len(ds), 5, rank=rank, world=world, seed=3)
    want = [ds.collate_fn([ds[i] for i in idxs]) for idxs in smp]
    rows = []
    for gb, wb in zip(D.PrefetchLoader(ds, smp, "cuda:0", depth=2, shape_group=grp), want):
        assert len(gb) == len(wb)
        for b, w in zip(gb, wb):
            own = int(w[13])
            mel, prior = b[11].cpu(), b[10].cpu()
            rows.append({"shape": tuple(b.shape), "max_mel_len": int(b[13]), "own": own, "items": len(w[12]),
                         "mel_frames": mel.shape[1], "prior_frames": prior.shape[2],
                         "mel_kept": bool(torch.equal(mel[:, :own], torch.from_numpy(w[11]).float())),
                         "prior_kept": bool(torch.equal(prior[:, :, :own], torch.from_numpy(w[10]).float())),
                         "padding_is_zero": not bool(mel[:, own:].any()) and not bool(prior[:, :, own:].any()),
                         "lens_kept": bool(torch.equal(b[12].cpu(), torch.from_numpy(w[12]))),
                         "others_kept": all(torch.equal(b[j].cpu(), torch.from_numpy(np.asarray(w[j])).to(b[j].dtype))
                                            for j in (3, 4, 6, 7, 14, 15, 16))})
    with pytest.raises(ValueError):
        D.PrefetchLoader(ds, smp, "cuda:0", workers=2, shape_group=grp)
    return rows


def test_loader_pads_to_the_longest_rank_and_attaches_the_shape(tree):  # noqa: F811
    g, d, pre, train, t2s = tree
    r0, r1 = _spawn("_loader_rank", 2, d, pre, train)
    assert len(r0) == len(r1) == 2                # one group of 5 items per rank: sub-batches of 4 and 1
    ragged = 0
    for a, b in zip(r0, r1):
        longest = max(a["own"], b["own"])
        ragged += a["own"] != b["own"]
        assert a["shape"] == b["shape"] == (a["items"] + b["items"], longest, 2)
        for row in (a, b):
            assert row["max_mel_len"] == row["mel_frames"] == row["prior_frames"] == longest
            assert row["mel_kept"] and row["prior_kept"] and row["padding_is_zero"] and row["lens_kept"]
            assert row["others_kept"]
    assert ragged >= 1                            # the ranks' lengths differ: something was padded


# ------------------------------------------------------------------ exact mode around a whole model
class _FrameEncoder(torch.nn.Module):
    """Stands in for the linguistic encoder: a learned frame embedding (no dropout: both calls of a step agree)."""

    def __init__(self, frames, H=256):
        super().__init__()
        self.table = torch.nn.Parameter(torch.randn(frames, H, generator=torch.Generator().manual_seed(1)))

    def forward(self, texts, src_lens, word_boundaries, src_masks, src_w_lens, src_w_masks, mel_masks, max_mel_len,
                attn_priors, p_targets, e_targets, d_targets, p_control, d_control):
        B = texts.shape[0]
        out = self.table[None, :max_mel_len].expand(B, -1, -1) * mel_masks.unsqueeze(-1)
        return (out, None, None, torch.zeros(B, 3, device=out.device), torch.zeros(B, 3, device=out.device),
                mel_masks.sum(1), mel_masks, None, None)


def _model_step(mg, manifest, stats, pair, exact):
    """One step_from_model + one evaluate_from_model on a batch of 48 and 40 frames whose whole-batch length is 56:
    exact mode gets the 48-frame batch and shape=(2, 56, 1), plain mode the same batch padded to 56 by hand."""
    B, own, Lg = 2, 48, 56
    args, pre, mc, tr = hot_path_configs("naive", 4, stats_dir=stats)
    enc = _FrameEncoder(Lg)
    model = mg.MixGANTTS(args, pre, mc, tr, linguistic_encoder=enc)
    load_seeded(model.diffusion, manifest, "diffusion_naive_ms0", 61)
    with torch.no_grad():
        model.diffusion.denoise_fn.output_projection.conv.weight.normal_(0, 0.05, generator=torch.Generator().manual_seed(3))
    D = mg.JCUDiscriminator(pre, mc, tr)
    load_seeded(D, manifest, "jcu_ms0", 62)
    model, D = model.cuda().train(), D.cuda()
    gen = torch.Generator().manual_seed(12)
    mel_lens = torch.tensor([own, own - 8])
    frames = own if exact else Lg
    mels = (torch.rand(B, Lg, 80, generator=gen) * 13.5 - 11.5) * (torch.arange(Lg)[None, :] < mel_lens[:, None]).unsqueeze(-1)
    cu = lambda a: a.cuda()  # noqa: E731
    batch = [["a", "b"], ["t"] * B, cu(torch.zeros(B, dtype=torch.long)), cu(torch.ones(B, 5, dtype=torch.long)),
             cu(torch.full((B,), 5)), 5, cu(torch.ones(B, 3, dtype=torch.long)), cu(torch.full((B,), 3)), 3, None, None,
             cu(mels[:, :frames].contiguous()), cu(mel_lens), frames, cu(torch.zeros(B, 5)), cu(torch.zeros(B, 5)),
             cu(torch.ones(B, 3, dtype=torch.long))]
    model.diffusion.t_fn = Tape([torch.tensor([3, 1]).numpy() for _ in range(4)])
    model.diffusion.noise_fn = Tape([torch.randn(B, 1, 80, Lg, generator=gen).numpy() for _ in range(12)])
    others = [p for n, p in model.named_parameters() if not n.startswith("diffusion.")]
    trainer = mg.HotPathTrainer(model.diffusion, D, tr, mc, extra_g_params=others, g_param_order=list(model.parameters()),
                                exact_shards=exact)
    seen = []
    trainer.grad_hook = lambda name, bucket: seen.append((name, bucket.flat.detach().cpu().numpy().copy()))
    asked = []

    def upstream(batch_, output, step, counts=None):
        asked.append(None if counts is None else (counts["n_items"], int(counts["words"]), int(counts["phonemes"]),
                                                  int(counts["attn_cells"]), int(counts["mel_rows"])))
        return 0.25 * (enc.table ** 2).mean()

    kw = {"shape": mg.BatchShape(B, Lg, 1)} if exact else {}
    out = trainer.log_scalars(trainer.step_from_model(model, list(batch), upstream_loss=upstream, pair=pair, **kw))
    ev = trainer.log_scalars(trainer.evaluate_from_model(model, list(batch), upstream_loss=upstream, **kw))
    assert model.diffusion.t_fn.i == 4 and model.diffusion.noise_fn.i == 12
    return out, ev, seen, asked


@pytest.mark.parametrize("pair", [False, True], ids=["unpaired", "paired"])
def test_step_from_model_pads_the_batch_and_equals_the_plain_step(mg, manifest, tmp_path_factory, pair):
    """Single process: exact mode's counts are the batch's own, so padding the 48-frame batch to the whole batch's 56
    frames inside the trainer must give the plain step on the hand-padded batch (bars of the two-rank test, step 1)."""
    stats = _stats(tmp_path_factory, "ms0")
    out, ev, seen, asked = _model_step(mg, manifest, stats, pair, True)
    ref_out, ref_ev, ref_seen, ref_asked = _model_step(mg, manifest, stats, pair, False)
    assert ref_asked == [None, None] and asked == [(2, 6, 10, 5 * 48 + 5 * 40, 88)] * 2
    assert [n for n, _ in seen] == [n for n, _ in ref_seen] == ["D", "G"]
    fails = []
    for (name, flat), (_, rflat) in zip(seen, ref_seen):
        err = _grad_err(flat, rflat)
        print("EXACTERR model pair=%s %s: gradient %.3e" % (pair, name, err))
        if not err <= 2e-4:
            fails.append((name, err))
    for label, got, ref in (("step", out, ref_out), ("eval", ev, ref_ev)):
        assert set(got) == set(ref)
        for k, r in ref.items():
            err = abs(got[k] - r) / max(1.0, abs(r))
            print("EXACTERR model pair=%s %s %s: %.8g vs %.8g, err %.3e" % (pair, label, k, got[k], r, err))
            if not err <= LOSS_T:
                fails.append((label, k, err))
    assert not fails, fails
