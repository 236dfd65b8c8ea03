"""Exact multi-rank steps on ragged shards, the parts that need no GPU: the new exports, the shape exchange and the SUM
gradient exchange on gloo with two processes, the identity itself on a toy model in float64 (each rank divides its
masked sum by the WHOLE batch's count and the gradients are summed: the single-process gradient; the mean of per-rank
masked means is not), and LinguisticEncoderLoss.terms(counts=...) whose shares add up to the terms on the whole batch."""
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import ROOT

TIMEOUT = 120
D = 6
LENS = ([7, 3], [2])          # rank 0 holds two items, rank 1 one: unequal item counts AND lengths


def test_exports_are_in_the_header_and_the_binding():
    import mixgan_tts_amd as mg
    from mixgan_tts_amd import _lib
    header = open(os.path.join(ROOT, "include", "mixgan_hip.h")).read()
    for name in ("mg_multi_loss_fwd_den", "mg_multi_loss_bwd_den", "mg_mel_count_rows"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.EXPORTS
    assert callable(mg.exchange_batch_shape) and callable(mg.data.pad_batch_to) and callable(mg.losses.mel_count_rows)
    assert mg.BatchShape(3, 5, 2)._fields == ("n_total", "max_len", "world")
    assert mg.ShardCounts.FIELDS == ("mel_rows", "words", "phonemes", "attn_cells")
    assert callable(mg.GradBucket.all_reduce_sum)
    import inspect
    assert inspect.signature(mg.HotPathTrainer.__init__).parameters["exact_shards"].default is False
    assert inspect.signature(mg.data.PrefetchLoader.__init__).parameters["shape_group"].default is None
    assert "counts" in inspect.signature(mg.LinguisticEncoderLoss.terms).parameters


def test_single_process_shape_is_its_arguments():
    import mixgan_tts_amd as mg
    assert mg.exchange_batch_shape(5, 77) == mg.BatchShape(5, 77, 1)
    c = mg.ShardCounts("cpu", n_items=5)
    c.put("words", torch.tensor(11))
    with pytest.raises(RuntimeError):
        c["words"]                         # not exchanged yet: would be one rank's count
    assert c.all_reduce_async() is False   # nothing to exchange on one process
    assert int(c["words"]) == 11 and c["n_items"] == 5 and c["words"].dtype == torch.int64


def test_pad_batch_to_pads_the_mel_axis_only():
    import numpy as np
    import mixgan_tts_amd as mg
    b = [None] * 17
    b[10] = np.ones((2, 4, 5), dtype=np.float32)
    b[11] = np.ones((2, 5, 3), dtype=np.float32)
    b[12], b[13] = np.array([5, 2]), 5
    b[14] = np.ones((2, 4), dtype=np.float32)
    out = mg.data.pad_batch_to(tuple(b), 8)
    assert out[10].shape == (2, 4, 8) and out[11].shape == (2, 8, 3) and out[13] == 8 and out[14].shape == (2, 4)
    assert (out[10][:, :, 5:] == 0).all() and (out[11][:, 5:] == 0).all() and (out[11][:, :5] == 1).all()
    assert (out[12] == b[12]).all() and b[11].shape == (2, 5, 3)
    t = [torch.from_numpy(x) if isinstance(x, np.ndarray) else x for x in b]
    assert mg.data.pad_batch_to(t, 8, in_place=True) is t and t[11].shape == (2, 8, 3)
    with pytest.raises(ValueError):
        mg.data.pad_batch_to(t, 7)


# ------------------------------------------------------------------ two processes on gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _toy_data():
    gen = torch.Generator().manual_seed(5)
    w0 = torch.randn(D, generator=gen, dtype=torch.float64)
    items = [[(torch.randn(n, D, generator=gen, dtype=torch.float64), torch.randn(n, generator=gen, dtype=torch.float64))
              for n in lens] for lens in LENS]
    return w0, items


def _masked_sum(w, items):
    """Sum of squared errors over the valid frames of a padded batch, and their number."""
    L = max(x.shape[0] for x, _ in items)
    xs = torch.stack([torch.nn.functional.pad(x, (0, 0, 0, L - x.shape[0])) for x, _ in items])
    ys = torch.stack([torch.nn.functional.pad(y, (0, L - y.shape[0])) for _, y in items])
    mask = torch.arange(L)[None, :] < torch.tensor([x.shape[0] for x, _ in items])[:, None]
    return ((xs @ w - ys).pow(2) * mask).sum(), int(mask.sum())


def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        try:
            import mixgan_tts_amd as mg
            res = {}
            lens = LENS[rank]
            res["shape"] = tuple(mg.exchange_batch_shape(len(lens), max(lens)))
            res["shapes"] = [tuple(s) for s in mg.distributed.exchange_batch_shapes([(1, 10 + rank), (2 + rank, 4)])]
            # GradBucket.all_reduce_sum / all_reduce_mean on whole-number gradients (exact in fp32)
            p = torch.nn.Parameter(torch.zeros(4))
            bucket = mg.GradBucket([p])
            p.grad = torch.full((4,), float(rank + 1))
            bucket.all_reduce_sum()
            res["sum"] = bucket.flat.tolist()
            p.grad = torch.full((4,), float(rank + 1))
            bucket.all_reduce_mean()
            res["mean"] = bucket.flat.tolist()
            # the toy model: masked mean of squared errors, ragged
            w0, items = _toy_data()
            w = w0.clone().requires_grad_(True)
            s, n = _masked_sum(w, items[rank])
            counts = mg.ShardCounts("cpu", n_items=sum(len(x) for x in LENS))
            counts.put("mel_rows", torch.tensor(n))
            counts.all_reduce_async()
            share = s / counts["mel_rows"]                      # exact mode: the WHOLE batch's count
            (g_exact,) = torch.autograd.grad(share, w, retain_graph=True)
            dist.all_reduce(g_exact, op=dist.ReduceOp.SUM)      # ... and a SUM
            (g_mean,) = torch.autograd.grad(s / n, w)           # the mean path: own count, averaged gradients
            dist.all_reduce(g_mean, op=dist.ReduceOp.SUM)
            g_mean /= world
            share = share.detach().clone()
            dist.all_reduce(share, op=dist.ReduceOp.SUM)
            res.update(count=int(counts["mel_rows"]), g_exact=g_exact.numpy(), g_mean=g_mean.numpy(), loss=float(share))
            q.put((rank, "ok", res))
        finally:
            dist.destroy_process_group()
    except Exception as exc:      # report instead of leaving the parent to wait
        q.put((rank, "error", repr(exc)))
        raise


@pytest.fixture(scope="module")
def two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted([q.get(timeout=TIMEOUT) for _ in range(2)], key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(TIMEOUT if p.exitcode is None and q.empty() else 10)
            if p.is_alive():
                p.kill()
    for rank, status, res in got:
        assert status == "ok", (rank, res)
    return [res for _, _, res in got]


def test_shape_exchange_on_two_ranks(two_ranks):
    for res in two_ranks:
        assert res["shape"] == (3, 7, 2)
        assert res["shapes"] == [(2, 11, 2), (5, 4, 2)]


def test_all_reduce_sum_does_not_divide(two_ranks):
    for res in two_ranks:
        assert res["sum"] == [3.0] * 4 and res["mean"] == [1.5] * 4


def test_toy_model_exact_gradients_equal_single_process(two_ranks):
    w0, items = _toy_data()
    w = w0.clone().requires_grad_(True)
    s, n = _masked_sum(w, items[0] + items[1])
    assert n == 12
    loss = s / n
    (ref,) = torch.autograd.grad(loss, w)
    scale = float(ref.abs().max())
    for res in two_ranks:
        assert res["count"] == n
        assert abs(res["loss"] - float(loss.detach())) <= 1e-12 * max(1.0, abs(float(loss.detach())))
        assert float((torch.from_numpy(res["g_exact"]) - ref).abs().max()) <= 1e-12 * scale
        # the mean of per-rank masked means weights rank 1's two frames like rank 0's ten
        assert float((torch.from_numpy(res["g_mean"]) - ref).abs().max()) > 1e-3 * scale


# ------------------------------------------------------------------ LinguisticEncoderLoss.terms(counts=...)
def _loss_configs(helper):
    pre = {"preprocessing": {"pitch": {"feature": "phoneme_level"}, "energy": {"feature": "phoneme_level"}}}
    tr = {"loss": {"lambda_d": 1.0, "lambda_p": 0.7, "lambda_e": 1.3}, "step": {"ctc_step": 10},
          "aligner": {"helper_type": helper, "guided_sigma": 0.4, "guided_lambda": 1.0, "guided_weight": 1.5,
                      "ctc_weight_start": 2.0, "ctc_weight_end": 0.5}}
    return pre, {}, tr


def _synthetic(rows, src_lens, w_lens, mel_lens, cut):
    """Outputs and batch of the items `rows` of a five-item synthetic batch.  cut: the 1-D masked slots are cut to
    these rows' own maximum length (what a rank would hold); the alignment tensors keep the whole batch's shape."""
    gen = torch.Generator().manual_seed(9)
    N, Ts, Tw, To = len(src_lens), max(src_lens), max(w_lens), max(mel_lens)
    r = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)  # noqa: E731
    p, e, logd, pt, et = r(N, Ts), r(N, Ts), r(N, Tw), r(N, Ts), r(N, Ts)
    dur = torch.randint(0, 9, (N, Tw), generator=gen)
    atts = [torch.softmax(r(N, To, Ts), -1) for _ in range(2)]
    logps = [r(N, 1, To, Ts) for _ in range(2)]
    sl, wl, ml = (torch.tensor(v)[rows] for v in (src_lens, w_lens, mel_lens))
    ts, tw = (int(sl.max()), int(wl.max())) if cut else (Ts, Tw)
    src_mask = torch.arange(ts)[None, :] < sl[:, None]
    w_mask = torch.arange(tw)[None, :] < wl[:, None]
    out = [None, None, None, None, p[rows, :ts], e[rows, :ts], logd[rows, :tw], dur[rows, :tw], src_mask, None, sl, ml,
           (None, [a[rows] for a in atts]), [lp[rows] for lp in logps], w_mask, None]
    batch = [None] * 17
    batch[14], batch[15] = pt[rows, :ts], et[rows, :ts]
    return batch, out


@pytest.mark.parametrize("helper", ["dga", "ctc"])
def test_encoder_loss_shares_add_up_to_the_whole_batch(helper):
    import mixgan_tts_amd as mg
    src_lens, w_lens, mel_lens = [9, 4, 6, 2, 7], [5, 2, 3, 1, 4], [30, 11, 17, 12, 23]
    loss = mg.LinguisticEncoderLoss(*_loss_configs(helper))
    whole = loss.terms(*_synthetic(list(range(5)), src_lens, w_lens, mel_lens, cut=False), 1)
    counts = {"n_items": 5, "words": sum(w_lens), "phonemes": sum(src_lens),
              "attn_cells": sum(a * b for a, b in zip(src_lens, mel_lens))}
    shards = [[0, 1, 2], [3, 4]]          # ragged: 3 + 2 items, every length vector differs
    local = [mg.LinguisticEncoderLoss.local_counts(_synthetic(rows, src_lens, w_lens, mel_lens, cut=True)[1])
             for rows in shards]
    for k in ("words", "phonemes", "attn_cells"):
        assert sum(int(c[k]) for c in local) == counts[k]
    shares = [loss.terms(*_synthetic(rows, src_lens, w_lens, mel_lens, cut=True), 1, counts=counts) for rows in shards]
    assert whole["total"].dtype == torch.float64
    for k, ref in whole.items():
        got = sum(float(s[k]) for s in shares)
        assert abs(got - float(ref)) <= 1e-12 * max(1.0, abs(float(ref))), (k, got, float(ref))
    # ... and they are shares, not the shards' own means
    own = [loss.terms(*_synthetic(rows, src_lens, w_lens, mel_lens, cut=True), 1) for rows in shards]
    assert abs(sum(float(s["total"]) for s in own) / 2 - float(whole["total"])) > 1e-6
