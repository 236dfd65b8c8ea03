"""Batch-sharded data parallelism for the training step: one process per GPU, RCCL over xGMI
(`torch.distributed` backend "nccl" is RCCL on ROCm), gloo on CPU for tests.

The reference has no multi-device path (its nn.DataParallel is pinned to one GPU, SURVEY.md
section 5).  The path shards over the batch with no data-path collective; the only exchange is
one SUM all-reduce per optimizer of the flattened gradients (G: 92 MB fp32, D: 7.5 MB), divided by
the world size, BEFORE `clip_grad_norm_` (train.py:81 clips the gradient the optimizer sees).
A single flat bucket per optimizer keeps the collective large (xGMI rings are per-link bound;
fewer, larger messages), and lets the D all-reduce overlap the start of the G phase on a side
stream when `async_op=True`.
"""
import collections

import torch
import torch.distributed as dist


def is_distributed():
    return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1


class GradBucket:
    """Flat fp32 buffer holding the gradients of a parameter list, so the all-reduce is one collective with no
    packing step.  `.grad` of every parameter is (re-)pointed at its slice: producers that know the layout write
    there directly (Denoiser.bind_grad_buffer: the backward's layer-major gradient arrays ARE slices of `flat`, and
    autograd adopts them as `.grad` without a copy), every other gradient is copied in by `gather()` in one
    multi-tensor launch.  `order` (optional) lists parameters in the order they should be laid out; the rest follow."""

    def __init__(self, params, order=None):
        wanted = [p for p in params if p.requires_grad]
        ids = {id(p) for p in wanted}
        first = [p for p in (order or []) if id(p) in ids]
        seen = {id(p) for p in first}
        self.params = first + [p for p in wanted if id(p) not in seen]
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device if self.params else torch.device("cpu")
        self.flat = torch.zeros(n, device=dev, dtype=torch.float32)
        self.views = []
        self.offsets = {}
        off = 0
        for p in self.params:
            self.views.append(self.flat[off:off + p.numel()].view_as(p))
            self.offsets[id(p)] = off
            off += p.numel()

    def gather(self):
        """Make `flat` hold the current gradients and every `.grad` alias its slice.  A parameter without a gradient
        on this rank (conditionally unused) contributes zeros AND gets `.grad` set, so that after the all-reduce every
        rank's optimizer steps it with the same averaged gradient (ranks must not diverge)."""
        src, dst = [], []
        for p, v in zip(self.params, self.views):
            if p.grad is None:
                v.zero_()
                p.grad = v
            elif p.grad.data_ptr() != v.data_ptr():
                src.append(p.grad)
                dst.append(v)
                p.grad = v
        if dst:
            torch._foreach_copy_(dst, src)
        return self.flat

    # ------------------------------------------------------------------ exchange
    # One SUM all-reduce per optimizer step, divided by the world size -- optionally in pieces: a producer that knows
    # a slice of `flat` is final before the rest (the denoiser's backward finishes its k=3 weight gradients, a third
    # of the G bucket, 0.6 ms before its last kernel) hands it to all_reduce_chunk_async, which puts the collective
    # behind an event on a side stream so that it runs next to the remaining backward kernels; all_reduce_mean then
    # reduces whatever is left and waits for the pieces.
    _pending = ()
    _side = None
    stub = False          # measurement only (bench.py --workload train): skip the collectives, keep everything else
    always_exchange = False   # run the collectives on a world of one too (proves the RCCL path; tests, bench)

    def exchanging(self):
        return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or self.always_exchange)

    def all_reduce_chunk_async(self, lo, hi, ready_event=None, group=None):
        """Start the SUM all-reduce of flat[lo:hi] now.  ready_event (torch.cuda.Event recorded on the producing
        stream) marks the point after which the slice is final; the collective waits for it instead of for everything
        queued on the current stream.  No-op (returns False) on one process or on CPU tensors."""
        if not self.exchanging() or not self.flat.is_cuda or hi <= lo:
            return False
        for (_, plo, phi) in self._pending:
            if lo < phi and plo < hi:
                raise RuntimeError("GradBucket: overlapping chunks in flight")
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.flat.device)
        cur = torch.cuda.current_stream(self.flat.device)
        if ready_event is not None:
            self._side.wait_event(ready_event)
        else:
            self._side.wait_stream(cur)
        work = None
        if not self.stub:
            with torch.cuda.stream(self._side):      # c10d orders the collective behind the CURRENT stream: the side one
                work = dist.all_reduce(self.flat[lo:hi], op=dist.ReduceOp.SUM, group=group, async_op=True)
        self._pending = tuple(self._pending) + ((work, lo, hi),)
        return True

    def all_reduce_sum(self, group=None, async_op=False):
        """all_reduce_mean without the division: the exchange of exact-shard training, where every rank's loss is
        already divided by the denominators of the whole batch and the SUM of the gradients is the single-process
        gradient (HotPathTrainer(exact_shards=True))."""
        return self.all_reduce_mean(group, async_op, mean=False)

    def all_reduce_mean(self, group=None, async_op=False, mean=True):
        """SUM all-reduce of the flat gradient (the parts not already in flight), then divide by the world size
        (mean=False: leave the sum)."""
        self.gather()
        if not self.exchanging():
            return None
        world = dist.get_world_size(group) if mean else 1
        pending, self._pending = self._pending, ()
        if pending and self.flat.is_cuda:
            # what the chunks did not cover, in as few collectives as possible
            cuts, at = [], 0
            for (_, lo, hi) in sorted(pending, key=lambda c: c[1]):
                if lo > at:
                    cuts.append((at, lo))
                at = max(at, hi)
            if at < self.flat.numel():
                cuts.append((at, self.flat.numel()))
            works = [w for (w, _, _) in pending if w is not None]
            if not self.stub:
                works += [dist.all_reduce(self.flat[lo:hi], op=dist.ReduceOp.SUM, group=group, async_op=True)
                          for (lo, hi) in cuts]
            for w in works:
                w.wait()                             # stream-level wait on the GPU, no host block
            if mean:
                self.flat.div_(world)
            return None
        if self.stub:
            return None
        work = dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=group, async_op=async_op)
        if async_op:
            return _Pending(work, self.flat, world)
        if mean:
            self.flat.div_(world)
        return None


class _Pending:
    def __init__(self, work, flat, world):
        self.work, self.flat, self.world = work, flat, world

    def wait(self):
        self.work.wait()
        if self.world != 1:
            self.flat.div_(self.world)


def shard_batch(n_items, rank=None, world=None):
    """Contiguous shard [lo, hi) of a batch of n_items for this rank (inference: no collective)."""
    if rank is None:
        rank = dist.get_rank() if is_distributed() else 0
    if world is None:
        world = dist.get_world_size() if is_distributed() else 1
    per = (n_items + world - 1) // world
    lo = min(n_items, rank * per)
    return lo, min(n_items, lo + per)


# ------------------------------------------------------------------ exact steps on ragged shards
# A term of the whole-batch loss is w_k * (sum over ranks of S_k,r) / D_k with D_k a count over the WHOLE batch.  A rank
# that divides its numerators by the global D_k holds a share of the loss; the shares add up to the single-process loss
# and the SUM of the gradients (GradBucket.all_reduce_sum) is the single-process gradient, for any split of the batch.
# What the ranks have to agree on: the number of items and the padded length (host integers, known before the step),
# and the data-dependent counts (device integers, exchanged while the D phase runs).
BatchShape = collections.namedtuple("BatchShape", "n_total max_len world")


def _collective_device(group=None):
    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")


def exchange_batch_shapes(pairs, group=None):
    """[(n_items, length), ...] of this rank, the same number of pairs on every rank -> [BatchShape, ...]: the item
    counts summed and the lengths maximised over the ranks, all in ONE collective (an all-gather of 2 * len(pairs)
    integers), returned as host integers -- the caller waits for the collective."""
    pairs = [(int(n), int(length)) for n, length in pairs]
    if not is_distributed():
        return [BatchShape(n, length, 1) for n, length in pairs]
    world = dist.get_world_size(group)
    mine = torch.tensor(pairs, dtype=torch.int64, device=_collective_device(group)).reshape(-1)
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine, group=group)
    table = torch.stack(every).cpu().reshape(world, len(pairs), 2)
    return [BatchShape(int(table[:, k, 0].sum()), int(table[:, k, 1].max()), world) for k in range(len(pairs))]


def exchange_batch_shape(n_items, length, group=None):
    """BatchShape(n_total, max_len, world) of one step: this rank's item count and padded length, SUM / MAX over the
    ranks in one small collective; its arguments on a single process."""
    return exchange_batch_shapes([(n_items, length)], group)[0]


class ShardCounts:
    """The data-dependent counts of one step as ONE int64 device vector -- counted mel rows, valid word positions,
    valid phoneme positions, sum of ilen * olen for guided attention -- integers, so that their SUM all-reduce is exact
    (16 ranks x 16 x 4000 x 80 is past 2^24: they become fp32 once, after the exchange).  `all_reduce_async` puts the
    collective behind an event on a side stream (the hand-off of GradBucket.all_reduce_chunk_async), `wait` makes the
    current stream wait for it right before the first term that divides by a count; nothing is read on the host.
    `n_items` is the host-known item count of the whole batch (BatchShape.n_total)."""

    FIELDS = ("mel_rows", "words", "phonemes", "attn_cells")
    always_exchange = False
    _side = {}

    def __init__(self, device, n_items=None):
        self.vec = torch.zeros(len(self.FIELDS), dtype=torch.int64, device=device)
        self.n_items = n_items
        self._work = self._done = None
        self._started = False

    def slot(self, name):
        """The one-element view a producer writes its local count into (before all_reduce_async)."""
        k = self.FIELDS.index(name)
        return self.vec[k:k + 1]

    def put(self, name, value):
        self.slot(name).copy_(torch.as_tensor(value).reshape(1))

    def all_reduce_async(self, group=None):
        """Start the SUM all-reduce of the vector; no-op on a single process.  Once per step."""
        if self._started:
            raise RuntimeError("ShardCounts: the counts were exchanged already")
        self._started = True
        if not (dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or self.always_exchange)):
            return False
        if not self.vec.is_cuda:
            self._work = dist.all_reduce(self.vec, op=dist.ReduceOp.SUM, group=group, async_op=True)
            return True
        dev = self.vec.device
        if dev not in ShardCounts._side:
            ShardCounts._side[dev] = torch.cuda.Stream(device=dev)
        side = ShardCounts._side[dev]
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        side.wait_event(ready)
        with torch.cuda.stream(side):          # c10d orders the collective behind the CURRENT stream: the side one
            self._work = dist.all_reduce(self.vec, op=dist.ReduceOp.SUM, group=group, async_op=True)
            self._work.wait()                  # stream-level: the side stream waits, the host does not
            self._done = torch.cuda.Event()
            self._done.record(side)
        self.vec.record_stream(side)
        return True

    def wait(self):
        if self._done is not None:
            torch.cuda.current_stream(self.vec.device).wait_event(self._done)
            self._done = self._work = None
        elif self._work is not None:
            self._work.wait()
            self._work = None

    def __getitem__(self, name):
        """The global count: `n_items` as a host integer, the others as 0-dim int64 device tensors (waits first)."""
        if name == "n_items":
            if self.n_items is None:
                raise KeyError("ShardCounts: n_items was not given")
            return self.n_items
        if not self._started:
            raise RuntimeError("ShardCounts: read before all_reduce_async -- these would be one rank's counts")
        self.wait()
        return self.vec[self.FIELDS.index(name)]
