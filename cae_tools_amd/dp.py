"""Data-parallel training: one process per GPU, every frozen global batch sharded over the ranks.

The reference has no multi-device path (it picks ONE device: conv_ae_model.py:294-297, 312-313);
this is the build's addition.  Semantics: the global batch of a step is the union of the ranks' local batches (rank r
takes rows shard_bounds(n, world, r) of the frozen batch, so the union IS the reference's batch); the loss is the mean
over the global batch, so each rank back-propagates sum(local terms)/global_count and a SUM all-reduce yields the
global-mean gradient on every rank; Adam then runs identically everywhere (weights stay bit-identical across ranks
because they start equal and see the same reduced gradient).  BatchNorm: sync_bn=True all-reduces the sum tables so that
N ranks x batch/N reproduce the single-device batch-N step (the parity mode); sync_bn=False keeps
per-rank batch statistics (torch DDP's behaviour without SyncBatchNorm; the throughput mode).

Two engine protocols:

* native (HipEngine): the collectives live INSIDE libcae_hip (include/cae_hip.h, cae_dp_*): an RCCL communicator owned
  by the library, gradient buckets all-reduced on a second HIP stream while backward still runs, the whole step replayed
  from one hipGraph.  torch.distributed is only the rendezvous that carries the 128-byte RCCL id.  The engine exposes
  set_cursor / claim_slots / dp_train_steps / dp_eval_steps / dp_read_losses / dp_broadcast.
* half-steps (UnetEngine / VaeEngine / LinearEngine behind GradientHalfSteps, and the CPU stand-ins of the gloo
  tests): .grads and .adam_step(), the gradient all-reduce between them being torch.distributed's, and one half-step
  protocol: .forward_backward_sync(which, perm, start, size, row0, global_batch, bn_world, allreduce) /
  .eval_step_sync(which, perm, start, size, row0, global_batch, allreduce), where this rank holds rows [row0, row0 +
  size) of the global batch and allreduce sums each table the engine passes over the ranks; both return a loss slot
  that .read_losses(first, count) / .loss_slots read.  train_step with sync_bn and run_batches drive it.  train_step
  without sync_bn drives the plain .forward_backward(which, perm, start, size, global_batch) instead (per-rank
  BatchNorm, gradient scaled by size / global_batch), which is also what bench.py's host all-reduce fallback runs.
"""
import contextlib

import torch


def shard_bounds(n, world, rank):
    """contiguous split of a global batch of n samples: rank r takes rows [lo, hi) — the union over
    ranks is the reference's single-device batch"""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class DataParallel:

    def __init__(self, engine, dist, group=None, sync_bn=False, overlap="auto"):
        self.engine = engine
        self.dist = dist
        self.group = group
        self.sync_bn = sync_bn   # BatchNorm over the global batch (parity with the single-device reference)
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.native = hasattr(engine, "dp_train_steps")
        if self.native and getattr(engine, "dp_world", 0) != self.world:
            engine.dp_init(dist, group)
        # native engines: first gradient bucket on the second stream (True), both on the main stream (False), or whichever
        # HipEngine.dp_calibrate measures as faster on this communicator, decided once before the first training step
        self.overlap = overlap
        self.calibration = None
        if self.native and overlap != "auto":
            engine.dp_set_overlap(bool(overlap))

    def _calibrate(self, which, perm, start, batch, global_batch):
        """dp_calibrate is COLLECTIVE (RCCL steps + an all-reduce of the timings), so whether it runs is decided from values
        every rank shares: a global batch smaller than the world leaves some rank's shard empty, and then no rank calibrates
        (the default structure stays) rather than some entering the collective and the others not."""
        if not (self.native and self.overlap == "auto" and self.calibration is None and not self.sync_bn):
            return
        if int(global_batch) < self.world:
            self.calibration = {}
            return
        self.calibration = self.engine.dp_calibrate(self.dist, which, perm, start, batch, global_batch, False,
                                                    group=self.group)

    def _stream_ctx(self):
        stream = getattr(self.engine, "stream", None)
        return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()

    def broadcast_parameters(self, src=0):
        """make every rank start from rank `src`'s weights / running stats / Adam state"""
        if self.native:
            self.engine.dp_broadcast(src)
            return
        with self._stream_ctx():
            for name in ("params", "buffers", "exp_avg", "exp_avg_sq"):
                t = getattr(self.engine, name, None)
                if t is not None:
                    self.dist.broadcast(t, src=src, group=self.group)

    def broadcast_buffers(self, src=0):
        """BatchNorm running statistics of rank `src` to every rank: with per-rank statistics the ranks' running
        averages differ (DDP broadcasts rank 0's every forward); done before a pass that scores with them and before
        saving, so that every rank evaluates one model"""
        if self.native:
            self.engine.dp_broadcast(src, params=False, buffers=True, moments=False)
        else:
            t = getattr(self.engine, "buffers", None)
            if t is not None:
                with self._stream_ctx():
                    self.dist.broadcast(t, src=src, group=self.group)

    def set_lr(self, lr):
        """the learning rate of the next optimiser steps; every rank must pass the same value (see agree())"""
        self.engine.set_lr(lr)

    def agree(self, value):
        """rank 0's `value` (a python float) on every rank: what a schedule that listens to a loss is fed, so that the ranks'
        rates cannot part over the last bits of a reduction"""
        device = getattr(self.engine, "device", None) or self.engine.grads.device
        t = torch.tensor([float(value)], dtype=torch.float64, device=device)
        src = self.dist.get_global_rank(self.group, 0) if self.group is not None else 0
        self.dist.broadcast(t, src=src, group=self.group)
        return float(t.item())

    def global_batch(self, local_size, equal=True):
        if equal:
            return local_size * self.world
        device = getattr(self.engine, "device", None) or self.engine.grads.device
        t = torch.tensor([local_size], dtype=torch.int64, device=device)
        self.dist.all_reduce(t, group=self.group)
        return int(t.item())

    # ---- one step -----------------------------------------------------------------------------
    def train_step(self, which, perm, start, size, global_batch=None):
        """one optimiser step on this rank's shard perm[start:start+size]; returns its loss slot"""
        gb = global_batch if global_batch is not None else size * self.world
        eng = self.engine
        if self.native:
            self._calibrate(which, perm, start, size, gb)
            slot = eng.claim_slots(1)
            eng.set_cursor(start, slot)
            eng.dp_train_steps(which, perm, size, gb, self.sync_bn, 1)
            return slot
        if self.sync_bn:
            slot = eng.forward_backward_sync(
                which, perm, start, size, shard_bounds(gb, self.world, self.rank)[0], gb, self.world,
                lambda table: self.dist.all_reduce(table, op=self.dist.ReduceOp.SUM, group=self.group))
        else:
            slot = eng.forward_backward(which, perm, start, size, gb)
        with self._stream_ctx():
            self.dist.all_reduce(eng.grads, op=self.dist.ReduceOp.SUM, group=self.group)
        eng.adam_step()
        return slot

    # ---- one pass (the epoch loops of conv_ae_model.py:185-221 over sharded global batches) ------------
    def run_batches(self, which, perm, n, global_batch, train=True):
        """One pass over perm[0:n] in GLOBAL batches of `global_batch` (the last one partial, drop_last=False as in
        conv_ae_model.py:291-292); this rank runs rows shard_bounds(size, world, rank) of each.  Returns the per-batch
        mean losses over the global batches, identical on every rank."""
        if not self.native:
            return self._run_half_steps(which, perm, n, global_batch, train)
        eng = self.engine
        (full, rem) = divmod(int(n), int(global_batch))
        nb = full + (1 if rem else 0)
        first = eng.claim_slots(nb)

        def steps(batch, gb, k):
            if train:
                eng.dp_train_steps(which, perm, batch, gb, self.sync_bn, k)
            else:
                eng.dp_eval_steps(which, perm, batch, gb, k)

        if full:
            (lo, hi) = shard_bounds(global_batch, self.world, self.rank)
            if train:
                self._calibrate(which, perm, lo, hi - lo, global_batch)
            eng.set_cursor(lo, first)      # the device cursor then moves one global batch per step
            left = full
            per_graph = getattr(eng, "STEPS_PER_GRAPH", 64)
            while left >= per_graph:       # three graph shapes per batch size at most: K steps, the remainder, 1 step
                steps(hi - lo, global_batch, per_graph)
                left -= per_graph
            if left:
                steps(hi - lo, global_batch, left)
        if rem:
            (lo, hi) = shard_bounds(rem, self.world, self.rank)
            eng.set_cursor(full * global_batch + lo, first + full)
            steps(hi - lo, rem, 1)         # hi == lo (an empty shard) still takes part in the collectives
        return eng.dp_read_losses(first, nb)

    def _run_half_steps(self, which, perm, n, global_batch, train):
        """run_batches over the sync half-steps: every shard (an empty one included) goes through the engine's global-batch
        entry points, whose tables this rank's all-reduce sums, so the losses are the global batch's; training then
        all-reduces the gradient and steps the optimiser.  sync_bn=False keeps BatchNorm statistics per rank (bn_world 0);
        the loss denominators and the dropout masks are the global batch's either way."""
        eng = self.engine

        def allreduce(t):
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)

        out, pending = [], []
        for b0 in range(0, int(n), int(global_batch)):
            gb = min(int(global_batch), int(n) - b0)
            (lo, hi) = shard_bounds(gb, self.world, self.rank)
            if train:
                slot = eng.forward_backward_sync(which, perm, b0 + lo, hi - lo, lo, gb, self.world if self.sync_bn else 0,
                                                 allreduce)
                with self._stream_ctx():
                    allreduce(eng.grads)
                eng.adam_step()
            else:
                slot = eng.eval_step_sync(which, perm, b0 + lo, hi - lo, lo, gb, allreduce)
            pending.append(slot)
            if slot == eng.loss_slots - 1:     # the slots wrap next: read what they hold
                out.extend(eng.read_losses(pending[0], len(pending)))
                pending = []
        if pending:
            out.extend(eng.read_losses(pending[0], len(pending)))
        return out


class GradientHalfSteps:
    """UnetEngine / VaeEngine / LinearEngine behind the half-step interface DataParallel drives: a persistent flat gradient
    buffer, the half-step protocol into it - forward_backward_sync / eval_step_sync (UNET, VAE), the single-device
    arithmetic at the global batch: global loss denominators, random masks / noise of the global rows and, with SyncBN,
    BatchNorm statistics over the global batch - and the optimiser half-step (*_apply_gradients) after the all-reduce.
    The plain forward_backward (DataParallel.train_step without sync_bn, bench.py's fallback) applies the local/global
    weight in the kernel that narrows the fp64 accumulator (grad_scale of *_forward_backward); its BatchNorm statistics
    stay per rank and the UNET's masked MSE divides by the LOCAL mask count (with unequal mask coverage the reduced
    gradient weights shards by sample count, not by valid-pixel count)."""

    def __init__(self, engine):
        self.engine = engine
        self.grads = torch.zeros(engine.n_param, dtype=torch.float32, device=engine.device)
        self.stream = engine.stream
        (self.params, self.exp_avg, self.exp_avg_sq) = (engine.params, engine.exp_avg, engine.exp_avg_sq)
        self.buffers = getattr(engine, "buffers", None)
        self._slot = 0

    @property
    def loss_slots(self):
        return self.engine.loss_slots

    def _next_slot(self):
        slot = self._slot
        self._slot = (slot + 1) % self.engine.loss_slots
        return slot

    def forward_backward(self, which, perm, start, size, global_batch):
        slot = self._next_slot()
        self.engine.forward_backward(which, perm, start, size, slot=slot, global_batch=global_batch, out=self.grads)
        return slot

    def forward_backward_sync(self, which, perm, start, size, row0, global_batch, bn_world, allreduce):
        slot = self._next_slot()
        self.engine.forward_backward_sync(which, perm, start, size, row0, global_batch, bn_world, allreduce, out=self.grads,
                                          slot=slot)
        return slot

    def eval_step_sync(self, which, perm, start, size, row0, global_batch, allreduce):
        slot = self._next_slot()
        self.engine.eval_step_sync(which, perm, start, size, row0, global_batch, allreduce, slot=slot)
        return slot

    def read_losses(self, first, count):
        return self.engine.read_losses(first, count)

    def adam_step(self):
        self.engine.apply_gradients(self.grads)

    def set_lr(self, lr):
        self.engine.set_lr(lr)


def data_parallel(engine, dist, sync_bn=False):
    """the DataParallel that drives `engine`: a native engine (HipEngine) as it is, any other behind GradientHalfSteps"""
    native = hasattr(engine, "dp_train_steps")
    return DataParallel(engine if native else GradientHalfSteps(engine), dist, sync_bn=sync_bn)


# ---- process-group plumbing for the model classes and CLIs ------------------------------------------

def env_world():
    """(rank, local_rank, world) from torch.distributed.run's environment; (0, 0, 1) outside it"""
    import os
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")))


def select_device():
    """Make LOCAL_RANK's GPU the current device of a rank of a torch.distributed.run launch.  Every entry point that may
    run in a rank (train / apply / evaluate, the CLIs) calls this BEFORE its first CUDA allocation: DSDataset and the
    engines allocate on torch.cuda.current_device(), which is 0 in every rank until somebody says otherwise, and an engine
    on GPU r must not be handed GPU-0 pointers.  No-op outside a launch and without a GPU.  Returns the local rank."""
    (rank, local_rank, world) = env_world()
    if world > 1 and torch.cuda.is_available() and torch.cuda.current_device() != local_rank:
        torch.cuda.set_device(local_rank)
    return local_rank


def ensure_process_group():
    """torch.distributed handle when this process is one rank of a torch.distributed.run launch (initialising the
    default group on first use: RCCL when a GPU is present), else None.  The GPU of a rank is LOCAL_RANK."""
    import os
    import torch.distributed as dist
    select_device()
    if dist.is_available() and dist.is_initialized():
        # CAE_FORCE_DP=1: take the data-parallel code path on a one-rank group too (rehearsal on a one-GPU box and in tests)
        return dist if dist.get_world_size() > 1 or os.environ.get("CAE_FORCE_DP") == "1" else None
    (rank, local_rank, world) = env_world()
    if world <= 1:
        return None
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29500")
    if torch.cuda.is_available():
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist
