"""DataParallel.run_batches over half-step engines (the UNET's global-batch entry points behind GradientHalfSteps) on CPU:
two gloo ranks drive a stand-in engine with the same members - forward_backward_sync / eval_step_sync returning a loss
slot, the all-reduce callback on its tables, grads / adam_step, read_losses / loss_slots - through partial and empty
shards, and must report the global batches' losses on both ranks, in the order of the tables, as one process computes
them."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N, GLOBAL_BATCH, LR = 7, 3, 0.05      # global batches 3, 3, 1: the last one leaves rank 1 an empty shard


def _data():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(N, generator=g, dtype=torch.float64)
    return x, 3.0 * x + 0.1 * torch.rand(N, generator=g, dtype=torch.float64)


class ShardEngine:
    """y = w x with a squared-error loss: per shard a 'BatchNorm' table {sum x, sum x^2} (summed over the ranks when
    bn_world > 0) and a loss table {sum squared error, rows}; the loss slot holds (global mse, mean of x the table saw)"""

    loss_slots = 4      # small, so that a pass wraps the slots

    def __init__(self):
        (self.x, self.t) = _data()
        self.w = torch.zeros(1, dtype=torch.float64)
        self.grads = torch.zeros(1, dtype=torch.float64)
        self.slots = [None] * self.loss_slots
        self.next_slot = 0
        self.calls = []

    def _slot(self):
        s = self.next_slot
        self.next_slot = (s + 1) % self.loss_slots
        return s

    def _step(self, perm, start, size, row0, global_batch, bn_world, allreduce, train):
        idx = perm[start:start + size]
        (x, t) = (self.x[idx], self.t[idx])
        self.calls.append(("shard", int(start), int(size), int(row0), int(global_batch)))
        bn = torch.stack([x.sum(), (x * x).sum()])
        if bn_world:
            allreduce(bn)
            self.calls.append(("bn", 2))
        err = self.w * x - t
        loss = torch.stack([(err * err).sum(), torch.tensor(float(size), dtype=torch.float64)])
        allreduce(loss)
        self.calls.append(("loss", 2))
        assert loss[1].item() == global_batch
        slot = self._slot()
        self.slots[slot] = (loss[0].item() / global_batch, bn[0].item() / global_batch if bn_world else 0.0)
        if train:
            self.grads.copy_((2 * err * x).sum().reshape(1) / global_batch)
        return slot

    def forward_backward_sync(self, which, perm, start, size, row0, global_batch, bn_world, allreduce):
        return self._step(perm, start, size, row0, global_batch, bn_world, allreduce, True)

    def eval_step_sync(self, which, perm, start, size, row0, global_batch, allreduce):
        return self._step(perm, start, size, row0, global_batch, 0, allreduce, False)

    def adam_step(self):
        self.w -= LR * self.grads

    def read_losses(self, first, count):
        return [self.slots[(first + i) % self.loss_slots] for i in range(count)]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    from cae_tools_amd.dp import DataParallel, shard_bounds
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {}
    perm = torch.tensor([4, 0, 6, 2, 5, 1, 3])
    for sync_bn in (True, False):
        eng = ShardEngine()
        par = DataParallel(eng, dist, sync_bn=sync_bn)
        assert not par.native
        train = [par.run_batches(0, perm, N, GLOBAL_BATCH, train=True) for _ in range(2)]
        test = par.run_batches(1, perm, N, GLOBAL_BATCH, train=False)
        res[sync_bn] = {"train": train, "test": test, "w": eng.w.item(), "calls": eng.calls}
        if sync_bn:   # one train_step on this rank's rows of the first global batch
            eng = ShardEngine()
            (lo, hi) = shard_bounds(GLOBAL_BATCH, world, rank)
            slot = DataParallel(eng, dist, sync_bn=True).train_step(0, perm, lo, hi - lo, GLOBAL_BATCH)
            res["train_step"] = {"loss": eng.read_losses(slot, 1)[0][0], "w": eng.w.item(), "shard": eng.calls[0],
                                 "want": ("shard", lo, hi - lo, lo, GLOBAL_BATCH)}
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _single_process():
    """the same passes on one device: SGD over the global batches of perm"""
    (x, t) = _data()
    perm = torch.tensor([4, 0, 6, 2, 5, 1, 3])
    w = 0.0
    train, ws = [], []
    for _ in range(2):
        losses = []
        for b0 in range(0, N, GLOBAL_BATCH):
            idx = perm[b0:b0 + GLOBAL_BATCH]
            err = w * x[idx] - t[idx]
            losses.append(((err * err).sum() / len(idx)).item())
            w -= LR * ((2 * err * x[idx]).sum() / len(idx)).item()
            ws.append(w)
        train.append(losses)
    test = []
    for b0 in range(0, N, GLOBAL_BATCH):
        idx = perm[b0:b0 + GLOBAL_BATCH]
        err = w * x[idx] - t[idx]
        test.append(((err * err).sum() / len(idx)).item())
    return train, test, w, ws[0]


def test_half_step_passes_over_two_ranks(tmp_path):
    from cae_tools_amd.dp import shard_bounds
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    ranks = [torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(world)]
    (train_ref, test_ref, w_ref, w1_ref) = _single_process()
    for sync_bn in (True, False):
        (a, b) = (ranks[0][sync_bn], ranks[1][sync_bn])
        # per-batch losses identical on both ranks (sync_bn: with the global batch's statistics too) ...
        assert a["train"] == b["train"] and a["test"] == b["test"] and a["w"] == b["w"]
        # ... and the global batches' losses one process computes
        for (got, want) in zip(a["train"], train_ref):
            np.testing.assert_allclose([l[0] for l in got], want, rtol=1e-12)
        np.testing.assert_allclose([l[0] for l in a["test"]], test_ref, rtol=1e-12)
        assert abs(a["w"] - w_ref) <= 1e-12
        # every rank, an empty shard included, passed its tables in the same order: per training step the BatchNorm
        # table (sync_bn only) then the loss table; per eval step the loss table
        for r in range(world):
            calls = ranks[r][sync_bn]["calls"]
            shards = [c for c in calls if c[0] == "shard"]
            want_shards = []
            for _ in range(3):
                for b0 in range(0, N, GLOBAL_BATCH):
                    gb = min(GLOBAL_BATCH, N - b0)
                    (lo, hi) = shard_bounds(gb, world, r)
                    want_shards.append(("shard", b0 + lo, hi - lo, lo, gb))
            assert shards == want_shards
            per_train = [("bn", 2), ("loss", 2)] if sync_bn else [("loss", 2)]
            tables = [c for c in calls if c[0] != "shard"]
            assert tables == per_train * 6 + [("loss", 2)] * 3
        assert [s[2] for s in ranks[1][sync_bn]["calls"] if s[0] == "shard"][2] == 0     # the empty shard took part
        if sync_bn:   # the statistics table was the global batch's
            x = _data()[0][torch.tensor([4, 0, 6])]
            assert abs(a["train"][0][0][1] - x.mean().item()) <= 1e-12
    # DataParallel.train_step with sync_bn: the first global step on both ranks
    for r in range(world):
        step = ranks[r]["train_step"]
        assert step["shard"] == step["want"]
        np.testing.assert_allclose(step["loss"], train_ref[0][0], rtol=1e-12)
        assert abs(step["w"] - w1_ref) <= 1e-12
