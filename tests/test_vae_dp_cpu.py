"""VarAEModel.train() data-parallel wiring on CPU: two gloo ranks run the model's train() over a stand-in engine (the members
GradientHalfSteps and DataParallel.run_batches drive: forward_backward_sync / eval_step_sync with their all-reduce callback,
apply_gradients, read_losses, the arenas), with the data-set set-up and the epilogue replaced.  Both ranks must train on rank
0's shuffles from rank 0's weights, size the engine to a rank's share of the global batch, cover every global batch with
their shards (an empty one included), record the same history and world, and only rank 0 may print and lead the epilogue."""
import io
import os
import socket
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_TRAIN, N_TEST, BATCH, EPOCHS = 7, 3, 3, 2     # global batches 3, 3, 1 (train) and 3 (test): shards 2/1, 2/1, 1/0, 2/1


class StandInEngine:
    """y = w . mean(perm rows): the loss table of a shard is {sum of its sample indices, its rows}, summed over the ranks"""

    LOSSES_PER_BATCH = 4

    def __init__(self, max_batch, rank):
        self.max_batch = max_batch
        self.n_param = 3
        (self.device, self.stream) = (torch.device("cpu"), None)
        self.params = torch.full((3,), 1.0 + rank)      # rank-dependent: train() must start every rank from rank 0's
        self.buffers = torch.full((2,), 10.0 + rank)
        (self.exp_avg, self.exp_avg_sq) = (torch.zeros(3), torch.zeros(3))
        self.loss_slots = 4
        self.slots = [None] * self.loss_slots
        self.calls = []

    # set-up calls of train()
    def set_hyper(self, **kw):
        self.hyper = kw

    def reset_optimizer(self):
        pass

    def set_dataset(self, which, x, t):
        pass

    def upload_perm(self, perm):
        return torch.as_tensor(np.asarray(perm), dtype=torch.int64)

    def sync(self):
        pass

    def _shard(self, which, perm, start, size, row0, global_batch, allreduce, slot):
        rows = perm[start:start + size]
        table = torch.tensor([float(rows.sum()), float(size)], dtype=torch.float64)
        allreduce(table)
        assert table[1].item() == global_batch
        self.calls.append((which, int(start), int(size), int(row0), int(global_batch)))
        mean = table[0].item() / global_batch
        self.slots[slot] = (mean, 0.0, 0.0, mean)
        return rows

    def forward_backward_sync(self, which, perm, start, size, row0, global_batch, world, allreduce, out=None, slot=0):
        assert world == 2      # sync_bn defaults to True: BatchNorm over the global batch
        rows = self._shard(which, perm, start, size, row0, global_batch, allreduce, slot)
        out.copy_(torch.tensor([float(rows.sum()), float(size), 1.0]) / global_batch)
        return out

    def eval_step_sync(self, which, perm, start, size, row0, global_batch, allreduce, slot=0):
        self._shard(which, perm, start, size, row0, global_batch, allreduce, slot)

    def apply_gradients(self, grads):
        self.params -= 0.01 * grads

    def read_losses(self, first, count):
        return [self.slots[first + i] for i in range(count)]


class _Ds:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def device_inputs(self):
        return None

    def device_outputs(self):
        return None


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cae_tools_amd.models.var_ae_model import VarAEModel
        m = VarAEModel(batch_size=BATCH, nr_epochs=EPOCHS, test_interval=1)
        seen = {}
        rng = np.random.default_rng(100 + rank)     # each rank draws its own shuffles: train() must use rank 0's

        def prologue(*args, **kw):
            seen["perms"] = (rng.permutation(N_TRAIN), rng.permutation(N_TEST))
            return (_Ds(N_TRAIN), _Ds(N_TEST)) + seen["perms"]

        def get_engine(max_batch):
            m._engine = StandInEngine(max_batch, rank)
            return m._engine

        def epilogue(*args, lead=True, **kw):
            seen["lead"] = lead
            return {}

        (m._train_prologue, m._get_engine, m._train_epilogue) = (prologue, get_engine, epilogue)
        buf = io.StringIO()
        with redirect_stdout(buf):
            m.train(["x"], "y", None, None)
        eng = m._engine
        torch.save({"calls": eng.calls, "params": eng.params.clone(), "buffers": eng.buffers.clone(), "history": m.history,
                    "timing": m.timing, "max_batch": eng.max_batch, "lead": seen["lead"], "stdout": buf.getvalue(),
                    "own_perms": seen["perms"]}, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_var_ae_model_train_shards_over_two_gloo_ranks(tmp_path):
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    (r0, r1) = (torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(world))
    (train_perm, test_perm) = r0["own_perms"]
    assert not np.array_equal(r1["own_perms"][0], train_perm)     # (so that the broadcast is what makes them agree)

    # one model: rank 0's weights and buffers, the same updates, the same history on both ranks
    assert torch.equal(r0["params"], r1["params"]) and torch.equal(r0["buffers"], r1["buffers"])
    assert torch.equal(r0["buffers"], torch.full((2,), 10.0))
    assert r0["history"] == r1["history"]

    # shards: rank r takes rows shard_bounds(gb, 2, r) of every global batch of rank 0's shuffle, an empty shard included
    from cae_tools_amd.dp import shard_bounds

    def expected(rank):
        calls = []
        for _ in range(EPOCHS):
            for (which, n) in ((0, N_TRAIN), (1, N_TEST)):
                for b0 in range(0, n, BATCH):
                    gb = min(BATCH, n - b0)
                    (lo, hi) = shard_bounds(gb, world, rank)
                    calls.append((which, b0 + lo, hi - lo, lo, gb))
        return calls
    assert r0["calls"] == expected(0) and r1["calls"] == expected(1)
    assert (0, 7, 0, 1, 1) in r1["calls"]      # the last training batch: rank 1 holds no row of it

    # the recorded losses are the global batches' means of rank 0's shuffle
    def mean_loss(perm, n):
        return float(np.mean([perm[b0:b0 + BATCH].mean() for b0 in range(0, n, BATCH)]))
    assert np.allclose(r0["history"]["train_loss"], [mean_loss(train_perm, N_TRAIN)] * EPOCHS)
    assert np.allclose(r0["history"]["test_loss"], [mean_loss(test_perm, N_TEST)] * EPOCHS)

    for r in (r0, r1):
        assert r["timing"]["world"] == 2
        assert r["max_batch"] == 2      # ceil(3 / 2)
    assert (r0["lead"], r1["lead"]) == (True, False)
    assert "Running on device" in r0["stdout"] and r1["stdout"] == ""
