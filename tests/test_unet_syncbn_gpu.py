"""UNET data parallelism with the single-device arithmetic on ONE GPU: one engine per rank, each on its own host thread,
each on its shard of a global batch through unet_forward_backward_sync / unet_eval_step_sync, with an all-reduce callback
that adds the engines' tables.  Their summed gradients, their losses and running statistics must equal one engine's step
on the whole batch - with dropout on and a loss mask that covers the shards very unequally, so that the global loss
denominators, the dropout masks of the global rows and the global BatchNorm statistics all have to be right."""
import threading

import numpy as np
import pytest
import torch

from unet_helpers import UnetCase

pytestmark = pytest.mark.gpu

DROPOUT = 0.1


def _batch():
    """5 rows (the case's first two batches) with a mask that leaves ~10 % of rows 0..2 and all of rows 3..4"""
    c = UnetCase("u_k4_b3")
    (x0, t0, m0) = c.step_batch(0)
    (x1, t1, m1) = c.step_batch(1)
    (x, t, m) = (torch.cat([x0, x1]), torch.cat([t0, t1]), torch.cat([m0, m1]).clone())
    g = torch.Generator().manual_seed(5)
    m[:3] *= (torch.rand(m[:3].shape, generator=g) < 0.1).float()
    m[3:] = 1.0
    return c, x, t, m


def _make(c, x, t, m, max_batch):
    from test_unet_hip_parity import _engine
    eng = _engine(c, max_batch=max_batch, dropout=DROPOUT, seed=7)
    eng.set_dataset(0, x, t, m)
    return eng


def _host(v):
    torch.cuda.synchronize()
    return v.detach().cpu().numpy().astype(np.float64)


def _run_ranks(engines, call, timeout=120):
    """call(r, engine, allreduce) on one thread per engine; allreduce adds the engines' tables behind a barrier.  Returns the
    tables' sizes in the order each rank passed them."""
    world = len(engines)
    barrier = threading.Barrier(world)
    tables = [None] * world
    sizes = [[] for _ in range(world)]
    errors = []

    def allreduce_for(r):
        def fn(table):
            torch.cuda.synchronize()
            tables[r] = table
            sizes[r].append(table.numel())
            barrier.wait()
            if r == 0:
                total = sum(tables[1:], tables[0].clone())
                for tb in tables:
                    tb.copy_(total)
                torch.cuda.synchronize()
            barrier.wait()
        return fn

    def run(r):
        try:
            call(r, engines[r], allreduce_for(r))
            engines[r].sync()
        except Exception as ex:  # pragma: no cover
            errors.append(ex)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=timeout)
    assert not any(th.is_alive() for th in threads), "a rank did not finish: a collective was left waiting"
    assert not errors, errors
    assert all(s == sizes[0] for s in sizes), f"the ranks passed different tables: {sizes}"
    return sizes[0]


def _shards(n, world):
    from cae_tools_amd.dp import shard_bounds
    return [shard_bounds(n, world, r) for r in range(world)]


def _check_step(c, x, t, m, world, n):
    full = _make(c, x, t, m, n)
    g_full = _host(full.forward_backward(0, None, 0, n, slot=0))
    loss_full = np.array(full.read_losses(0, 1)[0])
    shards = _shards(n, world)
    ranks = [_make(c, x, t, m, max(1, -(-n // world))) for _ in range(world)]
    grads = [torch.zeros(full.n_param, dtype=torch.float32, device="cuda:0") for _ in range(world)]

    def call(r, eng, allreduce):
        (lo, hi) = shards[r]
        eng.forward_backward_sync(0, None, lo, hi - lo, lo, n, world, allreduce, out=grads[r], slot=0)

    sizes = _run_ranks(ranks, call)
    levels = len(c.meta["spec"]["input_layers"])
    assert len(sizes) == 2 * (2 * levels + 1) + 1 and sizes.count(3) == 1
    g_sum = sum(_host(g) for g in grads)
    scale = np.abs(g_full).max()
    assert np.abs(g_sum - g_full).max() <= 2e-5 * scale, np.abs(g_sum - g_full).max() / scale
    for eng in ranks:
        np.testing.assert_allclose(np.array(eng.read_losses(0, 1)[0]), loss_full, rtol=1e-6, atol=0)
    b_full = _host(full.buffers)
    b0 = _host(ranks[0].buffers)
    for eng in ranks[1:]:
        assert np.array_equal(_host(eng.buffers), b0), "running statistics differ between the ranks"
    np.testing.assert_allclose(b0, b_full, rtol=1e-6, atol=1e-7)
    return full, g_full, shards


def test_two_ranks_equal_one_device():
    (c, x, t, m) = _batch()
    n = x.shape[0]
    (full, g_full, shards) = _check_step(c, x, t, m, 2, n)
    assert [hi - lo for (lo, hi) in shards] == [3, 2]
    # negative control: the local half-steps (per-rank BatchNorm, local mask count, rank-local dropout indices) miss it
    g_local = 0
    for (lo, hi) in shards:
        eng = _make(c, x, t, m, n)
        g_local = g_local + _host(eng.forward_backward(0, None, lo, hi - lo, slot=0, global_batch=n))
    assert np.abs(g_local - g_full).max() > 1e-3 * np.abs(g_full).max()


def test_three_ranks_with_an_empty_shard():
    (c, x, t, m) = _batch()
    # global batch 2 over 3 ranks: rows {0}, {1}, {} - rows 0 and 1 of the data set
    (_, _, shards) = _check_step(c, x, t, m, 3, 2)
    assert [hi - lo for (lo, hi) in shards] == [1, 1, 0]


def test_eval_step_sync_equals_one_device():
    (c, x, t, m) = _batch()
    n = x.shape[0]
    full = _make(c, x, t, m, n)
    full.eval_step(0, None, 0, n, slot=0)
    want = np.array(full.read_losses(0, 1)[0])
    for world in (2, 3):
        shards = _shards(n, world)
        ranks = [_make(c, x, t, m, n) for _ in range(world)]

        def call(r, eng, allreduce):
            (lo, hi) = shards[r]
            eng.eval_step_sync(0, None, lo, hi - lo, lo, n, allreduce, slot=0)

        assert _run_ranks(ranks, call) == [3]
        for eng in ranks:
            np.testing.assert_allclose(np.array(eng.read_losses(0, 1)[0]), want, rtol=1e-6, atol=0)


def test_one_rank_sync_path_matches_the_fused_step():
    (c, x, t, m) = _batch()
    n = x.shape[0]
    (a, b) = (_make(c, x, t, m, n), _make(c, x, t, m, n))
    grads = torch.zeros(a.n_param, dtype=torch.float32, device="cuda:0")
    calls = []
    steps = 3
    for i in range(steps):
        a.train_step(0, None, 0, n, slot=i)
        b.forward_backward_sync(0, None, 0, n, 0, n, 1, lambda tb: calls.append(tb.numel()), out=grads, slot=i)
        b.apply_gradients(grads)
    (la, lb) = (np.array(a.read_losses(0, steps)), np.array(b.read_losses(0, steps)))
    np.testing.assert_allclose(lb, la, rtol=1e-4, atol=1e-7)
    assert len(calls) == steps * (2 * (2 * len(c.meta["spec"]["input_layers"]) + 1) + 1)
    assert np.abs(_host(a.params) - _host(b.params)).max() <= 0.05 * c.meta["lr"] * steps


def test_shard_arguments_are_checked():
    from cae_tools_amd._lib import CaeError
    (c, x, t, m) = _batch()
    eng = _make(c, x, t, m, 3)
    noop = lambda tb: None  # noqa: E731
    with pytest.raises(CaeError):      # rows past the global batch
        eng.forward_backward_sync(0, None, 0, 3, 2, 4, 2, noop)
    with pytest.raises(CaeError):      # more rows than the engine holds
        eng.forward_backward_sync(0, None, 0, 4, 0, 5, 2, noop)
    with pytest.raises(ValueError):    # BatchNorm1d over a one-row global batch
        eng.forward_backward_sync(0, None, 0, 1, 0, 1, 1, noop)
    # ... but a one-row shard of a larger global batch is a legal step
    eng.forward_backward_sync(0, None, 0, 1, 0, 4, 1, lambda tb: None)
