"""VAE data parallelism with the single-device arithmetic on ONE GPU: one engine per rank, each on its own host thread, each on
its shard of a global batch through vae_forward_backward_sync / vae_eval_step_sync, with an all-reduce callback that adds the
engines' tables (tests/test_unet_syncbn_gpu.py's _run_ranks).  Their summed gradients, losses and running statistics must
equal one engine's step on the whole batch: the global BatchNorm statistics, the loss means and gradient coefficients over
the global batch, and the noise of the global rows all have to be right."""
import numpy as np
import pytest
import torch

from test_unet_syncbn_gpu import _host, _run_ranks
from test_vae_hip_parity import _engine, _feeds_batchnorm, _setup

pytestmark = pytest.mark.gpu

(FC, LATENT) = (16, 6)
HYPER = dict(lambda_mse=1.0, lambda_kl=0.5, lambda_ssim=2.0, seed=9)


def _case(B):
    return _setup((12, 12), (176, 192), FC, LATENT, B, seed=5)


def _make(case, max_batch):
    (spec, enc, dec, x, t) = case
    eng = _engine(spec, enc, dec, FC, LATENT, max_batch, **HYPER)
    eng.set_step(3)
    eng.set_dataset(0, x, t)
    return eng


def _n_bn(eng):
    return sum(1 for n in eng.tensors if n.endswith(".running_mean"))


def _shards(B, world):
    from cae_tools_amd.dp import shard_bounds
    return [shard_bounds(B, world, r) for r in range(world)]


def _sync_step(case, B, world, bn_world=None):
    """the ranks' forward_backward_sync on shards of B rows: (engines, per-rank gradients, the table sizes every rank passed)"""
    bounds = _shards(B, world)
    engines = [_make(case, max(1, max(hi - lo for (lo, hi) in bounds))) for _ in range(world)]
    grads = [None] * world

    def call(r, eng, allreduce):
        (lo, hi) = bounds[r]
        grads[r] = eng.forward_backward_sync(0, None, lo, hi - lo, lo, B, world if bn_world is None else bn_world, allreduce,
                                             slot=0)

    sizes = _run_ranks(engines, call)
    return engines, grads, sizes


def _one_engine(case, B):
    eng = _make(case, B)
    g = eng.forward_backward(0, None, 0, B, slot=0)
    return eng, _host(g)


def _check_equal_to_one_engine(case, B, world):
    (one, g1) = _one_engine(case, B)
    (engines, grads, sizes) = _sync_step(case, B, world)
    gsum = sum(_host(g) for g in grads)
    scale = np.abs(g1).max()
    assert np.abs(gsum - g1).max() <= 2e-5 * scale, np.abs(gsum - g1).max() / scale
    want = np.array(one.read_losses(0, 1)[0])
    bufs = [_host(e.buffers) for e in engines]
    for (r, eng) in enumerate(engines):
        np.testing.assert_allclose(eng.read_losses(0, 1)[0], want, rtol=1e-6, atol=0)
        np.testing.assert_allclose(bufs[r], _host(one.buffers), rtol=1e-6, atol=1e-9)
        np.testing.assert_array_equal(bufs[r], bufs[0])
    # the same tables in the same order on every rank (_run_ranks checks that): 2 per BatchNorm layer and the loss table
    assert len(sizes) == 2 * _n_bn(one) + 1
    assert sizes.count(3) == 1
    return one, g1, engines


def test_two_ranks_equal_one_engine():
    B = 5
    case = _case(B)
    (one, g1, _) = _check_equal_to_one_engine(case, B, 2)
    # ... which the half-step with per-rank statistics and local means does not: the test can tell the difference
    bounds = _shards(B, 2)
    old = 0
    for (lo, hi) in bounds:
        eng = _make(case, B)
        old = old + _host(eng.forward_backward(0, None, lo, hi - lo, slot=0, global_batch=B))
    assert np.abs(old - g1).max() > 1e-3 * np.abs(g1).max()


def test_three_ranks_with_an_empty_shard():
    case = _case(2)
    _check_equal_to_one_engine(case, 2, 3)      # shards 1 / 1 / 0


def test_per_rank_statistics_pass_only_the_loss_table():
    B = 5
    (engines, grads, sizes) = _sync_step(_case(B), B, 2, bn_world=0)
    assert sizes == [3]
    assert all(np.isfinite(_host(g)).all() for g in grads)
    (l0, l1) = (engines[0].read_losses(0, 1)[0], engines[1].read_losses(0, 1)[0])
    np.testing.assert_array_equal(l0, l1)


def test_noise_rows_are_the_global_rows():
    B = 5
    case = _case(B)
    (one, _) = _one_engine(case, B)
    (eps1, z1) = (one.debug_read("eps", (B, LATENT)), one.debug_read("z", (B, LATENT)))
    (engines, _, _) = _sync_step(case, B, 2)
    for ((lo, hi), eng) in zip(_shards(B, 2), engines):
        np.testing.assert_array_equal(eng.debug_read("eps", (hi - lo, LATENT)), eps1[lo:hi])
        np.testing.assert_allclose(eng.debug_read("z", (hi - lo, LATENT)), z1[lo:hi], rtol=1e-5, atol=1e-6)
    assert np.abs(eps1[3:5] - eps1[0:2]).max() > 0.1     # (rows of a shard do not repeat another shard's)


@pytest.mark.parametrize("world", [2, 3])
def test_eval_step_sync_equals_one_eval_step(world):
    B = 2 if world == 3 else 5
    case = _case(B)
    one = _make(case, B)
    one.eval_step(0, None, 0, B, slot=1)
    want = np.array(one.read_losses(1, 1)[0])
    bounds = _shards(B, world)
    engines = [_make(case, max(1, max(hi - lo for (lo, hi) in bounds))) for _ in range(world)]

    def call(r, eng, allreduce):
        (lo, hi) = bounds[r]
        eng.eval_step_sync(0, None, lo, hi - lo, lo, B, allreduce, slot=1)

    sizes = _run_ranks(engines, call)
    assert sizes == [3]
    for eng in engines:
        np.testing.assert_allclose(eng.read_losses(1, 1)[0], want, rtol=1e-6, atol=0)


def test_argument_checks():
    from cae_tools_amd._lib import CaeError
    eng = _make(_case(5), 3)
    with pytest.raises(CaeError):
        eng.forward_backward_sync(0, None, 0, 3, 3, 5, 1, lambda t: None)     # rows 3..6 of a batch of 5
    with pytest.raises(CaeError):
        eng.forward_backward_sync(0, None, 0, 4, 0, 5, 1, lambda t: None)     # 4 rows on an engine of 3
    with pytest.raises(CaeError):
        eng.eval_step_sync(0, None, 0, 2, 4, 5, lambda t: None)
    with pytest.raises(CaeError):
        eng.eval_step_sync(0, None, 0, 4, 0, 5, lambda t: None)


def test_one_rank_follows_the_plain_train_step():
    """world 1 with an identity all-reduce, step by step against vae_train_step: the same model up to fp32 rounding"""
    B = 5
    case = _case(B)
    (plain, dp) = (_make(case, B), _make(case, B))
    steps = 3
    g = torch.zeros(dp.n_param, dtype=torch.float32, device=dp.device)
    for s in range(steps):
        plain.train_step(0, None, 0, B, slot=s)
        dp.forward_backward_sync(0, None, 0, B, 0, B, 1, lambda t: None, out=g, slot=s)
        dp.apply_gradients(g)
        np.testing.assert_allclose(dp.read_losses(s, 1)[0], plain.read_losses(s, 1)[0], rtol=1e-5)
    (p0, p1) = (_host(plain.params), _host(dp.params))
    n_dec = max(int(n.split(".")[1]) for n in plain.tensors if n.startswith("dec/decoder_conv.")) // 3
    last_bias = "dec/decoder_conv.%d.bias" % (3 * n_dec)
    lr = 1e-3
    for (name, (arena, off, numel, _)) in plain.tensors.items():
        if arena != 0:
            continue
        # (biases in front of a BatchNorm have an exact gradient of 0: Adam turns their rounding noise into lr-sized steps)
        tol = (2.0 if _feeds_batchnorm(name, last_bias) else 0.05) * lr * steps
        err = np.abs(p0[off:off + numel] - p1[off:off + numel]).max()
        assert err <= tol, f"{name}: {err:.3e} > {tol:.3e}"
    np.testing.assert_allclose(_host(dp.buffers), _host(plain.buffers), rtol=1e-5, atol=1e-7)
