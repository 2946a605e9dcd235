"""UNET.train() data-parallel: two ranks (child processes, both on GPU 0, over a gloo group - RCCL refuses two ranks on one
device; gloo stages CUDA tensors through the host) must train one model, bit for bit the same on both ranks, and that model
must be the single-process train()'s up to fp32 summation order - dropout on, a loss mask, and a last global batch of one
row per rank."""
import io
import os
import socket
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KW = dict(batch_size=6, nr_epochs=2, test_interval=1, fc_size=10, encoded_dim_size=4, lr=1e-3, weight_decay=1e-5,
          dropout_rate=0.1, lambda_pearson=0.5)
STEPS = 2 * 3     # 14 samples in global batches of 6: 6, 6, 2 per epoch


def _train(model_path):
    """UNET.train() on the shared data; what the comparison needs"""
    from test_unet_model_api import _data
    from cae_tools_amd.models.unet import UNET, unet_layer_spec
    (train, test) = (_data(14, 1), _data(6, 2))
    torch.manual_seed(7)
    mt = UNET(**KW)
    mt.spec = unet_layer_spec(2, 1, (16, 16), [8, 16])
    buf = io.StringIO()
    with redirect_stdout(buf):
        mt.train(["lo"], "hi", train, test, model_path=model_path, mask_variable_name="valid")
    eng = mt._engine
    eng.sync()
    return {"params": eng.params.cpu(), "buffers": eng.buffers.cpu(), "history": mt.history, "timing": mt.timing,
            "max_batch": eng.max_batch, "stdout": buf.getvalue(), "tensors": dict(eng.tensors)}


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = _train(os.path.join(out_dir, f"model_rank{rank}"))
        torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_train_the_single_device_model(tmp_path):
    import multiprocessing
    ctx = multiprocessing.get_context("spawn")
    world = 2
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
    stuck = [p for p in procs if p.is_alive()]
    for p in stuck:
        p.terminate()
        p.join(timeout=30)
    assert not stuck, "a rank did not finish (a collective was left waiting)"
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    (r0, r1) = (torch.load(tmp_path / "rank0.pt", weights_only=False), torch.load(tmp_path / "rank1.pt", weights_only=False))

    # one model on both ranks
    assert torch.equal(r0["params"], r1["params"])
    assert torch.equal(r0["buffers"], r1["buffers"])
    assert r0["history"] == r1["history"]
    for r in (r0, r1):
        assert r["timing"]["world"] == 2
        assert r["max_batch"] == 3
    # only the lead rank saves and prints the epoch lines
    assert os.path.isdir(tmp_path / "model_rank0") and not os.path.exists(tmp_path / "model_rank1")
    assert "epoch: 1," in r0["stdout"] and "epoch:" not in r1["stdout"]

    # ... and it is the single-process model
    one = _train(str(tmp_path / "model_single"))
    assert one["timing"]["world"] == 1
    # Biases right before a BatchNorm have an exact gradient of 0, and those of the gated decoder layers nearly so (the
    # per-sample gate is all that keeps the BatchNorm from cancelling a shift): AdamW turns their rounding noise into
    # lr-sized steps of either sign on both sides, so they only get a bound on the update size.
    from unet_helpers import feeds_batchnorm
    last = len(one["tensors"]) and max(int(n.split(".")[1]) for n in one["tensors"] if n.startswith("dec/decoder_conv."))

    def noisy(key):
        return feeds_batchnorm(key) or (key.startswith("decoder_conv.") and key.endswith(".bias")
                                         and int(key.split(".")[1]) < last)
    for (name, (arena, off, numel, _)) in one["tensors"].items():
        if arena != 0:
            continue
        tol = (4.0 if noisy(name[4:]) else 0.05) * KW["lr"] * STEPS
        err = (r0["params"][off:off + numel].double() - one["params"][off:off + numel].double()).abs().max().item()
        assert err <= tol, f"{name}: {err:.3e} > {tol:.3e}"
    for key in ("train_loss", "test_loss"):
        np.testing.assert_allclose(r0["history"][key], one["history"][key], rtol=1e-4, atol=0)
    # (the running means follow the pre-BatchNorm biases above, which drift apart by AdamW-amplified rounding noise)
    np.testing.assert_allclose(r0["buffers"].numpy(), one["buffers"].numpy(), rtol=1e-4, atol=1e-3)
