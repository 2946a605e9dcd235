"""Bitwise run-to-run reproducibility of the UNET, VAE and Linear training steps (the ConvAE path's is
tests/test_reproducible_gpu.py).

Every cross-workgroup fp64 sum of these engines lands on a fixed grid first (acc_grid.h: ACC_STAT, ACC_GRAD, ACC_PLANE), or
is folded in a fixed order, and the fp32 split-K convolutions of the UNET combine their K slices without depending on which
finishes first (kernels_unet_mfma.h split_store: two slices by commuting fp32 atomics onto a zeroed map, more through partial
maps that k_slice_fold adds in slice order).  So two runs of the same steps from the same state give the same BITS in every
loss, parameter, Adam moment and running statistic.  Split counts quoted below follow the launch rules:
  k_pdown (pdown_slices): tiles = B * (Hs / (128 / Ws)) * ceil(Cs / (32 RBN)), RBN 2 where Cs <= 64 or B * Hs * Ws / 128 <= 256;
          K slices double while tiles * slices < 384, Cl / 4 / (2 slices) >= 4 and slices < 8;
  OpDown  (mfma_down_slices): tiles of 128 x 128 (Cs > 64) over (Cs, B * Hs * Ws); slices double while tiles * slices < 384,
          Cl / (2 slices) >= 8 and slices < 8."""
import json
import os
import socket

import numpy as np
import pytest
import torch

from unet_helpers import UnetCase

pytestmark = pytest.mark.gpu

CFG3_CHANNELS = [32, 64, 128, 256]
MEDIUM_CHANNELS = [16, 32, 64, 72]


def _same_bits(a, b, what):
    """a, b: (losses, [(name, tensor), ...]) of two runs"""
    (la, ta), (lb, tb) = a, b
    assert len(la) == len(lb)
    for i, (u, v) in enumerate(zip(la, lb)):
        assert u == v, f"{what}: loss {i} differs: {u!r} != {v!r}"
    for (name, u), (_, v) in zip(ta, tb):
        assert torch.equal(u, v), f"{what}: {name} differ in {int((u != v).sum())} of {u.numel()} entries"


def _state(eng):
    out = [("params", eng.params.cpu()), ("exp_avg", eng.exp_avg.cpu()), ("exp_avg_sq", eng.exp_avg_sq.cpu())]
    if getattr(eng, "buffers", None) is not None:
        out.append(("running statistics", eng.buffers.cpu()))
    return out


def _losses(eng, first, count):
    out = []
    for v in eng.read_losses(first, count):
        out.extend(v if isinstance(v, tuple) else (v,))
    return out


class _OneRankGroup:
    """a one-rank RCCL group for the data-parallel half-steps (what tools/bench_unet.py --force-dp runs)"""

    def __enter__(self):
        import torch.distributed as dist
        self.dist = dist
        self.made = False
        if not dist.is_initialized():
            with socket.socket() as s:
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
            os.environ["MASTER_ADDR"] = "127.0.0.1"
            os.environ["MASTER_PORT"] = str(port)
            torch.cuda.set_device(0)
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
            self.made = True
        return dist

    def __exit__(self, *exc):
        if self.made:
            self.dist.destroy_process_group()


def _sharded_steps(eng, steps, batch, perm=None):
    """the data-parallel step of a one-rank group: forward_backward_sync with SyncBN, the gradient all-reduce, the Adam
    half-step; the losses of every step"""
    from cae_tools_amd.dp import GradientHalfSteps
    with _OneRankGroup() as dist:
        half = GradientHalfSteps(eng)
        losses = []
        for k in range(steps):
            slot = half.forward_backward_sync(0, perm, (k % 2) * batch, batch, 0, batch, 1, dist.all_reduce)
            with torch.cuda.stream(eng.stream):
                dist.all_reduce(half.grads)
            half.adam_step()
            losses.extend(_losses(half, slot, 1))
        eng.sync()
    return losses


# ---- UNET --------------------------------------------------------------------------------------------------------------------

def _unet_run(chans, size, batch, steps=3, specialised=True, mode="train", seed=11):
    from cae_tools_amd.models.unet import Decoder, Encoder, unet_layer_spec
    from cae_tools_amd.unet_engine import UnetEngine
    spec = unet_layer_spec(3, 3, (size, size), chans)
    (fc, latent) = (128, 32) if chans == CFG3_CHANNELS else (20, 5)
    torch.manual_seed(seed)
    enc = Encoder(spec.get_input_layers(), latent, fc)
    dec = Decoder(spec.get_output_layers(), latent, fc)
    g = torch.Generator().manual_seed(seed + 1)
    n = 2 * batch
    x = torch.rand((n, 3, size, size), generator=g)
    t = torch.rand((n, 3, size, size), generator=g)
    m = (torch.rand((n, 1, size, size), generator=g) < 0.9).float()    # a partial loss mask
    eng = UnetEngine(spec, fc, latent, batch, device="cuda:0", specialised=specialised)
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(lr=1e-3, weight_decay=1e-5, dropout_rate=0.1, lambda_pearson=1.0, seed=3)
    eng.set_dataset(0, x.cuda(), t.cuda(), m.cuda())
    if mode == "sharded":
        losses = _sharded_steps(eng, steps, batch)
    else:
        for k in range(steps):
            eng.train_step(0, None, (k % 2) * batch, batch, slot=k)
        losses = _losses(eng, 0, steps)
        if mode == "eval":
            for k in range(2):
                eng.eval_step(0, None, k * batch, batch, slot=10 + k)
            losses += _losses(eng, 10, 2)
    eng.sync()
    out = (losses, _state(eng))
    eng.close()
    return out


@pytest.mark.parametrize("batch", [5, 32])
def test_unet_benchmark_geometry(batch):
    """cfg3: 3 x 256 x 256, channels 32/64/128/256, fc 128 / latent 32, dropout 0.1, a partial mask, 3 training steps.
    Batch 5 (few pixel tiles): k_pdown slices K of the encoder's 64 -> 128 layer (32 x 32 out: 80 tiles) 4 ways and of its
    128 -> 256 layer (16 x 16 out: 40 tiles) 8 ways, as for the decoder input gradients of the matching ConvTranspose2d
    layers - partial maps folded in slice order.  Batch 32 (the benchmark batch): only the 16 x 16 layers are sliced, 2 ways
    (256 tiles), through the commuting atomics; everything else is the plain fp64 sums on their grids (BatchNorm, loss moments,
    weight and bias gradients, the Linear layers' K slices)."""
    _same_bits(_unet_run(CFG3_CHANNELS, 256, batch), _unet_run(CFG3_CHANNELS, 256, batch), f"cfg3 batch {batch}")


@pytest.mark.parametrize("specialised", [True, False], ids=["specialised", "generic"])
def test_unet_other_kernel_families(specialised):
    """128 px, channels 16/32/64/72 (the geometry of test_mfma_path_at_medium_size_against_oracle_and_generic_kernels) at
    batch 3.  Specialised: the thin image-end kernels, k_pdown on the 32- and 64-channel layers (the 64-channel one sliced 2
    ways: 6 tiles, Cl = 32), and the tile engine's OpDown on the 72-channel 8 x 8 layer and the input gradient of its
    transposed twin (2 column tiles, Cl = 64: 8 K slices, folded in slice order).  Generic: the one-thread-per-output
    convolutions and k_wgrad's fp64 sums over 256-thread blocks."""
    what = "128 px " + ("specialised" if specialised else "generic")
    _same_bits(_unet_run(MEDIUM_CHANNELS, 128, 3, specialised=specialised),
               _unet_run(MEDIUM_CHANNELS, 128, 3, specialised=specialised), what)


def _golden_run(name):
    from cae_tools_amd.unet_engine import UnetEngine
    c = UnetCase(name)
    m = c.meta
    eng = UnetEngine(m["spec"], m["fc"], m["latent"], m["batch"], device="cuda:0")
    eng.load_state(c.state("init", "enc"), c.state("init", "dec"))
    eng.set_hyper(lr=m["lr"], weight_decay=m["weight_decay"], dropout_rate=m["dropout"], lambda_pearson=m["lambda_pearson"], seed=0)
    (x, t, mk) = c.step_batch(0)
    eng.set_dataset(0, x.cuda(), t.cuda(), mk.cuda())
    for k in range(3):
        eng.train_step(0, None, 0, x.shape[0], slot=k)
    eng.sync()
    out = (_losses(eng, 0, 3), _state(eng))
    eng.close()
    return out


def test_unet_golden_deep6():
    """the golden u_deep6_b4 case: six levels, every layer past the eighth repacked (a second repack launch), 3 steps"""
    _same_bits(_golden_run("u_deep6_b4"), _golden_run("u_deep6_b4"), "u_deep6_b4")


def test_unet_sharded_step():
    """the data-parallel step over a one-rank group at cfg3, batch 5 (SyncBN tables and the loss totals through the
    all-reduce, the gradient all-reduce, the Adam half-step) - twice"""
    _same_bits(_unet_run(CFG3_CHANNELS, 256, 5, mode="sharded"), _unet_run(CFG3_CHANNELS, 256, 5, mode="sharded"),
               "cfg3 sharded")


def test_unet_eval_steps():
    """two eval steps after the training steps (running statistics, no dropout): their losses, twice"""
    _same_bits(_unet_run(MEDIUM_CHANNELS, 128, 3, mode="eval"), _unet_run(MEDIUM_CHANNELS, 128, 3, mode="eval"), "eval steps")


# ---- VAE ---------------------------------------------------------------------------------------------------------------------

def _vae_run(in_size, out_size, batch, sharded=False, seed=13):
    from cae_tools_amd.models.decoder import Decoder
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.models.var_ae_model import VarEncoder
    from cae_tools_amd.vae_engine import VaeEngine
    spec = create_model_spec(input_size=in_size, input_channels=1, output_size=out_size, output_channels=1)
    torch.manual_seed(seed)
    enc = VarEncoder(spec.get_input_layers(), 32, 128)
    dec = Decoder(spec.get_output_layers(), 32, 128)
    g = torch.Generator().manual_seed(seed + 1)
    n = 2 * batch
    x = torch.rand((n, 1) + tuple(in_size), generator=g)
    t = torch.rand((n, 1) + tuple(out_size), generator=g)
    eng = VaeEngine(spec, 128, 32, batch, device="cuda:0")
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(seed=1)     # noise on: the reparameterisation draws eps from the seed
    eng.set_dataset(0, x.cuda(), t.cuda())
    if sharded:
        losses = _sharded_steps(eng, 3, batch)
    else:
        for k in range(3):
            eng.train_step(0, None, (k % 2) * batch, batch, slot=k)
        eng.eval_step(0, None, batch, batch, slot=3)
        losses = _losses(eng, 0, 4)
    eng.sync()
    out = (losses, _state(eng))
    eng.close()
    return out


@pytest.mark.parametrize("geom", [((64, 64), (512, 512), 16), ((12, 12), (176, 176), 4)], ids=["cfg5", "176px"])
def test_vae_steps(geom):
    """3 training steps (noise on) and an eval step: the KL sum (k_reparam), the MS-SSIM / contrast sums of every scale
    (k_ssim_fwd_rows at the finest scale, k_ssim_fwd_rows_multi for the coarse ones at cfg5), the MSE and bias-gradient sums
    of k_vae_loss_grad, and the ConvAE trunk's own sums.  cfg5: 64 x 64 -> 512 x 512 at batch 16; 176 px at batch 4."""
    (i, o, b) = geom
    _same_bits(_vae_run(i, o, b), _vae_run(i, o, b), f"VAE {o[0]} px")


def test_vae_sharded_step():
    """the data-parallel step of a one-rank group at 176 px, batch 4: the loss parts through the all-reduce - twice"""
    _same_bits(_vae_run((12, 12), (176, 176), 4, sharded=True), _vae_run((12, 12), (176, 176), 4, sharded=True), "VAE sharded")


# ---- Linear ------------------------------------------------------------------------------------------------------------------

def _linear_run(name):
    from cae_tools_amd.linear_engine import LinearEngine
    from test_linear_cpu import load
    (meta, z) = load(name)
    eng = LinearEngine(meta["in_shape"], meta["out_shape"], max_batch=8, device="cuda:0")
    eng.load_state({k: z["init/" + k] for k in meta["keys"]})
    eng.set_hyper(lr=meta["lr"], weight_decay=meta["weight_decay"])
    (x, t) = (torch.from_numpy(z["step0/x"]), torch.from_numpy(z["step0/t"]))
    eng.set_dataset(0, x, t)
    for k in range(4):
        eng.train_step(0, None, 0, x.shape[0], slot=k)
    eng.sync()
    return (_losses(eng, 0, 4), _state(eng))


def test_linear_steps():
    """4 steps at the golden lin_8_32_b5 geometry: the loss sum of k_mse over its workgroups"""
    _same_bits(_linear_run("lin_8_32_b5"), _linear_run("lin_8_32_b5"), "Linear")


# ---- model API ---------------------------------------------------------------------------------------------------------------

def _saved(folder):
    out = []
    for name in ("encoder.weights", "decoder.weights"):
        sd = torch.load(os.path.join(folder, name), weights_only=True)
        out.extend((f"{name}:{k}", v) for k, v in sd.items())
    with open(os.path.join(folder, "history.json")) as f:
        hist = json.load(f)
    return hist, out


def _same_model(a, b, what):
    (ha, sa), (hb, sb) = a, b
    assert ha == hb, f"{what}: history.json differs: {ha} != {hb}"
    assert [k for k, _ in sa] == [k for k, _ in sb]
    for (name, u), (_, v) in zip(sa, sb):
        assert torch.equal(u, v), f"{what}: {name} differ in {int((u != v).sum())} of {u.numel()} entries"


def test_unet_model_trains_twice_to_the_same_bits(tmp_path):
    """UNET(...).train twice in one process, same seeds, tiny data, 2 epochs (dropout on): the saved state dicts and
    history.json"""
    import io
    from contextlib import redirect_stdout
    from cae_tools_amd.data.arrays import DataArray, Dataset
    from cae_tools_amd.models.unet import UNET, unet_layer_spec

    def data(n, seed):
        rng = np.random.default_rng(seed)
        ds = Dataset()
        ds["lo"] = DataArray((280 + 10 * rng.random((n, 2, 16, 16))).astype(np.float32), dims=("n", "c", "y", "x"))
        ds["hi"] = DataArray((280 + 10 * rng.random((n, 1, 16, 16))).astype(np.float32), dims=("n", "c2", "y", "x"))
        ds["valid"] = DataArray((rng.random((n, 1, 16, 16)) < 0.85).astype(np.float32), dims=("n", "one", "y", "x"))
        return ds

    runs = []
    for r in range(2):
        (train, test) = (data(12, 1), data(4, 2))
        torch.manual_seed(7)
        mt = UNET(batch_size=4, nr_epochs=2, test_interval=1, fc_size=10, encoded_dim_size=4, lr=1e-3, weight_decay=1e-5,
                  dropout_rate=0.1, lambda_pearson=0.5)
        mt.spec = unet_layer_spec(2, 1, (16, 16), [8, 16])
        folder = str(tmp_path / f"run{r}")
        with redirect_stdout(io.StringIO()):
            mt.train(["lo"], "hi", train, test, model_path=folder, mask_variable_name="valid")
        runs.append(_saved(folder))
    _same_model(runs[0], runs[1], "UNET model")


def test_var_model_trains_twice_to_the_same_bits(tmp_path):
    """VarAEModel(...).train twice in one process, same seeds, tiny data (12 x 12 -> 176 x 176), 2 epochs: the saved state
    dicts and history.json"""
    import io
    from contextlib import redirect_stdout
    from cae_tools_amd.data.arrays import DataArray, Dataset
    from cae_tools_amd.models.var_ae_model import VarAEModel

    def data(n, seed):
        rng = np.random.default_rng(seed)
        hi = (285 + 8 * rng.random((n, 1, 176, 176))).astype(np.float32)
        lo = hi[:, :, ::15, ::15][:, :, :12, :12]
        ds = Dataset()
        ds["lowres"] = DataArray(np.ascontiguousarray(lo), dims=("n", "chan", "y", "x"))
        ds["hires"] = DataArray(hi, dims=("n", "chan", "y2", "x2"))
        return ds

    runs = []
    for r in range(2):
        (train, test) = (data(9, 1), data(4, 2))
        torch.manual_seed(3)
        mt = VarAEModel(batch_size=4, nr_epochs=2, test_interval=1, fc_size=12, encoded_dim_size=4, lr=1e-3, weight_decay=1e-5,
                        lambda_mse=1.0, lambda_kl=0.5, lambda_ssim=0.7, noise_seed=6)
        folder = str(tmp_path / f"run{r}")
        with redirect_stdout(io.StringIO()):
            mt.train(["lowres"], "hires", train, test, model_path=folder)
        runs.append(_saved(folder))
    _same_model(runs[0], runs[1], "VarAEModel")
