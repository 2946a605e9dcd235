"""UNET HIP path (include/cae_unet.h) against the reference-generated vectors (tests/golden/unet_*.npz) and, for
train-mode dropout (whose masks are a hash both sides share), against the pinned CPU oracle."""
import time

import numpy as np
import pytest
import torch

from unet_helpers import (ARGMAX_CAP, ARGMAX_TOL, DEEP_CASES, MEDIUM_CASES, RELU_TOL, TRAIN_CASES, UNET_CASES,  # noqa: F401
                          UnetCase, _against_aligned_oracles, _check_alignment, _grad_dict, feeds_batchnorm, relu_cap, unet_oracle)

pytestmark = pytest.mark.gpu


def _engine(case, max_batch=None, dropout=None, specialised=True, seed=0):
    from cae_tools_amd.unet_engine import UnetEngine
    m = case.meta
    eng = UnetEngine(m["spec"], m["fc"], m["latent"], max_batch or m["batch"], device="cuda:0", specialised=specialised)
    eng.load_state(case.state("init", "enc"), case.state("init", "dec"))
    eng.set_hyper(lr=m["lr"], weight_decay=m["weight_decay"], dropout_rate=m["dropout"] if dropout is None else dropout,
                  lambda_pearson=m["lambda_pearson"], seed=seed)
    return eng


@pytest.mark.parametrize("specialised", [True, False])
@pytest.mark.parametrize("name", UNET_CASES)
def test_eval_forward_and_losses(name, specialised):
    c = UnetCase(name)
    eng = _engine(c, specialised=specialised)
    y = eng.score(c.t("x0")).cpu().numpy()
    np.testing.assert_allclose(y, c.z["eval/y"], rtol=0, atol=5e-6)
    eng.set_dataset(0, c.t("x0"), c.t("t0"), None if c.meta["mask"] == "ones" else c.t("m0"))
    eng.eval_step(0, None, 0, c.z["x0"].shape[0], slot=3)
    (mse, pl) = eng.read_losses(3, 1)[0]
    np.testing.assert_allclose([mse, pl], c.z["eval/losses"], rtol=2e-5)


@pytest.mark.parametrize("specialised", [True, False])
@pytest.mark.parametrize("name", TRAIN_CASES)
def test_train_forward_backward(name, specialised):
    c = UnetCase(name)
    eng = _engine(c, specialised=specialised)
    (x, t, m) = c.step_batch(0)
    eng.set_dataset(0, x, t, None if c.meta["mask"] == "ones" else m)
    m = m if c.meta["mask"] != "ones" else torch.ones_like(m)
    _against_aligned_oracles(eng, c.meta["spec"], c.state("init", "enc"), c.state("init", "dec"), x, t, m,
                             c.meta["fc"], c.meta["latent"], f"{name} (specialised={specialised})",
                             lambda_pearson=c.meta["lambda_pearson"])
    # (the oracle is pinned to the reference's own gradients of this case by tests/test_unet_oracle_golden.py)
    np.testing.assert_allclose(eng.read_losses(0, 1)[0], c.z["step_losses"][0], rtol=2e-5)


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_adamw_steps(name):
    c = UnetCase(name)
    eng = _engine(c)
    nsteps = c.meta["nsteps"]
    losses = []
    for i in range(nsteps):
        (x, t, m) = c.step_batch(i)
        eng.set_dataset(0, x, t, None if c.meta["mask"] == "ones" else m)
        eng.train_step(0, None, 0, x.shape[0], slot=i)
        if i == 0:
            (enc, dec) = eng.export_state()
            for (pre, sd) in (("enc/", enc), ("dec/", dec)):
                for k, v in sd.items():
                    want = c.z["step1/" + pre + k]
                    if k.endswith("num_batches_tracked"):
                        assert int(v) == int(want)
                    elif feeds_batchnorm(pre + k):
                        assert np.abs(v.numpy() - want).max() <= 2.1 * c.meta["lr"], k   # Adam turns noise into +-lr
                    else:
                        # the first AdamW step is lr * g / (|g| + eps) = lr * sign(g) wherever |g| >> eps = 1e-8: entries
                        # whose reference gradient is significant must agree closely, the rest may differ by up to 2*lr
                        diff = np.abs(v.numpy() - want)
                        assert diff.max() <= 2.1 * c.meta["lr"], k
                        if ("grad/" + pre + k) in c.z:
                            sig = np.abs(c.z["grad/" + pre + k]) > 1e-5
                            assert (diff[sig] <= 2e-5 + 1e-4 * np.abs(want).max()).all(), k
                        else:   # running statistics
                            assert diff.max() <= 1e-5 + 1e-4 * np.abs(want).max(), k
    got = eng.read_losses(0, nsteps)
    np.testing.assert_allclose(np.array(got), c.z["step_losses"], rtol=5e-3)


def test_train_dropout_matches_oracle_hash_masks():
    """dropout 0.25 in train mode: the engine and the oracle draw the same hash masks"""
    c = UnetCase("u_k4_b3")
    eng = _engine(c, dropout=0.25, seed=77)
    eng.set_step(5)
    (x, t, m) = c.step_batch(0)
    eng.set_dataset(0, x, t, m)
    _against_aligned_oracles(eng, c.meta["spec"], c.state("init", "enc"), c.state("init", "dec"), x, t, m, c.meta["fc"],
                             c.meta["latent"], "u_k4_b3 dropout 0.25", dropout_rate=0.25, seed=77, step=5,
                             lambda_pearson=c.meta["lambda_pearson"], loss_rtol=2e-5)


def test_permutation_and_partial_batches():
    """samples are gathered through the permutation; a smaller batch than max_batch reuses the workspace"""
    c = UnetCase("u_rect_b4")
    eng = _engine(c, max_batch=4)
    (x, t, m) = c.step_batch(0)
    eng.set_dataset(0, x, t, m)
    perm = eng.upload_perm([2, 0, 3, 1])
    eng.eval_step(0, perm, 1, 3, slot=0)       # samples 0, 3, 1
    o = unet_oracle(c)
    idx = [0, 3, 1]
    want = o.eval_losses(x[idx], t[idx], m[idx])
    np.testing.assert_allclose(eng.read_losses(0, 1)[0], want, rtol=2e-5)


def test_errors():
    from cae_tools_amd._lib import CaeError
    from cae_tools_amd.unet_engine import UnetEngine, UnetPlan
    c = UnetCase("u_k4_b3")
    spec = c.meta["spec"]
    with pytest.raises(CaeError, match="one layer per encoder layer"):
        UnetPlan({"input_layers": spec["input_layers"], "output_layers": spec["output_layers"][:2]}, 8, 4, 2)
    bad = {"input_layers": spec["input_layers"], "output_layers": [dict(l) for l in spec["output_layers"]]}
    bad["output_layers"][1]["input_dimensions"] = [16, 4, 4]
    with pytest.raises(CaeError, match="2 x out_channels"):
        UnetPlan(bad, 8, 4, 2)
    eng = _engine(c)
    with pytest.raises(CaeError, match="not set"):
        eng.eval_step(0, None, 0, 2)
    eng.set_dataset(0, c.t("x0"), c.t("t0"), c.t("m0"))
    with pytest.raises(CaeError, match="outside the data set"):
        eng.eval_step(0, None, 2, 3)
    with pytest.raises(CaeError, match="outside 1"):
        eng.eval_step(0, None, 0, 9)
    # a one-sample TRAINING batch fails in the reference (BatchNorm1d: "Expected more than 1 value per channel")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        eng.train_step(0, None, 0, 1)
    eng.eval_step(0, None, 2, 1, slot=5)          # ... while a one-sample eval batch is fine
    o = unet_oracle(c)
    np.testing.assert_allclose(eng.read_losses(5, 1)[0], o.eval_losses(c.t("x0")[2:3], c.t("t0")[2:3], c.t("m0")[2:3]), rtol=2e-5)


def test_ragged_epoch_matches_oracle_batch_by_batch():
    """an epoch over 7 samples in batches of 3 (3 + 3 + 1 in eval mode; training drops nothing either: 3 + 3 + ... the
    reference's DataLoader has drop_last=False): per-batch loss pairs through run_batches"""
    c = UnetCase("u_rect_b4")
    (x, t, m) = (torch.cat([c.step_batch(i)[k] for i in range(3)]) for k in range(3))     # 4 + 3 + 4 = 11 samples
    (x, t, m) = (x[:7], t[:7], m[:7])
    eng = _engine(c, max_batch=3)
    eng.set_dataset(1, x, t, m)
    perm = eng.upload_perm([6, 2, 5, 0, 4, 1, 3])
    got = eng.run_batches(1, perm, 7, 3, train=False)
    o = unet_oracle(c)
    order = [6, 2, 5, 0, 4, 1, 3]
    want = [o.eval_losses(x[order[i:i + 3]], t[order[i:i + 3]], m[order[i:i + 3]]) for i in (0, 3, 6)]
    np.testing.assert_allclose(np.array(got), np.array(want), rtol=3e-5)


def _against_oracle_and_generic_kernels(in_c, out_c, size, chans, fc, latent, B):
    """one training forward + backward (dropout on) and a scoring pass, specialised and generic kernels, against the fp32
    and fp64 CPU oracles under this run's ReLU and max-pool decisions.  The generic kernels (one fp32 chain per output) are
    held to the same 3x bound as the specialised ones: they meet it on every geometry (worst ratio 0.53 here, 0.63 on the
    golden cases)"""
    from cae_tools_amd.models.unet import Decoder, Encoder, unet_layer_spec
    from cae_tools_amd.unet_engine import UnetEngine
    (h, w) = size
    spec = unet_layer_spec(in_c, out_c, size, chans)
    torch.manual_seed(123)
    enc = Encoder(spec.get_input_layers(), latent, fc)
    dec = Decoder(spec.get_output_layers(), latent, fc)
    g = torch.Generator().manual_seed(9)
    x = torch.rand((B, in_c, h, w), generator=g)
    t = torch.rand((B, out_c, h, w), generator=g)
    m = (torch.rand((B, 1, h, w), generator=g) < 0.85).float()
    res = {}
    for specialised in (True, False):
        eng = UnetEngine(spec, fc, latent, B, device="cuda:0", specialised=specialised)
        eng.load_state(enc.state_dict(), dec.state_dict())
        eng.set_hyper(dropout_rate=0.1, seed=4)
        eng.set_step(2)
        eng.set_dataset(0, x, t, m)
        (o, _, _, _) = _against_aligned_oracles(eng, spec.save(), enc.state_dict(), dec.state_dict(), x, t, m, fc, latent,
                                                f"{chans} {size} B={B} (specialised={specialised})", dropout_rate=0.1, seed=4,
                                                step=2)
        res[specialised] = eng.score(x).cpu().numpy()
    # (o: the last trip's fp32 oracle - like each engine it has seen one training forward, so its running statistics moved once)
    np.testing.assert_allclose(res[True], res[False], rtol=0, atol=2e-5)
    np.testing.assert_allclose(res[True], o.eval_forward(x).numpy(), rtol=0, atol=2e-5)


@pytest.mark.parametrize("size,chans,fc,latent,B", [(c[2][0],) + c[3:] for c in MEDIUM_CASES.values()], ids=list(MEDIUM_CASES))
def test_mfma_path_at_medium_size_against_oracle_and_generic_kernels(size, chans, fc, latent, B):
    """wide layers, odd batch, dropout on: the specialised kernels (image-end layers from an LDS patch with the weights in
    registers, wide layers from a patch with weight tiles, the im2col tile engine for what those do not take, the Linear
    kernels) against the CPU oracle and the generic kernels.  64 px, 32 / 64 / 96 channels: full tiles, a 64-row tile and a
    partly filled 128-row tile, maps 32 / 16 / 8 wide.  128 px, 16 / 32 / 64 / 72 channels: maps 64 ... 8 wide, a 16-channel
    image-end layer, channel counts the patch kernels take (32, 64) next to ones they leave to the tile engine (72)"""
    _against_oracle_and_generic_kernels(3, 3, (size, size), chans, fc, latent, B)


@pytest.mark.parametrize("name", list(DEEP_CASES))
def test_deep_unets_against_oracle_and_generic_kernels(name):
    """deeper and wider-spread UNETs than the cases above, the same checks.  5 levels at 256 px: nine layers with repacked
    weights (two repack launches), the encoder's input gradients on the tile engine and the patch kernels, the thin OpUp at
    the image end.  6 levels at 64 px down to a 1x1 bottleneck: ten repacked layers, attention with one hidden unit,
    weight gradients on the tile engine with fp64 atomics and on the generic kernel (maps 2 and 1 wide).  512 px: the tile
    engine on 256-wide image-end maps, k_up_thin<3> at the output, eight repacked layers (one launch, full).  20x28 with a
    34-channel 5x7 bottleneck: the Linear tile engine (1190 inputs) and the generic OpUp in specialised mode"""
    (in_c, out_c, size, chans, fc, latent, B) = DEEP_CASES[name]
    _against_oracle_and_generic_kernels(in_c, out_c, size, chans, fc, latent, B)


def _cfg3(B, seed):
    from cae_tools_amd.models.unet import Decoder, Encoder, unet_layer_spec
    spec = unet_layer_spec(3, 3, (256, 256), [32, 64, 128, 256])
    torch.manual_seed(11)
    enc = Encoder(spec.get_input_layers(), 32, 128)
    dec = Decoder(spec.get_output_layers(), 32, 128)
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 3, 256, 256), generator=g)
    t = torch.rand((B, 3, 256, 256), generator=g)
    m = (torch.rand((B, 1, 256, 256), generator=g) < 0.9).float()
    return spec, enc, dec, x, t, m


def test_benchmark_geometry_full_size_against_oracle():
    """BASELINE cfg3 layers (3x256x256, channels 32/64/128/256, fc128/latent32) at batch 5: the patch kernels on every wide
    layer, their split-K weight gradients, the thin-layer kernels and the 65536-wide Linear layers at their real sizes against
    the fp32 and fp64 CPU oracles, both following this run's ReLU and max-pool decisions where they cannot decide them (the
    im2col tile engine takes none of these layers: tests/test_unet_plan_cpu.py)
    (not batch 2: BatchNorm1d over two samples maps every feature to +-1 and amplifies fp32 rounding without bound)"""
    from cae_tools_amd.unet_engine import UnetEngine
    t0 = time.time()
    torch.set_num_threads(16)
    (fc, latent, B) = (128, 32, 5)
    (spec, enc, dec, x, t, m) = _cfg3(B, 12)
    eng = UnetEngine(spec, fc, latent, B, device="cuda:0")
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(dropout_rate=0.1, seed=21)
    eng.set_dataset(0, x, t, m)
    (o, _, _, _) = _against_aligned_oracles(eng, spec.save(), enc.state_dict(), dec.state_dict(), x, t, m, fc, latent,
                                            "cfg3 B=5", dropout_rate=0.1, seed=21)
    np.testing.assert_allclose(eng.score(x).cpu().numpy(), o.eval_forward(x).numpy(), rtol=0, atol=3e-5)
    print(f"[unet parity] cfg3 B=5: {time.time() - t0:.0f} s")


def test_benchmark_geometry_at_the_stated_batch():
    """BASELINE cfg3 at its STATED batch, 32 (the test above runs the same layers at batch 5): grid sizes, split-K choices and
    the pressure on the BatchNorm-sum shards change with the batch.  Every gradient against the fp32 and fp64 CPU oracles
    under this run's ReLU and max-pool decisions (dropout off: the reference's arithmetic exactly; the fp32 oracle's graph is
    freed before the fp64 one is built); eval rows equal to the same rows scored at batch 5 (eval mode is per sample); one
    AdamW step on the batch lowers its loss."""
    from cae_tools_amd.unet_engine import UnetEngine
    t0 = time.time()
    torch.set_num_threads(16)
    (fc, latent, B) = (128, 32, 32)
    (spec, enc, dec, x, t, m) = _cfg3(B, 14)
    eng = UnetEngine(spec, fc, latent, B, device="cuda:0")
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(dropout_rate=0.0, seed=21, lr=1e-4)
    eng.set_dataset(0, x, t, m)
    # eval: rows of the batch-32 call == the same rows scored five at a time
    y32 = eng.score(x).cpu().numpy()
    small = UnetEngine(spec, fc, latent, 5, device="cuda:0")
    small.load_state(enc.state_dict(), dec.state_dict())
    y5 = small.score(x[:5]).cpu().numpy()
    assert np.abs(y32[:5] - y5).max() <= 1e-6
    assert np.isfinite(y32).all()
    del small
    # train-mode step at batch 32 against the oracles
    _against_aligned_oracles(eng, spec.save(), enc.state_dict(), dec.state_dict(), x, t, m, fc, latent, "cfg3 B=32")
    first = eng.read_losses(0, 1)[0]
    # one small optimiser step on this batch (first-order regime), then the same batch again: the loss went down
    eng.train_step(0, None, 0, B, slot=1)
    eng.forward_backward(0, None, 0, B, slot=2)
    after = eng.read_losses(2, 1)[0]
    assert after[0] + after[1] < first[0] + first[1]
    print(f"[unet parity] cfg3 B=32: {time.time() - t0:.0f} s")


def test_mfma_path_non_square_odd_channel_counts():
    """96x160 maps, channels 16 / 40 / 72 (every tile shape partly filled), 2 -> 5 channels, batch 3, per-channel mask"""
    from cae_tools_amd.models.unet import Decoder, Encoder, unet_layer_spec
    from cae_tools_amd.unet_engine import UnetEngine
    spec = unet_layer_spec(2, 5, (96, 160), [16, 40, 72])
    (fc, latent, B) = (20, 7, 3)
    torch.manual_seed(31)
    enc = Encoder(spec.get_input_layers(), latent, fc)
    dec = Decoder(spec.get_output_layers(), latent, fc)
    g = torch.Generator().manual_seed(32)
    x = torch.rand((B, 2, 96, 160), generator=g)
    t = torch.rand((B, 5, 96, 160), generator=g)
    m = (torch.rand((B, 5, 96, 160), generator=g) < 0.8).float()
    eng = UnetEngine(spec, fc, latent, B, device="cuda:0")
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(dropout_rate=0.0)
    eng.set_dataset(0, x, t, m)
    (o, _, _, _) = _against_aligned_oracles(eng, spec.save(), enc.state_dict(), dec.state_dict(), x, t, m, fc, latent,
                                            "96x160 16-40-72 B=3")
    np.testing.assert_allclose(eng.score(x).cpu().numpy(), o.eval_forward(x).numpy(), rtol=0, atol=3e-5)
