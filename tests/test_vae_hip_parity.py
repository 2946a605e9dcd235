"""'var' path (include/cae_vae.h) against the build's own CPU definition (oracle/vae_oracle.py).  PARITY UNPINNED with
respect to the reference: it has no source for this model (see the oracle's header); these tests pin the HIP kernels to
the published definition only.

What this file is for: the loss parts at three sets of lambdas, three free-running Adam steps, the benchmark geometry, the
geometry errors and the two MS-SSIM kernel modes against each other.  Its gradient bound (5e-3 of a tensor's L2 norm, 2e-2 of
its maximum, against the fp32 definition, one geometry) is a smoke check: the gradients are held to the fp64 definition, at
every branch the trunk's planners take, in tests/test_vae_trunk_shapes_gpu.py (tests/test_vae_trunk_criterion_cpu.py shows
what passes the bound here and fails there), the MS-SSIM kernels per pixel in tests/test_vae_msssim_gpu.py."""
import numpy as np
import pytest
import torch

from helpers import assert_close_as_reference

pytestmark = pytest.mark.gpu

PARTS = ("mse", "kl", "1 - ms_ssim")


def _setup(in_size, out_size, fc, latent, B, seed, in_ch=1, out_ch=1):
    from cae_tools_amd.models.decoder import Decoder
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.models.var_ae_model import VarEncoder
    spec = create_model_spec(input_size=in_size, input_channels=in_ch, output_size=out_size, output_channels=out_ch)
    torch.manual_seed(seed)
    enc = VarEncoder(spec.get_input_layers(), latent, fc)
    dec = Decoder(spec.get_output_layers(), latent, fc)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand((B, in_ch) + tuple(in_size), generator=g)
    yy, xx = np.meshgrid(np.linspace(-1, 1, out_size[0]), np.linspace(-1, 1, out_size[1]), indexing="ij")
    t = torch.stack([torch.from_numpy((0.5 + 0.4 * np.sin(3 * yy * (b + 1) + 2 * xx)).astype(np.float32))[None].repeat(out_ch, 1, 1)
                     for b in range(B)])
    t = (t + 0.03 * torch.randn(t.shape, generator=g)).clamp(0, 1)
    return spec, enc, dec, x, t


def _engine(spec, enc, dec, fc, latent, B, **hyper):
    from cae_tools_amd.vae_engine import VaeEngine
    eng = VaeEngine(spec, fc, latent, B, device="cuda:0")
    eng.load_state(enc.state_dict(), dec.state_dict())
    eng.set_hyper(**hyper)
    return eng


def _grad_dict(eng, flat):
    flat = flat.cpu()
    return {n: flat[off:off + numel].view(shape) for n, (arena, off, numel, shape) in eng.tensors.items() if arena == 0}


def _feeds_batchnorm(key, last_bias):
    """conv biases (module index 3i) that are followed by a BatchNorm: their exact gradient is 0"""
    if not key.endswith(".bias") or key == last_bias or not ("encoder_cnn." in key or "decoder_conv." in key):
        return False
    return int(key.split(".")[1]) % 3 == 0


@pytest.mark.parametrize("lambdas", [(1.0, 1.0, 1.0), (0.5, 0.1, 2.0), (1.0, 0.0, 0.0)])
def test_losses_and_gradients_match_the_definition(lambdas):
    from oracle import vae_oracle as vo
    (fc, latent, B) = (16, 6, 3)
    (spec, enc, dec, x, t) = _setup((12, 12), (176, 192), fc, latent, B, seed=5)
    hyper = dict(lambda_mse=lambdas[0], lambda_kl=lambdas[1], lambda_ssim=lambdas[2], seed=9)
    o = vo.VaeOracle(spec.save(), enc.state_dict(), dec.state_dict(), **hyper)
    o64 = vo.VaeOracle(spec.save(), enc.state_dict(), dec.state_dict(), dtype=torch.float64, **hyper)
    o.step_count = o64.step_count = 4
    eng = _engine(spec, enc, dec, fc, latent, B, **hyper)
    eng.set_step(4)
    eng.set_dataset(0, x, t)
    # eval: z = mu, running statistics
    np.testing.assert_allclose(eng.score(x).cpu().numpy(), o.eval_forward(x).numpy(), rtol=0, atol=1e-5)
    eng.eval_step(0, None, 0, B, slot=2)
    want = o.eval_losses(x, t)
    got = eng.read_losses(2, 1)[0]
    np.testing.assert_allclose(got[:3], want, rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(got[3], lambdas[0] * want[0] + lambdas[1] * want[1] + lambdas[2] * want[2], rtol=2e-5)
    want64 = o64.eval_losses(x.double(), t.double())
    for i, part in enumerate(PARTS):      # no further from fp64 than 3 x the fp32 definition's own error (+ 1e-5 relative)
        assert_close_as_reference(got[i], want[i], want64[i], "eval " + part)
    # train: reparameterised sample with the shared noise hash
    g = _grad_dict(eng, eng.forward_backward(0, None, 0, B, slot=0))
    (parts, _) = o.loss_and_grads(x, t)
    np.testing.assert_allclose(eng.read_losses(0, 1)[0][:3], parts, rtol=3e-5, atol=1e-7)
    (parts64, _) = o64.loss_and_grads(x.double(), t.double())
    for i, part in enumerate(PARTS):
        assert_close_as_reference(eng.read_losses(0, 1)[0][i], parts[i], parts64[i], "train " + part)
    last_bias = "dec/decoder_conv.%d.bias" % (3 * (len(spec.get_output_layers()) - 1))
    for k, w in o.grads().items():
        (gv, wv) = (g[k].numpy().astype(np.float64), w.numpy().astype(np.float64))
        if _feeds_batchnorm(k, last_bias):
            assert np.abs(gv).max() < 2e-5 and np.abs(wv).max() < 2e-5, k       # bias in front of a BatchNorm: exactly 0
            continue
        assert np.linalg.norm(gv - wv) <= 5e-3 * max(np.linalg.norm(wv), 1e-9), k
        assert np.abs(gv - wv).max() <= 2e-2 * max(np.abs(wv).max(), 1e-7), k


def test_adam_steps_follow_the_definition():
    from oracle import vae_oracle as vo
    (fc, latent, B) = (12, 4, 4)
    (spec, enc, dec, x, t) = _setup((12, 12), (176, 176), fc, latent, B, seed=8)
    init = {pre + k: v.detach().clone().numpy() for (pre, m) in (("enc/", enc), ("dec/", dec)) for k, v in m.state_dict().items()}
    o = vo.VaeOracle(spec.save(), enc.state_dict(), dec.state_dict(), lr=1e-3, weight_decay=1e-5, seed=2)
    eng = _engine(spec, enc, dec, fc, latent, B, lr=1e-3, weight_decay=1e-5, seed=2)
    eng.set_dataset(0, x, t)
    want = [o.train_step(x, t) for _ in range(3)]
    for i in range(3):
        eng.train_step(0, None, 0, B, slot=i)
    got = eng.read_losses(0, 3)
    np.testing.assert_allclose(np.array(got)[:, :3], np.array(want), rtol=5e-3, atol=1e-6)
    (e_sd, d_sd) = eng.export_state()
    ref = o.state()
    # ... a bound an optimiser that does nothing meets as well.  So, as test_adam_steps_free_running (tests/test_hip_parity.py)
    # asks of the ConvAE's free-running steps: 99 % of every parameter tensor within a tenth of that bound, which a tensor that
    # did not move (every weight three rates from the definition's) misses five times over.  Not held to it: a bias in front
    # of a BatchNorm, whose gradient is rounding noise that Adam turns into steps of +-lr.
    # Why a quantile and no maximum.  Measured on an MI355X against the same three steps of the definition in fp64: 26 of the 27
    # tensors lie within 3x the fp32 definition's own distance + 3e-6 (the per-step Adam criterion of tests/test_hip_parity.py,
    # summed over three steps), most within 3x alone; dec/decoder_conv.0.weight has one element 1.48e-5 from fp64 where the fp32
    # definition's worst is 1.9e-6 (bound 8.8e-6), of a movement of 3.0e-3.  Adam's update is lr m / (sqrt(v) + eps), and where
    # a gradient of rounding size changes sign between steps |m| / sqrt(v) is decided by the rounding of the gradient: the
    # error of such an element goes as 1 / |g|, the maximum over a tensor is that of a heavy-tailed sample, and two fp32
    # evaluations differ in it by more than any fixed factor.  The lines below print both figures and the bias-corrected
    # |m| / sqrt(v) of the fp64 definition at the worst element: 1 for a steady gradient, 0.13 at that element, 0.42 - 1 at the
    # other tensors' worst.  The optimiser kernels' own arithmetic is held element by element in
    # tests/test_optim_elementwise_gpu.py.
    o64 = vo.VaeOracle(spec.save(), enc.state_dict(), dec.state_dict(), lr=1e-3, weight_decay=1e-5, seed=2, dtype=torch.float64)
    for _ in range(3):
        o64.train_step(x.double(), t.double())
    ref64 = o64.state()
    last_bias = "dec/decoder_conv.%d.bias" % (3 * (len(spec.get_output_layers()) - 1))
    bound = 3 * 2.1e-3                                                           # 3 Adam steps of lr 1e-3
    for (pre, sd, params64) in (("enc/", e_sd, o64.enc), ("dec/", d_sd, o64.dec)):
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == 3
                continue
            d = np.abs(v.numpy() - ref[pre + k].numpy()).reshape(-1)
            assert d.max() <= bound, k
            if "running_" in k or _feeds_batchnorm(pre + k, last_bias):
                continue
            start = init[pre + k].astype(np.float64)
            (moved, want32, want64) = (a.numpy().astype(np.float64) - start for a in (v, ref[pre + k], ref64[pre + k]))
            worst = int(np.abs(moved - want64).argmax())
            st = o64.optim.state[params64[k]]
            steady = float(st["exp_avg"].reshape(-1)[worst].abs() / st["exp_avg_sq"].reshape(-1)[worst].sqrt())
            steady *= (1 - 0.999 ** 3) ** 0.5 / (1 - 0.9 ** 3)                   # the bias corrections of step 3
            print(f"[vae adam] {pre + k}: movement {float(np.abs(want64).max()):.3e}, |hip - fp64| {float(np.abs(moved - want64).max()):.3e}, "
                  f"the fp32 definition's own {float(np.abs(want32 - want64).max()):.3e}, |m| / sqrt(v) there {steady:.3f}, "
                  f"99 % of |hip - fp32| below {float(np.quantile(d, 0.99)):.3e}")
            assert np.quantile(d, 0.99) <= 0.1 * bound, pre + k


def test_benchmark_geometry_cfg5():
    """BASELINE cfg5: 64x64 -> 512x512, 1 channel: loss parts and the MS-SSIM gradient at full size (batch 2)"""
    from oracle import vae_oracle as vo
    torch.set_num_threads(8)
    (fc, latent, B) = (128, 32, 2)
    (spec, enc, dec, x, t) = _setup((64, 64), (512, 512), fc, latent, B, seed=13)
    o = vo.VaeOracle(spec.save(), enc.state_dict(), dec.state_dict(), seed=3)
    eng = _engine(spec, enc, dec, fc, latent, B, seed=3)
    eng.set_dataset(0, x, t)
    g = _grad_dict(eng, eng.forward_backward(0, None, 0, B, slot=0))
    (parts, _) = o.loss_and_grads(x, t)
    np.testing.assert_allclose(eng.read_losses(0, 1)[0][:3], parts, rtol=5e-5, atol=1e-7)
    k = "dec/decoder_conv.%d.weight" % (3 * (len(spec.get_output_layers()) - 1))
    (gv, wv) = (g[k].numpy().astype(np.float64), o.grads()[k].numpy().astype(np.float64))
    assert np.linalg.norm(gv - wv) <= 1e-2 * np.linalg.norm(wv)


def test_benchmark_geometry_cfg5_at_the_stated_batch():
    """BASELINE cfg5 at its STATED batch, 16 (the test above runs batch 2): loss parts against the definition at batch 16,
    eval rows equal to the same rows scored at batch 2 (eval mode is per sample), finite gradients, and one Adam step on the
    batch lowers its loss.  PARITY UNPINNED with respect to the reference (no source for this model), like this whole file."""
    from oracle import vae_oracle as vo
    torch.set_num_threads(8)
    (fc, latent, B) = (128, 32, 16)
    (spec, enc, dec, x, t) = _setup((64, 64), (512, 512), fc, latent, B, seed=13)
    eng = _engine(spec, enc, dec, fc, latent, B, seed=3, lr=1e-4)
    eng.set_dataset(0, x, t)
    y16 = eng.score(x).cpu().numpy()
    small = _engine(spec, enc, dec, fc, latent, 2, seed=3)
    assert np.abs(y16[:2] - small.score(x[:2]).cpu().numpy()).max() <= 1e-6
    o = vo.VaeOracle(spec.save(), enc.state_dict(), dec.state_dict(), seed=3)
    (parts, _) = o.loss_and_grads(x, t)
    g = _grad_dict(eng, eng.forward_backward(0, None, 0, B, slot=0))
    first = eng.read_losses(0, 1)[0]
    np.testing.assert_allclose(first[:3], parts, rtol=5e-5, atol=1e-7)
    for k, v in g.items():
        assert np.isfinite(v.numpy()).all(), k
    k = "dec/decoder_conv.%d.weight" % (3 * (len(spec.get_output_layers()) - 1))
    (gv, wv) = (g[k].numpy().astype(np.float64), o.grads()[k].numpy().astype(np.float64))
    assert np.linalg.norm(gv - wv) <= 1e-2 * np.linalg.norm(wv)
    # one small Adam step on this batch, then the batch again with the SAME reparameterisation noise (the noise is a hash of
    # (seed, step): the step counter is put back): the training loss went down
    eng.set_step(0)
    eng.train_step(0, None, 0, B, slot=1)
    eng.set_step(0)
    eng.forward_backward(0, None, 0, B, slot=2)
    after = eng.read_losses(2, 1)[0]
    assert sum(after[:3]) < sum(first[:3])


def test_geometry_errors():
    from cae_tools_amd._lib import CaeError
    from cae_tools_amd.models.model_sizer import create_model_spec
    from cae_tools_amd.vae_engine import VaeEngine
    spec = create_model_spec(input_size=(16, 16), input_channels=1, output_size=(100, 100), output_channels=1)
    with pytest.raises(CaeError, match="MS-SSIM"):
        VaeEngine(spec, 8, 4, 2, device="cuda:0")


@pytest.mark.parametrize("shape", [((12, 12), (176, 192), 3), ((64, 64), (512, 512), 2)])
def test_row_streaming_msssim_kernels_equal_the_tile_kernels(shape):
    """vae_set_kernel_mode: the row-streaming MS-SSIM passes (a wave walks a strip of 64 columns; DPP neighbours, register ring)
    perform the tile kernels' arithmetic in the tile kernels' order - every loss part and every gradient agree to fp32 rounding
    (the compiler contracts a few multiply-adds differently in the two kernels: 3e-8 on a loss part).  176x192: strips and bands that end
    inside a wave, five scales down to 11x12; 512x512: the benchmark geometry (ten strips, sixteen bands)."""
    (in_size, out_size, B) = shape
    (fc, latent) = (16, 6)
    (spec, enc, dec, x, t) = _setup(in_size, out_size, fc, latent, B, seed=21)
    out = []
    for mode in (1, 0):
        eng = _engine(spec, enc, dec, fc, latent, B, lambda_mse=0.7, lambda_kl=0.3, lambda_ssim=1.5, seed=4)
        eng.set_kernel_mode(mode)
        eng.set_dataset(0, x, t)
        g = eng.forward_backward(0, None, 0, B, slot=0).cpu().numpy().astype(np.float64)
        out.append((np.array(eng.read_losses(0, 1)[0]), g))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-6)
    scale = np.abs(out[1][1]).max()
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=1e-4, atol=1e-6 * scale)
