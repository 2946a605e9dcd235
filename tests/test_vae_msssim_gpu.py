"""The MS-SSIM loss kernels of the 'var' path (kernels_vae.h: k_pool_pyramid, k_ssim_fwd_rows[_multi], k_ssim_bwd_rows[_multi],
k_ssim_combine, k_msssim_finalize, k_vae_loss_grad, and the tile kernels of kernel mode 0) against the fp64 definition, pixel
by pixel.  The engine's own sigmoid output y is read back (vae_debug_read "y") and the fp32 and fp64 definitions
(oracle/vae_oracle.py loss_parts_and_ssim_grad) are evaluated AT that y, so no ReLU decision of the network can differ between
the sides; the device's d(lambda_ssim (1 - MS-SSIM)) / dy ("gssim") is then held, per (batch, channel) plane, to

    max|gssim - g64| <= 3 max|g32 - g64| + 1e-5 max|g64|        (vae_helpers.assert_planes_close)

and the loss parts, z and the last layer's bias gradient to the same form (helpers.assert_close_as_reference).
tests/test_vae_msssim_criterion_cpu.py shows what this bound catches that the weight-gradient bound of
tests/test_vae_hip_parity.py does not.  PARITY UNPINNED with respect to the reference (no source for this model).

Targets: a sample's target is half the fp32 definition's own training-mode output for the batch it is in and half
test_vae_hip_parity._setup's sinusoid, so that every per-scale term of every plane is positive (asserted on the fp64 side: a
plane with a term <= 0 has a zero gradient and would test nothing; that branch has its own test below).

Worst |gssim - fp64| / bound over the planes, one run on an MI355X (row-streaming kernels / tile kernels):
  176x176 0.49 / 0.54   176x256 0.36 / 0.36   176x432 0.26 / 0.26   416x176 0.38 / 0.39   208x240 0.32 / 0.32
  176x256-c2 0.56 / 0.57   176x176-c3-in2 0.91 / 0.92 (its smallest per-scale term is 0.026: kappa = w M / f amplifies f's rounding)
  gather-perm 0.41 / 0.40   gather-start 0.56 / 0.55   gather-batch1 0.77 / 0.77
Before the kernels took the definition's own window values (kernels_vae.h make_gauss: libm's expf and a sequential sum gave a
window one ulp off in seven entries whose sum was 7.5e-8 larger) the same run gave 0.57 .. 2.78, over 1 in seven of the ten
cases and alike in both kernel modes, and every MS-SSIM loss part lay 1.1e-5 .. 1.3e-5 above fp64 (the fp32 definition: 3e-7)."""
import numpy as np
import pytest
import torch

from helpers import assert_close_as_reference
from vae_helpers import GEOMETRIES, LAMBDAS, assert_planes_close

pytestmark = pytest.mark.gpu

(FC, LATENT, SEED, STEP) = (16, 6, 4, 3)

# id -> (output size, in_ch, out_ch, samples in the data set, max_batch, batch, start, shuffled perm)
CASES = {"%dx%d" % s: (s, 1, 1, 3, 3, 3, 0, False) for s in GEOMETRIES}
CASES.update({
    "176x256-c2": ((176, 256), 1, 2, 3, 3, 3, 0, False),
    "176x176-c3-in2": ((176, 176), 2, 3, 3, 3, 3, 0, False),
    "gather-perm": ((176, 256), 1, 2, 7, 4, 3, 2, True),        # samples perm[2:5] of 7, max_batch 4
    "gather-start": ((176, 256), 1, 2, 7, 4, 3, 2, False),      # samples 2, 3, 4
    "gather-batch1": ((176, 256), 1, 2, 7, 4, 1, 5, True),      # the single sample perm[5]
})
PERM7 = [4, 0, 6, 2, 5, 1, 3]


def _make(case_id, last_layer_gain=1.0, mix=0.5):
    """model, data set and the batch's sample indices; targets mixed with the fp32 definition's output (module docstring)"""
    from oracle import vae_oracle as vo
    from test_vae_hip_parity import _setup
    (size, in_ch, out_ch, n, max_batch, batch, start, shuffled) = CASES[case_id]
    (spec, enc, dec, x, t) = _setup((12, 12), size, FC, LATENT, n, seed=21, in_ch=in_ch, out_ch=out_ch)
    (enc_sd, dec_sd) = (enc.state_dict(), dec.state_dict())
    if last_layer_gain != 1.0:
        k = "decoder_conv.%d.weight" % (3 * (len(spec.get_output_layers()) - 1))
        dec_sd[k] = dec_sd[k] * last_layer_gain
    perm = PERM7 if shuffled else None
    idx = [(perm[start + b] if perm else start + b) for b in range(batch)]
    hyper = dict(LAMBDAS, seed=SEED)
    o = vo.VaeOracle(spec.save(), enc_sd, dec_sd, **hyper)
    o.step_count = STEP
    with torch.no_grad():
        y_cpu = o.forward(x[idx], True)[0]
    t = t.clone()
    t[idx] = (mix * y_cpu + (1 - mix) * t[idx]).clamp(0, 1)
    return dict(spec=spec, enc=enc_sd, dec=dec_sd, x=x, t=t, perm=perm, idx=idx, hyper=hyper, max_batch=max_batch, batch=batch,
                start=start, size=size, out_ch=out_ch)


def _encoder_sides(c):
    """({dtype: (mu, logvar)} of the batch in training mode: the encoder of the definition in fp32 and in fp64; the noise)"""
    from oracle import vae_oracle as vo
    out = {}
    eps = vo.normal_noise(SEED, STEP, (c["batch"], LATENT))
    for dt in (torch.float32, torch.float64):
        o = vo.VaeOracle(c["spec"].save(), c["enc"], c["dec"], dtype=dt, **c["hyper"])
        with torch.no_grad():
            (mu, logvar) = vo.encoder_forward(c["spec"].save(), o.enc, c["x"][c["idx"]].to(dt), True)
        out[dt] = (mu, logvar)
    return out, eps


def _run(c, mode, t=None):
    """one forward_backward in kernel mode `mode`: (engine, flat gradient, loss parts, y, gssim)"""
    from test_vae_hip_parity import _engine
    eng = _engine(c["spec"], _as_modules(c["enc"]), _as_modules(c["dec"]), FC, LATENT, c["max_batch"], **c["hyper"])
    eng.set_kernel_mode(mode)
    eng.set_dataset(0, c["x"], c["t"] if t is None else t)
    return (eng,) + _step(eng, c)


class _as_modules:
    """test_vae_hip_parity._engine takes modules; a state dict in their place"""

    def __init__(self, sd):
        self.sd = sd

    def state_dict(self):
        return self.sd


def _step(eng, c):
    eng.set_step(STEP)
    perm = None if c["perm"] is None else eng.upload_perm(c["perm"])
    flat = eng.forward_backward(0, perm, c["start"], c["batch"], slot=0).cpu()
    shape = (c["batch"] * c["out_ch"],) + tuple(c["size"])
    return flat, np.array(eng.read_losses(0, 1)[0]), eng.debug_read("y", shape), eng.debug_read("gssim", shape)


def _definition_at(c, y, t, sides):
    """{dtype: (parts, g as (P, H, W) numpy)} of the definition at the device's y and the batch's targets"""
    from oracle import vae_oracle as vo
    yt = torch.from_numpy(y).view((c["batch"], c["out_ch"]) + tuple(c["size"]))
    out = {}
    for dt in (torch.float32, torch.float64):
        (parts, g) = vo.loss_parts_and_ssim_grad(yt, t[c["idx"]], sides[dt][0], sides[dt][1], c["hyper"]["lambda_ssim"], dt)
        out[dt] = (parts, g.flatten(0, 1).numpy())
    return yt, out


def _check_bias_gradient(c, eng, flat, yt, t, ref, what):
    """the last layer's bias gradient = sum over (b, h, w) of du, du = (lambda_mse 2 (y - t) / n + g) y (1 - y): through
    k_vae_loss_grad's own sum for one channel, through the k_chan_sums launch for more"""
    name = "dec/decoder_conv.%d.bias" % (3 * (len(c["spec"].get_output_layers()) - 1))
    (arena, off, numel, _) = eng.tensors[name]
    got = flat[off:off + numel].numpy()
    sums = {}
    for dt in (torch.float32, torch.float64):
        (yv, tv) = (yt.to(dt), t[c["idx"]].to(dt))
        g = torch.from_numpy(ref[dt][1]).view_as(yv)
        du = (c["hyper"]["lambda_mse"] * 2 * (yv - tv) / yv.numel() + g) * yv * (1 - yv)
        sums[dt] = du.sum(dim=(0, 2, 3)).numpy()
    assert_close_as_reference(got, sums[torch.float32], sums[torch.float64], what + " last-layer bias gradient")


@pytest.mark.parametrize("case_id", list(CASES))
def test_msssim_gradient_per_pixel(case_id):
    from oracle import vae_oracle as vo
    torch.set_num_threads(8)
    c = _make(case_id)
    (sides, eps) = _encoder_sides(c)
    (f32, f64) = (torch.float32, torch.float64)
    ref = y_of_ref = None
    for mode in (1, 0):
        what = f"{case_id} mode {mode}"
        (eng, flat, parts, y, gssim) = _run(c, mode)
        if ref is None or not np.array_equal(y, y_of_ref):       # (both modes leave the same y: one reference serves both)
            (yt, ref) = _definition_at(c, y, c["t"], sides)
            y_of_ref = y
            terms = vo.per_scale_terms(yt.double(), c["t"][c["idx"]].double())
            assert float(terms.min()) > 0, f"{what}: a per-scale term is <= 0: the plane's gradient is zero and tests nothing"
        ratio = assert_planes_close(gssim, ref[f32][1], ref[f64][1], what + " gssim")
        print(f"\n[msssim] {what}: worst |gssim - fp64| / bound = {ratio:.3f}; loss parts hip {parts[:3]}, fp64 {ref[f64][0]}")
        for i, part in enumerate(("mse", "kl", "1 - ms_ssim")):
            assert_close_as_reference(parts[i], ref[f32][0][i], ref[f64][0][i], f"{what} {part}")
        # the reparameterised sample: the noise is the hash's (both sides round an fp64 Box-Muller to fp32: one ulp), and z
        # follows the encoder of the definition with the fp32 noise the kernel drew, cast up
        e_dev = eng.debug_read("eps", (c["batch"], LATENT))
        np.testing.assert_allclose(e_dev, eps, rtol=1.2e-7, atol=0)
        z = {dt: (mu + torch.from_numpy(e_dev).to(dt) * torch.exp(0.5 * lv)).numpy() for dt, (mu, lv) in sides.items()}
        assert_close_as_reference(eng.debug_read("z", (c["batch"], LATENT)), z[f32], z[f64], what + " z")
        _check_bias_gradient(c, eng, flat, yt, c["t"], ref, what)
        assert np.isfinite(flat.numpy()).all(), what


def test_the_target_gather_matters():
    """the gather cases above would pass with the gather ignored if the samples' targets were alike: they are not"""
    c = _make("gather-perm")
    assert c["idx"] == [6, 2, 5]
    assert float((c["t"][c["idx"]] - c["t"][2:5]).abs().max()) > 0.1


@pytest.mark.parametrize("mode", [1, 0])
def test_anticorrelated_plane_takes_the_relu_branch(mode):
    """k_msssim_finalize's f <= 0 branch: plane 0's target replaced by 1 - y of that plane (anti-correlated at every scale; the
    step is bitwise reproducible, so y repeats) - its gradient is exactly 0, nothing is NaN or Inf, it adds exactly 1 to the
    mean of the loss part, and the other planes meet the per-pixel bound"""
    from oracle import vae_oracle as vo
    torch.set_num_threads(8)
    (f32, f64) = (torch.float32, torch.float64)
    # a flat y has local variance below C2 / 2 = 4.5e-4 and cs stays positive: raise the last layer's gain until the definition,
    # on its own output, sees plane 0 anti-correlated at all five scales and the other planes (whose targets follow their y)
    # still correlated, both with a margin; the device's y decides below.  The other planes' margin is a matter of
    # conditioning, not of sign alone: kappa_s = w_s M / f_s turns a rounding error d of the scalar f_s into d / f_s of the whole
    # plane's gradient, and the ratio of two implementations' errors in ONE scalar is not held by any factor; the cases of
    # test_msssim_gradient_per_pixel have every term above 0.02, so that is asked here too (targets 0.8 y + 0.2 sinusoid: the
    # raised gain saturates y and lowers the other planes' terms).  (176 x 176: the coarsest scale's single window spans
    # the whole map, so it sees the output's large-scale variance; the wider maps' coarse scales stayed positive up to gain 256.)
    for gain in (1.0, 1.5, 2.0, 2.5, 3.0, 4.0):
        c = _make("176x176", last_layer_gain=gain, mix=0.8)
        o = vo.VaeOracle(c["spec"].save(), c["enc"], c["dec"], dtype=f64, **c["hyper"])
        o.step_count = STEP
        with torch.no_grad():
            y_cpu = o.forward(c["x"][c["idx"]].double(), True)[0]
        t_cpu = c["t"][c["idx"]].double()
        t_cpu[0, 0] = 1 - y_cpu[0, 0]
        terms = vo.per_scale_terms(y_cpu, t_cpu).flatten(1)
        if float(terms[:, 0].max()) < -0.05 and float(terms[:, 1:].min()) > 0.02:
            break
    else:
        pytest.fail("no gain made plane 0 anti-correlated at every scale with the other planes correlated")
    (sides, _) = _encoder_sides(c)
    (eng, _, _, y, _) = _run(c, mode)
    shape = y.shape
    t2 = c["t"].clone()
    t2[0, 0] = torch.from_numpy(1 - y[0])
    eng.set_dataset(0, c["x"], t2)
    (flat, parts, y2, gssim) = _step(eng, c)
    np.testing.assert_array_equal(y2, y)
    (yt, ref) = _definition_at(c, y2, t2, sides)
    terms = vo.per_scale_terms(yt.double(), t2[c["idx"]].double()).flatten(1)
    assert float(terms[:, 0].max()) < 0, f"plane 0 does not enter the branch at every scale: {terms[:, 0]}"
    assert float(terms[:, 1:].min()) > 0, "another plane enters it as well"
    assert np.isfinite(gssim).all() and np.isfinite(flat.numpy()).all()
    assert np.all(gssim[0] == 0.0)
    assert np.all(ref[f32][1][0] == 0.0) and np.all(ref[f64][1][0] == 0.0)
    ratio = assert_planes_close(gssim, ref[f32][1], ref[f64][1], f"anti-correlated, mode {mode}", skip=(0,))
    print(f"\n[msssim] anti-correlated plane, mode {mode}, gain {gain}: other planes' worst ratio {ratio:.3f}; terms {terms[:, 0].tolist()}")
    assert_close_as_reference(parts[2], ref[f32][0][2], ref[f64][0][2], "1 - ms_ssim with an anti-correlated plane")
    # plane 0 contributes exactly 1 to the mean over the planes
    others = 1 - torch.prod(terms[:, 1:] ** vo.scale_weights(f64).view(-1, 1), dim=0)
    assert abs(ref[f64][0][2] - (1.0 + float(others.sum())) / shape[0]) <= 1e-12
