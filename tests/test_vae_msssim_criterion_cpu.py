"""The per-pixel MS-SSIM criterion of tests/test_vae_msssim_gpu.py (vae_helpers.assert_planes_close: per plane
max|got - fp64| <= 3 x the fp32 definition's own error + 1e-5 of the plane's maximum, on d(lambda_ssim (1 - MS-SSIM)) / dy at a
given y) against the bound tests/test_vae_hip_parity.py holds the weight gradients to (5e-3 of a tensor's L2 norm, 2e-2 of its
largest entry, after the decoder backward has summed the map), on the oracle alone: the fp32 definition passes it at every
geometry of the GPU test, and four stand-ins for subtly wrong MS-SSIM kernels fail it.

Measured (an untrained 12 x 12 -> 176 x 640 network, batch 3, lambdas 0.7 / 0.3 / 1.5; "old" = how far the mutant moves the
last decoder layer's weight gradient, the tensor that sums every pixel of the map, against the old 5e-3 L2 / 2e-2 max):

  mutant                                        per-pixel |mutant - fp64| / bound   old L2    old max   other tensors over the old bound
  seam   (scale 2, valid column 54 dropped)     1955                                2.5e-3    2.8e-3    seven deeper decoder weights, 5.0e-3 .. 8.1e-3 L2
  chain  (scale 4 read at x/8 - 1, last col)    165                                 2.2e-4    2.3e-4    none
  tap 2  (scale 3, window entry 0.036 missing)  698                                 2.3e-2    1.8e-2    most tensors, ~1e-2 L2
  tap 0  (scale 3, window entry 1.0e-3 missing) 20                                  1.2e-3    8.8e-4    the one-element last-layer bias, 6.4e-3
  kappa  (scale 1, H_v (W_v - 1))               23                                  2.4e-3    2.2e-3    none

So: chain, kappa and the outermost tap pass the old bound outright and fail this one 20 to 165 times over; the seam column
is inside the old bound on the last layer (and 2000 times over this one) but sits AT the old L2 bound on deeper decoder
tensors (1.0 .. 1.6 x), and at 176 x 432 - where one column is 1 / 98 of scale 2's width instead of 1 / 150 - the last
layer's weight moves by 6.0e-3 L2, 1.2 x the old bound: the old bound is not blind to it, it is three orders of magnitude less
sharp, and no geometry of the old GPU tests has a backward strip seam at scale 2 except 512 x 512, held to 1e-2 L2 there.  A
missing inner tap (0.036) is caught by both.  The one-element last-layer bias, a sum over the map that cancels to ~1e-3 of its
terms, is the old bound's most sensitive tensor (at 176 x 432 it flags chain at 2.5e-2 of its value, 1.25 x)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vae_helpers import GEOMETRIES, LAMBDAS, assert_planes_close, plane_ratios, synthetic_pair

MUTANT_SIZE = (176, 640)     # scale 2 is 44 x 160: valid width 150, so valid column 54 (the second backward strip's first) exists
(FC, LATENT, B) = (16, 6, 3)


def test_the_kernels_window_is_the_definitions():
    """bit for bit: one ulp in the window moved the device's loss by 1.2e-5 and its gradient past the bound (kernels_vae.h make_gauss)"""
    from cae_tools_amd import _lib
    from oracle import vae_oracle as vo
    w = np.zeros(11, dtype=np.float32)
    _lib.load().vae_gauss_window(w.ctypes.data)
    np.testing.assert_array_equal(w, vo.gaussian_window().numpy())


# ---- (a) the fp32 definition meets its own bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(GEOMETRIES), ids=lambda s: "%dx%d" % s)
def test_fp32_definition_meets_the_criterion(size):
    """ratio <= 1/3 on every plane; and the fp32 definition's own error, which sizes the bound (1e-5 .. 2e-4 of a plane's
    maximum: the variances are differences E[x^2] - E[x]^2 of numbers near 0.25), leaves every plane's bound at least ten times
    tighter than 2e-2 of the maximum, the per-entry bound the weight gradients are held to"""
    from oracle import vae_oracle as vo
    torch.set_num_threads(8)
    (y, t) = synthetic_pair(size, 2, 2, seed=31)
    zero = torch.zeros(2, LATENT)
    (p32, g32) = vo.loss_parts_and_ssim_grad(y, t, zero, zero, LAMBDAS["lambda_ssim"], torch.float32)
    (p64, g64) = vo.loss_parts_and_ssim_grad(y, t, zero, zero, LAMBDAS["lambda_ssim"], torch.float64)
    assert g32.dtype == torch.float32 and g64.dtype == torch.float64
    (g32, g64) = (g32.flatten(0, 1).numpy(), g64.flatten(0, 1).numpy())
    assert assert_planes_close(g32, g32, g64, "fp32 definition %dx%d" % size) <= 1 / 3 + 1e-9
    for p, (_, bound, own, scale) in enumerate(plane_ratios(g32, g32, g64)):
        print(f"\n[criterion] {size[0]}x{size[1]} plane {p}: fp32 definition's own error {own / scale:.2e} of the maximum")
        assert bound <= 2e-3 * scale
    assert abs(p32[2] - p64[2]) <= 1e-6 * p64[2]


# ---- (b) mutants: the fp32 definition with one autograd edge changed -----------------------------------------------------
class _GradEdit(torch.autograd.Function):
    """identity whose backward passes the gradient through `edit`"""

    @staticmethod
    def forward(ctx, x, edit):
        ctx.edit = edit
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.edit(g.clone()), None


def _conv_h(a, w):
    c = a.shape[1]
    return F.conv2d(a, w.view(1, 1, 1, -1).repeat(c, 1, 1, 1), groups=c)


def _filter_missing_tap(tap):
    """vae_oracle._filter whose horizontal pass lacks window entry `tap` in its BACKWARD only (the forward value is intact to rounding)"""
    def filt(x, g):
        c = x.shape[1]
        v = F.conv2d(x, g.view(1, 1, -1, 1).repeat(c, 1, 1, 1), groups=c)
        gm = g.clone()
        gm[tap] = 0
        return _conv_h(v.detach(), g) + _conv_h(v, gm) - _conv_h(v.detach(), gm)
    return filt


def _ms_ssim_variant(mutant=None, tap=2):
    """oracle/vae_oracle.py ms_ssim restated with four places a mutant can change (None: the definition itself, bit for bit -
    test_the_restatement_is_the_definition):
      "seam"   valid column 54 of scale 2's maps sends nothing back (a backward strip seam: the second strip's first map column)
      "chain"  the gradient that reaches scale 4's pooled map is read one column to the left in its last column (the pooling
               chain own4(x / 8) of k_ssim_combine read at x / 8 - 1)
      "tap"    window entry `tap` is missing from scale 3's backward filter, horizontal pass
      "kappa"  scale 1's term is divided by H_v (W_v - 1) instead of H_v W_v in the backward"""
    from oracle import vae_oracle as vo

    def ms_ssim(x, y):
        g = vo.gaussian_window(x.dtype)
        (c1, c2) = (vo.K1 ** 2, vo.K2 ** 2)
        terms = []
        last = len(vo.MS_WEIGHTS) - 1
        for s in range(last + 1):
            filt = _filter_missing_tap(tap) if (mutant == "tap" and s == 3) else vo._filter
            if mutant == "chain" and s == 4:
                def shift(gr):
                    gr[..., -1] = gr[..., -2]
                    return gr
                x = _GradEdit.apply(x, shift)
            (mu1, mu2) = (filt(x, g), filt(y, g))
            (s11, s22, s12) = (filt(x * x, g) - mu1 * mu1, filt(y * y, g) - mu2 * mu2, filt(x * y, g) - mu1 * mu2)
            cs_map = (2 * s12 + c2) / (s11 + s22 + c2)
            if mutant == "seam" and s == 2:
                def drop(gr):
                    gr[..., 54] = 0
                    return gr
                cs_map = _GradEdit.apply(cs_map, drop)
            ssim_map = ((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)) * cs_map
            (ssim_c, cs) = (ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1))
            if mutant == "kappa" and s == 1:
                wv = cs_map.shape[-1]
                cs = _GradEdit.apply(cs, lambda gr: gr * (wv / (wv - 1)))
            if s < last:
                terms.append(torch.relu(cs))
                pad = [d % 2 for d in x.shape[2:]]
                x = F.avg_pool2d(x, kernel_size=2, padding=pad)
                y = F.avg_pool2d(y, kernel_size=2, padding=pad)
        terms.append(torch.relu(ssim_c))
        stack = torch.stack(terms, dim=0)
        return torch.prod(stack ** vo.scale_weights(stack.dtype), dim=0).mean()
    return ms_ssim


@pytest.fixture(scope="module")
def case():
    """a whole untrained network at 12 x 12 -> 176 x 432 (test_vae_hip_parity._setup's), its y, and at that y the fp32 and fp64
    definition's map gradient; the fp32 definition's weight gradients are what the old bound compares with"""
    from oracle import vae_oracle as vo
    from test_vae_hip_parity import _setup
    torch.set_num_threads(8)
    (spec, enc, dec, x, t) = _setup((12, 12), MUTANT_SIZE, FC, LATENT, B, seed=21)
    hyper = dict(LAMBDAS, seed=4)
    o = vo.VaeOracle(spec.save(), enc.state_dict(), dec.state_dict(), **hyper)
    (parts, y) = o.loss_and_grads(x, t)
    with torch.no_grad():
        (mu, logvar) = vo.encoder_forward(spec.save(), o.enc, x, True)
    (_, g32) = vo.loss_parts_and_ssim_grad(y, t, mu, logvar, hyper["lambda_ssim"], torch.float32)
    (_, g64) = vo.loss_parts_and_ssim_grad(y, t, mu, logvar, hyper["lambda_ssim"], torch.float64)
    return dict(spec=spec.save(), enc=enc.state_dict(), dec=dec.state_dict(), x=x, t=t, y=y, mu=mu, logvar=logvar, hyper=hyper,
                grads=o.grads(), g32=g32.flatten(0, 1).numpy(), g64=g64.flatten(0, 1).numpy(),
                last_w="dec/decoder_conv.%d.weight" % (3 * (len(spec.get_output_layers()) - 1)))


def _mutant(case, monkeypatch, mutant, **kw):
    """(map gradient at the case's y, weight gradients of the whole network) of the fp32 definition with `mutant` in its MS-SSIM"""
    from oracle import vae_oracle as vo
    monkeypatch.setattr(vo, "ms_ssim", _ms_ssim_variant(mutant, **kw))
    (_, g) = vo.loss_parts_and_ssim_grad(case["y"], case["t"], case["mu"], case["logvar"], case["hyper"]["lambda_ssim"], torch.float32)
    o = vo.VaeOracle(case["spec"], case["enc"], case["dec"], **case["hyper"])
    o.loss_and_grads(case["x"], case["t"])
    monkeypatch.undo()
    return g.flatten(0, 1).numpy(), o.grads()


def _old_sense(case, grads):
    """the weight-gradient bound of test_losses_and_gradients_match_the_definition (5e-3 of the L2 norm, 2e-2 of the maximum) with
    the mutant in the place of the HIP result: (L2 and maximum distance on the last decoder layer's weight - the tensor next to
    the map, every pixel of which it sums - and the names of the other tensors over the bound)"""
    from test_vae_hip_parity import _feeds_batchnorm
    last_bias = case["last_w"].replace(".weight", ".bias")
    (figures, others) = (None, [])
    for k, w in case["grads"].items():
        if _feeds_batchnorm(k, last_bias):
            continue
        (gv, wv) = (grads[k].numpy().astype(np.float64), w.numpy().astype(np.float64))
        (l2, mx) = (np.linalg.norm(gv - wv) / max(np.linalg.norm(wv), 1e-9), np.abs(gv - wv).max() / max(np.abs(wv).max(), 1e-7))
        if k == case["last_w"]:
            figures = (l2, mx)
        elif l2 > 5e-3 or mx > 2e-2:
            others.append(f"{k} ({l2:.1e} L2, {mx:.1e} max)")
    return figures[0], figures[1], others


def _report(case, name, g, grads):
    """prints the measurement; True where the last decoder layer's weight gradient is inside the old bound"""
    ratios = [r for (r, _, _, _) in plane_ratios(g, case["g32"], case["g64"])]
    (l2, mx, others) = _old_sense(case, grads)
    print(f"\n[criterion] {name}: per-pixel |mutant - fp64| / bound = {max(ratios):.1f} (worst plane); last decoder weight gradient "
          f"moves by {l2:.2e} L2 (old bound 5e-3), {mx:.2e} of its maximum (old bound 2e-2); other tensors over the old bound: "
          f"{', '.join(others) or 'none'}")
    return l2 <= 5e-3 and mx <= 2e-2


def test_the_restatement_is_the_definition(case):
    from oracle import vae_oracle as vo
    (y, t) = (case["y"].clone().requires_grad_(True), case["t"])
    (a,) = torch.autograd.grad(vo.ms_ssim(y, t), y)
    (b,) = torch.autograd.grad(_ms_ssim_variant(None)(y, t), y)
    assert torch.equal(a, b)


@pytest.mark.parametrize("mutant", ["seam", "chain"])
def test_seam_and_chain_mutants_fail_the_criterion_but_pass_the_old_one(case, monkeypatch, mutant):
    (g, grads) = _mutant(case, monkeypatch, mutant)
    assert _report(case, mutant, g, grads)       # inside the old bound
    with pytest.raises(AssertionError, match=r"plane \d+ pixel \(row \d+, col \d+\)"):
        assert_planes_close(g, case["g32"], case["g64"], mutant)


@pytest.mark.parametrize("mutant,kw", [("tap", dict(tap=2)), ("tap", dict(tap=0)), ("kappa", {})], ids=["tap2", "tap0", "kappa"])
def test_tap_and_kappa_mutants_fail_the_criterion(case, monkeypatch, mutant, kw):
    """(whether the old bound sees them too is the measurement recorded in the module docstring, not an assertion)"""
    (g, grads) = _mutant(case, monkeypatch, mutant, **kw)
    _report(case, mutant + str(kw.get("tap", "")), g, grads)
    with pytest.raises(AssertionError, match=r"plane \d+ pixel \(row \d+, col \d+\)"):
        assert_planes_close(g, case["g32"], case["g64"], mutant)
