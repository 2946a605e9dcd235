"""The trunk of the 'var' engine - the ConvAE engine created with variational = true and driven through trunk_forward,
trunk_backward and trunk_adam (engine.hip, trunk_api.h) - against the fp64 definition (oracle/vae_oracle.py), at the branches
only trunk mode reaches: head_plan and tail_plan refuse it, so the middle runs k_down, k_gemm16 and k_gemm16_pair per layer
(its burst variant from 128 outputs on, also into the latent-gradient buffer), k_conv_bwd_pair and k_wgrad; k_reparam and
k_reparam_bwd sit between the Linear layers; the last decoder layer writes its raw output in a TRAINING step (S2_RAW on k_s2_fwd,
k_s2_fwd_cs and k_s2_fwd2, epi_plain on k_up) and takes the gradient of a loss computed outside (the last-layer variants of
k_s2_bwd2, k_s2_bwd and k_ig_bwd_pair); k_vae_loss_grad and k_chan_sums<ACC_GRAD> hand that gradient over.
tests/test_vae_hip_parity.py holds one geometry to the fp32 definition at 5e-3 of the norm; tests/test_vae_msssim_gpu.py
holds the MS-SSIM kernels per pixel.  PARITY UNPINNED with respect to the reference (no source for this model).

CASES lists, per (input, channels, output, channels, fc, latent, batch), the lines of the plan report (VaePlan.kernel_plan =
vae_debug_plan), read from the report and never recomputed.  test_cases_reach_what_they_name (no GPU) checks them against the
report, and that together the cases reach WANT:
- last-layer forward: s2_fwd, s2_fwd_cs and s2_fwd2 with the raw epilogue, up; backward: s2_bwd2, s2_bwd with 2 and with 3
  input channels per thread, ig_bwd_pair; 1, 2, 3, 4 and 5 output channels
- 1, 3 and 4 encoder layers; inner encoder layers none and on k_conv_bwd_pair
- every Linear backward with burst 0 and, but Linear 0 (whose input gradient carries the BatchNorm mask), with burst 1; Linear
  sizes that are multiples of 16 and that are not; one and two row tiles
- head and tail on `layers` with why=variational, in every case
UNREACHABLE lists what no 'var' geometry reaches, with the reason.  The same test holds every case's seed to the window of
relu_fix_for on the oracles alone (the fp32 and the fp64 definition disagree on at most max_flips ReLU decisions, each within
z_tol: its defaults) and its data to a well-conditioned MS-SSIM: every per-scale term of every plane at least MIN_TERM.
Why: a plane's gradient carries the factor w M / f per scale (f: the plane's mean cs or ssim of that scale), the same for
every pixel of the plane.  f is a mean of quotients whose numerators, filter(x y) - mu_x mu_y, are differences of numbers
near 0.25 kept in fp32: each pixel's term is good to ~1e-5 of the typical |cs|, and what of that is systematic stays in the
mean.  A plane whose positive and negative cs regions cancel to an f far below the typical |cs| therefore has a factor
that is off by 1e-5 x typical |cs| / f for the WHOLE plane - nothing that averages out in a weight gradient, and beyond the
criterion's own floor of 1e-5 as soon as f is well below its natural size.  That is the conditioning of the fp32 definition
of the loss, which tests/test_vae_msssim_gpu.py holds per pixel; this file is about the trunk, so its targets keep f at its
natural size: a sample's target is MIX of the fp32 definition's own output for the batch plus 1 - MIX of a sinusoid with
noise (test_vae_msssim_gpu.py mixes half and half and reaches terms of 0.026).

Per case, on the GPU (rows LEAD.. of a data set with spare rows; step 3; vae_helpers.LAMBDAS):
- one forward_backward: the three loss parts and every gradient no further from the fp64 definition than 3x the fp32
  definition is + 1e-5 of the maximum (helpers.assert_close_as_reference at its defaults), both definitions taking the
  engine's ReLU decisions where their own input is within rounding of zero (relu_fix_for); conv biases in front of a
  BatchNorm on magnitude only.  Of the same step: eps bit-equal to normal_noise; z, dL/dz ("vgz") and the heads' gradient
  ("fcgrad" 1) to the same form; dL/d(raw output) ("glast") per pixel against both definitions evaluated AT the engine's own
  y (vae_helpers.assert_planes_close), which holds the sum and the scaling of k_vae_loss_grad itself; the engine's own
  kernel_plan equals the listed report
- base, c2, enc3 (and lin-noburst-long, which runs only so: LEFT_OUT): the same step with lambda_ssim = 0.  Should a tensor
  miss the bound with all three terms on: within the bound here AND glast within its per-pixel bound says MS-SSIM
  backward, otherwise the trunk
- score() and the loss parts of an eval_step against the eval forward of both definitions, same form
- two fresh engines, two train_steps each: the same bits.

Worst |hip - fp64| / bound over the loss parts, the gradients and the intermediates (the tensor it was found on), as each case
printed it on an MI355X - for the next reader; no threshold depends on these:
              base  0.507 (enc/encoder_cnn.1.weight)    glast per pixel 0.326   lambda_ssim = 0: 0.215 (1 - ms_ssim), glast 0.016
                c2  0.456 (dec/decoder_conv.12.bias)    glast per pixel 0.357   lambda_ssim = 0: 0.265 (dec/decoder_lin.0.weight), glast 0.014
            c3-in2  0.412 (enc/encoder_lin.0.weight)    glast per pixel 0.431
                c4  0.435 (1 - ms_ssim)                 glast per pixel 0.616
                c5  0.418 (dec/decoder_conv.10.bias)    glast per pixel 0.928
              enc3  0.518 (enc/encoder_lin.0.weight)    glast per pixel 0.478   lambda_ssim = 0: 0.141 (1 - ms_ssim), glast 0.015
              enc4  0.439 (enc/encoder_cnn.4.bias)      glast per pixel 0.387
        lin-ragged  0.480 (1 - ms_ssim)                 glast per pixel 0.551
   lin-heads-burst  0.646 (dec/decoder_conv.10.weight)  glast per pixel 0.649
  lin-noburst-long  (LEFT_OUT)                                                  lambda_ssim = 0: 0.306 (1 - ms_ssim), glast 0.015
                b1  0.867 (dL/dz)                       glast per pixel 0.254
              wide  0.291 (dec/decoder_conv.0.weight)   glast per pixel 0.418
score() and the eval loss parts: at most 0.39 (an MS-SSIM part), score() itself 0.011 .. 0.013 everywhere.  eps was bit-equal in
every case, and no case needed a ReLU decision followed.
Time on an MI355X, both definitions on 8 CPU threads: the whole file 9 s; `wide`, the only large case (1.7 M output pixels),
2.0 s for its training step with both definitions, 0.6 s for scoring and eval - nothing of it is left out.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from helpers import assert_close_as_reference, bn_bias_keys, hip_relu_decisions, relu_fix_for
from vae_helpers import LAMBDAS, assert_planes_close

(LR, WD, SEED, STEP) = (1e-3, 1e-5, 7, 3)
LEAD = 2    # rows of the data set ahead of the batch
SPARE = 1   # ... and behind it
MIX = 0.85       # share of the definition's own output in a target (module docstring)
MIN_TERM = 0.25  # smallest per-scale MS-SSIM term a case's data may have: a quarter of a perfect match's 1
PERM7 = [4, 0, 6, 2, 5, 1, 3]
PARTS = ("mse", "kl", "1 - ms_ssim")

HEAD_TAIL = ("head fwd=layers why=variational", "tail bwd=layers why=variational")
_IG1 = "ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=1 ig_per=32 ig_dgroup=8 ig_wn8=1"
_ROWS = ("fwd=s2_fwd_rows<8,4,1,2> bwd=s2_bwd_rows<8,2,4,3,3,4,2,1>", "fwd=s2_fwd_rows<4,2,2,1> bwd=s2_bwd_rows<4,4,2,3,3,2,1,3>")
_LAST1 = "fwd=s2_fwd<2,1,4,4,64> epi=raw bwd=s2_bwd2<2,1,4,4,64>"


def _ctb(groups):
    return f"ct_bwd_lds ctb_kernel=band ctb_imgs=1 ctb_groups={groups} ctb_parts=5 ctb_bands=5 ctb_hb=2 ctb_sharded=1"


def _fc(b3, b2, b1):
    """the four Linear backwards, last first: burst of Linear 3, 2 and 1 (Linear 0 never)"""
    return tuple(f"fc{i} bwd=pair burst={b}" for (i, b) in ((3, b3), (2, b2), (1, b1), (0, 0)))


def _thin(dec0, groups, fc, last=_LAST1):
    """the five-layer decoder of a one-channel 176-row output: 32->16 (dec0), 16->8 on the band kernel, 8->4 and 4->2 on the row
    kernels, 2->1"""
    return (f"dec0 fwd=ct_fwd_lds<{dec0}> bwd={_IG1}", f"dec1 fwd=ct_fwd_lds<3,3> bwd={_ctb(groups)}", "dec2 " + _ROWS[0],
            "dec3 " + _ROWS[1], "dec4 " + last) + fc + ("enc conv0=own inner=-",)


# id, inp (H, W), ch input channels, out (H, W), oc output channels, fc / latent, batch, seed, plan: the report's lines but
# HEAD_TAIL, which every case has
Case = namedtuple("Case", "id inp ch out oc fc latent batch seed plan")

CASES = [
    # one encoder layer; 32->16 with 4x3 taps on ct_fwd_lds / ig_bwd_pair; last 2->1 on s2_fwd raw / s2_bwd2's last-layer variant;
    # the last bias gradient inside k_vae_loss_grad; Linear 3 has 640 outputs: burst
    Case("base", (12, 12), 1, (176, 192), 1, 16, 6, 3, 2000, _thin("4,3", 3, _fc(1, 0, 0))),
    # last 4->2: s2_fwd_cs with the raw epilogue in a training step, s2_bwd<4,2,2,4,4>'s last-layer variant; bias via k_chan_sums
    Case("c2", (12, 12), 1, (176, 256), 2, 16, 6, 3, 2010, (
        f"dec0 fwd=ct_fwd_lds<4,3> bwd={_IG1}",
        "dec1 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=4 ig_per=32 ig_dgroup=8 ig_wn8=1",
        "dec2 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=2 ig_tpw=1 ig_chunks=16 ig_per=32 ig_dgroup=4 ig_wn8=2",
        "dec3 fwd=s2_fwd_rows<8,4,1,1> bwd=s2_bwd_rows<8,2,4,3,3,4,1,1>",
        "dec4 fwd=s2_fwd_cs<4,2,4,4,64> epi=raw bwd=s2_bwd<4,2,2,4,4>") + _fc(0, 0, 0) + ("enc conv0=own inner=-",)),
    # last 6->3: s2_fwd raw (256 / 3: no channel split), s2_bwd with 3 channels per thread; two input channels into k_down / k_wgrad
    # (208x208: LEFT_OUT)
    Case("c3-in2", (12, 12), 2, (208, 208), 3, 16, 6, 3, 2020, (
        f"dec0 fwd=ig_fwd_s2 bwd={_IG1}",
        "dec1 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=4 ig_per=32 ig_dgroup=8 ig_wn8=1",
        "dec2 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=15 ig_per=32 ig_dgroup=8 ig_wn8=2",
        "dec3 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=2 ig_tpw=1 ig_chunks=61 ig_per=32 ig_dgroup=4 ig_wn8=8",
        "dec4 fwd=s2_fwd<6,3,4,4,64> epi=raw bwd=s2_bwd<6,3,3,4,4>") + _fc(0, 0, 0) + ("enc conv0=own inner=-",)),
    # last 8->4: s2_fwd_cs raw, s2_bwd<8,2,...>; the first decoder layers are wider (128->64 on the gather forward) (208x208: LEFT_OUT)
    Case("c4", (12, 12), 1, (208, 208), 4, 16, 6, 2, 2030, (
        f"dec0 fwd=ig_fwd_s2 bwd={_IG1}",
        "dec1 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=3 ig_per=32 ig_dgroup=8 ig_wn8=1",
        "dec2 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=10 ig_per=32 ig_dgroup=8 ig_wn8=2",
        "dec3 fwd=ig_fwd_s2 bwd=ig_bwd_pair ig_ksplit=2 ig_tpw=1 ig_chunks=41 ig_per=32 ig_dgroup=4 ig_wn8=6",
        "dec4 fwd=s2_fwd_cs<8,4,4,4,64> epi=raw bwd=s2_bwd<8,2,4,4,4>") + _fc(0, 0, 0) + ("enc conv0=own inner=-",)),
    # 10->5 is no S2 shape: the last layer on k_up with the plain epilogue and on ig_bwd_pair as the LAST layer; ragged
    # 16-channel tiles (160, 80, 40, 20, 10 channels)
    Case("c5", (12, 12), 1, (176, 176), 5, 16, 6, 2, 2040, (
        f"dec0 fwd=ig_fwd_s2 bwd={_IG1}",
        "dec1 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=2 ig_per=32 ig_dgroup=8 ig_wn8=1",
        "dec2 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=7 ig_per=32 ig_dgroup=8 ig_wn8=1",
        "dec3 fwd=ig_fwd_s2 bwd=ig_bwd_pair ig_ksplit=2 ig_tpw=1 ig_chunks=29 ig_per=32 ig_dgroup=4 ig_wn8=4",
        "dec4 fwd=up bwd=ig_bwd_pair ig_ksplit=2 ig_tpw=1 ig_chunks=119 ig_per=32 ig_dgroup=4 ig_wn8=15") + _fc(0, 0, 0)
        + ("enc conv0=own inner=-",)),
    # three encoder layers: k_conv_bwd_pair twice, k_wgrad on layer 0; a 1x1 map into the six-layer decoder
    Case("enc3", (32, 32), 1, (176, 176), 1, 16, 6, 3, 2050, (
        f"dec0 fwd=ct_fwd_lds<4,4> bwd={_IG1}", f"dec1 fwd=ct_fwd_lds<4,4> bwd={_IG1}", f"dec2 fwd=ct_fwd_lds<3,3> bwd={_ctb(3)}",
        "dec3 " + _ROWS[0], "dec4 " + _ROWS[1], "dec5 " + _LAST1) + _fc(0, 0, 0) + ("enc conv0=own inner=pair",)),
    # the benchmark's (cfg5) encoder and Linear sizes at the smallest output: four encoder layers; Linear 2 (128 outputs) on the
    # burst variant, storing into the latent-gradient buffer
    Case("enc4", (64, 64), 1, (176, 176), 1, 128, 32, 2, 2060, (
        f"dec0 fwd=ct_fwd_lds<4,4> bwd={_IG1}", f"dec1 fwd=ct_fwd_lds<4,4> bwd={_IG1}", f"dec2 fwd=ct_fwd_lds<3,3> bwd={_ctb(2)}",
        "dec3 " + _ROWS[0], "dec4 " + _ROWS[1], "dec5 " + _LAST1) + _fc(0, 1, 0) + ("enc conv0=own inner=pair",)),
    # heads of 10 columns, 17 rows: two row tiles, no Linear size a multiple of 16 (50, 20, 10, 5, 512 is Linear 3's alone)
    Case("lin-ragged", (12, 12), 1, (176, 176), 1, 20, 5, 17, 2070, (
        "dec0 fwd=ct_fwd_lds<4,4> bwd=ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=3 ig_per=32 ig_dgroup=8 ig_wn8=1",)
        + _thin("4,4", 17, _fc(1, 0, 0))[1:]),
    # the heads have 128 outputs: the burst variant on Linear 1's input gradient, with the ReLU-mask epilogue; Linear 2 with K = 160
    Case("lin-heads-burst", (12, 12), 1, (176, 176), 1, 160, 64, 3, 2080, _thin("4,4", 3, _fc(1, 1, 1))),
    # Linear 2 has 644 outputs, (644 / 4 + 3) / 4 = 41 k-steps per wave > kBurstSteps: the long contraction on the plain pair kernel
    # (its training step runs without the MS-SSIM term only: LEFT_OUT)
    Case("lin-noburst-long", (12, 12), 1, (176, 176), 1, 644, 6, 3, 2090, _thin("4,4", 3, _fc(1, 0, 0))),
    # one row, picked by a permutation from a 7-row data set: gathered rows, BatchNorm over one sample
    Case("b1", (12, 12), 1, (176, 192), 1, 16, 6, 1, 2100, _thin("4,3", 1, _fc(1, 0, 0))),
    # 22 x 44 x 108 = 104 544 >= 100 000 threads: the last layer on s2_fwd2 with the raw epilogue - the only large case
    Case("wide", (12, 12), 1, (176, 432), 1, 16, 6, 22, 2110, (
        "dec0 fwd=ct_fwd_lds<4,4> bwd=ig_bwd_pair ig_ksplit=4 ig_tpw=1 ig_chunks=9 ig_per=32 ig_dgroup=8 ig_wn8=2",
        "dec1 fwd=ct_fwd_lds<3,3> bwd=ig_bwd_pair ig_ksplit=2 ig_tpw=1 ig_chunks=45 ig_per=32 ig_dgroup=4 ig_wn8=6",
        "dec2 fwd=s2_fwd_rows<8,4,1,1> bwd=s2_bwd_rows<8,2,4,3,3,4,1,1>",
        "dec3 fwd=s2_fwd<4,2,3,3,64> epi=raw_stats bwd=s2_bwd2<4,2,3,3,64>",
        "dec4 fwd=s2_fwd2<2,1,4,4,64> epi=raw bwd=s2_bwd2<2,1,4,4,64>") + _fc(0, 0, 0) + ("enc conv0=own inner=-",)),
]
_IDS = [c.id for c in CASES]
SSIM_OFF = ("base", "c2", "enc3", "lin-noburst-long")   # the cases that run with lambda_ssim = 0 (the last one: only so, LEFT_OUT)
# What is left out, with what it measured on an MI355X.  At 176x176 the coarsest MS-SSIM scale is 11x11 and its valid region ONE
# position, so the plane-wide factor w M / f of that scale (module docstring) hangs on the rounding of a single quotient whose
# variances are differences of numbers near 0.25 over a denominator near c2 = 9e-4: one draw of an error of up to 0.25 * 6e-8 /
# 9e-4 = 2e-5 of the plane's gradient, on the device as in the fp32 definition, and the criterion then compares one such draw
# with three times another.  Every gradient of the three met assert_close_as_reference at 176x176 (worst 0.58, 0.90, 0.88);
# dL/d(raw output) missed the per-pixel bound around the image centre, where that scale weighs most.  c3-in2 and c4 therefore
# run at 208x208 (13x13, nine valid positions) on the same last-layer kernels; c5, enc3, enc4 and the other Linear cases stay
# at 176x176.  lin-noburst-long missed at 208x208 too (a BatchNorm weight at 1.33, with the MS-SSIM term alone 0.91, without it
# 0.23: the conditioning of the MS-SSIM gradient, not the trunk), so its training step runs without the MS-SSIM term only.
LEFT_OUT = {
    "c3-in2 at 176x176": "dL/d(raw output) |hip - fp64| / bound 1.39 (plane 2, row 84, col 81; 346 pixels over); runs at 208x208",
    "c4 at 176x176": "dL/d(raw output) |hip - fp64| / bound 1.05 (plane 6, row 95, col 95; 113 pixels over); runs at 208x208",
    "lin-noburst-long with the MS-SSIM term": "176x176: dL/d(raw output) 1.18 (plane 0, row 97, col 90; 455 pixels over); 208x208: "
                                              "dec/decoder_conv.10.weight 1.33; runs with lambda_ssim = 0",
}
WINDOW_BATCH = {"wide": 3}          # the batch at which the no-GPU test checks a case's ReLU window, where not the case's own

WANT = ({("last fwd", s) for s in ("s2_fwd raw", "s2_fwd_cs raw", "s2_fwd2 raw", "up")}
        | {("last bwd", s) for s in ("s2_bwd2", "s2_bwd ct 2", "s2_bwd ct 3", "ig_bwd_pair")}
        | {("output channels", n) for n in (1, 2, 3, 4, 5)} | {("enc layers", n) for n in (1, 3, 4)}
        | {("inner", "-"), ("inner", "pair")}
        | {(f"fc{i} burst", b) for i in (1, 2, 3) for b in (0, 1)} | {("fc0 burst", 0)}
        | {("linear sizes", "multiples of 16"), ("linear sizes", "ragged"), ("linear row tiles", 1), ("linear row tiles", 2)})

# what no 'var' geometry reaches: (item in WANT's terms) -> reason
UNREACHABLE = {
    ("last fwd tile width", 16): "an MS-SSIM output is at least 176 wide: 88 quads, 44 thread columns of k_s2_fwd2 - choose_s2_fwd takes 64",
    ("last fwd tile width", 32): "as for 16",
    ("last taps", "not 4x4"): "the output's height and width are multiples of 16, so even: a stride-2 layer without padding ends on an "
                              "even size only with an even kernel, and the sizer's kernels are 3 or 4",
    ("conv0", "adam"): "enc_conv0_in_adam_ok needs the inputs that only the fused head publishes, and head_plan refuses the trunk",
    ("fc0 burst", 1): "Linear 0's input gradient carries the BatchNorm mask epilogue, which the burst variant does not have",
}


@pytest.fixture(autouse=True)
def _oracle_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _spec(c):
    from cae_tools_amd.models.model_sizer import create_model_spec
    return create_model_spec(input_size=c.inp, input_channels=c.ch, output_size=c.out, output_channels=c.oc)


def _parse(lines):
    """report lines -> the dict kernel_plan returns"""
    plan = {}
    for line in lines:
        (name, *fields) = line.split()
        plan[name] = dict(f.split("=", 1) for f in fields)
    return plan


def _listed(c):
    return _parse(HEAD_TAIL + c.plan)


def _reached(cases):
    """what `cases` reach, in WANT's terms, read from the plan report; every listed line is checked against the report"""
    from cae_tools_amd.vae_engine import VaePlan
    reached = set()
    for c in cases:
        spec = _spec(c).save()
        p = VaePlan(spec, c.fc, c.latent, c.batch)
        try:
            plan = p.kernel_plan(c.batch, True)
        finally:
            p.close()
        assert plan == _listed(c), (c.id, plan)
        assert plan["head"] == {"fwd": "layers", "why": "variational"} and plan["tail"] == {"bwd": "layers", "why": "variational"}, c.id
        (enc, dec) = (spec["input_layers"], spec["output_layers"])
        last = plan[f"dec{len(dec) - 1}"]
        (fwd, _, targs) = last["fwd"].partition("<")
        reached.add(("last fwd", fwd + (" " + last["epi"] if "epi" in last else "")))
        if targs:
            (ci, co, kh, kw, tw) = map(int, targs.rstrip(">").split(","))
            reached.add(("last fwd tile width", tw))
        k = dec[-1]["kernel_size"]
        reached.add(("last taps", "4x4" if k in (4, [4, 4], (4, 4)) else "not 4x4"))
        (bwd, _, targs) = last["bwd"].partition("<")
        reached.add(("last bwd", bwd + (" ct " + targs.split(",")[1] if bwd == "s2_bwd" else "")))
        reached |= {("output channels", c.oc), ("enc layers", len(enc)), ("inner", plan["enc"]["inner"]), ("conv0", plan["enc"]["conv0"])}
        for i in range(4):
            assert plan[f"fc{i}"]["bwd"] == "pair", c.id
            reached.add((f"fc{i} burst", int(plan[f"fc{i}"]["burst"])))
        sizes = (c.fc, c.latent, 2 * c.latent)
        if all(s % 16 == 0 for s in sizes):
            reached.add(("linear sizes", "multiples of 16"))
        if all(s % 16 for s in sizes) and c.batch % 16:
            reached.add(("linear sizes", "ragged"))
        reached.add(("linear row tiles", -(-c.batch // 16)))
    return reached


def _rows(c):
    """the data set's row count, the permutation (None: rows in order) and the sample indices of the batch"""
    if c.id == "b1":
        return 7, PERM7, [PERM7[LEAD + b] for b in range(c.batch)]
    return LEAD + c.batch + SPARE, None, list(range(LEAD, LEAD + c.batch))


def _hyper(lambdas):
    return dict(lambdas, seed=SEED, lr=LR, weight_decay=WD)


def _oracles(spec, enc_sd, dec_sd, lambdas=LAMBDAS):
    """the fp32 and the fp64 definition at step STEP"""
    from oracle import vae_oracle as vo
    out = []
    for dt in (None, torch.float64):
        o = vo.VaeOracle(spec.save(), enc_sd, dec_sd, dtype=dt, **_hyper(lambdas))
        o.step_count = STEP
        out.append(o)
    return out


@functools.lru_cache(maxsize=None)
def _model(i, batch=None):
    """spec, initial state, data set and the batch's sample indices of case i (at another batch: for the ReLU window of `wide`);
    a sample's target is MIX of the fp32 definition's training-mode output for the batch and 1 - MIX of a sinusoid with noise"""
    from cae_tools_amd.models.decoder import Decoder
    from cae_tools_amd.models.var_ae_model import VarEncoder
    from vae_helpers import synthetic_pair
    c = CASES[i] if batch is None else CASES[i]._replace(batch=batch)
    spec = _spec(c)
    torch.manual_seed(c.seed)
    enc = VarEncoder(spec.get_input_layers(), c.latent, c.fc)
    dec = Decoder(spec.get_output_layers(), c.latent, c.fc)
    (n, perm, idx) = _rows(c)
    g = torch.Generator().manual_seed(c.seed + 1)
    x = torch.rand((n, c.ch) + tuple(c.inp), generator=g)
    (_, t) = synthetic_pair(c.out, n, c.oc, c.seed + 2)
    (enc_sd, dec_sd) = (enc.state_dict(), dec.state_dict())
    with torch.no_grad():
        y = _oracles(spec, enc_sd, dec_sd)[0].forward(x[idx], True)[0]
    t[idx] = (MIX * y + (1 - MIX) * t[idx]).clamp(0, 1)
    return spec, enc_sd, dec_sd, x, t, perm, idx


def test_cases_reach_what_they_name():
    """every case's plan is what CASES lists (VaePlan.kernel_plan, no GPU); together the cases reach WANT and nothing of
    UNREACHABLE; and on every case's seed the two definitions alone respect the window of relu_fix_for, with every per-scale
    MS-SSIM term of every plane at least MIN_TERM"""
    from oracle import vae_oracle as vo
    reached = _reached(CASES)
    assert WANT <= reached, sorted(map(str, WANT - reached))
    assert not reached & set(UNREACHABLE), sorted(map(str, reached & set(UNREACHABLE)))
    assert not WANT & set(UNREACHABLE)
    for (i, c) in enumerate(CASES):
        (spec, enc_sd, dec_sd, x, t, perm, idx) = _model(i, WINDOW_BATCH.get(c.id))
        xb = x[idx]
        (o32, o64) = _oracles(spec, enc_sd, dec_sd)
        (z32, z64) = (o32.relu_inputs(xb), o64.relu_inputs(xb.double()))
        relu_fix_for(o32, xb, {k: v > 0 for k, v in z64.items()}, f"{c.id}: fp32 definition against the fp64 definition's decisions")
        relu_fix_for(o64, xb.double(), {k: v > 0 for k, v in z32.items()}, f"{c.id}: fp64 definition against the fp32 definition's decisions")
        with torch.no_grad():
            y = o64.forward(xb.double(), True)[0]
        terms = vo.per_scale_terms(y, t[idx].double())
        assert float(terms.min()) >= MIN_TERM, f"{c.id}: a per-scale MS-SSIM term is {float(terms.min()):.4f} < {MIN_TERM}"


# ---- on the GPU -------------------------------------------------------------------------------------------------------------

class _TrunkView:
    """what helpers.hip_relu_decisions reads of an engine, served by VaeEngine.trunk_read"""

    def __init__(self, eng):
        (self.enc_layers, self.dec_layers, self.fc_size) = (eng.enc_layers, eng.dec_layers, eng.fc_size)
        self.debug_read = lambda what, index=0, count=None: eng.trunk_read(what, index, count)


def _engine(i, lambdas=LAMBDAS):
    from cae_tools_amd.vae_engine import VaeEngine
    c = CASES[i]
    (spec, enc_sd, dec_sd, x, t, perm, idx) = _model(i)
    eng = VaeEngine(spec, c.fc, c.latent, c.batch, device="cuda:0")
    eng.load_state(enc_sd, dec_sd)
    eng.set_hyper(**_hyper(lambdas))
    eng.set_step(STEP)
    eng.set_dataset(0, x, t)
    return eng, (None if perm is None else eng.upload_perm(perm))


def _ratio(got, ref32, exact64):
    """|got - exact| over assert_close_as_reference's bound (its default factor and floors)"""
    (got, ref32, exact64) = (np.asarray(a, dtype=np.float64) for a in (got, ref32, exact64))
    bound = 3.0 * float(np.abs(ref32 - exact64).max()) + 1e-5 * float(np.abs(exact64).max()) + 1e-9
    return float(np.abs(got - exact64).max()) / bound


def _glast_definition(y, t, lambdas, dtype):
    """dL/d(raw output) of the definition at a given sigmoid output y (B, C, H, W): (lambda_mse 2 (y - t) / n + d(lambda_ssim (1 -
    MS-SSIM)) / dy) y (1 - y), planes (B * C, H, W) in `dtype`"""
    from oracle import vae_oracle as vo
    y = y.detach().to(dtype).requires_grad_(True)
    zero = torch.zeros((1, 1), dtype=dtype)
    (mse, _, ssim) = vo.loss_parts(y, t.to(dtype), zero, zero)
    (g,) = torch.autograd.grad(lambdas["lambda_mse"] * mse + lambdas["lambda_ssim"] * ssim, y)
    yd = y.detach()
    return (g * yd * (1 - yd)).flatten(0, 1).numpy()


def _training_step(i, lambdas, what):
    """one forward_backward of case i against both definitions; returns the worst ratios, largest first"""
    from oracle import vae_oracle as vo
    from test_head_tail_shapes_gpu import _decisions_for
    c = CASES[i]
    (spec, enc_sd, dec_sd, x, t, perm, idx) = _model(i)
    (B, L) = (c.batch, c.latent)
    (xb, tb) = (x[idx], t[idx])
    (eng, perm_dev) = _engine(i, lambdas)
    assert eng.kernel_plan(B, True) == _listed(c), (what, eng.kernel_plan(B, True))
    flat = eng.forward_backward(0, perm_dev, LEAD, B, slot=1).cpu().numpy()
    parts = eng.read_losses(1, 1)[0]
    assert np.isfinite(flat).all(), what
    got = {n: flat[off:off + numel].reshape(shape) for n, (arena, off, numel, shape) in eng.tensors.items() if arena == 0}
    decisions = hip_relu_decisions(_TrunkView(eng), B)
    shape = (B * c.oc,) + tuple(c.out)
    mid = {"z": eng.debug_read("z", (B, L)), "dL/dz": eng.trunk_read("vgz", count=B * L).reshape(B, L),
           "dL/dheads": eng.trunk_read("fcgrad", 1, count=B * 2 * L).reshape(B, 2 * L)}
    (eps, y, glast) = (eng.debug_read("eps", (B, L)), eng.debug_read("y", shape), eng.trunk_read("glast", count=int(np.prod(shape))).reshape(shape))
    eng.close()
    # the noise is the hash's, bit for bit
    assert np.array_equal(eps, vo.normal_noise(SEED, STEP, (B, L))), f"{what}: eps differs from normal_noise"
    ref = []
    for (o, name, cast) in zip(_oracles(spec, enc_sd, dec_sd, lambdas), ("fp32", "fp64"), (lambda a: a, lambda a: a.double())):
        (fix, _) = relu_fix_for(o, cast(xb), _decisions_for(o, cast(xb), decisions, spec.save()), f"{what} {name} definition")
        trace = {}
        (p, _) = o.loss_and_grads(cast(xb), cast(tb), trace=trace, relu_fix=fix)
        (mu, logvar, z) = trace["heads"]
        ref.append((p, o.grads(), {"z": z.detach().numpy(), "dL/dz": z.grad.numpy(), "dL/dheads": torch.cat([mu.grad, logvar.grad], dim=1).numpy()}))
    ((p32, g32, m32), (p64, g64, m64)) = ref
    noisy = bn_bias_keys(spec.save())
    ratios = {part: _ratio([parts[j]], [p32[j]], [p64[j]]) for j, part in enumerate(PARTS)}
    ratios.update({k: _ratio(got[k], g32[k].numpy(), g64[k].numpy()) for k in g32 if k not in noisy})
    ratios.update({k: _ratio(mid[k], m32[k], m64[k]) for k in mid})
    # dL/d(raw output) per pixel, both definitions at the engine's own y: the network's rounding does not enter
    yt = torch.from_numpy(y).view((B, c.oc) + tuple(c.out))
    (gl32, gl64) = (_glast_definition(yt, tb, lambdas, dt) for dt in (torch.float32, torch.float64))
    top = sorted(((r, k) for k, r in ratios.items()), reverse=True)
    print(f"\n[vae trunk] {what}: worst |hip-fp64|/bound {top[0][0]:.3f} ({top[0][1]}), next {[(round(r, 3), k) for r, k in top[1:3]]}")
    ratios["glast"] = assert_planes_close(glast, gl32, gl64, what + " dL/d(raw output)")
    print(f"[vae trunk] {what}: worst per-pixel |glast-fp64|/bound {ratios['glast']:.3f}")
    for j, part in enumerate(PARTS):
        assert_close_as_reference([parts[j]], [p32[j]], [p64[j]], f"{what} {part}")
    np.testing.assert_allclose(parts[3], sum(lambdas["lambda_" + n] * parts[j] for j, n in enumerate(("mse", "kl", "ssim"))), rtol=1e-9)
    for k in mid:
        assert_close_as_reference(mid[k], m32[k], m64[k], f"{what} {k}")
    for k in g32:
        if k in noisy:
            # exactly zero in exact arithmetic: magnitude only
            assert np.abs(got[k]).max() <= 1e-6 + 1e-4 * float(g32[k].abs().max()), f"{what} {k}"
            continue
        assert_close_as_reference(got[k], g32[k].numpy(), g64[k].numpy(), f"{what} {k}")
    return top


_FULL = [i for (i, c) in enumerate(CASES) if c.id != "lin-noburst-long"]


@pytest.mark.gpu
@pytest.mark.parametrize("i", _FULL, ids=[_IDS[i] for i in _FULL])
def test_training_step_against_fp64_definition(i):
    _training_step(i, LAMBDAS, CASES[i].id)


@pytest.mark.gpu
@pytest.mark.parametrize("i", [_IDS.index(s) for s in SSIM_OFF], ids=SSIM_OFF)
def test_training_step_without_the_msssim_term(i):
    """the trunk apart from the conditioning of the MS-SSIM gradient (module docstring)"""
    _training_step(i, dict(LAMBDAS, lambda_ssim=0.0), CASES[i].id + " lambda_ssim=0")


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=_IDS)
def test_scoring_and_eval_step_against_fp64_definition(i):
    c = CASES[i]
    (spec, enc_sd, dec_sd, x, t, perm, idx) = _model(i)
    (xb, tb) = (x[idx], t[idx])
    (o32, o64) = _oracles(spec, enc_sd, dec_sd)
    (eng, perm_dev) = _engine(i)
    y = eng.score(xb.cuda()).cpu().numpy()
    (y32, y64) = (o32.eval_forward(xb).numpy(), o64.eval_forward(xb.double()).numpy())
    eng.eval_step(0, perm_dev, LEAD, c.batch, slot=2)
    parts = eng.read_losses(2, 1)[0]
    eng.close()
    (p32, p64) = (o32.eval_losses(xb, tb), o64.eval_losses(xb.double(), tb.double()))
    ratios = {part: _ratio([parts[j]], [p32[j]], [p64[j]]) for j, part in enumerate(PARTS)}
    ratios["score"] = _ratio(y, y32, y64)
    print(f"\n[vae trunk] {c.id} eval: |hip-fp64|/bound {({k: round(v, 3) for k, v in ratios.items()})}")
    assert_close_as_reference(y, y32, y64, f"{c.id} score()")
    for j, part in enumerate(PARTS):
        assert_close_as_reference([parts[j]], [p32[j]], [p64[j]], f"{c.id} eval {part}")


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=_IDS)
def test_two_runs_of_two_steps_give_the_same_bits(i):
    c = CASES[i]
    runs = []
    for _ in range(2):
        (eng, perm_dev) = _engine(i)
        for (slot, start) in enumerate((LEAD, 0)):
            eng.train_step(0, perm_dev, start, c.batch, slot=slot)
        losses = eng.read_losses(0, 2)
        eng.sync()
        runs.append((losses, eng.params.cpu(), eng.exp_avg.cpu(), eng.exp_avg_sq.cpu(), eng.buffers.cpu()))
        eng.close()
    (a, b) = runs
    assert a[0] == b[0], ("losses", a[0], b[0])
    for (u, v, name) in zip(a[1:], b[1:], ("params", "exp_avg", "exp_avg_sq", "running statistics")):
        assert torch.equal(u, v), f"{c.id}: {name} differ in {int((u != v).sum())} of {u.numel()} entries"
