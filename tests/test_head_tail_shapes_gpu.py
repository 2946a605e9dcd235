"""The narrow middle of the ConvAE step against the fp64 oracle, at every branch its host plans can take: the fused kernels
k_head_fwd and k_tail_bwd (kernels_head.h) as head_plan / tail_plan (engine_choose.h) shape them, the input staging
(head_stage_inputs) and the first encoder layer's weight gradient inside the optimiser launch (AdamConv0, kernels_generic.h).
The counterpart of test_ct_bwd_shapes_gpu.py for the encoder side: there every model has a 16x16 one-channel input with
fc 16 / latent 4, here the input, the encoder and the Linear sizes vary and the decoder is two to four thin layers
(create_model_spec(..., output_size=(28, 28), output_channels=1)) that other tests pin.

CASES lists, per (input, channels, kernel, stride, layer count, fc, latent, batch), the `head`, `tail` and `enc` lines of
the plan report (EnginePlan.kernel_plan) and the batch at which the head leaves the fused path.  The splits of the MFMA
stages ("lg:per": 2^lg waves share a tile's k-steps, `per` each) are read from the report, never recomputed here.
test_cases_reach_what_they_name (no GPU) checks every listed field against the report and that the cases together reach (WANT):
- head encoder: 1, 2, 3 and 4 layers; a first layer of 3x3 taps on one input channel, 3x3 on several, 5x5 and 2x2; stride 2
  and 3; 2, 4, 6, 8, 12 and 16 output channels; less than one, one to four and more than four first-layer positions per thread
- head staging and rows: `direct`, `gather4` and `scalar` staging; a batch below 16, of 16, and = 1 mod 16; 1, 2..8 and more
  than 8 row groups; Linear 3 in whole 16-column strips and with a ragged last strip
- head weights and splits: `late` weight pieces 0 and 1; no straddling piece and some; stages with lg 0, 2, 3 and 4; shares of
  at most 4 k-steps (4-deep k-batches) and of more (8-deep); a short last share; waves without a k-step
- tail: chain stages with lg 0, 2, 3 and 4, with a short last share and with empty waves; 2, 4, 8, 12, 16 and 32 channels in
  the BatchNorm sums (32: two passes of the c0 loop; 12: one wave per channel); sums stored and sums added (more than 8 row
  groups); a weight matrix of exactly 2048 float4s (the cap); head and tail fused, fused head with per-layer tail, per-layer
  head with fused tail
- AdamConv0: fewer than 256 positions, 256..4096, more than 4096 (the remainder loop); several input channels; 5x5 and 2x2
  taps; stride 3; a step where it is off because the head is not fused
- REFUSALS (no GPU): every `why=` of both planners that a spec can reach; UNREACHABLE_WHY lists the others with the reason.
The same test holds each case's seed to the window of relu_fix_for on the oracles alone: the fp32 and the fp64 oracle
disagree on at most max_flips ReLU decisions, each within z_tol (its defaults).

Per case, on the GPU (graph=False; rows 3.. of a data set with three more rows, so the cursor is not zero):
- one forward_backward in the default mode and one on the shape-generic kernels (mode 0): loss and every gradient no further
  from the fp64 oracle than 3x the fp32 oracle is (helpers.assert_close_as_reference), both oracles taking the HIP step's
  ReLU decisions where their own input is within rounding of zero (relu_fix_for); conv biases that feed a BatchNorm
  (bn_bias_keys) on magnitude only; score() within 1e-5 of the oracle's eval forward; the default-mode engine's own
  kernel_plan equals the listed report
- the `direct` cases and one `scalar` case: the same step through a device permutation (gather4 staging by permutation)
- every case whose conv-0 weight gradient rides in the optimiser launch, and the 83-batch case where it does not: one
  train_step from zero moments, the gradients recovered from exp_avg (as test_timed_path_gpu.py does), same criterion -
  forward_backward keeps that gradient in its own launch, so only this sees the staged batch copy, the saved gamma and the
  AdamConv0 remainder loop
- two fresh engines, two train_steps each: the same bits.

Worst |hip - fp64| / bound over the loss and the gradients (the tensor it was found on), as each case printed it on an
MI355X - for the next reader; no threshold depends on these:
   16x16x1-k3s2-fc128.64-b20 mode 1: 0.050 (enc/encoder_cnn.0.weight); mode 0: 0.053; permuted: 0.065; train_step: 0.051 (enc/encoder_cnn.0.weight)
    16x16x1-k3s2-fc100.8-b33 mode 1: 0.047 (dec/decoder_conv.1.weight); mode 0: 0.043; permuted: 0.081; train_step: 0.053 (dec/decoder_conv.1.weight)
   16x16x1-k3s2-fc100.16-b16 mode 1: 0.110 (enc/encoder_cnn.1.bias); mode 0: 0.138; permuted: 0.041; train_step: 0.109 (enc/encoder_cnn.1.bias)
   16x16x1-k3s2-fc160.32-b17 mode 1: 0.048 (enc/encoder_cnn.3.weight); mode 0: 0.083; permuted: 0.045; train_step: 0.047 (enc/encoder_cnn.3.weight)
   16x16x1-k3s2-fc128.48-b36 mode 1: 0.080 (enc/encoder_cnn.1.bias); mode 0: 0.049; permuted: 0.099; train_step: 0.080 (enc/encoder_cnn.1.bias)
   16x16x1-k3s2-fc128.32-b76 mode 1: 0.055 (dec/decoder_conv.1.weight); mode 0: 0.063; train_step: 0.047 (dec/decoder_conv.1.weight)
     16x16x1-k3s2-fc16.4-b82 mode 1: 0.059 (enc/encoder_cnn.1.weight); mode 0: 0.039; train_step: 0.057 (enc/encoder_cnn.1.weight)
     16x16x1-k3s2-fc16.4-b83 mode 1: 0.065 (enc/encoder_lin.0.bias); mode 0: 0.065; train_step: 0.064 (enc/encoder_lin.0.bias)
    32x32x1-k3s2-fc128.32-b9 mode 1: 0.108 (enc/encoder_cnn.1.weight); mode 0: 0.108; permuted: 0.077; train_step: 0.106 (enc/encoder_cnn.1.weight)
    32x32x1-k3s2-fc64.16-b17 mode 1: 0.084 (enc/encoder_cnn.1.bias); mode 0: 0.084; train_step: 0.084 (enc/encoder_cnn.1.bias)
     16x16x3-k3s2-fc16.4-b24 mode 1: 0.079 (dec/decoder_conv.1.weight); mode 0: 0.047; train_step: 0.078 (dec/decoder_conv.1.weight)
     21x18x2-k5s2-fc24.8-b25 mode 1: 0.067 (enc/encoder_cnn.1.weight); mode 0: 0.110; train_step: 0.069 (enc/encoder_cnn.1.weight)
      20x20x1-k3s3-fc20.4-b5 mode 1: 0.089 (enc/encoder_cnn.0.weight); mode 0: 0.090; permuted: 0.075; train_step: 0.090 (enc/encoder_cnn.0.weight)
     17x19x1-k3s2-fc16.4-b19 mode 1: 0.059 (dec/decoder_conv.1.weight); mode 0: 0.066; permuted: 0.069; train_step: 0.057 (dec/decoder_conv.1.weight)
     11x9x1-k3s2-fc16.4-b130 mode 1: 0.037 (dec/decoder_conv.1.weight); mode 0: 0.045; train_step: 0.039 (dec/decoder_conv.1.weight)
   18x18x1-k3s2n1-fc16.4-b67 mode 1: 0.321 (enc/encoder_lin.0.bias); mode 0: 0.066; train_step: 0.321 (enc/encoder_lin.0.bias)
   33x33x1-k3s2n1-fc16.4-b11 mode 1: 0.084 (dec/decoder_conv.0.bias); mode 0: 0.025; train_step: 0.086 (dec/decoder_conv.0.bias)
    64x64x1-k3s2n3-fc16.4-b2 mode 1: 0.060 (enc/encoder_cnn.4.bias); mode 0: 0.088; permuted: 0.065; train_step: 0.059 (enc/encoder_cnn.4.bias)
      48x48x1-k2s2-fc16.4-b1 mode 1: 0.147 (enc/encoder_cnn.1.weight); mode 0: 0.087; permuted: 0.122; train_step: 0.149 (enc/encoder_cnn.1.weight)
      48x48x1-k2s2-fc16.4-b2 mode 1: 0.060 (enc/encoder_cnn.4.bias); mode 0: 0.057; permuted: 0.108; train_step: 0.059 (enc/encoder_cnn.4.bias)
      32x32x4-k3s2-fc16.4-b6 mode 1: 0.135 (enc/encoder_cnn.1.weight); mode 0: 0.122
      32x32x2-k3s2-fc16.4-b6 mode 1: 0.080 (enc/encoder_cnn.6.weight); mode 0: 0.067
      9x9x1-k3s2-fc128.32-b7 mode 1: 0.308 (enc/encoder_cnn.1.bias); mode 0: 0.087; train_step: 0.306 (enc/encoder_cnn.1.bias)
Every score() sat within 6e-08 of the oracle's eval forward."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from helpers import assert_close_as_reference, bn_bias_keys, hip_relu_decisions, relu_fix_for

LR, WD = 1e-3, 1e-5
LEAD = 3   # rows of the data set ahead of the batch


def fused(enc, grid, stage, w4, late, straddle, fc0, fc1, fc2, fc3, lds):
    """the `head` line of a fused head: encoder layers, grid (row groups x Linear-3 strips), input staging, weight float4s, late
    pieces, used pieces that straddle two matrices, lg:per of the four Linear stages, LDS bytes"""
    return {"fwd": "fused", "enc": str(enc), "grid": grid, "stage": stage, "w4": str(w4), "late": str(late), "straddle": str(straddle),
            "fc0": fc0, "fc1": fc1, "fc2": fc2, "fc3": fc3, "lds": str(lds)}


def tail(rows, sums, g1, g0, gx, w2, w1, w0, lds):
    """the `tail` line of a fused tail: row groups, BatchNorm sums stored | added, lg:per of the chain stages and of the
    weight-gradient stages, LDS bytes"""
    return {"bwd": "fused", "rows": str(rows), "sums": sums, "g1": g1, "g0": g0, "gx": gx, "w2": w2, "w1": w1, "w0": w0, "lds": str(lds)}


def layers(why, side="fwd"):
    return {side: "layers", "why": why}


# inp (H, W), ch input channels, k kernel size, stride, count input_layer_count (None: the sizer's own depth), fc / latent,
# batch, leaves: the first batch whose head runs on the per-layer kernels (None: at every batch), the head / tail lines,
# conv0: "adam" (weight gradient in the optimiser launch of a train_step) | "own", inner: "pair" | "layers" | "-" (one layer)
Case = namedtuple("Case", "inp ch k stride count fc latent batch leaves head tail conv0 inner")

CASES = [
    # late pieces; head fc1 2:8 on 4 tiles, fc3 4:2; the tail's W1 has exactly 2048 float4s; last row group of 4
    Case((16, 16), 1, 3, 2, None, 128, 64, 20, 50,
         fused(2, "2x2", "direct", 5760, 1, 3, "0:9", "2:8", "0:16", "4:2", 151232),
         tail(2, "stored", "2:8", "0:16", "2:8", "0:4", "0:4", "0:4", 84416), "adam", "pair"),
    # K = 100: 25 k-steps over 16 waves, 2 each: a short last share and 3 empty waves (head fc1, fc3, tail g1); K = 8
    Case((16, 16), 1, 3, 2, None, 100, 8, 33, 77,
         fused(2, "3x2", "direct", 1700, 0, 2, "0:9", "4:2", "0:2", "4:2", 104336),
         tail(3, "stored", "4:2", "0:2", "2:7", "0:4", "0:4", "0:4", 60608), "adam", "pair"),
    # the same splits on exactly one full panel
    Case((16, 16), 1, 3, 2, None, 100, 16, 16, 77,
         fused(2, "1x2", "direct", 2100, 0, 2, "0:9", "4:2", "0:4", "4:2", 101840),
         tail(1, "stored", "4:2", "0:4", "2:7", "0:4", "0:4", "0:4", 60608), "adam", "pair"),
    # late pieces; fc1 3:5 (8-deep k-batches), fc3 4:3 with 2 empty waves, tail gx 2:10
    Case((16, 16), 1, 3, 2, None, 160, 32, 17, 74,
         fused(2, "2x2", "direct", 4640, 1, 3, "0:9", "3:5", "0:8", "4:3", 141200),
         tail(2, "stored", "3:5", "0:8", "2:10", "0:4", "0:4", "0:4", 76224), "adam", "pair"),
    # late pieces; 3 tiles on lg 2 (one idle tile slot)
    Case((16, 16), 1, 3, 2, None, 128, 48, 36, 77,
         fused(2, "3x2", "direct", 4736, 1, 3, "0:9", "2:8", "0:12", "4:2", 145088),
         tail(3, "stored", "2:8", "0:12", "2:8", "0:4", "0:4", "0:4", 71104), "adam", "pair"),
    # the benchmark's model at its last fused batch: gather4 staging by size, 5 row groups
    Case((16, 16), 1, 3, 2, None, 128, 32, 76, 77,
         fused(2, "5x2", "gather4", 3712, 0, 3, "0:9", "3:4", "0:8", "4:2", 154880),
         tail(5, "stored", "3:4", "0:8", "2:8", "0:4", "0:4", "0:4", 65984), "adam", "pair"),
    # the LDS boundary: the last fused batch ...
    Case((16, 16), 1, 3, 2, None, 16, 4, 82, 83,
         fused(2, "6x2", "gather4", 240, 0, 1, "0:9", "0:4", "0:1", "0:4", 155072),
         tail(6, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 32192), "adam", "pair"),
    # ... and the first on the per-layer kernels (conv 0's weight gradient in a launch of its own)
    Case((16, 16), 1, 3, 2, None, 16, 4, 83, 83,
         layers("lds"),
         tail(6, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 32192), "own", "pair"),
    # three encoder layers; fused head, per-layer tail (W0 has 72 * 128 / 4 > 2048 float4s); late pieces
    Case((32, 32), 1, 3, 2, None, 128, 32, 9, 17,
         fused(3, "1x2", "direct", 4864, 1, 3, "0:18", "3:4", "0:8", "4:2", 136352),
         layers("weights", "bwd"), "adam", "pair"),
    # three encoder layers, 8 channels into the tail, last row group of 1, gather4 staging by size
    Case((32, 32), 1, 3, 2, None, 64, 16, 17, 18,
         fused(3, "2x2", "gather4", 1920, 0, 1, "0:18", "0:16", "0:4", "0:16", 152352),
         tail(2, "stored", "0:16", "0:4", "0:16", "0:4", "0:4", "0:4", 58368), "adam", "pair"),
    # a 3x3 first layer on three channels; 6 and 12 output channels (ragged groups of four); fc0 4:2 (27 k-steps: 2 empty waves)
    Case((16, 16), 3, 3, 2, None, 16, 4, 24, 25,
         fused(2, "2x2", "gather4", 528, 0, 1, "4:2", "0:4", "0:1", "0:4", 152784),
         tail(2, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 45632), "adam", "pair"),
    # the non-3x3 branch (5x5) on two channels, one layer, 9x7 maps; fc0 3:8 (63 k-steps: a short last share)
    Case((21, 18), 2, 5, 2, None, 24, 8, 25, 26,
         fused(1, "2x4", "gather4", 1704, 0, 1, "3:8", "0:6", "0:2", "0:6", 152704),
         tail(2, "stored", "0:6", "0:2", "0:6", "0:4", "0:4", "0:4", 82880), "adam", "-"),
    # stride 3; 180 positions: first-layer and AdamConv0 threads without a position
    Case((20, 20), 1, 3, 3, None, 20, 4, 5, 67,
         fused(1, "1x3", "direct", 480, 0, 1, "0:18", "0:5", "0:1", "0:5", 53744),
         tail(1, "stored", "0:5", "0:1", "0:5", "0:4", "0:4", "0:4", 40096), "adam", "-"),
    # scalar staging (323 inputs per sample); non-square maps 8x9 and 3x4
    Case((17, 19), 1, 3, 2, None, 16, 4, 19, 63,
         fused(2, "2x2", "scalar", 288, 0, 1, "0:12", "0:4", "0:1", "0:4", 66048),
         tail(2, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 33728), "adam", "pair"),
    # scalar staging; a fused head with 9 row groups: the tail's sums are added, not stored; 5x4 maps
    Case((11, 9), 1, 3, 2, None, 16, 4, 130, 232,
         fused(1, "9x2", "scalar", 256, 0, 1, "0:10", "0:4", "0:1", "0:4", 98688),
         tail(9, "added", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 32672), "adam", "-"),
    # one layer, 8x8 maps, 4288 positions: 5 passes of the first-layer loop and the AdamConv0 remainder loop; fc0 4:2
    Case((18, 18), 1, 3, 2, 1, 16, 4, 67, 68,
         fused(1, "5x9", "gather4", 608, 0, 1, "4:2", "0:4", "0:1", "0:4", 155472),
         tail(5, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 50080), "adam", "-"),
    # scalar staging (1089); 16x16 maps, fc0 K = 512 (4:8); the tail's W0 has exactly 2048 float4s; Linear 3 with 338 outputs:
    # 22 strips, the last 2 columns wide
    Case((33, 33), 1, 3, 2, 1, 16, 4, 11, 12,
         fused(1, "1x22", "scalar", 2144, 0, 1, "4:8", "0:4", "0:1", "0:4", 153712),
         tail(1, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 123808), "adam", "-"),
    # 31x31 / 15x15 / 7x7 maps in LDS; fc0 4:7 (98 k-steps: 2 empty waves)
    Case((64, 64), 1, 3, 2, 3, 16, 4, 2, 3,
         fused(3, "1x9", "direct", 1664, 0, 1, "4:7", "0:4", "0:1", "0:4", 132832),
         tail(1, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 100352), "adam", "pair"),
    # four encoder layers (the cap; only 2x2 kernels fit the parameter block), 16 channels into the tail; fc0 4:3 (36
    # k-steps: 4 empty waves); batch 1 ...
    Case((48, 48), 1, 2, 2, None, 16, 4, 1, 7,
         fused(4, "1x5", "direct", 672, 0, 1, "4:3", "0:4", "0:1", "0:4", 63648),
         tail(1, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 52352), "adam", "pair"),
    # ... and 2
    Case((48, 48), 1, 2, 2, None, 16, 4, 2, 7,
         fused(4, "1x5", "direct", 672, 0, 1, "4:3", "0:4", "0:1", "0:4", 81120),
         tail(1, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 52352), "adam", "pair"),
    # per-layer head, fused tail with 32 channels: two passes of the c0 loop of its BatchNorm sums ...
    Case((32, 32), 4, 3, 2, None, 16, 4, 6, None,
         layers("params"),
         tail(1, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 81280), "own", "pair"),
    # ... and with 16
    Case((32, 32), 2, 3, 2, None, 16, 4, 6, None,
         layers("params"),
         tail(1, "stored", "0:4", "0:1", "0:4", "0:4", "0:4", "0:4", 52352), "own", "pair"),
    # added for WANT: every weight matrix starts on a piece boundary (1024 float4s each, Linear 3's strip 512): no straddling
    # piece; tail gx 3:4
    Case((9, 9), 1, 3, 2, None, 128, 32, 7, 265,
         fused(1, "1x2", "scalar", 3584, 0, 0, "0:8", "3:4", "0:8", "4:2", 98464),
         tail(1, "stored", "3:4", "0:8", "3:4", "0:4", "0:4", "0:4", 65440), "adam", "-"),
]


def _id(c):
    return f"{c.inp[0]}x{c.inp[1]}x{c.ch}-k{c.k}s{c.stride}" + (f"n{c.count}" if c.count else "") + f"-fc{c.fc}.{c.latent}-b{c.batch}"


_IDS = [_id(c) for c in CASES]

WANT = ({("enc layers", n) for n in (1, 2, 3, 4)}
        | {("first layer", s) for s in ("3x3 one channel", "3x3 several channels", "5x5", "2x2")}
        | {("stride", 2), ("stride", 3)} | {("enc cout", n) for n in (2, 4, 6, 8, 12, 16)}
        | {("first-layer passes", s) for s in ("< 1", "1..4", "> 4")}
        | {("stage", s) for s in ("direct", "gather4", "scalar")}
        | {("batch", s) for s in ("< 16", "16", "1 mod 16")} | {("head row groups", s) for s in ("1", "2..8", "> 8")}
        | {("linear 3", "whole strips"), ("linear 3", "ragged last strip")}
        | {("late", 0), ("late", 1), ("straddle", "0"), ("straddle", ">= 1")}
        | {("head lg", n) for n in (0, 2, 3, 4)}
        | {("head", s) for s in ("per <= 4", "per > 4", "short last share", "empty waves")}
        | {("tail lg", n) for n in (0, 2, 3, 4)} | {("tail", "short last share"), ("tail", "empty waves")}
        | {("tail channels", n) for n in (2, 4, 8, 12, 16, 32)} | {("tail sums", "stored"), ("tail sums", "added"), ("tail w4 at its cap",)}
        | {("fused", "fused"), ("fused", "layers"), ("layers", "fused")}
        | {("adam conv0", s) for s in ("< 256 positions", "256..4096 positions", "> 4096 positions", "several input channels",
                                       "non-3x3 taps", "stride 3", "off: head not fused")})

# (planner, why) -> (input, channels, kernel, count, fc, latent, batch, kernel mode) that reaches it
REFUSALS = {
    ("head", "mode"): ((16, 16), 1, 3, None, 16, 4, 4, 0),
    ("head", "depth"): ((100, 100), 1, 2, None, 16, 4, 2, 1),          # five 2x2 layers
    ("head", "channels"): ((7, 7), 64, 3, None, 4, 4, 2, 1),           # 128 output channels
    ("head", "params"): ((64, 64), 1, 3, None, 16, 4, 2, 1),           # the sizer's four 3x3 layers: the last has 16 * 8 * 9 weights
    ("head", "nin4"): ((8, 8), 1, 3, None, 16, 4, 2, 1),               # 2 x 3 x 3 = 18 inputs of Linear 0
    ("head", "weights"): ((4, 4), 1, 2, 1, 1028, 4, 2, 1),             # 8224 float4s
    ("head", "biases"): ((3, 5), 1, 3, 1, 1028, 4, 2, 1),              # 1028 biases of Linear 0
    ("head", "lds"): ((16, 16), 1, 3, None, 192, 32, 40, 1),
    ("tail", "mode"): ((16, 16), 1, 3, None, 16, 4, 4, 0),
    ("tail", "fc4"): ((16, 16), 1, 3, None, 16, 6, 2, 1),              # latent 6
    ("tail", "panel"): ((16, 16), 1, 3, None, 516, 4, 2, 1),           # 16 x 516 / 4 float4s of a panel
    ("tail", "weights"): ((16, 16), 1, 3, None, 256, 32, 2, 1),        # 256 x 36 / 4 float4s of W0
    ("tail", "channels"): ((7, 7), 64, 3, None, 4, 4, 2, 1),
    ("tail", "lds"): ((49, 49), 1, 3, 1, 4, 4, 2, 1),                  # 1152 inputs of Linear 0: two 16-row panels of them
}
# what no (spec, fc, latent, batch) reaches
UNREACHABLE_WHY = {
    ("head", "syncing"): "the report is that of a step without SyncBN",
    ("head", "variational"): "a ConvAE engine is not the variational trunk",
    ("head", "segments"): "at most 4 encoder layers get this far: 2 segments each and 4 bias vectors are the 12 that fit",
    ("tail", "syncing"): "the report is that of a step without SyncBN",
    ("tail", "variational"): "a ConvAE engine is not the variational trunk",
}
HEAD_WHY = ("mode", "syncing", "variational", "depth", "channels", "params", "segments", "nin4", "weights", "biases", "lds")   # head_plan's order
TAIL_WHY = ("mode", "syncing", "variational", "fc4", "panel", "weights", "channels", "lds")                                    # tail_plan's order


@pytest.fixture(autouse=True)
def _oracle_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _spec(inp, ch, k, stride, count):
    from cae_tools_amd.models.model_sizer import create_model_spec
    return create_model_spec(input_size=inp, input_channels=ch, output_size=(28, 28), output_channels=1, kernel_size=k, stride=stride,
                             input_layer_count=count)


def _plan(spec_dict, fc, latent, batch, mode=1):
    from cae_tools_amd.engine import EnginePlan
    p = EnginePlan(spec_dict, fc, latent, max_batch=max(batch, 8))
    try:
        p.set_kernel_mode(mode)
        return p.kernel_plan(batch, True)
    finally:
        p.close()


def _listed(c):
    return {"head": c.head, "tail": c.tail, "enc": {"conv0": c.conv0, "inner": c.inner}}


def _splits(report, names, ks):
    """(lg, per, k-steps) of the stages `names` of a report line; ks: their contraction lengths"""
    out = []
    for (name, k) in zip(names, ks):
        (lg, per) = map(int, report[name].split(":"))
        out.append((lg, per, (k + 3) // 4))
    return out


def _reached(cases):
    """what `cases` reach, in WANT's terms, read from the plan report; every listed field is checked against the report"""
    reached = set()
    for c in cases:
        what = _id(c)
        spec = _spec(c.inp, c.ch, c.k, c.stride, c.count).save()
        enc = spec["input_layers"]
        plan = _plan(spec, c.fc, c.latent, c.batch)
        assert {k: plan[k] for k in ("head", "tail", "enc")} == _listed(c), (what, plan)
        # the batch at which the head leaves the fused path
        if c.leaves is None:
            assert _plan(spec, c.fc, c.latent, 1)["head"]["fwd"] == "layers", what
        else:
            assert _plan(spec, c.fc, c.latent, c.leaves - 1)["head"]["fwd"] == "fused", what
            assert _plan(spec, c.fc, c.latent, c.leaves)["head"] == layers("lds"), what
        head_fused = c.head["fwd"] == "fused"
        tail_fused = c.tail["bwd"] == "fused"
        reached.add((c.head["fwd"], c.tail["bwd"]))
        (co0, h0, w0) = enc[0]["output_dimensions"]
        (cl, hl, wl) = enc[-1]["output_dimensions"]
        nin = cl * hl * wl
        n3 = int(np.prod(spec["output_layers"][0]["input_dimensions"]))   # outputs of Linear 3
        pos0 = c.batch * h0 * w0
        if head_fused:
            h = c.head
            assert int(h["enc"]) == len(enc) and h["grid"] == f"{-(-c.batch // 16)}x{-(-n3 // 16)}", what
            reached |= {("enc layers", len(enc)), ("stride", c.stride), ("stage", h["stage"]), ("late", int(h["late"])),
                        ("straddle", "0" if h["straddle"] == "0" else ">= 1")}
            reached |= {("enc cout", l["output_dimensions"][0]) for l in enc}
            reached.add(("first layer", {3: "3x3 one channel" if c.ch == 1 else "3x3 several channels", 5: "5x5", 2: "2x2"}[c.k]))
            reached.add(("first-layer passes", "< 1" if pos0 < 1024 else ("1..4" if pos0 <= 4096 else "> 4")))
            reached.add(("batch", "< 16") if c.batch < 16 else ("batch", "16") if c.batch == 16 else ("batch", "other"))
            if c.batch % 16 == 1 and c.batch > 16:
                reached.add(("batch", "1 mod 16"))
            groups = -(-c.batch // 16)
            reached.add(("head row groups", "1" if groups == 1 else ("2..8" if groups <= 8 else "> 8")))
            reached.add(("linear 3", "whole strips" if n3 % 16 == 0 else "ragged last strip"))
            for (lg, per, s) in _splits(h, ("fc0", "fc1", "fc2", "fc3"), (nin, c.fc, c.latent, c.fc)):
                reached |= {("head lg", lg), ("head", "per <= 4" if per <= 4 else "per > 4")}
                assert per == -(-s // (1 << lg)), what
                if lg and s % per:
                    reached.add(("head", "short last share"))
                if (1 << lg) * per - s >= per:
                    reached.add(("head", "empty waves"))
        if tail_fused:
            t = c.tail
            assert int(t["rows"]) == -(-c.batch // 16) and t["sums"] == ("stored" if int(t["rows"]) <= 8 else "added"), what
            reached |= {("tail channels", cl), ("tail sums", t["sums"])}
            if 2048 in (nin * c.fc // 4, c.fc * c.latent // 4):
                reached.add(("tail w4 at its cap",))
            # chain stages g1, g0, gx contract over the outputs of Linear 2, 1, 0
            for (lg, per, s) in _splits(t, ("g1", "g0", "gx"), (c.fc, c.latent, c.fc)):
                reached.add(("tail lg", lg))
                if lg and s % per:
                    reached.add(("tail", "short last share"))
                if (1 << lg) * per - s >= per:
                    reached.add(("tail", "empty waves"))
        if c.conv0 == "adam":
            assert head_fused, what
            reached.add(("adam conv0", "< 256 positions" if pos0 < 256 else ("256..4096 positions" if pos0 <= 4096 else "> 4096 positions")))
            if c.ch > 1:
                reached.add(("adam conv0", "several input channels"))
            if c.k != 3:
                reached.add(("adam conv0", "non-3x3 taps"))
            if c.stride == 3:
                reached.add(("adam conv0", "stride 3"))
        else:
            assert not head_fused, what
            reached.add(("adam conv0", "off: head not fused"))
        assert c.inner == ("pair" if len(enc) > 1 else "-"), what
    return reached


@functools.lru_cache(maxsize=None)
def _model(i):
    """spec, initial state and data of case i; the batch is rows LEAD.. of x / t"""
    from cae_tools_amd.models.encoder import Encoder
    from cae_tools_amd.models.decoder import Decoder
    c = CASES[i]
    spec = _spec(c.inp, c.ch, c.k, c.stride, c.count)
    seed = 1000 + 10 * i
    torch.manual_seed(seed)
    enc = Encoder(spec.get_input_layers(), encoded_space_dim=c.latent, fc_size=c.fc)
    dec = Decoder(spec.get_output_layers(), encoded_space_dim=c.latent, fc_size=c.fc)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand((LEAD + c.batch, c.ch) + tuple(c.inp), generator=g)
    t = torch.rand((LEAD + c.batch, 1, 28, 28), generator=g)
    return spec, enc.state_dict(), dec.state_dict(), x, t


def _oracles(spec, enc_sd, dec_sd):
    from oracle import cae_oracle as orc
    d64 = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return (orc.OracleModel(spec.save(), enc_sd, dec_sd, lr=LR, weight_decay=WD),
            orc.OracleModel(spec.save(), d64(enc_sd), d64(dec_sd), lr=LR, weight_decay=WD))


def test_cases_reach_what_they_name():
    """every case's head, tail and enc lines are what CASES lists (EnginePlan.kernel_plan, no GPU) and its head leaves the fused
    path at the listed batch; together the cases reach WANT; every refusal reason of both planners is reached by REFUSALS or
    listed in UNREACHABLE_WHY; and on every case's seed the two oracles alone respect the window of relu_fix_for"""
    reached = _reached(CASES)
    assert WANT <= reached, sorted(map(str, WANT - reached))
    assert set(REFUSALS) | set(UNREACHABLE_WHY) == {("head", w) for w in HEAD_WHY} | {("tail", w) for w in TAIL_WHY}
    assert not set(REFUSALS) & set(UNREACHABLE_WHY)
    for ((planner, why), (inp, ch, k, count, fc, latent, batch, mode)) in REFUSALS.items():
        plan = _plan(_spec(inp, ch, k, 2, count).save(), fc, latent, batch, mode)
        got = plan["head"] if planner == "head" else plan["tail"]
        assert got == layers(why, "fwd" if planner == "head" else "bwd"), (planner, why, got)
    for i in range(len(CASES)):
        (spec, enc_sd, dec_sd, x, t) = _model(i)
        xb = x[LEAD:]
        (o32, o64) = _oracles(spec, enc_sd, dec_sd)
        (z32, z64) = (o32.relu_inputs(xb), o64.relu_inputs(xb.double()))
        relu_fix_for(o32, xb, {k: v > 0 for k, v in z64.items()}, f"{_IDS[i]}: fp32 oracle against the fp64 oracle's decisions")
        relu_fix_for(o64, xb.double(), {k: v > 0 for k, v in z32.items()}, f"{_IDS[i]}: fp64 oracle against the fp32 oracle's decisions")


def _engine(i, mode, max_batch=None):
    from cae_tools_amd.engine import HipEngine
    c = CASES[i]
    (spec, enc_sd, dec_sd, x, t) = _model(i)
    eng = HipEngine(spec, c.fc, c.latent, max_batch=max_batch or c.batch, graph=False, specialised=mode)
    eng.load_state(enc_sd, dec_sd)
    eng.set_hyper(lr=LR, weight_decay=WD)
    eng.set_dataset(0, x.cuda(), t.cuda())
    return eng


def _ratio(got, ref32, exact64):
    """|got - exact| over assert_close_as_reference's bound (its default factor and floors)"""
    (got, ref32, exact64) = (np.asarray(a, dtype=np.float64) for a in (got, ref32, exact64))
    bound = 3.0 * float(np.abs(ref32 - exact64).max()) + 1e-5 * float(np.abs(exact64).max()) + 1e-9
    return float(np.abs(got - exact64).max()) / bound


def _decisions_for(oracle, x, decisions, spec):
    """`decisions` (hip_relu_decisions) with the oracle's own decision wherever the step cannot have one: hip_relu_decisions reads
    a ReLU's decision off the gradient behind it, and an output row or column of an encoder layer that the next layer's
    windows never reach (8x9 maps under a 3x3 kernel at stride 2: row 7) has gradient zero whatever the ReLU decided -
    nothing downstream depends on those positions"""
    enc = spec["input_layers"]
    out = dict(decisions)
    z = None
    for (l, nxt) in zip(range(len(enc)), enc[1:]):
        (_, h, w) = enc[l]["output_dimensions"]
        (_, nh, nw) = nxt["output_dimensions"]
        (k, s) = (nxt["kernel_size"], nxt["stride"])
        (rh, rw) = ((nh - 1) * s + k, (nw - 1) * s + k)   # rows / columns the next layer reads
        if rh < h or rw < w:
            z = oracle.relu_inputs(x) if z is None else z
            d = decisions[f"enc_conv{l}"].clone()
            own = z[f"enc_conv{l}"] > 0
            d[:, :, rh:, :] = own[:, :, rh:, :]
            d[:, :, :, rw:] = own[:, :, :, rw:]
            out[f"enc_conv{l}"] = d
    return out


def _check_step(i, eng, rows, loss, got, what):
    """the loss and the gradients (got(name) -> array) of the engine's last training-mode step on rows `rows` of the case's data
    against the two oracles"""
    c = CASES[i]
    (spec, enc_sd, dec_sd, x, t) = _model(i)
    (xb, tb) = (x[rows], t[rows])
    noisy = bn_bias_keys(spec.save())
    decisions = hip_relu_decisions(eng, c.batch)
    (ref32, ref64) = _oracles(spec, enc_sd, dec_sd)
    (fix32, _) = relu_fix_for(ref32, xb, _decisions_for(ref32, xb, decisions, spec.save()), what + " fp32 oracle")
    (fix64, _) = relu_fix_for(ref64, xb.double(), _decisions_for(ref64, xb.double(), decisions, spec.save()), what + " fp64 oracle")
    loss32, _ = ref32.loss_and_grads(xb, tb, relu_fix=fix32)
    loss64, _ = ref64.loss_and_grads(xb.double(), tb.double(), relu_fix=fix64)
    (g32, g64) = (ref32.grads(), ref64.grads())
    got = {k: np.asarray(got(k)) for k in g32}
    ratios = {"loss": _ratio([loss], [float(loss32)], [float(loss64)])}
    ratios.update({k: _ratio(got[k], g32[k].numpy(), g64[k].numpy()) for k in g32 if k not in noisy})
    top = sorted(((r, k) for k, r in ratios.items()), reverse=True)[:3]
    print(f"\n[head tail shapes] {what}: worst |hip-fp64|/bound {top[0][0]:.3f} ({top[0][1]}), next {[(round(r, 3), k) for r, k in top[1:]]}")
    assert_close_as_reference([loss], [float(loss32)], [float(loss64)], f"{what} loss")
    for k in g32:
        if k in noisy:
            # exactly zero in exact arithmetic: magnitude only
            assert np.abs(got[k]).max() <= 1e-6 + 1e-4 * float(g32[k].abs().max()), f"{what} {k}"
            continue
        assert_close_as_reference(got[k], g32[k].numpy(), g64[k].numpy(), f"{what} {k}")


def _fwdbwd(i, eng, perm, rows, what):
    c = CASES[i]
    slot = eng.forward_backward(0, None if perm is None else eng.upload_perm(perm), LEAD if perm is None else 0, c.batch, c.batch)
    loss = eng._read_losses(slot, 1)[0]
    eng.sync()
    _check_step(i, eng, rows, loss, lambda k: eng.grad_view(k).cpu().numpy(), what)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=_IDS)
def test_training_step_and_scoring_against_fp64_oracle(i):
    from oracle import cae_oracle as orc
    c = CASES[i]
    (spec, enc_sd, dec_sd, x, t) = _model(i)
    xb = x[LEAD:]
    y_ref = orc.OracleModel(spec.save(), enc_sd, dec_sd).eval_forward(xb).numpy()
    for mode in (1, 0):
        what = f"{_IDS[i]} mode={mode}"
        eng = _engine(i, mode)
        if mode == 1:
            plan = eng.kernel_plan(c.batch, True)
            assert {k: plan[k] for k in ("head", "tail", "enc")} == _listed(c), (what, plan)
        # scoring first, on the initial running statistics
        err = float(np.abs(eng.score(xb.cuda()).cpu().numpy() - y_ref).max())
        print(f"\n[head tail shapes] {what}: score max|diff| {err:.2e}")
        assert err <= 1e-5, (what, err)
        _fwdbwd(i, eng, None, slice(LEAD, None), what)
        eng.close()


_PERM = [i for (i, c) in enumerate(CASES) if c.head.get("stage") == "direct"] + [_IDS.index("17x19x1-k3s2-fc16.4-b19")]


@pytest.mark.gpu
@pytest.mark.parametrize("i", _PERM, ids=[_IDS[i] for i in _PERM])
def test_training_step_through_a_device_permutation(i):
    """the same step on rows picked by a permutation on the device: the head gathers them with 16-byte loads through the sample
    table (scalar loads for the 17x19 case); the oracle gets the permuted batch"""
    c = CASES[i]
    perm = np.random.default_rng(i).permutation(LEAD + c.batch)[:c.batch].astype(np.int32)
    eng = _engine(i, 1)
    _fwdbwd(i, eng, perm, torch.from_numpy(perm.astype(np.int64)), f"{_IDS[i]} permuted")
    eng.close()


_ADAM = [i for (i, c) in enumerate(CASES) if c.conv0 == "adam"] + [_IDS.index("16x16x1-k3s2-fc16.4-b83")]


@pytest.mark.gpu
@pytest.mark.parametrize("i", _ADAM, ids=[_IDS[i] for i in _ADAM])
def test_train_step_from_zero_moments(i):
    """one train_step from zero moments: exp_avg = (1 - beta1)(g + wd w), so every gradient of the step that the optimiser
    launch consumed - conv 0's weight gradient computed inside it - is recovered and held to the same criterion"""
    c = CASES[i]
    eng = _engine(i, 1)
    w0 = eng.params.cpu().numpy().astype(np.float64)
    loss = eng.train_step(0, None, LEAD, c.batch)
    eng.sync()
    # exp_avg is fp32: recovering g from it costs 6e-8 of |g + wd w|, well under the criterion's relative floor
    g = eng.exp_avg.cpu().numpy().astype(np.float64) / 0.1 - WD * w0

    def got(k):
        (arena, off, numel, shape) = eng.tensors[k]
        return g[off:off + numel].reshape(shape)

    _check_step(i, eng, slice(LEAD, None), loss, got, f"{_IDS[i]} train_step")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=_IDS)
def test_two_runs_of_two_steps_give_the_same_bits(i):
    c = CASES[i]
    runs = []
    for _ in range(2):
        eng = _engine(i, 1)
        losses = [eng.train_step(0, None, start, c.batch) for start in (LEAD, 0)]
        eng.sync()
        runs.append((losses, eng.params.cpu(), eng.exp_avg.cpu(), eng.exp_avg_sq.cpu(), eng.buffers.cpu()))
        eng.close()
    (a, b) = runs
    assert a[0] == b[0], ("losses", a[0], b[0])
    for (u, v, name) in zip(a[1:], b[1:], ("params", "exp_avg", "exp_avg_sq", "running statistics")):
        assert torch.equal(u, v), f"{_IDS[i]}: {name} differ in {int((u != v).sum())} of {u.numel()} entries"
