"""Hand-written layer definitions (tests/hand_specs.py) against the fp64 oracle: the decoder kernels where only a hand-written
spec puts them.  create_model_spec emits 3- or 4-tap kernels at stride 2 without output padding and channel counts that halve
from a power of two; cae_engine_create takes any kernel size and stride and output_padding < stride, and choose_dec_fwd /
choose_dec_bwd (engine_choose.h) send such layers into the specialised kernels.  What the specs reach
(tests/test_hand_specs_cpu.py::test_cases_reach_what_they_name checks it against the plan report, without a GPU):
- output padding on k_s2_fwd_rows / k_s2_bwd_rows (one and two images per wave), k_ct_fwd_lds (3x3 and 4x4 taps), k_ct_bwd_lds,
  k_ct_bwd_band (2 and 6 bands), k_s2_fwd_cs, k_s2_fwd, k_s2_bwd and k_s2_last_fused: with 3 taps OH = 2H + 2, a last row and
  column that receive the bias only and still count in the BatchNorm sums; with 4 taps OH = 2H + 3, so QH = H + 2 quad rows;
  the three slab writers among them (weight-gradient partials stored: a wrong count is an out-of-bounds store)
- k_ig_fwd_s2 in the default mode: K split over 1, 2 and 4 waves with a ragged last slice (16/16/16/2 and 16/10 channels), the
  unpaired path (W == 1), W == 2, the column-pair clamps at quad columns 0 and >= W, two tiles per wave with idle last waves
  (batch 8), 3, 5, 10 and 25 output channels, scoring (no sums), layer 0 (no BatchNorm on its input) and inner layers, 1x1,
  2x2, 2x3, 3x3 and 4x4 taps, output padding, and a map of 90 x 91 quads (the integer-division arm; k_ig_wgrad's too, and
  k_wgrad's in mode 0); in mode 5 (test_gather_forward_on_the_lds_staged_layers) the three geometries of
  test_ct_fwd_shapes_gpu.py at batch 3: 3x3 / 3x4 / 4x3 / 4x4 taps behind BatchNorm'd inputs, 12 to 128 input channels, 96 -> 48
  on a 1x1 map
- k_ig_bwd_pair with one K slice (K = Cout * KH * KW of 2, 8, 12, 16, 27, 45), K no multiple of 4, 1, 2, 6 and 7 taps, strides
  1 and 3 at ksplit 1 and 4, stride 2 at 1, 2 and 4
- k_up: the four-tap arm at stride 1 (k 2) and 3 (k 6), the general loop at k 3 / stride 1 and k 7 / stride 2, a kernel
  smaller than its stride (k 2 / stride 3, output padding 1: outputs that get the bias only)
- thin layers with output padding as layer 0, where the row kernels do not apply: k_s2_fwd_cs / k_s2_bwd_split (8 -> 4),
  k_s2_fwd / k_s2_bwd2 (4 -> 2, tile widths 32 and 64), k_s2_fwd / k_s2_bwd with three channels per thread (6 -> 3, 4x4);
  k_s2_last_fused with 16-byte target loads (OW = 44) and, in the one large case (wide_last, 1x451x451 at batch 8), with a
  second strip; scoring's last layer on k_s2_fwd2 there (8 x 113 x 113 thread positions).
No specialised decoder kernel that a spec at fc 16 / latent 4 and batch <= 8 can reach is left without a case here or in a
sibling file.  Left out, by size: k_s2_fwd2 with the BatchNorm-sum epilogue on a padded middle layer (100000 thread
positions at batch 8 are a 447 x 447 map with a layer behind it; test_s2_shapes_gpu.py runs that epilogue at its large
batches, without output padding).

The models' conv biases are drawn as torch's own initialiser draws them, uniform in +-1 / sqrt(fan_in) (hand_specs.model):
Encoder and Decoder zero them, and with zero biases the bias-only outputs are all 0 - a build whose k_ig_fwd_s2 and
k_s2_fwd_rows left the bias-only row out of the BatchNorm sums passed every case here with unchanged ratios while the biases
were zero.  Larger channel means are outside this file: with conv and BatchNorm biases uniform in +-0.5 the specialised
kernels sat up to 4.25x the bound from fp64 on five specs (7.1e-8 against a bound of 1.7e-8 on enc/encoder_cnn.0.weight,
padded_thin at batch 2; mode 0 stayed below 0.41), and in mode 0 gather_tpw / gather_wide differed from the fp32 oracle in
ReLU decisions at inputs of 1.8e-5 .. 3.5e-5 of the layer's scale (z_tol 1.2e-5): the one-pass variance E[y^2] - mean^2
loses what |mean| / std takes.

Per case (spec, batch), in the default mode, on the shape-generic kernels (mode 0) and, for the padded specs, in mode 3:
- score() within 1e-5 of the oracle's eval forward
- one forward_backward: loss and every gradient no further from the fp64 oracle than 3x the fp32 oracle is
  (helpers.assert_close_as_reference), both oracles taking the HIP step's ReLU decisions where their own input is within
  rounding of zero (relu_fix_for); conv biases that feed a BatchNorm (bn_bias_keys) on magnitude only
- one train_step of a fresh engine: the running means and variances under the same criterion (the bias-only row and column
  are part of the count)
and: two runs of two training steps give the same bits (default mode); on the padded specs the slabs give the bits of the
atomics (cae_set_kernel_mode bit 3) in modes 1 and 3.

Worst |hip - fp64| / bound over the loss, the gradients and the running statistics (the tensor it was found on), as each case
printed it on an MI355X - for the next reader; no threshold depends on these:
     padded_thin B=2 mode 1: 0.177 (dec/decoder_conv.1.weight); mode 0: 0.152; mode 3: 0.177
     padded_thin B=3 mode 1: 0.139 (enc/encoder_cnn.1.bias); mode 0: 0.233; mode 3: 0.139
   padded_thin33 B=2 mode 1: 0.036 (dec/decoder_conv.9.bias); mode 0: 0.065; mode 3: 0.036
   padded_thin33 B=3 mode 1: 0.087 (dec/decoder_conv.1.bias); mode 0: 0.045; mode 3: 0.087
     padded_rich B=2 mode 1: 0.046 (dec/decoder_lin.0.weight); mode 0: 0.050; mode 3: 0.035
     padded_rich B=3 mode 1: 0.034 (enc/encoder_lin.2.bias); mode 0: 0.101; mode 3: 0.030
  rich44_oddcout B=2 mode 1: 0.067 (enc/encoder_cnn.1.bias); mode 0: 0.132
  rich44_oddcout B=3 mode 1: 0.092 (enc/encoder_lin.2.bias); mode 0: 0.047
    gather_small B=2 mode 1: 0.061 (enc/encoder_cnn.0.weight); mode 0: 0.159
    gather_small B=3 mode 1: 0.066 (enc/encoder_lin.2.weight); mode 0: 0.148
        gather_k B=2 mode 1: 0.082 (dec/decoder_conv.12.bias); mode 0: 0.068
        gather_k B=3 mode 1: 0.093 (enc/encoder_lin.2.bias); mode 0: 0.079
      gather_tpw B=2 mode 1: 0.062 (dec/decoder_conv.1.weight); mode 0: 0.182
      gather_tpw B=3 mode 1: 0.097 (dec/decoder_conv.3.bias); mode 0: 0.156
      gather_tpw B=8 mode 1: 0.154 (dec/decoder_conv.3.weight); mode 0: 0.163
     gather_wide B=2 mode 1: 0.073 (dec/decoder_conv.3.weight); mode 0: 0.165
         strides B=2 mode 1: 0.073 (dec/decoder_lin.2.bias); mode 0: 0.086
         strides B=3 mode 1: 0.116 (enc/encoder_lin.2.weight); mode 0: 0.080
         first84 B=2 mode 1: 0.143 (enc/encoder_lin.0.weight); mode 0: 0.064
         first84 B=3 mode 1: 0.099 (enc/encoder_cnn.1.bias); mode 0: 0.113
         first42 B=2 mode 1: 0.053 (enc/encoder_cnn.1.weight); mode 0: 0.042
         first42 B=3 mode 1: 0.056 (enc/encoder_lin.2.bias); mode 0: 0.077
         first63 B=2 mode 1: 0.023 (enc/encoder_cnn.1.bias); mode 0: 0.049
         first63 B=3 mode 1: 0.144 (enc/encoder_lin.2.bias); mode 0: 0.045
       wide_last B=8 mode 1: 0.162 (enc/encoder_cnn.1.weight); mode 0: 0.222
Every score() sat within 6e-08 of the oracle's eval forward."""
import numpy as np
import pytest
import torch

import hand_specs as hs
from helpers import assert_close_as_reference, bn_bias_keys, hip_relu_decisions, relu_fix_for
from wgrad_slabs import ATOMICS

pytestmark = pytest.mark.gpu

CASES = [(name, batch) for (name, (_, _, batches)) in hs.SPECS.items() for batch in batches]
_IDS = [f"{name}-{batch}" for (name, batch) in CASES]
_PADDED = [(name, batch, mode) for (name, batch) in CASES if name in hs.PADDED for mode in (1, 3)]


@pytest.fixture(autouse=True)
def _oracle_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _engine(spec, enc_sd, dec_sd, x, t, batch, mode):
    from cae_tools_amd.engine import HipEngine
    eng = HipEngine(spec, hs.FC, hs.LATENT, max_batch=batch, graph=False, specialised=mode)
    eng.load_state(enc_sd, dec_sd)
    eng.set_hyper(lr=1e-3, weight_decay=1e-5)
    eng.set_dataset(0, x.cuda(), t.cuda())
    return eng


def _ratio(got, ref32, exact64):
    """|got - exact| over assert_close_as_reference's bound (its default factor and floors)"""
    (got, ref32, exact64) = (np.asarray(a, dtype=np.float64) for a in (got, ref32, exact64))
    bound = 3.0 * float(np.abs(ref32 - exact64).max()) + 1e-5 * float(np.abs(exact64).max()) + 1e-9
    return float(np.abs(got - exact64).max()) / bound


def _against_fp64(model, batch, mode, what, y_ref, expect=None):
    """score(), one forward_backward and one train_step's running statistics of `model` in kernel mode `mode` against the
    oracles; expect: hand_specs.expected rows the engine's own plan must show first"""
    from oracle import cae_oracle as orc
    (spec, enc_sd, dec_sd, xb, tb) = model
    noisy = bn_bias_keys(spec.save())
    d64 = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    eng = _engine(spec, enc_sd, dec_sd, xb, tb, batch, mode)
    if expect is not None:
        got_plan = hs.observed(eng.kernel_plan(batch, True), eng.kernel_plan(batch, False))
        assert got_plan == expect, (what, got_plan)
    # scoring first, on the initial running statistics
    y = eng.score(xb.cuda()).cpu().numpy()
    err = float(np.abs(y - y_ref).max())
    assert err <= 1e-5, (what, err)
    slot = eng.forward_backward(0, None, 0, batch, batch)
    loss = eng._read_losses(slot, 1)[0]
    eng.sync()
    decisions = hip_relu_decisions(eng, batch)
    ref32 = orc.OracleModel(spec.save(), enc_sd, dec_sd, lr=1e-3, weight_decay=1e-5)
    ref64 = orc.OracleModel(spec.save(), d64(enc_sd), d64(dec_sd), lr=1e-3, weight_decay=1e-5)
    (fix32, _) = relu_fix_for(ref32, xb, decisions, what + " fp32 oracle")
    (fix64, _) = relu_fix_for(ref64, xb.double(), decisions, what + " fp64 oracle")
    loss32, _ = ref32.loss_and_grads(xb, tb, relu_fix=fix32)
    loss64, _ = ref64.loss_and_grads(xb.double(), tb.double(), relu_fix=fix64)
    g64 = ref64.grads()
    got = {k: eng.grad_view(k).cpu().numpy() for k in g64}
    eng.close()
    # the running statistics after one training step of a fresh engine: the oracles' train-mode forward above left theirs
    eng = _engine(spec, enc_sd, dec_sd, xb, tb, batch, mode)
    eng.train_step(0, None, 0, batch)
    eng.sync()
    (s32, s64) = (ref32.state(), ref64.state())
    running = [k for k in s64 if k.endswith((".running_mean", ".running_var"))]
    assert len(running) == 2 * (len(spec.get_input_layers()) + len(spec.get_output_layers()) - 1)
    got_run = {k: eng.view(k).cpu().numpy() for k in running}
    eng.close()
    ratios = {"loss": _ratio([loss], [float(loss32)], [float(loss64)])}
    ratios.update({k: _ratio(got[k], g32.numpy(), g64[k].numpy()) for k, g32 in ref32.grads().items() if k not in noisy})
    ratios.update({k: _ratio(got_run[k], s32[k].numpy(), s64[k].numpy()) for k in running})
    top = sorted(((r, k) for k, r in ratios.items()), reverse=True)[:3]
    print(f"\n[hand specs] {what}: worst |hip-fp64|/bound {top[0][0]:.3f} ({top[0][1]}), next "
          f"{[(round(r, 3), k) for r, k in top[1:]]}; score max|diff| {err:.2e}")
    assert_close_as_reference([loss], [float(loss32)], [float(loss64)], f"{what} loss")
    for k, g32 in ref32.grads().items():
        if k in noisy:
            # exactly zero in exact arithmetic: magnitude only
            assert np.abs(got[k]).max() <= 1e-6 + 1e-4 * float(g32.abs().max()), f"{what} {k}"
            continue
        assert_close_as_reference(got[k], g32.numpy(), g64[k].numpy(), f"{what} {k}")
    for k in running:
        assert_close_as_reference(got_run[k], s32[k].numpy(), s64[k].numpy(), f"{what} {k}")


@pytest.mark.parametrize("name,batch", CASES, ids=_IDS)
def test_training_step_scoring_and_running_statistics_against_fp64_oracle(name, batch):
    from oracle import cae_oracle as orc
    model = hs.model(name, batch, seed=sum(map(ord, name)) + batch)
    (spec, enc_sd, dec_sd, xb, _) = model
    y_ref = orc.OracleModel(spec.save(), enc_sd, dec_sd).eval_forward(xb).numpy()
    for mode in hs.MODES[name]:
        _against_fp64(model, batch, mode, f"{name} B={batch} mode={mode}", y_ref, expect=hs.expected(name, mode))


@pytest.mark.parametrize("geometry", ["1x256x256", "3x82x83", "2x159x191"])
def test_gather_forward_on_the_lds_staged_layers(geometry):
    """mode 5 (cae_set_kernel_mode bit 2): k_ig_fwd_s2 on every layer that k_ct_fwd_lds runs by default, at batch 3"""
    import test_ct_fwd_shapes_gpu as ctf
    from oracle import cae_oracle as orc
    (out_c, out_h, out_w) = g = tuple(map(int, geometry.split("x")))
    assert g in ctf.GEOMETRIES
    (spec, enc_sd, dec_sd, x, t) = ctf._model(out_c, out_h, out_w, 3, seed=out_h * 7 + out_w + out_c)
    model = (spec, enc_sd, dec_sd, x[:3], t[:3])
    eng = _engine(*model, 3, 5)
    plans = (eng.kernel_plan(3, True), eng.kernel_plan(3, False))
    eng.close()
    for l in ctf.LAYERS[g]:
        assert all(p[f"dec{l[0]}"]["fwd"] == "ig_fwd_s2" for p in plans), (geometry, plans)
    y_ref = orc.OracleModel(spec.save(), enc_sd, dec_sd).eval_forward(model[3]).numpy()
    _against_fp64(model, 3, 5, f"{geometry} B=3 mode=5", y_ref)


@pytest.mark.parametrize("name,batch", CASES, ids=_IDS)
def test_two_runs_of_two_steps_give_the_same_bits(name, batch):
    (spec, enc_sd, dec_sd, x, t) = hs.model(name, 2 * batch, seed=5)
    runs = []
    for _ in range(2):
        eng = _engine(spec, enc_sd, dec_sd, x, t, batch, 1)
        losses = [eng.train_step(0, None, k * batch, batch) for k in range(2)]
        eng.sync()
        runs.append((losses, eng.params.cpu(), eng.exp_avg.cpu(), eng.exp_avg_sq.cpu(), eng.buffers.cpu()))
        eng.close()
    (a, b) = runs
    assert a[0] == b[0], ("losses", a[0], b[0])
    for (u, v, what) in zip(a[1:], b[1:], ("params", "exp_avg", "exp_avg_sq", "running statistics")):
        assert torch.equal(u, v), f"{name} B={batch}: {what} differ in {int((u != v).sum())} of {u.numel()} entries"


def _same_bits(a, b, what):
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} entries differ"


@pytest.mark.parametrize("name,batch,mode", _PADDED, ids=[f"{n}-{b}-mode{m}" for (n, b, m) in _PADDED])
def test_slabs_give_the_bits_of_the_atomics(name, batch, mode):
    """as test_wgrad_fold_gpu.py's test of this name: the gradient arena of one forward_backward, and weights, moments and
    running statistics after three steps, with the partial slabs and with the atomics of cae_set_kernel_mode bit 3"""
    (spec, enc_sd, dec_sd, x, t) = hs.model(name, 3 * batch, seed=len(name) + batch)
    got = {}
    for m in (mode, mode | ATOMICS):
        eng = _engine(spec, enc_sd, dec_sd, x, t, batch, m)
        slot = eng.forward_backward(0, None, 0, batch, batch)
        loss = eng._read_losses(slot, 1)[0]
        eng.sync()
        grads = eng.grads.cpu().clone()
        eng.close()
        eng = _engine(spec, enc_sd, dec_sd, x, t, batch, m)
        losses = [eng.train_step(0, None, k * batch, batch) for k in range(3)]
        eng.sync()
        got[m] = (loss, grads, losses, eng.params.cpu(), eng.exp_avg.cpu(), eng.exp_avg_sq.cpu(), eng.buffers.cpu())
        eng.close()
    (a, b) = (got[mode], got[mode | ATOMICS])
    assert a[0] == b[0] and a[2] == b[2], ("losses", a[0], b[0], a[2], b[2])
    _same_bits(a[1], b[1], "fp32 gradient arena of forward_backward")
    for (u, v, what) in zip(a[3:], b[3:], ("weights", "exp_avg", "exp_avg_sq", "running statistics")):
        _same_bits(u, v, f"{what} after three training steps")
