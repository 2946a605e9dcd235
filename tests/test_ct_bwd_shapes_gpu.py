"""The backward of the channel-rich decoder layers against the fp64 oracle, at every branch its host plans can take:
k_ct_bwd_lds (whole images staged), k_ct_bwd_band (bands of input rows staged; both kernels_ctbwd.h) and the gather pair
k_ig_bwd_pair (kernels_igemm.h), as ct_bwd_plan / ct_bwd_band_plan / ig_bwd_plan (engine_choose.h) choose and shape them.
The counterpart of test_ct_fwd_shapes_gpu.py.  Both plans depend on the BATCH: the same layer changes kernel and workgroup
layout as the batch grows, so the cases are (geometry, batch, kernel mode) and half of them are large batches.

CASES are sizer-made models (create_model_spec, 16x16 inputs); each lists, per channel-rich decoder layer, the fields of the
plan report (EnginePlan.kernel_plan: ctb_* / ig_*).  test_cases_reach_what_they_name (no GPU) checks every listed field
against the report and that the cases together reach (WANT):
- k_ct_bwd_band: hb = 1; hb > 1 with a full and with a short last band; 2 bands and 8 (the cap); one, two and three or more
  blocks of 16 input channels; square and non-square maps; an odd batch
- k_ct_bwd_lds, the six cells a sizer-made decoder reaches: imgs = 1 with parts = 1; imgs = 1 with parts > 1 where the band
  kernel was refused because Cout * gstr > 4096 and where it was refused because 16 * astr > 1024 (gstr / astr: the band's
  gradient rows / input rows per channel; the 16->8 layer of the benchmark geometry at batch 128 fails both, 11x11 maps
  only the second); imgs > 1 with parts > 1 and a whole last image group (default mode), the same with a short last group
  (B % imgs != 0: mode 3 only); imgs > 1 with parts = 1, whole and short last group
- a layer that ct_bwd_plan takes at batch 2 and gives back to the gather pair at the case's batch (Cin * N * groups > 400000)
- decoder layer 0 (its producer is a Linear layer: no BatchNorm on its input, no producer sums) and a middle layer, on each
  kernel
- 8, 16, 24 and 32 output channels; 48 do not fit the weight staging (16 * Cout * 9 floats > 3 pieces of 16 bytes per thread):
  that layer stays on the gather pair in mode 3
- the sharded weight-gradient accumulator (Cin = 16: the automatic mask) and the plain one (other layers, mode 3)
- k_ig_bwd_pair: ksplit 2 and 4; one and two tiles per wave; per = 32 and per > 32; chunks = 1, 2..8 and more than 8
  (w_n8 > 1); 3x3, 3x4, 4x3 and 4x4 taps; a ragged block of input channels (24 or 12).  ksplit = 1 needs Cout * KH * KW <= 48:
  those layers are all stride-2-specialised (kernels_s2.h), and test_sweep_reaches_no_ksplit_1_plan confirms that no sizer-made
  decoder reaches it: the hand-written layer definitions of test_hand_specs_gpu.py do (ksplit = 1 at strides 1, 2 and 3, K no
  multiple of 4, kernels of 1, 2, 6 and 7 taps).
Not here: a 3x3 layer with OH > 2H + 1 (the staging assumes nothing about the rows below 2H; a sizer-made decoder never pairs
a 3x3 kernel with output padding, so only a hand-written spec reaches it): test_hand_specs_gpu.py runs k_ct_bwd_lds and
k_ct_bwd_band, 2 and 6 bands, at OH = 2H + 2.

Per case, one training step in the case's mode and (small batches only) one on the shape-generic kernels (mode 0):
- loss and every gradient no further from the fp64 oracle than 3x the fp32 oracle is (helpers.assert_close_as_reference),
  both oracles taking the HIP step's ReLU decisions where their own input is within rounding of zero (relu_fix_for); conv
  biases that feed a BatchNorm (bn_bias_keys) on magnitude only
- score() within 1e-5 of the oracle's eval forward
- default-mode cases: two runs of two training steps give the same bits (mode 3 is a diagnostic switch without that promise).

Worst |hip - fp64| / bound over the loss and the gradients (the tensor it was found on), as each case printed it on an
MI355X - for the next reader; no threshold depends on these:
      2x24x24 B=32  mode 1: 0.096 (enc/encoder_cnn.0.weight); mode 0: 0.200
      2x24x24 B=130 mode 1: 0.060 (enc/encoder_cnn.3.weight)
      2x24x24 B=192 mode 1: 0.055 (enc/encoder_cnn.3.weight)
      2x89x89 B=2   mode 1: 0.067 (dec/decoder_conv.0.weight); mode 0: 0.060
      2x96x96 B=96  mode 1: 0.041 (enc/encoder_lin.2.weight)
    1x256x256 B=128 mode 1: 0.062 (enc/encoder_cnn.0.weight)
      2x87x87 B=384 mode 1: 0.045 (enc/encoder_cnn.3.weight)
      2x81x81 B=512 mode 1: 0.118 (dec/decoder_conv.12.bias)
    2x105x105 B=384 mode 1: 0.023 (dec/decoder_conv.1.bias)
      3x82x83 B=384 mode 1: 0.046 (enc/encoder_cnn.1.weight)
      2x99x99 B=9   mode 3: 0.055 (dec/decoder_lin.2.weight); mode 0: 0.070
      3x48x48 B=32  mode 3: 0.073 (enc/encoder_lin.0.bias); mode 0: 0.067
      2x79x50 B=2   mode 3: 0.089 (enc/encoder_cnn.1.weight); mode 0: 0.100
    3x159x130 B=3   mode 3: 0.067 (enc/encoder_cnn.1.weight); mode 0: 0.073
    2x129x129 B=2   mode 3: 0.055 (enc/encoder_lin.0.bias); mode 0: 0.083
    2x129x129 B=256 mode 3: 0.052 (enc/encoder_cnn.1.weight)
Every score() sat within 9e-8 of the oracle's eval forward."""
import numpy as np
import pytest
import torch

from helpers import assert_close_as_reference, bn_bias_keys, hip_relu_decisions, relu_fix_for

FC, LATENT = 16, 4


def ctb(kernel, imgs, groups, parts, bands=0, hb=0, sharded=1):
    return {"bwd": "ct_bwd_lds", "ctb_kernel": kernel, "ctb_imgs": str(imgs), "ctb_groups": str(groups), "ctb_parts": str(parts),
            "ctb_bands": str(bands), "ctb_hb": str(hb), "ctb_sharded": str(sharded)}


def ig(ksplit, tpw, chunks, per, dgroup, wn8):
    return {"bwd": "ig_bwd_pair", "ig_ksplit": str(ksplit), "ig_tpw": str(tpw), "ig_chunks": str(chunks), "ig_per": str(per),
            "ig_dgroup": str(dgroup), "ig_wn8": str(wn8)}


# ((output channels, height, width), batch, kernel mode, also on the generic kernels, {decoder layer: its backward's report})
# every layer on ct_bwd_lds or ig_bwd_pair is listed; the large batches run their own mode only
CASES = [
    # ---- default mode ----
    ((2, 24, 24), 32, 1, True, {0: ctb("band", 1, 32, 2, 2, 1)}),                       # layer 0 16->8 2x2: two bands of one row
    ((2, 24, 24), 130, 1, False, {0: ctb("lds", 1, 130, 1)}),                           # ... one image, one part
    ((2, 24, 24), 192, 1, False, {0: ctb("lds", 2, 96, 2)}),                            # ... pairs of images, task list split in two
    ((2, 89, 89), 2, 1, True, {0: ig(4, 1, 1, 32, 8, 1), 1: ig(4, 1, 1, 32, 8, 1),      # 4x4 taps, one chunk
                               2: ctb("band", 1, 2, 5, 5, 2)}),                          # 10x10: five full bands of two rows
    ((2, 96, 96), 96, 1, False, {0: ig(4, 1, 3, 32, 8, 1), 1: ig(4, 1, 19, 32, 8, 3),
                                 2: ctb("lds", 1, 96, 2)}),                              # 11x11: a band of 6 rows has 16 * 66 > 1024
    ((1, 256, 256), 128, 1, False, {0: ig(4, 1, 9, 32, 8, 2), 1: ig(4, 1, 49, 32, 8, 7),
                                    2: ctb("lds", 1, 128, 2)}),                          # 15x15: a band of 8 rows has 8 * 17 * 31 > 4096
    ((2, 87, 87), 384, 1, False, {0: ig(4, 1, 3, 32, 8, 1), 1: ig(4, 1, 48, 32, 8, 6),
                                  2: ctb("lds", 2, 192, 1)}),                            # 10x10: pairs of images, whole last group
    ((2, 81, 81), 512, 1, False, {0: ig(4, 1, 4, 32, 8, 1), 1: ig(4, 1, 64, 32, 8, 8),
                                  2: ctb("lds", 3, 171, 1)}),                            # 9x9: threes, the last group has two
    ((2, 105, 105), 384, 1, False, {0: ig(4, 1, 12, 32, 8, 2), 1: ig(4, 1, 38, 64, 16, 5),
                                    2: ig(2, 1, 216, 64, 8, 27)}),                       # 12x12 16->8: back on the gather pair
    ((3, 82, 83), 384, 1, False, {0: ig(4, 1, 3, 32, 8, 1), 1: ig(4, 1, 48, 32, 8, 6),   # 4x4, 3x3,
                                  2: ig(4, 1, 81, 96, 24, 11),                           # 24->12 3x4,
                                  3: ig(2, 2, 380, 96, 6, 48)}),                         # 12->6 4x3: two tiles per wave
    # ---- mode 3: the LDS-staged backward wherever it fits ----
    ((2, 99, 99), 9, 3, True, {0: ctb("lds", 2, 5, 8, sharded=0),                       # layer 0 64->32: four blocks, last group of one
                               1: ctb("band", 1, 9, 5, 5, 1, sharded=0),                 # 32->16 5x5
                               2: ig(4, 1, 9, 32, 8, 2)}),
    ((3, 48, 48), 32, 3, True, {0: ctb("lds", 3, 11, 7, sharded=0),                     # layer 0 48->24: three blocks, last group of two
                                1: ig(4, 1, 7, 32, 8, 1), 2: ig(2, 1, 31, 32, 4, 4)}),
    ((2, 79, 50), 2, 3, True, {0: ctb("band", 1, 2, 4, 4, 1, sharded=0),                # layer 0 32->16 4x2
                               1: ctb("band", 1, 2, 5, 5, 2)}),                          # 16->8 9x5: the last band has one row
    ((3, 159, 130), 3, 3, True, {0: ig(4, 1, 1, 32, 8, 1),                              # 96->48: does not fit the weight staging
                                 1: ctb("band", 1, 3, 5, 5, 2, sharded=0),               # 48->24 9x7, odd batch, short last band
                                 2: ig(4, 1, 7, 32, 8, 1), 3: ig(2, 1, 29, 32, 4, 4)}),
    ((2, 129, 129), 2, 3, True, {0: ctb("band", 1, 2, 3, 3, 1, sharded=0), 1: ctb("band", 1, 2, 7, 7, 1, sharded=0),
                                 2: ctb("band", 1, 2, 8, 8, 2)}),                        # 15x15: eight bands, the cap
    ((2, 129, 129), 256, 3, False, {0: ig(4, 1, 18, 32, 8, 3),                          # 64->32: back on the gather pair
                                    1: ctb("lds", 3, 86, 1, sharded=0),                  # 32->16 7x7: threes, last group of one
                                    2: ctb("lds", 1, 256, 1)}),
]
_IDS = ["x".join(map(str, g)) + f"-{b}-mode{m}" for (g, b, m, _, _) in CASES]

kCtbThreads = 512   # kernels_ctbwd.h
# caps of the issue that set the sizes: batch x output elements, and the largest BatchNorm'd map (test_s2_shapes_gpu.py's
# largest LARGE_BATCH case), at which relu_fix_for's max_flips has held in this suite
MAX_OUTPUT, MAX_BN_MAP = 13_000_000, 512 * 4 * 54 * 54


@pytest.fixture(autouse=True)
def _oracle_threads():
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def _spec(out_c, out_h, out_w):
    from cae_tools_amd.models.model_sizer import create_model_spec
    return create_model_spec(input_size=(16, 16), input_channels=1, output_size=(out_h, out_w), output_channels=out_c)


def _plan(spec_dict, batch, mode):
    from cae_tools_amd.engine import EnginePlan
    p = EnginePlan(spec_dict, FC, LATENT, max_batch=max(batch, 8))
    try:
        p.set_kernel_mode(mode)
        return p.kernel_plan(batch, True)
    finally:
        p.close()


def _bwd_report(entry):
    return {k: v for (k, v) in entry.items() if k == "bwd" or k.startswith(("ctb_", "ig_"))}


def _model(out_c, out_h, out_w, n, seed):
    from cae_tools_amd.models.encoder import Encoder
    from cae_tools_amd.models.decoder import Decoder
    spec = _spec(out_c, out_h, out_w)
    torch.manual_seed(seed)
    enc = Encoder(spec.get_input_layers(), encoded_space_dim=LATENT, fc_size=FC)
    dec = Decoder(spec.get_output_layers(), encoded_space_dim=LATENT, fc_size=FC)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand((n, 1, 16, 16), generator=g)
    t = torch.rand((n, out_c, out_h, out_w), generator=g)
    return spec, enc.state_dict(), dec.state_dict(), x, t


def _engine(spec, enc_sd, dec_sd, x, t, batch, mode):
    from cae_tools_amd.engine import HipEngine
    eng = HipEngine(spec, FC, LATENT, max_batch=batch, graph=False, specialised=mode)
    eng.load_state(enc_sd, dec_sd)
    eng.set_hyper(lr=1e-3, weight_decay=1e-5)
    eng.set_dataset(0, x.cuda(), t.cuda())
    return eng


def _dims(layer):
    k = layer["kernel_size"]
    (kh, kw) = (k, k) if isinstance(k, int) else tuple(k)
    (ci, h, w) = layer["input_dimensions"]
    (co, oh, ow) = layer["output_dimensions"]
    return ci, h, w, co, oh, ow, kh, kw


WANT = {("band", "hb 1"), ("band", "full last band"), ("band", "short last band"), ("band", "bands", 2), ("band", "bands", 8),
        ("band", "blocks", 1), ("band", "blocks", 2), ("band", "blocks", 3), ("band", "square", True), ("band", "square", False),
        ("band", "odd batch"), ("band", "layer 0"), ("band", "middle layer"),
        ("lds", "imgs 1", "parts 1"), ("lds", "imgs 1", "parts > 1", "refused: Cout * gstr"),
        ("lds", "imgs 1", "parts > 1", "refused: 16 * astr"),
        ("lds", "imgs > 1", "parts > 1", "whole last group", "mode 1"), ("lds", "imgs > 1", "parts > 1", "short last group", "mode 3"),
        ("lds", "imgs > 1", "parts 1", "whole last group"), ("lds", "imgs > 1", "parts 1", "short last group"),
        ("lds", "layer 0"), ("lds", "middle layer"),
        ("given back above 400000",), ("cout 48 does not fit",),
        ("ct", "cout", 8), ("ct", "cout", 16), ("ct", "cout", 24), ("ct", "cout", 32), ("ct", "sharded", True), ("ct", "sharded", False),
        ("ig", "ksplit", 2), ("ig", "ksplit", 4), ("ig", "tpw", 1), ("ig", "tpw", 2), ("ig", "per 32"), ("ig", "per > 32"),
        ("ig", "chunks 1"), ("ig", "chunks 2..8"), ("ig", "chunks > 8"), ("ig", "ragged cin"),
        ("ig", "taps", 3, 3), ("ig", "taps", 3, 4), ("ig", "taps", 4, 3), ("ig", "taps", 4, 4)}


def _reached(cases):
    """what `cases` reach, in WANT's terms, read from the plan report; every listed field is checked against the report"""
    reached = set()
    for (geometry, batch, mode, generic_too, layers) in cases:
        spec = _spec(*geometry).save()
        dec = spec["output_layers"]
        what = (geometry, batch, mode)
        (out_c, out_h, out_w) = geometry
        assert batch * out_c * out_h * out_w <= MAX_OUTPUT, what
        assert max(batch * l["output_dimensions"][0] * l["output_dimensions"][1] * l["output_dimensions"][2] for l in dec[:-1]) <= MAX_BN_MAP, what
        assert generic_too == (batch < 64), what   # the large batches run the case's own mode only
        plan = _plan(spec, batch, mode)
        at_2 = _plan(spec, 2, mode)
        got = {i: _bwd_report(plan[f"dec{i}"]) for i in range(len(dec)) if plan[f"dec{i}"]["bwd"] in ("ct_bwd_lds", "ig_bwd_pair")}
        assert got == layers, (what, got)
        for (i, rep) in layers.items():
            (ci, h, w, co, oh, ow, kh, kw) = _dims(dec[i])
            pos = "layer 0" if i == 0 else "middle layer"
            if rep["bwd"] == "ig_bwd_pair":
                (ksplit, tpw, chunks, per, wn8) = (int(rep[k]) for k in ("ig_ksplit", "ig_tpw", "ig_chunks", "ig_per", "ig_wn8"))
                assert wn8 == (chunks + 7) // 8
                reached |= {("ig", "ksplit", ksplit), ("ig", "tpw", tpw), ("ig", "per 32") if per == 32 else ("ig", "per > 32"),
                            ("ig", "chunks 1") if chunks == 1 else (("ig", "chunks 2..8") if chunks <= 8 else ("ig", "chunks > 8")),
                            ("ig", "taps", kh, kw)}
                if ci % 16:
                    reached.add(("ig", "ragged cin"))
                if at_2[f"dec{i}"]["bwd"] == "ct_bwd_lds":
                    # the LDS-staged kernel takes this layer at batch 2: what gives it back is the bound on the images per
                    # accumulator address (no more images per workgroup than the staging registers hold, so at least this
                    # many groups)
                    imgs_cap = min(4 * 7 * kCtbThreads // (co * oh * ow), 4 * 2 * kCtbThreads // (16 * h * w))
                    assert ci * co * 9 * -(-batch // imgs_cap) > 400000, what
                    reached.add(("given back above 400000",))
                if mode == 3 and (kh, kw) == (3, 3) and ci % 16 == 0 and co == 48 and at_2[f"dec{i}"]["bwd"] == "ig_bwd_pair":
                    assert 16 * co * 9 > 4 * 3 * kCtbThreads   # the block's weight rows against kCtbW4 pieces per thread
                    reached.add(("cout 48 does not fit",))
                continue
            (kernel, imgs, groups, parts, bands, hb, sharded) = (rep["ctb_kernel"], *(int(rep[k]) for k in (
                "ctb_imgs", "ctb_groups", "ctb_parts", "ctb_bands", "ctb_hb", "ctb_sharded")))
            assert (kh, kw) == (3, 3) and ci % 16 == 0 and groups == -(-batch // imgs), what
            assert sharded == (ci == 16), what   # the automatic mask's layers have the sharded accumulator
            reached |= {("ct", "cout", co), ("ct", "sharded", bool(sharded)), (kernel, pos)}
            if kernel == "band":
                assert imgs == 1 and bands == parts >= 2 and bands == -(-h // hb), what
                reached |= {("band", "bands", bands), ("band", "blocks", min(ci // 16, 3)), ("band", "square", h == w)}
                reached.add(("band", "hb 1") if hb == 1 else ("band", "full last band" if h % hb == 0 else "short last band"))
                if batch % 2:
                    reached.add(("band", "odd batch"))
            else:
                assert bands == 0 and hb == 0, what
                last = "whole last group" if batch % imgs == 0 else "short last group"
                if imgs == 1 and parts == 1:
                    reached.add(("lds", "imgs 1", "parts 1"))
                elif imgs == 1:
                    # workgroups to spare and yet no bands: which of the band kernel's two staging conditions refused
                    hb_ = -(-h // parts)
                    assert -(-h // hb_) > 1, what
                    (gstr, astr) = ((2 * hb_ + 1) * ow, hb_ * w)
                    assert co * gstr > 8 * kCtbThreads or 16 * astr > 2 * kCtbThreads, what
                    if co * gstr > 8 * kCtbThreads:
                        reached.add(("lds", "imgs 1", "parts > 1", "refused: Cout * gstr"))
                    if 16 * astr > 2 * kCtbThreads:
                        reached.add(("lds", "imgs 1", "parts > 1", "refused: 16 * astr"))
                elif parts > 1:
                    reached.add(("lds", "imgs > 1", "parts > 1", last, f"mode {mode}"))
                else:
                    reached.add(("lds", "imgs > 1", "parts 1", last))
    return reached


def test_cases_reach_what_they_name():
    """every case's layers are on the kernel, and launched with the fields, that CASES lists (EnginePlan.kernel_plan, no GPU);
    the cases respect the size caps; together they reach WANT; and WANT is what the module's docstring lists"""
    reached = _reached(CASES)
    assert WANT <= reached, sorted(map(str, WANT - reached))
    # a short last group with parts > 1 needs mode 3: in the default mode only 16->8 layers stage whole images, and their
    # imgs > 1 with parts > 1 lies at batches that are multiples of imgs for the cases here
    assert ("lds", "imgs > 1", "parts > 1", "short last group", "mode 1") not in reached


def test_sweep_reaches_no_ksplit_1_plan():
    """ig_bwd_plan's ksplit = 1 (at most 12 k-steps: Cout * KH * KW <= 48) is out of a sizer-made decoder's reach: layers that
    thin are all stride-2-specialised.  The sweep of test_engine_plan_cpu.py, in the default mode and in mode 3."""
    seen = set()
    for out_c in (1, 2, 3):
        for out_h in range(60, 301, 3):
            for out_w in sorted({out_h, out_h + 1, 63, 64, 100, 129, 255, 256}):
                if not 60 <= out_w <= 300:
                    continue
                try:
                    spec = _spec(out_c, out_h, out_w).save()
                except Exception:   # the sizer finds no decoder for this size
                    continue
                for mode in (1, 3):
                    for batch in (2, 32, 512):
                        plan = _plan(spec, batch, mode)
                        seen |= {int(v["ig_ksplit"]) for (k, v) in plan.items() if v.get("bwd") == "ig_bwd_pair"}
    assert seen == {2, 4}, seen


def _ratio(got, ref32, exact64):
    """|got - exact| over assert_close_as_reference's bound (its default factor and floors)"""
    (got, ref32, exact64) = (np.asarray(a, dtype=np.float64) for a in (got, ref32, exact64))
    bound = 3.0 * float(np.abs(ref32 - exact64).max()) + 1e-5 * float(np.abs(exact64).max()) + 1e-9
    return float(np.abs(got - exact64).max()) / bound


@pytest.mark.gpu
@pytest.mark.parametrize("geometry,batch,case_mode,generic_too,layers", CASES, ids=_IDS)
def test_training_step_and_scoring_against_fp64_oracle(geometry, batch, case_mode, generic_too, layers):
    from oracle import cae_oracle as orc
    (out_c, out_h, out_w) = geometry
    spec, enc_sd, dec_sd, xb, tb = _model(out_c, out_h, out_w, batch, seed=out_h * 7 + out_w + out_c)
    noisy = bn_bias_keys(spec.save())
    y_ref = orc.OracleModel(spec.save(), enc_sd, dec_sd).eval_forward(xb).numpy()
    d64 = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    for mode in ((case_mode, 0) if generic_too else (case_mode,)):
        what = f"{geometry} B={batch} mode={mode}"
        eng = _engine(spec, enc_sd, dec_sd, xb, tb, batch, mode)
        if mode == case_mode:
            plan = eng.kernel_plan(batch, True)
            for (i, rep) in layers.items():
                assert _bwd_report(plan[f"dec{i}"]) == rep, (what, plan)
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
        ratios = {"loss": _ratio([loss], [float(loss32)], [float(loss64)])}
        ratios.update({k: _ratio(got[k], g32.numpy(), g64[k].numpy()) for k, g32 in ref32.grads().items() if k not in noisy})
        top = sorted(((r, k) for k, r in ratios.items()), reverse=True)[:3]
        print(f"\n[ct bwd shapes] {what}: worst |hip-fp64|/bound {top[0][0]:.3f} ({top[0][1]}), next "
              f"{[(round(r, 3), k) for r, k in top[1:]]}; score max|diff| {err:.2e}")
        assert_close_as_reference([loss], [float(loss32)], [float(loss64)], f"{what} loss")
        for k, g32 in ref32.grads().items():
            if k in noisy:
                # exactly zero in exact arithmetic: magnitude only
                assert np.abs(got[k]).max() <= 1e-6 + 1e-4 * float(g32.abs().max()), f"{what} {k}"
                continue
            assert_close_as_reference(got[k], g32.numpy(), g64[k].numpy(), f"{what} {k}")


_DEFAULT = [(g, b) for (g, b, m, _, _) in CASES if m == 1]


@pytest.mark.gpu
@pytest.mark.parametrize("geometry,batch", _DEFAULT, ids=["x".join(map(str, g)) + f"-{b}" for (g, b) in _DEFAULT])
def test_two_runs_of_two_steps_give_the_same_bits(geometry, batch):
    (out_c, out_h, out_w) = geometry
    spec, enc_sd, dec_sd, x, t = _model(out_c, out_h, out_w, 2 * batch, seed=5)
    runs = []
    for _ in range(2):
        eng = _engine(spec, enc_sd, dec_sd, x, t, batch, 1)
        losses = [eng.train_step(0, None, k * batch, batch) for k in range(2)]
        eng.sync()
        runs.append((losses, eng.params.cpu(), eng.exp_avg.cpu(), eng.exp_avg_sq.cpu(), eng.buffers.cpu()))
        eng.close()
    (a, b) = runs
    assert a[0] == b[0], ("losses", a[0], b[0])
    for (u, v, name) in zip(a[1:], b[1:], ("params", "exp_avg", "exp_avg_sq", "running statistics")):
        assert torch.equal(u, v), f"{geometry} B={batch}: {name} differ in {int((u != v).sum())} of {u.numel()} entries"
