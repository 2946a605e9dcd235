"""shared helpers of the UNET tests: golden-case loading (tests/golden/unet_*.npz|json, written by
tests/golden/make_golden_unet.py from the reference's own class bodies)"""
import glob
import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UNET_CASES = sorted(os.path.basename(p)[5:-5] for p in glob.glob(os.path.join(GOLDEN, "unet_*.json")))
TRAIN_CASES = [c for c in UNET_CASES if "eval" not in c]

# the UNET geometries tests/test_unet_hip_parity.py runs against the oracle and the generic kernels, beside the golden
# cases; tests/test_unet_plan_cpu.py checks which kernel families each reaches.  id -> (in_ch, out_ch, (h, w), channels,
# fc, latent, batch)
MEDIUM_CASES = {
    "64px_32-64-96": (3, 3, (64, 64), [32, 64, 96], 24, 6, 5),
    "128px_16-32-64-72": (3, 3, (128, 128), [16, 32, 64, 72], 20, 5, 3),
}
DEEP_CASES = {
    # five levels: nine layers with repacked weights (two repack launches)
    "5lvl_256px_16-256": (3, 3, (256, 256), [16, 32, 64, 128, 256], 24, 6, 4),
    # six levels to a 1x1 bottleneck: attention with one hidden unit, BatchNorm over the batch alone at the bottom, ten
    # repacked layers
    "6lvl_64px_1x1": (1, 1, (64, 64), [8, 8, 16, 16, 16, 16], 16, 4, 6),
    # 512 px: 256-wide image-end maps (too wide for the thin kernels), eight repacked layers (one launch, exactly full)
    "512px_8-8-16-16-32": (3, 3, (512, 512), [8, 8, 16, 16, 32], 20, 5, 3),
    # a 5x7 bottleneck of 34 channels: Linear layers of 1190 inputs (not a multiple of 4: the Linear tile engine), 34-channel
    # layers the tile engine's OpUp does not take (no repacked weights: the generic transposed convolution)
    "20x28_34ch": (2, 2, (20, 28), [16, 34], 12, 5, 5),
}


class UnetCase:

    def __init__(self, name):
        with open(os.path.join(GOLDEN, f"unet_{name}.json")) as f:
            self.meta = json.load(f)
        self.z = dict(np.load(os.path.join(GOLDEN, f"unet_{name}.npz")))
        if "x0" not in self.z:   # compact cases (make_golden_unet.py) store the first batch once, as step 0's
            for (k, src) in (("x0", "step0/x"), ("t0", "step0/t"), ("m0", "step0/m")):
                self.z[k] = self.z[src]
        self.name = name

    def state(self, prefix, which):
        keys = self.meta["enc_keys"] if which == "enc" else self.meta["dec_keys"]
        return {k: torch.from_numpy(self.z[f"{prefix}/{which}/{k}"].copy()) for k in keys}

    def t(self, key):
        return torch.from_numpy(self.z[key].copy())

    def step_batch(self, i):
        return self.t(f"step{i}/x"), self.t(f"step{i}/t"), self.t(f"step{i}/m")


def unet_oracle(case, prefix="init", **kw):
    from oracle import unet_oracle as uo
    m = case.meta
    args = dict(lr=m["lr"], weight_decay=m["weight_decay"], dropout_rate=m["dropout"], lambda_pearson=m["lambda_pearson"])
    args.update(kw)
    return uo.UnetOracle(m["spec"], case.state(prefix, "enc"), case.state(prefix, "dec"), **args)


def hip_relu_decisions(eng, spec_json, fc, latent, B):
    """(output > 0) at every ReLU site of the HIP engine's last training forward, for oracle.unet_oracle.ReluAlign: the
    encoder skips (ReLU outputs), the four Linear activations and the decoder inputs (after their dropout: a False there may
    also mean 'dropped', which ReluAlign is indifferent to)"""
    dec = {}
    for i, l in enumerate(spec_json["input_layers"]):
        (c, h, w) = l["output_dimensions"]
        dec[f"enc{i}"] = eng.debug_read(f"enc_s{i}", B * c * h * w) > 0
    (c2, h2, w2) = spec_json["output_layers"][0]["input_dimensions"]
    for k, (name, n) in enumerate((("efc0", fc), ("efc1", latent), ("dfc0", fc), ("dfc1", c2 * h2 * w2))):
        dec[name] = eng.debug_read(f"fc_a{k}", B * n) > 0
    for j, l in enumerate(spec_json["output_layers"][:-1]):
        (c, h, w) = l["output_dimensions"]
        dec[f"dec{j}"] = eng.debug_read(f"dec_din{j + 1}", B * 2 * c * h * w) > 0
    return dec


def hip_argmax_decisions(eng, spec_json, B):
    """{'att{j}': (B, C) flat index of the FIRST maximum of each (b, c) plane of the gated map u} at every attention gate of
    the HIP engine's last forward, for oracle.unet_oracle.ArgmaxAlign.  k_pool keeps the first maximum; `u` is written by the
    forward's transposed convolution alone (the backward only reads it), so after forward_backward it still holds the values
    the gate pooled - until the next forward (score() included) overwrites it."""
    out = {}
    for j, l in enumerate(spec_json["output_layers"][:-1]):
        (c, h, w) = l["output_dimensions"]
        u = eng.debug_read(f"dec_u{j}", B * c * h * w).reshape(B, c, h * w)
        out[f"att{j}"] = np.argmax(u, axis=2)
    return out


def feeds_batchnorm(key):
    """biases added right before a BatchNorm: their exact gradient is 0 (BatchNorm removes any per-channel constant), so
    every implementation holds rounding noise there"""
    return key.endswith(".bias") and (("encoder_cnn." in key and int(key.split(".")[1]) % 4 == 0)
                                      or "encoder_lin.0." in key or "decoder_lin.0." in key)


# a bias in front of a BatchNorm: the golden tests' bound on its rounding-sized gradient
BN_BIAS_ROUNDING = 2e-5


def grad_ratios(got, want32, want64, factor=3.0, floor_rel=1e-5, floor_abs=1e-9):
    """{key: (|got - fp64|, bound, |fp32 - fp64|)} in the max norm, bound = factor * |fp32 - fp64| + floor_rel * max|fp64| +
    floor_abs: tests/helpers.py assert_close_as_reference's criterion, per gradient tensor"""
    out = {}
    for k, w64 in want64.items():
        if feeds_batchnorm(k):
            continue
        w64 = np.asarray(w64, dtype=np.float64)
        g = np.asarray(got[k], dtype=np.float64)
        own = float(np.abs(np.asarray(want32[k], dtype=np.float64) - w64).max())
        err = float(np.abs(g - w64).max())
        out[k] = (err, factor * own + floor_rel * float(np.abs(w64).max()) + floor_abs, own)
    return out


def assert_unet_grads(got, want32, want64, what, factor=3.0, floor_rel=1e-5, floor_abs=1e-9, factors=None):
    """every gradient tensor of `got` (the HIP engine's) against the fp64 oracle's: no further from it than `factor` times the
    fp32 oracle's own error on that tensor (+ floor_rel of the tensor's largest fp64 entry + floor_abs).  The three come from
    one step under the same ReLU / argmax alignment.  `factors`: {key: factor} overrides for single tensors.  Biases in front
    of a BatchNorm must be rounding-sized on all three sides.  Returns the worst err / bound over the tensors."""
    with_override = dict(factors or {})
    worst = 0.0
    for k, w64 in want64.items():
        if not feeds_batchnorm(k):
            continue
        sizes = [float(np.abs(np.asarray(v[k], dtype=np.float64)).max()) for v in (got, want32, want64)]
        assert max(sizes) <= BN_BIAS_ROUNDING, \
            f"{what}: {k} feeds a BatchNorm, its gradient must be rounding-sized: max |hip| {sizes[0]:.3e}, |fp32| {sizes[1]:.3e}, |fp64| {sizes[2]:.3e}"
    for k in want64:
        if feeds_batchnorm(k):
            continue
        f = with_override.get(k, factor)
        ((err, bound, own),) = grad_ratios({k: got[k]}, {k: want32[k]}, {k: want64[k]}, f, floor_rel, floor_abs).values()
        assert err <= bound, (f"{what}: {k}: |hip - fp64| {err:.3e} > bound {bound:.3e} ({f:g} x the fp32 oracle's own "
                              f"error {own:.3e} + {floor_rel:g} x max|fp64| {float(np.abs(np.asarray(want64[k])).max()):.3e})")
        worst = max(worst, err / bound)
    return worst


def aligned_oracle_grads(spec_json, enc_sd, dec_sd, x, t, m, relu=None, argmax=None, dropout_rate=0.0, seed=0, step=0,
                         relu_tol=1e-5, argmax_tol=1e-5, lambda_pearson=1.0):
    """one training forward + backward of the fp32 and then the fp64 oracle, both under ReluAlign(relu) and
    ArgmaxAlign(argmax) with the same windows; the fp32 graph is freed before the fp64 one is built.  Returns
    (fp32 oracle, (mse, pearson) of fp32, fp32 grads, fp64 grads, alignment report of both sides)"""
    import gc
    from oracle import unet_oracle as uo
    to64 = lambda sd: {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    report = {}
    res = []
    for (dt, enc, dec, xs) in (("fp32", enc_sd, dec_sd, (x, t, m)), ("fp64", to64(enc_sd), to64(dec_sd),
                                                                      (x.double(), t.double(), m.double()))):
        o = uo.UnetOracle(spec_json, enc, dec, dropout_rate=dropout_rate, seed=seed, lambda_pearson=lambda_pearson)
        o.step_count = step
        with uo.ReluAlign(relu or {}, tol=relu_tol) as ra, uo.ArgmaxAlign(argmax or {}, tol=argmax_tol) as aa:
            (mse, pl, _) = o.loss_and_grads(*xs)
        report[dt] = dict(relu=sum(ra.followed.values()), relu_worst=ra.worst, argmax=sum(aa.followed.values()),
                          argmax_worst=aa.worst, relu_sites=dict(ra.followed))
        res.append((o if dt == "fp32" else None, (mse, pl), o.grads()))
        del o
        gc.collect()
    (o32, losses, g32) = res[0]
    return o32, losses, g32, res[1][2], report


def _grad_dict(eng, flat):
    flat = flat.cpu()
    return {n: flat[off:off + numel].view(shape) for n, (arena, off, numel, shape) in eng.tensors.items() if arena == 0}


# Alignment windows.  ReLU: a BatchNorm output that the HIP run and an oracle put on different sides of zero is followed where
# the oracle's own value is within RELU_TOL of zero.  Measured over every geometry of this file (Row 1): with
# dropout off (cfg3 batch 32, 28 decisions followed) every followed decision is a noise flip, the worst at |z| = 4.0e-6; a
# 1e-5 window left the dropout-on geometries at up to 9.8e-6.  So the window is 1e-4, 10x the largest.  (With dropout on, a
# HIP 'False' may also be a dropped element, which then fills the window: harmless, the element is zero either way.)
# Max-pool: a HIP index is followed where the oracle's value there is within ARGMAX_TOL of its own maximum; the one gap
# followed measured 4.8e-7 (64 px, generic kernels): 1e-5 is 20x that.
RELU_TOL = 1e-4
ARGMAX_TOL = 1e-5
# Count caps.  A decision can differ only where |z| is within the noise of zero.  With N ReLU outputs of unit-variance
# BatchNorm (density ~0.4 at zero) and a noise of at most RELU_TOL / 10 = 1e-5, the expected count is N x 0.4 x 2e-5 =
# 8e-6 N; the cap is that plus 8: 488 at cfg3 batch 32 (N ~ 6e7), where 28 were followed.  The gate pools B x C planes of
# 1e2 .. 1e5 entries; two entries at the top within 1e-6 of each other showed up once in all the planes of this file
# (~2e4): 4 is generous.
ARGMAX_CAP = 4


def relu_cap(decisions):
    return 8 + math.ceil(8e-6 * sum(np.asarray(v).size for v in decisions.values()))


def _check_alignment(rep, relu, what):
    cap = relu_cap(relu)
    for side in ("fp32", "fp64"):
        r = rep[side]
        assert r["relu"] <= cap, (f"{what} ({side} oracle): {r['relu']} ReLU decisions followed > cap {cap} (worst |z| followed "
                                  f"{r['relu_worst']:.2e}; per site {r['relu_sites']})")
        assert r["argmax"] <= ARGMAX_CAP, (f"{what} ({side} oracle): {r['argmax']} max-pool decisions followed > {ARGMAX_CAP} "
                                           f"(worst gap followed {r['argmax_worst']:.2e})")


def _against_aligned_oracles(eng, spec_json, enc_sd, dec_sd, x, t, m, fc, latent, what, dropout_rate=0.0, seed=0, step=0,
                             lambda_pearson=1.0, loss_rtol=3e-5):
    """one forward_backward of `eng` (dataset 0 set, its hyper-parameters matching the arguments) against the fp32 and fp64
    oracles, both following this run's ReLU and max-pool decisions where they cannot decide them: losses, every gradient
    tensor through assert_unet_grads.  Returns (fp32 oracle, HIP gradients, worst ratio, alignment report)"""
    B = x.shape[0]
    grads = _grad_dict(eng, eng.forward_backward(0, None, 0, B, slot=0))
    got_losses = eng.read_losses(0, 1)[0]
    # (read before anything else overwrites the activations: score() would)
    relu = hip_relu_decisions(eng, spec_json, fc, latent, B)
    amax = hip_argmax_decisions(eng, spec_json, B)
    (o32, losses, g32, g64, rep) = aligned_oracle_grads(spec_json, enc_sd, dec_sd, x, t, m, relu, amax, dropout_rate=dropout_rate,
                                                        seed=seed, step=step, relu_tol=RELU_TOL, argmax_tol=ARGMAX_TOL,
                                                        lambda_pearson=lambda_pearson)
    ratios = grad_ratios(grads, g32, g64)
    top = sorted(((e / b, k) for k, (e, b, _) in ratios.items()), reverse=True)[:3]
    print(f"\n[unet parity] {what}: worst |hip-fp64|/bound {top[0][0]:.3f} ({top[0][1]}), next {[(round(r, 3), k) for r, k in top[1:]]}; "
          f"ReLU followed {rep['fp32']['relu']}/{rep['fp64']['relu']} (cap {relu_cap(relu)}) worst |z| "
          f"{max(rep['fp32']['relu_worst'], rep['fp64']['relu_worst']):.2e}; argmax followed {rep['fp32']['argmax']}/"
          f"{rep['fp64']['argmax']} worst gap {max(rep['fp32']['argmax_worst'], rep['fp64']['argmax_worst']):.2e}")
    _check_alignment(rep, relu, what)
    np.testing.assert_allclose(got_losses, losses, rtol=loss_rtol)
    worst = assert_unet_grads(grads, g32, g64, what)
    return o32, grads, worst, rep


# ---- below the kernel family: what the launch code switches on (tests/test_unet_shapes_cpu.py, test_unet_shapes_gpu.py) ----
# id -> (in_ch, out_ch, (h, w), channels, fc, latent, batches, max_batch): the geometries tests/test_unet_shapes_gpu.py runs
# against the fp64 oracle.  tests/test_unet_shapes_cpu.py pins the plan fields each is aimed at and checks that, with the
# rows of tests/test_unet_plan_cpu.py, they reach every cell of SHAPE_BRANCHES.
SHAPE_CASES = {
    # flat 1296 = 10 * 128 + 16: 11 K slices with a 16-wide last tile.  Batch 33: RB 2 with one row in the second block;
    # 40 / 57: k_lin_outer below / above 64 KiB of LDS, B % 8 of 0 and 1; 64 -> 65: the big layers drop to the tile engine
    "lin_k1296": (2, 2, (24, 24), [8, 36], 12, 4, (33, 40, 57, 64, 65), 96),
    # N = 132: a 4-wide second column tile on the sliced forward; the input gradient's two slices, the second 4 long; the
    # fold without a bias; k_lin_outer's grid y = 2; batch 61 pads to 64 rows
    "lin_fc132": (2, 2, (32, 32), [8, 24], 132, 8, (5, 61), 61),
    # fc > 1024: all four Linear layers on the big kernels, K = 4 and N = 4 among them, 9 slices with a 4-wide remainder
    "lin_fc1028": (1, 1, (32, 32), [8, 24], 1028, 4, (3, 34), 34),
    # k_thin_down<1,2> and <2,4>, k_up_thin<4>, 3 tiles per image (fewer than a group of 8)
    "thin_c2_c4": (2, 4, (24, 64), [32, 8], 8, 4, (3,), 3),
    # k_thin_down<2,4> with 10 tiles per image: groups of 8 and 2
    "thin_c4_short": (4, 2, (80, 64), [40, 8], 8, 4, (2,), 2),
    # 128-wide thin maps (one map row per tile): k_thin_up<1|4|2, 2> with 6 waves in 2 workgroups (two idle waves),
    # k_thin_down<2,1> (48 channels)
    "wide_c1": (1, 1, (8, 256), [24, 8], 8, 4, (3,), 3),
    "wide_c2_c4": (2, 4, (8, 256), [16, 8], 8, 4, (3,), 3),
    "wide_c4_c2": (4, 2, (8, 256), [32, 8], 8, 4, (3,), 3),
    # k_pdown and k_pup on 128-wide maps
    "wide_patch128": (8, 32, (8, 256), [32, 16], 8, 4, (3,), 3),
    # k_pdown<4> with two K slices and k_pup<2> on 16-wide maps; RB 2 at 768 K slices
    "tall_rbn4": (3, 3, (256, 64), [64, 96], 12, 4, (33,), 33),
    # the tile engine's OpDown cells no other test reaches: 64 x 256 with 1 and > 2 slices, 32 x 512 with > 2, 128 x 128 with 1
    "mfma_cells": (2, 2, (48, 48), [8, 40, 32, 24], 12, 4, (3,), 3),
    # the 4-wave weight-gradient tiles with fp64 atomics: one batch BELOW max_batch needs more K slices than max_batch does
    # (8 chunks per slice up to 4096 chunks, 9 from there), so its partial tiles do not fit the buffer sized at max_batch
    "wgrad_atomics_32": (12, 2, (64, 64), [20, 8], 8, 4, (64,), 65),
    "wgrad_atomics_64": (12, 12, (64, 64), [20, 8], 8, 4, (64,), 65),
    "wgrad_atomics_128": (12, 12, (64, 64), [72, 8], 8, 4, (32,), 33),
}


def _slice_class(n):
    n = int(n)
    return "1" if n == 1 else "2" if n == 2 else ">2"


def _lin_k_class(slices, partial):
    """one K slice (direct store) / several with a whole last tile / several with a partly filled last tile"""
    return "one" if int(slices) == 1 else "partial" if partial == "1" else "whole"


def plan_cells(plan):
    """{cell}: the template instantiation, K-slice regime and LDS regime of every launch of one kernel_plan (UnetPlan), as
    tuples that begin with the op and the family"""
    out = set()
    for name, f in plan.items():
        if name == "pack":
            continue
        down, up, wgrad = f.get("down", "-"), f.get("up", "-"), f.get("wgrad", "-")
        if down == "thin":
            out.add(("down", "thin", f"rbn{f['down.rbn']}", f"cl{f['down.cl']}"))
        elif down == "patch":
            out.add(("down", "patch", f"rbn{f['down.rbn']}", _slice_class(f["down.nsplit"])))
        elif down == "mfma":
            out.add(("down", "mfma", f["down.tile"], _slice_class(f["down.nsplit"])))
        if up in ("thin", "up_thin"):
            out.add(("up", up, f"cl{f['up.cl']}"))
        elif up == "patch":
            out.add(("up", "patch", f"rbn{f['up.rbn']}"))
        elif up == "mfma":
            out.add(("up", "mfma", f["up.tile"]))
        if wgrad in ("thin", "thin_atomic"):
            out.add(("wgrad", "thin", f"rbn{f['wgrad.rbn']}"))
        elif wgrad == "patch":
            out.add(("wgrad", "patch", f["wgrad.wrxwc"]))
        elif wgrad in ("mfma", "mfma_atomic"):
            out.add(("wgrad", "mfma", f["wgrad.tile"], "partial_tiles" if wgrad == "mfma" else "atomics"))
        fwd = f.get("fwd", "-")
        if fwd == "lin_big":
            out.add(("fwd", "lin_big", f"rb{f['fwd.rb']}", _lin_k_class(f["fwd.slices"], f["fwd.partial"])))
            if f.get("bwd", "-") == "lin_big":
                out.add(("bwd", "lin_big", f"rb{f['bwd.rb']}", _lin_k_class(f["bwd.slices"], f["bwd.partial"])))
                out.add(("bwd", "lin_outer", "lds>64K" if int(f["outer_lds"]) > 65536 else "lds<=64K"))
        elif fwd in ("tile", "gemm16"):
            out.add(("fwd", fwd))
            if f.get("bwd", "-") == fwd:
                out.add(("bwd", fwd))
    return out
