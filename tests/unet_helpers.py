"""shared helpers of the UNET tests: golden-case loading (tests/golden/unet_*.npz|json, written by
tests/golden/make_golden_unet.py from the reference's own class bodies)"""
import glob
import json
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
