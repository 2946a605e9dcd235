"""Which kernels the UNET engine runs, read from the choosers its launch code switches on (unet_debug_plan in
include/cae_unet.h, UnetPlan.kernel_plan), without a GPU:
- every layer with a repack buffer that runs OpUp has its weights repacked before the step, at any depth (the repack
  launch takes 8 layers; a ninth used to be dropped silently and ran on a zero-filled buffer);
- the geometries of the GPU parity tests reach the kernel families their docstrings name, and together every branch of
  the choosers but the ones listed in UNREACHABLE, which no valid UNET reaches (checked over a sweep of specs)."""
import itertools
import random

import pytest

from unet_helpers import DEEP_CASES, MEDIUM_CASES, TRAIN_CASES, UNET_CASES, UnetCase

from cae_tools_amd.models.unet import unet_layer_spec
from cae_tools_amd.unet_engine import UnetPlan

PACK_PER_LAUNCH = 8                   # PackSet (kernels_unet_mfma.h): layers one k_pack_up_weights launch repacks
READS_WP = {"thin", "patch", "mfma"}  # the OpUp families that read the repacked weights (k_up_thin<CL> and k_up read w)

# every branch of choose_down / choose_up / choose_wgrad / choose_lin (csrc/unet_engine.hip)
BRANCHES = {("down", f) for f in ("thin", "patch", "mfma", "generic")} | \
           {("up", f) for f in ("thin", "up_thin", "patch", "mfma", "generic")} | \
           {("wgrad", f) for f in ("thin", "thin_atomic", "patch", "mfma", "mfma_atomic", "generic")} | \
           {(op, f) for op in ("fwd", "bwd") for f in ("lin_big", "gemm16", "tile", "generic")}
# (layer kind, op, family) that no valid UNET reaches, and why
UNREACHABLE = {
    ("enc", "wgrad", "thin_atomic"): "the partial-tile buffer is sized for every thin layer at max_batch, and a thin weight "
                                     "gradient's partial tiles grow with the batch",
    ("dec", "wgrad", "thin_atomic"): "as for the encoder",
    # an encoder layer's OpUp writes the gradient of the previous layer's output, whose channels also feed a skip
    # connection into a ChannelAttention (>= 8 channels); the thin OpUp kernels take <= 4 output channels
    ("enc", "up", "thin"): "the thin-order repack of an encoder layer would need <= 4 channels on a skip connection",
    ("enc", "up", "up_thin"): "k_up_thin<CL> would need <= 4 channels on a skip connection",
}


def _plan(spec, fc, latent, batch, train, specialised=True, max_batch=None):
    p = UnetPlan(spec, fc, latent, max_batch or batch)
    p.set_kernel_mode(specialised)
    try:
        return p.kernel_plan(batch, train)
    finally:
        p.close()


def _conv_layers(plan):
    return {k: v for k, v in plan.items() if k[:3] in ("enc", "dec")}


def _reached(plan):
    """{(layer kind, op, family)} of one plan"""
    out = set()
    for name, fields in plan.items():
        if name == "pack":
            continue
        for op in ("down", "up", "wgrad", "fwd", "bwd"):
            if fields.get(op, "-") != "-":
                out.add((name.rstrip("0123456789"), op, fields[op]))
    return out


# ---- repack coverage ---------------------------------------------------------------------------------
# id -> (unet_layer_spec arguments, fc, latent, batch, layers repacked in a training step)
REPACK_SPECS = {
    "d1_8px": ((2, 2, (8, 8), [8]), 6, 3, 3, 0),
    "d2_24x16": ((2, 1, (24, 16), [8, 24]), 10, 4, 4, 2),
    "d3_64px": ((3, 3, (64, 64), [32, 64, 96]), 24, 6, 5, 4),
    "d4_cfg3": ((3, 3, (256, 256), [32, 64, 128, 256]), 128, 32, 5, 7),
    "d4_cfg3_b32": ((3, 3, (256, 256), [32, 64, 128, 256]), 128, 32, 32, 7),
    "d5_256px": ((3, 3, (256, 256), [16, 32, 64, 128, 256]), 24, 6, 4, 9),
    "d5_512px": ((3, 3, (512, 512), [8, 8, 16, 16, 32]), 20, 5, 3, 8),
    "d6_64px_1x1": ((1, 1, (64, 64), [8, 8, 16, 16, 16, 16]), 16, 4, 4, 10),
    "d6_64px_8ch": ((1, 1, (64, 64), [8, 8, 8, 8, 8, 8]), 16, 4, 4, 10),     # the golden case u_deep6_b4
    "d6_256px": ((3, 3, (256, 256), [8, 16, 16, 32, 32, 32]), 16, 4, 4, 11),
    "d7_128px_1x1": ((1, 1, (128, 128), [8, 8, 8, 16, 16, 16, 16]), 16, 4, 4, 12),
}


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", REPACK_SPECS)
def test_every_layer_with_a_repack_buffer_is_repacked(name, train):
    (args, fc, latent, batch, want_train) = REPACK_SPECS[name]
    plan = _plan(unet_layer_spec(*args), fc, latent, batch, train)
    n = sum(k.startswith("enc") for k in plan)
    assert n == len(args[3])
    packed = []
    for layer, f in _conv_layers(plan).items():
        runs_up = layer.startswith("dec") or (train and layer != "enc0")
        if f["up"] in READS_WP:
            assert f["wp"] == "1", f"{layer}: OpUp family {f['up']} without a repack buffer"
        if runs_up and f["wp"] == "1":
            assert f["packed"] == "1", f"{layer} has a repack buffer and runs OpUp ({f['up']}), but its weights are never repacked"
        if f["packed"] == "1":
            assert runs_up and f["wp"] == "1", f"{layer} is repacked but does not use it"
            packed.append(layer)
    assert int(plan["pack"]["entries"]) == len(packed)
    assert int(plan["pack"]["launches"]) == (len(packed) + PACK_PER_LAUNCH - 1) // PACK_PER_LAUNCH
    if train:
        assert len(packed) == want_train, plan


def test_generic_kernels_repack_nothing():
    (args, fc, latent, batch, _) = REPACK_SPECS["d6_64px_1x1"]
    plan = _plan(unet_layer_spec(*args), fc, latent, batch, True, specialised=False)
    assert plan["pack"] == {"entries": "0", "launches": "0"}
    for layer, f in _conv_layers(plan).items():
        assert f["packed"] == "0" and f["down"] == f["wgrad"] == "generic" and f["up"] == ("-" if layer == "enc0" else "generic"), layer


CFG3_PLAN = {   # the benchmark geometry's training step: one repack launch for its seven layers
    "enc0": "thin/-/thin", "enc1": "patch/patch/patch", "enc2": "patch/patch/patch", "enc3": "patch/patch/patch",
    "dec0": "patch/patch/patch", "dec1": "patch/patch/patch", "dec2": "patch/patch/patch", "dec3": "thin/thin/thin",
}


@pytest.mark.parametrize("batch", [5, 32])
def test_benchmark_geometry_plan(batch):
    plan = _plan(unet_layer_spec(3, 3, (256, 256), [32, 64, 128, 256]), 128, 32, batch, True)
    assert {k: "/".join((f["down"], f["up"], f["wgrad"])) for k, f in _conv_layers(plan).items()} == CFG3_PLAN
    assert [plan[f"fc{k}"]["fwd"] for k in range(4)] == ["lin_big", "gemm16", "gemm16", "lin_big"]
    assert plan["pack"] == {"entries": "7", "launches": "1"}
    assert all(f["packed"] == "1" for k, f in _conv_layers(plan).items() if k != "enc0")


def test_plan_arguments():
    from cae_tools_amd._lib import CaeError
    p = UnetPlan(unet_layer_spec(2, 2, (8, 8), [8]), 6, 3, 4)
    with pytest.raises(CaeError, match="outside 1 .. 4"):
        p.kernel_plan(5, True)
    with pytest.raises(CaeError, match="needs"):
        import ctypes as C
        from cae_tools_amd._lib import check
        check(p.lib.unet_debug_plan(p.handle, 4, 1, C.create_string_buffer(16), 16))
    p.close()


# ---- dispatch coverage -------------------------------------------------------------------------------
def _row(test, spec, fc, latent, batches, modes=(True, False), claims=(), max_batch=None):
    return dict(test=test, spec=spec, fc=fc, latent=latent, batches=batches, modes=modes, claims=set(claims), max_batch=max_batch)


CFG3 = unet_layer_spec(3, 3, (256, 256), [32, 64, 128, 256])
# what the GPU tests of tests/test_unet_hip_parity.py run: spec, batches (train, eval), kernel modes, and the families the
# test's docstring names as (layer kind, op, family)
GPU_ROWS = {
    **{f"golden_{n}": _row("test_eval_forward_and_losses / test_train_forward_backward / test_adamw_steps",
                           UnetCase(n).meta["spec"], UnetCase(n).meta["fc"], UnetCase(n).meta["latent"],
                           {(UnetCase(n).meta["batch"], False)} | ({(UnetCase(n).meta["batch"], True),
                                                                    (max(UnetCase(n).meta["batch"] - 1, 2), True)}
                                                                   if n in TRAIN_CASES else set()))
       for n in UNET_CASES},
    "medium_64px": _row("test_mfma_path_at_medium_size_against_oracle_and_generic_kernels[64px_32-64-96]",
                        unet_layer_spec(*MEDIUM_CASES["64px_32-64-96"][:4]), *MEDIUM_CASES["64px_32-64-96"][4:6],
                        {(5, True), (5, False)},
                        claims={("enc", "down", "thin"), ("enc", "down", "patch"), ("enc", "down", "mfma"),
                                ("fc", "fwd", "lin_big"), ("fc", "fwd", "gemm16")}),
    "medium_128px": _row("test_mfma_path_at_medium_size_against_oracle_and_generic_kernels[128px_16-32-64-72]",
                         unet_layer_spec(*MEDIUM_CASES["128px_16-32-64-72"][:4]), *MEDIUM_CASES["128px_16-32-64-72"][4:6],
                         {(3, True), (3, False)},
                         claims={("enc", "down", "thin"), ("enc", "down", "patch"), ("enc", "down", "mfma")}),
    "deep_5lvl": _row("test_deep_unets_against_oracle_and_generic_kernels[5lvl_256px_16-256]",
                      unet_layer_spec(*DEEP_CASES["5lvl_256px_16-256"][:4]), *DEEP_CASES["5lvl_256px_16-256"][4:6],
                      {(4, True), (4, False)},
                      claims={("enc", "up", "mfma"), ("enc", "up", "patch"), ("dec", "up", "thin"), ("enc", "wgrad", "patch")}),
    "deep_6lvl": _row("test_deep_unets_against_oracle_and_generic_kernels[6lvl_64px_1x1]",
                      unet_layer_spec(*DEEP_CASES["6lvl_64px_1x1"][:4]), *DEEP_CASES["6lvl_64px_1x1"][4:6],
                      {(6, True), (6, False)},
                      claims={("enc", "up", "mfma"), ("enc", "wgrad", "mfma_atomic"), ("enc", "wgrad", "generic")}),
    "deep_512px": _row("test_deep_unets_against_oracle_and_generic_kernels[512px_8-8-16-16-32]",
                       unet_layer_spec(*DEEP_CASES["512px_8-8-16-16-32"][:4]), *DEEP_CASES["512px_8-8-16-16-32"][4:6],
                       {(3, True), (3, False)},
                       claims={("enc", "down", "mfma"), ("dec", "up", "up_thin"), ("enc", "up", "mfma")}),
    "deep_20x28": _row("test_deep_unets_against_oracle_and_generic_kernels[20x28_34ch]",
                       unet_layer_spec(*DEEP_CASES["20x28_34ch"][:4]), *DEEP_CASES["20x28_34ch"][4:6],
                       {(5, True), (5, False)},
                       claims={("fc", "fwd", "tile"), ("fc", "bwd", "tile"), ("enc", "up", "generic"), ("dec", "up", "generic")}),
    "cfg3_b5": _row("test_benchmark_geometry_full_size_against_oracle", CFG3, 128, 32, {(5, True), (5, False)}, modes=(True,),
                    claims={("enc", "down", "patch"), ("enc", "wgrad", "patch"), ("dec", "up", "patch"), ("enc", "down", "thin"),
                            ("enc", "wgrad", "thin"), ("dec", "up", "thin"), ("fc", "fwd", "lin_big"), ("fc", "bwd", "lin_big")}),
    "cfg3_b32": _row("test_benchmark_geometry_at_the_stated_batch", CFG3, 128, 32, {(32, True), (32, False)}, modes=(True,),
                     claims={("enc", "down", "patch"), ("fc", "bwd", "lin_big")}),
    "cfg3_b32_small": _row("test_benchmark_geometry_at_the_stated_batch", CFG3, 128, 32, {(5, False)}, modes=(True,)),
    "96x160": _row("test_mfma_path_non_square_odd_channel_counts", unet_layer_spec(2, 5, (96, 160), [16, 40, 72]), 20, 7,
                   {(3, True), (3, False)}, modes=(True,),
                   claims={("enc", "down", "mfma"), ("dec", "up", "mfma"), ("enc", "wgrad", "mfma")}),
}


def _row_reached(row):
    out = set()
    for specialised in row["modes"]:
        for (batch, train) in row["batches"]:
            out |= _reached(_plan(row["spec"], row["fc"], row["latent"], batch, train, specialised,
                                  max_batch=max(b for b, _ in row["batches"])))
    return out


@pytest.mark.parametrize("row", [r for r in GPU_ROWS if GPU_ROWS[r]["claims"]])
def test_gpu_tests_reach_the_families_they_name(row):
    r = GPU_ROWS[row]
    missing = r["claims"] - _row_reached(r)
    assert not missing, f"{r['test']} no longer reaches {sorted(missing)}"


def test_gpu_tests_reach_every_branch():
    reached = set()
    for r in GPU_ROWS.values():
        reached |= _row_reached(r)
    got = {(op, f) for (_, op, f) in reached}
    unreachable = {(op, f) for (_, op, f) in UNREACHABLE}
    assert not got - BRANCHES, f"families this test does not know: {sorted(got - BRANCHES)}"
    left = BRANCHES - got - unreachable
    assert not left, f"no GPU test reaches {sorted(left)}"


def _sweep_specs(count, seed=5):
    rng = random.Random(seed)
    for _ in range(count):
        n = rng.randint(1, 7)
        scale = 2 ** n
        (h, w) = (scale * rng.choice([1, 2, 3, 4, 5, 8]), scale * rng.choice([1, 2, 3, 4, 5, 8]))
        while h * w > 512 * 512:
            (h, w) = (h // 2 // scale * scale or scale, w)
        chans = [rng.choice([8, 12, 16, 24, 32, 40, 64, 72]) for _ in range(n)]
        if n == 1:
            chans = [rng.choice([2, 4, 8, 16])]
        yield unet_layer_spec(rng.randint(1, 4), rng.randint(1, 4), (h, w), chans), rng.choice([2, 3, 4, 5, 8, 16])


def test_unreachable_branches_are_not_reached_by_any_spec():
    seen = set()
    for (spec, max_batch) in _sweep_specs(150):
        for (batch, train) in itertools.product(sorted({max_batch, max(1, max_batch // 2), 1}), (True, False)):
            if train and batch == 1:
                continue
            got = _reached(_plan(spec, 16, 4, batch, train, max_batch=max_batch))
            bad = got & set(UNREACHABLE)
            assert not bad, (bad, spec.save(), batch)
            seen |= got
    assert len({(op, f) for (_, op, f) in seen}) >= 15     # (the sweep is not vacuous)
