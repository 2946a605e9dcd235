"""What the UNET launch code switches on BELOW the kernel family - template arguments, K-slice regimes, tiles per workgroup, the
LDS size of k_lin_outer - read from the sub-family fields of unet_debug_plan (UnetPlan.kernel_plan), which come from the
functions the launches call.  Without a GPU:
- the geometries of tests/test_unet_shapes_gpu.py (unet_helpers.SHAPE_CASES) run the instantiations and splits they are aimed at;
- together with the rows of tests/test_unet_plan_cpu.py they reach every cell of SHAPE_BRANCHES but the ones in UNREACHABLE,
  each with the reason in the choosers' arithmetic, which a sweep of specs confirms."""
import itertools
import random

import pytest

from test_unet_plan_cpu import GPU_ROWS, _sweep_specs
from unet_helpers import SHAPE_CASES, plan_cells

from cae_tools_amd.models.unet import unet_layer_spec
from cae_tools_amd.unet_engine import UnetPlan

TILES = ("32x512", "64x256", "128x128")
SLICES = ("1", "2", ">2")               # one K slice / two (commuting atomics on a zeroed map) / more (partial maps and a fold)
LIN_K = ("one", "whole", "partial")     # one K slice / several with a whole last tile / several with a partly filled last tile

# every cell the launch code can switch to (unet_helpers.plan_cells names them)
SHAPE_BRANCHES = \
    {("down", "thin", f"rbn{r}", f"cl{c}") for r in (1, 2) for c in (1, 2, 3, 4)} | \
    {("down", "patch", f"rbn{r}", s) for r in (2, 4) for s in SLICES} | \
    {("down", "mfma", t, s) for t in TILES for s in SLICES} | \
    {("up", f, f"cl{c}") for f in ("thin", "up_thin") for c in (1, 2, 3, 4)} | \
    {("up", "patch", f"rbn{r}") for r in (1, 2)} | \
    {("up", "mfma", t) for t in TILES} | \
    {("wgrad", "thin", f"rbn{r}") for r in (1, 2)} | \
    {("wgrad", "patch", w) for w in ("2x2", "4x1")} | \
    {("wgrad", "mfma", t, how) for t in TILES + ("1wave",) for how in ("partial_tiles", "atomics")} | \
    {(op, "lin_big", f"rb{r}", k) for op in ("fwd", "bwd") for r in (1, 2) for k in LIN_K} | \
    {("bwd", "lin_outer", lds) for lds in ("lds<=64K", "lds>64K")} | \
    {(op, f) for op in ("fwd", "bwd") for f in ("tile", "gemm16")}

# cells no valid UNET reaches, each with the reason in the choosers' arithmetic
UNREACHABLE = {
    ("down", "patch", "rbn4", ">2"): "pdown_slices takes RBN 4 only where B * tiles > 256, which puts the tile count B * tiles * "
                                     "ceil(Cs / 128) at 257 or more; a third slice needs tiles * 2 < 384",
    ("wgrad", "mfma", "1wave", "partial_tiles"): "mfma_wgrad_part_bytes is 0 for the single-wave path (<= 8 channels on the big "
                                                 "side), and choose_wgrad takes 0 bytes of partial tiles for 'atomics'",
}


def _cells(spec, fc, latent, batches, max_batch, modes=(True,), trains=(True, False)):
    """{cell: (batch, train)} over the plans of one engine"""
    out = {}
    p = UnetPlan(spec, fc, latent, max_batch)
    try:
        for specialised in modes:
            p.set_kernel_mode(specialised)
            for (b, train) in itertools.product(batches, trains):
                for c in plan_cells(p.kernel_plan(b, train)):
                    out.setdefault(c, (b, train))
    finally:
        p.close()
    return out


def _case_plan(name, batch, train=True):
    (in_c, out_c, size, chans, fc, latent, _, max_batch) = SHAPE_CASES[name]
    p = UnetPlan(unet_layer_spec(in_c, out_c, size, chans), fc, latent, max_batch)
    try:
        return p.kernel_plan(batch, train)
    finally:
        p.close()


def _sub(fields, keys):
    return {k: fields.get(k) for k in keys}


# (case, batch) -> {layer: {field: value}}: what each GPU case is aimed at, as the launch code's own functions answer it
PINS = {
    ("lin_k1296", 33): {   # flat 1296 = 10 * 128 + 16; RB 2 with one row in the second block
        "fc0": {"fwd": "lin_big", "fwd.rb": "2", "fwd.slices": "11", "fwd.partial": "1", "bwd.slices": "1", "outer_lds": "43520"},
        "fc3": {"fwd": "lin_big", "fwd.slices": "1", "fwd.ntiles": "11", "fwd.nlast": "16", "bwd.rb": "2", "bwd.slices": "11",
                "bwd.partial": "1"},
        "enc1": {"down": "mfma", "down.tile": "64x256", "down.nsplit": "1"}},
    ("lin_k1296", 40): {"fc0": {"fwd": "lin_big", "fwd.rb": "2", "outer_lds": "43520"}},
    ("lin_k1296", 57): {"fc0": {"fwd": "lin_big", "fwd.rb": "2", "outer_lds": "69632"}},   # B8 = 64: above 64 KiB
    ("lin_k1296", 64): {"fc0": {"fwd": "lin_big", "fwd.rb": "2", "outer_lds": "69632"}, "fc3": {"bwd": "lin_big", "bwd.slices": "11"}},
    ("lin_k1296", 65): {"fc0": {"fwd": "tile", "bwd": "tile", "fwd.tile": "32x512", "fwd.slices": "6"},
                        "fc3": {"fwd": "tile", "bwd": "tile", "fwd.tile": "128x128", "bwd.slices": "6"}},
    ("lin_fc132", 5): {
        "fc0": {"fwd": "lin_big", "fwd.rb": "1", "fwd.slices": "12", "fwd.partial": "0", "fwd.ntiles": "2", "fwd.nlast": "4",
                "bwd.slices": "2", "bwd.partial": "1"},
        "fc3": {"fwd": "lin_big", "fwd.slices": "2", "fwd.partial": "1", "bwd.slices": "12", "bwd.partial": "0"}},
    ("lin_fc132", 61): {"fc0": {"fwd": "lin_big", "fwd.rb": "2", "fwd.slices": "12", "bwd.rb": "2", "bwd.slices": "2", "outer_lds": "69632"}},
    ("lin_fc1028", 3): {
        "fc0": {"fwd": "lin_big", "fwd.rb": "1", "fwd.ntiles": "9", "fwd.nlast": "4", "bwd.slices": "9", "bwd.partial": "1"},
        "fc1": {"fwd": "lin_big", "fwd.slices": "9", "fwd.partial": "1", "fwd.ntiles": "1", "fwd.nlast": "4", "bwd.slices": "1"},
        "fc2": {"fwd": "lin_big", "fwd.slices": "1", "fwd.partial": "1", "bwd.slices": "9"},
        "fc3": {"fwd": "lin_big", "fwd.slices": "9", "bwd.slices": "12"}},
    ("lin_fc1028", 34): {f"fc{k}": {"fwd": "lin_big", "bwd": "lin_big", "fwd.rb": "2", "bwd.rb": "2"} for k in range(4)},
    ("thin_c2_c4", 3): {   # 3 tiles per image: one short group
        "enc0": {"down": "thin", "down.rbn": "1", "down.cl": "2", "down.tpw": "3", "down.groups": "1", "wgrad": "thin", "wgrad.tpw": "3"},
        "enc1": {"down": "mfma", "down.tile": "32x512", "down.nsplit": "4"},
        "dec1": {"down": "thin", "down.rbn": "2", "down.cl": "4", "up": "up_thin", "up.cl": "4", "wgrad.rbn": "2"}},
    ("thin_c4_short", 2): {   # 10 tiles per image: groups of 8 and 2
        "enc0": {"down": "thin", "down.rbn": "2", "down.cl": "4", "down.tpw": "8", "down.groups": "2", "wgrad": "thin",
                 "wgrad.tpw": "8", "wgrad.groups": "2"},
        "dec1": {"down": "mfma", "down.tile": "128x128", "down.nsplit": "1"}},
    ("wide_c1", 3): {
        "enc0": {"down": "thin", "down.rbn": "1", "down.cl": "1", "down.Ws": "128", "down.tpw": "4"},
        "dec1": {"down": "thin", "down.rbn": "2", "down.cl": "1", "up": "thin", "up.cl": "1", "up.waves": "6", "up.wgs": "2"}},
    ("wide_c2_c4", 3): {
        "enc0": {"down": "thin", "down.rbn": "1", "down.cl": "2", "down.Ws": "128"},
        "dec1": {"down": "thin", "down.rbn": "1", "down.cl": "4", "up": "thin", "up.cl": "4", "up.waves": "6", "up.wgs": "2"}},
    ("wide_c4_c2", 3): {
        "enc0": {"down": "thin", "down.rbn": "1", "down.cl": "4", "down.Ws": "128"},
        "dec1": {"down": "thin", "down.rbn": "2", "down.cl": "2", "up": "thin", "up.cl": "2", "up.waves": "6", "up.wgs": "2"}},
    ("wide_patch128", 3): {
        "enc0": {"down": "patch", "down.rbn": "2", "down.nsplit": "1", "down.Ws": "128"},
        "dec1": {"down": "patch", "down.nsplit": "2", "down.Ws": "128", "up": "patch", "up.rbn": "1", "up.Ws": "128"}},
    ("tall_rbn4", 33): {
        "enc1": {"down": "patch", "down.rbn": "4", "down.nsplit": "2", "down.Ws": "16", "up": "patch", "up.rbn": "2", "up.Ws": "16",
                 "wgrad": "patch", "wgrad.wrxwc": "2x2"},
        "dec0": {"down": "patch", "down.rbn": "4", "down.nsplit": "2", "up": "patch", "up.rbn": "2", "up.Ws": "16"},
        "fc0": {"fwd": "lin_big", "fwd.rb": "2", "fwd.slices": "768"}, "fc3": {"bwd.rb": "2", "bwd.slices": "768"}},
    ("mfma_cells", 3): {
        "enc0": {"down": "mfma", "down.tile": "32x512", "down.nsplit": "1"},
        "enc1": {"down": "mfma", "down.tile": "64x256", "down.nsplit": "1"},
        "enc2": {"down": "mfma", "down.tile": "32x512", "down.nsplit": "4"},
        "dec1": {"down": "mfma", "down.tile": "64x256", "down.nsplit": "4"},
        "dec2": {"down": "mfma", "down.tile": "128x128", "down.nsplit": "1"}},
    # one batch below max_batch: 4096 (2048) chunks in 8-chunk slices are 512 (256) slices, the 4160 (2112) chunks of
    # max_batch in 9-chunk slices 463 (235), and the partial-tile buffer is sized for max_batch
    ("wgrad_atomics_32", 64): {"enc0": {"wgrad": "mfma_atomic", "wgrad.tile": "32x512", "wgrad.slices": "512", "wgrad.per": "8"}},
    ("wgrad_atomics_64", 64): {"dec1": {"wgrad": "mfma_atomic", "wgrad.tile": "64x256", "wgrad.slices": "512", "wgrad.per": "8"}},
    ("wgrad_atomics_128", 32): {"enc0": {"wgrad": "mfma_atomic", "wgrad.tile": "128x128", "wgrad.slices": "256", "wgrad.per": "8"}},
}


def check_pins(name, batch, plan=None):
    """the pinned plan fields of one GPU case at one batch (tests/test_unet_shapes_gpu.py asserts them before it runs)"""
    plan = plan or _case_plan(name, batch)
    for layer, want in PINS[(name, batch)].items():
        got = _sub(plan[layer], want)
        assert got == want, f"{name} B={batch} {layer}: the launch code answers {got}, the case is aimed at {want}"


def test_every_case_and_batch_is_pinned():
    assert set(PINS) == {(n, b) for n, c in SHAPE_CASES.items() for b in c[6]}


@pytest.mark.parametrize("name,batch", sorted(PINS), ids=[f"{n}-B{b}" for n, b in sorted(PINS)])
def test_gpu_cases_run_what_they_are_aimed_at(name, batch):
    check_pins(name, batch)


def test_sub_family_fields_come_with_every_family():
    """every layer line carries the fields of its family (plan_cells reads them all: a missing one is a KeyError)"""
    for name, c in SHAPE_CASES.items():
        for b in c[6]:
            for train in (True, False):
                assert plan_cells(_case_plan(name, b, train))


def _case_cells():
    out = {}
    for name, (in_c, out_c, size, chans, fc, latent, batches, max_batch) in SHAPE_CASES.items():
        for c, (b, train) in _cells(unet_layer_spec(in_c, out_c, size, chans), fc, latent, batches, max_batch).items():
            if train:   # (the GPU module runs training steps and score(); an eval plan's cells are a subset)
                out.setdefault(c, f"{name} B={b}")
    return out


def _row_cells():
    out = {}
    for name, r in GPU_ROWS.items():
        max_batch = max(b for b, _ in r["batches"])
        p = UnetPlan(r["spec"], r["fc"], r["latent"], max_batch)
        try:
            for specialised in r["modes"]:
                p.set_kernel_mode(specialised)
                for (b, train) in r["batches"]:
                    for c in plan_cells(p.kernel_plan(b, train)):
                        out.setdefault(c, name)
        finally:
            p.close()
    return out


def test_gpu_tests_reach_every_cell():
    reached = {**_row_cells(), **_case_cells()}
    assert not set(reached) - SHAPE_BRANCHES, f"cells this test does not know: {sorted(set(reached) - SHAPE_BRANCHES)}"
    assert not set(reached) & set(UNREACHABLE), f"reached, yet listed as unreachable: {sorted(set(reached) & set(UNREACHABLE))}"
    left = SHAPE_BRANCHES - set(reached) - set(UNREACHABLE)
    assert not left, f"no GPU test reaches {sorted(left)}"


def test_every_case_adds_a_cell():
    """no case of SHAPE_CASES is idle: each reaches a cell that the rows of test_unet_plan_cpu.py do not"""
    old = set(_row_cells())
    for name, (in_c, out_c, size, chans, fc, latent, batches, max_batch) in SHAPE_CASES.items():
        own = set(_cells(unet_layer_spec(in_c, out_c, size, chans), fc, latent, batches, max_batch, trains=(True,)))
        assert own - old, name


def _wide_sweep(count, seed=17):
    """the sweep of test_unet_plan_cpu.py, then specs with 1-8 and 32 image channels, non-square sizes and batches up to 96"""
    for (spec, max_batch) in _sweep_specs(60):
        yield spec, 16, 4, max_batch
    rng = random.Random(seed)
    for _ in range(count):
        n = rng.randint(1, 5)
        scale = 2 ** n
        (h, w) = (scale * rng.choice([1, 2, 3, 4, 5, 8, 16]), scale * rng.choice([1, 2, 3, 4, 5, 8, 16]))
        while h * w > 256 * 256:
            (h, w) = (max(h // 2 // scale * scale, scale), w) if h >= w else (h, max(w // 2 // scale * scale, scale))
        chans = [rng.choice([8, 12, 16, 24, 32, 40, 64, 72, 96, 128, 136]) for _ in range(n)]
        chan_io = [1, 2, 3, 4, 5, 6, 7, 8, 32]
        yield (unet_layer_spec(rng.choice(chan_io), rng.choice(chan_io), (h, w), chans), rng.choice([8, 12, 132, 1028]), rng.choice([4, 8]),
               rng.choice([2, 3, 5, 8, 16, 31, 32, 33, 48, 56, 57, 64, 65, 96]))


def test_unreachable_cells_are_not_reached_by_any_spec():
    seen = set()
    for (spec, fc, latent, max_batch) in _wide_sweep(240):
        batches = sorted({max_batch, max_batch - 1, max(2, max_batch // 2), 2} - {0, 1})
        got = set(_cells(spec, fc, latent, batches, max_batch))
        assert not got - SHAPE_BRANCHES, (got - SHAPE_BRANCHES, spec.save())
        bad = got & set(UNREACHABLE)
        assert not bad, (bad, spec.save(), max_batch)
        seen |= got
    assert len(seen) >= 50, len(seen)     # (the sweep is not vacuous)
