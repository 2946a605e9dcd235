"""What the Linear engine launches, read from the code its launch runs (lin_debug_plan in include/cae_linear.h,
LinearPlan.kernel_plan), without a GPU:
- over a sweep of nin x nout x batch, the forward's K split covers K with no empty slice, splits exactly when the rule of
  gemm_slices says so (>= 64 chunks of 16 and fewer than 256 tiles), writes slices * nout * batch floats of partial tiles, and
  the room the workspace holds for them (reported as `room gpart_bytes`) fits every batch up to max_batch;
- the plans of the GPU cases (tests/linear_shapes.py) are the pinned literals, and together they reach every tile shape, more
  than two slices, a ragged last slice, a 1-element last chunk, the split threshold from both sides, and a second column and
  row tile.  The `tiles >= 256` no-split branch at nin >= 1009 needs nout >= 32768 (0.7 GB of state): it is covered here only."""
import ctypes as C

import pytest

from linear_shapes import CASES, PLANS, SPLIT_CASES

from cae_tools_amd._lib import CaeError, check
from cae_tools_amd.linear_engine import LinearPlan

NIN = (1, 3, 60, 1008, 1009, 1083, 1089, 4096)
NOUT = (1, 30, 32, 33, 56, 64, 65, 143, 385, 40000)
BATCHES = (1, 3, 128, 129, 257, 520)
KC = 16   # IG_KC: the K chunk of the tile engine


def _tile(nout):
    """(name, rows, columns) of the tile igemm_tile picks for this many rows"""
    return ("32x512", 32, 512) if nout <= 32 else ("64x256", 64, 256) if nout <= 64 else ("128x128", 128, 128)


def _ceil(a, b):
    return (a + b - 1) // b


@pytest.mark.parametrize("nout", NOUT)
@pytest.mark.parametrize("nin", NIN)
def test_forward_k_split_over_the_sweep(nin, nout):
    p = LinearPlan((1, 1, nin), (1, 1, nout), max(BATCHES))
    try:
        chunks = _ceil(nin, KC)
        (name, tn, tm) = _tile(nout)
        seen_split = False
        for batch in BATCHES:
            for train in (True, False):
                plan = p.kernel_plan(batch, train)
                f = plan["fwd"]
                (slices, per, part) = (int(f["slices"]), int(f["per"]), int(f["part_bytes"]))
                (ct, rt) = (_ceil(batch, tm), _ceil(nout, tn))
                what = f"{nin} -> {nout}, batch {batch}: {f}"
                assert f["tile"] == name and f["grid"] == f"{ct}x{rt}", what
                assert slices >= 1 and slices * per >= chunks, what
                assert (slices - 1) * per < chunks, what            # no empty slice
                assert (slices == 1) == (chunks < 64 or ct * rt >= 256), what
                assert part == (slices * nout * batch * 4 if slices > 1 else 0), what
                seen_split |= slices > 1
                if train:   # rows nout, columns nin, K = batch in one slice, straight into the fp64 accumulator
                    assert plan["wgrad"] == {"tile": name, "grid": f"{_ceil(nin, tm)}x{rt}", "slices": "1"}, what
                else:
                    assert plan["wgrad"] == {}, what
        room = int(p.kernel_plan(1, False)["room"]["gpart_bytes"])
        # every batch the engine accepts, not just the swept ones
        most = max(int(p.kernel_plan(b, False)["fwd"]["part_bytes"]) for b in range(1, p.max_batch + 1))
        assert most <= room, f"{nin} -> {nout}: partial tiles of {most} bytes, room for {room}"
        assert seen_split == (room > 0)
        assert p.workspace_bytes >= room + 4 * p.max_batch * (nin + 2 * nout) + 8 * (nin * nout + nout)
    finally:
        p.close()


def test_the_sweep_reaches_both_no_split_reasons():
    """few chunks (nin <= 1008) and many tiles (40000 rows = 313 row tiles) - the second one no GPU test runs"""
    p = LinearPlan((1, 1, 4096), (1, 1, 40000), 4)
    assert p.kernel_plan(4, True)["fwd"] == {"tile": "128x128", "grid": "1x313", "slices": "1", "per": "256", "part_bytes": "0"}
    p.close()
    p = LinearPlan((1, 1, 4096), (1, 1, 385), 4)
    assert p.kernel_plan(4, True)["fwd"] == {"tile": "128x128", "grid": "1x4", "slices": "16", "per": "16", "part_bytes": "98560"}
    p.close()


@pytest.mark.parametrize("key", list(PLANS), ids=[f"{n}-b{b}" for (n, b) in PLANS])
def test_gpu_case_plans_are_the_pinned_ones(key):
    (name, batch) = key
    (in_shape, out_shape, batches) = CASES[name]
    assert batch in batches
    p = LinearPlan(in_shape, out_shape, max(batches))
    try:
        assert p.kernel_plan(batch, True) == PLANS[key]
        assert p.kernel_plan(batch, False) == {**PLANS[key], "wgrad": {}}
    finally:
        p.close()


def test_gpu_cases_reach_every_branch_between_them():
    assert set(PLANS) == {(n, b) for n, (_, _, bs) in CASES.items() for b in bs}
    fwd = {k: v["fwd"] for k, v in PLANS.items()}
    nin = {n: CASES[n][0][0] * CASES[n][0][1] * CASES[n][0][2] for n in CASES}
    assert {f["tile"] for f in fwd.values()} == {"32x512", "64x256", "128x128"}
    # every tile shape with a split K, and with a second column tile
    assert {f["tile"] for f in fwd.values() if int(f["slices"]) > 2} == {"32x512", "64x256", "128x128"}
    assert {f["tile"] for f in fwd.values() if int(f["grid"].split("x")[0]) > 1} == {"32x512", "64x256", "128x128"}
    assert any(int(f["grid"].split("x")[1]) > 1 and int(f["slices"]) > 1 for f in fwd.values())      # a second row tile, split
    ragged = [(n, b) for (n, b), f in fwd.items() if int(f["slices"]) > 1 and _ceil(nin[n], KC) % int(f["per"])]
    assert ragged, "no case whose last K slice is shorter than the others"
    assert any(nin[n] % KC == 1 for (n, b), f in fwd.items() if int(f["slices"]) > 1), "no split case with a 1-element last chunk"
    assert any(nin[n] % 4 == 3 for (n, b), f in fwd.items() if int(f["slices"]) > 1), "no split case with K = 3 mod 4"
    assert (nin["edge_1008"], fwd[("edge_1008", 4)]["slices"]) == (1008, "1")
    assert (nin["edge_1009"], fwd[("edge_1009", 4)]["slices"]) == (1009, "4")
    assert {n for (n, b), f in fwd.items() if int(f["slices"]) > 1} == set(SPLIT_CASES)
    assert {nin["tiny_k1"], nin["tiny_k3"]} == {1, 3}


def test_plan_arguments():
    p = LinearPlan((1, 2, 3), (1, 1, 5), 4)
    assert (p.nin, p.nout, p.n_param) == (6, 5, 35)
    with pytest.raises(CaeError, match="outside 1 .. 4"):
        p.kernel_plan(5, True)
    with pytest.raises(CaeError, match="outside 1 .. 4"):
        p.kernel_plan(0, False)
    with pytest.raises(CaeError, match="needs"):
        check(p.lib.lin_debug_plan(p.handle, 4, 1, C.create_string_buffer(16), 16))
    p.close()
