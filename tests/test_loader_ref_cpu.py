"""loader_ref.py held to the reference-generated golden files, and its seeded inputs held to telling the loader's promised
arithmetic from its neighbours.  No GPU: everything here is a statement about the numpy reference that
test_loader_kernels_gpu.py compares the kernels with, and about the inputs it feeds them."""
import json
import os

import numpy as np
import pytest

import loader_ref as ref
from cae_tools_amd.models.model_metric import metrics_from_sums

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DS = np.load(os.path.join(GOLDEN, "ds_dataset.npz"), allow_pickle=False)
META = json.load(open(os.path.join(GOLDEN, "ds_dataset.json")))
MM = np.load(os.path.join(GOLDEN, "model_metric.npz"))


def _bits(x):
    return np.ascontiguousarray(x).tobytes()


# ---- the golden data set, bit for bit --------------------------------------------------------------

def test_scan_gives_the_golden_normalisation_parameters():
    (mins, maxs, omin, omax) = META["normalisation_parameters"]
    for name in META["input_names"]:
        assert ref.scan(DS[name]) == (0, mins[name], maxs[name])
    assert ref.scan(DS["hires"]) == (0, omin, omax)
    bad = DS["lowres"].copy()
    bad[0, 0, 0, 0] = bad[3, 0, 1, 1] = np.nan
    assert ref.scan(bad) == (2, float(np.nanmin(bad)), float(np.nanmax(bad)))


def test_normalise_and_pack_give_the_golden_inputs_and_outputs():
    (mins, maxs, omin, omax) = META["normalisation_parameters"]
    names = META["input_names"]
    norm = np.full(DS["norm_in"].shape, -7.0, dtype=np.float32)
    raw = np.full(DS["norm_in"].shape, -7.0, dtype=np.float32)
    off = 0
    for name in names:
        norm = ref.pack(norm, ref.normalise(DS[name], mins[name], maxs[name]), off)
        raw = ref.pack(raw, ref.normalise(DS[name], mins[name], maxs[name], enable=False), off)
        off += DS[name].shape[1]
    assert off == norm.shape[1]
    assert norm.dtype == DS["norm_in"].dtype and _bits(norm) == _bits(DS["norm_in"])
    # the constant variable: a range of 0 normalises to 0 (the last two channels)
    assert mins["const"] == maxs["const"] and not norm[:, -2:].any()
    assert _bits(raw[2]) == _bits(DS["raw_in2"])
    out = ref.normalise(DS["hires"], omin, omax)
    assert out.dtype == DS["norm_out"].dtype and _bits(out) == _bits(DS["norm_out"])


def test_pack_with_a_row_table_is_the_golden_samples_in_that_order():
    (mins, maxs, _, _) = META["normalisation_parameters"]
    n = DS["lowres"].shape[0]
    order = np.random.default_rng(4).permutation(n)
    rows = np.argsort(order)
    got = ref.pack(np.zeros((n, 1) + DS["lowres"].shape[2:], dtype=np.float32),
                   ref.normalise(DS["lowres"], mins["lowres"], maxs["lowres"]), 0, rows)
    assert _bits(got) == _bits(DS["norm_in"][order, :1])


def test_denormalise_gives_the_golden_denormalisation():
    """denorm_in -> denorm_out is the reference DSDataset's own denormalise_output on an fp64 array (make_golden.py)"""
    (_, _, omin, omax) = META["normalisation_parameters"]
    assert DS["denorm_in"].dtype == np.float64
    got = ref.denormalise(DS["denorm_in"], omin, omax)
    assert got.dtype == np.float64 and _bits(got) == _bits(DS["denorm_out"])
    y32 = DS["denorm_in"].astype(np.float32)
    assert _bits(ref.denormalise(y32, omin, omax)) == _bits(omin + (y32.astype(np.float64) * (omax - omin)))


@pytest.mark.parametrize("tag", ["masked", "all"])
def test_exact_metric_sums_give_the_golden_metrics(tag):
    mask = MM["mask"] if tag == "masked" else None
    (sums, mags) = ref.metric_sums_exact(MM["y"], MM["truth"], mask, float(MM["vmin"]), float(MM["vmax"]))
    keep = (MM["mask"] != 0) if tag == "masked" else np.ones(MM["mask"].shape, dtype=bool)
    assert np.array_equal(sums[:, 0], keep.reshape(keep.shape[0], -1).sum(axis=1))
    assert (mags >= np.abs(sums)).all()
    got = metrics_from_sums(sums)
    for k in ("mse", "rmse", "mae", "mean_pearson_correlation"):
        assert got[k] == pytest.approx(float(MM[f"{tag}/{k}"]), rel=1e-11, abs=0)


def test_metric_terms_follow_the_mask_and_its_broadcast():
    rng = np.random.default_rng(8)
    y = rng.random((2, 3, 4, 5), dtype=np.float32)
    a = (288.0 + 10.0 * rng.random((2, 3, 4, 5))).astype(np.float32)
    m = np.array([0.0, 0.5, -1.0, 2.0, 0.0])[rng.integers(0, 5, (2, 1, 4, 5))]
    (terms, keep, e) = ref.metric_terms(y, a, m, 288.0, 298.0)
    assert terms.shape == (8, 2, 3, 4, 5) and keep.shape == y.shape
    assert np.array_equal(keep, np.broadcast_to(m != 0, y.shape))
    assert _bits(e) == _bits(ref.denormalise(y, 288.0, 298.0))
    assert _bits(terms[7]) == _bits((a.astype(np.float64) - e) ** 2)
    (sums, _) = ref.metric_sums_exact(y, a, np.zeros((2, 1, 4, 5)), 288.0, 298.0)
    assert not sums.any()


# ---- the inputs tell the promised arithmetic from its neighbours ---------------------------------------

def _share(a, b):
    return float(np.mean(a.view(np.uint32) != b.view(np.uint32)))


def test_wide_variable_separates_fp32_steps_from_fp64_once_and_from_the_reciprocal():
    v = ref.wide_variable(100000)
    (lo, hi) = ref.bounds_of(v)
    want = ref.normalise(v, lo, hi)
    assert want.min() == 0.0 and want.max() == 1.0
    once = _share(want, ref.normalise_fp64_once(v, lo, hi))
    recip = _share(want, ref.normalise_reciprocal(v, lo, hi))
    print(f"wide: fp64-once differs on {once:.1%}, reciprocal on {recip:.1%}")
    assert once >= 0.10
    assert recip >= 0.05


def test_narrow_variable_separates_division_from_the_reciprocal():
    v = ref.narrow_variable(100000)
    (lo, hi) = ref.bounds_of(v)
    want = ref.normalise(v, lo, hi)
    recip = _share(want, ref.normalise_reciprocal(v, lo, hi))
    print(f"narrow: reciprocal differs on {recip:.1%}, fp64-once on {_share(want, ref.normalise_fp64_once(v, lo, hi)):.1%}")
    assert recip >= 0.05


def test_arbitrary_fp64_parameters_separate_two_roundings_from_fma():
    y = ref.unit_scores(3000)
    (lo, hi) = ref.ARBITRARY_F64
    two = ref.denormalise(y, lo, hi)
    one = ref.denormalise_fma(y, lo, hi)
    differ = int((two != one).sum())
    print(f"arbitrary fp64 parameters: fma differs on {differ} of {y.size}")
    assert differ >= 20
    assert np.abs(two - one).max() <= np.spacing(hi)        # and by one unit in the last place at the most
    # the same e enters the metric sums
    a = (lo + (hi - lo) * ref.unit_scores(3000, seed=7)).astype(np.float32)
    (_, _, e) = ref.metric_terms(y, a, None, lo, hi)
    assert _bits(e) == _bits(two) and int((e != one).sum()) >= 20
    picked = ref.fma_sensitive_scores(lo, hi)
    assert picked.size == differ
    assert (ref.denormalise(picked, lo, hi) != ref.denormalise_fma(picked, lo, hi)).all()


def test_fp32_valued_parameters_cannot_separate_them():
    """vmin and vmax that are fp32 values leave y * (vmax - vmin) exact in fp64, so a contracted fma gives the same bits:
    why the kernels' two rounded operations need ARBITRARY_F64 to be seen"""
    y = ref.unit_scores(3000)
    for (lo, hi) in (ref.FP32_VALUED, ref.bounds_of(ref.narrow_variable(1000))):
        assert float(np.float32(lo)) == lo and float(np.float32(hi)) == hi
        assert _bits(ref.denormalise(y, lo, hi)) == _bits(ref.denormalise_fma(y, lo, hi))
