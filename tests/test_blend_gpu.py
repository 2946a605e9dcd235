"""cae_case_error_moments and cae_blend_predictions on the GPU.  The per-case rows of moments against the numpy restatement of
the definition (blend_ref.py, np.longdouble): n exactly, every floating-point sum of m terms within (m + 4) 2^-53 S|t| - for a
plane of a partial second tile (1 x 67) and one of 77 tiles (70 x 70: a lane of the fold takes a second tile), 1 to 8
candidates, every element kind and a mixed list, NaN and inf in target and candidates, a case without a pair; the columns n,
S e_m and S e_m^2 bit for bit against cae_case_compare; the same bits for the cases cut 2 + 3 and on a second run; one call
with more work items than the grid cap covers.  The blended field against the numpy loop with assert_array_equal.  Then blend
fit and blend apply through the command's main on 12 synthetic cases: the blend's mse as cae_case_compare measures it is no
larger than any candidate's and agrees with the record's quadratic form within the bound blend_ref derives.

Largest |got - want| / bound measured on an MI355X (each check prints its figure before it asserts): 0.032 at plane 1 x 67
(M = 3), 3.8e-4 at 70 x 70, 0.026 with mixed kinds, 0 with fp32 operands and on the 131 115 cases past the grid cap, 4.5e-3 on
the end-to-end file; end to end (convex) |measured mse - the record's| = 2.2e-16 against a bound of 2.3e-13, ratio 9.7e-4."""
import io
import json
import math
import os
import re
from contextlib import redirect_stdout
from functools import lru_cache

import numpy as np
import pytest

import blend_ref
from cae_tools_amd.case_ops import (blend_predictions, case_compare, case_error_moments, device_operand, moments_width, operand_cases)

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cae_tools_amd", "csrc")
KINDS = {"f32": np.dtype("<f4"), "f64": np.dtype("<f8"), "f32be": np.dtype(">f4"), "f64be": np.dtype(">f8")}
PLANES = [(1, 67), (70, 70)]
(N, C) = (5, 3)


def _cap(name):
    with open(os.path.join(CSRC, "host_blend.h")) as f:
        return int(re.search(r"constexpr int64_t " + name + r" = (\d+);", f.read()).group(1))


@lru_cache(maxsize=None)
def _fields(h, w, m, gaps=True):
    """(the target (N, h w), m predictions likewise) in float64: the predictions the target plus a shared and an own part;
    with gaps NaN and inf scattered in the target and in two candidates, and case 3 without a pair"""
    rng = np.random.default_rng(1000 * h + 10 * w + m)
    plane = h * w
    a = rng.normal(290.0, 5.0, (N, plane))
    shared = rng.normal(0.0, 1.0, (N, plane))
    preds = [a + shared + rng.normal(0.1 * k, 0.5 + 0.3 * k, (N, plane)) for k in range(m)]
    if gaps:
        for (x, bad) in ((a, [math.nan, math.inf, -math.inf]), (preds[0], [math.nan, -math.inf]), (preds[m - 1], [math.inf, math.nan])):
            where = rng.random(x.shape) < 0.04
            x[where] = rng.choice(bad, int(where.sum()))
        a[3] = math.nan
    for x in [a] + preds:
        x.setflags(write=False)
    return a, tuple(preds)


def _operand(x, h, w, dtype=np.float64, fill=7.5):
    """(N, plane) as an (N, C, h, w) array of dtype whose channel 0 holds x"""
    out = np.full((x.shape[0], C, h, w), fill, dtype=dtype)
    out[:, 0] = x.reshape(x.shape[0], h, w)
    return out


@lru_cache(maxsize=None)
def _reference(h, w, m, kind="f64"):
    """the reference of the fields as the kernel reads them in `kind`: computed once, shared, never changed"""
    (a, preds) = _fields(h, w, m)
    cast = lambda x: x.astype(KINDS[kind]).astype(np.float64)      # noqa: E731
    return blend_ref.Reference([cast(p) for p in preds], cast(a))


# ---- cae_case_error_moments ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("plane", PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_moments_against_the_reference_and_case_compare(plane, m):
    (h, w) = plane
    (a, preds) = _fields(h, w, m)
    ops = [device_operand(_operand(p, h, w)) for p in preds]
    t = device_operand(_operand(a, h, w))
    got = case_error_moments(ops, t)
    assert got.shape == (N, moments_width(m)) == (N, blend_ref.width(m))
    ref = _reference(h, w, m)
    ref.check(got, f"plane {h} x {w}, M {m}")
    assert (got[3] == 0.0).all() and not np.signbit(got[3]).any() and 0 < got[0, 0] < h * w
    # n, S e_m and S e_m^2 are cae_case_compare's bits
    (mine, theirs) = blend_ref.compare_columns(m)
    assert np.array_equal(got[:, mine], case_compare(ops, t)[:, theirs])
    # a second run, and the cases cut 2 + 3
    assert case_error_moments(ops, t).tobytes() == got.tobytes()
    cut = [case_error_moments([operand_cases(op, c0, c1) for op in ops], operand_cases(t, c0, c1)) for (c0, c1) in ((0, 2), (2, 5))]
    assert np.concatenate(cut).tobytes() == got.tobytes()


@pytest.mark.parametrize("kind", ["f32", "f64", "f32be", "f64be", "mixed"])
@pytest.mark.parametrize("plane", PLANES, ids=lambda p: f"{p[0]}x{p[1]}")
def test_moments_of_every_element_kind(plane, kind):
    """predictions and target in one kind, and a mixed list (f32, f64 big-endian, f64 against an f32 big-endian target) that
    the wrapper converts to fp64 on the device"""
    (h, w) = plane
    m = 3
    (a, preds) = _fields(h, w, m)
    kinds = ["f32", "f64be", "f64", "f32be"] if kind == "mixed" else [kind] * 4
    ops = [device_operand(_operand(p, h, w, KINDS[k])) for (p, k) in zip(preds, kinds)]
    t = device_operand(_operand(a, h, w, KINDS[kinds[3]]))
    got = case_error_moments(ops, t)
    cast = lambda x, k: x.astype(KINDS[k]).astype(np.float64)      # noqa: E731
    ref = _reference(h, w, m, kind) if kind != "mixed" else blend_ref.Reference([cast(p, k) for (p, k) in zip(preds, kinds)], cast(a, kinds[3]))
    ref.check(got, f"plane {h} x {w}, {kind}")
    (mine, theirs) = blend_ref.compare_columns(m)
    assert np.array_equal(got[:, mine], case_compare(ops, t)[:, theirs])
    if kind.endswith("be"):         # the byte order changes no bit
        native = [device_operand(_operand(p, h, w, KINDS[kind[:3]])) for p in preds]
        assert case_error_moments(native, device_operand(_operand(a, h, w, KINDS[kind[:3]]))).tobytes() == got.tobytes()


def test_more_work_items_than_the_grid_cap():
    """planes of 3 pixels are one tile, a work item is a tile of 8 cases and a workgroup takes 4 at a time: 32 cap + 43 cases
    are cap + 2 workgroups' worth, so the first workgroups walk their loop twice with a ragged last run of cases; the fold
    takes 4 cases a workgroup and goes round 8 times.  fp32: 1.5 MB an operand"""
    cap = _cap("BD_MOMENT_GROUPS")
    n = 32 * cap + 43
    rng = np.random.default_rng(3)
    a = rng.normal(290.0, 5.0, (n, 3)).astype(np.float32)
    preds = [(a + rng.normal(0.0, 1.0 + k, (n, 3))).astype(np.float32) for k in range(2)]
    a[rng.random(a.shape) < 0.02] = np.nan
    a[n - 1] = np.inf
    got = case_error_moments([p.reshape(n, 1, 1, 3) for p in preds], a.reshape(n, 1, 1, 3))
    blend_ref.Reference(preds, a).check(got, f"{n} cases past the cap of {cap} workgroups")
    assert (got[n - 1] == 0.0).all() and got[:, 0].sum() > 2.9 * n


# ---- cae_blend_predictions -------------------------------------------------------------------------------------------------

# (3, 2, 1, 33): 66 elements a case - fp64 cases start on 16-byte boundaries and end in a ragged quad
BLEND_SHAPES = [(N, C, 1, 67), (N, C, 70, 70), (3, 2, 1, 33)]


@lru_cache(maxsize=None)
def _candidates(shape, m):
    rng = np.random.default_rng(sum(shape) + m)
    preds = [rng.normal(290.0, 5.0 + k, shape) for k in range(m)]
    for p in preds[:2]:
        where = rng.random(shape) < 0.03
        p[where] = rng.choice([math.nan, math.inf, -math.inf], int(where.sum()))
    for p in preds:
        p.setflags(write=False)
    return tuple(preds)


@pytest.mark.parametrize("kind", ["f32", "f64", "f32be", "f64be", "mixed"])
@pytest.mark.parametrize("shape", BLEND_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_blend_against_the_numpy_loop(shape, kind):
    for (m, weights, intercept) in ((1, [1.0], 0.0), (2, [0.25, 0.75], 0.0), (3, [0.7, -0.3, 0.6], 1.5), (5, [0.1, 0.2, 0.3, 0.25, 0.15], -2.0 ** -3),
                                    (8, [0.3, 0.0, 0.1, 0.05, -0.0, 0.25, 0.2, 0.1], 0.0)):
        kinds = [["f32", "f64be", "f64", "f32be"][k % 4] if kind == "mixed" else kind for k in range(m)]
        preds = [p.astype(KINDS[k]) for (p, k) in zip(_candidates(shape, m), kinds)]
        got = blend_predictions(preds, weights, intercept)
        assert got.shape == shape and got.dtype == np.float64
        want = blend_ref.blend(preds, weights, intercept)
        np.testing.assert_array_equal(got, want, err_msg=f"{shape} {kind} M {m}")
        assert np.isnan(got).any() and np.isfinite(got).any()
        if m == 1:      # w = 1 and c = 0: the candidate itself where it is finite
            first = preds[0].astype(np.float64)
            assert np.array_equal(got[np.isfinite(first)], first[np.isfinite(first)]) and np.isnan(got[~np.isfinite(first)]).all()


def test_a_zero_weight_over_a_candidate_that_is_all_nan():
    shape = (N, C, 1, 67)
    preds = [np.array(p) for p in _candidates(shape, 3, )]
    preds[1][:] = math.nan
    weights = [0.4, 0.0, 0.6]
    got = blend_predictions(preds, weights, 0.5)
    np.testing.assert_array_equal(got, blend_ref.blend(preds, weights, 0.5))
    np.testing.assert_array_equal(got, blend_ref.blend([preds[0], preds[2]], [0.4, 0.6], 0.5))
    assert np.array_equal(np.isnan(got), ~(np.isfinite(preds[0]) & np.isfinite(preds[2])))
    assert np.isnan(blend_predictions(preds, [0.4, 1e-300, 0.6], 0.5)).all()       # a weight that is not 0 reads it
    # every weight 0: the intercept everywhere, no candidate read
    assert (blend_predictions(preds, [0.0, 0.0, 0.0], 0.25) == 0.25).all()


def test_blend_past_the_grid_cap():
    """a lane takes 4 elements and a workgroup 1024 at a time: 2 cases of 1024 x 1028 fp32 are 4096 elements past the cap's
    reach, on the 16-byte path"""
    cap = _cap("BD_FIELD_GROUPS")
    shape = (2, 1, 1024, cap // 2 + 4)
    assert shape[0] * shape[2] * shape[3] > cap * 1024
    rng = np.random.default_rng(8)
    preds = [rng.normal(290.0, 5.0, shape).astype(np.float32) for _ in range(2)]
    preds[1][1, 0, 1023, -5:] = np.inf
    got = blend_predictions(preds, [0.375, 0.625])
    np.testing.assert_array_equal(got, blend_ref.blend(preds, [0.375, 0.625]))
    assert np.isnan(got[1, 0, 1023, -5:]).all() and np.isfinite(got[1, 0, 1023, :-5]).all()


# ---- blend fit -> blend apply ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scored(tmp_path_factory):
    """12 cases of 1 x 20 x 20: the target and three candidates, each the target plus a shared and an own noise of different
    sizes; the third candidate is stored in fp32; a day per three cases"""
    from cae_tools_amd.data import netcdf3
    root = tmp_path_factory.mktemp("blend")
    rng = np.random.default_rng(21)
    shape = (12, 1, 20, 20)
    a = rng.normal(290.0, 5.0, shape)
    shared = rng.normal(0.0, 1.0, shape)
    fields = {"hires": a, "conv_output": a + 0.8 * shared + rng.normal(0.1, 0.6, shape), "unet_output": a + 0.5 * shared + rng.normal(-0.1, 0.9, shape),
              "linear_output": (a - 0.4 * shared + rng.normal(0.0, 1.2, shape)).astype(np.float32)}
    dims = ("n", "c", "y", "x")
    variables = {name: (dims, x, {}) for (name, x) in fields.items()}
    variables["day"] = (("n",), np.repeat(np.arange(4.0), 3), {})
    path = str(root / "scored.nc")
    netcdf3.write(path, {"n": 12, "c": 1, "y": 20, "x": 20}, variables)
    return root, path, fields


@pytest.mark.parametrize("flags", [[], ["--blend-mode", "affine", "--blend-intercept", "--blend-block-variable", "day", "--blend-folds", "2"]],
                         ids=["convex", "affine-intercept-blocks"])
def test_fit_then_apply(scored, flags):
    from cae_tools_amd.cli import blend as cli
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.utils import blend, compare
    (root, path, fields) = scored
    tag = "b" if flags else "a"
    (record_path, out_path, report) = (str(root / f"blend_{tag}.json"), str(root / f"blended_{tag}.nc"), str(root / f"report_{tag}"))
    names = ["conv_output", "unet_output", "linear_output"]
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["fit", "--inputs", path, "--output-variable", "hires", "--blend-variables", *names, "--blend-labels", "conv", "unet", "linear",
                  "--blend-resamples", "300", "--blend-seed", "3", "--blend-file", record_path, "--output-html-folder", report] + flags)
        cli.main(["apply", path, out_path, "--blend-file", record_path])
    with open(record_path) as f:
        rec = json.loads(f.read(), parse_constant=lambda name: pytest.fail(f"{name} is not strict JSON"))
    for key in ("variables", "labels", "mode", "fit_intercept", "weights", "weights_hex", "intercept", "intercept_hex", "n_cases", "n_unit",
                "pixels_counted", "pixels_left_out", "candidates", "error_correlation", "mse_blend", "best_single", "mse_best_single", "gain",
                "cross_validation", "resamples", "seed", "confidence", "block_variable"):
        assert key in rec, key
    assert (rec["variables"], rec["labels"], rec["n_cases"], rec["pixels_counted"], rec["pixels_left_out"]) == (names, ["conv", "unet", "linear"], 12, 4800, 0)
    assert (rec["n_unit"], rec["mode"], rec["fit_intercept"], rec["cross_validation"]["folds"]) == ((4, "affine", True, 2) if flags else (12, "convex", False, 5))
    w = np.array([float.fromhex(t) for t in rec["weights_hex"]])
    c = float.fromhex(rec["intercept_hex"])
    assert w.tolist() == rec["weights"] and c == rec["intercept"] and abs(w.sum() - 1.0) < 1e-12 and (bool(flags) or (c == 0.0 and (w > 0).all()))
    for cand in rec["candidates"]:
        assert cand["weight"]["interval"][0] <= cand["weight"]["value"] <= cand["weight"]["interval"][1] and cand["weight"]["degenerate"] == 0
    assert rec["gain"]["interval"][0] <= rec["gain"]["value"] <= rec["gain"]["interval"][1] and rec["gain"]["value"] > 0.0
    assert rec["cross_validation"]["mse_blend"] < rec["cross_validation"]["mse_best_single"]
    lines = [ln for ln in log.getvalue().splitlines() if ln.startswith("blend")]
    assert len(lines) == 2 and lines[0].startswith(f"blend: 3 candidates, {rec['n_unit']} units, {rec['mode']}") and lines[1].startswith("blend apply: ")
    with open(os.path.join(report, "blend", "index.html")) as f:
        page = f.read()
    assert page.count("<h2>Error correlation</h2>") == 1 and page.count('alt="weights of the blend"') == 1

    # the record is the restatement's: the moments, the fit and the resamples' ranks from the package's host code
    table = compare.units(case_error_moments([fields[v] for v in names], fields["hires"]), np.repeat(np.arange(4.0), 3) if flags else None)[0]
    blend_ref.Reference([fields[v].reshape(12, -1) for v in names], fields["hires"].reshape(12, -1)).check(
        case_error_moments([fields[v] for v in names], fields["hires"]), "the scored file")
    found = blend.fit(table, rec["mode"], rec["fit_intercept"])
    assert np.array_equal(found["weights"], w) and found["intercept"] == c and found["mse_blend"] == rec["mse_blend"]

    # the written file: the inputs' variables unchanged plus the new one, which is the numpy loop's
    (before, after) = (open_dataset(path), open_dataset(out_path))
    assert list(after.data_vars) == list(before.data_vars) + ["blend_output"]
    for name in before.data_vars:
        (x, y) = (np.asarray(before[name].values), np.asarray(after[name].values))
        assert x.dtype == y.dtype and tuple(before[name].dims) == tuple(after[name].dims) and x.tobytes() == y.tobytes(), name
    field = np.asarray(after["blend_output"].values)
    assert field.dtype == np.float64 and tuple(after["blend_output"].dims) == tuple(before["conv_output"].dims)
    np.testing.assert_array_equal(field, blend_ref.blend([fields[v] for v in names], w, c))

    # the blend's mse as cae_case_compare measures it: no larger than any candidate's, and the record's within the bound
    total = compare.column_sums(case_compare([field], fields["hires"]))
    measured = total[4] / total[0]
    singles = compare.column_sums(case_compare([fields[v] for v in names], fields["hires"]))
    each = [singles[4 + 4 * k] / singles[0] for k in range(3)]
    assert total[0] == 4800 and measured <= min(each)
    assert all(math.isclose(cand["mse"], v, rel_tol=1e-13) for (cand, v) in zip(rec["candidates"], each))      # blocks add in another order
    (bound, parts) = blend_ref.end_to_end_bound([fields[v].astype(np.float64).reshape(12, -1) for v in names], fields["hires"].reshape(12, -1), w, c)
    gap = abs(measured - rec["mse_blend"])
    print(f"blend {rec['mode']}: measured mse {measured!r}, the record's {rec['mse_blend']!r}, |difference| {gap:.3e}, bound {bound:.3e} "
          f"({', '.join(f'{k} {v:.3e}' for (k, v) in parts.items())}), ratio {gap / bound:.3e}")
    assert gap <= bound
    with pytest.raises(ValueError, match="already holds a variable 'blend_output'"):
        cli.main(["apply", out_path, str(root / "again.nc"), "--blend-file", record_path])
