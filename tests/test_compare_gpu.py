"""cae_case_compare and cae_bootstrap_sums on the GPU.  The per-case rows against the numpy restatement of the definition
(compare_ref.py, np.longdouble): n, tied and the wins exactly, every floating-point sum of m terms within (m + 4) 2^-53 S|t| -
for every plane, number of cases, number of candidates, element kind and non-finite value; a case's independence from the
call, run-to-run identity and whole rows, byte for byte; refused calls write nothing.  The resampled sums against the
restatement's sequential sums with np.array_equal, on both sides of the LDS budget (160 KiB) and of the lane-shape threshold
(2^17 lanes), with rows of NaN, inf and -0.0 and a cut into two calls.  Then train_cae -> apply_cae -> compare with a copy
and a noisy copy of the prediction as competitors.

Largest |got - want| / bound measured on an MI355X (each check of the sums prints its figure before it asserts): 0.19 at
plane 1 (9 cases, M = 8: one term, where the three roundings of a square stand against a bound of five), 0.034 at plane 65,
5.5e-4 at plane 4099, 0.011 over the 16 pairs of element kinds, 0.0070 with NaN and inf, 2.3e-5 on the scored file of the
workflow.  n, tied and the wins are exact everywhere, the resampled sums the restatement's bits at every shape."""
import ctypes as C
import io
import json
import math
import os
from contextlib import redirect_stdout
from fractions import Fraction

import numpy as np
import pytest
import torch

import compare_ref
from compare_ref import Reference
from cae_tools_amd import _lib
from cae_tools_amd.case_ops import bootstrap_sums, case_compare, device_operand, operand_cases

pytestmark = pytest.mark.gpu

KINDS = {"f32": _lib.ELEM_F32, "f32be": _lib.ELEM_F32_BE, "f64": _lib.ELEM_F64, "f64be": _lib.ELEM_F64_BE}


def _fields(rng, m, n, plane, dtype=np.float64):
    """a target and m predictions (n, plane): the predictions the target plus noise of a growing size, some pixels shared
    exactly between neighbours so that ties occur"""
    a = rng.normal(290.0, 5.0, (n, plane)).astype(dtype)
    preds = []
    for k in range(m):
        p = (a + rng.normal(0.1 * k, 1.0 + 0.2 * k, (n, plane))).astype(dtype)
        if k:
            same = rng.random((n, plane)) < 0.1
            p[same] = preds[k - 1][same]
        preds.append(p)
    return preds, a


def _shape(x, c=1):
    """(n, plane) as an (n, c, 1, plane) operand whose channel 0 holds x"""
    out = np.full((x.shape[0], c, 1, x.shape[1]), 7.5, dtype=x.dtype)
    out[:, 0, 0] = x
    return out


# ---- cae_case_compare ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 3, 8])
@pytest.mark.parametrize("n_case", [1, 3, 9])
@pytest.mark.parametrize("plane", [1, 63, 64, 65, 4099])
def test_planes_cases_and_candidates(plane, n_case, m):
    """4099 pixels are 65 tiles: a lane of the fold takes a second tile; 9 cases are a second run of cases"""
    (preds, a) = _fields(np.random.default_rng(plane * 100 + n_case * 10 + m), m, n_case, plane)
    got = case_compare([_shape(p) for p in preds], _shape(a))
    assert got.shape == (n_case, 2 + 4 * m)
    ref = Reference(preds, a)
    ref.check(got, f"plane {plane}, {n_case} cases, M {m}")
    if m == 1:
        assert np.array_equal(got[:, 5], got[:, 0]) and (got[:, 1] == 0).all()
    elif plane >= 63:
        assert got[:, 1].sum() > 0          # the shared pixels tie


def test_every_element_kind_and_two_channels(tmp_path):
    """predictions and target as fp32, fp64 and as the big-endian slabs of a NetCDF-3 file; operands with C = 2; predictions
    of mixed kinds, which the wrapper converts to fp64 on the device"""
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import as_numpy, open_dataset
    (n, h, w) = (3, 5, 31)
    (preds, a) = _fields(np.random.default_rng(5), 2, n, h * w)
    wide = lambda x, dtype: np.stack([x.reshape(n, h, w), np.full((n, h, w), -3.0)], axis=1).astype(dtype)    # noqa: E731
    variables = {}
    for (name, x) in (("a", a), ("p0", preds[0]), ("p1", preds[1])):
        variables[name + "32"] = (("n", "c", "y", "x"), wide(x, np.float32), {})
        variables[name + "64"] = (("n", "c", "y", "x"), wide(x, np.float64), {})
    path = str(tmp_path / "kinds.nc")
    netcdf3.write(path, {"n": n, "c": 2, "y": h, "x": w}, variables)
    ds = open_dataset(path)

    def operand(name, kind):
        x = {"a": a, "p0": preds[0], "p1": preds[1]}[name]
        if kind.endswith("be"):
            slab = as_numpy(ds[name + ("32" if kind == "f32be" else "64")])
            assert slab.dtype.byteorder == ">"
            return device_operand(slab)
        return device_operand(wide(x, np.float32 if kind == "f32" else np.float64))

    f32 = lambda x: x.astype(np.float32)      # noqa: E731
    refs = {(4, 4): Reference([f32(p) for p in preds], f32(a)), (4, 8): Reference([f32(p) for p in preds], a),
            (8, 4): Reference(preds, f32(a)), (8, 8): Reference(preds, a)}
    found = {}
    for kp in KINDS:
        for ka in KINDS:
            ops = [operand("p0", kp), operand("p1", kp)]
            t = operand("a", ka)
            assert ops[0].kind == KINDS[kp] and t.kind == KINDS[ka] and ops[0].shape[1] == 2
            found[(kp, ka)] = case_compare(ops, t)
            refs[(ops[0].elem_bytes, t.elem_bytes)].check(found[(kp, ka)], f"{kp} against {ka}")
            part = case_compare([operand_cases(op, 1, 3) for op in ops], operand_cases(t, 1, 3))
            assert part.tobytes() == found[(kp, ka)][1:].tobytes()
    for ka in KINDS:        # the byte order changes no bit
        assert found[("f32", ka)].tobytes() == found[("f32be", ka)].tobytes() and found[("f64", ka)].tobytes() == found[("f64be", ka)].tobytes()
    # mixed kinds: the odd ones are converted to native fp64 exactly
    for (k0, k1) in (("f32", "f64"), ("f32be", "f64be"), ("f64be", "f32")):
        mixed = case_compare([operand("p0", k0), operand("p1", k1)], operand("a", "f64"))
        want = Reference([f32(preds[0]) if "32" in k0 else preds[0], f32(preds[1]) if "32" in k1 else preds[1]], a)
        want.check(mixed, f"{k0} with {k1}")


def test_values_that_are_not_finite_and_a_case_without_a_pair():
    rng = np.random.default_rng(9)
    (preds, a) = _fields(rng, 3, 4, 200)
    for (x, bad) in ((a, [math.nan, math.inf, -math.inf]), (preds[1], [math.nan, -math.inf, math.inf])):
        where = rng.random(x.shape) < 0.05
        x[where] = rng.choice(bad, int(where.sum()))
    a[2] = math.nan             # a case without a pair
    got = case_compare([_shape(p) for p in preds], _shape(a))
    ref = Reference(preds, a)
    ref.check(got, "NaN and inf in the target and in one candidate")
    assert (got[2] == 0.0).all() and not np.signbit(got[2]).any() and 0 < got[0, 0] < 200
    assert (got[:, 0] == ref.pair.sum(axis=1)).all()


def test_identical_candidates_tie_everywhere():
    (preds, a) = _fields(np.random.default_rng(4), 1, 3, 130)
    got = case_compare([_shape(preds[0]), _shape(preds[0].copy())], _shape(a))
    Reference([preds[0], preds[0]], a).check(got, "two identical candidates")
    assert np.array_equal(got[:, 1], got[:, 0]) and (got[:, 5] == 0).all() and (got[:, 9] == 0).all()
    assert np.array_equal(got[:, 2:5], got[:, 6:9])


def test_a_case_does_not_depend_on_the_call_and_two_runs_are_identical():
    (preds, a) = _fields(np.random.default_rng(6), 3, 11, 4099)
    ops = [device_operand(_shape(p, c=2)) for p in preds]
    t = device_operand(_shape(a))
    full = case_compare(ops, t)
    assert case_compare(ops, t).tobytes() == full.tobytes()
    for (c0, c1) in ((0, 1), (3, 8), (8, 11), (10, 11)):
        part = case_compare([operand_cases(op, c0, c1) for op in ops], operand_cases(t, c0, c1))
        assert part.tobytes() == full[c0:c1].tobytes(), (c0, c1)
    # an operand that starts at an odd element: the alignment changes no bit
    flat = torch.from_numpy(np.concatenate([np.zeros(1), preds[0].reshape(-1)])).cuda()
    shifted = flat[1:].view(11, 1, 1, 4099)
    assert shifted.data_ptr() % 16 == 8
    lib = _lib.load()
    out = torch.empty((11, 14), dtype=torch.float64, device="cuda")
    need = int(lib.cae_case_compare_workspace_bytes(11, 4099, 3))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * 3)(shifted.data_ptr(), ops[1].tensor.data_ptr(), ops[2].tensor.data_ptr())
    strides = (C.c_int64 * 3)(4099, ops[1].stride, ops[2].stride)
    assert lib.cae_case_compare(ptrs, _lib.ELEM_F64, strides, 3, *t.args(), 11, 4099, out.data_ptr(), ws.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == full.tobytes()


def test_rows_are_written_whole_and_bad_arguments_write_nothing():
    lib = _lib.load()
    (n, plane, m) = (3, 70, 2)
    (preds, a) = _fields(np.random.default_rng(2), m, n, plane)
    dev = [torch.from_numpy(x).cuda() for x in preds + [a]]
    out = torch.full((n * 10,), -7.0, dtype=torch.float64, device="cuda")
    need = int(lib.cae_case_compare_workspace_bytes(n, plane, m))
    assert need == n * 2 * 10 * 8
    ws = torch.full((need // 8,), -7.0, dtype=torch.float64, device="cuda")
    good = dict(ptrs=[dev[0].data_ptr(), dev[1].data_ptr()], kp=_lib.ELEM_F64, strides=[plane, plane], m=m, a=dev[2].data_ptr(),
                ka=_lib.ELEM_F64, as_=plane, n=n, plane=plane, sums=out.data_ptr(), ws=ws.data_ptr(), wsb=need)

    def call(**change):
        g = dict(good, **change)
        ptrs = (C.c_void_p * len(g["ptrs"]))(*g["ptrs"])
        strides = (C.c_int64 * len(g["strides"]))(*g["strides"])
        return lib.cae_case_compare(ptrs, g["kp"], strides, g["m"], g["a"], g["ka"], g["as_"], g["n"], g["plane"], g["sums"], g["ws"],
                                    g["wsb"], None)

    bad = [(dict(kp=4), "bad argument"), (dict(m=0), "bad argument"), (dict(m=9), "bad argument"), (dict(n=-1), "bad argument"),
           (dict(strides=[plane, -1]), "negative stride"), (dict(ptrs=[dev[0].data_ptr(), None]), "null pointer"),
           (dict(sums=None), "null pointer"), (dict(as_=plane - 1), "shorter than the plane"), (dict(strides=[1 << 59, plane]), "reaches 2^60"),
           (dict(a=dev[2].data_ptr() + 4), "aligned"), (dict(ws=ws.data_ptr() + 8), "aligned"),
           (dict(wsb=need - 1), f"needs a workspace of {need} bytes"), (dict(ws=None), f"needs a workspace of {need} bytes")]
    for (change, text) in bad:
        assert call(**change) == -1 and text in lib.cae_last_error().decode(), (change, lib.cae_last_error())
    for change in (dict(n=0), dict(plane=0)):
        assert call(**change) == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (ws == -7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(n, 10)
    Reference(preds, a).check(got, "over a pre-filled output")       # every entry was overwritten: none is -7
    table = torch.full((37 * 3,), 1.0, dtype=torch.float64, device="cuda")
    res = torch.full((100 * 3,), -7.0, dtype=torch.float64, device="cuda")
    for change in (dict(n_unit=0), dict(n_col=33), dict(first=(1 << 32) - 99), dict(table=None), dict(out=res.data_ptr() + 4)):
        g = dict(dict(table=table.data_ptr(), n_unit=37, n_col=3, first=0, b=100, seed=0, out=res.data_ptr()), **change)
        assert lib.cae_bootstrap_sums(g["table"], g["n_unit"], g["n_col"], g["first"], g["b"], g["seed"], g["out"], None) == -1
    torch.cuda.synchronize()
    assert (res == -7.0).all()


# ---- cae_bootstrap_sums ----------------------------------------------------------------------------------------------------

# (n_unit, n_col, resamples).  2048 x 10 doubles are exactly the 160 KiB LDS budget, 2049 x 10 just above it (read through
# L2).  (5, 5, 65536) has 2^17 lanes of 4 columns, the threshold from which a lane takes 4 columns, (5, 5, 65535) stays below
# it (a lane a column); (5200, 4, 131072) is at that threshold with a table above the LDS budget.
SHAPES = [(1, 1, 1), (3, 2, 65), (37, 3, 4096), (130, 26, 257), (2049, 5, 64), (2048, 10, 96), (2049, 10, 96), (5, 5, 65536), (5, 5, 65535),
          (5200, 4, 131072)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resampled_sums_are_the_restatements_bits(shape):
    (n_unit, n_col, b) = shape
    rng = np.random.default_rng(n_unit * 7 + n_col)
    table = rng.gamma(2.0, 1.0, (n_unit, n_col)) * rng.choice([-1.0, 1.0], (n_unit, n_col))
    got = bootstrap_sums(table, b, seed=5)
    assert got.shape == (b, n_col) and got.dtype == np.float64
    rows = b if n_unit <= 2049 else 64           # the restatement's loop over the draws: all resamples where it is short
    assert np.array_equal(got[:rows], compare_ref.sums(table, rows, seed=5))
    if rows < b:
        assert np.array_equal(got[-rows:], compare_ref.sums(table, rows, seed=5, first=b - rows))


def test_nan_inf_and_negative_zero_propagate_as_ieee_adds():
    table = np.random.default_rng(1).normal(0.0, 1.0, (37, 4))
    table[3, 0] = math.nan
    table[5, 1] = math.inf
    table[7, 1] = -math.inf
    table[:, 2] = -0.0
    table[:, 3] = 0.0
    table[11, 3] = -0.0
    got = bootstrap_sums(table, 257, seed=3)
    want = compare_ref.sums(table, 257, seed=3)
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))
    assert np.isnan(got[:, 0]).any() and np.isfinite(got[:, 0]).any() and np.isnan(got[:, 1]).any() and np.isinf(got[:, 1]).any()
    assert (got[:, 2] == 0.0).all() and not np.signbit(got[:, 2:]).any()      # +0.0 + -0.0 is +0.0


def test_a_cut_of_the_resamples_and_the_pairing():
    table = np.random.default_rng(2).gamma(2.0, 1.0, (130, 26))
    whole = bootstrap_sums(table, 257, seed=(1 << 64) - 3)
    assert np.array_equal(whole, compare_ref.sums(table, 257, seed=(1 << 64) - 3))
    cut = np.concatenate([bootstrap_sums(table, 100, seed=(1 << 64) - 3), bootstrap_sums(table, 157, seed=(1 << 64) - 3, first=100)])
    assert cut.tobytes() == whole.tobytes() and bootstrap_sums(table, 257, seed=(1 << 64) - 3).tobytes() == whole.tobytes()
    # another table of the same n_unit takes the same units: a column of ones counts them, the identity column names them
    j = compare_ref.units(130, 257, seed=(1 << 64) - 3)
    other = np.stack([np.ones(130), np.arange(130.0)], axis=1)
    got = bootstrap_sums(other, 257, seed=(1 << 64) - 3)
    assert (got[:, 0] == 130.0).all() and np.array_equal(got[:, 1], j.sum(axis=1).astype(np.float64))
    top = bootstrap_sums(other, 3, seed=1, first=(1 << 32) - 3)              # the last resamples there are
    assert np.array_equal(top, compare_ref.sums(other, 3, seed=1, first=(1 << 32) - 3))


# ---- train_cae -> apply_cae -> compare --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def workflow(tmp_path_factory):
    """a tiny ConvAE trained for 2 epochs and applied; a copy of its prediction and a copy plus seeded noise as two more
    variables of the scored file, and a day per three cases"""
    from cae_tools_amd.cli import apply_cae, train_cae
    from cae_tools_amd.data import datagen, netcdf3
    from cae_tools_amd.data.arrays import open_dataset
    root = tmp_path_factory.mktemp("compare")
    paths = {}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        ds = datagen.generate("circle", 12, seed=seed)
        paths[part] = str(root / f"{part}.nc")
        netcdf3.write(paths[part], {d: int(k) for (d, k) in ds.dims.items()},
                      {name: (tuple(da.dims), np.asarray(da.values), {}) for (name, da) in ds.data_vars.items()})
    (model_dir, plain, scored) = (str(root / "model"), str(root / "plain.nc"), str(root / "scored.nc"))
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model_dir,
                        "--input-variables", "lowres", "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"])
        apply_cae.main([paths["test"], plain, "--model-folder", model_dir])
    ds = open_dataset(plain)
    variables = {name: (tuple(da.dims), np.asarray(da.values), {}) for (name, da) in ds.data_vars.items()}
    (dims, pred, _) = variables["model_output"]
    spread = float(np.std(np.asarray(ds["hires"].values)))
    variables["copy_output"] = (dims, pred.copy(), {})
    variables["noisy_output"] = (dims, pred + np.random.default_rng(7).normal(0.0, 0.5 * spread, pred.shape).astype(pred.dtype), {})
    variables["day"] = ((dims[0],), np.repeat(np.arange(4.0), 3), {})
    netcdf3.write(scored, {d: int(k) for (d, k) in ds.dims.items()}, variables)
    return root, model_dir, plain, scored


def _inside(stat):
    return stat["interval"][0] <= stat["value"] <= stat["interval"][1]


def test_train_apply_compare(workflow):
    from cae_tools_amd.cli import compare as cli
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.utils import compare
    (root, model_dir, plain, scored) = workflow
    flags = ["--test-inputs", scored, "--model-folder", model_dir, "--compare-variables", "copy_output", "noisy_output",
             "--compare-labels", "ours", "copy", "noisy", "--compare-resamples", "2000", "--compare-seed", "3", "--compare-baseline", "bicubic"]
    (out1, out2, out3) = (str(root / "report_1"), str(root / "report_2"), str(root / "report_3"))
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(flags + ["--output-html-folder", out1])
    with redirect_stdout(io.StringIO()):
        cli.main(flags + ["--output-html-folder", out2])
        cli.main(flags + ["--output-html-folder", out3, "--compare-block-variable", "day", "--compare-confidence", "9/10"])
    with open(os.path.join(out1, "compare_test.json"), "rb") as f:
        text = f.read()
    with open(os.path.join(out2, "compare_test.json"), "rb") as f:
        assert f.read() == text                 # the same command twice writes the same bytes
    rec = json.loads(text, parse_constant=lambda name: pytest.fail(f"{name} is not strict JSON"))
    assert sorted(f for f in os.listdir(out1) if f.startswith("compare_")) == ["compare_test.json"]
    for key in ("variables", "labels", "resamples", "seed", "confidence", "block_variable", "n_cases", "n_unit", "pixels_counted",
                "pixels_left_out", "pixels_tied", "tied_share", "candidates", "competitors", "baseline"):
        assert key in rec, key
    assert (rec["variables"], rec["labels"]) == (["model_output", "copy_output", "noisy_output"], ["ours", "copy", "noisy"])
    assert (rec["resamples"], rec["seed"], rec["confidence"], rec["block_variable"]) == (2000, 3, "19/20", None)
    assert (rec["n_cases"], rec["n_unit"], rec["pixels_counted"], rec["pixels_left_out"]) == (12, 12, 12 * 256 * 256, 0)
    for cand in rec["candidates"]:
        for key in compare.CANDIDATE_STATS:
            assert set(cand[key]) == {"value", "interval", "degenerate"} and _inside(cand[key]) and cand[key]["degenerate"] == 0, (cand["label"], key)
    (copy, noisy) = rec["competitors"]
    for comp in (copy, noisy):
        for key in ("delta_mse", "skill", "p_better", "significant", "win_share", "reference_win_share", "tied_share"):
            assert key in comp, key
        assert _inside(comp["delta_mse"]) and _inside(comp["skill"])
    assert copy["delta_mse"]["value"] == 0.0 and copy["delta_mse"]["interval"] == [0.0, 0.0] and copy["significant"] is False
    assert copy["win_share"] == 0.0 and copy["p_better"] == 0.0 and rec["candidates"][0]["win_share"] == 0.0
    assert noisy["significant"] is True and noisy["delta_mse"]["interval"][0] > 0.0 and noisy["p_better"] == 1.0 and noisy["skill"]["value"] > 0.0
    # the copy ties the model wherever the noisy copy is not nearer to the target
    assert 0.0 < noisy["win_share"] < 0.5 and rec["pixels_tied"] + round(noisy["win_share"] * rec["pixels_counted"]) == rec["pixels_counted"]
    assert rec["candidates"][0]["mse"] == rec["candidates"][1]["mse"]
    base = rec["baseline"]
    assert (base["mode"], base["variable"]) == ("bicubic", "lowres") and _inside(base["skill"]) and _inside(base["baseline_mse"])

    # the record is the restatement's: the sums, their resamples and the ranks from numpy
    ds = open_dataset(scored)
    table = case_compare([np.asarray(ds[v].values) for v in rec["variables"]], np.asarray(ds["hires"].values))
    Reference([np.asarray(ds[v].values)[:, 0] for v in rec["variables"]], np.asarray(ds["hires"].values)[:, 0]).check(table, "the scored file")
    resampled = compare_ref.sums(table, 2000, seed=3)
    total = compare.column_sums(table)
    for k in range(3):
        (lo, hi, _) = compare_ref.interval(compare_ref.mse(resampled, k), Fraction(19, 20))
        assert rec["candidates"][k]["mse"] == {"value": compare_ref.mse(total, k), "interval": [lo, hi], "degenerate": 0}
    delta = compare_ref.mse(resampled, 2) - compare_ref.mse(resampled, 0)
    assert noisy["delta_mse"]["interval"] == list(compare_ref.interval(delta, Fraction(19, 20))[:2])

    # the printed line and the report's section
    lines = [ln for ln in log.getvalue().splitlines() if ln.startswith("compare ")]
    assert len(lines) == 1 and lines[0].startswith("compare test: 3 candidates, 12 units x 2000 resamples at 19/20: ours mse ")
    assert "copy delta 0 [0, 0] (not significant)" in lines[0] and "(significant)" in lines[0] and "skill against interpolation of lowres" in lines[0]
    with open(os.path.join(out1, "index.html")) as f:
        page = f.read()
    assert page.count("<h2>Model comparison</h2>") == 1 and page.count('alt="test mse by candidate"') == 1

    # blocks: four days of three cases are the units
    with open(os.path.join(out3, "compare_test.json")) as f:
        blocks = json.load(f)
    assert (blocks["n_unit"], blocks["n_cases"], blocks["block_variable"], blocks["confidence"]) == (4, 12, "day", "9/10")
    units = compare_ref.block_units(table, np.repeat(np.arange(4.0), 3).tolist())
    (lo, hi, _) = compare_ref.interval(compare_ref.mse(compare_ref.sums(units, 2000, seed=3), 2), Fraction(9, 10))
    assert blocks["candidates"][2]["mse"]["interval"] == [lo, hi]


def test_no_variables_gives_the_models_own_intervals_and_no_flags_evaluate_caes_files(workflow):
    from cae_tools_amd.cli import compare as cli, evaluate_cae
    (root, model_dir, plain, scored) = workflow
    (own, off, ref) = (str(root / "own"), str(root / "off"), str(root / "ref"))
    with redirect_stdout(io.StringIO()):
        cli.main(["--test-inputs", plain, "--model-folder", model_dir, "--output-html-folder", own, "--compare-resamples", "500"])
        evaluate_cae.main(["--test-inputs", plain, "--model-folder", model_dir, "--output-html-folder", ref])
        evaluate_cae.main(["--test-inputs", plain, "--model-folder", model_dir, "--output-html-folder", off])
    with open(os.path.join(own, "compare_test.json")) as f:
        rec = json.load(f)
    assert len(rec["candidates"]) == 1 and rec["competitors"] == [] and rec["baseline"] is None and rec["tied_share"] == 0.0
    assert rec["candidates"][0]["win_share"] == 1.0 and all(_inside(rec["candidates"][0][k]) for k in ("mse", "rmse", "mae", "bias"))
    # without the option the evaluator writes what it wrote before: the same files with the same bytes, and the page with the
    # option on is that page up to the new section
    assert sorted(os.listdir(off)) == sorted(os.listdir(ref)) == ["index.html"]
    with open(os.path.join(off, "index.html"), "rb") as f, open(os.path.join(ref, "index.html"), "rb") as g:
        plain_page = f.read()
        assert plain_page == g.read() and b"Model comparison" not in plain_page
    with open(os.path.join(own, "index.html"), "rb") as f:
        page = f.read()
    start = page.index(b"<h2>Model comparison</h2>")
    assert plain_page.startswith(page[:start].rstrip())
