"""The host side of the interpolation baseline without a GPU: the numpy restatement of the definition (baseline_ref.py)
against torch.nn.functional.interpolate in float64 within the reference's own bound, identity sizes, the counting rule
around a NaN tap, the rules of utils/baseline.scores_from_sums and summary, the strict JSON, the command's flags, the
report's section and the library's exports.

Largest |torch fp64 - reference| / bound measured (each check prints its figure): 0.24 (bicubic, (2,3) -> (7,5)), 0.089
(bilinear, (16,16) -> (256,256)), 0 for nearest: torch evaluates the cubics in fp64 in the definition's unfactored form, whose
error is absolute, and still stays inside the bound derived for the kernel's factored form on these fields."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import baseline_ref
from baseline_ref import Reference
from cae_tools_amd.utils import baseline, report

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("nearest", "bilinear", "bicubic")
TORCH_MODES = {"nearest": "nearest-exact", "bilinear": "bilinear", "bicubic": "bicubic"}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shapes", [((1, 1), (3, 5)), ((2, 3), (7, 5)), ((4, 4), (64, 64)), ((16, 16), (256, 256)), ((9, 9), (4, 4))])
def test_reference_against_torch_in_fp64(shapes, mode):
    import torch
    (i, o) = shapes
    rng = np.random.default_rng(i[0] * 10 + o[1])
    low = 290.0 + 5.0 * rng.random((2,) + i)
    (field, mag, ok) = baseline_ref.upsample(low, o, mode)
    assert ok.all() and field.shape == (2,) + o
    kw = {} if mode == "nearest" else {"align_corners": False}
    got = torch.nn.functional.interpolate(torch.from_numpy(low)[:, None], size=o, mode=TORCH_MODES[mode], **kw)[:, 0].numpy()
    assert got.dtype == np.float64
    err = np.abs(got.astype(np.longdouble) - field)
    bound = baseline_ref.K * baseline_ref.U * mag
    print(f"torch fp64 vs reference {i} -> {o} {mode}: max |got - want| / bound = {float(np.max(err / bound)):.3e}")
    assert (err <= bound).all()
    if mode == "nearest":
        assert (err == 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(1, 1), (3, 3), (5, 8)])
def test_identity_sizes_give_the_input_bit_for_bit(shape, mode):
    rng = np.random.default_rng(3)
    low = rng.standard_normal((2,) + shape)
    (field, _, ok) = baseline_ref.upsample(low, shape, mode)
    assert ok.all() and field.astype(np.float64).tobytes() == low.tobytes()
    ref = Reference(low, low, low + 1.0, mode)          # pred = low: never strictly better than b = low
    assert ref.sums[:, 5].tolist() == [0, 0] and ref.sums[:, 0].tolist() == [shape[0] * shape[1]] * 2
    assert np.array_equal(ref.sums[:, 1], ref.sums[:, 3]) and np.array_equal(ref.sums[:, 2], ref.sums[:, 4])


@pytest.mark.parametrize("mode,side", [("nearest", 1), ("bilinear", 2), ("bicubic", 4)])
def test_a_nan_tap_removes_its_whole_footprint(mode, side):
    """at ratio 4 an interior input pixel lies under side * 4 output rows and columns shifted by the half-pixel offset
    (nearest: 4; bilinear: 8; bicubic: 16), whatever its weight there; a corner's footprint is cut by the clamp, which makes
    several taps of a pixel the same input pixel"""
    rng = np.random.default_rng(5)
    (n_in, n_out) = (8, 32)
    low = rng.random((1, n_in, n_in))
    actual = rng.random((1, n_out, n_out))
    low[0, 4, 3] = np.nan
    ref = Reference(low, None, actual, mode)
    assert ref.sums[0, 0] == n_out * n_out - (4 * side) ** 2
    rows = np.where(~ref.counted[0].all(axis=1))[0]
    cols = np.where(~ref.counted[0].all(axis=0))[0]
    # input pixel j is tap of the outputs whose floor(src) lies in [j - side / 2, j + side / 2 - 1] (nearest: floor == j)
    first = {1: lambda j: 4 * j, 2: lambda j: 4 * j - 2, 4: lambda j: 4 * j - 6}[side]
    assert (rows[0], rows.size, cols[0], cols.size) == (first(4), 4 * side, first(3), 4 * side)
    assert np.isnan(ref.field[0][np.ix_(rows, cols)]).all() and np.isfinite(ref.field[0][ref.counted[0]]).all()
    assert (ref.sums[0, 3:] == 0).all()                 # no prediction
    # the corner: every output whose clamped taps reach input (0, 0)
    low = rng.random((1, n_in, n_in))
    low[0, 0, 0] = np.inf
    ref = Reference(low, actual, actual, mode)
    reach = {1: 4, 2: 6, 4: 10}[side]                   # nearest rows 0..3, bilinear floor(src) <= 0, bicubic floor(src) <= 1
    assert ref.sums[0, 0] == n_out * n_out - reach * reach
    assert not ref.counted[0, :reach, :reach].any()
    # a value of the target or of the prediction that is not finite takes its own pixel alone
    (p, a) = (actual.copy(), actual.copy())
    (p[0, 31, 31], a[0, 31, 0], a[0, 30, 0]) = (np.nan, -np.inf, np.inf)
    assert Reference(low, p, a, mode).sums[0, 0] == n_out * n_out - reach * reach - 3


def test_scores_and_summary_rules():
    sums = np.array([[100, 50, 40, 30, 10, 80], [10, 5, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0], [4, 2, 2, 4, 8, 1]], dtype=np.float64)
    s = baseline.scores_from_sums(sums)
    assert s["baseline_mae"][:2].tolist() == [0.5, 0.5] and s["baseline_mse"][:2].tolist() == [0.4, 0.0]
    assert s["model_mse"][[0, 1, 3]].tolist() == [0.1, 0.1, 2.0] and s["model_mae"][0] == 0.3
    assert s["skill"][0] == 1.0 - 10.0 / 40.0 and math.isnan(s["skill"][1]) and math.isnan(s["skill"][2]) and s["skill"][3] == -3.0
    assert s["win_fraction"][[0, 1, 3]].tolist() == [0.8, 0.0, 0.25] and math.isnan(s["win_fraction"][2])
    assert all(math.isnan(s[k][2]) for k in ("baseline_mae", "baseline_mse", "model_mae", "model_mse"))
    assert s["pixels"].dtype == np.int64 and s["pixels"].tolist() == [100, 10, 0, 4]
    rec = baseline.summary(sums, "bicubic", "lowres", (16, 16), (10, 10))
    assert (rec["mode"], rec["variable"], rec["in_shape"], rec["out_shape"]) == ("bicubic", "lowres", [16, 16], [10, 10])
    assert (rec["n_cases"], rec["n_counted"], rec["pixels_counted"], rec["pixels_left_out"]) == (4, 2, 114, 400 - 114)
    assert rec["pooled_skill"] == 1.0 - 19.0 / 42.0 and rec["baseline_mse"] == 42.0 / 114.0 and rec["baseline_mae"] == 57.0 / 114.0
    assert rec["model_mse"] == 19.0 / 114.0 and rec["win_fraction"] == 81.0 / 114.0
    assert rec["mean_skill"] == (0.75 - 3.0) / 2 and rec["median_skill"] == (0.75 - 3.0) / 2 and rec["skill_positive"] == 0.5
    assert rec["case_pixels"] == [100, 10, 0, 4] and rec["case_skill"][0] == 0.75 and math.isnan(rec["case_skill"][2])
    # an empty partition and one without a counted pixel: nothing has a denominator
    for empty in (np.zeros((0, 6)), np.zeros((3, 6))):
        rec = baseline.summary(empty, "nearest", "v", (2, 2), (4, 4))
        assert (rec["n_cases"], rec["n_counted"], rec["pixels_counted"]) == (empty.shape[0], 0, 0)
        assert rec["pixels_left_out"] == empty.shape[0] * 16
        for k in ("pooled_skill", "baseline_mse", "baseline_mae", "model_mse", "mean_skill", "median_skill", "skill_positive", "win_fraction"):
            assert math.isnan(rec[k]), k
    assert baseline.MODES == baseline_ref.MODES


def test_json_is_strict_and_the_line(tmp_path):
    sums = np.array([[100, 50, 40, 30, 10, 80], [10, 5, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0]], dtype=np.float64)
    rec = baseline.summary(sums, "bilinear", "lowres", (4, 4), (10, 10))
    path = baseline.write_json(str(tmp_path / "baseline_test.json"), rec)
    text = open(path).read()
    assert "NaN" not in text and "Infinity" not in text
    back = json.loads(text, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert back["case_skill"] == [0.75, None, None] and back["case_baseline_mse"] == [0.4, 0.0, None]
    assert back["pooled_skill"] == 1.0 - 11.0 / 40.0 and back["mean_skill"] == 0.75 and back["skill_positive"] == 1.0
    assert (back["mode"], back["variable"], back["n_cases"], back["n_counted"]) == ("bilinear", "lowres", 3, 1)
    assert baseline.line("test", rec) == ("baseline test: bilinear of lowres, pooled skill 0.725 (baseline mse 0.363636, "
                                          "model mse 0.1), 1/3 cases better")
    none = baseline.summary(np.zeros((1, 6)), "nearest", "v", (2, 2), (4, 4))
    assert baseline.line("train", none) == "baseline train: nearest of v, pooled skill none (baseline mse none, model mse none), 0/1 cases better"
    assert json.loads(open(baseline.write_json(str(tmp_path / "b.json"), none)).read())["pooled_skill"] is None


def test_cli_flags_are_evaluate_cae_plus_two():
    from cae_tools_amd.cli import baseline as cli, evaluate_cae
    flags = lambda parser: [(a.option_strings, a.dest, a.nargs, a.default, a.required, a.type)   # noqa: E731
                            for a in parser._actions if a.option_strings and a.dest != "help"]
    (mine, theirs) = (flags(cli.build_parser()), flags(evaluate_cae.build_parser()))
    assert mine[:len(theirs)] == theirs
    assert [f[0] for f in mine[len(theirs):]] == [["--baseline-variable"], ["--baseline-mode"]]
    args = cli.build_parser().parse_args(["--model-folder", "m"])
    assert (args.baseline_variable, args.baseline_mode) == (None, "bicubic")
    args = cli.build_parser().parse_args(["--model-folder", "m", "--baseline-mode", "nearest", "--baseline-variable", "t2m"])
    assert (args.baseline_variable, args.baseline_mode) == ("t2m", "nearest")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--model-folder", "m", "--baseline-mode", "lanczos"])


# sha256 of evaluation_report's page for the golden record, as test_ssim_cpu.py holds it
REPORT_SHA256 = "0a26c705f2bab559c1df1dee37ad957c941d84ce2aa0652d349c3549845789f1"


def test_report_section_is_off_by_default():
    with open(os.path.join(HERE, "golden", "report_layout.json")) as f:
        rec = json.load(f)["record"]
    rng = np.random.default_rng(7)
    measures = [(p, {m: rng.random(20) for m in rec["measures"]}) for p in rec["partitions"]]
    page = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"])
    assert hashlib.sha256(page.encode("utf-8")).hexdigest() == REPORT_SHA256
    assert page == report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], baseline=None)
    assert "Skill against interpolation" not in page
    sums = np.array([[100, 50, 40, 30, 10, 80], [10, 5, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0]], dtype=np.float64)
    record = baseline.summary(sums, "bicubic", "lowres", (4, 4), (10, 10))
    with_section = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], baseline=[("test", record)])
    assert with_section.count("Skill against interpolation") == 1
    assert "test: bicubic interpolation of lowres, 4 x 4 to 10 x 10, 1 of 3 cases" in with_section
    assert with_section.count('alt="test skill histogram"') == 1
    for cell in ("<td>pooled skill</td>", "<td>0.725</td>", "<td>baseline mse</td>", "<td>0.363636</td>",
                 "<td>pixels counted / left out</td>", "<td>110 / 190</td>"):
        assert cell in with_section, cell
    assert with_section.count("<img") == page.count("<img") + 1


def test_the_library_exports_the_baseline_entry_points():
    from cae_tools_amd import _lib
    lib = _lib.load()
    for name in ("cae_case_baseline", "cae_case_baseline_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    # one partial of six doubles per (case, 64-row band, 64-column strip)
    assert lib.cae_case_baseline_workspace_bytes(3, 65, 130) == 3 * 2 * 3 * 6 * 8
    assert lib.cae_case_baseline_workspace_bytes(1, 1, 1) == 48
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, (1 << 30) + 1, 4)):
        assert lib.cae_case_baseline_workspace_bytes(*bad) == 0
