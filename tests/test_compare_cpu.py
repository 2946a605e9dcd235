"""The host side of the model comparison without a GPU: the index generator and the sequential sums of the numpy restatement
(compare_ref.py) held to the definition's statistical properties, the package's units, ranks, statistics and record held to the
restatement and to hand-made tables, the flags and refusals of the command before any GPU call, and the CAE_ERR_ARG refusals of
cae_case_compare and cae_bootstrap_sums with made-up addresses that are never dereferenced."""
import ctypes as C
import json
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import compare_ref
from cae_tools_amd import _lib
from cae_tools_amd.cli import compare as cli
from cae_tools_amd.models import evaluation_analyses as analyses
from cae_tools_amd.utils import compare
from cae_tools_amd.utils.report import evaluation_report


# ---- the generator ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def drawn():
    return compare_ref.units(37, 4096, seed=0)


def test_the_draws_are_the_splitmix64_sequence():
    """draw (r, i) is output x + 1 of the sequential generator, x = (r << 32) | i: resample 0 reads outputs 1 .. n"""
    seq = compare_ref.splitmix64(7, 37)
    want = [((z >> 32) * 37) >> 32 for z in seq]
    assert compare_ref.units(37, 1, seed=7)[0].tolist() == want
    assert compare_ref.units(37, 3, seed=(1 << 64) - 1).max() < 37          # a seed at the top of the range wraps


def test_unit_counts_are_uniform(drawn):
    counts = np.bincount(drawn.reshape(-1), minlength=37)
    expected = drawn.size / 37.0
    chi2 = float(np.sum((counts - expected) ** 2 / expected))
    print(f"chi-square of the unit counts, 36 degrees of freedom: {chi2:.1f}")
    assert chi2 < 36 + 4 * math.sqrt(72)


def test_no_resample_is_drawn_twice(drawn):
    multisets = np.sort(drawn, axis=1)
    assert np.unique(multisets, axis=0).shape[0] == drawn.shape[0]
    distinct = np.mean([np.unique(row).size for row in drawn]) / 37.0
    print(f"distinct share {distinct:.3f}")
    assert 0.62 < distinct < 0.65                                           # 1 - (1 - 1/37)^37 = 0.637


def test_a_call_from_first_is_the_rows_of_the_call_from_zero(drawn):
    assert np.array_equal(compare_ref.units(37, 157, seed=0, first=100), drawn[100:257])
    table = np.random.default_rng(5).gamma(2, 1, (37, 3))
    whole = compare_ref.sums(table, 257, seed=0)
    assert np.array_equal(compare_ref.sums(table, 157, seed=0, first=100), whole[100:])


def test_spread_and_mean_of_the_resampled_sums():
    table = np.random.default_rng(5).gamma(2, 1, (37, 3))
    t = compare_ref.sums(table, 4096, seed=0)
    ratio = t.std(axis=0, ddof=1) / np.sqrt(37 * table.var(axis=0))
    print(f"spread of T over sqrt(n var(S)): {ratio}")
    assert (np.abs(ratio - 1.0) < 0.05).all()
    stderr = t.std(axis=0, ddof=1) / math.sqrt(4096)
    assert (np.abs(t.mean(axis=0) - table.sum(axis=0)) < 4 * stderr).all()
    # the same units for every column and for another table of the same n_unit: paired
    j = compare_ref.units(37, 4096, seed=0)
    assert np.allclose(t[:, 1], table[j, 1].sum(axis=1), rtol=1e-12)


# ---- ranks, units, statistics ------------------------------------------------------------------------------------------------

def test_interval_ranks_on_a_hand_made_table():
    c = Fraction(19, 20)
    assert compare.interval_ranks(1000, c) == (25, 976)
    assert compare.interval_ranks(999, c) == (25, 975)              # ceil(24.975)
    assert compare.interval_ranks(40, c) == (1, 40)
    assert compare.interval_ranks(41, c) == (2, 40)                 # ceil(1.025)
    assert compare.interval_ranks(10, Fraction(1, 2)) == (3, 8)     # ceil(2.5)
    assert compare.interval_ranks(1, c) == (1, 1)
    for (n, conf) in ((1000, c), (999, c), (7, Fraction(9, 10)), (123, Fraction(4, 5))):
        assert compare.interval_ranks(n, conf) == compare_ref.ranks(n, conf)
    values = np.arange(1000.0)[::-1].copy()
    stat = compare._stat(3.0, values, c)
    assert stat == {"value": 3.0, "interval": [24.0, 975.0], "degenerate": 0}


def test_too_few_resamples_are_refused():
    with pytest.raises(ValueError, match="too few resamples for this confidence"):
        compare.interval_ranks(0, Fraction(19, 20))
    assert compare.parse_confidence("0.95") == Fraction(19, 20) and compare.parse_confidence("9/10") == Fraction(9, 10)
    for bad in ("1", "0", "x", 0.95, "1.5"):
        with pytest.raises(ValueError, match="compare_confidence"):
            compare.parse_confidence(bad)


def test_degenerate_resamples_are_left_out_and_counted():
    values = np.array([1.0, math.nan, 3.0, math.inf, 2.0, -math.inf, 4.0])
    stat = compare._stat(2.5, values, Fraction(1, 2))
    assert stat["degenerate"] == 3 and stat["interval"] == [1.0, 4.0]       # 4 finite values: k = 1
    none = compare._stat(math.nan, np.array([math.nan, math.nan]), Fraction(1, 2))
    assert none["degenerate"] == 2 and all(math.isnan(v) for v in none["interval"])
    # a resample without a pixel has no mse: its statistic is NaN and is left out
    table = np.array([[4.0, 0.0, 1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    resampled = np.array([[8.0, 0.0, 2.0, 4.0, 6.0, 8.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [4.0, 0.0, 1.0, 2.0, 3.0, 4.0]])
    rec = compare.summary(table, resampled, ["p"], ["p"], Fraction(1, 2), 3, 0, n_cases=2, plane=4)
    assert rec["candidates"][0]["mse"] == {"value": 0.75, "interval": [0.75, 0.75], "degenerate": 1}
    assert rec["pixels_counted"] == 4 and rec["pixels_left_out"] == 4 and rec["competitors"] == []


def test_block_units():
    rows = np.arange(12.0).reshape(6, 2) + 0.1
    block = np.array([20, 10, 20, 30, 10, 20])
    (table, index) = compare.units(rows, block)
    assert index.tolist() == [0, 1, 0, 2, 1, 0]
    want = np.stack([(rows[0] + rows[2]) + rows[5], rows[1] + rows[4], rows[3]])
    assert np.array_equal(table, want) and np.array_equal(table, compare_ref.block_units(rows, block.tolist()))
    (plain, index) = compare.units(rows)
    assert np.array_equal(plain, rows) and index.tolist() == list(range(6))
    with pytest.raises(ValueError, match="one block value per case"):
        compare.units(rows, block[:5])
    assert np.array_equal(compare.column_sums(rows), ((((rows[0] + rows[1]) + rows[2]) + rows[3]) + rows[4]) + rows[5])


def _table(rng, n_unit, m, same=None):
    """a table of sums as cae_case_compare forms them: n, tied, then (S e, S|e|, S e^2, wins) per candidate"""
    table = np.zeros((n_unit, 2 + 4 * m))
    table[:, 0] = rng.integers(50, 100, n_unit)
    for k in range(m):
        table[:, 2 + 4 * k] = rng.normal(0, 1, n_unit)
        table[:, 3 + 4 * k] = rng.gamma(2, 1, n_unit) * (1 + k)
        table[:, 4 + 4 * k] = rng.gamma(2, 1, n_unit) * (1 + k)
        table[:, 5 + 4 * k] = np.floor(table[:, 0] / (m + 1))
    if same is not None:
        table[:, 2 + 4 * same:6 + 4 * same] = table[:, 2:6]
    table[:, 1] = table[:, 0] - table[:, 5::4].sum(axis=1)
    return table


def test_summary_against_the_restatement(tmp_path):
    rng = np.random.default_rng(3)
    table = _table(rng, 37, 3, same=1)
    table[:, 12] *= 4.0                                                     # the third candidate is clearly worse
    resampled = compare_ref.sums(table, 2000, seed=11)
    c = Fraction(19, 20)
    rec = compare.summary(table, resampled, ["model_output", "copy", "worse"], ["a", "b", "c"], c, 2000, 11, n_cases=37, plane=100,
                          block_variable=None)
    total = compare.column_sums(table)
    assert (rec["n_unit"], rec["n_cases"], rec["resamples"], rec["seed"], rec["confidence"]) == (37, 37, 2000, 11, "19/20")
    assert rec["pixels_counted"] == int(total[0]) and rec["pixels_left_out"] == 3700 - int(total[0])
    for k in range(3):
        cand = rec["candidates"][k]
        assert cand["mse"]["value"] == compare_ref.mse(total, k)
        (lo, hi, degenerate) = compare_ref.interval(compare_ref.mse(resampled, k), c)
        assert cand["mse"]["interval"] == [lo, hi] and cand["mse"]["degenerate"] == degenerate == 0
        assert cand["rmse"]["value"] == math.sqrt(cand["mse"]["value"]) and cand["mae"]["value"] == total[3 + 4 * k] / total[0]
        assert cand["bias"]["value"] == total[2 + 4 * k] / total[0] and cand["win_share"] == total[5 + 4 * k] / total[0]
        for key in compare.CANDIDATE_STATS:
            assert cand[key]["interval"][0] <= cand[key]["value"] <= cand[key]["interval"][1]
    (copy, worse) = rec["competitors"]
    assert copy["delta_mse"] == {"value": 0.0, "interval": [0.0, 0.0], "degenerate": 0} and not copy["significant"]
    assert copy["skill"]["value"] == 0.0 and copy["p_better"] == 0.0
    delta = compare_ref.mse(resampled, 2) - compare_ref.mse(resampled, 0)
    assert worse["delta_mse"]["value"] == compare_ref.mse(total, 2) - compare_ref.mse(total, 0)
    assert worse["delta_mse"]["interval"] == list(compare_ref.interval(delta, c)[:2])
    assert worse["significant"] and worse["p_better"] == float(np.mean(delta > 0)) and worse["skill"]["value"] > 0
    assert worse["skill"]["value"] == 1.0 - compare_ref.mse(total, 0) / compare_ref.mse(total, 2)
    assert worse["reference_win_share"] == rec["candidates"][0]["win_share"] and worse["tied_share"] == total[1] / total[0]
    # the writers
    path = compare.write_json(str(tmp_path / "compare_test.json"), dict(rec, extra=math.nan))
    with open(path) as f:
        stored = json.loads(f.read(), parse_constant=lambda name: pytest.fail(f"{name} is not strict JSON"))
    assert stored["extra"] is None and stored["candidates"][2]["mse"] == rec["candidates"][2]["mse"]
    text = compare.line("test", rec)
    assert text.startswith("compare test: 3 candidates, 37 units x 2000 resamples at 19/20: a mse ")
    assert "b delta 0 [0, 0] (not significant)" in text and "(significant)" in text
    svg = compare.svg_bars(rec, "mse")
    assert svg.count('class="candidate"') == 3 and svg.count('class="interval"') == 3
    rows = compare.section_rows(rec)
    assert len(rows) == 4 and all(len(r) == len(rows[0]) for r in rows) and rows[2][0] == "b" and rows[2][11] == "no"


def test_baseline_summary():
    rng = np.random.default_rng(8)
    table = np.stack([rng.integers(50, 100, 20).astype(float), rng.gamma(2, 1, 20), rng.gamma(2, 2, 20), rng.gamma(2, 1, 20),
                      rng.gamma(2, 1, 20), np.zeros(20)], axis=1)
    resampled = compare_ref.sums(table, 500, seed=2)
    base = compare.baseline_summary(table, resampled, Fraction(9, 10), "bicubic", "lowres")
    total = compare.column_sums(table)
    assert base["skill"]["value"] == 1.0 - total[4] / total[2] and base["label"] == "interpolation of lowres"
    assert base["skill"]["interval"] == list(compare_ref.interval(1.0 - resampled[:, 4] / resampled[:, 2], Fraction(9, 10))[:2])
    assert base["skill"]["interval"][0] <= base["skill"]["value"] <= base["skill"]["interval"][1]


# ---- the command and the evaluator -------------------------------------------------------------------------------------------

def test_cli_parser():
    parser = cli.build_parser()
    args = parser.parse_args(["--model-folder", "m", "--test-inputs", "scored.nc"])
    assert (args.compare_variables, args.compare_labels, args.compare_resamples, args.compare_seed) == ([], None, 10000, 0)
    assert (args.compare_confidence, args.compare_block_variable, args.compare_baseline) == ("0.95", None, None)
    assert args.test_inputs == ["scored.nc"] and args.output_html_folder == ""          # evaluate_cae's flags are all there
    args = parser.parse_args(["--model-folder", "m", "--compare-variables", "u", "v", "--compare-labels", "a", "b", "c",
                              "--compare-resamples", "1000000", "--compare-seed", "7", "--compare-confidence", "9/10",
                              "--compare-block-variable", "day", "--compare-baseline", "bilinear"])
    assert (args.compare_variables, args.compare_labels, args.compare_resamples, args.compare_seed) == (["u", "v"], ["a", "b", "c"], 10 ** 6, 7)
    assert (args.compare_confidence, args.compare_block_variable, args.compare_baseline) == ("9/10", "day", "bilinear")
    assert parser.parse_args(["--model-folder", "m", "--compare-variables"]).compare_variables == []
    for bad in (["--compare-resamples", "0"], ["--compare-resamples", "1000001"], ["--compare-resamples", "x"], ["--compare-seed", "-1"],
                ["--compare-confidence", "1"], ["--compare-confidence", "0"], ["--compare-confidence", "abc"],
                ["--compare-baseline", "cubic"], ["--compare-labels"]):
        with pytest.raises(SystemExit):
            parser.parse_args(["--model-folder", "m"] + bad)
    # refused by main before the model folder is looked at
    for bad in (["--compare-variables", "u", "u"], ["--compare-variables", "model_output"], ["--compare-variables", *"abcdefgh"],
                ["--compare-variables", "u", "--compare-labels", "only"], ["--compare-variables", "u", "--compare-labels", "a", "a"]):
        with pytest.raises(SystemExit):
            cli.main(["--model-folder", "no_such_model_folder", "--test-inputs", "scored.nc"] + bad)


def _ev(**changes):
    ev = SimpleNamespace(compare=True, model_output_variable="model_output", compare_variables=["other"], compare_labels=None,
                         compare_resamples=10000, compare_seed=0, compare_confidence="0.95", compare_block_variable=None,
                         compare_baseline=None, training_paths=[], testing_paths=[])
    for (k, v) in changes.items():
        setattr(ev, k, v)
    return ev


@pytest.mark.parametrize("changes, text", [
    (dict(compare_resamples=0), "compare_resamples must be an integer from 1 to 1000000, got 0"),
    (dict(compare_resamples=10 ** 6 + 1), "compare_resamples must be an integer from 1 to 1000000, got 1000001"),
    (dict(compare_resamples=2.5), "compare_resamples must be an integer from 1 to 1000000, got 2.5"),
    (dict(compare_seed=-1), "compare_seed must be an integer from 0 to 2^64 - 1, got -1"),
    (dict(compare_confidence="1.0"), "compare_confidence: coverage level '1.0' is not between 0 and 1"),
    (dict(compare_confidence=0.95), "compare_confidence: coverage level 0.95: give the decimal text or a Fraction, a float has already lost it"),
    (dict(compare_variables=list("abcdefgh")), "compare_variables: at most 7 variables beside the prediction expected, got 8"),
    (dict(compare_variables=["a", "a"]), "compare_variables: 'a' is named twice (the prediction variable is the first candidate)"),
    (dict(compare_labels=["x"]), "compare_labels: 2 labels expected, one per candidate with the prediction first, got 1"),
    (dict(compare_baseline="cubic"), "compare_baseline must be one of nearest, bilinear, bicubic, got 'cubic'"),
])
def test_refusals_before_the_model_is_loaded(changes, text):
    with pytest.raises(ValueError) as refused:
        analyses.COMPARE.check(_ev(**changes))
    assert str(refused.value) == text
    analyses.COMPARE.check(_ev(compare=False, **changes))       # switched off, nothing is looked at


def test_the_files_are_refused_before_the_model_is_loaded(tmp_path):
    """a missing variable, a shape mismatch and a block variable that is not per case: refused from the file alone"""
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    path = str(tmp_path / "scored.nc")
    field = np.zeros((4, 1, 6, 5), dtype=np.float32)
    netcdf3.write(path, {"n": 4, "c": 1, "y": 6, "x": 5, "y2": 3},
                  {"model_output": (("n", "c", "y", "x"), field, {}), "other": (("n", "c", "y", "x"), field, {}),
                   "small": (("n", "c", "y2", "x"), field[:, :, :3], {}), "day": (("n",), np.arange(4.0), {}),
                   "row": (("y",), np.arange(6.0), {})})
    analyses.COMPARE.check(_ev(testing_paths=[path], compare_block_variable="day"))
    assert analyses.COMPARE in analyses.ANALYSES and analyses.COMPARE.enabled(_ev()) and not analyses.COMPARE.enabled(_ev(compare=False))
    for (changes, text) in ((dict(compare_variables=["absent"]), "compare needs the variable 'absent' in the test data set"),
                            (dict(compare_variables=["small"]), "do not match"),
                            (dict(compare_variables=["day"]), "do not match"),
                            (dict(compare_block_variable="row"), "is not a variable of the test data set with one value per case"),
                            (dict(compare_block_variable="absent"), "is not a variable of the test data set with one value per case")):
        with pytest.raises(ValueError, match=text):
            analyses.COMPARE.check(_ev(testing_paths=[path], **changes))
        with pytest.raises(ValueError, match=text):         # the constructor refuses before it looks at the model folder
            ModelEvaluator([], [path], model_path="no_such_model_folder", compare=True,
                           **{"compare_variables": ["other"], **changes})
    with pytest.raises(SystemExit):
        cli.main(["--model-folder", "no_such_model_folder", "--test-inputs", path, "--compare-variables", "u", "u"])
    with pytest.raises(ValueError, match="compare needs the variable 'absent'"):
        cli.main(["--model-folder", "no_such_model_folder", "--test-inputs", path, "--compare-variables", "absent"])


def test_report_with_the_option_off_and_on():
    metrics = {"test": {"mse": 1.0, "mae": 0.5}}
    measures = [("test", {"mae": np.array([0.5, 0.25]), "mse": np.array([1.0, 0.5])})]
    plain = evaluation_report(metrics, measures)
    assert evaluation_report(metrics, measures, compare=None) == plain and "Model comparison" not in plain
    table = _table(np.random.default_rng(1), 12, 2)
    rec = compare.summary(table, compare_ref.sums(table, 200, seed=0), ["model_output", "other"], ["ours", "theirs"],
                          Fraction(19, 20), 200, 0, n_cases=12, plane=100)
    page = evaluation_report(metrics, measures, compare=[("test", rec)])
    assert page.count("<h2>Model comparison</h2>") == 1 and "test: 2 candidates on " in page
    assert page.count('alt="test mse by candidate"') == 1 and "theirs" in page
    start = page.index("<h2>Model comparison</h2>")
    assert plain.startswith(page[:start].rstrip())      # what comes before the section is the plain page's


# ---- the entry points' host side -------------------------------------------------------------------------------------------

def test_workspace_rule():
    size = _lib.load().cae_case_compare_workspace_bytes
    assert size(0, 64, 2) == 0 and size(3, 0, 2) == 0 and size(3, 64, 0) == 0 and size(3, 64, 9) == 0 and size(-1, 64, 1) == 0
    assert size(1, 1, 1) == 6 * 8 and size(3, 64, 2) == 3 * 10 * 8 and size(3, 65, 8) == 3 * 2 * 34 * 8
    assert size(9, 4099, 3) == 9 * 65 * 14 * 8 and size(1 << 40, 1 << 30, 1) == 0


no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal tables run without a GPU only: their addresses are made up")
(P0, P1, A, SUMS, WS, TABLE, OUT) = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000)
COMPARE_CALL = dict(ptrs=[P0, P1], pred_kind=2, strides=[80, 80], n_pred=2, actual=A, actual_kind=2, actual_stride=80, n_case=3, plane=70,
                    sums=SUMS, workspace=WS, workspace_bytes=1 << 20, stream=None)
COMPARE_TABLE = [
    ("bad argument", [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(n_pred=0), dict(n_pred=9), dict(n_case=-1),
                      dict(plane=-1)]),
    ("null list of predictions", [dict(ptrs=None), dict(strides=None)]),
    ("negative stride", [dict(strides=[80, -1]), dict(actual_stride=-80)]),
    ("null pointer", [dict(ptrs=[P0, None]), dict(actual=None), dict(sums=None)]),
    ("a case stride is shorter than the plane", [dict(strides=[69, 80]), dict(strides=[80, 69]), dict(actual_stride=69)]),
    ("an operand reaches 2^60 elements from its pointer", [dict(strides=[80, 1 << 59]), dict(actual_stride=1 << 59),
                                                          dict(n_case=1 << 31, plane=1 << 30, strides=[1 << 30, 1 << 30],
                                                               actual_stride=1 << 30)]),
    ("pointers must be aligned to their element size, the workspace to 16 bytes",
     [dict(ptrs=[P0, P1 + 4]), dict(actual=A + 4), dict(actual=A + 2, actual_kind=0), dict(sums=SUMS + 4), dict(workspace=WS + 8)]),
    ("needs a workspace of 480 bytes", [dict(workspace=None), dict(workspace_bytes=479)]),
]


def _compare_call(lib, args):
    n = len(args["ptrs"]) if args["ptrs"] is not None else 0
    ptrs = (C.c_void_p * n)(*args["ptrs"]) if args["ptrs"] is not None else None
    strides = (C.c_int64 * len(args["strides"]))(*args["strides"]) if args["strides"] is not None else None
    return lib.cae_case_compare(ptrs, args["pred_kind"], strides, args["n_pred"], args["actual"], args["actual_kind"], args["actual_stride"],
                                args["n_case"], args["plane"], args["sums"], args["workspace"], args["workspace_bytes"], args["stream"])


@no_gpu
@pytest.mark.parametrize("row", [(text, change) for (text, changes) in COMPARE_TABLE for change in changes],
                         ids=lambda r: r[0][:24] + ":" + ",".join(r[1]))
def test_case_compare_refusal(row):
    """the call is answered by the host, with CAE_ERR_ARG and this text"""
    (text, change) = row
    lib = _lib.load()
    assert _compare_call(lib, dict(COMPARE_CALL, **change)) == -1
    assert text in lib.cae_last_error().decode()


@no_gpu
def test_case_compare_empty_calls_succeed_on_the_host():
    lib = _lib.load()
    for change in (dict(n_case=0), dict(plane=0), dict(n_case=0, actual=None, sums=None, workspace=None, workspace_bytes=0)):
        assert _compare_call(lib, dict(COMPARE_CALL, **change)) == 0


BOOT_NAMES = "table n_unit n_col first n_resample seed out stream".split()
BOOT_CALL = dict(table=TABLE, n_unit=37, n_col=3, first=0, n_resample=100, seed=0, out=OUT, stream=None)
BOOT_TABLE = [
    ("bad argument", [dict(n_unit=0), dict(n_unit=(1 << 20) + 1), dict(n_col=0), dict(n_col=33), dict(first=-1), dict(n_resample=-1),
                      dict(first=(1 << 32) - 99), dict(first=1 << 32, n_resample=1), dict(n_resample=(1 << 32) + 1),
                      dict(first=1 << 62, n_resample=1 << 62)]),
    ("null pointer", [dict(table=None), dict(out=None)]),
    ("pointers must be 8-byte aligned", [dict(table=TABLE + 4), dict(out=OUT + 2)]),
]


@no_gpu
@pytest.mark.parametrize("row", [(text, change) for (text, changes) in BOOT_TABLE for change in changes],
                         ids=lambda r: r[0][:24] + ":" + ",".join(f"{k}={v}" for (k, v) in r[1].items()))
def test_bootstrap_sums_refusal(row):
    (text, change) = row
    lib = _lib.load()
    args = dict(BOOT_CALL, **change)
    assert lib.cae_bootstrap_sums(*[args[name] for name in BOOT_NAMES]) == -1
    assert text in lib.cae_last_error().decode()


@no_gpu
def test_bootstrap_sums_without_a_resample_succeeds_on_the_host():
    lib = _lib.load()
    args = dict(BOOT_CALL, n_resample=0, first=1 << 32, table=None, out=None)
    assert lib.cae_bootstrap_sums(*[args[name] for name in BOOT_NAMES]) == 0


def test_the_wrappers_refuse_before_the_gpu():
    from cae_tools_amd.case_ops import bootstrap_sums, case_compare
    for (table, b, kw, text) in ((np.zeros((0, 3)), 5, {}, "a table"), (np.zeros((3, 33)), 5, {}, "a table"), (np.zeros(3), 5, {}, "a table"),
                                 (np.zeros((3, 2)), -1, {}, "must lie within"), (np.zeros((3, 2)), 2, dict(first=(1 << 32) - 1), "must lie within"),
                                 (np.zeros((3, 2)), 2, dict(seed=-1), "seed must be")):
        with pytest.raises(ValueError, match=text):
            bootstrap_sums(table, b, **kw)
    assert bootstrap_sums(np.zeros((3, 2)), 0).shape == (0, 2)
    with pytest.raises(ValueError, match="1 to 8 predictions expected"):
        case_compare([], np.zeros((2, 1, 3, 3)))
    with pytest.raises(ValueError, match="1 to 8 predictions expected"):
        case_compare([np.zeros((2, 1, 3, 3))] * 9, np.zeros((2, 1, 3, 3)))
