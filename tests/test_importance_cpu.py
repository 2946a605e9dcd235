"""The host side of permutation importance without a GPU: the permutations against the restated rule (importance_ref.py), the
groups and their refusals, utils/importance.summary on hand-made sums against hand-worked values, strict JSON, the line, the
chart, the command-line parser, the evaluator's refusals with their exact messages, the report with the option off, and what
the host side of cae_normalise_pack_gather and cae_case_importance refuses.

The refusal tables follow test_joint_hist_refusals_cpu.py: the addresses are made-up integers that no call here dereferences,
every row is answered by the host before a launch, and the rows are skipped where a GPU is present (test_importance_gpu.py
covers the refusals with real buffers there)."""
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import importance_ref
from cae_tools_amd import _lib
from cae_tools_amd.cli import importance as cli
from cae_tools_amd.models import evaluation_analyses as analyses
from cae_tools_amd.utils import importance
from cae_tools_amd.utils.report import evaluation_report


# ---- permutations --------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 257])
def test_every_row_is_one_cycle(n):
    p = importance.permutations(n, 5, 11)
    assert p.shape == (5, n) and p.dtype == np.int32
    for row in p:
        assert sorted(row.tolist()) == list(range(n))
        assert importance_ref.is_single_cycle(row)
        assert (row != np.arange(n)).all()                 # no case keeps its own values
    assert np.array_equal(p, importance_ref.sattolo(n, 5, 11))      # the rule, restated
    assert np.array_equal(p, importance.permutations(n, 5, 11))     # reproducible
    assert np.array_equal(p[:2], importance.permutations(n, 2, 11))     # a repeat does not depend on how many there are


def test_permutations_differ_across_repeats_and_seeds():
    p = importance.permutations(257, 3, 0)
    q = importance.permutations(257, 3, 1)
    assert len({row.tobytes() for row in p}) == 3
    assert all(a.tobytes() != b.tobytes() for (a, b) in zip(p, q))
    assert importance.permutations(2, 3, 5).tolist() == [[1, 0]] * 3       # two cases have one cycle
    with pytest.raises(ValueError, match="at least 2 cases expected, got 1"):
        importance.permutations(1, 1, 0)
    with pytest.raises(ValueError, match="at least 1 repeat expected, got 0"):
        importance.permutations(4, 0, 0)


# ---- groups ----------------------------------------------------------------------------------------

NAMES = ["lowres", "albedo", "elevation"]


def test_parse_groups():
    assert importance.parse_groups(None) is None
    assert importance.parse_groups(None, NAMES) == [["lowres"], ["albedo"], ["elevation"]]
    assert importance.parse_groups(["albedo,elevation", "lowres"], NAMES) == [["albedo", "elevation"], ["lowres"]]
    assert importance.parse_groups([" albedo , elevation "]) == [["albedo", "elevation"]]
    assert importance.check_groups(["albedo", ("lowres", "elevation")], NAMES) == [["albedo"], ["lowres", "elevation"]]
    assert importance.group_name(["albedo", "elevation"]) == "albedo+elevation"


@pytest.mark.parametrize("arguments, text", [
    ([], "importance_groups: at least one group expected"),
    (["albedo,,lowres"], "importance_groups: a group must name at least one input variable, got 'albedo,,lowres'"),
    ([""], "importance_groups: a group must name at least one input variable, got ''"),
    (["albedo,lowres,albedo"], "importance_groups: 'albedo' is named twice in the group 'albedo,lowres,albedo'"),
    (["albedo,skin"], "importance_groups: 'skin' is not an input variable of the model (lowres, albedo, elevation)"),
])
def test_parse_groups_refusals(arguments, text):
    with pytest.raises(ValueError) as refused:
        importance.parse_groups(arguments, NAMES)
    assert str(refused.value) == text


# ---- summary ---------------------------------------------------------------------------------------

def _sums():
    """three groups, two repeats, two cases of four pixels; group "b" is the unperturbed model; group "c" has no pair"""
    s = np.zeros((3, 2, 2, 8))
    #                n  Se1^2 Se0^2 S|e1| S|e0| SdP^2 grew shrank
    s[0, 0, 0] = [4, 16.0, 4.0, 8.0, 4.0, 4.0, 3, 1]
    s[0, 0, 1] = [4, 8.0, 12.0, 4.0, 6.0, 12.0, 1, 3]
    s[0, 1, 0] = [4, 36.0, 4.0, 12.0, 4.0, 16.0, 4, 0]
    s[0, 1, 1] = [2, 12.0, 12.0, 4.0, 6.0, 8.0, 1, 1]
    for r in range(2):
        s[1, r, 0] = [4, 4.0, 4.0, 4.0, 4.0, 0.0, 0, 0]
        s[1, r, 1] = [4, 12.0, 12.0, 6.0, 6.0, 0.0, 0, 0]
    return s


def test_summary_against_hand_worked_values():
    rec = importance.summary([["a"], ["b"], ["c", "d"]], _sums(), seed=3)
    assert (rec["n_cases"], rec["repeats"], rec["seed"], rec["n_groups"]) == (2, 2, 3, 3)
    (a, b, c) = rec["groups"]
    # a, repeat 0: 24 / 8 and 16 / 8; repeat 1: 48 / 6 and 16 / 6
    assert a["mse_permuted"] == [3.0, 8.0] and a["mse_base"] == [2.0, 16.0 / 6.0]
    assert a["mean_mse_permuted"] == 5.5 and a["mean_mse_base"] == (2.0 + 16.0 / 6.0) / 2
    d = [1.0, 8.0 - 16.0 / 6.0]
    assert a["importance"] == (d[0] + d[1]) / 2
    assert a["importance_sd"] == pytest.approx(abs(d[1] - d[0]) / math.sqrt(2.0), rel=1e-15)
    assert a["ratio"] == 5.5 / ((2.0 + 16.0 / 6.0) / 2)
    assert a["mae_permuted"] == [1.5, 16.0 / 6.0] and a["mae_base"] == [1.25, 10.0 / 6.0]
    assert a["mae_importance"] == ((1.5 - 1.25) + (16.0 / 6.0 - 10.0 / 6.0)) / 2
    assert a["pairs"] == 14 and a["sensitivity"] == math.sqrt(40.0 / 14.0)
    assert a["cases_grew"] == 2 / 4                 # (0, 0) and (1, 0) grew; (0, 1) shrank; (1, 1) stayed
    assert a["pixels_grew"] == 9 / 14 and a["pixels_shrank"] == 5 / 14
    assert (a["pixels_grew_count"], a["pixels_shrank_count"]) == (9, 5)
    assert a["case_delta_mse"] == [((16.0 - 4.0) / 4 + (36.0 - 4.0) / 4) / 2, ((8.0 - 12.0) / 4 + 0.0) / 2]
    # b: nothing moved
    assert b["importance"] == 0.0 and b["importance_sd"] == 0.0 and b["ratio"] == 1.0 and b["sensitivity"] == 0.0
    assert b["cases_grew"] == 0.0 and b["pixels_grew"] == 0.0 and b["case_delta_mse"] == [0.0, 0.0]
    # c: no pair, so no quotient has a value
    assert c["name"] == "c+d" and c["variables"] == ["c", "d"] and c["pairs"] == 0
    for key in ("importance", "importance_sd", "ratio", "mean_mse_base", "sensitivity", "cases_grew", "pixels_grew", "mae_importance"):
        assert math.isnan(c[key]), key
    assert all(math.isnan(v) for v in c["mse_base"] + c["case_delta_mse"])
    assert [g["rank"] for g in rec["groups"]] == [1, 2, 3] and rec["order"] == ["a", "b", "c+d"]
    assert rec["mse_base"] == a["mean_mse_base"]
    # the rank follows the importance, a group without a value last
    swapped = importance.summary([["c"], ["b"], ["a"]], _sums()[::-1])
    assert swapped["order"] == ["a", "b", "c"] and [g["rank"] for g in swapped["groups"]] == [3, 2, 1]


def test_one_repeat_has_no_spread_and_json_is_strict(tmp_path):
    rec = importance.summary([["a"], ["c"]], _sums()[[0, 2], :1], maps=np.zeros((2, 3, 2, 2)))
    assert rec["repeats"] == 1 and math.isnan(rec["groups"][0]["importance_sd"]) and rec["groups"][0]["importance"] == 1.0
    path = importance.write_json(str(tmp_path / "importance_test.json"), rec)
    with open(path) as f:
        text = f.read()
    assert "NaN" not in text and "Infinity" not in text
    back = json.loads(text, parse_constant=lambda token: pytest.fail(f"{token} in strict JSON"))
    assert "maps" not in back
    assert back["groups"][0]["importance_sd"] is None and back["groups"][0]["importance"] == 1.0
    assert back["groups"][1]["importance"] is None and back["groups"][1]["mse_base"] == [None]
    assert back["groups"][1]["case_delta_mse"] == [None, None] and back["groups"][1]["pairs"] == 0
    assert importance.line("test", rec) == "importance test: 2 groups x 1 permutations of 2 cases, base mse 2: a +1 (x1.5), c none (xnone)"
    rows = importance.section_rows(rec)
    assert rows[0][:3] == ["Rank", "Group", "base mse"] and [r[1] for r in rows[1:]] == ["a", "c"]
    assert rows[1][2:6] == ["2", "3", "1", "none"]
    assert importance.heading(rec) == "2 groups, 1 permutation of 2 cases, seed 0"


def test_line_and_chart():
    rec = importance.summary([["a"], ["b"], ["c", "d"]], _sums())
    (a, b) = rec["groups"][:2]
    assert importance.line("train", rec) == (f"importance train: 3 groups x 2 permutations of 2 cases, base mse {a['mean_mse_base']:.6g}: "
                                             f"a {a['importance']:+.6g} (x{a['ratio']:.6g}), b +0 (x1), c+d none (xnone)")
    svg = importance.svg_bars(rec, "importance +- sd")
    assert svg.count('class="group"') == 2 and svg.count('class="spread"') == 1 and svg.count('class="zero"') == 1
    assert f'data-name="a" data-importance="{a["importance"]:.6g}" data-sd="{a["importance_sd"]:.6g}"' in svg
    assert svg.index('data-name="a"') < svg.index('data-name="b"')
    empty = importance.svg_bars(importance.summary([["c"]], _sums()[2:]), "t")
    assert 'class="group"' not in empty and empty.startswith("<svg")


def test_delta_maps():
    maps = np.zeros((1, 3, 1, 3))
    maps[0, :, 0, 0] = [4, 10.0, 6.0]
    maps[0, :, 0, 1] = [2, 1.0, 4.0]
    delta = importance.delta_maps({"maps": maps})
    assert delta.shape == (1, 1, 3) and delta[0, 0, 0] == 1.0 and delta[0, 0, 1] == -1.5 and math.isnan(delta[0, 0, 2])


# ---- the command line ------------------------------------------------------------------------------

def test_cli_parser():
    parser = cli.build_parser()
    args = parser.parse_args(["--model-folder", "m"])
    assert (args.importance_repeats, args.importance_seed, args.importance_groups, args.importance_maps) == (5, 0, None, False)
    args = parser.parse_args(["--model-folder", "m", "--test-inputs", "scored.nc", "--importance-repeats", "64", "--importance-seed", "9",
                              "--importance-groups", "lowres", "albedo,elevation", "--importance-maps"])
    assert (args.importance_repeats, args.importance_seed, args.importance_maps) == (64, 9, True)
    assert importance.parse_groups(args.importance_groups) == [["lowres"], ["albedo", "elevation"]]
    assert args.test_inputs == ["scored.nc"] and args.output_html_folder == ""      # evaluate_cae's flags are all there
    for bad in (["--importance-repeats", "0"], ["--importance-repeats", "65"], ["--importance-seed", "-1"], ["--importance-groups"]):
        with pytest.raises(SystemExit):
            parser.parse_args(["--model-folder", "m"] + bad)
    with pytest.raises(SystemExit):
        cli.main(["--model-folder", "m", "--importance-groups", "a,a"])


# ---- the evaluator's refusals ----------------------------------------------------------------------

def _ev(**changes):
    """what the analysis' checks read of an evaluator"""
    data = {"one": {"lowres": SimpleNamespace(shape=(1, 1, 4, 4)), "albedo": SimpleNamespace(shape=(1, 1, 4, 4))},
            "no_albedo": {"lowres": SimpleNamespace(shape=(5, 1, 4, 4))},
            "fine": {"lowres": SimpleNamespace(shape=(2, 1, 4, 4)), "albedo": SimpleNamespace(shape=(2, 1, 4, 4))}}
    ev = SimpleNamespace(importance=True, importance_repeats=5, importance_seed=0, importance_groups=None, importance_maps=False,
                         model_input_variables=["lowres", "albedo"], model_path="model", testing_paths=["fine"], training_paths=[])
    ev._open = lambda paths: data[paths[0]] if paths else None
    for (k, v) in changes.items():
        setattr(ev, k, v)
    return ev


@pytest.mark.parametrize("changes, text", [
    (dict(importance_repeats=0), "importance_repeats must be an integer from 1 to 64, got 0"),
    (dict(importance_repeats=65), "importance_repeats must be an integer from 1 to 64, got 65"),
    (dict(importance_repeats=2.5), "importance_repeats must be an integer from 1 to 64, got 2.5"),
    (dict(importance_seed=-1), "importance_seed must be an integer, 0 or more, got -1"),
    (dict(importance_groups=[["lowres", "lowres"]]), "importance_groups: 'lowres' is named twice in the group 'lowres,lowres'"),
    (dict(importance_groups=[]), "importance_groups: at least one group expected"),
])
def test_refusals_before_the_model_is_loaded(changes, text):
    with pytest.raises(ValueError) as refused:
        analyses.IMPORTANCE.check(_ev(**changes))
    assert str(refused.value) == text
    analyses.IMPORTANCE.check(_ev(importance=False, **changes))        # switched off, nothing is looked at


@pytest.mark.parametrize("changes, text", [
    (dict(importance_groups=[["lowres"], ["skin"]]), "importance_groups: 'skin' is not an input variable of the model (lowres, albedo)"),
    (dict(testing_paths=["one"]), "importance needs at least 2 cases to permute, the test data set has 1"),
    (dict(training_paths=["one"]), "importance needs at least 2 cases to permute, the train data set has 1"),
    (dict(testing_paths=["no_albedo"]),
     "importance needs the model's input variables in the test data set: albedo of model is not there"),
])
def test_refusals_once_the_model_is_known(changes, text):
    with pytest.raises(ValueError) as refused:
        analyses.check_importance_model(_ev(**changes))
    assert str(refused.value) == text
    analyses.check_importance_model(_ev(importance=False, **changes))


def test_the_checks_pass_what_is_right_and_the_constructor_refuses_first():
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    ev = _ev(importance_groups=[["albedo", "lowres"]], importance_repeats=64, training_paths=["fine"])
    analyses.IMPORTANCE.check(ev)
    analyses.check_importance_model(ev)
    assert analyses.ANALYSES[-1] is analyses.IMPORTANCE and analyses.IMPORTANCE.enabled(ev)
    with pytest.raises(ValueError, match="importance_repeats must be an integer from 1 to 64, got 0"):
        ModelEvaluator([], ["scored.nc"], model_path="no_such_model_folder", importance=True, importance_repeats=0)


# ---- the report ------------------------------------------------------------------------------------

def test_report_with_the_option_off_and_on():
    metrics = {"test": {"mse": 1.0, "mae": 0.5}}
    measures = [("test", {"mae": np.array([0.5, 0.25]), "mse": np.array([1.0, 0.5])})]
    plain = evaluation_report(metrics, measures)
    assert evaluation_report(metrics, measures, importance=None) == plain
    assert "Input importance" not in plain
    rec = importance.summary([["a"], ["b"], ["c", "d"]], _sums())
    page = evaluation_report(metrics, measures, importance=([("test", rec)], "importance/index.html"))
    assert page.count("<h2>Input importance</h2>") == 1 and "test: 3 groups, 2 permutations of 2 cases, seed 0" in page
    assert page.count('alt="test input importance"') == 1 and 'href="importance/index.html"' in page
    assert f"<td>{rec['groups'][0]['importance']:.6g}</td>" in page
    no_link = evaluation_report(metrics, measures, importance=([("test", rec)], None))
    assert "importance/index.html" not in no_link and "<h2>Input importance</h2>" in no_link
    start = page.index("<h2>Input importance</h2>")
    assert plain.startswith(page[:start].rstrip())      # what comes before the section is the plain page's


# ---- what the two entry points refuse --------------------------------------------------------------

no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal table runs without a GPU only: its addresses are made up")
(OK, ARG) = (0, -1)
(B, Q, A, SUMS, MAP, WS, SRC, DST, ROW) = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000)
BIG = 1 << 59       # as a case stride of 3 cases: 2 * 2^59 + plane elements from the pointer, above 2^60

I_NAMES = "base base_stride pert pert_stride actual actual_kind actual_stride n_case plane vmin range sums map workspace workspace_bytes stream".split()
I_CALL = dict(base=B, base_stride=70, pert=Q, pert_stride=72, actual=A, actual_kind=2, actual_stride=75, n_case=3, plane=70, vmin=288.0,
              range=10.0, sums=SUMS, map=MAP, workspace=WS, workspace_bytes=384, stream=None)
NOTHING = dict(base=None, pert=None, actual=None, sums=None, map=None, workspace=None, workspace_bytes=0)
I_TABLE = [
    (ARG, "cae_case_importance: bad argument (a CAE_ELEM_* kind, n_case >= 0, plane >= 0)",
     [dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1), dict(plane=-1)]),
    (ARG, "cae_case_importance: negative stride", [dict(base_stride=-1), dict(pert_stride=-1), dict(actual_stride=-1)]),
    (ARG, "cae_case_importance: vmin and range must be finite",
     [dict(vmin=math.nan), dict(vmin=math.inf), dict(range=math.nan), dict(range=-math.inf)]),
    (OK, "", [dict(n_case=0, **NOTHING), dict(plane=0, **NOTHING), dict(n_case=0, plane=0, **NOTHING)]),
    (ARG, "cae_case_importance: null pointer", [dict(base=None), dict(pert=None), dict(actual=None), dict(sums=None)]),
    (ARG, "cae_case_importance: a case stride is shorter than the plane",
     [dict(base_stride=69), dict(pert_stride=69), dict(actual_stride=69)]),
    (ARG, "cae_case_importance: an operand reaches 2^60 elements from its pointer",
     [dict(base_stride=BIG), dict(pert_stride=BIG), dict(actual_stride=BIG),
      dict(n_case=1 << 31, plane=1 << 30, base_stride=1 << 30, pert_stride=1 << 30, actual_stride=1 << 30)]),
    (ARG, "cae_case_importance: pointers must be aligned to their element size, the workspace to 16 bytes",
     [dict(base=B + 2), dict(pert=Q + 1), dict(actual=A + 4), dict(sums=SUMS + 4), dict(map=MAP + 4), dict(workspace=WS + 8)]),
    (ARG, "cae_case_importance: needs a workspace of 384 bytes (cae_case_importance_workspace_bytes)",
     [dict(workspace=None), dict(workspace_bytes=383), dict(workspace_bytes=0)]),
]

G_NAMES = "src n_src c_src hw dst n_dst c_dst c_off vmin range enable rows stream".split()
G_CALL = dict(src=SRC, n_src=5, c_src=2, hw=35, dst=DST, n_dst=7, c_dst=4, c_off=1, vmin=1.0, range=2.0, enable=1, rows=ROW, stream=None)
G_TABLE = [
    (ARG, "cae_normalise_pack_gather: bad argument (n_src >= 0, n_dst >= 0, c_src >= 1, hw >= 0, 0 <= c_off <= c_dst - c_src)",
     [dict(n_src=-1), dict(n_dst=-1), dict(c_src=0), dict(hw=-1), dict(c_off=-1), dict(c_off=3), dict(c_dst=1, c_off=0)]),
    (ARG, "cae_normalise_pack_gather: more than 2^31 - 1 rows", [dict(n_src=1 << 31), dict(n_dst=1 << 31)]),
    (OK, "", [dict(n_dst=0, src=None, dst=None, rows=None), dict(hw=0, src=None, dst=None, rows=None)]),
    (ARG, "cae_normalise_pack_gather: null pointer", [dict(src=None), dict(dst=None), dict(rows=None)]),
    (ARG, "cae_normalise_pack_gather: an operand reaches 2^60 elements from its pointer",
     [dict(n_src=1 << 30, hw=1 << 30), dict(n_dst=1 << 30, hw=1 << 29)]),
    (ARG, "cae_normalise_pack_gather: pointers must be 4-byte aligned", [dict(src=SRC + 2), dict(dst=DST + 1), dict(rows=ROW + 2)]),
]


def _rows(table):
    return [(rc, text, change) for (rc, text, changes) in table for change in changes]


def _row_id(row):
    return ",".join(f"{k}={v}" for (k, v) in row[2].items())


def test_the_rows_are_distinct_and_the_call_needs_that_workspace():
    for (table, call, names) in ((I_TABLE, I_CALL, I_NAMES), (G_TABLE, G_CALL, G_NAMES)):
        rows = _rows(table)
        assert len(set(map(_row_id, rows))) == len(rows)
        assert list(call) == names
    lib = _lib.load()
    assert lib.cae_case_importance_workspace_bytes(3, 70) == 384        # 3 cases x 2 tiles of 64 pixels x 8 doubles
    assert lib.cae_case_importance_workspace_bytes(1, 64) == 64 and lib.cae_case_importance_workspace_bytes(1, 65) == 128
    assert lib.cae_case_importance_workspace_bytes(0, 70) == 0 and lib.cae_case_importance_workspace_bytes(3, 0) == 0


def _refusal(fn, names, call, row):
    (rc, text, change) = row
    lib = _lib.load()
    args = dict(call, **change)
    assert set(change) <= set(call)
    got = getattr(lib, fn)(*(args[n] for n in names))
    message = lib.cae_last_error().decode() if got != OK else ""
    print(f"{_row_id(row)}: {got} {message!r}")
    assert (got, message) == (rc, text)


@no_gpu
@pytest.mark.parametrize("row", _rows(I_TABLE), ids=_row_id)
def test_case_importance_refusal(row):
    """the call is answered by the host, with this code and this text"""
    _refusal("cae_case_importance", I_NAMES, I_CALL, row)


@no_gpu
@pytest.mark.parametrize("row", _rows(G_TABLE), ids=_row_id)
def test_pack_gather_refusal(row):
    _refusal("cae_normalise_pack_gather", G_NAMES, G_CALL, row)
