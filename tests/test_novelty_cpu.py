"""The host side of the novelty analysis without a GPU: utils/novelty.summary on hand-made per-case arrays against hand-worked
quintiles, order statistics and Spearman's rank correlation with ties, what has no value, strict JSON, the line and the chart,
the parsers of cli.novelty and apply_cae with their refusals, the evaluator's refusal without a reference set, the report
with the option off and on, the workspace rule of cae_case_neighbours and what its host side refuses (made-up addresses that
no call dereferences, run where there is no GPU; test_neighbours_gpu.py covers the refusals with real buffers)."""
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cae_tools_amd import _lib
from cae_tools_amd.cli import apply_cae
from cae_tools_amd.cli import novelty as cli
from cae_tools_amd.models import evaluation_analyses as analyses
from cae_tools_amd.utils import novelty
from cae_tools_amd.utils.report import evaluation_report


def _case(values, k=2, features=4, nearest=None, refs=20):
    """a case record whose novelty is `values` (NaN: an invalid case): dist2[:, k - 1] = features * v^2"""
    v = np.asarray(values, dtype=np.float64)
    n = v.size
    dist2 = np.full((n, k), np.inf)
    dist2[:, k - 1] = np.where(np.isnan(v), np.inf, features * v * v)
    dist2[:, 0] = np.where(np.isnan(v), np.inf, features * (v / 2) ** 2)
    index = np.tile(np.arange(k, dtype=np.int32), (n, 1)) if nearest is None else np.asarray(nearest, dtype=np.int32)
    index = np.where(np.isnan(v)[:, None], -1, index).astype(np.int32)
    count = np.where(np.isnan(v), -1, k).astype(np.int32)
    return novelty.case_record(dist2, index, count, features, refs, refs)


def test_case_record():
    dist2 = np.array([[0.0, 16.0], [4.0, np.inf], [np.inf, np.inf]])
    index = np.array([[3, 1], [2, -1], [-1, -1]], dtype=np.int32)
    rec = novelty.case_record(dist2, index, np.array([2, 1, -1], dtype=np.int32), 4, 9, 8)
    assert rec["novelty"][0] == 2.0 and rec["novelty"][1] == math.inf and math.isnan(rec["novelty"][2])
    assert rec["nearest"][0] == 0.0 and rec["nearest"][1] == 1.0 and math.isnan(rec["nearest"][2])
    assert rec["nearest_case"].tolist() == [3, 2, -1] and rec["nearest_case"].dtype == np.int32
    assert (rec["k"], rec["features"], rec["reference_cases"], rec["valid_reference_cases"]) == (2, 4, 9, 8)


def test_summary_against_hand_worked_values():
    # eleven cases, case 4 invalid; the valid ones in ascending novelty are 9, 0, 7, 2, 5, 1, 10, 3, 8, 6
    values = [0.25, 0.75, 0.5, 1.0, math.nan, 0.625, 2.0, 0.375, 1.5, 0.125, 0.875]
    mse = np.array([2.0, 6.0, 4.0, 8.0, 100.0, 5.0, 20.0, 3.0, 12.0, 1.0, 7.0])
    mae = mse / 2
    reference = _case(np.arange(1, 21) / 16.0)          # 20 leave-one-out values 1/16 .. 20/16
    rec = novelty.summary(_case(values), reference=reference, mse=mse, mae=mae)
    assert (rec["n_cases"], rec["valid_cases"], rec["k"], rec["features"]) == (11, 10, 2, 4)
    assert (rec["novelty_min"], rec["novelty_median"], rec["novelty_max"]) == (0.125, 0.6875, 2.0)
    # ranks ceil(20 p / 100) = 10, 18, 19, 20
    assert rec["reference"] == {"n": 20, "p50": 10 / 16, "p90": 18 / 16, "p95": 19 / 16, "p99": 20 / 16}
    assert rec["outside_95"] == 0.2 and rec["outside_99"] == 0.2       # 1.5 and 2.0 of ten valid cases
    bins = rec["quintiles"]
    assert [b["cases"] for b in bins] == [2, 2, 2, 2, 2]
    assert [b["mse"] for b in bins] == [1.5, 3.5, 5.5, 7.5, 16.0] and [b["mae"] for b in bins] == [0.75, 1.75, 2.75, 3.75, 8.0]
    assert (bins[0]["novelty_lo"], bins[0]["novelty_hi"], bins[4]["novelty_lo"], bins[4]["novelty_hi"]) == (0.125, 0.25, 1.5, 2.0)
    assert rec["top_bottom_mse_ratio"] == 16.0 / 1.5
    assert rec["spearman_mse"] == pytest.approx(1.0, abs=1e-15)         # the mse ascends with the novelty, the invalid case is left out
    assert [m["case"] for m in rec["most_novel"]] == [6, 8, 3, 10, 1, 5, 2, 7, 0, 9]
    assert rec["most_novel"][0] == {"case": 6, "novelty": 2.0, "nearest": 1.0, "nearest_case": 0}
    assert math.isnan(rec["case_novelty"][4]) and rec["case_nearest_case"][4] == -1


def test_quintiles_of_few_cases_and_ties_go_by_case_index():
    rec = novelty.summary(_case([0.5, 0.5, 0.5]), mse=np.array([1.0, 2.0, 4.0]), mae=np.array([1.0, 1.0, 1.0]))
    # ranks 0, 1, 2 of m = 3: bins floor(5 r / 3) = 0, 1, 3; bins 2 and 4 are empty
    assert [b["cases"] for b in rec["quintiles"]] == [1, 1, 0, 1, 0]
    assert [b["mse"] for b in rec["quintiles"][:2]] == [1.0, 2.0] and rec["quintiles"][3]["mse"] == 4.0
    assert math.isnan(rec["quintiles"][2]["mse"]) and math.isnan(rec["top_bottom_mse_ratio"])
    assert [m["case"] for m in rec["most_novel"]] == [0, 1, 2]
    assert math.isnan(rec["spearman_mse"])                              # zero rank variance
    assert rec["reference"]["n"] == 0 and math.isnan(rec["reference"]["p95"]) and math.isnan(rec["outside_95"])


def test_spearman_with_ties_and_without_enough_pairs():
    # ranks 1, 2.5, 2.5, 4 against 1, 4, 2.5, 2.5: S da db = 2.25, S da^2 = S db^2 = 4.5
    assert novelty.spearman([1.0, 2.0, 2.0, 3.0], [1.0, 3.0, 2.0, 2.0]) == pytest.approx(0.5, abs=1e-15)
    assert novelty.average_ranks([3.0, 1.0, 3.0, 3.0]).tolist() == [3.0, 1.0, 3.0, 3.0]
    assert novelty.spearman([1.0, 2.0, 3.0], [3.0, 2.0, 1.0]) == pytest.approx(-1.0, abs=1e-15)
    assert math.isnan(novelty.spearman([1.0, 2.0], [1.0, 2.0]))
    assert math.isnan(novelty.spearman([1.0, 2.0, math.nan, math.inf], [1.0, 2.0, 3.0, 4.0]))     # two pairs where both are finite
    assert math.isnan(novelty.spearman([1.0, 2.0, 3.0], [5.0, 5.0, 5.0]))


def test_order_statistic():
    v = np.sort(np.array([5.0, 1.0, 3.0]))
    assert [novelty.order_statistic(v, p) for p in (1, 33, 34, 50, 67, 99, 100)] == [1.0, 1.0, 3.0, 3.0, 5.0, 5.0, 5.0]
    assert math.isnan(novelty.order_statistic(np.zeros(0), 50))


def test_json_is_strict_and_the_line_and_chart(tmp_path):
    case = _case([0.5, math.inf, math.nan, 0.25], nearest=[[2, 3], [1, -1], [0, 0], [5, 6]])
    rec = novelty.summary(case, reference=_case([0.125, 0.25]), mse=np.array([1.0, math.nan, 2.0, 3.0]), mae=np.array([1.0, 2.0, 2.0, 3.0]))
    path = novelty.write_json(str(tmp_path / "novelty_test.json"), rec)
    with open(path) as f:
        text = f.read()
    assert "NaN" not in text and "Infinity" not in text
    got = json.loads(text)
    assert got["case_novelty"] == [0.5, None, None, 0.25] and got["novelty_max"] is None and got["case_nearest_case"] == [2, 1, -1, 5]
    assert got["most_novel"][0]["case"] == 1 and got["most_novel"][0]["novelty"] is None
    assert got["valid_cases"] == 3 and got["outside_95"] == 2 / 3
    assert novelty.line("test", rec).startswith("novelty test: 4 cases against 20 reference cases, k 2, 4 features: median 0.5, max inf, "
                                                "outside p95 0.666667, p99 0.666667, spearman with mse ")
    assert novelty.heading(rec) == "3 of 4 cases against 20 reference cases, k 2, 4 features"
    rows = novelty.section_rows(rec)
    assert rows[0] == ["Name", "Value"] and len(rows) == 7 + 5
    chart = novelty.svg_quintiles(rec, "mse by novelty quintile")
    assert chart.startswith("<svg") and chart.count('class="quintile"') == sum(1 for b in rec["quintiles"] if math.isfinite(b["mse"]))
    empty = novelty.svg_quintiles(novelty.summary(_case([math.nan])), "t")
    assert 'class="quintile"' not in empty and empty.startswith("<svg")


def test_check_k():
    assert novelty.check_k(1) == 1 and novelty.check_k(32) == 32
    for bad in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match="novelty_k must be an integer from 1 to 32"):
            novelty.check_k(bad)


# ---- the command lines -----------------------------------------------------------------------------

def test_cli_parser():
    parser = cli.build_parser()
    args = parser.parse_args(["--model-folder", "m", "--train-inputs", "train.nc"])
    assert (args.novelty_k, args.novelty_reference) == (5, None)
    args = parser.parse_args(["--model-folder", "m", "--test-inputs", "scored.nc", "--novelty-k", "32", "--novelty-reference", "a.nc", "b.nc"])
    assert (args.novelty_k, args.novelty_reference) == (32, ["a.nc", "b.nc"])
    assert args.test_inputs == ["scored.nc"] and args.output_html_folder == ""      # evaluate_cae's flags are all there
    for bad in (["--novelty-k", "0"], ["--novelty-k", "33"], ["--novelty-k", "x"], ["--novelty-reference"]):
        with pytest.raises(SystemExit):
            parser.parse_args(["--model-folder", "m"] + bad)
    with pytest.raises(SystemExit):         # no reference set: refused before the model folder is looked at
        cli.main(["--model-folder", "no_such_model_folder", "--test-inputs", "scored.nc"])


def test_apply_cae_flags(tmp_path):
    parser = apply_cae.build_parser()
    base = ["in.nc", "out.nc", "--model-folder", "m"]
    assert apply_cae.novelty_keywords(parser.parse_args(base)) == {}
    reference = str(tmp_path / "train.nc")
    open(reference, "wb").close()
    args = parser.parse_args(base + ["--novelty-variable", "nov", "--novelty-reference", reference])
    assert apply_cae.novelty_keywords(args) == {"novelty_variable": "nov", "k": 5}
    args = parser.parse_args(base + ["--novelty-variable", "nov", "--novelty-reference", reference, "--novelty-k", "7"])
    assert apply_cae.novelty_keywords(args) == {"novelty_variable": "nov", "k": 7}
    for (bad, text) in ((["--novelty-variable", "nov"], "need each other"), (["--novelty-reference", reference], "need each other"),
                        (["--novelty-k", "3"], "--novelty-k needs"),
                        (["--novelty-variable", "nov", "--novelty-reference", reference, "--novelty-k", "0"], "from 1 to 32"),
                        (["--novelty-variable", "nov", "--novelty-reference", reference, "--novelty-k", "33"], "from 1 to 32"),
                        (["--novelty-variable", "model_output", "--novelty-reference", reference], "must differ"),
                        (["--novelty-variable", "nov", "--novelty-reference", str(tmp_path / "none.nc")], "not found")):
        with pytest.raises(SystemExit, match=text):
            apply_cae.novelty_keywords(parser.parse_args(base + bad))
    with pytest.raises(SystemExit, match="need each other"):        # main refuses before a rank is spawned or a model loaded
        apply_cae.main(["in.nc", "out.nc", "--model-folder", "no_such_model_folder", "--novelty-variable", "nov"])


# ---- the evaluator ---------------------------------------------------------------------------------

def _ev(**changes):
    ev = SimpleNamespace(novelty=True, novelty_k=5, novelty_reference=None, training_paths=["train.nc"], testing_paths=["test.nc"])
    for (k, v) in changes.items():
        setattr(ev, k, v)
    return ev


@pytest.mark.parametrize("changes, text", [
    (dict(training_paths=[]), "novelty needs a reference set: the training files, or novelty_reference, the files of the reference set"),
    (dict(novelty_k=0), "novelty_k must be an integer from 1 to 32, got 0"),
    (dict(novelty_k=33), "novelty_k must be an integer from 1 to 32, got 33"),
    (dict(novelty_k=1.5), "novelty_k must be an integer from 1 to 32, got 1.5"),
])
def test_refusals_before_the_model_is_loaded(changes, text):
    with pytest.raises(ValueError) as refused:
        analyses.NOVELTY.check(_ev(**changes))
    assert str(refused.value) == text
    analyses.NOVELTY.check(_ev(novelty=False, **changes))      # switched off, nothing is looked at


def test_the_checks_pass_what_is_right_and_the_constructor_refuses_first():
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    analyses.NOVELTY.check(_ev())
    analyses.NOVELTY.check(_ev(training_paths=[], novelty_reference=["ref.nc"]))
    assert analyses.NOVELTY in analyses.ANALYSES and analyses.NOVELTY.enabled(_ev()) and not analyses.NOVELTY.enabled(_ev(novelty=False))
    with pytest.raises(ValueError, match="novelty needs a reference set"):
        ModelEvaluator([], ["scored.nc"], model_path="no_such_model_folder", novelty=True)
    with pytest.raises(ValueError, match="novelty_k must be an integer from 1 to 32, got 40"):
        ModelEvaluator(["train.nc"], ["scored.nc"], model_path="no_such_model_folder", novelty=True, novelty_k=40)


def test_report_with_the_option_off_and_on():
    metrics = {"test": {"mse": 1.0, "mae": 0.5}}
    measures = [("test", {"mae": np.array([0.5, 0.25]), "mse": np.array([1.0, 0.5])})]
    plain = evaluation_report(metrics, measures)
    assert evaluation_report(metrics, measures, novelty=None) == plain and "Novelty of the cases" not in plain
    rec = novelty.summary(_case([0.5, 0.25]), reference=_case([0.125, 0.25, 0.5]), mse=np.array([1.0, 0.5]), mae=np.array([0.5, 0.25]))
    page = evaluation_report(metrics, measures, novelty=[("test", rec)])
    assert page.count("<h2>Novelty of the cases</h2>") == 1 and "test: 2 of 2 cases against 20 reference cases, k 2, 4 features" in page
    assert page.count('alt="test mse by novelty quintile"') == 1
    start = page.index("<h2>Novelty of the cases</h2>")
    assert plain.startswith(page[:start].rstrip())      # what comes before the section is the plain page's


# ---- the entry point's host side -------------------------------------------------------------------

def test_workspace_rule():
    lib = _lib.load()
    size = lib.cae_case_neighbours_workspace_bytes
    assert size(0, 10, 5) == 0 and size(-1, 10, 5) == 0 and size(10, -1, 5) == 0 and size(10, 10, 0) == 0 and size(10, 10, 33) == 0
    assert size(1 << 31, 10, 5) == 0
    # no reference: the validity of the queries alone
    assert size(3, 0, 5) == 16 and size(4, 0, 32) == 16
    # one query tile, every reference tile a split of its own: 3 splits of 10 queries and 5 entries, 12 bytes each
    assert size(10, 130, 5) == 3 * 10 * 5 * 8 + 3 * 10 * 5 * 4 + (10 + 130) * 4
    # so many query tiles that a workgroup walks a run of reference tiles: 65 tiles want 16 splits of 17 tiles, runs of 2, 9 splits
    assert size(4097, 1025, 1) == 9 * 4097 * 8 + (9 * 4097 + 1) // 2 * 8 + (4097 + 1025) * 4


no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal table runs without a GPU only: its addresses are made up")
(Q, R, D2, IDX, CNT, WS) = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000)
NAMES = "query n_query query_stride ref n_ref ref_stride dim k ref_base self_offset merge dist2 index count workspace workspace_bytes stream".split()
CALL = dict(query=Q, n_query=5, query_stride=8, ref=R, n_ref=6, ref_stride=8, dim=8, k=3, ref_base=0, self_offset=-1, merge=0, dist2=D2,
            index=IDX, count=CNT, workspace=WS, workspace_bytes=1 << 20, stream=None)
TABLE = [
    ("bad argument", [dict(k=0), dict(k=33), dict(n_query=-1), dict(n_ref=-1), dict(ref_base=-1), dict(ref_base=(1 << 31) - 6),
                      dict(self_offset=-2), dict(merge=2), dict(merge=-1), dict(n_query=1 << 31)]),
    ("dim must be at least 1 while rows exist", [dict(dim=0), dict(dim=-3)]),
    ("a row stride is shorter than dim", [dict(query_stride=7), dict(ref_stride=7)]),
    ("null output", [dict(dist2=None), dict(index=None), dict(count=None)]),
    ("null operand with rows to read", [dict(query=None), dict(ref=None)]),
    ("an operand reaches 2^60 elements from its pointer", [dict(query_stride=1 << 59), dict(ref_stride=1 << 58)]),
    ("pointers must be aligned to their element size", [dict(query=Q + 2), dict(ref=R + 1), dict(dist2=D2 + 4), dict(index=IDX + 2),
                                                        dict(count=CNT + 1)]),
    ("needs a workspace of 232 bytes", [dict(workspace=None), dict(workspace_bytes=231), dict(workspace=WS + 4)]),
]
ROWS = [(text, change) for (text, changes) in TABLE for change in changes]


@no_gpu
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r[0][:24] + ":" + ",".join(f"{k}={v}" for (k, v) in r[1].items()))
def test_case_neighbours_refusal(row):
    """the call is answered by the host, with CAE_ERR_ARG and this text"""
    (text, change) = row
    lib = _lib.load()
    args = dict(CALL, **change)
    assert lib.cae_case_neighbours(*[args[name] for name in NAMES]) == -1
    assert text in lib.cae_last_error().decode()


@no_gpu
def test_case_neighbours_empty_query_set_succeeds_on_the_host():
    lib = _lib.load()
    args = dict(CALL, n_query=0, query=None, workspace=None, workspace_bytes=0)
    assert lib.cae_case_neighbours(*[args[name] for name in NAMES]) == 0
