"""Neighbourhood skill without a GPU: utils/fss.py against hand-worked sums, the identities of the definition on the numpy
restatement (fss_ref.py), NaN handling, pooling past 2^63, strict JSON, the command's parser with its '<' tokens, the
evaluator's refusals with their texts, and one build_html with fraction_skill replaced by the restatement: the JSON, the
printed line, the page and the report's section."""
import io
import json
import math
import os
from contextlib import redirect_stderr, redirect_stdout

import numpy as np
import pytest

from cae_tools_amd.utils import distribution, fss, report
from fss_ref import contingency, reference
from test_evaluator_freeze_cpu import GPU_CALLS, METRICS, PATCH_MODULES, Calls, _dataset, model  # noqa: F401  (model: a fixture)


# ---- the restatement and the identities ----------------------------------------------------------

def test_reference_by_hand():
    """a 3 x 4 plane, one threshold: the windows of width 1 and 3 counted by hand"""
    a = np.array([[[1, 0, 0, 1], [0, 1, 0, 0], [1, 1, 0, 0]]], dtype=np.float64)
    p = np.array([[[0, 1, 0, 1], [0, 1, 0, 0], [0, 1, 1, 0]]], dtype=np.float64)
    got = reference(p, a, [0.5], [1, 3, 5])
    # width 1: 12 windows, 5 events in p and in a (their squares are themselves), 3 in both
    assert got[0, 0, 0].tolist() == [12, 5, 5, 5, 5, 3]
    # width 3: x0 = 0: cM = 4 (p columns 0..2), cO = 4; x0 = 1: cM = 5, cO = 3
    assert got[0, 0, 1].tolist() == [2, 9, 7, 16 + 25, 16 + 9, 16 + 15]
    assert got[0, 0, 2].tolist() == [0] * 6                 # wider than a side: no window
    # a gap at (1, 1): strict leaves no 3 x 3 window, ignore keeps both with the pixel a non-event in both fields
    p[0, 1, 1] = np.nan
    assert reference(p, a, [0.5], [3])[0, 0, 0].tolist() == [0] * 6
    assert reference(p, a, [0.5], [3], "ignore")[0, 0, 0].tolist() == [2, 7, 5, 9 + 16, 9 + 4, 9 + 8]
    assert reference(p, a, [0.5], [1])[0, 0, 0].tolist() == [11, 4, 4, 4, 4, 2]
    assert reference(p, a, [0.5], [1], "ignore")[0, 0, 0].tolist() == [11, 4, 4, 4, 4, 2]     # the window without a pair is left out
    # below-events, -0.0 as 0.0, a value on the threshold
    z = np.array([[[-0.0, 0.0, -1.0, 1.0]]])
    assert reference(z, z, [(0.0, "below")], [1])[0, 0, 0].tolist() == [4, 1, 1, 1, 1, 1]
    assert reference(z, z, [(0.0, "above")], [1])[0, 0, 0].tolist() == [4, 3, 3, 3, 3, 3]


def test_identities_on_the_restatement():
    rng = np.random.default_rng(5)
    a = rng.random((3, 9, 12))
    p = np.roll(a, 2, axis=2) + 0.05 * rng.standard_normal(a.shape)
    a[0, 2, 3] = np.nan
    p[1, 5, 5] = np.inf
    thresholds = [0.3, (0.2, "below"), 0.8]
    for gaps in ("strict", "ignore"):
        got = reference(p, a, thresholds, [1, 3, 9], gaps)
        for (t, (value, side)) in enumerate(((0.3, "above"), (0.2, "below"), (0.8, "above"))):
            for c in range(3):
                (pairs, hits, misses, alarms) = contingency(p[c:c + 1], a[c:c + 1], value, side)
                assert got[c, t, 0].tolist() == [pairs, hits + alarms, hits + misses, hits + alarms, hits + misses, hits]
        same = reference(a, a, thresholds, [1, 3, 9], gaps)
        scores = fss.scores_from_sums(same, [1, 3, 9])
        defined = same[..., 3] + same[..., 4] > 0
        assert defined.any() and (scores["case_fss"][defined] == 1.0).all() and np.isnan(scores["case_fss"][~defined]).all()
    # h == w == n: one window, the sums are the totals
    (q, b) = (p[2:, :9, :9], a[2:, :9, :9])
    one = reference(q, b, [0.5], [9])[0, 0, 0]
    (cm, co) = (int((q >= 0.5).sum()), int((b >= 0.5).sum()))
    assert one.tolist() == [1, cm, co, cm * cm, co * co, cm * co]
    # strict and ignore agree where every pixel is a pair
    assert np.array_equal(reference(q, b, thresholds, [1, 3, 5]), reference(q, b, thresholds, [1, 3, 5], "ignore"))


def test_pattern_rolled_by_nine_columns():
    """what the score is for: the datagen pattern at its 90th percentile with the prediction the target rolled by 9 columns
    is penalised twice pixel by pixel (pooled FSS between 0.8 and 0.9 at width 1, depending on the cases drawn) and nearly
    perfect in neighbourhoods much wider than the displacement (above 0.99 at width 129), rising with every width"""
    from cae_tools_amd.data import datagen
    ds = datagen.generate("circle", 4, seed=99)
    a = np.asarray(ds["hires"].values, dtype=np.float64)[:, 0]
    p = np.roll(a, 9, axis=2)
    widths = [1, 9, 33, 129]
    scores = fss.scores_from_sums(reference(p, a, [float(np.quantile(a, 0.9))], widths), widths)
    print(scores["fss"], scores["fss_uniform"], scores["skilful_width"])
    curve = scores["fss"][0]
    assert 0.8 < curve[0] < 0.9 and curve[3] > 0.99 and all(b > a for (a, b) in zip(curve, curve[1:]))
    assert abs(scores["fss_uniform"][0] - 0.55) < 1e-3 and abs(scores["frequency_bias"][0][0] - 1.0) < 1e-12   # a roll keeps the events


# ---- utils/fss.py ----------------------------------------------------------------------------------

def test_scores_by_hand():
    # two cases, one threshold, widths 1 and 3
    sums = np.array([[[[10, 4, 5, 4, 5, 2], [2, 9, 7, 41, 25, 31]]],
                     [[[6, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]]], dtype=np.int64)
    s = fss.scores_from_sums(sums, [1, 3])
    assert s["n_cases"] == 2 and s["pooled_sums"] == [[[16, 4, 5, 4, 5, 2], [2, 9, 7, 41, 25, 31]]]
    assert s["case_fss"][0, 0].tolist() == [1.0 - 5.0 / 9.0, 1.0 - 4.0 / 66.0]
    assert np.isnan(s["case_fss"][1]).all()                # no event in either field: no denominator
    assert s["fss"] == [[1.0 - 5.0 / 9.0, 1.0 - 4.0 / 66.0]]
    assert s["f_target"] == [[5 / 16, 7 / 18]] and s["f_prediction"] == [[4 / 16, 9 / 18]]
    assert s["frequency_bias"] == [[4 / 5, 9 / 7]]
    assert s["fss_uniform"] == [0.5 + 5 / 32]
    assert s["skilful_width"] == [3]                        # 0.444 < 0.656 <= 0.939
    # nothing anywhere
    none = fss.scores_from_sums(np.zeros((0, 2, 1, 6), dtype=np.int64), [1])
    assert none["pooled_sums"] == [[[0] * 6]] * 2 and none["skilful_width"] == [None, None]
    assert all(math.isnan(v) for row in none["fss"] for v in row) and all(math.isnan(v) for v in none["fss_uniform"])
    for bad in (np.zeros((1, 1, 2, 6)), np.zeros((1, 1, 2, 5), dtype=np.int64), np.zeros((1, 2, 6), dtype=np.int64)):
        with pytest.raises(ValueError, match="scores_from_sums: "):
            fss.scores_from_sums(bad, [1, 3])


def test_pooling_passes_2_63_without_wrapping():
    """400 cases at the bound of a case: the pooled sums are Python integers above 2^63, and the score is still exact"""
    top = (1 << 28) * 16641 * 16641                 # 7.4e16: the largest sum of a case
    case = np.array([[[1 << 28, (1 << 28) * 16641, (1 << 28) * 16641, top, top, top]]], dtype=np.int64)
    sums = np.repeat(case[None], 400, axis=0)
    s = fss.scores_from_sums(sums, [129])
    assert s["pooled_sums"][0][0][3] == 400 * top > (1 << 63)
    assert s["fss"] == [[1.0]] and s["f_target"] == [[1.0]] and s["frequency_bias"] == [[1.0]]
    half = sums.copy()
    half[:, 0, 0, 5] = top // 2                     # S cM cO half of S cM^2: FSS = 1 - (2 top - top) / (2 top)
    assert fss.scores_from_sums(half, [129])["fss"] == [[0.5]]
    assert (fss.scores_from_sums(half, [129])["case_fss"] == 0.5).all()


def test_checks_and_defaults():
    assert fss.default_widths(256, 256) == [1, 3, 5, 9, 17, 33, 65] and fss.default_widths(16, 40) == [1, 3, 5, 9]
    assert fss.default_widths(0, 5) == []
    assert fss.check_widths((1, 3, 129)) == [1, 3, 129]
    for bad in ([], [2], [0], [131], [3, 1], [3, 3], list(range(1, 19, 2)), [1.5], ["x"], None):
        with pytest.raises(ValueError):
            fss.check_widths(bad)
    assert fss.check_thresholds([1, (2.5, "below"), [3, "above"]]) == ([1.0, 2.5, 3.0], [0, 1, 0])
    for bad in ([], [0.0] * 9, [math.nan], [math.inf], [(1.0, "over")], ["x"], [(1.0, 2.0, 3.0)], 5):
        with pytest.raises(ValueError):
            fss.check_thresholds(bad)
    assert fss.label(291.5, "above") == ">=291.5" and fss.label(1.0, "below", 0.05) == "<q5" and fss.label(1.0, "above", 0.995) == ">=q99.5"


@pytest.fixture(scope="module")
def record():
    rng = np.random.default_rng(8)
    a = rng.random((3, 8, 8))
    p = np.roll(a, 1, axis=2)
    thresholds = [(0.1, "below"), 0.9, 2.0]             # nothing reaches 2.0: its scores have no denominator
    widths = [1, 3, 5]
    scores = fss.scores_from_sums(reference(p, a, thresholds, widths), widths)
    return fss.summary(scores, thresholds, widths, "strict", 8, 8, [0.05, 0.9, None])


def test_summary_json_line_rows_and_page(record, tmp_path):
    assert [t["label"] for t in record["thresholds"]] == ["<q5", ">=q90", ">=2"]
    assert [t["side"] for t in record["thresholds"]] == ["below", "above", "above"] and record["widths"] == [1, 3, 5]
    path = fss.write_json(str(tmp_path / "fss_test.json"), record)
    with open(path) as f:
        text = f.read()
    back = json.loads(text, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert "NaN" not in text and back["fss"][2] == [None, None, None] and back["skilful_width"][2] is None
    assert back["pooled_sums"] == record["pooled_sums"] and back["gaps"] == "strict" and back["n_cases"] == 3
    assert np.asarray(back["case_fss"], dtype=object).shape == (3, 3, 3)
    assert back["thresholds"][2] == {"value": 2.0, "side": "above", "percentile": None, "label": ">=2"}
    line = fss.line("test", record)
    shown = ["none" if n is None else str(n) for n in record["skilful_width"]]
    assert line == f"fss test: 3 cases, widths 1..5 (strict), skilful width <q5 {shown[0]}, >=q90 {shown[1]}, >=2 none"
    rows = fss.section_rows(record)
    assert rows[0] == ["Threshold", "value", "target frequency", "frequency bias", "uniform FSS", "skilful width", "FSS n = 1",
                       "FSS n = 3", "FSS n = 5"]
    assert len(rows) == 4 and rows[3][0] == ">=2" and rows[3][2] == "0" and rows[3][3:] == ["none", "0.5", "none", "none", "none", "none"]
    assert rows[2][6] == f"{record['fss'][1][0]:.6g}"
    page_path = fss.write_page(str(tmp_path / "fss"), [("test", record)])
    assert page_path == str(tmp_path / "fss" / "index.html")
    with open(page_path) as f:
        page = f.read()
    assert page.count('alt="test fss ') == 3 and 'alt="test fss &lt;q5"' in page and "test: 3 cases of 8 x 8, gaps strict" in page
    svg = fss.svg_curve(record, 1, "t")
    assert svg.count('class="series"') == 2 and 'data-name="uniform"' in svg and 'data-name="&gt;=q90"' in svg
    with pytest.raises(ValueError, match="do not belong"):
        fss.summary({**record}, [0.5], [1, 3, 5], "strict", 8, 8)
    with pytest.raises(ValueError, match="gaps must be one of strict, ignore"):
        fss.summary({**record}, [(0.1, "below"), 0.9, 2.0], [1, 3, 5], "lenient", 8, 8)


def test_report_section_is_off_by_default(record):
    measures = [("test", {"mae": np.array([0.1, 0.2]), "mse": np.array([0.01, 0.04])})]
    plain = report.evaluation_report({}, measures)
    assert "Neighbourhood skill" not in plain
    page = report.evaluation_report({}, measures, fss=([("test", record)], "fss/index.html"))
    assert page.count("<h2>Neighbourhood skill</h2>") == 1 and page.count('href="fss/index.html"') == 1
    assert "test: 3 thresholds, widths 1, 3, 5, 3 cases, gaps strict" in page
    assert page[:page.index("<h2>Neighbourhood skill</h2>")].rstrip() == plain[:plain.index("</body>")].rstrip()


# ---- the command and the evaluator -------------------------------------------------------------------

def test_cli_flags_are_evaluate_cae_plus_the_four():
    from cae_tools_amd.cli import evaluate_cae, fss as cli
    base = {a.dest for a in evaluate_cae.build_parser()._actions}
    mine = {a.dest for a in cli.build_parser()._actions}
    assert mine - base == {"fss_thresholds", "fss_percentiles", "fss_widths", "fss_gaps"} and base <= mine
    args = cli.build_parser().parse_args(["--model-folder", "m"])
    assert (args.fss_thresholds, args.fss_percentiles, args.fss_widths, args.fss_gaps) == (None, None, None, "strict")
    args = cli.build_parser().parse_args(["--model-folder", "m", "--fss-percentiles", "<5", "90", "99.5", "--fss-widths", "1", "9", "129",
                                          "--fss-gaps", "ignore"])
    assert args.fss_percentiles == [(5.0, "below"), (90.0, "above"), (99.5, "above")]
    assert (args.fss_widths, args.fss_gaps, args.fss_thresholds) == ([1, 9, 129], "ignore", None)
    args = cli.build_parser().parse_args(["--model-folder", "m", "--fss-thresholds", "<273.15", "300"])
    assert args.fss_thresholds == [(273.15, "below"), (300.0, "above")] and args.fss_percentiles is None
    for bad in (["--fss-thresholds", "1", "--fss-percentiles", "90"], ["--fss-thresholds", "warm"], ["--fss-thresholds", "<"],
                ["--fss-thresholds", "nan"], ["--fss-widths", "2"], ["--fss-widths", "131"], ["--fss-widths", "0"],
                ["--fss-gaps", "lenient"], ["--fss-thresholds"]):
        with pytest.raises(SystemExit), redirect_stdout(io.StringIO()), redirect_stderr(io.StringIO()):
            cli.build_parser().parse_args(["--model-folder", "m"] + bad)
    assert "fss <partition>: <n> cases, widths <first>..<last> (<gaps>), skilful width" in cli.__doc__


def test_constructor_refusals(model, tmp_path):  # noqa: F811
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    nowhere = str(tmp_path / "no_model")
    steps = [(dict(fss_thresholds=[1.0], fss_percentiles=[90]), "fss_thresholds and fss_percentiles exclude each other"),
             (dict(fss_thresholds=[]), "1 to 8 thresholds expected, got 0"),
             (dict(fss_thresholds=[0.0] * 9), "1 to 8 thresholds expected, got 9"),
             (dict(fss_thresholds=[math.nan]), "the thresholds must be finite, got nan"),
             (dict(fss_thresholds=[(1.0, "over")]), "a threshold's side must be one of above, below, got 'over'"),
             (dict(fss_percentiles=[0]), "fss_percentiles must lie between 0 and 100, got [0.0]"),
             (dict(fss_percentiles=[(100, "below")]), "fss_percentiles must lie between 0 and 100, got [100.0]"),
             (dict(fss_widths=[1, 2]), "1 to 8 odd, strictly ascending widths from 1 to 129 expected, got [1, 2]"),
             (dict(fss_widths=[3, 1]), "1 to 8 odd, strictly ascending widths from 1 to 129 expected, got [3, 1]"),
             (dict(fss_widths=[131]), "1 to 8 odd, strictly ascending widths from 1 to 129 expected, got [131]"),
             (dict(fss_gaps="lenient"), "fss_gaps must be one of strict, ignore, got 'lenient'")]
    for (options, text) in steps:           # each refusal comes before the model is loaded: there is none at this path
        with pytest.raises(ValueError) as refused:
            ModelEvaluator(None, None, model_path=nowhere, fss=True, **options)
        assert str(refused.value) == text
    # the earlier refusals keep their place in front of it
    with pytest.raises(ValueError, match="strata needs strata_variable"):
        ModelEvaluator(None, None, model_path=nowhere, fss=True, fss_gaps="lenient", strata=True)
    # options that are off are not checked
    with redirect_stdout(io.StringIO()):
        ev = ModelEvaluator(None, None, model_path=model, fss_widths=[2], fss_gaps="lenient")
    assert ev.fss is False


class FssCalls(Calls):
    """the freeze test's stand-ins, and the restatement in place of fraction_skill"""

    def fraction_skill(self, pred, actual, thresholds, widths=None, gaps="strict", device=None):
        self.note("fraction_skill", pred, actual, thresholds=len(thresholds), widths=list(widths), gaps=gaps)
        return reference(self.plane(pred), self.plane(actual), thresholds, widths, gaps)


def _build(model, out, monkeypatch, **options):  # noqa: F811
    import importlib
    from cae_tools_amd.models import model_evaluator
    (train, test) = (_dataset(5, 11), _dataset(4, 12))
    calls = FssCalls((("train", train), ("test", test)))
    for module in PATCH_MODULES:
        module = importlib.import_module(module)
        for call in GPU_CALLS + ("fraction_skill",):
            if hasattr(module, call):
                monkeypatch.setattr(module, call, getattr(calls, call))
    log = io.StringIO()
    with redirect_stdout(log):
        ev = model_evaluator.ModelEvaluator(None, None, output_html_folder=out, model_path=model, fss=True, **options)
        ev.build_html("case", train, test, METRICS)
    return train, test, calls, log.getvalue().splitlines()


def test_build_html_with_the_restatement(model, tmp_path, monkeypatch):  # noqa: F811
    out = str(tmp_path / "report")
    (train, test, calls, printed) = _build(model, out, monkeypatch, distribution=True)
    assert sorted(f for f in os.listdir(out) if f.startswith("fss")) == ["fss", "fss_test.json", "fss_train.json"]
    assert os.listdir(os.path.join(out, "fss")) == ["index.html"]
    # after the distribution's calls: the range over both partitions, then per partition the histogram and the windows
    mine = calls.log[-8:]
    assert [c.split("(")[0] for c in mine] == ["case_range"] * 4 + ["joint_histogram", "fraction_skill"] * 2
    assert mine[5] == "fraction_skill(test:model_output, test:hires, thresholds=4, widths=[1, 3, 5, 9, 17, 33], gaps=strict)"
    assert sorted(u for u in calls.uploads if ":" in u) == sorted(set(u for u in calls.uploads if ":" in u))
    with open(os.path.join(out, "fss_test.json")) as f:
        rec = json.load(f, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    with open(os.path.join(out, "distribution_test.json")) as f:
        dist = json.load(f)
    # a percentile threshold is the distribution's quantile of the target
    levels = dist["quantile_levels"]
    assert [t["percentile"] for t in rec["thresholds"]] == [q for (q, _) in distribution.THRESHOLDS]
    assert [t["side"] for t in rec["thresholds"]] == [side for (_, side) in distribution.THRESHOLDS]
    assert [t["value"] for t in rec["thresholds"]] == [dist["quantile_target"][levels.index(q)] for (q, _) in distribution.THRESHOLDS]
    assert [t["label"] for t in rec["thresholds"]] == ["<q5", ">=q90", ">=q95", ">=q99"]
    assert (rec["widths"], rec["gaps"], rec["h"], rec["w"], rec["n_cases"]) == ([1, 3, 5, 9, 17, 33], "strict", 64, 64, 4)
    (p, a) = (np.asarray(test["model_output"].values)[:, 0], np.asarray(test["hires"].values, dtype=np.float64)[:, 0])
    want = reference(p, a, [(t["value"], t["side"]) for t in rec["thresholds"]], rec["widths"])
    assert rec["pooled_sums"] == want.astype(object).sum(axis=0).tolist()
    assert rec["pooled_sums"][1][0][0] == 4 * 64 * 64 - 1          # width 1, strict: the pairs
    assert 0.0 < rec["fss"][1][0] < rec["fss"][1][-1] <= 1.0
    lines = [ln for ln in printed if ln.startswith("fss ")]
    assert len(lines) == 2 and lines[0] == fss.line("test", rec) and lines[1].startswith("fss train: 5 cases, widths 1..33 (strict), ")
    with open(os.path.join(out, "index.html")) as f:
        page = f.read()
    assert page.count("<h2>Neighbourhood skill</h2>") == 1 and page.count('href="fss/index.html"') == 1
    assert "test: 4 thresholds, widths 1, 3, 5, 9, 17, 33, 4 cases, gaps strict" in page
    assert page.index("<h2>Value distribution</h2>") < page.index("<h2>Neighbourhood skill</h2>") < page.index("<h2>Training Summary</h2>")
    with open(os.path.join(out, "fss", "index.html")) as f:
        curves = f.read()
    assert curves.count('data-partition="') == 2 and curves.count('alt="test fss ') == 4


def test_build_html_with_given_thresholds(model, tmp_path, monkeypatch):  # noqa: F811
    out = str(tmp_path / "report")
    (train, test, calls, printed) = _build(model, out, monkeypatch, fss_thresholds=[(0.25, "below"), 0.75], fss_widths=[1, 9, 65],
                                           fss_gaps="ignore")
    # the values are used as given: no range, no histogram
    assert [c.split("(")[0] for c in calls.log if "case_range" in c or "joint_histogram" in c] == []
    assert calls.log[-1] == "fraction_skill(train:model_output, train:hires, thresholds=2, widths=[1, 9, 65], gaps=ignore)"
    with open(os.path.join(out, "fss_train.json")) as f:
        rec = json.load(f)
    assert [(t["value"], t["side"], t["percentile"], t["label"]) for t in rec["thresholds"]] == \
        [(0.25, "below", None, "<0.25"), (0.75, "above", None, ">=0.75")]
    assert rec["widths"] == [1, 9, 65] and rec["pooled_sums"][0][2] == [0] * 6 and rec["fss"][0][2] is None   # 65 > 64: no window
    assert printed[-1].startswith("fss train: 5 cases, widths 1..65 (ignore), skilful width <0.25 ")
