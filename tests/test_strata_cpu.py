"""Skill by stratum without a GPU: utils/strata.py against direct numpy on a small synthetic set, the index rule of the
restatement (strata_ref.py) against exact integer arithmetic, the command's parser, the evaluator's refusals with their
texts, and one build_html with the GPU calls replaced by the restatement: the JSON, the printed line and the report's
section."""
import io
import json
import math
import os
from contextlib import redirect_stdout

import numpy as np
import pytest

from cae_tools_amd.utils import report, strata
from strata_ref import Reference, on_target_grid, source_index, strata_of
from test_evaluator_freeze_cpu import GPU_CALLS, METRICS, PATCH_MODULES, Calls, _dataset, model  # noqa: F401  (model: a fixture)


# ---- the index rule ----------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [((5, 5), (5, 5)), ((1, 1), (6, 9)), ((3, 5), (7, 11)), ((9, 9), (4, 4)), ((4, 4), (33, 65)),
                                   ((16, 16), (256, 256))], ids=str)
def test_source_index_against_integer_arithmetic(sizes):
    """floor((y + 0.5) * sh / h) is floor((2 y + 1) sh / (2 h)) in integers; the identity at equal sizes, 0 for one sample"""
    ((sh, sw), (h, w)) = sizes
    for (n_in, n_out) in ((sh, h), (sw, w)):
        exact = [min(((2 * y + 1) * n_in) // (2 * n_out), n_in - 1) for y in range(n_out)]
        assert source_index(n_out, n_in).tolist() == exact
        if n_in == n_out:
            assert exact == list(range(n_out))
        if n_in == 1:
            assert set(exact) == {0}
    s = np.arange(2 * sh * sw, dtype=np.float64).reshape(2, sh, sw)
    got = on_target_grid(s, h, w)
    assert got.shape == (2, h, w) and got[1, h - 1, w - 1] == s[1, source_index(h, sh)[-1], source_index(w, sw)[-1]]


def test_strata_of_values_on_edges_and_signed_zero():
    edges = [-1.0, 0.0, 0.5]
    assert strata_of([-2.0, -1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 1e300, -1e300], edges).tolist() == [0, 1, 1, 2, 2, 2, 3, 3, 0]
    assert strata_of([3.0, -3.0], []).tolist() == [0, 0]


# ---- edges and labels --------------------------------------------------------------------------

def test_edges_from_classes_counts_and_labels():
    (edges, names) = strata.edges_from_classes([30, 10, 20, 10, 21])
    assert edges == [15.0, 20.5, 25.5] and names == ["= 10", "= 20", "= 21", "= 30"]
    # a value that is not listed counts to the nearest listed class
    assert strata_of([9.0, 14.0, 16.0, 20.4, 24.0, 26.0, 99.0], edges).tolist() == [0, 0, 1, 1, 2, 3, 3]
    assert strata.edges_from_classes([7.0]) == ([], ["= 7"])
    for bad in ([], [1.0, math.nan], [math.inf]):
        with pytest.raises(ValueError, match="strata classes"):
            strata.edges_from_classes(bad)
    assert strata.edges_from_count(0.0, 8.0, 4) == [2.0, 4.0, 6.0]
    assert strata.edges_from_count(288.0, 298.0, 1) == []
    # a degenerate range is one stratum
    for (lo, hi) in ((3.0, 3.0), (4.0, 3.0), (math.inf, -math.inf), (0.0, math.inf), (-1.7e308, 1.7e308), (1.0, 1.0 + 2.0 ** -52)):
        assert strata.edges_from_count(lo, hi, 8) == [], (lo, hi)
    assert strata.labels([]) == ["all"] and strata.labels([1.5]) == ["< 1.5", ">= 1.5"]
    assert strata.labels([0.0, 0.25, 1000.0]) == ["< 0", "[0, 0.25)", "[0.25, 1000)", ">= 1000"]
    assert strata.check_edges([0, 1, 2.5]) == [0.0, 1.0, 2.5] and strata.check_edges([]) == []
    for bad in ([1.0, 1.0], [2.0, 1.0], [math.nan], [0.0, math.inf]):
        with pytest.raises(ValueError, match="strata_edges must be finite and strictly ascending"):
            strata.check_edges(bad)
    with pytest.raises(ValueError, match="at most 64 strata expected, got 65"):
        strata.check_edges(list(range(64)))


# ---- the scores --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synthetic():
    """4 cases of 12 x 10 about 290 under a 3 x 5 stratifier; one stratum stays empty, some values are missing"""
    rng = np.random.default_rng(5)
    a = 290.0 + 3.0 * rng.standard_normal((4, 12, 10))
    p = 290.0 + 0.8 * (a - 290.0) + 0.3 * rng.standard_normal(a.shape) + 0.2
    s = rng.uniform(0.0, 3.0, (4, 3, 5))
    s[2, 1, 1] = np.nan
    (p[0, 0, 0], a[1, 1, 1], p[3, 4, 4]) = (np.nan, np.inf, -np.inf)
    edges = [1.0, 2.0, 3.0, 5.0]           # nothing lies in [3, 5): stratum 3 is empty
    return p, a, s, edges


def _two_passes(p, a, s, edges, shift):
    first = Reference(p, a, s, edges, shift)
    counts = {"members": first.members, "pairs": first.pairs, "unclassified": first.unclassified}
    means = strata.stratum_means(counts, first.sums, shift)
    second = Reference(p, a, s, edges, means)
    return counts, first.sums, second.sums, means


def test_scores_from_sums_against_numpy(synthetic):
    (p, a, s, edges) = synthetic
    (counts, sums, centred, means) = _two_passes(p, a, s, edges, 293.0)
    got = strata.scores_from_sums(counts, sums, centred, shift=293.0, centred_shift=means)
    v = on_target_grid(s, 12, 10)
    k = np.where(np.isfinite(v), strata_of(np.where(np.isfinite(v), v, 0.0), edges), -1)
    pair = (k >= 0) & np.isfinite(p) & np.isfinite(a)
    assert got["n_strata"] == 5 and got["pixels"] == p.size and got["unclassified"] == int((k < 0).sum()) == 4 * 2      # one source pixel
    close = lambda x, y: abs(x - y) <= 1e-12 * max(1.0, abs(y))      # noqa: E731
    for j in range(5):
        at = pair & (k == j)
        assert got["members"][j] == int((k == j).sum()) and got["pairs"][j] == int(at.sum())
        if not at.any():
            assert j >= 3 and all(math.isnan(got[name][j]) for name in strata.SCORES + ("mse_share",)) and got["share"][j] == 0.0
            continue
        (pj, aj) = (p[at], a[at])
        want = {"mean_target": aj.mean(), "mean_prediction": pj.mean(), "bias": (pj - aj).mean(), "mae": np.abs(pj - aj).mean(),
                "rmse": math.sqrt(((pj - aj) ** 2).mean()), "correlation": np.corrcoef(pj, aj)[0, 1],
                "sd_ratio": pj.std() / aj.std(), "share": at.sum() / pair.sum(),
                "mse_share": ((pj - aj) ** 2).sum() / ((p[pair] - a[pair]) ** 2).sum()}
        for (name, value) in want.items():
            assert close(got[name][j], value), (j, name, got[name][j], value)
    assert abs(sum(got["share"]) - 1.0) < 1e-12 and abs(np.nansum(got["mse_share"]) - 1.0) < 1e-12
    (pp, aa) = (p[pair], a[pair])
    pooled = {"mean_target": aa.mean(), "mean_prediction": pp.mean(), "bias": (pp - aa).mean(), "mae": np.abs(pp - aa).mean(),
              "rmse": math.sqrt(((pp - aa) ** 2).mean()), "correlation": np.corrcoef(pp, aa)[0, 1], "sd_ratio": pp.std() / aa.std()}
    for (name, value) in pooled.items():
        assert close(got["pooled"][name], value), (name, got["pooled"][name], value)
    assert got["pooled"]["pairs"] == int(pair.sum()) and got["pooled"]["members"] == int((k >= 0).sum())
    # one pass about a common shift gives the same scores, less exactly in the second moments
    once = strata.scores_from_sums(counts, sums, shift=293.0)
    assert once["bias"][:3] == got["bias"][:3] and abs(once["correlation"][0] - got["correlation"][0]) < 1e-9
    # nothing counted at all
    none = strata.scores_from_sums({"members": [0, 0], "pairs": [0, 0], "unclassified": 7}, np.zeros((2, 8)))
    assert none["pixels"] == 7 and math.isnan(none["pooled"]["rmse"]) and all(math.isnan(v) for v in none["rmse"])
    with pytest.raises(ValueError, match="scores_from_sums"):
        strata.scores_from_sums(counts, sums[:, :7])


def test_json_is_strict_the_line_and_the_chart(tmp_path, synthetic):
    (p, a, s, edges) = synthetic
    (counts, sums, centred, means) = _two_passes(p, a, s, edges, 0.0)
    record = strata.summary(strata.scores_from_sums(counts, sums, centred, centred_shift=means), "elevation", 0, edges, None, (3, 5), (12, 10))
    path = strata.write_json(str(tmp_path / "strata_test.json"), record)
    with open(path) as f:
        text = f.read()
    rec = json.loads(text, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert "NaN" not in text and rec["rmse"][3] is None and rec["correlation"][3] is None and rec["rmse"][0] is not None
    assert rec["labels"] == ["< 1", "[1, 2)", "[2, 3)", "[3, 5)", ">= 5"] and rec["edges"] == edges and rec["variable"] == "elevation"
    assert (rec["in_shape"], rec["out_shape"], rec["channel"]) == ([3, 5], [12, 10], 0)
    finite = [(r, name) for (r, name) in zip(rec["rmse"], rec["labels"]) if r is not None]
    (low, high) = (min(finite), max(finite))
    assert strata.line("test", record) == strata.line("test", rec) == (
        f"strata test: elevation, 5 strata, rmse {low[0]:.6g} ({low[1]}) .. {high[0]:.6g} ({high[1]}), unclassified 8")
    rows = strata.section_rows(rec)
    assert len(rows) == 1 + 5 + 1 and rows[0][0] == "Stratum" and rows[4][0] == "[3, 5)" and rows[4][7] == "none"
    assert rows[-1][0] == "all strata" and rows[-1][2] == str(rec["pooled"]["pairs"])
    svg = strata.svg_bars(rec, "bias +- rmse by elevation")
    assert svg.count('class="stratum"') == 3 and svg.count('class="spread"') == 3 and svg.count('class="zero"') == 1
    assert 'data-label="&lt; 1"' in svg
    empty = strata.summary(strata.scores_from_sums({"members": [0], "pairs": [0], "unclassified": 0}, np.zeros((1, 8))), "v", 0, [])
    assert strata.svg_bars(empty, "t").count('class="stratum"') == 0
    assert strata.line("train", empty) == "strata train: v, 1 strata, rmse none (none) .. none (none), unclassified 0"
    with pytest.raises(ValueError, match="do not belong together"):
        strata.summary(strata.scores_from_sums(counts, sums), "v", 0, edges[:2])


def test_report_section_is_off_by_default(synthetic):
    (p, a, s, edges) = synthetic
    (counts, sums, centred, means) = _two_passes(p, a, s, edges, 0.0)
    record = strata.summary(strata.scores_from_sums(counts, sums, centred, centred_shift=means), "elevation", 0, edges)
    measures = [("test", {"mae": np.array([0.1, 0.2]), "mse": np.array([0.01, 0.04])})]
    plain = report.evaluation_report({}, measures)
    assert "Skill by stratum" not in plain
    page = report.evaluation_report({}, measures, strata=[("test", record)])
    assert page.count("<h2>Skill by stratum</h2>") == 1 and page.count('alt="test skill by stratum"') == 1
    assert f"test: 5 strata of elevation, {record['pooled']['pairs']} pixel pairs, 8 pixels unclassified" in page
    # everything in front of the section is the page without it
    assert page[:page.index("<h2>Skill by stratum</h2>")].rstrip() == plain[:plain.index("</body>")].rstrip()


# ---- the command and the evaluator -------------------------------------------------------------

def test_cli_flags_are_evaluate_cae_plus_the_strata():
    from cae_tools_amd.cli import evaluate_cae, strata as cli
    base = {a.dest for a in evaluate_cae.build_parser()._actions}
    mine = {a.dest for a in cli.build_parser()._actions}
    assert mine - base == {"strata_variable", "strata_channel", "strata_edges", "strata_classes", "strata_count"} and base <= mine
    args = cli.build_parser().parse_args(["--model-folder", "m", "--strata-variable", "elevation", "--strata-edges", "500", "1500"])
    assert (args.strata_variable, args.strata_channel, args.strata_edges, args.strata_classes, args.strata_count) == \
        ("elevation", 0, [500.0, 1500.0], None, None)
    args = cli.build_parser().parse_args(["--model-folder", "m", "--strata-variable", "land_cover", "--strata-channel", "1",
                                          "--strata-classes", "1", "2", "5"])
    assert (args.strata_channel, args.strata_classes) == (1, [1.0, 2.0, 5.0])
    for bad in ([], ["--strata-variable", "v", "--strata-count", "0"], ["--strata-variable", "v", "--strata-count", "65"],
                ["--strata-variable", "v", "--strata-count", "4", "--strata-edges", "1"],
                ["--strata-variable", "v", "--strata-classes", "4", "--strata-edges", "1"]):
        with pytest.raises(SystemExit), redirect_stdout(io.StringIO()), __import__("contextlib").redirect_stderr(io.StringIO()):
            cli.build_parser().parse_args(["--model-folder", "m"] + bad)


def test_constructor_refusals(model, tmp_path):  # noqa: F811
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    nowhere = str(tmp_path / "no_model")
    steps = [(dict(), "strata needs strata_variable, the name of the stratifier in the data set"),
             (dict(strata_variable="v", strata_edges=[1.0], strata_classes=[1.0]), "strata_edges and strata_classes exclude each other"),
             (dict(strata_variable="v", strata_edges=[2.0, 1.0]), "strata_edges must be finite and strictly ascending, got [2.0, 1.0]"),
             (dict(strata_variable="v", strata_edges=[0.0, math.inf]), "strata_edges must be finite and strictly ascending, got [0.0, inf]"),
             (dict(strata_variable="v", strata_edges=list(range(64))), "at most 64 strata expected, got 65"),
             (dict(strata_variable="v", strata_classes=list(range(65))), "at most 64 strata expected, got 65"),
             (dict(strata_variable="v", strata_count=0), "strata_count must be an integer from 1 to 64, got 0"),
             (dict(strata_variable="v", strata_count=65), "strata_count must be an integer from 1 to 64, got 65"),
             (dict(strata_variable="v", strata_count=2.5), "strata_count must be an integer from 1 to 64, got 2.5")]
    for (options, text) in steps:           # each refusal comes before the model is loaded: there is none at this path
        with pytest.raises(ValueError) as refused:
            ModelEvaluator(None, None, model_path=nowhere, strata=True, **options)
        assert str(refused.value) == text
    # the earlier refusals keep their place in front of it
    with pytest.raises(ValueError, match="ensemble_size must be an integer"):
        ModelEvaluator(None, None, model_path=nowhere, strata=True, ensemble_size=1)
    # options that are off are not checked
    with redirect_stdout(io.StringIO()):
        ModelEvaluator(None, None, model_path=model, strata_edges=[2.0, 1.0], strata_count=0)


class StrataCalls(Calls):
    """the freeze test's stand-ins, and the restatement in place of strata_sums"""

    def strata_sums(self, pred, actual, strata, edges, shift=0.0, channel=0, device=None):  # noqa: F811
        self.note("strata_sums", pred, actual, strata, edges=len(edges), shift="scalar" if np.ndim(shift) == 0 else "per stratum",
                  channel=channel)
        s = strata.tensor
        ref = Reference(self.plane(pred), self.plane(actual), s[:, channel] if s.ndim == 4 else s.reshape(-1, 1, 1), edges, shift)
        return {"members": ref.members, "pairs": ref.pairs, "unclassified": ref.unclassified}, ref.sums


def _build(model, out, monkeypatch, **options):  # noqa: F811
    import importlib
    from cae_tools_amd.models import model_evaluator
    (train, test) = (_dataset(5, 11), _dataset(4, 12))
    calls = StrataCalls((("train", train), ("test", test)))
    for module in PATCH_MODULES:
        module = importlib.import_module(module)
        for call in GPU_CALLS + ("strata_sums",):
            if hasattr(module, call):
                monkeypatch.setattr(module, call, getattr(calls, call))
    log = io.StringIO()
    with redirect_stdout(log):
        ev = model_evaluator.ModelEvaluator(None, None, output_html_folder=out, model_path=model, strata=True, **options)
        ev.build_html("case", train, test, METRICS)
    return train, test, calls, log.getvalue().splitlines()


def test_build_html_with_the_restatement(model, tmp_path, monkeypatch):  # noqa: F811
    out = str(tmp_path / "report")
    (train, test, calls, printed) = _build(model, out, monkeypatch, strata_variable="lowres", strata_count=4)
    assert sorted(f for f in os.listdir(out) if f.startswith("strata")) == ["strata_test.json", "strata_train.json"]
    # the range goes over both partitions, then two passes per partition; the stratifier went up once per partition
    assert [c.split("(")[0] for c in calls.log if "strata" in c or "case_range" in c] == ["case_range", "case_range"] + ["strata_sums"] * 4
    assert calls.log[-4:] == [f"strata_sums({part}:model_output, {part}:hires, {part}:lowres, edges=3, shift={how}, channel=0)"
                              for part in ("test", "train") for how in ("scalar", "per stratum")]
    assert sorted(u for u in calls.uploads if "lowres" in u) == ["test:lowres", "train:lowres"]
    with open(os.path.join(out, "strata_test.json")) as f:
        rec = json.load(f, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert rec["edges"] == [0.25, 0.5, 0.75] and rec["labels"] == ["< 0.25", "[0.25, 0.5)", "[0.5, 0.75)", ">= 0.75"]
    assert (rec["variable"], rec["in_shape"], rec["out_shape"]) == ("lowres", [16, 16], [64, 64])
    assert sum(rec["members"]) == 4 * 64 * 64 and sum(rec["pairs"]) == 4 * 64 * 64 - 1 and rec["unclassified"] == 0
    (p, a) = (np.asarray(test["model_output"].values)[:, 0], np.asarray(test["hires"].values, dtype=np.float64)[:, 0])
    k = strata_of(on_target_grid(np.asarray(test["lowres"].values, dtype=np.float64)[:, 0], 64, 64), rec["edges"])
    ok = np.isfinite(p) & np.isfinite(a)
    for j in range(4):
        at = ok & (k == j)
        assert rec["pairs"][j] == int(at.sum()) and abs(rec["bias"][j] - (p[at] - a[at]).mean()) < 1e-12
        assert abs(rec["correlation"][j] - np.corrcoef(p[at], a[at])[0, 1]) < 1e-12
    assert abs(rec["pooled"]["rmse"] - math.sqrt(((p[ok] - a[ok]) ** 2).mean())) < 1e-12
    lines = [ln for ln in printed if ln.startswith("strata ")]
    assert len(lines) == 2 and lines[0] == strata.line("test", rec) and lines[1].startswith("strata train: lowres, 4 strata, rmse ")
    with open(os.path.join(out, "index.html")) as f:
        page = f.read()
    assert page.count("<h2>Skill by stratum</h2>") == 1
    assert page.count('alt="test skill by stratum"') == 1 and page.count('alt="train skill by stratum"') == 1


def test_build_html_one_value_per_case_and_a_missing_variable(model, tmp_path, monkeypatch):  # noqa: F811
    out = str(tmp_path / "report")
    (train, test, calls, printed) = _build(model, out, monkeypatch, strata_variable="time", strata_edges=[9.0])
    with open(os.path.join(out, "strata_train.json")) as f:
        rec = json.load(f)
    # the cases at 0 and 6 hours, then those at 12, 18 and 24
    assert rec["members"] == [2 * 64 * 64, 3 * 64 * 64] and rec["in_shape"] == [1, 1] and rec["labels"] == ["< 9", ">= 9"]
    assert not any("case_range" in c for c in calls.log)
    assert "strata train: time, 2 strata, rmse " in printed[-1]
    for (name, text) in (("elevation", "strata variable 'elevation' is not a variable of the test data set"), ("y", "strata variable 'y'")):
        with pytest.raises(ValueError, match=text):
            _build(model, str(tmp_path / name), monkeypatch, strata_variable=name)
    with pytest.raises(ValueError, match="strata_channel 1 is not a channel of 'lowres', which has 1"):
        _build(model, str(tmp_path / "channel"), monkeypatch, strata_variable="lowres", strata_channel=1)
