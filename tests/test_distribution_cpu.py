"""The host arithmetic of the value distributions (cae_tools_amd/utils/distribution.py) on counts made by hand and by the
numpy restatement of cae_joint_hist (distribution_ref.py): the quantile rule against numpy's inverted_cdf quantile, the
marginals, the contingency counts, the distances, the conditional slope, strict JSON, the report section and the command's
flags.  No GPU.

The quantile rule: with r = q n, the first fine bin k with cum[k] >= r and a count holds the sample of rank ceil(r), which is
what np.quantile(..., method="inverted_cdf") returns, and the rule's value lies in that bin: the two differ by at most one
fine bin width w.  The margin 1e-9 w covers the rounding of the bin edges lo + w k (a few 2^-53 of hi).  Over 200 seeded
draws of 1 to 5000 values the largest difference seen was 0.99 w."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

from cae_tools_amd.utils import distribution, report
from distribution_ref import Reference, fine_bins

HERE = os.path.dirname(os.path.abspath(__file__))


def _counts(p, a, lo, hi, n_bin, sub):
    ref = Reference(p, a, lo, hi, n_bin, sub)
    return ref.joint, ref.marg, ref.cond, ref.outside


def test_quantile_rule_against_inverted_cdf():
    rng = np.random.default_rng(11)
    worst = 0.0
    for draw in range(200):
        n = int(rng.integers(1, 5001))
        (n_bin, sub) = ((1, 2, 7, 128)[draw % 4], (1, 3, 32)[(draw // 4) % 3])
        (lo, hi) = (float(rng.normal()), 0.0)
        hi = lo + float(rng.uniform(0.5, 20.0))
        kind = draw % 3
        if kind == 0:
            v = rng.uniform(lo, hi, n)
        elif kind == 1:
            v = np.clip(rng.normal(0.5 * (lo + hi), 0.2 * (hi - lo), n), lo, hi)
        else:
            v = np.clip(np.round(rng.uniform(lo, hi, n), 1), lo, hi)       # many ties
        n_fine = n_bin * sub
        count = np.bincount(fine_bins(v, lo, hi, n_bin, sub), minlength=n_fine)
        w = (hi - lo) / n_fine
        for q in distribution.QUANTILES:
            got = distribution.quantile_from_counts(count, lo, hi, q)
            want = float(np.quantile(v, q, method="inverted_cdf"))
            worst = max(worst, abs(got - want) / w)
            assert abs(got - want) <= w * (1 + 1e-9), (draw, n, n_bin, sub, q, got, want)
    print(f"quantile rule: largest |got - inverted_cdf| = {worst:.3f} fine bin widths")
    assert math.isnan(distribution.quantile_from_counts(np.zeros(8, dtype=np.int64), 0.0, 1.0, 0.5))
    # one value: every quantile is in its bin
    one = np.zeros(10, dtype=np.int64)
    one[3] = 1
    assert 0.3 < distribution.quantile_from_counts(one, 0.0, 1.0, 0.01) <= 0.4 + 1e-12


@pytest.fixture(scope="module")
def damped():
    """a target with a broad distribution and a prediction regressed half way to the mean, plus noise"""
    rng = np.random.default_rng(5)
    a = rng.normal(300.0, 4.0, 40000)
    p = 300.0 + 0.5 * (a - 300.0) + rng.normal(0.0, 0.3, a.size)
    (lo, hi) = (float(min(a.min(), p.min())), float(max(a.max(), p.max())))
    return p, a, lo, hi


def test_marginals_and_contingency_add_up(damped):
    (p, a, lo, hi) = damped
    for (n_bin, sub) in ((128, 8), (7, 3), (1, 1)):
        (joint, marg, cond, outside) = _counts(p, a, lo, hi, n_bin, sub)
        curves = distribution.curves_from_counts(joint, marg, cond, outside, lo, hi, n_pixels=a.size + 5)
        assert curves["pairs"] == a.size and curves["pixels_left_out"] == 5 and (curves["n_bin"], curves["sub"]) == (n_bin, sub)
        # the coarse marginals from the joint counts are the summed fine marginals
        assert np.array_equal(joint.sum(axis=1), marg[0].reshape(n_bin, sub).sum(axis=1))
        assert np.array_equal(joint.sum(axis=0), marg[1].reshape(n_bin, sub).sum(axis=1))
        assert curves["target_count"] == joint.sum(axis=1).tolist() and curves["prediction_count"] == joint.sum(axis=0).tolist()
        assert len(curves["edges"]) == n_bin + 1 and curves["edges"][0] == lo and abs(curves["edges"][-1] - hi) <= 1e-12 * abs(hi)
        assert [t["q"] for t in curves["exceedance"]] == [0.05, 0.9, 0.95, 0.99]
        for t in curves["exceedance"]:
            assert t["hits"] + t["misses"] + t["false_alarms"] + t["correct_negatives"] == a.size
            assert 0 <= t["edge"] <= n_bin
            event = (fine_bins(a, lo, hi, n_bin, sub) // sub >= t["edge"]) == (t["side"] == "above")
            assert t["hits"] + t["misses"] == int(event.sum())
            if n_bin == 128:
                assert abs(t["fraction"] - t["q"]) < 0.02 and 0 <= t["pod"] < 1 and t["frequency_bias"] < 1
                # the damped prediction is too warm in the cold tail and too cold in the warm tail
                assert (t["tail_bias"] > 0) == (t["side"] == "below")
                assert t["tail_bias"] == pytest.approx(float((p - a)[event].mean()), rel=1e-9)
        if n_bin == 1:
            t = curves["exceedance"][1]
            assert (t["edge"], t["fraction"]) == (1, 1.0) and math.isnan(t["pod"]) and math.isnan(t["tail_bias"])
    # ties go to the lower edge: two bins of equal count, q = 0.5 is met by edge 1 alone; q = 0.25 lies between edges 0 and 1
    joint = np.array([[5, 0], [0, 5]])
    cond = np.zeros((2, 2, 4))
    assert distribution.contingency(joint, cond, 0.0, 2.0, 0.5, "above")["edge"] == 1
    assert distribution.contingency(joint, cond, 0.0, 2.0, 0.25, "above")["edge"] == 0
    got = distribution.contingency(joint, cond, 0.0, 2.0, 0.5, "above")
    assert (got["value"], got["hits"], got["misses"], got["false_alarms"], got["pod"], got["far"], got["csi"]) == (1.0, 5, 0, 0, 1.0, 0.0, 1.0)


def test_distances_of_identical_marginals(damped):
    (p, a, lo, hi) = damped
    curves = distribution.curves_from_counts(*_counts(a, a, lo, hi, 64, 4), lo, hi)
    assert curves["wasserstein1"] == 0.0 and curves["perkins_score"] == 1.0 and curves["perkins_bins"] == 64
    assert curves["quantile_difference"] == [0.0] * len(distribution.QUANTILES)
    assert all(t["pod"] == 1.0 and t["far"] == 0.0 and t["csi"] == 1.0 and t["frequency_bias"] == 1.0 for t in curves["exceedance"])
    shifted = distribution.curves_from_counts(*_counts(a + 1.0, a, lo, hi + 1.0, 64, 4), lo, hi + 1.0)
    # a shift by s moves every quantile by s: W1 = s up to the fine bin width
    w = (hi + 1.0 - lo) / 256
    assert abs(shifted["wasserstein1"] - 1.0) <= w and 0 < shifted["perkins_score"] < 1
    assert all(abs(d - 1.0) <= 2 * w for d in shifted["quantile_difference"])


def test_conditional_slope(damped):
    (p, a, lo, hi) = damped
    same = distribution.curves_from_counts(*_counts(a, a, lo, hi, 128, 8), lo, hi)
    assert same["conditional_slope"] == pytest.approx(1.0, abs=1e-12)
    mean = float(a.mean())
    half = mean + 0.5 * (a - mean)
    curves = distribution.curves_from_counts(*_counts(half, a, lo, hi, 128, 8), lo, hi)
    # the bin means of p are mean + (bin mean of a - mean) / 2 up to the rounding of the sums: the slope is 0.5
    assert curves["conditional_slope"] == pytest.approx(0.5, abs=1e-9)
    assert all(b is None or math.isnan(b) or abs(b - 0.5 * (mean - m)) < 1e-9 for (b, m) in zip(curves["bias"], curves["mean_target"]))
    noisy = distribution.curves_from_counts(*_counts(p, a, lo, hi, 128, 8), lo, hi)
    assert 0.45 < noisy["conditional_slope"] < 0.55
    # reliability: the mean target given the prediction follows p = 300 + (a - 300) / 2 backwards, slope about 2 / (1 + noise)
    assert math.isnan(distribution.curves_from_counts(np.zeros((4, 4)), np.zeros((2, 8)), np.zeros((2, 4, 4)), np.zeros(4), 0.0, 1.0)
                      ["conditional_slope"])
    one_bin = distribution.curves_from_counts(*_counts(a, a, lo, hi, 1, 1), lo, hi)
    assert math.isnan(one_bin["conditional_slope"])


def test_json_is_strict_and_the_line(tmp_path, damped):
    (p, a, lo, hi) = damped
    curves = distribution.curves_from_counts(*_counts(p, a, lo, hi, 16, 2), lo, hi, n_pixels=a.size)
    path = distribution.write_json(str(tmp_path / "distribution_test.json"), curves)
    text = open(path).read()
    assert "NaN" not in text and "Infinity" not in text
    back = json.loads(text, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert back["pairs"] == a.size and back["pixels_left_out"] == 0 and back["summary"]["perkins_bins"] == 16
    assert np.asarray(back["joint"]).shape == (16, 16) and len(back["marginal_target"]) == 32
    s = distribution.summary(curves)
    line = distribution.line("test", curves)
    assert line == (f"distribution test: slope {s['conditional_slope']:.6g}, q95 bias {s['q95_bias']:.6g}, W1 {s['wasserstein1']:.6g}, "
                    f"Perkins {s['perkins_score']:.6g}, POD/FAR at q95 {s['pod_q95']:.6g}/{s['far_q95']:.6g}")
    # nothing counted: every score is NaN in memory and null in the file
    empty = distribution.curves_from_counts(np.zeros((4, 4)), np.zeros((2, 8)), np.zeros((2, 4, 4)), np.zeros(4), 0.0, 1.0, n_pixels=9)
    assert empty["pairs"] == 0 and empty["pixels_left_out"] == 9 and math.isnan(empty["wasserstein1"])
    back = json.loads(open(distribution.write_json(str(tmp_path / "e.json"), empty)).read(),
                      parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert back["wasserstein1"] is None and back["perkins_score"] is None and back["bias"] == [None] * 4
    assert back["quantile_target"] == [None] * 9 and back["exceedance"][2]["pod"] is None and back["summary"]["q95_bias"] is None
    assert distribution.line("train", empty) == ("distribution train: slope none, q95 bias none, W1 none, Perkins none, "
                                                 "POD/FAR at q95 none/none")
    page = distribution.write_page(str(tmp_path / "distribution"), [("test", curves), ("train", empty)])
    html = open(page).read()
    assert html.count('class="distribution"') == 2 and html.count('alt="test joint density"') == 1
    for title in ("conditional bias", "reliability", "Q-Q", "marginals"):
        assert html.count(f'alt="test {title}"') == 1
    assert distribution.density_png(curves["joint"])[:8] == b"\x89PNG\r\n\x1a\n"


def test_cli_flags_are_evaluate_cae_plus_one():
    from cae_tools_amd.cli import distribution as cli, evaluate_cae
    flags = lambda parser: [(a.option_strings, a.dest, a.nargs, a.default, a.required)   # noqa: E731
                            for a in parser._actions if a.option_strings and a.dest != "help"]
    (mine, theirs) = (flags(cli.build_parser()), flags(evaluate_cae.build_parser()))
    assert mine[:len(theirs)] == theirs
    assert [f[0] for f in mine[len(theirs):]] == [["--distribution-bins"]]
    assert cli.build_parser().parse_args(["--model-folder", "m"]).distribution_bins == 128
    assert cli.build_parser().parse_args(["--model-folder", "m", "--distribution-bins", "1"]).distribution_bins == 1
    for bad in ("0", "129", "x"):
        with pytest.raises(SystemExit):
            cli.build_parser().parse_args(["--model-folder", "m", "--distribution-bins", bad])


# sha256 of evaluation_report's page for the golden record, as test_baseline_cpu.py holds it
REPORT_SHA256 = "0a26c705f2bab559c1df1dee37ad957c941d84ce2aa0652d349c3549845789f1"


def test_report_section_is_off_by_default(damped):
    (p, a, lo, hi) = damped
    with open(os.path.join(HERE, "golden", "report_layout.json")) as f:
        rec = json.load(f)["record"]
    rng = np.random.default_rng(7)
    measures = [(part, {m: rng.random(20) for m in rec["measures"]}) for part in rec["partitions"]]
    page = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"])
    assert hashlib.sha256(page.encode("utf-8")).hexdigest() == REPORT_SHA256
    assert page == report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], distribution=None)
    assert "Value distribution" not in page
    curves = distribution.curves_from_counts(*_counts(p, a, lo, hi, 16, 2), lo, hi, n_pixels=a.size + 3)
    with_section = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"],
                                            distribution=([("test", curves)], "distribution/index.html"))
    assert with_section.count("<h2>Value distribution</h2>") == 1
    assert f"test: {a.size} pixel pairs, 16 bins over [{lo:.6g}, {hi:.6g}]" in with_section
    assert '<a href="distribution/index.html">' in with_section
    s = distribution.summary(curves)
    for cell in ("<td>Perkins score</td>", f"<td>{s['perkins_score']:.6g}</td>", f"<td>{s['conditional_slope']:.6g}</td>",
                 "<td>bins of the Perkins score</td>", "<td>16</td>", f"<td>{a.size} / 3 / 0</td>"):
        assert cell in with_section, cell
    assert with_section.count("<img") == page.count("<img")
    start = with_section.index("<h2>Value distribution</h2>")
    end = with_section.index("<h2>Training Summary</h2>")
    assert with_section[:start] + with_section[end:] == page


def test_the_library_exports_the_joint_hist_entry_points():
    from cae_tools_amd import _lib, engine
    lib = _lib.load()
    for name in ("cae_joint_hist", "cae_joint_hist_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert callable(engine.joint_histogram)
    # one partial of 2 x n_bin x 4 doubles per workgroup; a workgroup per four (case, 4096-element chunk) items, at most 1024
    assert lib.cae_joint_hist_workspace_bytes(1, 1, 1, 1) == 64
    assert lib.cae_joint_hist_workspace_bytes(3, 4097, 128, 8) == 2 * 64 * 128
    assert lib.cae_joint_hist_workspace_bytes(2000, 65536, 128, 8) == 1024 * 64 * 128
    for bad in ((0, 4, 8, 8), (-1, 4, 8, 8), (1, 0, 8, 8), (1, 4, 0, 8), (1, 4, 129, 8), (1, 4, 8, 0), (1, 4, 8, 33), (1 << 20, 1 << 20, 8, 8)):
        assert lib.cae_joint_hist_workspace_bytes(*bad) == 0
