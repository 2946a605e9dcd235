"""The host side of the prediction intervals (cae_tools_amd/utils/conformal.py, cli/calibrate.py, apply_cae --interval): the
rank rule against Fractions, level parsing and its refusals, the calibration record's round trip with +inf, the numpy
restatement's own identities, and the command-line refusals that are decided before the GPU is touched."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import conformal_ref
from cae_tools_amd.utils import conformal

LEVELS = [Fraction(1, 2), Fraction(4, 5), Fraction(9, 10), Fraction(19, 20), Fraction(999999, 1000000)]


def test_rank_rule_is_the_ceiling():
    for level in LEVELS:
        for n in range(301):
            want = math.ceil((n + 1) * level)
            assert conformal.rank(n, level) == want == conformal_ref.rank(n, level)
    # the first finite ranks the documents name
    assert [min(n for n in range(400) if conformal.rank(n, v) <= n) for v in LEVELS[:4]] == [1, 4, 9, 19]
    assert conformal.rank(0, Fraction(1, 2)) == 1 and conformal.rank(999998, LEVELS[4]) == 999999


def test_level_parsing_is_exact():
    assert conformal.parse_levels(["0.9", ".95", "0.999999"]) == [Fraction(9, 10), Fraction(19, 20), Fraction(999999, 1000000)]
    assert conformal.parse_levels(list(conformal.DEFAULT_LEVELS)) == [Fraction(4, 5), Fraction(9, 10), Fraction(19, 20)]
    assert conformal.parse_level(" 0.90 ") == Fraction(9, 10) == conformal.parse_level("9/10") == conformal.parse_level(Fraction(9, 10))
    assert Fraction(0.9) != Fraction(9, 10)       # why no level passes through a float
    assert conformal.level_text(Fraction(18, 20)) == "9/10"


@pytest.mark.parametrize("bad", ["0", "1", "1e-7", "nan", "inf", "-0.5", "1.5", "", "ninety", "0.9999999", 0.9, None])
def test_levels_refused(bad):
    with pytest.raises(ValueError):
        conformal.parse_level(bad)


@pytest.mark.parametrize("bad", [["0.9", "0.8"], ["0.9", "0.90"], ["0.5", "0.9", "9/10"], [], ["0.1"] * 9,
                                 ["0.1", "0.2", "0.3", "0.4", "0.5", "0.6", "0.7", "0.8", "0.9"]])
def test_level_lists_refused(bad):
    with pytest.raises(ValueError):
        conformal.parse_levels(bad)


def test_group_names():
    assert conformal.GROUPS == {"pixel": 0, "pooled": 1}
    with pytest.raises(ValueError):
        conformal.check_group("case")


def _pixel_calibration(rng, levels, shape=(3, 5)):
    (h, w) = shape
    q = np.sort(rng.random((len(levels), h, w)), axis=0)
    q[-1, 0, 0] = np.inf
    q[:, 1, 2] = np.inf
    n = rng.integers(0, 40, size=(h, w))
    return q, n


def test_record_round_trip_pixel(tmp_path):
    rng = np.random.default_rng(5)
    levels = conformal.parse_levels(["0.8", "0.9", "0.95"])
    (q, n) = _pixel_calibration(rng, levels)
    pooled = np.array([0.25, 1.0 / 3.0, np.inf])
    record = conformal.make_record("pixel", levels, "hires", "spread", 40, q, n, pooled, coverage=([70, 80, 90], 100))
    paths = conformal.write_record(str(tmp_path), record, q=q, n=n, shape=(3, 5))
    assert sorted(os.path.basename(p) for p in paths) == ["calibration.json", "calibration.nc"]
    with open(tmp_path / "calibration.json") as f:
        text = f.read()
    assert "Infinity" not in text and "NaN" not in text
    stored = json.loads(text)
    assert stored["levels"] == ["4/5", "9/10", "19/20"] and stored["pooled_quantiles"][2] is None
    assert (stored["group"], stored["output_variable"], stored["scale_variable"], stored["cases"]) == ("pixel", "hires", "spread", 40)
    assert (stored["n_min"], stored["n_median"], stored["n_max"]) == (int(n.min()), float(np.median(n)), int(n.max()))
    assert stored["test_coverage"] == [0.7, 0.8, 0.9] and stored["test_pairs"] == 100
    back = conformal.read_record(str(tmp_path))
    assert back["levels"] == levels
    assert np.array_equal(np.array(back["pooled_quantiles"]).view(np.uint64), pooled.view(np.uint64))
    assert back["quantile"].dtype == np.float64 and np.array_equal(back["quantile"].view(np.uint64), q.view(np.uint64))
    assert np.array_equal(back["count"], n)
    assert back["finite_groups"] == [int(np.isfinite(row).sum()) for row in q] and back["groups"] == 15
    lines = conformal.summary_lines(back)
    assert len(lines) == 3 and lines[0].startswith("calibrate 4/5 pixel: ") and "held-out coverage 70/100 = 0.7" in lines[0]


def test_record_round_trip_pooled(tmp_path):
    levels = conformal.parse_levels(["0.5", "0.999999"])
    q = np.array([0.1 + 0.2, np.inf])
    (tmp_path / "calibration.nc").write_bytes(b"left by an earlier pixel calibration")
    record = conformal.make_record("pooled", levels, "hires", None, 7, q, np.int64(7 * 12), q)
    conformal.write_record(str(tmp_path), record)
    assert sorted(os.listdir(tmp_path)) == ["calibration.json"]
    back = conformal.read_record(str(tmp_path))
    assert back["pooled_quantiles"][0] == 0.1 + 0.2 and back["pooled_quantiles"][1] == math.inf
    assert back["scale_variable"] is None and "quantile" not in back and "test_coverage" not in back
    assert back["finite_groups"] == [1, 0] and back["median_q"] == [0.1 + 0.2, math.inf]
    assert conformal.summary_lines(back) == ["calibrate 1/2 pooled: 1/1 groups finite, median q 0.3",
                                             "calibrate 999999/1000000 pooled: 0/1 groups finite, median q inf"]


def test_interval_request(tmp_path):
    levels = conformal.parse_levels(["0.8", "0.9"])
    q = np.array([1.0, 2.0])
    conformal.write_record(str(tmp_path), conformal.make_record("pooled", levels, "hires", "spread", 30, q, np.int64(30), q))
    (record, index, names) = conformal.interval_request(str(tmp_path), "0.90", "spread", None, "pred")
    assert index == 1 and names == ("pred_lower", "pred_upper") and record["pooled_quantiles"] == [1.0, 2.0]
    assert conformal.interval_request(str(tmp_path), Fraction(4, 5), "spread", ["lo", "hi"])[1:] == (0, ("lo", "hi"))
    for (level, scale, names) in (("0.95", "spread", None), ("0.9", None, None), ("0.9", "other", None), ("0.9", "spread", ["a", "a"]),
                                  ("0.9", "spread", ["a"]), ("0.9", "spread", ["model_output", "b"]), ("0.899999", "spread", None)):
        with pytest.raises(ValueError):
            conformal.interval_request(str(tmp_path), level, scale, names)
    with pytest.raises(FileNotFoundError):
        conformal.interval_request(str(tmp_path / "nowhere"), "0.9")


def test_restatement_identities():
    """the restatement against its own definition: the k-th smallest has at least k scores at or below it and fewer than k
    below it; the pooled quantile of one pixel's scores is that pixel's"""
    rng = np.random.default_rng(11)
    (p, a) = (rng.random((25, 1, 4, 6)), rng.random((25, 2, 4, 6)))
    a[:, 0][rng.random((25, 4, 6)) < 0.2] = np.nan
    a[:, 0, 0, 0] = np.nan
    s = rng.random((25, 1, 4, 6)) - 0.1
    levels = ["1/2", "9/10", "19/20"]
    for scale in (None, s):
        (q, n) = conformal_ref.quantiles(p, a, levels, "pixel", scale)
        assert n[0, 0] == 0 and np.isinf(q[:, 0, 0]).all() and np.isfinite(q[0]).mean() > 0.5
        k = np.array([[[conformal_ref.rank(v, level) for v in row] for row in n] for level in levels])
        (le, n2) = conformal_ref.counts(p, a, q, "pixel", scale)
        (lt, _) = conformal_ref.counts(p, a, q, "pixel", scale, strict=True)
        fin = np.isfinite(q)
        assert np.array_equal(n, n2) and (le[fin] >= k[fin]).all() and (lt[fin] < k[fin]).all() and (k[~fin] > np.broadcast_to(n, k.shape)[~fin]).all()
        assert (q[1:] >= q[:-1]).all()
        (q1, n1) = conformal_ref.quantiles(p[:, :, 2:3, 3:4], a[:, :, 2:3, 3:4], levels, "pooled", None if scale is None else scale[:, :, 2:3, 3:4])
        assert np.array_equal(q1, q[:, 2, 3]) and n1 == n[2, 3]
    (lo, hi) = conformal_ref.bounds(p, np.inf, s)
    ok = s[:, 0] > 0
    assert np.isnan(lo[~ok]).all() and (lo[ok] == -np.inf).all() and (hi[ok] == np.inf).all()


# ---- command lines, refused before the GPU is touched ---------------------------------------------------

@pytest.fixture
def folder(tmp_path):
    """a model folder as far as the refusals look at it: parameters.json and a pooled calibration for 0.8 and 0.9 with a scale"""
    (tmp_path / "parameters.json").write_text(json.dumps({"type": "ConvAEModel"}))
    levels = conformal.parse_levels(["0.8", "0.9"])
    q = np.array([1.0, 2.0])
    conformal.write_record(str(tmp_path), conformal.make_record("pooled", levels, "hires", "spread", 30, q, np.int64(30), q))
    return str(tmp_path)


def _refused(argv):
    from cae_tools_amd.cli import apply_cae
    with pytest.raises(SystemExit) as stop:
        apply_cae.main(argv)
    assert stop.value.code not in (0, None)
    return str(stop.value.code)


def test_apply_refuses_interval_without_calibration(tmp_path):
    (tmp_path / "parameters.json").write_text(json.dumps({"type": "ConvAEModel"}))
    assert "calibration.json" in _refused(["in.nc", "out.nc", "--model-folder", str(tmp_path), "--interval", "0.9"])


def test_apply_refuses_uncalibrated_level(folder):
    assert "was not calibrated" in _refused(["in.nc", "out.nc", "--model-folder", folder, "--interval", "0.95", "--scale-variable", "spread"])
    assert "not between 0 and 1" in _refused(["in.nc", "out.nc", "--model-folder", folder, "--interval", "1", "--scale-variable", "spread"])


def test_apply_refuses_mismatched_scale(folder):
    assert "differs from the calibrated one" in _refused(["in.nc", "out.nc", "--model-folder", folder, "--interval", "0.9"])
    assert "differs from the calibrated one" in _refused(["in.nc", "out.nc", "--model-folder", folder, "--interval", "0.9",
                                                          "--scale-variable", "sigma"])


def test_apply_refuses_interval_options_without_interval(folder):
    assert "need --interval" in _refused(["in.nc", "out.nc", "--model-folder", folder, "--interval-variables", "lo", "hi"])
    assert "need --interval" in _refused(["in.nc", "out.nc", "--model-folder", folder, "--scale-variable", "spread"])


def test_calibrate_refuses_levels_and_folders(tmp_path, capsys):
    from cae_tools_amd.cli import calibrate
    base = ["--calibration-inputs", "c.nc", "--output-variable", "hires", "--model-folder", str(tmp_path)]
    for coverage in (["0.9", "0.8"], ["1"], ["0.9", "0.9"], ["nan"]):
        with pytest.raises(SystemExit) as stop:
            calibrate.main(base + ["--coverage", *coverage])
        assert stop.value.code == 2
    capsys.readouterr()
    with pytest.raises(SystemExit) as stop:
        calibrate.main(base)
    assert "no trained model" in str(stop.value.code)
    args = calibrate.build_parser().parse_args(base)
    assert args.coverage == ["0.8", "0.9", "0.95"] and args.group == "pooled" and args.scale_variable is None and args.test_inputs is None


def test_apply_keywords_refused_by_the_models_before_any_work():
    """apply(interval=...) without a folder, and the interval options without interval"""
    from cae_tools_amd.models.base_model import BaseModel
    model = BaseModel()
    with pytest.raises(ValueError, match="needs the model folder"):
        model._interval_request("0.9", None, None, "model_output")
    with pytest.raises(ValueError, match="need interval"):
        model._interval_request(None, ["a", "b"], None, "model_output")
    assert model._interval_request(None, None, None, "model_output") is None
