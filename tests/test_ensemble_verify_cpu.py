"""The host half of the ensemble verification, without a GPU: utils/ensemble_scores.py against the definition
(tests/ensemble_verify_ref.py) and against answers worked out by hand, the verify_ensemble command's flags and its refusal
of a folder that holds no VAE, and the report's "Ensemble verification" section.  The kernel's half is
tests/test_ensemble_verify_gpu.py, the model's tests/test_vae_verify_gpu.py."""
import json
import os
import re
import warnings

import numpy as np
import pytest

import ensemble_verify_ref as ref
from golden.make_golden_report import report_items
from test_evaluator_cpu import _bar_counts, _golden, _model_folder, _svgs
from cae_tools_amd.utils import ensemble_scores, report


def test_scores_follow_the_formulas_on_random_sums():
    rng = np.random.default_rng(4)
    for k in (2, 3, 16, 64):
        sums = rng.random((9, 5)) * [0, 5.0, 1.0, 9.0, 4.0]
        sums[:, 0] = rng.integers(1, 1000, size=9)
        sums[4] = 0.0                                            # a case without a counted pixel
        ranks = np.append(rng.integers(0, 500, size=k + 1), 17)
        got = ensemble_scores.scores_from_sums(sums, ranks, k)
        (n, a, b, e, v) = sums.sum(axis=0)
        assert got["n"] == int(n) and got["ensemble_size"] == k and got["tied"] == 17
        assert got["crps"] == pytest.approx((a - b) / n, rel=1e-15)
        assert got["fair_crps"] == pytest.approx((a - b * k / (k - 1)) / n, rel=1e-15)
        assert got["rmse_mean"] == pytest.approx(np.sqrt(e / n), rel=1e-15)
        assert got["spread"] == pytest.approx(np.sqrt(v / n), rel=1e-15)
        assert got["spread_skill"] == pytest.approx(np.sqrt((k + 1) / k) * np.sqrt(v / n) / np.sqrt(e / n), rel=1e-14)
        assert got["rank_counts"] == ranks[:k + 1].tolist()
        np.testing.assert_allclose(got["rank_frequencies"], ranks[:k + 1] / ranks[:k + 1].sum(), rtol=1e-15)
        assert sum(got["rank_frequencies"]) == pytest.approx(1.0)
        case = got["case_crps"]
        assert np.isnan(case[4]) and np.isfinite(np.delete(case, 4)).all()
        np.testing.assert_allclose(np.delete(case, 4), np.delete((sums[:, 1] - sums[:, 2]) / np.where(sums[:, 0] > 0, sums[:, 0], 1), 4),
                                   rtol=1e-15)
        with pytest.raises(ValueError):
            ensemble_scores.scores_from_sums(sums, ranks[:-1], k)
    with pytest.raises(ValueError):
        ensemble_scores.scores_from_sums(np.zeros((1, 5)), np.zeros(3), 1)


def test_scores_of_the_definition_on_draws():
    """the whole chain on the CPU: draws -> the definition's sums -> scores; crps of an ensemble against the sample formula
    mean_k |m_k - a| - 1/(2 K^2) sum_{i,j} |m_i - m_j|"""
    rng = np.random.default_rng(9)
    (n_case, k, plane) = (3, 7, 50)
    y = rng.random((n_case, k, plane)).astype(np.float32)
    a = 280.0 + 10.0 * rng.random((n_case, plane))
    (sums, ranks, _) = ref.verify(y, a, 280.0, 10.0)
    got = ensemble_scores.scores_from_sums(sums, ranks, k)
    m = 280.0 + y.astype(np.float64) * 10.0
    crps = np.abs(m - a[:, None, :]).mean(axis=1) - np.abs(m[:, :, None, :] - m[:, None, :, :]).sum(axis=(1, 2)) / (2 * k * k)
    assert got["n"] == n_case * plane and got["tied"] == 0
    assert got["crps"] == pytest.approx(crps.mean(), rel=1e-12)
    np.testing.assert_allclose(got["case_crps"], crps.mean(axis=1), rtol=1e-12)
    assert got["rmse_mean"] == pytest.approx(np.sqrt(((m.mean(axis=1) - a) ** 2).mean()), rel=1e-12)
    assert got["spread"] == pytest.approx(np.sqrt(m.var(axis=1, ddof=1).mean()), rel=1e-9)
    assert got["rank_counts"] == np.bincount((m < a[:, None, :]).sum(axis=1).reshape(-1), minlength=k + 1).tolist()


def test_known_answers():
    # all members equal to the target: crps 0, every pixel tied at rank 0
    y = np.full((2, 5, 6), 0.375, dtype=np.float32)
    a = np.full((2, 6), 288.0 + 0.375 * 10.5)
    (sums, ranks, _) = ref.verify(y, a, 288.0, 10.5)
    got = ensemble_scores.scores_from_sums(sums, ranks, 5)
    assert got["crps"] == 0.0 and got["fair_crps"] == 0.0 and got["rmse_mean"] == 0.0 and got["spread"] == 0.0
    assert got["rank_counts"] == [12, 0, 0, 0, 0, 0] and got["tied"] == 12 and (got["case_crps"] == 0.0).all()
    assert np.isnan(got["spread_skill"])
    # K = 2 by hand: members 0.25 and 0.75, target 0.5: A = (0.25 + 0.25) / 2, B = 0.5 / 4, one member below
    y = np.array([[[0.25], [0.75]]], dtype=np.float32)
    (sums, ranks, _) = ref.verify(y, np.array([[0.5]]), 0.0, 1.0)
    assert sums.tolist() == [[1.0, 0.25, 0.125, 0.0, 0.125]] and ranks.tolist() == [0, 1, 0, 0]
    got = ensemble_scores.scores_from_sums(sums, ranks, 2)
    assert got["crps"] == 0.125 and got["fair_crps"] == 0.0 and got["spread"] == np.sqrt(0.125)
    # for one member the crps is the absolute error: A alone
    assert ensemble_scores.case_crps([[4.0, 6.0, 0.0, 0.0, 0.0]]).tolist() == [1.5]


def test_no_counted_pixel_gives_nan_without_a_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = ensemble_scores.scores_from_sums(np.zeros((3, 5)), np.zeros(6, dtype=np.int64), 4)
        skipped = ref.verify(np.full((1, 4, 3), np.nan, dtype=np.float32), np.zeros((1, 3)), 0.0, 1.0)
    for key in ("crps", "fair_crps", "rmse_mean", "spread", "spread_skill", "tied_fraction"):
        assert np.isnan(got[key]), key
    assert got["n"] == 0 and np.isnan(got["rank_frequencies"]).all() and np.isnan(got["case_crps"]).all()
    assert (skipped[0] == 0.0).all() and (skipped[1] == 0).all()


def test_json_record_is_strict_json():
    empty = ensemble_scores.scores_from_sums(np.zeros((2, 5)), np.zeros(5, dtype=np.int64), 3)
    text = json.dumps(ensemble_scores.json_record(empty), allow_nan=False)
    assert "NaN" not in text
    back = json.loads(text)
    assert back["crps"] is None and back["spread_skill"] is None and back["tied_fraction"] is None and back["n"] == 0
    assert back["rank_frequencies"] == [None] * 4 and back["case_crps"] == [None, None] and back["rank_counts"] == [0] * 4
    sums = np.array([[4.0, 6.0, 2.0, 8.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    some = ensemble_scores.scores_from_sums(sums, [1, 2, 1, 0, 3], 3)
    back = json.loads(json.dumps(ensemble_scores.json_record({**some, "case_sums": sums}, skip=("case_sums",)), allow_nan=False))
    assert "case_sums" not in back and back["crps"] == some["crps"] == 1.0 and back["case_crps"] == [1.0, None]
    assert back["rank_frequencies"] == some["rank_frequencies"] and back["tied"] == 3


def test_cli_flags_are_evaluate_cae_s_plus_two():
    from cae_tools_amd.cli import verify_ensemble
    names = [a.option_strings[0] for a in verify_ensemble.build_parser()._actions if a.option_strings and a.dest != "help"]
    assert names == _golden("evaluate_cae_flags.json") + ["--ensemble-size", "--ensemble-seed"]
    args = verify_ensemble.build_parser().parse_args(["--model-folder", "m", "--ensemble-size", "8"])
    assert (args.ensemble_size, args.ensemble_seed, args.output_html_folder) == (8, 0, "")
    with pytest.raises(SystemExit):
        verify_ensemble.build_parser().parse_args(["--model-folder", "m"])          # --ensemble-size is required


def test_cli_refuses_a_folder_without_a_vae_before_any_gpu_work(tmp_path, monkeypatch):
    from cae_tools_amd.cli import evaluate_cae, verify_ensemble
    _model_folder(str(tmp_path / "model"))

    def never(*args, **kwargs):
        raise AssertionError("the evaluator was started")

    monkeypatch.setattr(evaluate_cae, "run", never)
    argv = ["--model-folder", str(tmp_path / "model"), "--output-html-folder", str(tmp_path / "out"), "--ensemble-size", "4"]
    with pytest.raises(SystemExit, match="needs a VarAEModel folder.*holds a ConvAEModel"):
        verify_ensemble.main(argv)
    # the same folder called a VAE: the size is checked next, still before the evaluator
    with open(tmp_path / "model" / "parameters.json") as f:
        parameters = json.load(f)
    with open(tmp_path / "model" / "parameters.json", "w") as f:
        json.dump({**parameters, "type": "VarAEModel"}, f)
    for size in ("1", "65"):
        with pytest.raises(SystemExit, match="from 2 to 64"):
            verify_ensemble.main(argv[:-1] + [size])
    assert not os.path.exists(tmp_path / "out")


def test_evaluator_refuses_an_ensemble_of_a_model_that_has_none(tmp_path):
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    _model_folder(str(tmp_path))
    with pytest.raises(ValueError, match="needs a VarAEModel"):
        ModelEvaluator(None, None, model_path=str(tmp_path), ensemble_size=4)
    for size in (1, 65, 2.5):
        with pytest.raises(ValueError, match="from 2 to 64"):
            ModelEvaluator(None, None, model_path=str(tmp_path), ensemble_size=size)


def test_verify_ensemble_checks_the_size_before_any_gpu_work():
    from cae_tools_amd.models.var_ae_model import VarAEModel
    for size in (1, 65, 3.5):
        with pytest.raises(ValueError, match="from 2 to 64"):
            VarAEModel().verify_ensemble(None, ["lowres"], "hires", size)


def _page(rec, ensemble):
    rng = np.random.default_rng(7)
    measures = [(p, {m: rng.random(20) for m in rec["measures"]}) for p in rec["partitions"]]
    return report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], ensemble=ensemble)


def test_report_without_an_ensemble_is_the_page_as_it_was():
    fixture = _golden("report_layout.json")
    page = _page(fixture["record"], None)
    assert report_items(page) == fixture["items"]
    rng = np.random.default_rng(7)
    rec = fixture["record"]
    measures = [(p, {m: rng.random(20) for m in rec["measures"]}) for p in rec["partitions"]]
    assert page == report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"])
    assert "Ensemble verification" not in page


def test_report_with_an_ensemble_has_the_section():
    fixture = _golden("report_layout.json")
    k = 4
    sums = np.array([[100.0, 60.0, 20.0, 50.0, 30.0], [0.0, 0.0, 0.0, 0.0, 0.0], [50.0, 20.0, 5.0, 10.0, 12.0]])
    ranks = [40, 30, 20, 35, 25, 6]
    record = ensemble_scores.scores_from_sums(sums, ranks, k)
    record["mae"] = 0.625
    page = _page(fixture["record"], [("test", record)])
    plain = _page(fixture["record"], None)
    items = report_items(page)
    assert ["h2", "Ensemble verification"] in items
    assert ["h3", "test: 4 members, 150 pixels, 6 tied"] in items
    at = items.index(["h2", "Ensemble verification"])
    end = at + 3 + len(report.ENSEMBLE_ROWS) + 2                    # h2, h3, the header row, the rows, two images
    assert items[at + 3 + len(report.ENSEMBLE_ROWS):end] == [["img", ""], ["img", ""]]
    assert items[:at] + items[end:] == report_items(plain)
    rows = [i[1] for i in items[at + 2:at + 3 + len(report.ENSEMBLE_ROWS)]]
    assert rows[0] == "Score Name|Score Value"
    assert [r.split("|")[0] for r in rows[1:]] == [label for (label, _) in report.ENSEMBLE_ROWS]
    assert rows[1] == "crps|" + f"{record['crps']:0.6g}" and rows[3].endswith("|0.625")
    (svgs, before) = (_svgs(page), _svgs(plain))
    assert len(svgs) == len(before) + 2
    extra = [s for s in svgs if s not in before]
    assert [int(c) for c in re.findall(r'<rect class="rank" data-count="(\d+)"', extra[0])] == ranks[:k + 1]
    assert sum(_bar_counts(extra[1])) == 2 and "1 non-finite values not shown" in extra[1]     # the case without a pixel
