"""evaluate_cae on the CPU: the report's layout against the reference's HTML builder (tests/golden/report_layout.json,
made by make_golden_report.py), the SVG histograms against numpy, the CLI's flags against the reference's, and the
evaluator's refusal of an input variable the model does not have.  The GPU half is tests/test_evaluator_gpu.py."""
import base64
import json
import os
import re

import numpy as np
import pytest

from golden.make_golden_report import report_items
from cae_tools_amd.utils import report

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def _svgs(page):
    """the inline SVG documents of a page, in order"""
    return [base64.b64decode(m).decode() for m in re.findall(r'src="data:image/svg\+xml;base64,([A-Za-z0-9+/=]+)"', page)]


def _bar_counts(svg):
    return [int(c) for c in re.findall(r'<rect class="bar" data-count="(\d+)"', svg)]


def test_report_layout_matches_the_reference_builder():
    fixture = _golden("report_layout.json")
    rec = fixture["record"]
    rng = np.random.default_rng(7)
    measures = [(p, {m: rng.random(20) for m in rec["measures"]}) for p in rec["partitions"]]
    page = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"])
    assert report_items(page) == fixture["items"]
    svgs = _svgs(page)
    assert len(svgs) == 5
    assert all(s.startswith("<svg") and s.rstrip().endswith("</svg>") for s in svgs)
    assert [sum(_bar_counts(s)) for s in svgs[:4]] == [20, 20, 20, 20]


def test_report_without_a_partition_or_history():
    metrics = {"test": {"mse": 1.0, "mae": 0.5}}
    page = report.evaluation_report(metrics, [("test", {"mae": [1.0], "mse": [2.0]})], {"type": "UNET"}, None)
    items = report_items(page)
    assert ["h3", "Train Metrics"] not in items and ["h3", "train"] not in items
    assert items[-1] == ["tr", "type|UNET"]
    assert ["tr", "total epochs|3"] not in items and len(_svgs(page)) == 2


def test_report_escapes_text():
    params = {"note": "<b>&\"quoted\"</b>"}
    page = report.evaluation_report({}, [], params, None)
    assert "<b>" not in page
    assert ["tr", 'note|<b>&"quoted"</b>'] in report_items(page)


@pytest.mark.parametrize("values", [
    np.random.default_rng(1).normal(size=1000),
    np.random.default_rng(2).exponential(size=257),
    np.array([3.25]),
    np.full(40, 0.125),
    np.concatenate([np.zeros(50), np.ones(3) * 1e6]),
    np.arange(7, dtype=np.float64),
])
def test_histogram_bars_equal_numpy(values):
    svg = report.svg_histogram(values, "mae")
    (counts, _) = np.histogram(values, bins="auto")
    assert _bar_counts(svg) == counts.tolist()


def test_histogram_leaves_out_non_finite_values():
    v = np.array([1.0, 2.0, np.nan, 2.5, np.inf, 3.0])
    svg = report.svg_histogram(v, "mse")
    (counts, _) = np.histogram(v[np.isfinite(v)], bins="auto")
    assert _bar_counts(svg) == counts.tolist()
    assert "2 non-finite values not shown" in svg
    assert _bar_counts(report.svg_histogram([np.nan], "mse")) == []


def test_history_plot_leaves_out_losses_that_are_not_positive():
    svg = report.svg_history({"nr_epochs": 4, "train_loss": [1.0, 0.1, 0.0, 0.01], "test_loss": [2.0, -1.0, 0.5, 0.2]})
    points = dict(re.findall(r'data-name="(\w+)" data-points="(\d+)"', svg))
    assert points == {"train": "3", "test": "3"}


def test_cli_flags_equal_the_reference():
    from cae_tools_amd.cli.evaluate_cae import build_parser
    names = [a.option_strings[0] for a in build_parser()._actions if a.option_strings and a.dest != "help"]
    assert names == _golden("evaluate_cae_flags.json")
    args = build_parser().parse_args(["--model-folder", "m"])
    assert args.output_html_folder == "" and args.prediction_variable is None


def _model_folder(path):
    """a ConvAEModel folder written without training (weights from the initialiser)"""
    import torch
    from cae_tools_amd.models.conv_ae_model import ConvAEModel
    from cae_tools_amd.models.model_sizer import create_model_spec
    torch.manual_seed(0)
    mt = ConvAEModel(fc_size=8, encoded_dim_size=2, nr_epochs=1)
    (mt.input_shape, mt.output_shape) = ((1, 16, 16), (1, 64, 64))
    mt.spec = create_model_spec(input_size=(16, 16), input_channels=1, output_size=(64, 64), output_channels=1)
    mt._modules()
    mt.normalisation_parameters = [{"lowres": 0.0}, {"lowres": 1.0}, 0.0, 1.0]
    mt.set_input_spec([{"name": "lowres", "shape": [1, 16, 16]}])
    mt.set_output_spec({"name": "hires", "shape": [1, 64, 64]})
    mt.save(path)
    return mt


def test_evaluator_refuses_an_input_the_model_does_not_have(tmp_path, capsys):
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    mt = _model_folder(str(tmp_path / "model"))
    with pytest.raises(Exception, match="requested sst is not a model input"):
        ModelEvaluator(None, None, model_path=str(tmp_path / "model"), input_variables=["lowres", "sst"])
    ev = ModelEvaluator(None, None, model_path=str(tmp_path / "model"), input_variables=["lowres"])
    assert f"Evaluating model id={mt.get_model_id()}" in capsys.readouterr().out
    assert (ev.output_variable, ev.model_output_variable, ev.output_html_path) == ("hires", "model_output", None)


def test_model_loader_knows_the_four_types(tmp_path):
    from cae_tools_amd.models.model_loader import load_model, model_classes
    assert sorted(model_classes()) == ["ConvAEModel", "LinearModel", "UNET", "VarAEModel"]
    _model_folder(str(tmp_path))
    assert type(load_model(str(tmp_path))).__name__ == "ConvAEModel"
    with open(tmp_path / "parameters.json", "w") as f:
        json.dump({"type": "SRCNN"}, f)
    with pytest.raises(SystemExit, match="SRCNN"):
        load_model(str(tmp_path))


def test_compute_measure_is_the_reference_formula(tmp_path):
    """compute_measure (one case, numpy) - what case_measures computes for every case at once on the GPU"""
    from cae_tools_amd.data.arrays import DataArray, Dataset
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    _model_folder(str(tmp_path))
    ev = ModelEvaluator(None, None, model_path=str(tmp_path))
    rng = np.random.default_rng(3)
    (p, a) = (rng.random((3, 2, 5, 4)), rng.random((3, 1, 5, 4)).astype(np.float32))
    ds = Dataset({"model_output": DataArray(p, dims=("n", "c", "y", "x")), "hires": DataArray(a, dims=("n", "c1", "y", "x"))})
    d = p[1, 0] - a[1, 0].astype(np.float64)
    assert ev.compute_measure(ds, 1, "mae") == np.mean(np.abs(d))
    assert ev.compute_measure(ds, 1, "mse") == np.mean(d ** 2)
    with pytest.raises(ValueError):
        ev.compute_measure(ds, 1, "rmse")
