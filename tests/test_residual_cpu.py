"""The residual target without a GPU: the restatement's consistency bound (residual_ref.py), the
train_cae flags, the refusals of the paths that do not serve a residual model, the parameters.json round trip and the refusal
of a data set without the residual variable."""
import json
import os

import numpy as np
import pytest

import baseline_ref
import loader_ref
import residual_ref
from cae_tools_amd.cli import train_cae
from cae_tools_amd.data.arrays import DataArray, Dataset
from cae_tools_amd.models.base_model import residual_refusal
from cae_tools_amd.models.conv_ae_model import ConvAEModel
from cae_tools_amd.models.linear_model import LinearModel
from cae_tools_amd.models.model_loader import load_model
from cae_tools_amd.models.unet import UNET
from cae_tools_amd.models.var_ae_model import VarAEModel

N = 3
KEYS = ("residual_variable", "residual_mode", "residual_min", "residual_max")


def _pair(i, o, seed=0):
    """a narrow temperature-like pair (loader_ref.narrow_variable): low (N, h, w) and target (N, H, W) as fp32"""
    low = loader_ref.narrow_variable(N * i[0] * i[1], seed=102 + seed).reshape((N,) + i)
    target = loader_ref.narrow_variable(N * o[0] * o[1], seed=202 + seed).reshape((N,) + o)
    return low, target


@pytest.mark.parametrize("mode", ["nearest", "bilinear", "bicubic"])
@pytest.mark.parametrize("shapes", [((5, 3), (70, 130)), ((4, 4), (64, 64)), ((16, 16), (8, 8))])
def test_round_trip_is_within_the_bound(shapes, mode):
    (i, o) = shapes
    (low, target) = _pair(i, o)
    b = baseline_ref.upsample(low.astype(np.float64), o, mode)[0].astype(np.float64)      # any fp64 field serves as b
    (k, rmin, rmax) = residual_ref.scan(target, b)
    assert k == 0 and rmin < rmax
    y = residual_ref.pack(target, b, rmin, rmax)
    assert y.dtype == np.float32 and float(y.min()) == 0.0 and float(y.max()) == 1.0
    p = residual_ref.restore(y, b, rmin, rmax)
    err = np.abs(p - target.astype(np.float64))
    limit = residual_ref.round_trip_bound(target, b, rmin, rmax)
    print(f"restatement round trip {mode} {o}: max error / bound = {float(np.max(err / limit)):.3e}")
    assert (err <= limit).all()
    # rows land where dst_rows says
    rows = [2, 0, 1]
    moved = residual_ref.pack(target, b, rmin, rmax, dst_rows=rows)
    assert all(np.array_equal(moved[rows[c]], y[c]) for c in range(N))


def test_span_zero_gives_zeros_and_values_that_are_not_finite_give_nan():
    (low, _) = _pair((4, 4), (8, 8))
    b = baseline_ref.upsample(low.astype(np.float64), (8, 8), "nearest")[0].astype(np.float64)
    target = b.astype(np.float32)           # fp32 values: the residual is exactly zero
    assert residual_ref.scan(target, b) == (0, 0.0, 0.0)
    y = residual_ref.pack(target, b, 0.0, 0.0)
    assert not y.view(np.uint32).any()
    assert np.array_equal(residual_ref.restore(y, b, 0.0, 0.0), b)
    b[1, 2, 3] = np.nan
    target[2, 0, 0] = np.inf
    (k, rmin, rmax) = residual_ref.scan(target, b)
    assert (k, rmin, rmax) == (2, 0.0, 0.0)
    y = residual_ref.pack(target, b, rmin, rmax)
    lost = np.zeros(b.shape, dtype=bool)
    lost[1, 2, 3] = lost[2, 0, 0] = True
    assert np.array_equal(np.isnan(y), lost) and np.array_equal(np.isnan(residual_ref.restore(y, b, rmin, rmax)), lost)
    raw = residual_ref.pack(target, b, rmin, rmax, enable=False)
    assert np.array_equal(np.isnan(raw), lost) and not raw[~lost].any()


BASE = ["--train-inputs", "a.nc", "--test-inputs", "b.nc", "--model-folder", "m", "--input-variables", "low", "aux",
        "--output-variable", "high"]


def test_train_cae_flags():
    parse = train_cae.build_cli_parser().parse_args
    assert train_cae.residual_settings(parse(BASE)) == (None, "bicubic")
    assert train_cae.residual_settings(parse(BASE + ["--residual-variable", "aux"])) == ("aux", "bicubic")
    assert train_cae.residual_settings(parse(BASE + ["--residual-variable", "aux", "--residual-mode", "bilinear"])) == ("aux", "bilinear")
    assert train_cae.residual_settings(parse(BASE + ["--residual-mode", "nearest"])) == ("low", "nearest")      # the first input
    with pytest.raises(SystemExit):
        parse(BASE + ["--residual-mode", "lanczos"])


def test_continue_training_keeps_the_folder_and_refuses_a_contradiction():
    parse = train_cae.build_cli_parser().parse_args
    held = {"residual_variable": "low", "residual_mode": "bilinear", "residual_min": -1.0, "residual_max": 2.0}
    assert train_cae.residual_settings(parse(BASE), held) == ("low", "bilinear")
    assert train_cae.residual_settings(parse(BASE + ["--residual-variable", "low", "--residual-mode", "bilinear"]), held) == ("low", "bilinear")
    for flags in (["--residual-variable", "aux"], ["--residual-mode", "bicubic"]):
        with pytest.raises(SystemExit, match="--continue-training: the model folder was trained with the residual over 'low'"):
            train_cae.residual_settings(parse(BASE + flags), held)
    assert train_cae.residual_settings(parse(BASE), {}) == (None, "bicubic")       # a folder from before the feature
    with pytest.raises(SystemExit, match="no residual target"):
        train_cae.residual_settings(parse(BASE + ["--residual-variable", "low"]), {})


def test_contradicting_flags_end_train_cae_before_anything_is_opened(tmp_path):
    folder = tmp_path / "model"
    folder.mkdir()
    (folder / "parameters.json").write_text(json.dumps({"type": "ConvAEModel", "residual_variable": "low", "residual_mode": "bicubic"}))
    argv = ["--train-inputs", "missing.nc", "--test-inputs", "missing.nc", "--model-folder", str(folder), "--input-variables", "low",
            "--output-variable", "high", "--continue-training", "--residual-mode", "nearest"]
    with pytest.raises(SystemExit, match="cannot change that"):
        train_cae.main(argv)


def _residual_model(cls=ConvAEModel, **keywords):
    model = cls(residual_variable="low", **keywords)
    (model.residual_min, model.residual_max) = (-1.5, 2.25)
    return model


def test_constructor_keywords():
    for cls in (ConvAEModel, UNET, VarAEModel, LinearModel):
        plain = cls()
        assert plain.residual_variable is None and plain.residual_mode == "bicubic"
        model = cls(residual_variable="low", residual_mode="bilinear")
        assert (model.residual_variable, model.residual_mode) == ("low", "bilinear")
        assert set(KEYS) <= set(cls.OPTIONAL_PARAM_KEYS)
        with pytest.raises(ValueError, match="residual_mode must be one of"):
            cls(residual_variable="low", residual_mode="lanczos")


@pytest.mark.parametrize("path, call", [
    ("apply_scene", lambda m: m.apply_scene(None, ["low"])),
    ("importance", lambda m: m.importance(None, ["low"], "high")),
])
def test_refused_paths_name_themselves(path, call):
    model = _residual_model()
    with pytest.raises(NotImplementedError) as refused:
        call(model)
    assert str(refused.value) == residual_refusal(path, "low")
    assert path in str(refused.value) and "'low'" in str(refused.value)


@pytest.mark.parametrize("path, call", [
    ("apply(ensemble_size=...)", lambda m: m.apply(None, ["low"], ensemble_size=4)),
    ("generate", lambda m: m.generate(2)),
    ("decode", lambda m: m.decode(np.zeros((1, 4), dtype=np.float32))),
    ("verify_ensemble", lambda m: m.verify_ensemble(None, ["low"], "high", 4)),
])
def test_refused_ensemble_paths_of_the_vae(path, call):
    model = _residual_model(VarAEModel)
    with pytest.raises(NotImplementedError) as refused:
        call(model)
    assert str(refused.value) == residual_refusal(path, "low")


def test_a_plain_model_is_not_refused_by_the_helper():
    ConvAEModel()._refuse_residual("apply_scene")


def _saved_linear(folder, **keywords):
    model = LinearModel(**keywords)
    (model.input_shape, model.output_shape) = ((1, 4, 4), (1, 8, 8))
    model.normalisation_parameters = [{"low": 0.0}, {"low": 1.0}, 280.0, 300.0]
    model._build()
    model.save(str(folder))
    return model


def test_parameters_round_trip_with_the_keys(tmp_path):
    model = _saved_linear(tmp_path, residual_variable="low", residual_mode="bilinear")
    with open(os.path.join(tmp_path, "parameters.json")) as f:
        stored = json.load(f)
    assert {k: stored[k] for k in KEYS} == {"residual_variable": "low", "residual_mode": "bilinear", "residual_min": None,
                                            "residual_max": None}
    (model.residual_min, model.residual_max) = (-1.5, 2.25)
    model.save(str(tmp_path))
    loaded = load_model(str(tmp_path))
    assert (loaded.residual_variable, loaded.residual_mode, loaded.residual_min, loaded.residual_max) == ("low", "bilinear", -1.5, 2.25)
    assert loaded.get_parameters() == model.get_parameters()
    with open(os.path.join(tmp_path, "normalisation.weights")) as f:
        assert json.load(f) == [{"low": 0.0}, {"low": 1.0}, 280.0, 300.0]       # the target's own range, as ever


def test_parameters_round_trip_without_the_keys(tmp_path):
    model = _saved_linear(tmp_path)
    with open(os.path.join(tmp_path, "parameters.json")) as f:
        stored = json.load(f)
    assert not set(KEYS) & set(stored)          # parameters.json is what it always was
    loaded = load_model(str(tmp_path))
    assert loaded.residual_variable is None and loaded.residual_mode == "bicubic"
    assert loaded.residual_min is None and loaded.residual_max is None
    assert loaded.get_parameters() == model.get_parameters()


def test_apply_refuses_a_data_set_without_the_residual_variable():
    model = _residual_model()
    model.residual_variable = "coarse"
    model.normalise_input = True
    model.normalisation_parameters = [{"low": 0.0}, {"low": 1.0}, 280.0, 300.0]
    ds = Dataset({"low": DataArray(np.zeros((2, 1, 4, 4), dtype=np.float32), dims=("box", "channel", "y", "x"))})
    with pytest.raises(ValueError, match="'coarse'"):
        model.apply(ds, ["low"])
    assert "model_output" not in ds
