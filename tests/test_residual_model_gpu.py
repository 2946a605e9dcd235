"""Residual learning through the model classes on the GPU ("Residual target"): a model trained with
residual_variable saves the four keys and the target's own range, apply() is cae_residual_restore_f64 of the engine's scores
bit for bit, evaluate() measures the restored prediction, the CLIs make the round trip, the paths that denormalise on their
own refuse, and without the keyword DSDataset is what it was.  Data and sizes of test_model_api.py::test_train_save_load_apply."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import residual_ref

pytestmark = pytest.mark.gpu

KEYS = ("residual_variable", "residual_mode", "residual_min", "residual_max")
_DATA = {}


def _data():
    if not _DATA:
        from cae_tools_amd.data import datagen
        _DATA.update(train=datagen.generate("circle", 21, seed=1234), test=datagen.generate("circle", 9, seed=4321))
    return _DATA["train"], _DATA["test"]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if x.dtype == np.float64 else np.uint32)


def _low(ds):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(ds["lowres"].values), dtype=np.float32)).cuda()


def _train_load_apply_evaluate(cls, folder, mode, **keywords):
    """the whole run for one model class; returns the loaded model"""
    from cae_tools_amd.data import datagen
    from cae_tools_amd.device_ops import residual_restore, residual_scan
    from cae_tools_amd.models import base_model
    from cae_tools_amd.models.ds_dataset import DSDataset
    from cae_tools_amd.models.model_metric import ModelMetric
    (train, test) = _data()
    torch.manual_seed(5)
    mt = cls(batch_size=8, nr_epochs=3, test_interval=1, lr=1e-3, weight_decay=1e-5, residual_variable="lowres",
             residual_mode=mode, **keywords)
    with redirect_stdout(io.StringIO()):
        metrics = mt.train(["lowres"], "hires", train, test, model_path=folder)
    assert len(mt.history["train_loss"]) == 3 and all(np.isfinite(mt.history["train_loss"]))

    # the folder: the four keys, and normalisation.weights with the target's own scanned range
    with open(os.path.join(folder, "parameters.json")) as f:
        stored = json.load(f)
    hires = torch.from_numpy(np.ascontiguousarray(np.asarray(train["hires"].values), dtype=np.float32)).cuda()
    (k, rmin, rmax) = residual_scan(_low(train), hires, mode=mode)
    assert k == 0 and rmin < 0.0 < rmax
    assert {key: stored[key] for key in KEYS} == {"residual_variable": "lowres", "residual_mode": mode, "residual_min": rmin,
                                                   "residual_max": rmax}
    with redirect_stdout(io.StringIO()):
        plain = DSDataset(train, ["lowres"], "hires")
    with open(os.path.join(folder, "normalisation.weights")) as f:
        assert json.load(f) == plain.get_normalisation_parameters()
    assert float(np.asarray(train["hires"].values).min()) == plain.min_output

    # load and apply: the prediction is the restored residual of the engine's scores, bit for bit
    m2 = cls()
    m2.load(folder)
    assert (m2.residual_variable, m2.residual_mode, m2.residual_min, m2.residual_max) == ("lowres", mode, rmin, rmax)
    score = datagen.generate("circle", 9, seed=4321)
    with redirect_stdout(io.StringIO()):
        m2.apply(score, ["lowres"], "model_output")
        packed = m2._model_dataset(score, ["lowres"], "lowres", normalise_in=m2.normalise_input)
    pred = np.asarray(score["model_output"].values)
    assert pred.dtype == np.float64 and pred.shape == (9, 1, 256, 256) and np.isfinite(pred).all()
    scores = m2._score_all(packed.device_inputs())
    want = residual_restore(_low(score), scores, rmin, rmax, mode=mode, enable=True).cpu().numpy()
    assert np.array_equal(_bits(pred), _bits(want))
    # ... which is the restatement of the restore over the interpolated input
    from cae_tools_amd.case_ops import upsample
    b = upsample(_low(score), (256, 256), mode=mode)
    assert np.array_equal(_bits(pred[:, 0]), _bits(residual_ref.restore(scores.cpu().numpy(), b, rmin, rmax)))

    # evaluate(): the metrics of the restored fp32 prediction against the stored target, as the host ModelMetric has them
    with redirect_stdout(io.StringIO()):
        got = m2.evaluate(m2._model_dataset(test, ["lowres"], "hires", normalise_in=m2.normalise_input, normalise_out=False))
    restored = pred.astype(np.float32).astype(np.float64)
    truth = np.asarray(test["hires"].values)
    mm = ModelMetric()
    for i in range(truth.shape[0]):
        mm.accumulate(truth[i], restored[i], np.ones(truth.shape[1:]))
    want = mm.get_metrics()
    for key in want:
        assert got[key] == pytest.approx(float(want[key]), rel=1e-9), key
    # the metrics train() returned are those of the prediction too, not of the residual: the model at the end of training
    # is the one that was saved
    for key in want:
        assert metrics["test"][key] == pytest.approx(float(want[key]), rel=1e-9), key

    # the paths that denormalise on their own refuse, naming themselves
    with pytest.raises(NotImplementedError) as refused:
        m2.apply_scene(score, ["lowres"])
    assert str(refused.value) == base_model.residual_refusal("apply_scene", "lowres")
    with pytest.raises(NotImplementedError) as refused:
        m2.importance(test, ["lowres"], "hires")
    assert str(refused.value) == base_model.residual_refusal("importance", "lowres")
    return m2


def test_convae_train_save_load_apply_evaluate(tmp_path):
    from cae_tools_amd.models.conv_ae_model import ConvAEModel
    _train_load_apply_evaluate(ConvAEModel, str(tmp_path / "model"), "bicubic", fc_size=16, encoded_dim_size=4)


def test_linear_through_the_shared_path(tmp_path):
    from cae_tools_amd.models.linear_model import LinearModel
    _train_load_apply_evaluate(LinearModel, str(tmp_path / "model"), "bilinear")


def test_cli_train_then_apply(tmp_path):
    from cae_tools_amd.cli import apply_cae, train_cae
    from cae_tools_amd.data import datagen
    from cae_tools_amd.data.arrays import open_dataset
    (tr, te) = (str(tmp_path / "train.nc"), str(tmp_path / "test.nc"))
    datagen.generate("circle", 12, seed=1).to_netcdf(tr)
    datagen.generate("circle", 6, seed=2).to_netcdf(te)
    folder = str(tmp_path / "m")
    common = ["--train-inputs", tr, "--test-inputs", te, "--model-folder", folder, "--input-variables", "lowres",
              "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2", "--batch-size", "5"]
    with redirect_stdout(io.StringIO()):
        train_cae.main(common + ["--residual-variable", "lowres", "--residual-mode", "bilinear"])
    with open(os.path.join(folder, "parameters.json")) as f:
        stored = json.load(f)
    assert stored["residual_variable"] == "lowres" and stored["residual_mode"] == "bilinear"
    assert stored["residual_min"] < 0.0 < stored["residual_max"]
    out = str(tmp_path / "scored.nc")
    with redirect_stdout(io.StringIO()):
        apply_cae.main([te, out, "--model-folder", folder])
    pred = open_dataset(out)["model_output"]
    assert pred.shape == (6, 1, 256, 256) and pred.dtype == np.float64 and np.isfinite(np.asarray(pred.values)).all()
    # the folder's settings hold when training continues; a flag that contradicts them ends the run
    with pytest.raises(SystemExit, match="cannot change that"):
        train_cae.main(common + ["--continue-training", "--residual-mode", "nearest"])
    with redirect_stdout(io.StringIO()):
        train_cae.main(common + ["--continue-training"])
    with open(os.path.join(folder, "parameters.json")) as f:
        again = json.load(f)
    assert again["residual_variable"] == "lowres" and again["residual_mode"] == "bilinear"
    with open(os.path.join(folder, "history.json")) as f:
        assert json.load(f)["nr_epochs"] == 4


def test_dataset_without_the_keyword_is_what_it_was_and_with_it_packs_the_residual():
    from cae_tools_amd.case_ops import upsample
    from cae_tools_amd.data.arrays import DataArray
    from cae_tools_amd.models.ds_dataset import DSDataset
    (_, test) = _data()
    order = np.random.default_rng(3).permutation(9).astype(np.int32)
    with redirect_stdout(io.StringIO()):
        plain = DSDataset(test, ["lowres"], "hires")
        keyword = DSDataset(test, ["lowres"], "hires", residual=None)
        resid = DSDataset(test, ["lowres"], "hires", residual=("lowres", "bicubic"))
    assert keyword.residual is None and keyword.get_residual_parameters() is None
    for (a, b) in zip(plain.device_batches(order), keyword.device_batches(order)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(plain.device_outputs().view(torch.int32), keyword.device_outputs().view(torch.int32))
    y = torch.rand((9, 1, 256, 256), device="cuda")
    assert torch.equal(plain.denormalise_device(y).view(torch.int64), keyword.denormalise_device(y).view(torch.int64))

    # with it: the target the engine is handed is the packed residual, in the frozen order, and the inputs are untouched
    hires = np.ascontiguousarray(np.asarray(test["hires"].values), dtype=np.float32)
    b = upsample(_low(test), (256, 256), mode="bicubic")
    (k, rmin, rmax) = residual_ref.scan(hires, b)
    assert k == 0 and resid.get_residual_parameters() == [rmin, rmax]
    assert resid.get_normalisation_parameters() == plain.get_normalisation_parameters()
    (x, t) = resid.device_batches(order)
    assert torch.equal(x.view(torch.int32), plain.device_batches(order)[0].view(torch.int32))
    rows = np.empty(9, dtype=np.int64)
    rows[order] = np.arange(9)
    assert np.array_equal(_bits(t.cpu().numpy()[:, 0]), _bits(residual_ref.pack(hires, b, rmin, rmax, dst_rows=rows)))
    assert np.array_equal(_bits(resid.device_outputs().cpu().numpy()[:, 0]), _bits(residual_ref.pack(hires, b, rmin, rmax)))
    assert torch.equal(resid.device_target().view(torch.int32), plain.device_target().view(torch.int32))
    restored = resid.denormalise_device(resid.device_outputs()).cpu().numpy()[:, 0]
    assert (np.abs(restored - hires[:, 0]) <= residual_ref.round_trip_bound(hires, b, rmin, rmax)).all()
    resid.set_residual_parameters([rmin - 1.0, rmax + 1.0])
    assert resid.get_residual_parameters() == [rmin - 1.0, rmax + 1.0]
    assert np.array_equal(_bits(resid.device_outputs().cpu().numpy()[:, 0]), _bits(residual_ref.pack(hires, b, rmin - 1.0, rmax + 1.0)))

    # a residual that is not finite is refused with the count; more than one output channel likewise
    coarse = np.array(np.asarray(test["lowres"].values), dtype=np.float32)
    coarse[4, 0, 3, 7] = np.nan
    from cae_tools_amd.data.arrays import Dataset
    with_coarse = Dataset({"lowres": test["lowres"], "hires": test["hires"], "coarse": DataArray(coarse, dims=test["lowres"].dims)})
    with pytest.raises(ValueError) as refused, redirect_stdout(io.StringIO()):
        DSDataset(with_coarse, ["lowres"], "hires", residual=("coarse", "nearest"))
    assert str(refused.value) == "residual of hires over coarse contains 256 values that are not finite"
    dims = test["hires"].dims
    two = DataArray(np.concatenate([hires, hires], axis=1), dims=(dims[0], "two_channels", dims[2], dims[3]))
    with pytest.raises(ValueError, match="one channel"), redirect_stdout(io.StringIO()):
        DSDataset(Dataset({"lowres": test["lowres"], "hires": two}), ["lowres"], "hires", residual=("lowres", "bicubic"))
