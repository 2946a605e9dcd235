"""apply(self_ensemble=...) on the GPU ("Dihedral augmentation"), bit for bit against a reference built
here: the packed inputs turned with numpy for each code of the group, scored with _score_all, turned back with numpy by the
inverse codes, stacked [draw][case] and reduced by case_ops.ensemble_moments (cae_ensemble_moments).  ConvAE and UNET with
"dihedral" on 7 cases, the ConvAE with "flips" on planes that are not square; case_chunk 1, 3 and 7 give the same bits; and
without the keyword apply_cae writes the file it always wrote, byte for byte.

The constant case.  All orientations of a constant input are the same input, so the K scores are one field y, bit for bit;
but y is not itself symmetric (zero padding, the dense bottleneck), so the K fields turned BACK differ and their spread is
not 0: the members of the ensemble are the 4 or 8 turns of y.  What does hold, and is held here to 4 ulp of the range, the
rounding of cae_ensemble_moments' formula: the mean is vmin + (y_0 + S (y_k - y_0) / K) * range and the spread
sqrt((S d^2 - (S d)^2 / K) / (K - 1)) * |range| over the turns y_k of the PLAIN apply's score of that case, and where the
turns of a pixel agree - the whole plane for a score that is constant - the spread is exactly 0 and the mean the plain
prediction."""
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from cae_tools_amd.utils import augment

pytestmark = pytest.mark.gpu

N = 7
_MODELS = {}


def _data(n, seed, in_shape, out_shape, constant_case=None):
    from cae_tools_amd.data.arrays import DataArray, Dataset
    rng = np.random.default_rng(seed)
    lo = (280 + 10 * rng.random((n,) + in_shape)).astype(np.float32)
    if constant_case is not None:
        lo[constant_case] = np.float32(284.5)
    ds = Dataset()
    ds["lo"] = DataArray(lo, dims=("n", "c", "y", "x"))
    ds["hi"] = DataArray((280 + 10 * rng.random((n,) + out_shape)).astype(np.float32), dims=("n", "c2", "y2", "x2"))
    ds["valid"] = DataArray((rng.random((n, 1) + out_shape[1:]) < 0.85).astype(np.float32), dims=("n", "one", "y2", "x2"))
    return ds


def _model(name):
    """a model of two epochs, trained once per module: (model, input shape, output shape)"""
    if name not in _MODELS:
        from cae_tools_amd.models.conv_ae_model import ConvAEModel
        from cae_tools_amd.models.unet import UNET, unet_layer_spec
        common = dict(batch_size=5, nr_epochs=2, test_interval=1, lr=1e-3, weight_decay=1e-5)
        if name == "unet":
            (mt, shapes) = (UNET(fc_size=10, encoded_dim_size=4, dropout_rate=0.1, **common), ((2, 16, 16), (1, 16, 16)))
            mt.spec = unet_layer_spec(2, 1, (16, 16), [8, 16])
        else:
            shapes = ((1, 16, 16), (1, 32, 32)) if name == "conv" else ((1, 8, 12), (1, 32, 48))
            mt = ConvAEModel(fc_size=16, encoded_dim_size=4, **common)
        torch.manual_seed(11)
        with redirect_stdout(io.StringIO()):
            mt.train(["lo"], "hi", _data(12, 1, *shapes), _data(5, 2, *shapes), mask_variable_name="valid")      # the UNET's loss mask
        _MODELS[name] = (mt, shapes)
    return _MODELS[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _reference(mt, score, group):
    """(mean, spread) float64 numpy arrays, by numpy turns around _score_all and the cae_ensemble_moments wrapper"""
    from cae_tools_amd.case_ops import ensemble_moments
    with redirect_stdout(io.StringIO()):
        ds = mt._model_dataset(score, ["lo"], "lo", normalise_in=mt.normalise_input)
    x = ds.device_inputs().cpu().numpy()
    draws = []
    for code in range(group):
        turned = np.ascontiguousarray(augment.apply(x, code))
        y = mt._score_all(torch.from_numpy(turned).cuda()).cpu().numpy()
        draws.append(np.ascontiguousarray(augment.apply(y, augment.inverse_code(code))))
    stacked = torch.from_numpy(np.stack(draws)).cuda()
    (mean, std) = ensemble_moments(stacked, ds.min_output, ds.max_output, want_std=True)
    return mean.cpu().numpy(), std.cpu().numpy(), np.stack(draws), (ds.min_output, ds.max_output)


@pytest.mark.parametrize("name, mode", [("conv", "dihedral"), ("unet", "dihedral"), ("conv_wide", "flips")])
def test_self_ensemble_against_numpy_turns(name, mode):
    (mt, shapes) = _model(name)
    group = augment.GROUPS[mode]
    score = _data(N, 5, *shapes, constant_case=2)
    (mean, std, draws, (vmin, vmax)) = _reference(mt, score, group)
    results = {}
    for chunk in (None, 1, 3, 7):
        ds = _data(N, 5, *shapes, constant_case=2)
        with redirect_stdout(io.StringIO()):
            mt.apply(ds, ["lo"], "p", self_ensemble=mode, self_ensemble_spread="s", case_chunk=chunk)
        (p, s) = (np.asarray(ds["p"].values), np.asarray(ds["s"].values))
        assert p.dtype == s.dtype == np.float64 and p.shape == s.shape == (N,) + shapes[1]
        assert tuple(ds["p"].dims) == tuple(ds["s"].dims) == ("n", "model_output_channel", "model_output_y", "model_output_x")
        results[chunk] = (p, s)
        assert np.array_equal(_bits(p), _bits(mean)), f"mean, case_chunk {chunk}"
        assert np.array_equal(_bits(s), _bits(std)), f"spread, case_chunk {chunk}"
    assert np.isfinite(mean).all() and (std >= 0).all() and (std > 0).any()
    # without the spread the mean is the same, and no second variable appears
    ds = _data(N, 5, *shapes, constant_case=2)
    with redirect_stdout(io.StringIO()):
        mt.apply(ds, ["lo"], "p", self_ensemble=mode)
    assert np.array_equal(_bits(np.asarray(ds["p"].values)), _bits(mean)) and "s" not in ds

    # the constant case (the module's docstring): its K scores are the plain score's bits, and mean and spread are the
    # formula over the turns of the plain score, to 4 ulp of the range
    plain = _data(N, 5, *shapes, constant_case=2)
    with redirect_stdout(io.StringIO()):
        mt.apply(plain, ["lo"], "p")
        packed = mt._model_dataset(plain, ["lo"], "lo", normalise_in=mt.normalise_input)
    y = mt._score_all(packed.device_inputs()[2:3]).cpu().numpy()[0]
    turns = np.stack([np.ascontiguousarray(augment.apply(y, augment.inverse_code(k))) for k in range(group)])
    assert np.array_equal(turns.view(np.uint32), draws[:, 2].view(np.uint32))
    rng = vmax - vmin
    d = turns.astype(np.float64) - turns[0].astype(np.float64)
    want_mean = vmin + (turns[0].astype(np.float64) + d.sum(0) / group) * rng
    want_std = np.sqrt(np.maximum(0.0, ((d * d).sum(0) - d.sum(0) ** 2 / group) / (group - 1))) * abs(rng)
    tol = 4 * np.spacing(abs(rng))
    print(f"{name} {mode}: constant case |mean - formula| {np.abs(mean[2] - want_mean).max():.3g}, |spread - formula| "
          f"{np.abs(std[2] - want_std).max():.3g}, 4 ulp of the range {tol:.3g}")
    assert np.abs(mean[2] - want_mean).max() <= tol
    agree = (turns == turns[0]).all(0)
    assert (std[2][agree] == 0.0).all()
    assert np.abs(mean[2][agree] - np.asarray(plain["p"].values)[2][agree]).max(initial=0.0) <= tol
    # the spread's formula cancels: S d^2 - (S d)^2 / K loses up to K ulp of S d^2, so the spread is held in its square
    var_tol = 4 * group * np.spacing((d * d).sum(0).max()) * rng * rng + tol * tol
    assert np.abs(std[2] ** 2 - want_std ** 2).max() <= var_tol


def test_refusals_come_before_the_scoring():
    from cae_tools_amd.models import base_model
    (mt, shapes) = _model("conv")
    (wide, wide_shapes) = _model("conv_wide")
    score = _data(3, 5, *shapes)
    cases = [
        (dict(self_ensemble="turns"), ValueError, "self_ensemble must be one of flips, dihedral, got 'turns'"),
        (dict(self_ensemble_spread="s"), ValueError, "self_ensemble_spread needs self_ensemble='flips' or 'dihedral'"),
        (dict(self_ensemble="flips", interval="0.9"), ValueError,
         "interval needs the plain prediction the model was calibrated with: leave self_ensemble out"),
        (dict(self_ensemble="flips", ensemble_size=4), ValueError, "self_ensemble and ensemble_size are two ensembles: ask for one of them"),
        (dict(self_ensemble="flips", case_chunk=0), ValueError, "case_chunk must be an integer of at least 1, got 0"),
    ]
    for (keywords, kind, text) in cases:
        with pytest.raises(kind) as refused:
            mt.apply(score, ["lo"], "p", **keywords)
        assert str(refused.value) == text and "p" not in score
    with pytest.raises(ValueError) as refused:
        wide.apply(_data(3, 5, *wide_shapes), ["lo"], "p", self_ensemble="dihedral")
    assert str(refused.value) == "self_ensemble='dihedral' transposes, which needs square planes: got 8 x 12; use 'flips'"
    mt.residual_variable = "lo"
    try:
        with pytest.raises(NotImplementedError) as refused:
            mt.apply(score, ["lo"], "p", self_ensemble="flips")
        assert str(refused.value) == base_model.residual_refusal("apply(self_ensemble=...)", "lo")
    finally:
        mt.residual_variable = None


def test_without_the_flag_apply_cae_writes_the_same_file(tmp_path):
    """the unchanged path: BaseModel.apply_device's prediction written by to_netcdf, against the command line's file, byte for
    byte; then the flags through the command line"""
    from cae_tools_amd.cli import apply_cae
    from cae_tools_amd.data.arrays import open_dataset
    (mt, shapes) = _model("conv")
    (folder, data, out, direct, both) = (str(tmp_path / f) for f in ("m", "score.nc", "out.nc", "direct.nc", "both.nc"))
    mt.save(folder)
    _data(N, 5, *shapes).to_netcdf(data)
    with redirect_stdout(io.StringIO()):
        apply_cae.main([data, out, "--model-folder", folder])
        ds = open_dataset(data)
        mt.apply_device(ds, ["lo"], "model_output")
        ds.to_netcdf(direct)
    with open(out, "rb") as f, open(direct, "rb") as g:
        assert f.read() == g.read()
    with redirect_stdout(io.StringIO()):
        apply_cae.main([data, both, "--model-folder", folder, "--self-ensemble", "dihedral", "--self-ensemble-spread", "spread"])
    got = open_dataset(both)
    (mean, std, _, _) = _reference(mt, _data(N, 5, *shapes), 8)
    assert np.array_equal(_bits(np.asarray(got["model_output"].values)), _bits(mean))
    assert np.array_equal(_bits(np.asarray(got["spread"].values)), _bits(std))
    with pytest.raises(SystemExit, match="--self-ensemble-spread needs --self-ensemble"):
        apply_cae.main([data, both, "--model-folder", folder, "--self-ensemble-spread", "spread"])
    assert os.path.getsize(out) < os.path.getsize(both)
