"""train(augment=...) on the GPU ("Dihedral augmentation"), bit for bit.

The equivalence: one epoch with augment="dihedral", seed 3, must be one epoch WITHOUT augmentation on a data set whose input,
output and mask variables were turned case by case with numpy by augment.codes(3, 0, 12, 8) - same seed for the weights and
the shuffle, 12 cases in batches of 5 (the last batch partial).  Weights, Adam moments, running statistics, the loss
history and the printed epoch lines must be the same bits; this rests on the run-to-run reproducibility of
test_reproducible_gpu.py / test_reproducible_models_gpu.py.  The minimum and maximum of a variable do not change when the
pixels of its cases change places, so both runs normalise alike.  All four model classes at small configurations, the ConvAE
also on non-square planes with "flips" (where "dihedral" is refused), a second train() call (epoch number 1), the residual
target checked at the bound buffer, evaluate() on the pristine data, and augmentation off against the call without the
keyword."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from cae_tools_amd.utils import augment

pytestmark = pytest.mark.gpu

(N_TRAIN, N_TEST, BATCH, SEED) = (12, 5, 5, 3)


def _data(n, seed, in_shape, out_shape, mask=False):
    from cae_tools_amd.data.arrays import DataArray, Dataset
    rng = np.random.default_rng(seed)
    ds = Dataset()
    ds["lo"] = DataArray((280 + 10 * rng.random((n,) + in_shape)).astype(np.float32), dims=("n", "c", "y", "x"))
    ds["hi"] = DataArray((280 + 10 * rng.random((n,) + out_shape)).astype(np.float32), dims=("n", "c2", "y2", "x2"))
    if mask:
        ds["valid"] = DataArray((rng.random((n, 1) + out_shape[1:]) < 0.85).astype(np.float32), dims=("n", "one", "y2", "x2"))
    return ds


def _turned(ds, codes):
    """every variable of ds with case j turned by codes[j], in numpy"""
    from cae_tools_amd.data.arrays import DataArray, Dataset
    out = Dataset()
    for name in ("lo", "hi", "valid"):
        if name in ds:
            values = np.asarray(ds[name].values)
            out[name] = DataArray(np.stack([np.ascontiguousarray(augment.apply(values[j], c)) for (j, c) in enumerate(codes)]),
                                  dims=ds[name].dims)
    return out


def _unet(**kw):
    from cae_tools_amd.models.unet import UNET, unet_layer_spec
    mt = UNET(fc_size=10, encoded_dim_size=4, dropout_rate=0.1, lambda_pearson=0.5, **kw)
    mt.spec = unet_layer_spec(2, 1, (16, 16), [8, 16])
    return mt


def _conv(**kw):
    from cae_tools_amd.models.conv_ae_model import ConvAEModel
    return ConvAEModel(fc_size=16, encoded_dim_size=4, **kw)


def _var(**kw):
    from cae_tools_amd.models.var_ae_model import VarAEModel
    return VarAEModel(fc_size=12, encoded_dim_size=4, lambda_mse=1.0, lambda_kl=0.5, lambda_ssim=0.7, noise_seed=6, **kw)


def _linear(**kw):
    from cae_tools_amd.models.linear_model import LinearModel
    return LinearModel(**kw)


# name: (constructor, input shape, output shape, mask variable)
MODELS = {
    "conv": (_conv, (1, 16, 16), (1, 32, 32), None),
    "unet": (_unet, (2, 16, 16), (1, 16, 16), "valid"),
    "var": (_var, (1, 12, 12), (1, 176, 176), None),
    "linear": (_linear, (1, 8, 8), (1, 16, 16), None),
}
CONV_WIDE = (_conv, (1, 8, 12), (1, 32, 48), None)


def _state(mt):
    eng = mt._engine
    eng.sync()
    out = [("params", eng.params.cpu()), ("exp_avg", eng.exp_avg.cpu()), ("exp_avg_sq", eng.exp_avg_sq.cpu())]
    if getattr(eng, "buffers", None) is not None:
        out.append(("running statistics", eng.buffers.cpu()))
    return out


def _epoch_lines(text):
    """what train() printed for its epochs: the lines up to `elapsed:`, those that name a duration or the device left out"""
    lines = text.split("elapsed:")[0].splitlines()
    return [l for l in lines if l.strip() and "time" not in l and "seconds" not in l and "device" not in l
            and "train method" not in l and "DSDataset" not in l and "loarder" not in l and not l.startswith("{")]


def _train(config, train, test, calls, **first_keywords):
    """a fresh model, seeded, trained len(calls) times: calls[i] are the keywords of train() number i.  Returns (model, state,
    history, epoch lines of every call, metrics of the last call)."""
    (make, _, _, mask) = config
    torch.manual_seed(7)
    mt = make(batch_size=BATCH, nr_epochs=1, test_interval=1, lr=1e-3, weight_decay=1e-5, **first_keywords)
    lines = []
    metrics = None
    for (data, keywords) in calls:
        out = io.StringIO()
        with redirect_stdout(out):
            metrics = mt.train(["lo"], "hi", data, test, mask_variable_name=mask, **keywords)
        lines.append(_epoch_lines(out.getvalue()))
    return mt, _state(mt), json.loads(json.dumps(mt.history)), lines, metrics


def _same(a, b, what):
    (_, sa, ha, la, _), (_, sb, hb, lb, _) = a, b
    assert ha == hb, f"{what}: history differs: {ha} != {hb}"
    assert la == lb and all(len(l) >= 1 for l in la), f"{what}: printed epoch lines differ: {la} != {lb}"
    for ((name, u), (_, v)) in zip(sa, sb):
        assert torch.equal(u, v), f"{what}: {name} differ in {int((u != v).sum())} of {u.numel()} entries"


def _sets(config):
    (_, in_shape, out_shape, mask) = config
    return (_data(N_TRAIN, 1, in_shape, out_shape, mask is not None), _data(N_TEST, 2, in_shape, out_shape, mask is not None))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_an_augmented_epoch_is_an_epoch_on_the_turned_data(name):
    config = MODELS[name]
    (train, test) = _sets(config)
    codes = augment.codes(SEED, 0, N_TRAIN, 8)
    assert len(set(codes.tolist())) > 3 and (codes >= 4).any()      # the epoch does turn and transpose
    got = _train(config, train, test, [(train, dict(augment="dihedral", augment_seed=SEED))])
    want = _train(config, train, test, [(_turned(train, codes), {})])
    _same(got, want, name)
    mt = got[0]
    assert (mt.augment, mt.augment_seed) == ("dihedral", SEED)
    assert mt.get_parameters()["augment"] == "dihedral" and mt.get_parameters()["augment_seed"] == SEED
    assert "augment" not in want[0].get_parameters() and "augment_seed" not in want[0].get_parameters()
    plain = _train(config, train, test, [(train, {})])
    assert not all(torch.equal(u, v) for ((_, u), (_, v)) in zip(got[1], plain[1])), "the augmentation changed nothing"
    # evaluate() after the augmented run saw the pristine training set: the metrics train() returned are those of a data set
    # built afresh
    with redirect_stdout(io.StringIO()):
        fresh = mt._model_dataset(train, ["lo"], "hi", normalise_in=mt.normalise_input, normalise_out=False,
                                  mask_variable_name=config[3])
        again = mt.evaluate(fresh)
        scores = mt._score_all(fresh.device_inputs()).cpu().numpy().astype(np.float64)
    first = got[4]["train"]
    if int(np.prod(config[2])) <= 4096:
        assert again == first
        return
    # The VAE's 176 x 176 plane is 8 chunks of k_metric_sums, whose partial sums meet in fp64 atomics in whatever order the
    # workgroups finish: evaluate() is not the same bits from call to call there, with or without augmentation.  A sum of 8
    # partials carries at most u = 7 * 2^-53 of its absolute terms, whatever the order; the quotients of sums of positive
    # terms twice that; the correlation r = cov / sqrt(va ve) of a case what cov, va and ve - differences of such sums, each
    # within 4 u (S a'^2 + S e'^2) - carry into it.
    u = 7 * 2.0 ** -53
    for key in ("mse", "rmse", "mae"):
        print(f"{name}: {key} {again[key]!r} against {first[key]!r}")
        assert abs(again[key] - first[key]) <= 2 * u * first[key], key
    (vmin, vmax) = (fresh.min_output, fresh.max_output)
    a = np.asarray(train["hi"].values, dtype=np.float64).reshape(N_TRAIN, -1) - vmin
    e = scores.reshape(N_TRAIN, -1) * (vmax - vmin)
    n = a.shape[1]
    (va, ve) = ((a * a).sum(1) - a.sum(1) ** 2 / n, (e * e).sum(1) - e.sum(1) ** 2 / n)
    r = ((a * e).sum(1) - a.sum(1) * e.sum(1) / n) / np.sqrt(va * ve)
    each = 4 * u * ((a * a).sum(1) + (e * e).sum(1))
    bound = float(np.mean(each / np.sqrt(va * ve) + np.abs(r) * (each / va + each / ve) / 2))
    key = "mean_pearson_correlation"
    print(f"{name}: {key} {again[key]!r} against {first[key]!r}, bound {bound:.3g}")
    assert abs(again[key] - first[key]) <= 2 * bound      # either call within `bound` of the exact value


def test_flips_on_planes_that_are_not_square_and_dihedral_refused_there():
    (train, test) = _sets(CONV_WIDE)
    codes = augment.codes(SEED, 0, N_TRAIN, 4)
    assert len(set(codes.tolist())) > 2
    got = _train(CONV_WIDE, train, test, [(train, dict(augment="flips", augment_seed=SEED))])
    want = _train(CONV_WIDE, train, test, [(_turned(train, codes), {})])
    _same(got, want, "conv 8 x 12 -> 32 x 48, flips")
    with pytest.raises(ValueError) as refused:
        _train(CONV_WIDE, train, test, [(train, dict(augment="dihedral"))])
    assert str(refused.value) == "augment='dihedral' transposes, which needs square planes: got 8 x 12; use 'flips'"


@pytest.mark.parametrize("name", ["conv", "linear"])
def test_a_second_train_call_continues_the_stream(name):
    """the second call is epoch number 1: history["nr_epochs"] + epoch.  The keywords given once stay the model's."""
    config = MODELS[name]
    (train, test) = _sets(config)
    got = _train(config, train, test, [(train, dict(augment="dihedral", augment_seed=SEED)), (train, {})])
    want = _train(config, train, test, [(_turned(train, augment.codes(SEED, 0, N_TRAIN, 8)), {}),
                                        (_turned(train, augment.codes(SEED, 1, N_TRAIN, 8)), {})])
    _same(got, want, name + ", two calls")
    assert got[0]._augmenter.epoch == 1 and got[2]["nr_epochs"] == 2
    assert not np.array_equal(augment.codes(SEED, 0, N_TRAIN, 8), augment.codes(SEED, 1, N_TRAIN, 8))


@pytest.mark.parametrize("name", ["conv", "unet"])
def test_the_residual_target_is_turned_at_the_buffer(name):
    """the interpolation does not commute with a flip bit for bit, so a residual model is not compared with a run on turned
    data: after the epoch's rewrite every bound buffer is the numpy turn of its pristine array - device_inputs(), the packed
    residual device_outputs() and the mask - row i being case order[i] for the ConvAE's frozen batch order"""
    config = MODELS[name]
    (train, test) = _sets(config)
    (mt, _, history, _, _) = _train(config, train, test, [(train, dict(augment="dihedral", augment_seed=SEED))],
                                    residual_variable="lo", residual_mode="bilinear")
    aug = mt._augmenter
    assert aug.epoch == 0 and len(aug.pairs) == (3 if name == "unet" else 2) and np.isfinite(history["train_loss"]).all()
    assert (aug.order is not None) == (name == "conv")
    order = np.arange(N_TRAIN) if aug.order is None else aug.order
    assert sorted(order.tolist()) == list(range(N_TRAIN))
    codes = augment.codes(SEED, 0, N_TRAIN, 8)
    with redirect_stdout(io.StringIO()):
        packed = mt._model_dataset(train, ["lo"], "hi", normalise_in=mt.normalise_input, normalise_out=mt.normalise_output,
                                   mask_variable_name=config[3])
        pristine_target = packed.device_outputs().cpu().numpy()
    assert np.array_equal(aug.pairs[1][0].cpu().numpy().view(np.uint32), pristine_target.view(np.uint32))
    assert pristine_target.min() >= 0.0 and pristine_target.max() <= 1.0 and mt.residual_min < 0.0     # it IS the packed residual
    for (pristine, buffer) in aug.pairs:
        (p, b) = (pristine.cpu().numpy(), buffer.cpu().numpy())
        want = np.stack([np.ascontiguousarray(augment.apply(p[j], codes[j])) for j in order])
        assert np.array_equal(b.view(np.uint32), want.view(np.uint32))


def test_with_augmentation_off_nothing_changes():
    """two epochs with augment=None against the same call without the keyword: the code path of before, the same bits, and
    no new key in parameters.json"""
    config = MODELS["conv"]
    (train, test) = _sets(config)
    runs = []
    for keywords in ({}, dict(augment=None)):
        (make, _, _, _) = config
        torch.manual_seed(7)
        mt = make(batch_size=BATCH, nr_epochs=2, test_interval=1, lr=1e-3, weight_decay=1e-5)
        with redirect_stdout(io.StringIO()):
            mt.train(["lo"], "hi", train, test, **keywords)
        assert mt._augmenter is None and "augment" not in mt.get_parameters() and "augment_seed" not in mt.get_parameters()
        runs.append((mt, _state(mt), mt.history, [["-"]], None))
    _same(runs[0], runs[1], "augment=None")


def test_the_model_folder_keeps_the_setting_and_the_cli_passes_it(tmp_path):
    from cae_tools_amd.cli import train_cae
    from cae_tools_amd.models.model_loader import load_model
    config = MODELS["linear"]
    (train, test) = _sets(config)
    (tr, te, folder) = (str(tmp_path / "train.nc"), str(tmp_path / "test.nc"), str(tmp_path / "m"))
    train.to_netcdf(tr)
    test.to_netcdf(te)
    common = ["--train-inputs", tr, "--test-inputs", te, "--model-folder", folder, "--input-variables", "lo", "--output-variable",
              "hi", "--method", "linear", "--nr-epochs", "1", "--batch-size", "5"]
    with redirect_stdout(io.StringIO()):
        train_cae.main(common + ["--augment", "dihedral", "--augment-seed", "3"])
    with open(os.path.join(folder, "parameters.json")) as f:
        stored = json.load(f)
    assert (stored["augment"], stored["augment_seed"]) == ("dihedral", 3)
    with redirect_stdout(io.StringIO()):
        mt = load_model(folder)
    assert (mt.augment, mt.augment_seed) == ("dihedral", 3)
    # --continue-training: the folder's values are the defaults, a flag given overrides them
    with redirect_stdout(io.StringIO()):
        train_cae.main(common + ["--continue-training", "--augment", "flips"])
    with open(os.path.join(folder, "parameters.json")) as f:
        stored = json.load(f)
    assert (stored["augment"], stored["augment_seed"]) == ("flips", 3)
