"""evaluate_cae on the GPU: cae_case_measures (the per-case mae / mse of ModelEvaluator.compute_measure,
model_evaluator.py:87-95) against numpy in fp64 for every element kind, shape and layout it takes, and the whole
train_cae -> apply_cae -> evaluate_cae sequence for the four model types."""
import base64
import ctypes as C
import io
import json
import os
import re
import sqlite3
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from golden.make_golden_report import report_items
from cae_tools_amd import _lib
from cae_tools_amd.engine import case_measures

pytestmark = pytest.mark.gpu


def _numpy_measures(p, a):
    d = np.asarray(p, dtype=np.float64)[:, 0] - np.asarray(a)[:, 0].astype(np.float64)
    return np.stack([np.abs(d).mean(axis=(1, 2)), (d ** 2).mean(axis=(1, 2))], axis=1)


def _close(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def _netcdf_slabs(tmp_path, name, p, a):
    """p and a written to a NetCDF-3 file and read back as the big-endian views of its mapping that the loader hands on"""
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import as_numpy, open_dataset
    dims = {"n": p.shape[0], "c": p.shape[1], "ca": a.shape[1], "y": p.shape[2], "x": p.shape[3]}
    path = str(tmp_path / f"{name}.nc")      # one file per pair: the views map it
    netcdf3.write(path, dims, {"pred": (("n", "c", "y", "x"), p, {}), "target": (("n", "ca", "y", "x"), a, {})})
    ds = open_dataset(path)
    (pb, ab) = (as_numpy(ds["pred"]), as_numpy(ds["target"]))
    assert pb.dtype.byteorder == ">" and ab.dtype.byteorder == ">"
    return pb, ab


@pytest.mark.parametrize("shape", [(1, 1), (63, 64), (255, 257), (256, 256)])
@pytest.mark.parametrize("channels", [1, 3])
def test_every_kind_matches_numpy(tmp_path, shape, channels):
    rng = np.random.default_rng(shape[0] * 10 + channels)
    n = 5
    p64 = 290 + 5 * rng.random((n, channels) + shape)
    a32 = (290 + 5 * rng.random((n, channels) + shape)).astype(np.float32)
    (p32, a64) = (p64.astype(np.float32), a32.astype(np.float64) + 1e-3 * rng.random(a32.shape))
    (p64be, a32be) = _netcdf_slabs(tmp_path, "p64_a32", p64, a32)
    (p32be, a64be) = _netcdf_slabs(tmp_path, "p32_a64", p32, a64)
    dev = torch.device("cuda")
    for (p, a, pn, an) in [(p64, a32, p64, a32), (p32, a64, p32, a64), (p64be, a32be, p64, a32), (p32be, a64be, p32, a64),
                           (p64be, a64, p64, a64), (p32, a32be, p32, a32),
                           (torch.from_numpy(p64).to(dev), a32be, p64, a32),
                           (torch.from_numpy(p32).to(dev), torch.from_numpy(a32).to(dev), p32, a32)]:
        _close(case_measures(p, a), _numpy_measures(pn, an))


def _raw_measures(p_dev, pk, p_off, ps, a_dev, ak, a_off, as_, n, plane):
    """cae_case_measures on element offsets into flat device buffers (case starts of any alignment), as (mae, mse)"""
    lib = _lib.load()
    (pe, ae) = (4 if pk in (0, 1) else 8, 4 if ak in (0, 1) else 8)
    out = torch.empty((n, 2), dtype=torch.float64, device=p_dev.device)
    need = int(lib.cae_case_measures_workspace_bytes(n, plane))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=p_dev.device)
    _lib.check(lib.cae_case_measures(p_dev.data_ptr() + p_off * pe, pk, ps, a_dev.data_ptr() + a_off * ae, ak, as_, n,
                                     plane, out.data_ptr(), ws.data_ptr(), need, None))
    return out.cpu().numpy() / plane


@pytest.mark.parametrize("plane,stride_p,stride_a", [(4099, 4101, 4103), (13, 13, 15), (65536, 65537, 65539),
                                                     (5, 7, 6), (9000, 9001, 9000)])
@pytest.mark.parametrize("offsets", [(1, 3), (0, 1), (2, 2)])
def test_unaligned_case_starts(plane, stride_p, stride_a, offsets):
    """fp32 cases that start at every 4-byte phase of a 16-byte line, against fp32 and fp64 partners"""
    rng = np.random.default_rng(plane + offsets[0])
    n = 6
    (po, ao) = offsets
    pf = rng.random(po + n * stride_p).astype(np.float32)
    af = rng.random(ao + n * stride_a).astype(np.float32)
    a64 = rng.random(ao + n * stride_a)
    cases = lambda buf, off, st: np.stack([buf[off + i * st: off + i * st + plane] for i in range(n)])  # noqa: E731
    want32 = cases(pf, po, stride_p).astype(np.float64) - cases(af, ao, stride_a)
    want64 = cases(pf, po, stride_p).astype(np.float64) - cases(a64, ao, stride_a)
    (pd, ad, a64d) = (torch.from_numpy(pf).cuda(), torch.from_numpy(af).cuda(), torch.from_numpy(a64).cuda())
    for (adev, ak, want) in ((ad, _lib.ELEM_F32, want32), (a64d, _lib.ELEM_F64, want64)):
        got = _raw_measures(pd, _lib.ELEM_F32, po, stride_p, adev, ak, ao, stride_a, n, plane)
        _close(got, np.stack([np.abs(want).mean(axis=1), (want ** 2).mean(axis=1)], axis=1))


def test_seventy_thousand_cases():
    rng = np.random.default_rng(70000)
    p = rng.random((70000, 1, 1, 4))
    a = rng.random((70000, 2, 1, 4)).astype(np.float32)
    _close(case_measures(p, a), _numpy_measures(p, a))


def test_nan_and_inf_stay_in_their_case():
    rng = np.random.default_rng(5)
    p = rng.random((7, 1, 63, 65))
    a = rng.random((7, 1, 63, 65)).astype(np.float32)
    p[1, 0, 10, 3] = np.nan
    a[3, 0, 62, 64] = np.inf
    p[5, 0, 0, 0] = np.inf
    a[5, 0, 0, 0] = np.inf             # inf - inf: NaN
    p[6, 0, 30, 31] = -np.inf
    got = case_measures(p, a)
    with np.errstate(invalid="ignore"):
        want = _numpy_measures(p, a)
    assert np.isnan(got[1]).all() and np.isnan(got[5]).all()
    assert np.isposinf(got[3]).all() and np.isposinf(got[6]).all()
    for i in (0, 2, 4):
        _close(got[i], want[i])


def test_two_runs_agree_bit_for_bit():
    rng = np.random.default_rng(11)
    p = torch.from_numpy(rng.random((40, 1, 256, 256))).cuda()
    a = torch.from_numpy(rng.random((40, 1, 256, 256)).astype(np.float32)).cuda()
    first = case_measures(p, a)
    second = case_measures(p.clone(), a.clone())
    assert first.tobytes() == second.tobytes()


# ---- train_cae -> apply_cae -> evaluate_cae ---------------------------------------------------

def _svgs(page):
    return [base64.b64decode(m).decode() for m in re.findall(r'src="data:image/svg\+xml;base64,([A-Za-z0-9+/=]+)"', page)]


def _bar_counts(svg):
    return [int(c) for c in re.findall(r'<rect class="bar" data-count="(\d+)"', svg)]


def _table(items, title):
    """the rows of the table after heading `title`, header row first"""
    k = items.index(["h3", title]) + 1
    rows = []
    while k < len(items) and items[k][0] == "tr":
        rows.append(items[k][1].split("|"))
        k += 1
    return rows


def _square(ds):
    """the circle data at 64 x 64 on both sides (a UNET's decoder mirrors its encoder): the 16 x 16 input repeated 4 x 4,
    the 256 x 256 target averaged over 4 x 4 blocks"""
    from cae_tools_amd.data.arrays import DataArray, Dataset
    lo = np.asarray(ds["lowres"].values)
    hi = np.asarray(ds["hires"].values)
    out = Dataset()
    out["hires"] = DataArray(hi.reshape(hi.shape[0], 1, 64, 4, 64, 4).mean(axis=(3, 5)).astype(np.float32),
                             dims=("n", "chan", "y", "x"))
    out["lowres"] = DataArray(np.repeat(np.repeat(lo, 4, axis=2), 4, axis=3), dims=("n", "chan", "y", "x"))
    return out


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from cae_tools_amd.data import datagen
    root = tmp_path_factory.mktemp("evaluate")
    paths = {}
    for (part, n, seed) in (("train", 20, 1234), ("test", 12, 4321)):
        ds = datagen.generate("circle", n, seed=seed)
        paths[part] = str(root / f"{part}.nc")
        ds.to_netcdf(paths[part])
        paths["square_" + part] = str(root / f"square_{part}.nc")
        _square(ds).to_netcdf(paths["square_" + part])
    return root, paths


ANALYSES = {"skill_maps": {"skill_maps": True}, "spectra": {"spectra": True}, "ssim": {"ssim": True},
            "baseline": {"baseline": True, "baseline_mode": "bilinear"}, "distribution": {"distribution": True, "distribution_bins": 32}}


def test_analyses_together_equal_each_alone(tmp_path):
    """The five analyses switched on together share their operands on the GPU; each alone uploads its own.  Every
    <analysis>_test.json and skill_test.nc and every per-case variable is the same bytes either way, for a scored file and for
    an unscored one whose prediction comes from apply_device."""
    from cae_tools_amd.cli import apply_cae, train_cae
    from cae_tools_amd.data import datagen
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    paths = {part: str(tmp_path / f"{part}.nc") for part in ("train", "test")}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        datagen.generate("circle", 12, seed=seed).to_netcdf(paths[part])
    (model, scored) = (str(tmp_path / "model"), str(tmp_path / "scored_test.nc"))
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                        "--input-variables", "lowres", "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"])
        apply_cae.main([paths["test"], scored, "--model-folder", model])

    class Recording(ModelEvaluator):
        def build_html(self, case_dimension, train_ds, test_ds, model_metrics):
            before = set(test_ds.keys())
            super().build_html(case_dimension, train_ds, test_ds, model_metrics)
            self.added = {k: np.asarray(test_ds[k].values).tobytes() for k in test_ds.keys() if k not in before}

    def run(name, source, options):
        """(the files {name: bytes} an analysis writes per partition, the per-case variables {name: bytes})"""
        out = str(tmp_path / f"report_{name}")
        with redirect_stdout(io.StringIO()):
            ev = Recording([], [source], output_html_folder=out, model_path=model, **options)
            ev.run()
        files = {}
        for f in sorted(os.listdir(out)):
            if f.endswith("_test.json") or f == "skill_test.nc":
                with open(os.path.join(out, f), "rb") as fh:
                    files[f] = fh.read()
        return files, ev.added

    sources = {"scored": scored, "unscored": paths["test"]}
    together = {kind: run(f"all_{kind}", source, {k: v for o in ANALYSES.values() for (k, v) in o.items()})
                for (kind, source) in sources.items()}
    for (kind, (files, added)) in together.items():
        assert sorted(files) == ["baseline_test.json", "distribution_test.json", "skill_test.nc", "spectra_test.json", "ssim_test.json"]
        # the unscored data set also gets the prediction apply_device has made
        assert sorted(added) == sorted(["baseline_mse", "mae", "ms_ssim", "mse", "psnr", "skill", "ssim"]
                                       + ["model_output"] * (kind == "unscored"))
    for (k, (name, options)) in enumerate(ANALYSES.items()):
        kind = ("scored", "unscored")[k % 2]
        (files, added) = run(f"{name}_{kind}", sources[kind], options)
        assert len(files) == 1 and {"mae", "mse"} <= set(added)
        for (f, data) in files.items():
            assert data == together[kind][0][f], f"{f} of {name} alone ({kind})"
        for (v, data) in added.items():
            assert data == together[kind][1][v], f"{v} of {name} alone ({kind})"


@pytest.mark.parametrize("method", ["conv", "unet", "var", "linear"])
def test_train_apply_evaluate(data, method):
    from cae_tools_amd.cli import apply_cae, evaluate_cae, train_cae
    from cae_tools_amd.data.arrays import as_numpy, open_dataset
    from cae_tools_amd.models.ds_dataset import DSDataset
    from cae_tools_amd.models.model_loader import load_model
    (root, paths) = data
    extra = []
    if method == "unet":       # a UNET's layers come from a definitions file (cli/train_cae.py:143-147)
        from cae_tools_amd.models.unet import unet_layer_spec
        paths = {"train": paths["square_train"], "test": paths["square_test"]}
        layers = str(root / "unet_layers.json")
        with open(layers, "w") as f:
            json.dump(unet_layer_spec(1, 1, (64, 64), [8, 16]).save(), f)
        extra = ["--layer-definitions-path", layers]
    model = str(root / f"model_{method}")
    scored = str(root / f"scored_{method}.nc")
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                        "--input-variables", "lowres", "--output-variable", "hires", "--method", method, "--nr-epochs", "2",
                        "--batch-size", "10", "--latent-size", "4", "--fc-size", "16"] + extra)
        apply_cae.main([paths["test"], scored, "--model-folder", model])

    db = str(root / f"db_{method}.db")
    out1 = str(root / f"report_{method}_scored")
    log = io.StringIO()
    with redirect_stdout(log):
        evaluate_cae.main(["--test-inputs", scored, "--model-folder", model, "--output-html-folder", out1,
                           "--database-path", db, "--input-variables", "lowres"])
    printed = log.getvalue()
    assert "Evaluating training cases: 0, test cases: 12" in printed and "Applying model" not in printed
    out2 = str(root / f"report_{method}_apply")
    log = io.StringIO()
    with redirect_stdout(log):
        evaluate_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                           "--output-html-folder", out2])
    assert "Applying model to generate train scores" in log.getvalue()
    assert "Applying model to generate test scores" in log.getvalue()

    # the metric tables are model.evaluate() formatted 0.3f
    mt = load_model(model)
    want = {}
    with redirect_stdout(io.StringIO()):
        for (part, path) in (("test", paths["test"]), ("train", paths["train"])):
            ds = DSDataset(open_dataset(path), ["lowres"], "hires", normalise_in=mt.normalise_input, normalise_out=False)
            ds.set_normalisation_parameters(mt.normalisation_parameters)
            want[part] = mt.evaluate(ds)
    pages = {}
    for out in (out1, out2):
        with open(os.path.join(out, "index.html")) as f:
            pages[out] = f.read()
    items1, items2 = report_items(pages[out1]), report_items(pages[out2])
    assert _table(items1, "Test Metrics")[1:] == [[k, f"{v:0.3f}"] for k, v in want["test"].items()]
    assert _table(items2, "Train Metrics")[1:] == [[k, f"{v:0.3f}"] for k, v in want["train"].items()]
    assert ["h3", "Train Metrics"] not in items1

    # per-case measures of the scored file against numpy, and the histograms drawn from them
    sds = open_dataset(scored)
    (pred, target) = (as_numpy(sds["model_output"]), as_numpy(sds["hires"]))
    assert pred.dtype == np.dtype(">f8") and target.dtype == np.dtype(">f4")
    got = case_measures(pred, target)
    ref = _numpy_measures(pred, target)
    _close(got, ref)
    svgs1 = _svgs(pages[out1])
    assert len(svgs1) == 3
    for (k, svg) in enumerate(svgs1[:2]):
        assert _bar_counts(svg) == np.histogram(ref[:, k], bins="auto")[0].tolist()
    # the apply path measures the prediction it has just made on the GPU: the same histograms for the test partition
    svgs2 = _svgs(pages[out2])
    assert len(svgs2) == 5
    assert [_bar_counts(s) for s in svgs2[:2]] == [_bar_counts(s) for s in svgs1[:2]]

    # history plot and parameters table
    with open(os.path.join(model, "parameters.json")) as f:
        params = json.load(f)
    with open(os.path.join(model, "history.json")) as f:
        history = json.load(f)
    assert 'data-name="train"' in svgs1[-1] and 'data-name="test"' in svgs1[-1]
    k = items1.index(["h2", "Training Parameters"])
    rows = [r[1] for r in items1[k + 1:] if r[0] == "tr"]
    assert rows == ["Parameter Name|Parameter Value", f"total epochs|{history['nr_epochs']}"] + \
        [f"{key}|{value}" for key, value in params.items()]
    assert items1[-1] == ["img", ""]

    # one MODEL_EVALUATIONS row whose metrics are the printed ones
    with sqlite3.connect(db) as conn:
        rows = conn.execute("SELECT model_id, train_path, test_path, metrics FROM MODEL_EVALUATIONS").fetchall()
    assert len(rows) == 1
    (model_id, train_path, test_path, metrics) = rows[0]
    assert (model_id, train_path, test_path) == (mt.get_model_id(), "", scored)
    metrics = json.loads(metrics)
    for (key, value) in metrics["test"].items():
        assert f"\t{key:30s}:{value}" in printed
        # model.evaluate() again: cae_metric_sums folds its chunks with fp64 atomics, so only close, not the same bits
        assert value == pytest.approx(float(want["test"][key]), rel=1e-9, abs=1e-12)
