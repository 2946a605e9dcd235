"""ModelEvaluator.build_html frozen, without a GPU: every file it writes, every line it prints, every variable it adds to
the data sets and the sequence of its GPU calls, for four configurations, with the GPU calls replaced by small numpy
stand-ins (their numerics are tested elsewhere); and the constructor's refusals in their order.  The frozen values are
the sha256 strings below, with the lines they are taken over in tests/golden/evaluator_freeze.json.  A PNG is hashed after
inflating its IDAT, the one embedded in distribution/index.html included: deflate's bytes may differ between zlib builds."""
import base64
import hashlib
import io
import json
import os
import re
import struct
import zlib
from contextlib import redirect_stdout

import numpy as np
import pytest

from cae_tools_amd.data.arrays import DataArray, Dataset, as_numpy
from cae_tools_amd.utils import ensemble_scores, spectra, ssim
from test_evaluator_cpu import _model_folder

# where the evaluator looks its GPU calls up: (module, names); a name is replaced wherever a module has it
PATCH_MODULES = ("cae_tools_amd.models.model_evaluator", "cae_tools_amd.models.evaluation_analyses")
GPU_CALLS = ("device_operand", "case_measures", "case_range", "render_cases", "pixel_sums", "case_spectra", "case_ssim",
             "case_baseline", "joint_histogram")


# ---- the stand-ins -----------------------------------------------------------------------------

class Operand:
    """what the stand-in device_operand returns: the fp64 copy of the array, its shape and the name of its source"""

    def __init__(self, x, label):
        self.tensor = np.asarray(x, dtype=np.float64)
        self.shape = tuple(self.tensor.shape)
        self.label = label


class Calls:
    """the stand-ins of one build_html: `log` holds one line per call but device_operand's, `uploads` the label of every
    array that reached device_operand as something other than an operand"""

    def __init__(self, partitions):
        self.names = {}
        self.keep = []          # the arrays named, so that no id is used twice
        for (partition, ds) in partitions:
            if ds is not None:
                for v in ds.keys():
                    arr = as_numpy(ds[v])
                    self.names[id(arr)] = f"{partition}:{v}"
                    self.keep.append(arr)
        self.log = []
        self.uploads = []

    def label(self, x):
        if x is None:
            return "None"
        if isinstance(x, Operand):
            return x.label
        return self.names.get(id(x), f"array{tuple(np.shape(x))}")

    def note(self, name, *operands, **kw):
        extra = "".join(f", {k}={v}" for (k, v) in kw.items())
        self.log.append(f"{name}({', '.join(self.label(x) for x in operands)}{extra})")

    def device_operand(self, x, device=None):
        if isinstance(x, Operand):
            return x
        self.uploads.append(self.label(x))
        return Operand(x, self.label(x))

    @staticmethod
    def plane(x):
        """channel 0 as (N, H, W) float64"""
        return (x.tensor if isinstance(x, Operand) else np.asarray(x, dtype=np.float64))[:, 0]

    def case_measures(self, pred, actual, device=None):
        self.note("case_measures", pred, actual)
        d = self.plane(pred) - self.plane(actual)
        return np.stack([np.abs(d).mean(axis=(1, 2)), (d * d).mean(axis=(1, 2))], axis=1)

    def case_range(self, arr, sub=None, device=None):
        self.note("case_range", arr, sub)
        v = self.plane(arr) - (self.plane(sub) if sub is not None else 0.0)
        v = v[np.isfinite(v)]
        return (float(v.min()), float(v.max()), int(v.size)) if v.size else (float("inf"), float("-inf"), 0)

    def render_cases(self, arr, lo, hi, cases=None, sub=None, flip_y=False, device=None):
        self.note("render_cases", arr, sub, lo=lo, hi=hi, cases=list(cases) if cases is not None else None, flip_y=bool(flip_y))
        v = self.plane(arr) - (self.plane(sub) if sub is not None else 0.0)
        v = v[np.arange(v.shape[0]) if cases is None else np.asarray(cases, dtype=np.int64)]
        with np.errstate(invalid="ignore"):
            t = np.clip((v - lo) / (hi - lo), 0.0, 1.0) if hi > lo else np.where(np.isnan(v), np.nan, 0.5)
            index = np.where(np.isnan(v), 0, 1 + np.floor(254.0 * np.nan_to_num(t) + 0.5)).astype(np.uint8)
        if flip_y:
            index = index[:, ::-1]
        return np.concatenate([np.zeros(index.shape[:2] + (1,), dtype=np.uint8), index], axis=2)

    def pixel_sums(self, pred, actual, shift=0.0, case_chunk=0, device=None):
        self.note("pixel_sums", pred, actual, shift="scalar" if np.ndim(shift) == 0 else "per pixel")
        (p, a) = (self.plane(pred), self.plane(actual))
        ok = np.isfinite(p) & np.isfinite(a)
        shift = np.broadcast_to(np.asarray(shift, dtype=np.float64), (2,) + p.shape[1:])
        (d, a1, p1) = (np.where(ok, p - a, 0.0), np.where(ok, a - shift[0], 0.0), np.where(ok, p - shift[1], 0.0))
        return np.stack([ok.sum(axis=0).astype(np.float64), d.sum(axis=0), np.abs(d).sum(axis=0), (d * d).sum(axis=0),
                         a1.sum(axis=0), p1.sum(axis=0), (a1 * a1).sum(axis=0), (p1 * p1).sum(axis=0), (a1 * p1).sum(axis=0)])

    def case_spectra(self, pred, actual, device=None):
        self.note("case_spectra", pred, actual)
        (p, a) = (self.plane(pred), self.plane(actual))
        m = spectra.bin_count(*p.shape[1:])
        counted = np.isfinite(p).all(axis=(1, 2)) & np.isfinite(a).all(axis=(1, 2))
        b = np.arange(1, m + 1, dtype=np.float64)
        sums = np.stack([64.0 / (b * b), 64.0 / b, 48.0 / (b * b), 16.0 / b], axis=1)[None] * (1.0 + np.arange(p.shape[0]))[:, None, None]
        return np.where(counted[:, None, None], sums, 0.0), counted

    def case_ssim(self, pred, actual, vmin, vmax, n_scale=None, device=None):
        self.note("case_ssim", pred, actual, vmin=vmin, vmax=vmax)
        (p, a) = (self.plane(pred), self.plane(actual))
        n_scale = ssim.default_scales(*p.shape[1:])
        ok = np.isfinite(p).all(axis=(1, 2)) & np.isfinite(a).all(axis=(1, 2))
        n = np.where(ok, 2916.0, 0.0)
        share = 1.0 - 0.0625 * (1 + np.arange(p.shape[0]) % 4)
        return np.repeat(np.stack([n, n * share, n * (share + 0.03125)], axis=1)[:, None], n_scale, axis=1)

    def case_baseline(self, low, pred, actual, mode="bicubic", field=False, device=None):
        self.note("case_baseline", low, pred, actual, mode=mode)
        (lo, p, a) = (self.plane(low), self.plane(pred), self.plane(actual))
        f = a.shape[1] // lo.shape[1]
        b = np.repeat(np.repeat(lo, f, axis=1), f, axis=2)
        ok = np.isfinite(a) & np.isfinite(p) & np.isfinite(b)
        (db, dp) = (np.where(ok, b - a, 0.0), np.where(ok, p - a, 0.0))
        total = lambda v: v.sum(axis=(1, 2)).astype(np.float64)      # noqa: E731
        return np.stack([total(ok), total(np.abs(db)), total(db * db), total(np.abs(dp)), total(dp * dp),
                         total(ok & (np.abs(dp) < np.abs(db)))], axis=1)

    def joint_histogram(self, pred, actual, lo, hi, n_bin=128, sub=8, device=None):
        self.note("joint_histogram", pred, actual, lo=lo, hi=hi, n_bin=n_bin, sub=sub)
        (p, a) = (self.plane(pred), self.plane(actual))
        ok = np.isfinite(p) & np.isfinite(a)
        (p, a) = (p[ok], a[ok])
        n_fine = n_bin * sub
        fine = lambda v: np.clip(np.floor((v - lo) * (n_fine / (hi - lo))), 0, n_fine - 1).astype(np.int64)      # noqa: E731
        (fa, fp) = (fine(a), fine(p))
        joint = np.zeros((n_bin, n_bin), dtype=np.int64)
        np.add.at(joint, (fa // sub, fp // sub), 1)
        marg = np.stack([np.bincount(fa, minlength=n_fine), np.bincount(fp, minlength=n_fine)]).astype(np.int64)
        d = p - a
        cond = np.zeros((2, n_bin, 4))
        for (k, (key, own)) in enumerate(((fa // sub, a), (fp // sub, p))):
            for (j, v) in enumerate((d, np.abs(d), d * d, own - lo)):
                cond[k, :, j] = np.bincount(key, weights=v, minlength=n_bin)
        outside = np.array([(a < lo).sum(), (a > hi).sum(), (p < lo).sum(), (p > hi).sum()], dtype=np.int64)
        return joint, marg, cond, outside


class VarAEModel:
    """a stand-in for load_model's result in configuration D: what the evaluator reads of a model, and a verify_ensemble
    of synthetic sums"""
    normalisation_parameters = [{"lowres": 0.0}, {"lowres": 1.0}, 0.0, 1.0]

    def __init__(self, path):
        self.path = path

    def get_model_id(self):
        return "frozen-var"

    def get_input_variable_names(self):
        return ["lowres"]

    def get_output_variable_name(self):
        return "hires"

    def verify_ensemble(self, score_ds, input_variables, output_variable, ensemble_size, ensemble_seed=0):
        n = int(score_ds[output_variable].shape[0])
        k = int(ensemble_size)
        case = 1.0 + np.arange(n, dtype=np.float64)
        sums = np.stack([np.full(n, 4096.0), 512.0 * case, 128.0 * case, 64.0 * case, 32.0 * case], axis=1)
        sums[n - 1] = 0.0           # a case without a counted pixel: its crps is null in the file
        ranks = np.array([100 * (j + 1) for j in range(k + 1)] + [7], dtype=np.int64)
        return {**ensemble_scores.scores_from_sums(sums, ranks, k), "case_sums": sums, "ensemble_seed": int(ensemble_seed)}


# ---- the model folder and the data ---------------------------------------------------------------

@pytest.fixture(scope="module")
def model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("freeze") / "model")
    _model_folder(path)
    with open(os.path.join(path, "parameters.json")) as f:
        parameters = json.load(f)
    parameters["model_id"] = "frozen-model-id"      # a fresh id each run otherwise: index.html prints the parameters
    with open(os.path.join(path, "parameters.json"), "w") as f:
        json.dump(parameters, f)
    with open(os.path.join(path, "history.json"), "w") as f:
        json.dump({"nr_epochs": 3, "train_loss": [0.5, 0.25, 0.125], "test_loss": [0.75, 0.5, 0.375]}, f)
    return path


def _dataset(n, seed):
    """n cases: hires fp32 64 x 64, model_output fp64, lowres 16 x 16 stored as >f4, 1-D y and x, time along the cases.
    The values are small multiples of 1/32, so that every sum of them is exact in whatever order it is taken."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 17, size=(n, 1, 16, 16)) / 16.0
    target = np.repeat(np.repeat(low, 4, axis=2), 4, axis=3) + rng.integers(-2, 3, size=(n, 1, 64, 64)) / 16.0
    pred = target + rng.integers(-4, 5, size=target.shape) / 32.0
    target[0, 0, 5, 7] = np.nan         # one case whose measures are NaN
    ds = Dataset()
    ds["hires"] = DataArray(target.astype(np.float32), dims=("case", "chan", "y", "x"))
    ds["model_output"] = DataArray(pred, dims=("case", "chan", "y", "x"))
    ds["lowres"] = DataArray(low.astype(">f4"), dims=("case", "chan", "ylo", "xlo"))
    ds["y"] = DataArray(np.arange(64, dtype=np.float64), dims=("y",))
    ds["x"] = DataArray(np.arange(64, dtype=np.float64) * 0.5, dims=("x",))
    ds["time"] = DataArray(np.arange(n, dtype=np.float64) * 6.0, dims=("case",), attrs={"units": "hours since 2000-01-01"})
    return ds


METRICS = {"test": {"mse": 0.0625, "mae": 0.125}, "train": {"mse": 0.03125, "mae": 0.0625}}
OPTIONS = dict(skill_maps=True, spectra=True, ssim=True, baseline=True, baseline_mode="bilinear", distribution=True,
               distribution_bins=16)
PAGES = dict(input_variables=["lowres"], sample_count=3, x_coordinate="x", y_coordinate="y", time_coordinate="time")
CONFIGURATIONS = {"A": (True, {**OPTIONS, **PAGES}), "B": (True, OPTIONS), "C": (False, {}), "D": (True, {"ensemble_size": 4})}


# ---- what is frozen ------------------------------------------------------------------------------

def _png_digest(data):
    """sha256 over a PNG's chunks with the IDAT stream inflated"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    (h, k, idat) = (hashlib.sha256(), 8, b"")
    while k < len(data):
        (size,) = struct.unpack(">I", data[k:k + 4])
        (kind, body) = (data[k + 4:k + 8], data[k + 8:k + 8 + size])
        if kind == b"IDAT":
            idat += body
        else:
            h.update(kind + body)
        k += 12 + size
    h.update(zlib.decompress(idat))
    return h.hexdigest()


def _file_digest(path):
    with open(path, "rb") as f:
        data = f.read()
    if path.endswith(".png"):
        return _png_digest(data)
    if path.endswith(".html"):
        data = re.sub(rb"data:image/png;base64,([A-Za-z0-9+/=]+)",
                      lambda m: b"png:" + _png_digest(base64.b64decode(m.group(1))).encode(), data)
    return hashlib.sha256(data).hexdigest()


def _digest_of(lines):
    return hashlib.sha256("\n".join(lines).encode("utf-8")).hexdigest()


def _run(model, tmp_path, monkeypatch, name):
    """one build_html of configuration `name`: (files {relative path: digest}, printed lines, variables [(partition, name,
    digest)], the Calls)"""
    import importlib
    from cae_tools_amd.models import model_evaluator
    (with_train, options) = CONFIGURATIONS[name]
    (train, test) = (_dataset(5, 11) if with_train else None, _dataset(4, 12))
    before = {p: list(ds.keys()) for (p, ds) in (("train", train), ("test", test)) if ds is not None}
    calls = Calls((("train", train), ("test", test)))
    for module in PATCH_MODULES:
        module = importlib.import_module(module)
        for call in GPU_CALLS:
            if hasattr(module, call):
                monkeypatch.setattr(module, call, getattr(calls, call))
    if "ensemble_size" in options:
        monkeypatch.setattr(model_evaluator, "load_model", VarAEModel)
    out = str(tmp_path / f"report_{name}")
    log = io.StringIO()
    with redirect_stdout(log):
        ev = model_evaluator.ModelEvaluator(None, None, output_html_folder=out, model_path=model, **options)
        ev.build_html("case", train, test, METRICS)
    files = {}
    for (folder, _, found) in os.walk(out):
        for f in found:
            path = os.path.join(folder, f)
            files[os.path.relpath(path, out).replace(os.sep, "/")] = _file_digest(path)
    printed = [line for line in log.getvalue().splitlines() if not line.startswith("Evaluating model id=")]
    variables = [(p, v, hashlib.sha256(np.asarray(ds[v].values).tobytes()).hexdigest()[:16])
                 for (p, ds) in (("test", test), ("train", train)) if ds is not None for v in ds.keys() if v not in before[p]]
    return dict(sorted(files.items())), printed, variables, calls


def _frozen():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluator_freeze.json")) as f:
        return json.load(f)


# sha256 per configuration of: the "path digest" lines of every file written, sorted by path; the printed lines; the
# "partition variable digest" lines of the variables added to the data sets, in order; the GPU calls, in order.
# tests/golden/evaluator_freeze.json holds the lines themselves, which is what a failure is compared against.
FROZEN_SHA256 = {
    "A": {"files": "a78c1c4081fe75c3b2404116e3f956cc83f7e72ec63c5b2312cf5aedfe6aff4a",
          "printed": "dbea29ba2b5c3ee33b77b40a6acd598feb9e94d441ac6d8288bac2b3b081f6b2",
          "variables": "5b597d73ae9a1454ca33a65c00dacbba5f4e36d837bd7fe39ef8da367c4814f5",
          "calls": "a75bffaf4a7c9988c0065f653a18d63c88969ff7cfc27133b61d753dba63ac5b"},
    "B": {"files": "67ec983ae9b6a9a4baa12dd6329052ed45460d94c6f0f4109a8ce8d187d5b427",
          "printed": "dbea29ba2b5c3ee33b77b40a6acd598feb9e94d441ac6d8288bac2b3b081f6b2",
          "variables": "5b597d73ae9a1454ca33a65c00dacbba5f4e36d837bd7fe39ef8da367c4814f5",
          "calls": "47daba842d8163255da4034697b3c06f52c98e0d27f884d78d33e983176789dd"},
    "C": {"files": "878d32f80f0ee2a59f0a182e93bedb3fc64cac649b02a1a06f52963c6b4b78b8",
          "printed": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
          "variables": "1c0d456e64ebbe145ab350bc885213492cf5aa6a957e6298e8252f3e99110e0c",
          "calls": "c78604e087bf56f6ac3a565cf06896e8a479866de7ccbcd5e1ad42f4f7ac9017"},
    "D": {"files": "a00842f4d451afcf47d87210bfd1b1daa3574c2fdacaefbe5e24e2c917231d3d",
          "printed": "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855",
          "variables": "9507ea7146a842aeba342f24a485ad92f85a45eee245004e772bb8d2eeaeb5a9",
          "calls": "5fea09720011314dc73ff942b322374ca9114b1b70ae5bda0327c1bf3e239ba6"},
}


@pytest.mark.parametrize("name", sorted(CONFIGURATIONS))
def test_build_html_is_frozen(model, tmp_path, monkeypatch, name):
    (files, printed, variables, calls) = _run(model, tmp_path, monkeypatch, name)
    got = {"files": [f"{k} {v}" for (k, v) in files.items()], "printed": printed,
           "variables": [" ".join(v) for v in variables], "calls": calls.log}
    want = _frozen()[name]
    for key in ("files", "printed", "variables", "calls"):
        assert got[key] == want[key], f"configuration {name}: {key}"
        assert _digest_of(got[key]) == FROZEN_SHA256[name][key], f"configuration {name}: {key}"
    assert len(files) == {"A": 55, "B": 27}.get(name, len(files))


@pytest.mark.parametrize("name", sorted(CONFIGURATIONS))
def test_no_array_is_uploaded_twice(model, tmp_path, monkeypatch, name):
    """within one build_html no array of a data set reaches device_operand as something other than an operand twice"""
    calls = _run(model, tmp_path, monkeypatch, name)[3]
    named = [u for u in calls.uploads if ":" in u]
    assert sorted(named) == sorted(set(named))


def test_constructor_refusals_in_order(model, tmp_path):
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    nowhere = str(tmp_path / "no_model")
    bad = dict(baseline=True, baseline_mode="lanczos", distribution=True, distribution_bins=0, ensemble_size=1)
    steps = [({}, "baseline_mode must be one of nearest, bilinear, bicubic, got 'lanczos'"),
             ({"baseline_mode": "nearest"}, "distribution_bins must be an integer from 1 to 128, got 0"),
             ({"distribution_bins": 2.5}, "distribution_bins must be an integer from 1 to 128, got 2.5"),
             ({"distribution_bins": 128}, "ensemble_size must be an integer from 2 to 64, got 1"),
             ({"ensemble_size": 65}, "ensemble_size must be an integer from 2 to 64, got 65")]
    for (change, text) in steps:        # each refusal comes before the model is loaded: there is none at this path
        bad.update(change)
        with pytest.raises(ValueError) as refused:
            ModelEvaluator(None, None, model_path=nowhere, **bad)
        assert str(refused.value) == text
    with redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError) as refused:
            ModelEvaluator(None, None, model_path=model, **{**bad, "ensemble_size": 4})
    assert str(refused.value) == f"ensemble_size needs a VarAEModel (train_cae --method var): {model} holds a ConvAEModel"
    # options that are off are not checked
    with redirect_stdout(io.StringIO()):
        ModelEvaluator(None, None, model_path=model, baseline_mode="lanczos", distribution_bins=0)
