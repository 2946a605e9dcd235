"""ModelEvaluator — the evaluate_cae back end with the reference's constructor and run() / evaluate_model_metrics() /
build_html() / compute_measure() surface (src/cae_tools/models/model_evaluator.py).

The metrics are model.evaluate() (scoring and cae_metric_sums on the GPU).  The report's per-case mae / mse of channel 0
(:87-95, one numpy pass per case and measure there) are one streaming cae_case_measures pass per partition, reading the
NetCDF-3 slabs as the file stores them, or the prediction the evaluator has just produced where it is still on the GPU.
Departures from the reference: no output folder means metrics and database row only, not a crash on the
unset report path; a missing --prediction-variable means apply()'s default "model_output", not None; the plots are SVG
drawn by utils/report.py in place of seaborn PNGs.

The case pages (--x-coordinate, --y-coordinate and --time-coordinate all given) are netcdf2html's where that optional
package imports.  Elsewhere the package makes its own (utils/case_pages.py): <partition>/index.html with one row per
case, worst mse first, and channel 0 (only) of the requested input variables, the target, the prediction and the error
prediction - target as palette PNGs.  netcdf2html is not part of the reference tree, so ranges and colours are this
package's definition: each input variable is scaled over its own finite values in both partitions, target and
prediction share one range, the error is scaled over +-max|prediction - target| (cae_case_range); a pixel's palette
index is 0 for NaN and 1 + round-half-up(254 * clamp((v - lo) / (hi - lo), 0, 1)) otherwise, computed in fp64 on the GPU
(cae_render_cases) from the slabs as stored and from the prediction where it still lies in HBM.

skill_maps=True (cli/skill_maps.py; not a reference feature) adds the transposed reduction: per partition the per-pixel
count, bias, mae, rmse, correlation and sd_ratio of channel 0 over the cases, from two streaming passes over the operands
on the GPU (cae_pixel_sums about the midpoint of the output normalisation range, then cae_pixel_sums_about each pixel's
means for the variances; utils/skill_maps.py), written as skill_<partition>.nc beside index.html and drawn on
maps/index.html, which the report then links.  The six maps of a partition go to the GPU as six one-channel cases and are ranged and drawn by the case
pages' kernels; ranges go over both partitions (count over [0, largest number of cases], bias over +-max|bias|).

ensemble_size=K (cli/verify_ensemble.py; a VarAEModel only, not a reference feature) verifies the model's K-member ensemble
against the target per partition (VarAEModel.verify_ensemble, cae_ensemble_verify on the GPU): ensemble_<partition>.json
with the scores, rank counts, K and seed (strict JSON: a score that is not finite is null), a per-case crps variable beside mae / mse in the data set, and the report's
"Ensemble verification" section.

spectra=True (cli/spectra.py; not a reference feature) adds the reduction along scale: per partition the radially binned
power spectra of prediction and target, their ratio, the spectral coherence and the error spectrum of channel 0 from one
cae_case_spectra pass on the GPU (a direct fp64 DFT of every case; utils/spectra.py), written as
spectra_<partition>.json and drawn on spectra/index.html, which the report then links.

ssim=True (cli/ssim.py; not a reference feature) adds the structural scores: per partition and case the SSIM, the MS-SSIM
(five scales, where min(h, w) > 160) and the PSNR of channel 0 against the model's output normalisation range, from one
cae_case_ssim pass on the GPU (fp64, the VAE loss's definition with a rule for missing data; utils/ssim.py, DESIGN.md
section 9) and the mse already measured: ssim_<partition>.json, per-case ssim / ms_ssim / psnr variables beside mae / mse
in the data set, and the report's "Structural similarity" section.

baseline=True (cli/baseline.py; not a reference feature) answers whether the model is better than interpolating its own
input: channel 0 of baseline_variable (default: the model's first input variable) is interpolated to the target's grid
(baseline_mode "nearest", "bilinear" or "bicubic", torch's align_corners=False formulas) inside the kernel that compares it,
one cae_case_baseline pass on the GPU (fp64; utils/baseline.py): baseline_<partition>.json with the
pooled and per-case skill 1 - model_mse / baseline_mse, per-case baseline_mse / skill variables beside mae / mse in the
data set, and the report's "Skill against interpolation" section.

distribution=True (cli/distribution.py; not a reference feature) adds the reduction along value: per partition the joint
histogram of prediction against target over distribution_bins (1 to 128) coarse bins, the two fine marginal histograms and
the per-bin error sums of channel 0 from one cae_joint_hist pass on the GPU (utils/distribution.py)
over the range of the finite values of target and prediction in the partitions present (cae_case_range; hi = lo + 1 where
that range is degenerate): distribution_<partition>.json with the conditional bias, reliability, quantiles, Wasserstein-1
distance, Perkins score and exceedance scores, distribution/index.html with the joint density and the curves, and the
report's "Value distribution" section.
"""
import json
import os

import numpy as np

from ..data.arrays import as_numpy, open_mfdataset
from ..case_ops import (case_baseline, case_measures, case_range, case_spectra, case_ssim, device_operand, joint_histogram, pixel_sums,
                        render_cases)
from ..utils import baseline as baseline_scores
from ..utils import case_pages, ensemble_scores, skill_maps
from ..utils import distribution as distribution_curves
from ..utils import spectra as spectra_curves
from ..utils import ssim as ssim_scores
from ..utils.model_database import ModelDatabase
from ..utils.report import evaluation_report
from .base_model import _make_data_array
from .ds_dataset import DSDataset
from .model_loader import load_model

MEASURES = ("mae", "mse")


class ModelEvaluator:

    def __init__(self, training_paths, testing_paths, output_html_folder="", model_output_variable="", model_path="",
                 database_path="", input_variables=[], sample_count=None, x_coordinate="", y_coordinate="",
                 time_coordinate="", skill_maps=False, ensemble_size=None, ensemble_seed=0, spectra=False, ssim=False,
                 baseline=False, baseline_variable=None, baseline_mode="bicubic", distribution=False, distribution_bins=128):
        self.training_paths = list(training_paths) if training_paths else []
        self.testing_paths = list(testing_paths) if testing_paths else []
        self.output_html_folder = output_html_folder
        self.output_html_path = os.path.join(output_html_folder, "index.html") if output_html_folder else None
        self.model_path = model_path
        self.model_output_variable = model_output_variable or "model_output"
        self.database_path = database_path
        self.db = ModelDatabase(database_path) if database_path else None
        self.input_variables = list(input_variables) if input_variables is not None else []
        self.sample_count = sample_count
        self.x_coordinate = x_coordinate
        self.y_coordinate = y_coordinate
        self.time_coordinate = time_coordinate
        self.skill_maps = skill_maps
        self.spectra = spectra
        self.ssim = ssim
        (self.baseline, self.baseline_variable, self.baseline_mode) = (baseline, baseline_variable, baseline_mode)
        if baseline and baseline_mode not in baseline_scores.MODES:
            raise ValueError(f"baseline_mode must be one of {', '.join(baseline_scores.MODES)}, got {baseline_mode!r}")

        (self.distribution, self.distribution_bins) = (distribution, distribution_bins)
        if distribution and (int(distribution_bins) != distribution_bins or not 1 <= int(distribution_bins) <= 128):
            raise ValueError(f"distribution_bins must be an integer from 1 to 128, got {distribution_bins!r}")

        (self.ensemble_size, self.ensemble_seed) = (ensemble_size, int(ensemble_seed))
        if ensemble_size is not None and (int(ensemble_size) != ensemble_size or not 2 <= int(ensemble_size) <= 64):
            raise ValueError(f"ensemble_size must be an integer from 2 to 64, got {ensemble_size!r}")

        self.model = load_model(self.model_path)
        if ensemble_size is not None and type(self.model).__name__ != "VarAEModel":
            raise ValueError(f"ensemble_size needs a VarAEModel (train_cae --method var): {self.model_path} holds a "
                             f"{type(self.model).__name__}")
        print(f"Evaluating model id={self.model.get_model_id()}")
        self.model_input_variables = self.model.get_input_variable_names()
        self.output_variable = self.model.get_output_variable_name()
        for input_variable in self.input_variables:
            if input_variable not in self.model_input_variables:
                raise Exception(f"requested {input_variable} is not a model input")
        if self.baseline and not self.baseline_variable:
            self.baseline_variable = self.model_input_variables[0]
        self._device_predictions = {}
        self._page_ops = {}          # the case pages' device operands and value ranges
        self._page_range = None

    def compute_measure(self, dataset, idx, measure):
        """one case's mae or mse of channel 0 (:87-95); build_html computes all cases at once with case_measures"""
        predicted = np.asarray(dataset[self.model_output_variable][idx, 0, :, :].values, dtype=np.float64)
        actual = dataset[self.output_variable][idx, 0, :, :].values
        if measure == "mae":
            return np.mean(np.abs(predicted - actual))
        elif measure == "mse":
            return np.mean(np.power(predicted - actual, 2))
        else:
            raise ValueError("Unknown measure: " + measure)

    def run(self):
        (case_dimension, train_ds, test_ds, metrics) = self.evaluate_model_metrics()
        if self.output_html_path:
            self.build_html(case_dimension, train_ds, test_ds, metrics)

    def _open(self, paths):
        """the files of one partition concatenated along the case dimension (None when there are none)"""
        if not paths:
            return None
        first = open_mfdataset(paths[:1])
        if len(paths) == 1:
            return first
        return open_mfdataset(paths, concat_dim=first[self.output_variable].dims[0], combine="nested")

    def _dataset(self, ds):
        dsdata = DSDataset(ds, self.model.get_input_variable_names(), self.model.get_output_variable_name(),
                           normalise_in=self.model.normalise_input, normalise_out=False)
        dsdata.set_normalisation_parameters(self.model.normalisation_parameters)
        return dsdata

    def evaluate_model_metrics(self):
        train_ds = self._open(self.training_paths)
        test_ds = self._open(self.testing_paths)
        either = train_ds if train_ds is not None else test_ds
        case_dimension = either[self.output_variable].dims[0] if either is not None else None
        training_cases_count = 0 if train_ds is None else train_ds[self.output_variable].shape[0]
        testing_cases_count = 0 if test_ds is None else test_ds[self.output_variable].shape[0]
        print("Evaluating training cases: %d, test cases: %d" % (training_cases_count, testing_cases_count))

        metrics = {}
        if test_ds is not None:
            metrics["test"] = self.model.evaluate(self._dataset(test_ds))
            self.model.dump_metrics("Test Metrics", metrics["test"])
        if train_ds is not None:
            metrics["train"] = self.model.evaluate(self._dataset(train_ds))
            self.model.dump_metrics("Train Metrics", metrics["train"])
        if self.db:
            self.db.add_evaluation_result(self.model.get_model_id(), ",".join(self.training_paths),
                                          ",".join(self.testing_paths), metrics)
        return case_dimension, train_ds, test_ds, metrics

    def case_measures(self, ds, partition):
        """{"mae": (n,), "mse": (n,)} of every case of a partition; the prediction is measured on the GPU where
        build_html has just made it, else as the dataset holds it"""
        pred = self._device_predictions.get(partition)
        if pred is None:
            pred = as_numpy(ds[self.model_output_variable])
        m = case_measures(pred, as_numpy(ds[self.output_variable]))
        return {"mae": m[:, 0], "mse": m[:, 1]}

    def build_html(self, case_dimension, train_ds, test_ds, model_metrics):
        # partitions without scores are scored first (:163-168)
        for (partition, ds) in (("train", train_ds), ("test", test_ds)):
            if ds is not None and self.model_output_variable not in ds:
                print(f"Applying model to generate {partition} scores")
                self._device_predictions[partition] = self.model.apply_device(
                    ds, input_variables=self.model.get_input_variable_names(),
                    prediction_variable=self.model_output_variable)

        with open(os.path.join(self.model_path, "history.json")) as f:
            training_losses = json.loads(f.read())
        with open(os.path.join(self.model_path, "parameters.json")) as f:
            training_parameters = json.loads(f.read())

        measures = []
        ensemble = []
        ssim = []
        baseline = []
        case_links = {}
        for (partition, ds) in (("test", test_ds), ("train", train_ds)):
            if ds is None:
                continue
            values = self.case_measures(ds, partition)
            for measure in MEASURES:
                ds[measure] = _make_data_array(ds, values[measure], (case_dimension,))
            if self.ensemble_size is not None:
                ds["crps"] = _make_data_array(ds, self._verify_ensemble(partition, ds, values, ensemble), (case_dimension,))
            measures.append((partition, values))
            if self.x_coordinate and self.y_coordinate and self.time_coordinate:
                if self._case_summary(case_dimension, partition, ds, train_ds, test_ds):
                    case_links[partition] = partition + "/index.html"
            if self.ssim:       # after the case pages: their uploads are used again
                for (name, v) in self._ssim(partition, ds, values, ssim).items():
                    ds[name] = _make_data_array(ds, v, (case_dimension,))
            if self.baseline:
                for (name, v) in self._baseline(partition, ds, baseline).items():
                    ds[name] = _make_data_array(ds, v, (case_dimension,))

        maps_link = self._skill_maps(train_ds, test_ds) if self.skill_maps else None
        spectra_link = self._spectra(train_ds, test_ds) if self.spectra else None
        distribution = self._distribution(train_ds, test_ds) if self.distribution else None
        self._page_ops = {}
        page = evaluation_report(model_metrics, measures, training_parameters, training_losses, case_links, maps_link,
                                 ensemble=ensemble or None, spectra_link=spectra_link, ssim=ssim or None,
                                 **({"baseline": baseline} if baseline else {}),
                                 **({"distribution": distribution} if distribution else {}))
        os.makedirs(self.output_html_folder, exist_ok=True)
        with open(self.output_html_path, "w") as f:
            f.write(page)

    def _verify_ensemble(self, partition, ds, values, records):
        """VarAEModel.verify_ensemble on one partition: ensemble_<partition>.json in the output folder, the report's record
        appended to `records`; returns the per-case crps"""
        scores = self.model.verify_ensemble(ds, self.model.get_input_variable_names(), self.output_variable,
                                            int(self.ensemble_size), self.ensemble_seed)
        record = {k: v for (k, v) in scores.items() if k not in ("case_sums", "case_crps")}
        record["mae"] = float(np.mean(values["mae"])) if len(values["mae"]) else float("nan")
        os.makedirs(self.output_html_folder, exist_ok=True)
        with open(os.path.join(self.output_html_folder, f"ensemble_{partition}.json"), "w") as f:
            # strict JSON: what is not finite (no counted pixel) is written as null
            json.dump(ensemble_scores.json_record({**record, "case_crps": scores["case_crps"]}), f, indent=1, allow_nan=False)
        records.append((partition, {**record, "case_crps": scores["case_crps"]}))
        return scores["case_crps"]

    def _case_summary(self, case_dimension, partition, ds, train_ds, test_ds):
        """the case pages of one partition: netcdf2html's (:205-253, 285-293) where that optional package imports, else
        the package's own (utils/case_pages.py, rendered on the GPU); False when they cannot be made"""
        try:
            from netcdf2html.api.netcdf2html_converter import Netcdf2HtmlConverter
        except ImportError:
            return self._native_case_summary(case_dimension, partition, ds, train_ds, test_ds)
        try:
            layers = {}
            shared = [self.output_variable, self.model_output_variable]
            for v in self.input_variables + shared:
                group = shared if v in shared else [v]
                arrays = [np.asarray(d[name].values, dtype=np.float64) for d in (train_ds, test_ds) if d is not None
                          for name in group]
                layers[v] = {"label": v, "type": "single", "min_value": float(min(np.nanmin(a) for a in arrays)),
                             "max_value": float(max(np.nanmax(a) for a in arrays)), "cmap": "coolwarm"}
            config = {"dimensions": {"case": case_dimension},
                      "coordinates": {"x": self.x_coordinate, "y": self.y_coordinate, "time": self.time_coordinate},
                      "image": {"grid-width": 250, "max-zoom": 10}, "layers": layers}
            converter = Netcdf2HtmlConverter(config, ds, os.path.join(self.output_html_folder, partition), title=partition,
                                             sample_count=self.sample_count)
            converter.run()
            return True
        except Exception:
            print("Unable to create case summary")
            return False

    # ---- the package's own case pages ---------------------------------------------------------

    def _page_operands(self, partition, ds):
        """{variable: device operand} of what a partition's pages draw, uploaded once: the NetCDF slabs as stored, and
        the prediction where build_html has just made it"""
        ops = self._page_ops.get(partition)
        if ops is None:
            ops = {v: device_operand(as_numpy(ds[v])) for v in self.input_variables + [self.output_variable]}
            pred = self._device_predictions.get(partition)
            ops[self.model_output_variable] = device_operand(pred if pred is not None
                                                             else as_numpy(ds[self.model_output_variable]))
            self._page_ops[partition] = ops
        return ops

    def _page_ranges(self, train_ds, test_ds):
        """{layer: (lo, hi)} over both partitions (cae_case_range, channel 0, finite values): each input variable its own,
        target and prediction one shared range, the error prediction - target the symmetric +-max|d|.  A layer without
        a finite value gets (0, 0): everything that is not NaN is then drawn at the middle level."""
        if self._page_range is not None:
            return self._page_range
        parts = [self._page_operands(p, d) for (p, d) in (("train", train_ds), ("test", test_ds)) if d is not None]

        def span(pairs):
            found = [case_range(a, sub=b) for (a, b) in pairs]
            if sum(f[2] for f in found) == 0:
                return 0.0, 0.0
            return min(f[0] for f in found), max(f[1] for f in found)

        (target, pred) = (self.output_variable, self.model_output_variable)
        ranges = {v: span([(ops[v], None) for ops in parts]) for v in self.input_variables}
        ranges[target] = ranges[pred] = span([(ops[v], None) for ops in parts for v in (target, pred)])
        (lo, hi) = span([(ops[pred], ops[target]) for ops in parts])
        bound = max(abs(lo), abs(hi))
        ranges[case_pages.ERROR_LAYER] = (-bound, bound)
        self._page_range = ranges
        return ranges

    def _flip_y(self, ds, variable):
        """True when the y coordinate lies along the variable's image rows and ascends (first case / column where it has
        more dimensions): row 0 of the picture is then the largest y"""
        try:
            yc = ds[self.y_coordinate]
        except KeyError:
            return False
        ydim = ds[variable].dims[-2]
        if ydim not in yc.dims:
            return False
        along = np.asarray(yc.values)[tuple(slice(None) if d == ydim else 0 for d in yc.dims)]
        return bool(along.size > 1 and along[-1] > along[0])

    def _case_times(self, ds, case_dimension, cases):
        """(the time coordinate's value of each selected case, its units), or (None, "") when the coordinate is not
        indexed by the case dimension"""
        try:
            tc = ds[self.time_coordinate]
        except KeyError:
            return None, ""
        if tuple(tc.dims) != (case_dimension,):
            return None, ""
        return np.asarray(tc.values)[cases], str(getattr(tc, "attrs", {}).get("units", ""))

    def _native_case_summary(self, case_dimension, partition, ds, train_ds, test_ds):
        try:
            ops = self._page_operands(partition, ds)
            ranges = self._page_ranges(train_ds, test_ds)
            (target, pred) = (self.output_variable, self.model_output_variable)
            cases = case_pages.select_cases(int(ds[target].shape[0]), self.sample_count)
            flip = self._flip_y(ds, target)      # the prediction and the error are drawn the way the target is
            layers = []
            for v in self.input_variables:
                layers.append((v, *ranges[v], render_cases(ops[v], *ranges[v], cases=cases, flip_y=self._flip_y(ds, v))))
            for v in (target, pred):
                layers.append((v, *ranges[v], render_cases(ops[v], *ranges[v], cases=cases, flip_y=flip)))
            error = case_pages.ERROR_LAYER
            layers.append((error, *ranges[error],
                           render_cases(ops[pred], *ranges[error], cases=cases, sub=ops[target], flip_y=flip)))
            measures = {m: np.asarray(ds[m].values)[cases] for m in MEASURES}
            (times, units) = self._case_times(ds, case_dimension, cases)
            case_pages.write_case_pages(os.path.join(self.output_html_folder, partition), partition, cases, layers,
                                        measures, times=times, time_units=units)
            return True
        except Exception as ex:
            print("Unable to create case summary")
            print(f"\t{type(ex).__name__}: {ex}")
            return False

    # ---- per-pixel skill maps ------------------------------------------------------------------

    def _skill_shift(self):
        """the midpoint of the model's output normalisation range, or 0.0 when that is not finite: the sums' second
        moments are taken about it"""
        try:
            mid = 0.5 * (float(self.model.normalisation_parameters[2]) + float(self.model.normalisation_parameters[3]))
        except (TypeError, ValueError, IndexError):
            return 0.0
        return mid if np.isfinite(mid) else 0.0

    def _skill_coordinates(self, ds, dims):
        """{name: (dimension, values, attrs)} of the y / x coordinate variables that are 1-D along the target's image
        dimensions"""
        found = {}
        for (name, dim) in ((self.y_coordinate, dims[0]), (self.x_coordinate, dims[1])):
            if name and name in ds and tuple(ds[name].dims) == (dim,):
                found[name] = (dim, np.asarray(ds[name].values), dict(getattr(ds[name], "attrs", {})))
        return found

    def _skill_maps(self, train_ds, test_ds):
        """skill_<partition>.nc and maps/index.html; returns the page's href for the report"""
        (target, pred) = (self.output_variable, self.model_output_variable)
        shift = self._skill_shift()
        parts = []
        for (partition, ds) in (("test", test_ds), ("train", train_ds)):
            if ds is None:
                continue
            ops = self._page_ops.get(partition, {})         # what the case pages have uploaded already
            p = ops.get(pred, self._device_predictions.get(partition))
            (p, a) = (device_operand(p if p is not None else as_numpy(ds[pred])),
                      device_operand(ops.get(target, as_numpy(ds[target]))))
            sums = pixel_sums(p, a, shift)
            # the second moments once more about each pixel's own means: variances without the cancellation
            centred = pixel_sums(p, a, skill_maps.pixel_means(sums, shift))
            maps = skill_maps.maps_from_sums(sums, centred)
            dims = tuple(ds[target].dims[-2:])
            skill_maps.write_netcdf(os.path.join(self.output_html_folder, f"skill_{partition}.nc"), maps, dims,
                                    self._skill_coordinates(ds, dims))
            flip = bool(self.y_coordinate) and self._flip_y(ds, target)
            parts.append((partition, int(ds[target].shape[0]), device_operand(skill_maps.stack_maps(maps)), flip))
        if not parts:
            return None
        n_case = max(p[1] for p in parts)
        ranges = {}
        for (k, name) in enumerate(skill_maps.MAPS):
            ranges[name] = skill_maps.map_range(name, [case_range(op.tensor[k:k + 1]) for (_, _, op, _) in parts], n_case)
        pages = [(partition, n, [(name, *ranges[name], render_cases(op, *ranges[name], cases=[k], flip_y=flip)[0])
                                 for (k, name) in enumerate(skill_maps.MAPS)]) for (partition, n, op, flip) in parts]
        skill_maps.write_maps_page(os.path.join(self.output_html_folder, "maps"), pages)
        return "maps/index.html"

    # ---- power spectra ---------------------------------------------------------------------------

    def _spectra(self, train_ds, test_ds):
        """spectra_<partition>.json and spectra/index.html; returns the page's href for the report.  Every rank would
        compute all cases: the pass is not sharded."""
        (target, pred) = (self.output_variable, self.model_output_variable)
        parts = []
        for (partition, ds) in (("test", test_ds), ("train", train_ds)):
            if ds is None:
                continue
            ops = self._page_ops.get(partition, {})         # what the case pages have uploaded already
            p = ops.get(pred, self._device_predictions.get(partition))
            (p, a) = (device_operand(p if p is not None else as_numpy(ds[pred])),
                      device_operand(ops.get(target, as_numpy(ds[target]))))
            (sums, counted) = case_spectra(p, a)
            (h, w) = (int(a.shape[2]), int(a.shape[3]))
            curves = spectra_curves.curves_from_sums(sums, counted, h, w)
            os.makedirs(self.output_html_folder, exist_ok=True)
            spectra_curves.write_json(os.path.join(self.output_html_folder, f"spectra_{partition}.json"), curves, h, w)
            er = curves["effective_resolution"]
            print(f"spectra {partition}: effective_resolution {'none' if er is None else format(er, '.6g')} pixels, "
                  f"{curves['n_counted']}/{curves['n_cases']} cases")
            parts.append((partition, curves))
        if not parts:
            return None
        spectra_curves.write_page(os.path.join(self.output_html_folder, "spectra"), parts)
        return "spectra/index.html"

    # ---- value distributions ---------------------------------------------------------------------

    DISTRIBUTION_SUB = 8        # fine bins of a coarse bin: 1024 fine bins at the default 128

    def _distribution(self, train_ds, test_ds):
        """distribution_<partition>.json and distribution/index.html; returns ([(partition, curves)], the page's href) for
        the report, or None without a partition.  The range is shared by the partitions present: the minimum and the
        maximum of the finite values of target and prediction (cae_case_range), hi = lo + 1 where it is degenerate."""
        (target, pred) = (self.output_variable, self.model_output_variable)
        found = []
        for (partition, ds) in (("test", test_ds), ("train", train_ds)):
            if ds is None:
                continue
            ops = self._page_ops.get(partition, {})         # what the case pages have uploaded already
            p = ops.get(pred, self._device_predictions.get(partition))
            found.append((partition, device_operand(p if p is not None else as_numpy(ds[pred])),
                          device_operand(ops.get(target, as_numpy(ds[target])))))
        if not found:
            return None
        spans = [case_range(op) for (_, p, a) in found for op in (p, a)]
        spans = [s for s in spans if s[2] > 0]
        (lo, hi) = (min(s[0] for s in spans), max(s[1] for s in spans)) if spans else (0.0, 0.0)
        if not (np.isfinite(hi - lo) and hi > lo and np.isfinite(self.distribution_bins * self.DISTRIBUTION_SUB / (hi - lo))):
            hi = lo + 1.0
        parts = []
        os.makedirs(self.output_html_folder, exist_ok=True)
        for (partition, p, a) in found:
            counts = joint_histogram(p, a, lo, hi, n_bin=int(self.distribution_bins), sub=self.DISTRIBUTION_SUB)
            curves = distribution_curves.curves_from_counts(*counts, lo, hi, n_pixels=int(a.shape[0]) * int(a.shape[2]) * int(a.shape[3]))
            distribution_curves.write_json(os.path.join(self.output_html_folder, f"distribution_{partition}.json"), curves)
            print(distribution_curves.line(partition, curves))
            parts.append((partition, curves))
        distribution_curves.write_page(os.path.join(self.output_html_folder, "distribution"), parts)
        return parts, "distribution/index.html"

    # ---- structural similarity -------------------------------------------------------------------

    def _ssim(self, partition, ds, values, records):
        """ssim_<partition>.json in the output folder and the report's record appended to `records`; returns the per-case
        {"ssim", "ms_ssim", "psnr"} arrays.  The range of SSIM and PSNR is the model's output normalisation range."""
        (target, pred) = (self.output_variable, self.model_output_variable)
        (vmin, vmax) = (float(self.model.normalisation_parameters[2]), float(self.model.normalisation_parameters[3]))
        ops = self._page_ops.get(partition, {})         # what the case pages have uploaded already
        p = ops.get(pred, self._device_predictions.get(partition))
        (p, a) = (device_operand(p if p is not None else as_numpy(ds[pred])),
                  device_operand(ops.get(target, as_numpy(ds[target]))))
        (h, w) = (int(a.shape[2]), int(a.shape[3]))
        scores = ssim_scores.scores_from_sums(case_ssim(p, a, vmin, vmax), h, w, mse=values["mse"], vmin=vmin, vmax=vmax)
        record = ssim_scores.summary(scores, h, w, vmin, vmax)
        os.makedirs(self.output_html_folder, exist_ok=True)
        ssim_scores.write_json(os.path.join(self.output_html_folder, f"ssim_{partition}.json"), record)
        print(ssim_scores.line(partition, record))
        records.append((partition, record))
        return {k: scores[k] for k in ("ssim", "ms_ssim", "psnr")}

    # ---- skill against interpolating the input ---------------------------------------------------

    def _baseline(self, partition, ds, records):
        """baseline_<partition>.json in the output folder and the report's record appended to `records`; returns the
        per-case {"baseline_mse", "skill"} arrays"""
        (target, pred, name) = (self.output_variable, self.model_output_variable, self.baseline_variable)
        if name not in ds or len(ds[name].shape) != 4:
            raise ValueError(f"baseline variable {name!r} is not a 4-dimensional variable of the {partition} data set")
        ops = self._page_ops.get(partition, {})         # what the case pages have uploaded already
        p = ops.get(pred, self._device_predictions.get(partition))
        (low, p, a) = (device_operand(ops.get(name, as_numpy(ds[name]))),
                       device_operand(p if p is not None else as_numpy(ds[pred])),
                       device_operand(ops.get(target, as_numpy(ds[target]))))
        sums = case_baseline(low, p, a, mode=self.baseline_mode)
        record = baseline_scores.summary(sums, self.baseline_mode, name, low.shape[2:], a.shape[2:])
        os.makedirs(self.output_html_folder, exist_ok=True)
        baseline_scores.write_json(os.path.join(self.output_html_folder, f"baseline_{partition}.json"), record)
        print(baseline_scores.line(partition, record))
        records.append((partition, record))
        return {"baseline_mse": np.asarray(record["case_baseline_mse"], dtype=np.float64),
                "skill": np.asarray(record["case_skill"], dtype=np.float64)}
