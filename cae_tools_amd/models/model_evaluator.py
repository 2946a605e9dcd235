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

The optional analyses that are no reference feature - ensemble verification, structural similarity, skill against
interpolation, per-pixel skill maps, power spectra, value distributions, skill by stratum, neighbourhood skill, input importance, novelty of the cases and the comparison of models - are the units of
evaluation_analyses.py, which build_html runs in their fixed order.  What they and the case pages read on the GPU comes
from one operand cache (operand): a partition's variable is uploaded once per build_html, whatever is switched on.
"""
import json
import os

import numpy as np

from ..data.arrays import as_numpy, open_mfdataset
from ..case_ops import case_measures, case_range, device_operand, render_cases
from ..utils import case_pages
from ..utils.model_database import ModelDatabase
from ..utils.report import evaluation_report
from .base_model import _make_data_array
from . import evaluation_analyses as analyses
from .ds_dataset import DSDataset  # noqa: F401  (this module's public name since before EngineModel built the data sets)
from .model_loader import load_model

MEASURES = ("mae", "mse")


class ModelEvaluator:

    def __init__(self, training_paths, testing_paths, output_html_folder="", model_output_variable="", model_path="",
                 database_path="", input_variables=[], sample_count=None, x_coordinate="", y_coordinate="",
                 time_coordinate="", skill_maps=False, ensemble_size=None, ensemble_seed=0, spectra=False, ssim=False,
                 baseline=False, baseline_variable=None, baseline_mode="bicubic", distribution=False, distribution_bins=128,
                 strata=False, strata_variable=None, strata_channel=0, strata_edges=None, strata_classes=None, strata_count=8,
                 fss=False, fss_thresholds=None, fss_percentiles=None, fss_widths=None, fss_gaps="strict",
                 importance=False, importance_repeats=5, importance_seed=0, importance_groups=None, importance_maps=False,
                 novelty=False, novelty_k=5, novelty_reference=None, compare=False, compare_variables=None, compare_labels=None,
                 compare_resamples=10000, compare_seed=0, compare_confidence="0.95", compare_block_variable=None,
                 compare_baseline=None):
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
        (self.distribution, self.distribution_bins) = (distribution, distribution_bins)
        (self.ensemble_size, self.ensemble_seed) = (ensemble_size, int(ensemble_seed))
        (self.strata, self.strata_variable, self.strata_channel) = (strata, strata_variable, strata_channel)
        (self.strata_edges, self.strata_classes, self.strata_count) = (strata_edges, strata_classes, strata_count)
        (self.fss, self.fss_thresholds, self.fss_percentiles) = (fss, fss_thresholds, fss_percentiles)
        (self.fss_widths, self.fss_gaps) = (fss_widths, fss_gaps)
        (self.importance, self.importance_repeats, self.importance_seed) = (importance, importance_repeats, importance_seed)
        (self.importance_groups, self.importance_maps) = (importance_groups, importance_maps)
        (self.novelty, self.novelty_k) = (novelty, novelty_k)
        self.novelty_reference = list(novelty_reference) if novelty_reference else None
        (self.compare, self.compare_variables) = (compare, list(compare_variables) if compare_variables else [])
        self.compare_labels = list(compare_labels) if compare_labels else None
        (self.compare_resamples, self.compare_seed, self.compare_confidence) = (compare_resamples, compare_seed, compare_confidence)
        (self.compare_block_variable, self.compare_baseline) = (compare_block_variable, compare_baseline)
        for unit in (analyses.BASELINE, analyses.DISTRIBUTION, analyses.ENSEMBLE,       # the refusals come in this order,
                     analyses.STRATA, analyses.FSS, analyses.IMPORTANCE,                # all before the model is loaded
                     analyses.NOVELTY, analyses.COMPARE):
            unit.check(self)
        self.model = load_model(self.model_path)
        analyses.check_ensemble_model(self)
        print(f"Evaluating model id={self.model.get_model_id()}")
        self.model_input_variables = self.model.get_input_variable_names()
        self.output_variable = self.model.get_output_variable_name()
        for input_variable in self.input_variables:
            if input_variable not in self.model_input_variables:
                raise Exception(f"requested {input_variable} is not a model input")
        if self.baseline and not self.baseline_variable:
            self.baseline_variable = self.model_input_variables[0]
        analyses.check_importance_model(self)
        analyses.check_compare_model(self)
        self._device_predictions = {}
        self._run = None             # inside build_html: (case dimension, [(partition, data set)] in page order)
        self._operands = None        # inside build_html: {(partition, variable): device operand}
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
        return self.model._model_dataset(ds, self.model.get_input_variable_names(), self.model.get_output_variable_name(),
                                         normalise_in=self.model.normalise_input, normalise_out=False)

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

    def operand(self, partition, ds, variable):
        """The device operand of one variable of a partition: the NetCDF slab as stored, or the prediction where build_html
        has just made it on the GPU.  The one place where the evaluator uploads an array of a data set: inside build_html
        the operand is kept, so the measures, the case pages and every analysis share one upload, and all are dropped
        before the report is written - what a run with case pages holds on the device, no more.  Outside build_html
        nothing is kept."""
        op = (self._operands or {}).get((partition, variable))
        if op is None:
            pred = self._device_predictions.get(partition) if variable == self.model_output_variable else None
            op = device_operand(pred if pred is not None else as_numpy(ds[variable]))
            if self._operands is not None:
                self._operands[(partition, variable)] = op
        return op

    def operands(self, partition, ds):
        """(prediction, target) of a partition as device operands"""
        return self.operand(partition, ds, self.model_output_variable), self.operand(partition, ds, self.output_variable)

    def case_measures(self, ds, partition):
        """{"mae": (n,), "mse": (n,)} of every case of a partition; the prediction is measured on the GPU where
        build_html has just made it, else as the dataset holds it"""
        m = case_measures(*self.operands(partition, ds))
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

        parts = [(partition, ds) for (partition, ds) in (("test", test_ds), ("train", train_ds)) if ds is not None]
        units = [unit for unit in analyses.ANALYSES if unit.enabled(self)]
        measures = []
        report = {}         # evaluation_report's keywords, filled by the analyses

        def add(ds, variables):
            for (name, v) in variables.items():
                ds[name] = _make_data_array(ds, v, (case_dimension,))

        (self._run, self._operands) = ((case_dimension, parts), {})
        try:
            for (partition, ds) in parts:
                values = self.case_measures(ds, partition)
                measures.append((partition, values))
                add(ds, values)
                for unit in units:
                    if unit.partition:
                        add(ds, unit.partition(self, partition, ds, values, report))
            for unit in units:
                if unit.after and parts:
                    unit.after(self, parts, report)
        finally:
            (self._run, self._operands) = (None, None)
        page = evaluation_report(model_metrics, measures, training_parameters, training_losses, **report)
        os.makedirs(self.output_html_folder, exist_ok=True)
        with open(self.output_html_path, "w") as f:
            f.write(page)

    def case_summary(self, partition, ds):
        """the case pages of one partition: netcdf2html's (:205-253, 285-293) where that optional package imports, else
        the package's own (utils/case_pages.py, rendered on the GPU); False when they cannot be made"""
        try:
            from netcdf2html.api.netcdf2html_converter import Netcdf2HtmlConverter
        except ImportError:
            return self._native_case_summary(partition, ds)
        try:
            (case_dimension, parts) = self._run
            layers = {}
            shared = [self.output_variable, self.model_output_variable]
            for v in self.input_variables + shared:
                group = shared if v in shared else [v]
                arrays = [np.asarray(d[name].values, dtype=np.float64) for (_, d) in parts for name in group]
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

    def _page_ranges(self):
        """{layer: (lo, hi)} over both partitions (cae_case_range, channel 0, finite values): each input variable its own,
        target and prediction one shared range, the error prediction - target the symmetric +-max|d|.  A layer without
        a finite value gets (0, 0): everything that is not NaN is then drawn at the middle level."""
        if self._page_range is not None:
            return self._page_range
        parts = self._run[1][::-1]          # train before test

        def span(variables, sub=None):
            found = [case_range(self.operand(p, d, v), sub=self.operand(p, d, sub) if sub else None)
                     for (p, d) in parts for v in variables]
            if sum(f[2] for f in found) == 0:
                return 0.0, 0.0
            return min(f[0] for f in found), max(f[1] for f in found)

        (target, pred) = (self.output_variable, self.model_output_variable)
        ranges = {v: span([v]) for v in self.input_variables}
        ranges[target] = ranges[pred] = span([target, pred])
        (lo, hi) = span([pred], sub=target)
        bound = max(abs(lo), abs(hi))
        ranges[case_pages.ERROR_LAYER] = (-bound, bound)
        self._page_range = ranges
        return ranges

    def flip_y(self, ds, variable):
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

    def _native_case_summary(self, partition, ds):
        try:
            ranges = self._page_ranges()
            (target, pred) = (self.output_variable, self.model_output_variable)
            cases = case_pages.select_cases(int(ds[target].shape[0]), self.sample_count)
            flip = self.flip_y(ds, target)      # the prediction and the error are drawn the way the target is

            def layer(v, name=None, sub=None, flip_y=flip):
                name = name or v
                return (name, *ranges[name], render_cases(self.operand(partition, ds, v), *ranges[name], cases=cases,
                                                          sub=self.operand(partition, ds, sub) if sub else None, flip_y=flip_y))

            layers = [layer(v, flip_y=self.flip_y(ds, v)) for v in self.input_variables] + [layer(target), layer(pred)]
            layers.append(layer(pred, case_pages.ERROR_LAYER, sub=target))
            measures = {m: np.asarray(ds[m].values)[cases] for m in MEASURES}
            (times, units) = self._case_times(ds, self._run[0], cases)
            case_pages.write_case_pages(os.path.join(self.output_html_folder, partition), partition, cases, layers,
                                        measures, times=times, time_units=units)
            return True
        except Exception as ex:
            print("Unable to create case summary")
            print(f"\t{type(ex).__name__}: {ex}")
            return False
