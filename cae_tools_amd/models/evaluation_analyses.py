"""The optional outputs of ModelEvaluator.build_html, none of them a reference feature: ensemble verification, case pages,
structural similarity, skill against interpolation, per-pixel skill maps, power spectra, value distributions, skill by
stratum, neighbourhood skill, input importance, novelty of the cases and the comparison of models.

Each is one Analysis of functions over the evaluator `ev`:
    enabled(ev)                                     whether its option is on
    check(ev)                                       raises the option's refusal; called from the evaluator's constructor
    partition(ev, partition, ds, values, report)    inside build_html's loop over the partitions, after the per-case measures
                                                    `values`: returns {variable: per-case array} to add to the data set
    after(ev, parts, report)                        once after that loop; parts = [(partition, ds)] in page order
Both put what utils/report.evaluation_report shows of the analysis into `report` under that function's keyword.  The operands
come from the evaluator's cache (ev.operand, ev.operands), so a partition's target, prediction and input go to the GPU once
whatever is switched on.  ANALYSES holds them in the order build_html runs them.
"""
import os
from collections import namedtuple

import numpy as np

from ..case_ops import (bootstrap_table, case_baseline, case_compare, case_range, case_spectra, case_ssim, device_operand, fraction_skill,
                        joint_histogram, pixel_sums, render_cases, strata_sums)
from ..data.arrays import as_numpy, open_mfdataset
from ..utils import baseline as baseline_scores
from ..utils import compare as compare_scores
from ..utils import distribution as distribution_curves
from ..utils import ensemble_scores, skill_maps
from ..utils import fss as fss_scores
from ..utils import importance as importance_scores
from ..utils import novelty as novelty_scores
from ..utils import spectra as spectra_curves
from ..utils import ssim as ssim_scores
from ..utils import strata as strata_scores

Analysis = namedtuple("Analysis", "enabled check partition after", defaults=(None, None, None))


def _keep(ev, module, kind, partition, record, records, *extra):
    """the common end of an analysis of one partition: <kind>_<partition>.json in the output folder by the module's
    write_json, its line printed where it has one, and the record kept for the report"""
    os.makedirs(ev.output_html_folder, exist_ok=True)
    module.write_json(os.path.join(ev.output_html_folder, f"{kind}_{partition}.json"), record, *extra)
    if hasattr(module, "line"):
        print(module.line(partition, record))
    records.append((partition, record))


# ---- ensemble verification -------------------------------------------------------------------

def check_ensemble(ev):
    if ev.ensemble_size is not None and (int(ev.ensemble_size) != ev.ensemble_size or not 2 <= int(ev.ensemble_size) <= 64):
        raise ValueError(f"ensemble_size must be an integer from 2 to 64, got {ev.ensemble_size!r}")


def check_ensemble_model(ev):
    if ev.ensemble_size is not None and type(ev.model).__name__ != "VarAEModel":
        raise ValueError(f"ensemble_size needs a VarAEModel (train_cae --method var): {ev.model_path} holds a "
                         f"{type(ev.model).__name__}")


def _ensemble(ev, partition, ds, values, report):
    """ensemble_size=K (cli/verify_ensemble.py; a VarAEModel only) verifies the model's K-member ensemble against the target
    per partition (VarAEModel.verify_ensemble, cae_ensemble_verify on the GPU): ensemble_<partition>.json with the scores,
    rank counts, K and seed (strict JSON: a score that is not finite is null), a per-case crps variable beside mae / mse in
    the data set, and the report's "Ensemble verification" section."""
    scores = ev.model.verify_ensemble(ds, ev.model.get_input_variable_names(), ev.output_variable, int(ev.ensemble_size),
                                      ev.ensemble_seed)
    record = {k: v for (k, v) in scores.items() if k not in ("case_sums", "case_crps")}
    record["mae"] = float(np.mean(values["mae"])) if len(values["mae"]) else float("nan")
    _keep(ev, ensemble_scores, "ensemble", partition, {**record, "case_crps": scores["case_crps"]},
          report.setdefault("ensemble", []))
    return {"crps": scores["case_crps"]}


# ---- case pages ------------------------------------------------------------------------------

def _case_pages(ev, partition, ds, values, report):
    """the case pages (--x-coordinate, --y-coordinate and --time-coordinate all given): ModelEvaluator.case_summary"""
    if ev.case_summary(partition, ds):
        report.setdefault("case_links", {})[partition] = partition + "/index.html"
    return {}


# ---- structural similarity -------------------------------------------------------------------

def _ssim(ev, partition, ds, values, report):
    """ssim=True (cli/ssim.py) adds the structural scores: per partition and case the SSIM, the MS-SSIM (five scales, where
    min(h, w) > 160) and the PSNR of channel 0 against the model's output normalisation range, from one cae_case_ssim pass on
    the GPU (fp64, the VAE loss's definition with a rule for missing data; utils/ssim.py) and the mse
    already measured: ssim_<partition>.json, per-case ssim / ms_ssim / psnr variables beside mae / mse in the data set, and
    the report's "Structural similarity" section."""
    (vmin, vmax) = (float(ev.model.normalisation_parameters[2]), float(ev.model.normalisation_parameters[3]))
    (p, a) = ev.operands(partition, ds)
    (h, w) = (int(a.shape[2]), int(a.shape[3]))
    scores = ssim_scores.scores_from_sums(case_ssim(p, a, vmin, vmax), h, w, mse=values["mse"], vmin=vmin, vmax=vmax)
    _keep(ev, ssim_scores, "ssim", partition, ssim_scores.summary(scores, h, w, vmin, vmax), report.setdefault("ssim", []))
    return {k: scores[k] for k in ("ssim", "ms_ssim", "psnr")}


# ---- skill against interpolating the input ---------------------------------------------------

def check_baseline(ev):
    if ev.baseline and ev.baseline_mode not in baseline_scores.MODES:
        raise ValueError(f"baseline_mode must be one of {', '.join(baseline_scores.MODES)}, got {ev.baseline_mode!r}")


def _baseline(ev, partition, ds, values, report):
    """baseline=True (cli/baseline.py) answers whether the model is better than interpolating its own input: channel 0 of
    baseline_variable (default: the model's first input variable) is interpolated to the target's grid (baseline_mode
    "nearest", "bilinear" or "bicubic", torch's align_corners=False formulas) inside the kernel that compares it, one
    cae_case_baseline pass on the GPU (fp64; utils/baseline.py): baseline_<partition>.json with the
    pooled and per-case skill 1 - model_mse / baseline_mse, per-case baseline_mse / skill variables beside mae / mse in the
    data set, and the report's "Skill against interpolation" section."""
    name = ev.baseline_variable
    if name not in ds or len(ds[name].shape) != 4:
        raise ValueError(f"baseline variable {name!r} is not a 4-dimensional variable of the {partition} data set")
    (low, (p, a)) = (ev.operand(partition, ds, name), ev.operands(partition, ds))
    record = baseline_scores.summary(case_baseline(low, p, a, mode=ev.baseline_mode), ev.baseline_mode, name, low.shape[2:],
                                     a.shape[2:])
    _keep(ev, baseline_scores, "baseline", partition, record, report.setdefault("baseline", []))
    return {"baseline_mse": np.asarray(record["case_baseline_mse"], dtype=np.float64),
            "skill": np.asarray(record["case_skill"], dtype=np.float64)}


# ---- per-pixel skill maps --------------------------------------------------------------------

def _skill_shift(ev):
    """the midpoint of the model's output normalisation range, or 0.0 when that is not finite: the sums' second
    moments are taken about it"""
    try:
        mid = 0.5 * (float(ev.model.normalisation_parameters[2]) + float(ev.model.normalisation_parameters[3]))
    except (TypeError, ValueError, IndexError):
        return 0.0
    return mid if np.isfinite(mid) else 0.0


def _skill_coordinates(ev, ds, dims):
    """{name: (dimension, values, attrs)} of the y / x coordinate variables that are 1-D along the target's image
    dimensions"""
    found = {}
    for (name, dim) in ((ev.y_coordinate, dims[0]), (ev.x_coordinate, dims[1])):
        if name and name in ds and tuple(ds[name].dims) == (dim,):
            found[name] = (dim, np.asarray(ds[name].values), dict(getattr(ds[name], "attrs", {})))
    return found


def _skill_maps(ev, parts, report):
    """skill_maps=True (cli/skill_maps.py) adds the transposed reduction: per partition the per-pixel count, bias, mae, rmse,
    correlation and sd_ratio of channel 0 over the cases, from two streaming passes over the operands on the GPU
    (cae_pixel_sums about the midpoint of the output normalisation range, then cae_pixel_sums_about each pixel's means for
    the variances; utils/skill_maps.py), written as skill_<partition>.nc beside index.html and drawn on maps/index.html,
    which the report then links.  The six maps of a partition go to the GPU as six one-channel cases and are ranged and
    drawn by the case pages' kernels; ranges go over both partitions (count over [0, largest number of cases], bias over
    +-max|bias|)."""
    target = ev.output_variable
    shift = _skill_shift(ev)
    drawn = []
    for (partition, ds) in parts:
        (p, a) = ev.operands(partition, ds)
        sums = pixel_sums(p, a, shift)
        # the second moments once more about each pixel's own means: variances without the cancellation
        centred = pixel_sums(p, a, skill_maps.pixel_means(sums, shift))
        maps = skill_maps.maps_from_sums(sums, centred)
        dims = tuple(ds[target].dims[-2:])
        skill_maps.write_netcdf(os.path.join(ev.output_html_folder, f"skill_{partition}.nc"), maps, dims,
                                _skill_coordinates(ev, ds, dims))
        flip = bool(ev.y_coordinate) and ev.flip_y(ds, target)
        drawn.append((partition, int(ds[target].shape[0]), device_operand(skill_maps.stack_maps(maps)), flip))
    n_case = max(d[1] for d in drawn)
    ranges = {}
    for (k, name) in enumerate(skill_maps.MAPS):
        ranges[name] = skill_maps.map_range(name, [case_range(op.tensor[k:k + 1]) for (_, _, op, _) in drawn], n_case)
    pages = [(partition, n, [(name, *ranges[name], render_cases(op, *ranges[name], cases=[k], flip_y=flip)[0])
                             for (k, name) in enumerate(skill_maps.MAPS)]) for (partition, n, op, flip) in drawn]
    skill_maps.write_maps_page(os.path.join(ev.output_html_folder, "maps"), pages)
    report["maps_link"] = "maps/index.html"


# ---- power spectra ---------------------------------------------------------------------------

def _spectra(ev, parts, report):
    """spectra=True (cli/spectra.py) adds the reduction along scale: per partition the radially binned power spectra of
    prediction and target, their ratio, the spectral coherence and the error spectrum of channel 0 from one cae_case_spectra
    pass on the GPU (a direct fp64 DFT of every case; utils/spectra.py), written as
    spectra_<partition>.json and drawn on spectra/index.html, which the report then links.  Every rank would compute all
    cases: the pass is not sharded."""
    found = []
    for (partition, ds) in parts:
        (p, a) = ev.operands(partition, ds)
        (h, w) = (int(a.shape[2]), int(a.shape[3]))
        _keep(ev, spectra_curves, "spectra", partition, spectra_curves.curves_from_sums(*case_spectra(p, a), h, w), found, h, w)
    spectra_curves.write_page(os.path.join(ev.output_html_folder, "spectra"), found)
    report["spectra_link"] = "spectra/index.html"


# ---- value distributions ---------------------------------------------------------------------

DISTRIBUTION_SUB = 8        # fine bins of a coarse bin: 1024 fine bins at the default 128


def check_distribution(ev):
    if ev.distribution and (int(ev.distribution_bins) != ev.distribution_bins or not 1 <= int(ev.distribution_bins) <= 128):
        raise ValueError(f"distribution_bins must be an integer from 1 to 128, got {ev.distribution_bins!r}")


def _value_span(operands, n_bin):
    """(lo, hi) of a joint_histogram pass of n_bin coarse bins: the range of the finite values of the operands, one
    cae_case_range each in their order; hi = lo + 1 where that range is degenerate"""
    spans = [case_range(op) for op in operands]
    spans = [s for s in spans if s[2] > 0]
    (lo, hi) = (min(s[0] for s in spans), max(s[1] for s in spans)) if spans else (0.0, 0.0)
    if not (np.isfinite(hi - lo) and hi > lo and np.isfinite(n_bin * DISTRIBUTION_SUB / (hi - lo))):
        hi = lo + 1.0
    return lo, hi


def _distribution(ev, parts, report):
    """distribution=True (cli/distribution.py) adds the reduction along value: per partition the joint histogram of
    prediction against target over distribution_bins (1 to 128) coarse bins, the two fine marginal histograms and the
    per-bin error sums of channel 0 from one cae_joint_hist pass on the GPU (utils/distribution.py) over
    the range of the finite values of target and prediction in the partitions present (cae_case_range; hi = lo + 1 where that
    range is degenerate): distribution_<partition>.json with the conditional bias, reliability, quantiles, Wasserstein-1
    distance, Perkins score and exceedance scores, distribution/index.html with the joint density and the curves, and the
    report's "Value distribution" section."""
    pairs = [(partition, *ev.operands(partition, ds)) for (partition, ds) in parts]
    (lo, hi) = _value_span([op for (_, p, a) in pairs for op in (p, a)], ev.distribution_bins)
    found = []
    for (partition, p, a) in pairs:
        counts = joint_histogram(p, a, lo, hi, n_bin=int(ev.distribution_bins), sub=DISTRIBUTION_SUB)
        curves = distribution_curves.curves_from_counts(*counts, lo, hi, n_pixels=int(a.shape[0]) * int(a.shape[2]) * int(a.shape[3]))
        _keep(ev, distribution_curves, "distribution", partition, curves, found)
    distribution_curves.write_page(os.path.join(ev.output_html_folder, "distribution"), found)
    report["distribution"] = (found, "distribution/index.html")


# ---- skill by stratum ------------------------------------------------------------------------

def check_strata(ev):
    if not ev.strata:
        return
    if not ev.strata_variable:
        raise ValueError("strata needs strata_variable, the name of the stratifier in the data set")
    if ev.strata_edges is not None and ev.strata_classes is not None:
        raise ValueError("strata_edges and strata_classes exclude each other")
    if ev.strata_edges is not None:
        strata_scores.check_edges(ev.strata_edges)
    elif ev.strata_classes is not None:
        if len(strata_scores.edges_from_classes(ev.strata_classes)[1]) > strata_scores.MAX_STRATA:
            raise ValueError(f"at most {strata_scores.MAX_STRATA} strata expected, got {len(set(map(float, ev.strata_classes)))}")
    elif int(ev.strata_count) != ev.strata_count or not 1 <= int(ev.strata_count) <= strata_scores.MAX_STRATA:
        raise ValueError(f"strata_count must be an integer from 1 to {strata_scores.MAX_STRATA}, got {ev.strata_count!r}")


def _strata_plane(op, ds, name, channel):
    """what case_range, which reads channel 0 of (N, C, H, W), is given for the stratifier: the operand itself for channel 0
    of a 4-D variable; else the one plane (a slice of the variable), or the values of a 1-D variable as (N, 1, 1, 1)"""
    if len(op.shape) == 4 and channel == 0:
        return op
    values = as_numpy(ds[name])
    return values.reshape(-1, 1, 1, 1) if values.ndim == 1 else values[:, channel:channel + 1]


def _strata(ev, parts, report):
    """strata=True (cli/strata.py) conditions the error on a variable that is neither target nor prediction: channel
    strata_channel of strata_variable - 4-D with the case dimension first, on the target's grid or a coarser or finer one
    over the same extent, or 1-D along the case dimension - cuts the pixels into strata by strata_edges, by strata_classes
    (an edge midway between neighbouring classes) or into strata_count equal bins over the range of the stratifier's finite
    values in the partitions present (cae_case_range).  Per partition two cae_strata_sums passes on the GPU (about the
    midpoint of the output normalisation range, then about each stratum's own means for the variances; utils/strata.py,
    DESIGN.md section 9): strata_<partition>.json with pixels, pairs, share, bias, mae, rmse, correlation, sd_ratio and the
    share of the squared error per stratum and pooled, and the report's "Skill by stratum" section.  Every rank would
    compute all cases: the pass is not sharded."""
    (name, channel) = (ev.strata_variable, int(ev.strata_channel))
    found = []
    for (partition, ds) in parts:
        if name not in ds or len(ds[name].shape) not in (1, 4) or ds[name].shape[0] != ds[ev.output_variable].shape[0]:
            raise ValueError(f"strata variable {name!r} is not a variable of the {partition} data set with the case dimension "
                             "first and 4 dimensions, or 1 along the cases")
        if len(ds[name].shape) == 4 and not 0 <= channel < ds[name].shape[1]:
            raise ValueError(f"strata_channel {channel} is not a channel of {name!r}, which has {ds[name].shape[1]}")
        found.append((partition, ds, ev.operand(partition, ds, name), *ev.operands(partition, ds)))
    names = None
    if ev.strata_edges is not None:
        edges = strata_scores.check_edges(ev.strata_edges)
    elif ev.strata_classes is not None:
        (edges, names) = strata_scores.edges_from_classes(ev.strata_classes)
    else:
        spans = [case_range(_strata_plane(s, ds, name, channel)) for (_, ds, s, _, _) in found]
        spans = [sp for sp in spans if sp[2] > 0]
        (lo, hi) = (min(sp[0] for sp in spans), max(sp[1] for sp in spans)) if spans else (0.0, 0.0)
        edges = strata_scores.edges_from_count(lo, hi, int(ev.strata_count))
    shift = _skill_shift(ev)
    kept = []
    for (partition, _, s, p, a) in found:
        (counts, sums) = strata_sums(p, a, s, edges, shift, channel=channel)
        # the second moments once more about each stratum's own means: variances without the cancellation
        means = strata_scores.stratum_means(counts, sums, shift)
        centred = strata_sums(p, a, s, edges, means, channel=channel)[1]
        scores = strata_scores.scores_from_sums(counts, sums, centred, shift=shift, centred_shift=means)
        in_shape = s.shape[2:] if len(s.shape) == 4 else (1, 1)
        _keep(ev, strata_scores, "strata", partition,
              strata_scores.summary(scores, name, channel, edges, names, in_shape, a.shape[2:]), kept)
    report["strata"] = kept


# ---- neighbourhood skill ---------------------------------------------------------------------

FSS_BINS = 128              # coarse bins of the joint_histogram pass that turns percentiles into values: distribution's default


def _fss_percentiles(ev):
    """[(q, side)] of the percentile form: fss_percentiles as given, numbers ("above") or (q, side) pairs of percent values,
    else utils/distribution.THRESHOLDS; q as a fraction"""
    if ev.fss_percentiles is None:
        return list(distribution_curves.THRESHOLDS)
    (values, sides) = fss_scores.check_thresholds(ev.fss_percentiles)
    if any(not 0.0 < v < 100.0 for v in values):
        raise ValueError(f"fss_percentiles must lie between 0 and 100, got {values}")
    return [(v / 100.0, "below" if s else "above") for (v, s) in zip(values, sides)]


def check_fss(ev):
    if not ev.fss:
        return
    if ev.fss_thresholds is not None and ev.fss_percentiles is not None:
        raise ValueError("fss_thresholds and fss_percentiles exclude each other")
    if ev.fss_thresholds is not None:
        fss_scores.check_thresholds(ev.fss_thresholds)
    else:
        _fss_percentiles(ev)
    if ev.fss_widths is not None:
        fss_scores.check_widths(ev.fss_widths)
    if ev.fss_gaps not in fss_scores.GAPS:
        raise ValueError(f"fss_gaps must be one of {', '.join(fss_scores.GAPS)}, got {ev.fss_gaps!r}")


def _fss(ev, parts, report):
    """fss=True (cli/fss.py) adds the reduction along displacement: per partition the Fractions Skill Score of channel 0 for
    up to 8 event thresholds over up to 8 neighbourhood widths (fss_widths, default 1, 3, 5, 9, 17, 33, 65 as far as the plane
    allows), from one cae_case_fss pass on the GPU (exact integer window sums; utils/fss.py).  The
    thresholds are fss_thresholds in data units, numbers ("above": v >= t) or (value, "above" | "below") pairs, or else the
    fss_percentiles (percent values likewise; default the 5th below and the 90th, 95th and 99th above) of the target's
    distribution in the partition: utils/distribution.quantile_from_counts on the target's fine marginal of one
    joint_histogram pass of 128 x 8 bins over the range rule of the distribution analysis, so that a percentile threshold is
    the quantile_target of distribution_<partition>.json.  fss_gaps "strict" leaves out a window over a value that is not
    finite, "ignore" only a window without any pair.  fss_<partition>.json holds the threshold values used, the pooled sums,
    the pooled and per-case FSS, the event frequencies, the uniform level and the skilful width; fss/index.html the curves;
    the report gets the "Neighbourhood skill" section.  Every rank would compute all cases: the pass is not sharded."""
    pairs = [(partition, *ev.operands(partition, ds)) for (partition, ds) in parts]
    quantiles = None
    if ev.fss_thresholds is None:
        quantiles = _fss_percentiles(ev)
        (lo, hi) = _value_span([op for (_, p, a) in pairs for op in (p, a)], FSS_BINS)
    found = []
    for (partition, p, a) in pairs:
        (h, w) = (int(a.shape[2]), int(a.shape[3]))
        if quantiles is None:
            (thresholds, percentiles) = (list(ev.fss_thresholds), None)
        else:
            marg = joint_histogram(p, a, lo, hi, n_bin=FSS_BINS, sub=DISTRIBUTION_SUB)[1]
            values = [distribution_curves.quantile_from_counts(marg[0], lo, hi, q) for (q, _) in quantiles]
            if not all(np.isfinite(values)):
                raise ValueError(f"fss: the {partition} partition has no pixel where target and prediction are finite, so no "
                                 "percentile of the target")
            (thresholds, percentiles) = ([(v, side) for (v, (_, side)) in zip(values, quantiles)], [q for (q, _) in quantiles])
        widths = fss_scores.default_widths(h, w) if ev.fss_widths is None else fss_scores.check_widths(ev.fss_widths)
        sums = fraction_skill(p, a, thresholds, widths=widths, gaps=ev.fss_gaps)
        record = fss_scores.summary(fss_scores.scores_from_sums(sums, widths), thresholds, widths, ev.fss_gaps, h, w, percentiles)
        _keep(ev, fss_scores, "fss", partition, record, found)
    fss_scores.write_page(os.path.join(ev.output_html_folder, "fss"), found)
    report["fss"] = (found, "fss/index.html")


# ---- input importance ------------------------------------------------------------------------

def check_importance(ev):
    if not ev.importance:
        return
    importance_scores.check_repeats(ev.importance_repeats)
    if int(ev.importance_seed) != ev.importance_seed or int(ev.importance_seed) < 0:
        raise ValueError(f"importance_seed must be an integer, 0 or more, got {ev.importance_seed!r}")
    importance_scores.check_groups(ev.importance_groups)


def check_importance_model(ev):
    """what check_importance cannot see before the model is loaded: the groups name input variables of the model, and every
    partition holds those variables and at least 2 cases"""
    if not ev.importance:
        return
    names = list(ev.model_input_variables)
    importance_scores.check_groups(ev.importance_groups, names)
    for (partition, paths) in (("test", ev.testing_paths), ("train", ev.training_paths)):
        ds = ev._open(paths)
        if ds is None:
            continue
        missing = [name for name in names if name not in ds]
        if missing:
            raise ValueError(f"importance needs the model's input variables in the {partition} data set: {', '.join(missing)} "
                             f"of {ev.model_path} {'is' if len(missing) == 1 else 'are'} not there")
        n = int(ds[names[0]].shape[0])
        if n < 2:
            raise ValueError(f"importance needs at least 2 cases to permute, the {partition} data set has {n}")


def _importance(ev, parts, report):
    """importance=True (cli/importance.py) asks which of its inputs the model uses: permutation importance.  Per partition
    every case is given another case's values for one group of input variables (importance_groups; default every variable
    on its own) by importance_repeats single-cycle permutations drawn from importance_seed, the batch is scored again
    through the model and the growth of the error against the target is reduced on the GPU (BaseModel.importance:
    cae_normalise_pack_gather and cae_case_importance; utils/importance.py): importance_<partition>.json
    with, per group, the pooled mse and mae with and without the permutation per repeat, importance = their difference with
    its standard deviation over the repeats, the ratio, the sensitivity of the prediction, the shares of cases and pixels
    whose error grew, the rank and the per-case change of the mse; the report's "Input importance" section; and with
    importance_maps importance/index.html, one map of the change of the mse per pixel and group, drawn the way the skill maps
    are over one symmetric range."""
    found = []
    drawn = []
    for (partition, ds) in parts:
        record = ev.model.importance(ds, ev.model_input_variables, ev.output_variable, groups=ev.importance_groups,
                                     repeats=int(ev.importance_repeats), seed=int(ev.importance_seed), maps=bool(ev.importance_maps))
        _keep(ev, importance_scores, "importance", partition, record, found)
        if ev.importance_maps:
            flip = bool(ev.y_coordinate) and ev.flip_y(ds, ev.output_variable)
            drawn.append((partition, record, device_operand(importance_scores.delta_maps(record)[:, None]), flip))
    link = None
    if drawn:
        spans = [s for s in (case_range(op) for (_, _, op, _) in drawn) if s[2] > 0]
        bound = max((max(abs(s[0]), abs(s[1])) for s in spans), default=0.0)
        pages = [(partition, record, -bound, bound,
                  [(g["name"], render_cases(op, -bound, bound, cases=[k], flip_y=flip)[0]) for (k, g) in enumerate(record["groups"])])
                 for (partition, record, op, flip) in drawn]
        importance_scores.write_maps_page(os.path.join(ev.output_html_folder, "importance"), pages)
        link = "importance/index.html"
    report["importance"] = (found, link)


# ---- novelty of the cases --------------------------------------------------------------------

def check_novelty(ev):
    if not ev.novelty:
        return
    novelty_scores.check_k(ev.novelty_k)
    if not ev.novelty_reference and not ev.training_paths:
        raise ValueError("novelty needs a reference set: the training files, or novelty_reference, the files of the reference set")


def _novelty_reference(ev):
    """(the reference data set, the record of that set searched against itself, leave-one-out): the train partition, or the
    files of novelty_reference.  Computed once per build_html and kept beside the operands, which are dropped with them."""
    key = ("novelty", "reference")
    found = ev._operands.get(key)
    if found is None:
        ds = ev._open(list(ev.novelty_reference)) if ev.novelty_reference else dict(ev._run[1])["train"]
        found = (ds, ev.model.novelty(ds, None, ev.model_input_variables, k=int(ev.novelty_k), same=True))
        ev._operands[key] = found
    return found


def _novelty(ev, partition, ds, values, report):
    """novelty=True (cli/novelty.py) asks whether a case is anything like what the model was trained on: every case of the
    partition, packed and normalised as the model sees it, gets its novelty_k nearest cases of the reference set - the train
    partition, or the files of novelty_reference - on the GPU, exact in fp64 (BaseModel.novelty: cae_case_neighbours;
    utils/novelty.py).  The train partition against itself is leave-one-out, and that pass also gives
    the reference's own distribution of novelty, so it runs once.  novelty_<partition>.json holds the min, median and max
    of the novelty, the reference's 50th, 90th, 95th and 99th order statistics, the shares of the cases above the 95th and
    99th, Spearman's rank correlation of novelty with the mse, the mse and mae per novelty quintile, the ten most novel cases
    and the per-case values; the data set gets per-case novelty and nearest_case variables beside mae / mse, the report the
    "Novelty of the cases" section."""
    (ref_ds, loo) = _novelty_reference(ev)
    own = partition == "train" and not ev.novelty_reference
    case = loo if own else ev.model.novelty(ds, ref_ds, ev.model_input_variables, k=int(ev.novelty_k))
    record = novelty_scores.summary(case, reference=loo, mse=values["mse"], mae=values["mae"])
    _keep(ev, novelty_scores, "novelty", partition, record, report.setdefault("novelty", []))
    return {"novelty": case["novelty"], "nearest_case": case["nearest_case"]}


# ---- model comparison ------------------------------------------------------------------------

def _compare_settings(ev):
    """(variables, labels, resamples, seed, confidence) of the comparison, each refused where it is wrong"""
    (variables, labels) = compare_scores.check_candidates(ev.model_output_variable, ev.compare_variables, ev.compare_labels)
    return (variables, labels, compare_scores.check_resamples(ev.compare_resamples), compare_scores.check_seed(ev.compare_seed),
            compare_scores.parse_confidence(ev.compare_confidence))


def _compare_files(ev, partition, ds, variables, target=None):
    """refuses a partition that does not hold the comparison's variables in the shapes it needs.  target None: before the
    model is loaded its name is not known, so the candidates are held to the first of them that is there."""
    found = [v for v in variables[1:] if v not in ds]
    if found:
        raise ValueError(f"compare needs the variable {found[0]!r} in the {partition} data set (apply_cae --prediction-variable "
                         f"{found[0]} writes it)")
    shapes = [(v, tuple(ds[v].shape)) for v in ([target] if target else []) + list(variables) if v in ds]
    for (v, shape) in shapes:
        if len(shape) != 4 or shape[0] != shapes[0][1][0] or shape[2:] != shapes[0][1][2:]:
            raise ValueError(f"compare: {v!r} {shape} and {shapes[0][0]!r} {shapes[0][1]} of the {partition} data set do not match: "
                             "(N, C, H, W) variables with N, H and W in common expected")
    name = ev.compare_block_variable
    if name:
        if name not in ds or len(ds[name].shape) != 1 or (shapes and ds[name].shape[0] != shapes[0][1][0]):
            raise ValueError(f"compare_block_variable {name!r} is not a variable of the {partition} data set with one value per case")
    if shapes and not ev.compare_block_variable and shapes[0][1][0] > compare_scores.MAX_UNITS:
        raise ValueError(f"compare: at most {compare_scores.MAX_UNITS} resampling units expected, the {partition} data set has "
                         f"{shapes[0][1][0]} cases; name a compare_block_variable")


def check_compare(ev):
    """the refusals of the settings, and of the files as far as they can be seen before the model is loaded: no GPU yet"""
    if not ev.compare:
        return
    variables = _compare_settings(ev)[0]
    if ev.compare_baseline is not None and ev.compare_baseline not in baseline_scores.MODES:
        raise ValueError(f"compare_baseline must be one of {', '.join(baseline_scores.MODES)}, got {ev.compare_baseline!r}")
    for (partition, paths) in (("test", ev.testing_paths), ("train", ev.training_paths)):
        if paths and (len(variables) > 1 or ev.compare_block_variable):
            for path in paths:
                _compare_files(ev, partition, open_mfdataset([path]), variables)


def check_compare_model(ev):
    """what check_compare cannot see before the model is loaded: the candidates have the target's cases and plane"""
    if not ev.compare:
        return
    variables = _compare_settings(ev)[0]
    for (partition, paths) in (("test", ev.testing_paths), ("train", ev.training_paths)):
        ds = ev._open(paths)
        if ds is not None:
            _compare_files(ev, partition, ds, variables, target=ev.output_variable)
            name = ev.model_input_variables[0]
            if ev.compare_baseline is not None and (name not in ds or len(ds[name].shape) != 4):
                raise ValueError(f"compare_baseline needs the model's first input variable {name!r} as a 4-dimensional variable "
                                 f"of the {partition} data set")


def _compare(ev, partition, ds, values, report):
    """compare=True (cli/compare.py) asks whether a difference between models survives resampling the cases: the evaluator's
    prediction and the compare_variables - other models' predictions in the same scored files (apply_cae
    --prediction-variable) - are held against the target on the pixels where the target and all of them are finite, one
    streaming cae_case_compare pass on the GPU; the per-case sums, or with compare_block_variable the sums of the cases of
    equal value, are the units of a paired bootstrap on the GPU (cae_bootstrap_sums: compare_resamples resamples drawn from
    compare_seed; utils/compare.py).  compare_<partition>.json holds per candidate mse, rmse, mae and
    bias with their intervals at compare_confidence, per competitor delta_mse, skill, p_better, significant and the shares
    of pixels won and tied; with compare_baseline the skill against interpolating the first input with its interval, from
    cae_case_baseline's sums resampled with the same seed.  The report gets the "Model comparison" section."""
    (variables, labels, resamples, seed, confidence) = _compare_settings(ev)
    a = ev.operand(partition, ds, ev.output_variable)
    rows = case_compare([ev.operand(partition, ds, v) for v in variables], a)
    block = as_numpy(ds[ev.compare_block_variable]) if ev.compare_block_variable else None
    table = compare_scores.units(rows, block)[0]
    if not 1 <= table.shape[0] <= compare_scores.MAX_UNITS:
        raise ValueError(f"compare: 1 to {compare_scores.MAX_UNITS} resampling units expected, the {partition} data set has {table.shape[0]}")
    base = None
    if ev.compare_baseline is not None:
        name = ev.model_input_variables[0]
        sums = case_baseline(ev.operand(partition, ds, name), ev.operand(partition, ds, ev.model_output_variable), a,
                             mode=ev.compare_baseline)
        units = compare_scores.units(sums, block)[0]
        base = compare_scores.baseline_summary(units, bootstrap_table(units, resamples, seed), confidence, ev.compare_baseline, name)
    record = compare_scores.summary(table, bootstrap_table(table, resamples, seed), variables, labels, confidence, resamples, seed,
                                    n_cases=rows.shape[0], plane=int(a.shape[2]) * int(a.shape[3]),
                                    block_variable=ev.compare_block_variable or None, baseline=base)
    _keep(ev, compare_scores, "compare", partition, record, report.setdefault("compare", []))
    return {}


ENSEMBLE = Analysis(lambda ev: ev.ensemble_size is not None, check_ensemble, partition=_ensemble)
CASE_PAGES = Analysis(lambda ev: ev.x_coordinate and ev.y_coordinate and ev.time_coordinate, partition=_case_pages)
SSIM = Analysis(lambda ev: ev.ssim, partition=_ssim)
BASELINE = Analysis(lambda ev: ev.baseline, check_baseline, partition=_baseline)
SKILL_MAPS = Analysis(lambda ev: ev.skill_maps, after=_skill_maps)
SPECTRA = Analysis(lambda ev: ev.spectra, after=_spectra)
DISTRIBUTION = Analysis(lambda ev: ev.distribution, check_distribution, after=_distribution)
STRATA = Analysis(lambda ev: ev.strata, check_strata, after=_strata)
FSS = Analysis(lambda ev: ev.fss, check_fss, after=_fss)
# in the order build_html runs them: per partition ensemble, case pages, ssim, baseline, novelty, compare; then skill maps,
# spectra, distribution, strata, fss, importance
IMPORTANCE = Analysis(lambda ev: ev.importance, check_importance, after=_importance)
NOVELTY = Analysis(lambda ev: ev.novelty, check_novelty, partition=_novelty)
COMPARE = Analysis(lambda ev: ev.compare, check_compare, partition=_compare)
ANALYSES = (ENSEMBLE, CASE_PAGES, SSIM, BASELINE, NOVELTY, COMPARE, SKILL_MAPS, SPECTRA, DISTRIBUTION, STRATA, FSS, IMPORTANCE)
