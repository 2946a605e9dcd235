"""blend - fit the weights of a blend of up to 8 models scored on the same files, and apply them.

    python -m cae_tools_amd.cli.blend fit --inputs scored.nc --output-variable hires \\
        --blend-variables model_output unet_output linear_output --blend-labels convae unet linear --output-html-folder report
    python -m cae_tools_amd.cli.blend apply scored.nc blended.nc --blend-file blend.json

fit: the candidates - prediction variables of the same scored files, as apply_cae --prediction-variable V writes them from
several model folders - are held against --output-variable on the pixels where it and all of them are finite, in one streaming
pass on the GPU that forms per case n, S e_m and every S e_i e_j of the errors e_m = P_m - a (cae_case_error_moments).  With
weights that add to 1 the blend's mse is w' E w with E = S e_i e_j / n, so the weights (--blend-mode convex: Sw = 1 and w >= 0,
the default; affine: Sw = 1; equal: 1 / M; with --blend-intercept also a constant), their K-fold cross-validated gain over the
best single candidate (--blend-folds K, default 5, 0 switches it off) and their bootstrap intervals (--blend-resamples B,
default 2000, 0 for none; --blend-seed S; --blend-confidence C; --blend-block-variable NAME: cases of equal value are resampled
together and share a fold; cae_bootstrap_sums) all come from those rows without a second read of the data (utils/blend.py,
DESIGN.md section 9).  It writes --blend-file (default blend.json) - the weights and the intercept as float.hex() text as well
as numbers, per candidate mse and bias, the error correlation matrix, the in-sample mse of the blend and of the best single
candidate, the gain, the cross-validation and the intervals - prints one line

    blend: <M> candidates, <U> units, <mode>: <label> <w> [lo, hi], ...; mse <x> against <label> <y>, gain <g> [lo, hi]; cross-validated (<K> folds) gain <g>

and with --output-html-folder DIR writes DIR/blend/index.html with the error-correlation table and a bar chart of the weights
with interval whiskers.

apply: the data set is written to OUTPUT with one more float64 variable (--prediction-variable, default blend_output) on the
dimensions of the first candidate: intercept + S w_m P_m over all channels with the fitted bits (cae_blend_predictions), NaN
where a candidate with a weight other than 0 is not finite.  A candidate whose weight is 0 is not read and need not be there.

Not a reference command, and it needs no model folder."""
import argparse
import os

import numpy as np

from ..data.arrays import DataArray, as_numpy, open_mfdataset
from ..utils import blend as blend_scores
from ..utils import compare as compare_scores


def _checked(check):
    def parse(text):
        try:
            return check(int(text))
        except ValueError as refused:
            raise argparse.ArgumentTypeError(str(refused)) from None
    return parse


def _confidence(text):
    try:
        blend_scores.parse_confidence(text)
    except ValueError as refused:
        raise argparse.ArgumentTypeError(str(refused)) from None
    return text


def build_parser():
    p = argparse.ArgumentParser(prog="blend", description="fit the weights of a blend of models scored on the same files, and apply them")
    sub = p.add_subparsers(dest="command", required=True)
    f = sub.add_parser("fit", help="fit the weights from the error moments of the candidates (blend.json)")
    f.add_argument("--inputs", nargs="+", required=True, metavar="F", help="the scored file(s) that hold the target and the candidates")
    f.add_argument("--output-variable", required=True, metavar="NAME", help="the target variable")
    f.add_argument("--blend-variables", nargs="+", required=True, metavar="V", help="the candidates: 1 to 8 prediction variables")
    f.add_argument("--blend-labels", nargs="+", default=None, metavar="L", help="one label per candidate (default the variables' names)")
    f.add_argument("--blend-mode", choices=list(blend_scores.MODES), default=blend_scores.DEFAULT_MODE,
                   help="convex: weights >= 0 that add to 1 (default); affine: weights that add to 1; equal: 1 / M")
    f.add_argument("--blend-intercept", action="store_true", help="also fit a constant")
    f.add_argument("--blend-block-variable", default=None, metavar="NAME",
                   help="a variable with one value per case: cases of equal value are resampled together and share a fold")
    f.add_argument("--blend-folds", type=_checked(blend_scores.check_folds), default=blend_scores.DEFAULT_FOLDS, metavar="K",
                   help="folds of the cross-validation, 0 switches it off (default 5)")
    f.add_argument("--blend-resamples", type=_checked(blend_scores.check_resamples), default=blend_scores.DEFAULT_RESAMPLES, metavar="B",
                   help="bootstrap resamples, 0 for no intervals, at most 10^6 (default 2000)")
    f.add_argument("--blend-seed", type=_checked(blend_scores.check_seed), default=0, metavar="S", help="seed of the resamples (default 0)")
    f.add_argument("--blend-confidence", type=_confidence, default=blend_scores.DEFAULT_CONFIDENCE, metavar="C",
                   help="confidence of the intervals as decimal text or num/den (default 0.95)")
    f.add_argument("--blend-file", default=blend_scores.DEFAULT_FILE, metavar="PATH", help="the record to write (default blend.json)")
    f.add_argument("--output-html-folder", default=None, metavar="DIR", help="also write DIR/blend/index.html")
    a = sub.add_parser("apply", help="write the data set with the blended field as one more variable")
    a.add_argument("data_paths", nargs="+", metavar="DATA", help="the file(s) that hold the candidates")
    a.add_argument("output_path", metavar="OUTPUT", help="the file to write: the data plus the blended field")
    a.add_argument("--blend-file", required=True, metavar="PATH", help="the record blend fit wrote")
    a.add_argument("--prediction-variable", default=blend_scores.DEFAULT_PREDICTION_VARIABLE, metavar="NAME",
                   help="name of the variable to create (default blend_output)")
    return p


def check_fit_files(ds, target, variables, block_variable, folds):
    """refuses a data set that does not hold the target and the candidates as (N, C, H, W) variables with N, H and W in common,
    a block variable that is not per case, more than 2^20 units, or fewer units than folds; returns (n_cases, plane, n_unit)"""
    for v in [target] + list(variables):
        if v not in ds:
            raise ValueError(f"blend fit needs the variable {v!r} in the data set (apply_cae --prediction-variable writes a candidate)")
    shapes = [(v, tuple(ds[v].shape)) for v in [target] + list(variables)]
    for (v, shape) in shapes:
        if len(shape) != 4 or shape[0] != shapes[0][1][0] or shape[2:] != shapes[0][1][2:]:
            raise ValueError(f"blend fit: {v!r} {shape} and {shapes[0][0]!r} {shapes[0][1]} do not match: (N, C, H, W) variables with N, H "
                             "and W in common expected")
    n = int(shapes[0][1][0])
    n_unit = n
    if block_variable:
        if block_variable not in ds or len(ds[block_variable].shape) != 1 or ds[block_variable].shape[0] != n:
            raise ValueError(f"blend_block_variable {block_variable!r} is not a variable of the data set with one value per case")
        n_unit = int(compare_scores.units(np.zeros((n, 1)), as_numpy(ds[block_variable]))[0].shape[0])
    elif n > blend_scores.MAX_UNITS:
        raise ValueError(f"blend fit: at most {blend_scores.MAX_UNITS} resampling units expected, the data set has {n} cases; name a "
                         "blend_block_variable")
    if not 1 <= n_unit <= blend_scores.MAX_UNITS:
        raise ValueError(f"blend fit: 1 to {blend_scores.MAX_UNITS} resampling units expected, the data set has {n_unit}")
    blend_scores.check_folds(folds, n_unit)
    return n, int(shapes[0][1][2]) * int(shapes[0][1][3]), n_unit


def fit(args):
    (variables, labels) = blend_scores.check_candidates(args.blend_variables, args.blend_labels)
    mode = blend_scores.check_mode(args.blend_mode)
    (folds, resamples, seed) = (blend_scores.check_folds(args.blend_folds), blend_scores.check_resamples(args.blend_resamples),
                                blend_scores.check_seed(args.blend_seed))
    confidence = blend_scores.parse_confidence(args.blend_confidence)
    if args.output_variable in variables:
        raise ValueError(f"blend_variables: {args.output_variable!r} is the target")
    ds = open_mfdataset(args.inputs)
    (n_cases, plane, _) = check_fit_files(ds, args.output_variable, variables, args.blend_block_variable, folds)
    # everything above is refused before the GPU library is loaded
    from ..case_ops import bootstrap_table, case_error_moments
    rows = case_error_moments([as_numpy(ds[v]) for v in variables], as_numpy(ds[args.output_variable]))
    block = as_numpy(ds[args.blend_block_variable]) if args.blend_block_variable else None
    table = compare_scores.units(rows, block)[0]
    resampled = bootstrap_table(table, resamples, seed) if resamples else None
    record = blend_scores.summary(table, resampled, variables, labels, mode, args.blend_intercept, confidence, resamples, seed, folds,
                                  n_cases=n_cases, plane=plane, block_variable=args.blend_block_variable or None)
    blend_scores.write_json(args.blend_file, record)
    if args.output_html_folder:
        folder = os.path.join(args.output_html_folder, "blend")
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, "index.html"), "w") as f:
            f.write(blend_scores.page(record))
    print(blend_scores.line(record))
    return record


def check_apply_files(ds, variables, weights, name):
    """refuses a name that already exists, a candidate with a weight other than 0 that is missing, and candidates that differ
    in shape; returns the candidates that are read and their weights"""
    if name in ds:
        raise ValueError(f"blend apply: the data set already holds a variable {name!r}; choose another --prediction-variable")
    kept = [(v, w) for (v, w) in zip(variables, weights) if w != 0.0]
    for (v, _) in kept:
        if v not in ds:
            raise ValueError(f"blend apply needs the variable {v!r} in the data set (apply_cae --prediction-variable writes it)")
    shapes = [(v, tuple(ds[v].shape)) for (v, _) in kept]
    for (v, shape) in shapes:
        if len(shape) != 4 or shape != shapes[0][1]:
            raise ValueError(f"blend apply: {v!r} {shape} and {shapes[0][0]!r} {shapes[0][1]} differ in shape: (N, C, H, W) candidates of "
                             "one shape expected")
    return [v for (v, _) in kept], np.array([w for (_, w) in kept], dtype=np.float64)


def apply(args):
    (variables, weights, intercept, _) = blend_scores.read_json(args.blend_file)
    ds = open_mfdataset(args.data_paths)
    (kept, w) = check_apply_files(ds, variables, weights, args.prediction_variable)
    # everything above is refused before the GPU library is loaded
    from ..case_ops import blend_predictions
    y = blend_predictions([as_numpy(ds[v]) for v in kept], w, intercept)
    ds[args.prediction_variable] = DataArray(y, dims=tuple(ds[kept[0]].dims))
    ds.to_netcdf(args.output_path)
    print(f"blend apply: {args.prediction_variable} = {intercept!r} + " + " + ".join(f"{wk!r} * {v}" for (v, wk) in zip(kept, w.tolist()))
          + f" written to {args.output_path}")


def main(argv=None):
    args = build_parser().parse_args(argv)
    return fit(args) if args.command == "fit" else apply(args)


if __name__ == "__main__":
    main()
