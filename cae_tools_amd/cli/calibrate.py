"""calibrate - split conformal calibration of a trained model (build-only; not a reference command): a held-out calibration
set is scored exactly as apply_cae scores it, the absolute residual of channel 0 against --output-variable (divided by
--scale-variable where one is named) is ranked on the GPU, per pixel (--group pixel) or over all pixels (--group pooled), and
for every --coverage level the exact order statistic of rank ceil((n + 1) level) is kept (BaseModel.calibrate:
cae_score_quantiles; utils/conformal.py, DESIGN.md section 9 'prediction intervals').  The model folder receives
calibration.json - group, levels as num/den, variable names, cases, min / median / max of the valid scores per group, the
pooled quantiles (null for +inf) and, with --test-inputs, the held-out coverage - and for the pixel group calibration.nc with
quantile(level, y, x) and count(y, x); nothing else in the folder changes.  apply_cae --interval L then writes prediction -+ q
beside the prediction.  With exchangeable cases the interval covers the target with at least the stated probability, whatever
the model; a group with fewer than 1 / (1 - L) - 1 scores has q = +inf, an interval that says so.  One line per level is
printed:

    calibrate <num/den> <group>: <finite>/<groups> groups finite, median q <q>[, held-out coverage <covered>/<pairs> = <c>]

    python -m cae_tools_amd.cli.calibrate --calibration-inputs calib.nc --model-folder model --output-variable hires \\
        --coverage 0.8 0.9 0.95 --group pixel --test-inputs test.nc

Coverage levels are read as exact decimals (0.9 is 9/10), never as floats."""
import argparse
import os

import numpy as np

from ..data.arrays import DataArray, open_mfdataset
from ..utils import conformal


def build_parser():
    p = argparse.ArgumentParser(description="split conformal calibration of a model folder (calibration.json, calibration.nc)")
    p.add_argument("--calibration-inputs", nargs="+", required=True, metavar="F", help="netcdf file(s) with the held-out calibration cases")
    p.add_argument("--model-folder", required=True, help="folder of the trained model; receives the calibration")
    p.add_argument("--input-variables", nargs="+", help="name of the input variable(s) (default: the model's)")
    p.add_argument("--output-variable", required=True, help="name of the target variable")
    p.add_argument("--coverage", nargs="+", default=list(conformal.DEFAULT_LEVELS), metavar="L",
                   help="1 to 8 ascending coverage levels as decimals (default 0.8 0.9 0.95)")
    p.add_argument("--group", choices=sorted(conformal.GROUPS), default="pooled", help="one quantile per pixel, or one for all pixels")
    p.add_argument("--scale-variable", default=None, metavar="NAME",
                   help="a variable on the target's grid the residual is divided by (e.g. an ensemble spread apply_cae wrote)")
    p.add_argument("--test-inputs", nargs="+", default=None, metavar="F", help="netcdf file(s) whose held-out coverage is reported")
    p.add_argument("--mask-variable", type=str, default=None, help="name of the mask variable")
    p.add_argument("--gpus", type=int, default=1, help="shard the cases over this many GPUs of the node")
    return p


def open_cases(paths, input_variables):
    """the files as one data set, a per-case input variable broadcast over the plane as apply_cae broadcasts it"""
    ds = open_mfdataset(paths, concat_dim="box", combine="nested")
    case_dimension = ds[input_variables[0]].dims[0]
    for var in input_variables:
        if tuple(ds[var].dims) == (case_dimension,):
            (y_dim, x_dim) = (ds.dims["y"], ds.dims["x"])
            vals = np.asarray(ds[var].values)
            ds[var] = DataArray(np.broadcast_to(vals[:, None, None, None], (vals.shape[0], 1, y_dim, x_dim)).copy(),
                                dims=(case_dimension, "channel", "y", "x"))
    return ds


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        levels = conformal.parse_levels(args.coverage)
    except ValueError as refused:
        parser.error(str(refused))
    if not os.path.exists(os.path.join(args.model_folder, "parameters.json")):
        raise SystemExit(f"{args.model_folder} holds no trained model (parameters.json)")
    from ._launch import maybe_spawn_ranks
    rc = maybe_spawn_ranks("cae_tools_amd.cli.calibrate", args.gpus, argv)   # before anything touches the GPU
    if rc is not None:
        if rc:
            raise SystemExit(rc)
        return
    from .. import dp as _dp
    from ..models.model_loader import load_model
    _dp.select_device()
    model = load_model(args.model_folder)
    names = args.input_variables or model.get_input_variable_names()
    if not names:
        raise SystemExit("Please specify the input variable names using --input-variables")
    ds = open_cases(args.calibration_inputs, names)
    test_ds = open_cases(args.test_inputs, names) if args.test_inputs else None
    for (what, data) in (("calibration", ds), ("test", test_ds)):
        for name in (args.output_variable, args.scale_variable):
            if data is not None and name is not None and name not in data:
                raise SystemExit(f"the {what} inputs hold no variable {name!r}")
    record = model.calibrate(ds, names, args.output_variable, levels, group=args.group, scale_variable=args.scale_variable,
                             model_path=args.model_folder, test_ds=test_ds, mask_variable_name=args.mask_variable)
    for line in conformal.summary_lines(record):
        print(line)


if __name__ == "__main__":
    main()
