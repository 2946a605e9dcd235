"""apply_cae — command line front end with the reference's arguments
(src/cae_tools/cli/apply_cae.py:28-90): load a model folder, score the input file(s) on the GPU,
write inputs + the denormalised prediction variable to a NetCDF file."""
import argparse
import json
import os

import numpy as np

from ..data.arrays import DataArray, open_mfdataset
from ..models.model_loader import load_model
from ..utils.augment import GROUPS as AUGMENT_GROUPS


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("data_paths", nargs="+", help="path to netcdf4 file(s) containing data to which model is applied")
    p.add_argument("output_path", help="path to write the netcdf4 file containing input data plus model outputs")
    p.add_argument("--model-folder", help="folder to save the trained model to", required=True)
    p.add_argument("--input-variables", nargs="+", help="name of the input variable(s) in training/test data", required=False)
    p.add_argument("--prediction-variable", help="name of the prediction variable to create in output data",
                   default="model_output")
    p.add_argument("--mask-variable", type=str, help="name of the mask variable", default=None)
    p.add_argument("--gpus", type=int, default=1, help="build-only: shard the cases over this many GPUs of the node")
    p.add_argument("--ensemble-size", type=int, default=None, metavar="K",
                   help="build-only, --method var models: decode K sampled latents per case and store their per-pixel mean")
    p.add_argument("--spread-variable", default=None, metavar="NAME",
                   help="with --ensemble-size K >= 2: also store the per-pixel standard deviation of the K fields under NAME")
    p.add_argument("--ensemble-seed", type=int, default=0, metavar="S", help="seed of the ensemble's noise")
    p.add_argument("--latent-variable", default=None, metavar="NAME",
                   help="--method var models: also store the latent mean and log-variance as NAME_mu and NAME_logvar")
    p.add_argument("--interval", default=None, metavar="L",
                   help="build-only: also store the prediction interval of coverage L (a level the model folder was calibrated "
                        "for: python -m cae_tools_amd.cli.calibrate) as two more variables")
    p.add_argument("--interval-variables", nargs=2, default=None, metavar=("LO", "HI"),
                   help="names of the two bounds (default: <prediction-variable>_lower and _upper)")
    p.add_argument("--scale-variable", default=None, metavar="NAME",
                   help="with --interval: the variable the calibration divided the residual by")
    p.add_argument("--self-ensemble", choices=list(AUGMENT_GROUPS), default=None,
                   help="build-only: score every case in the 4 (flips) or 8 (dihedral: square planes only) orientations of the "
                        "group, turn the outputs back and store their per-pixel mean")
    p.add_argument("--self-ensemble-spread", default=None, metavar="NAME",
                   help="with --self-ensemble: also store the per-pixel standard deviation of the orientations under NAME")
    p.add_argument("--novelty-variable", default=None, metavar="NAME",
                   help="build-only: also store the novelty of every scored case against --novelty-reference under NAME")
    p.add_argument("--novelty-reference", nargs="+", default=None, metavar="F",
                   help="with --novelty-variable: the file(s) of the reference set, usually the training data")
    p.add_argument("--novelty-k", type=int, default=None, metavar="K",
                   help="with --novelty-variable: the novelty is the distance to the K-th nearest reference case, 1 to 32 (default 5)")
    return p


def novelty_keywords(args):
    """the BaseModel.apply_novelty keywords of --novelty-variable (empty: none asked for), checked here, before any rank is
    spawned or the GPU touched"""
    if args.novelty_variable is None and args.novelty_reference is None:
        if args.novelty_k is not None:
            raise SystemExit("--novelty-k needs --novelty-variable NAME and --novelty-reference F ...")
        return {}
    if args.novelty_variable is None or args.novelty_reference is None:
        raise SystemExit("--novelty-variable and --novelty-reference need each other")
    from ..utils import novelty
    try:
        k = novelty.check_k(5 if args.novelty_k is None else args.novelty_k)
    except ValueError as refused:
        raise SystemExit(f"--novelty-k: {refused}") from None
    if args.novelty_variable == args.prediction_variable:
        raise SystemExit("--novelty-variable must differ from --prediction-variable")
    missing = [path for path in args.novelty_reference if not os.path.exists(path)]
    if missing:
        raise SystemExit(f"--novelty-reference: {', '.join(missing)} not found")
    return {"novelty_variable": args.novelty_variable, "k": k}


def _open_cases(paths, names):
    """the files concatenated along the case dimension, a per-case variable among `names` broadcast to a (case, 1, y, x) field"""
    ds = open_mfdataset(paths, concat_dim="box", combine="nested")
    case_dimension = ds[names[0]].dims[0]
    for var in names:
        if tuple(ds[var].dims) == (case_dimension,):
            (y_dim, x_dim) = (ds.dims["y"], ds.dims["x"])
            vals = np.asarray(ds[var].values)
            ds[var] = DataArray(np.broadcast_to(vals[:, None, None, None], (vals.shape[0], 1, y_dim, x_dim)).copy(),
                                dims=(case_dimension, "channel", "y", "x"))
    return ds, case_dimension


def interval_keywords(args):
    """the apply() keywords of --interval (empty: none asked for), checked against the folder's calibration.json here, before
    any rank is spawned or the GPU touched"""
    if args.interval is None:
        if args.interval_variables is not None or args.scale_variable is not None:
            raise SystemExit("--interval-variables and --scale-variable need --interval L")
        return {}
    from ..utils import conformal
    try:
        conformal.interval_request(args.model_folder, args.interval, args.scale_variable, args.interval_variables,
                                   args.prediction_variable)
    except (ValueError, FileNotFoundError) as refused:
        raise SystemExit(f"--interval: {refused}") from None
    return {"interval": args.interval, "interval_variables": args.interval_variables, "scale_variable": args.scale_variable}


def self_ensemble_keywords(args):
    """the apply() keywords of --self-ensemble (empty: none asked for), checked against the folder's parameters.json here, before
    any rank is spawned or the GPU touched"""
    if args.self_ensemble is None:
        if args.self_ensemble_spread is not None:
            raise SystemExit("--self-ensemble-spread needs --self-ensemble {flips,dihedral}")
        return {}
    if args.interval is not None:
        raise SystemExit("--interval needs the plain prediction the model was calibrated with: leave --self-ensemble out")
    if args.ensemble_size is not None:
        raise SystemExit("--self-ensemble and --ensemble-size are two ensembles: ask for one of them")
    if args.self_ensemble_spread is not None and args.self_ensemble_spread == args.prediction_variable:
        raise SystemExit("--self-ensemble-spread must differ from --prediction-variable")
    from ..models.base_model import residual_refusal
    from ..utils import augment
    with open(os.path.join(args.model_folder, "parameters.json")) as f:
        parameters = json.load(f)
    if parameters.get("residual_variable") is not None:
        raise SystemExit("--self-ensemble: " + residual_refusal("apply(self_ensemble=...)", parameters["residual_variable"]))
    try:
        augment.check_square(args.self_ensemble, [parameters["input_shape"], parameters["output_shape"]], "self_ensemble")
    except ValueError as refused:
        raise SystemExit(f"--self-ensemble: {refused}") from None
    return {"self_ensemble": args.self_ensemble, "self_ensemble_spread": args.self_ensemble_spread}


def ensemble_keywords(args):
    """the VarAEModel.apply keywords the command line asks for (empty: the plain apply).  They need a VarAEModel folder:
    parameters.json is read here, before any rank is spawned or the GPU touched, and anything else is refused."""
    asked = {k: v for k, v in (("ensemble_size", args.ensemble_size), ("spread_variable", args.spread_variable),
                               ("latent_variable", args.latent_variable)) if v is not None}
    if not asked and not args.ensemble_seed:
        return {}
    with open(os.path.join(args.model_folder, "parameters.json")) as f:
        model_type = json.load(f).get("type")
    if model_type != "VarAEModel":
        raise SystemExit("--ensemble-size / --spread-variable / --ensemble-seed / --latent-variable need a VarAEModel folder "
                         f"(the VAE, train_cae --method var): {args.model_folder} holds a {model_type}")
    if args.spread_variable is not None and (args.ensemble_size is None or args.ensemble_size < 2):
        raise SystemExit("--spread-variable needs --ensemble-size K with K >= 2")
    if args.ensemble_size is not None and args.ensemble_size < 1:
        raise SystemExit("--ensemble-size must be at least 1")
    asked["ensemble_seed"] = args.ensemble_seed
    return asked


def main(argv=None):
    args = build_parser().parse_args(argv)
    ensemble = ensemble_keywords(args)
    ensemble.update(interval_keywords(args))
    ensemble.update(self_ensemble_keywords(args))
    novelty = novelty_keywords(args)
    if "interval" in ensemble and "ensemble_size" in ensemble:
        raise SystemExit("--interval needs the plain prediction the model was calibrated with: leave --ensemble-size out")
    from ._launch import maybe_spawn_ranks
    rc = maybe_spawn_ranks("cae_tools_amd.cli.apply_cae", args.gpus, argv)   # before anything touches the GPU
    if rc is not None:
        if rc:
            raise SystemExit(rc)
        return
    from .. import dp as _dp
    _dp.select_device()     # inside a rank: LOCAL_RANK's GPU before the first allocation
    mt = load_model(args.model_folder)

    model_names = mt.get_input_variable_names()
    input_variable_names = args.input_variables
    if not input_variable_names:
        if model_names is None:
            raise Exception("Please specify the input variable names using --input-variables")
        input_variable_names = model_names
    elif model_names is not None and input_variable_names != model_names:
        raise Exception(f"input_variables [{','.join(input_variable_names)}] inconsistent with those used to train "
                        f"the model [{','.join(model_names)}]")

    (score_ds, case_dimension) = _open_cases(args.data_paths, model_names or input_variable_names)
    print("Applying model for %d cases" % score_ds[case_dimension].shape[0])
    mt.apply(score_ds, input_variable_names, args.prediction_variable, mask_variable_name=args.mask_variable, **ensemble)
    if novelty:
        (reference_ds, _) = _open_cases(args.novelty_reference, model_names or input_variable_names)
        mt.apply_novelty(score_ds, reference_ds, input_variable_names, **novelty)
    if int(os.environ.get("RANK", "0")) == 0:       # every rank holds all predictions (all-gather); rank 0 writes
        score_ds.to_netcdf(args.output_path)


if __name__ == "__main__":
    main()
