"""train_cae — command line front end with the reference's flags (src/cae_tools/cli/train_cae.py:19-53).

--method conv (ConvAEModel, the hot path), unet (UNET), var (VarAEModel: the reference's default method, whose model
source is missing there - this build's own definition, PARITY UNPINNED) and linear (LinearModel) are
implemented; the other method names are accepted by the parser, as in the reference, and rejected with a clear message
(the reference itself constructs no model for vae/unet_res/srcnn_res/resunet_gan: SURVEY.md fact 3).
Build-only flags: --gpus N (data-parallel ConvAE training over N GPUs of this node, one process per GPU) and --local-bn;
--residual-variable NAME / --residual-mode MODE train any of the four on the residual over the interpolated input
(DESIGN.md §9 'Residual target': the idea behind the reference's unet_res / srcnn_res names); --augment {flips,dihedral} /
--augment-seed S turn every training case by a symmetry of the square before every epoch (DESIGN.md §9 'Dihedral augmentation').
"""
import argparse
import json
import os
import time

import numpy as np

from ..data.arrays import DataArray, open_mfdataset
from ..lr_schedule import check_scheduler_type
from ..utils.augment import GROUPS as AUGMENT_GROUPS
from ..utils.baseline import MODES as RESIDUAL_MODES
from ..models.conv_ae_model import ConvAEModel
from ..models.unet import UNET
from ..models.linear_model import LinearModel
from ..models.var_ae_model import VarAEModel
from ..models.model_loader import load_model
from ..models.model_sizer import ModelSpec


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--train-inputs", nargs="+", help="path(s) to netcdf4 file containing training data", required=True)
    p.add_argument("--test-inputs", nargs="+", help="path(s) to netcdf4 file containing test data", required=True)
    p.add_argument("--model-folder", help="folder to save the trained model to", required=True)
    p.add_argument("--continue-training", action="store_true", help="continue training model")
    p.add_argument("--input-variables", nargs="+", help="name of the input variable(s) in training/test data", required=True)
    p.add_argument("--output-variable", help="name of the output variable in training/test data", required=True)
    p.add_argument("--nr-epochs", type=int, help="number of training epochs", default=500)
    p.add_argument("--latent-size", type=int, help="size of the latent space", default=4)
    p.add_argument("--fc-size", type=int, help="size of the fully-connected layers", default=16)
    p.add_argument("--batch-size", type=int, help="number of images to process in one batch", default=10)
    p.add_argument("--learning-rate", type=float, help="the learning rate", default=0.001)
    for (flag, typ, default, text) in [
            ("--lr-step-size", int, 500, "the schedular steps for the learning rate"),
            ("--lr-gamma", float, 0.5, "decay factor of the scheduled learning rate"),
            ("--lambda-mse", float, 1, "controls the strength of the mse loss in vae"),
            ("--lambda-kl", float, 1, "controls the strength of the kl loss in vae"),
            ("--lambda-l1", float, 0.001, "controls the strength of l1 regularization"),
            ("--lambda-pearson", float, 1, "controls the strength of the pearson loss"),
            ("--lambda-ssim", float, 1, "controls the strength of the ssim loss"),
            ("--lambda-additional", float, 1, "controls the strength of additional regularization"),
            ("--weight-decay", float, 1e-5, "weight decay coefficient"),
            ("--dropout-rate", float, 1e-1, "dropout rate")]:
        p.add_argument(flag, type=typ, help=text, default=default)
    p.add_argument("--additional-loss", type=str, default=None, help="additional loss types ('contrastive', 'histogram', 'perceptual')")
    p.add_argument("--scheduler-type", type=str, default=None, help="scheduler type ('StepLR', 'ReduceLROnPlateau', 'ExponentialLR','CosineAnnealingLR')")
    p.add_argument("--method", choices=["conv", "unet", "unet_res", "srcnn_res", "resunet_gan", "var", "vae", "linear"],
                   default="var", help="methods")
    p.add_argument("--layer-definitions-path", help="specify path of a JSON file with layer definitions", default=None)
    p.add_argument("--stride", type=int, help="stride to use in convolutional layers", default=2)
    p.add_argument("--kernel-size", type=int, help="kernel size to use in convolutional layers", default=3)
    p.add_argument("--input-layer-count", type=int, help="number of input convolutional layers", default=None)
    p.add_argument("--output-layer-count", type=int, help="number of output convolutional layers", default=None)
    p.add_argument("--model-id", type=str, help="specify the model id when creating a model", default=None)
    p.add_argument("--database-path", type=str, help="path to a database to store evaluation results", default=None)
    p.add_argument("--chunk-size", type=int, help="chunk size for xarray", default=1000)
    p.add_argument("--include-coasts", help="include coastal areas", default=False)
    p.add_argument("--mask-variable", type=str, help="name of the mask variable", default=None)
    # build-only: the reference trains on one device
    p.add_argument("--gpus", type=int, default=1, help="train data-parallel on this many GPUs of the node (conv method)")
    p.add_argument("--local-bn", action="store_true", help="with --gpus N: per-GPU BatchNorm statistics instead of statistics "
                   "over the global batch (faster; no longer the single-device arithmetic)")
    return p


def build_cli_parser():
    """build_parser() - the reference's flag table and the data-parallel flags - with the residual-target flags the command
    line takes on top (build-only; DESIGN.md §9 'Residual target')"""
    p = build_parser()
    p.add_argument("--residual-variable", type=str, default=None, metavar="NAME",
                   help="train on the output minus this low-resolution variable interpolated to the output grid, and add it back "
                        "when the model is applied (default with --residual-mode alone: the first input variable)")
    p.add_argument("--residual-mode", choices=list(RESIDUAL_MODES), default=None,
                   help="interpolation of the residual variable (default: bicubic)")
    p.add_argument("--augment", choices=list(AUGMENT_GROUPS), default=None,
                   help="turn every training case before every epoch: by the two flips and the half turn (flips), or by all eight "
                        "symmetries of the square (dihedral: square planes only).  Default: off; with --continue-training, what the "
                        "model folder was trained with")
    p.add_argument("--augment-seed", type=_augment_seed, default=None, metavar="S",
                   help="seed of the augmentation's codes (default: 0; with --continue-training, the model folder's)")
    return p


def _augment_seed(text):
    value = int(text)
    if not 0 <= value < 1 << 64:
        raise argparse.ArgumentTypeError("a seed from 0 to 2^64 - 1 expected")
    return value


def augment_keywords(args):
    """the train() keywords of --augment / --augment-seed: a flag that was not given is left out, so that a continued model
    keeps its folder's value and a fresh one its default (off, seed 0)"""
    keywords = {}
    if args.augment is not None:
        keywords["augment"] = args.augment
    if args.augment_seed is not None:
        keywords["augment_seed"] = args.augment_seed
    return keywords


def residual_settings(args, folder_parameters=None):
    """(variable, mode) the run trains its residual target with, (None, "bicubic") without one.  folder_parameters: the
    parameters.json of the folder --continue-training continues; its settings hold, and a flag that contradicts them ends
    the run."""
    asked = args.residual_variable is not None or args.residual_mode is not None
    variable = (args.residual_variable or args.input_variables[0]) if asked else None
    mode = args.residual_mode or "bicubic"
    if folder_parameters is None:
        return variable, mode
    held = (folder_parameters.get("residual_variable"), folder_parameters.get("residual_mode") or "bicubic")
    if asked and ((args.residual_variable is not None and args.residual_variable != held[0]) or
                  (args.residual_mode is not None and args.residual_mode != held[1]) or held[0] is None):
        was = f"the residual over '{held[0]}' ({held[1]})" if held[0] is not None else "no residual target"
        raise SystemExit(f"--continue-training: the model folder was trained with {was}; --residual-variable / --residual-mode "
                         "cannot change that")
    return held


def broadcast_case_variables(ds, variables, case_dimension):
    """a (case,) variable becomes (case, 1, y, x) by broadcasting (cli/train_cae.py:73-109)"""
    for var in variables:
        if tuple(ds[var].dims) == (case_dimension,):
            print(f"Variable '{var}' does not follow the dimension (box, channel, y, x). Extending dimensions...")
            (y_dim, x_dim) = (ds.dims["y"], ds.dims["x"])
            vals = np.asarray(ds[var].values)
            ds[var] = DataArray(np.broadcast_to(vals[:, None, None, None], (vals.shape[0], 1, y_dim, x_dim)).copy(),
                                dims=(case_dimension, "channel", "y", "x"))


def main(argv=None):
    args = build_cli_parser().parse_args(argv)
    try:    # a misspelt scheduler ends the run here, before ranks are spawned and the GPU library is loaded
        check_scheduler_type(args.scheduler_type)
    except ValueError as ex:
        raise SystemExit(f"--scheduler-type: {ex}")
    schedule = dict(scheduler_type=args.scheduler_type, lr_step_size=args.lr_step_size, lr_gamma=args.lr_gamma)
    folder_parameters = None
    if args.continue_training:      # the folder's residual settings hold: a contradicting flag ends the run here
        with open(os.path.join(args.model_folder, "parameters.json")) as f:
            folder_parameters = json.loads(f.read())
    (residual_variable, residual_mode) = residual_settings(args, folder_parameters)
    residual = dict(residual_variable=residual_variable, residual_mode=residual_mode)
    from ._launch import maybe_spawn_ranks
    from .. import dp as _dp
    if max(int(args.gpus or 1), _dp.env_world()[2]) > 1:
        # only ConvAEModel has a data-parallel training path: any other model under N ranks would be trained N times
        # independently, all ranks writing the same model folder and database.  Decided BEFORE ranks are spawned.
        kind = "ConvAEModel" if args.method == "conv" else args.method
        if args.continue_training:
            with open(os.path.join(args.model_folder, "parameters.json")) as f:
                kind = json.loads(f.read()).get("type")
        if kind != "ConvAEModel":
            raise SystemExit(f"--gpus {args.gpus}: data-parallel training is implemented for --method conv (ConvAEModel) only; "
                             f"this run would train a '{kind}' model - use --gpus 1")
    rc = maybe_spawn_ranks("cae_tools_amd.cli.train_cae", args.gpus, argv)   # before anything touches the GPU
    if rc is not None:
        if rc:
            raise SystemExit(rc)
        return
    _dp.select_device()     # inside a rank: LOCAL_RANK's GPU before the first allocation
    train_ds = open_mfdataset(args.train_inputs, concat_dim="box", combine="nested")
    test_ds = open_mfdataset(args.test_inputs, concat_dim="box", combine="nested")
    case_dimension = train_ds[args.output_variable].dims[0]
    print("Training cases: %d, Test cases: %d" % (train_ds[case_dimension].shape[0], test_ds[case_dimension].shape[0]))
    training_paths = ";".join(args.train_inputs)
    test_paths = ";".join(args.test_inputs)
    broadcast_case_variables(train_ds, args.input_variables, case_dimension)
    broadcast_case_variables(test_ds, args.input_variables, case_dimension)

    if args.continue_training:
        mt = load_model(args.model_folder)
        mt.nr_epochs = args.nr_epochs
        mt.lr = args.learning_rate
        mt._init_schedule(**schedule)
        mt.batch_size = args.batch_size
    else:
        if args.method == "conv":
            mt = ConvAEModel(fc_size=args.fc_size, encoded_dim_size=args.latent_size, nr_epochs=args.nr_epochs,
                             batch_size=args.batch_size, lr=args.learning_rate, **schedule, **residual)
        elif args.method == "unet":     # cli/train_cae.py:131-135
            mt = UNET(fc_size=args.fc_size, encoded_dim_size=args.latent_size, nr_epochs=args.nr_epochs,
                      batch_size=args.batch_size, lr=args.learning_rate, lambda_l1=args.lambda_l1,
                      lambda_pearson=args.lambda_pearson, database_path=args.database_path,
                      weight_decay=args.weight_decay, dropout_rate=args.dropout_rate, **schedule, **residual)
        elif args.method == "var":      # the reference's default method; its model source is missing there
            mt = VarAEModel(fc_size=args.fc_size, encoded_dim_size=args.latent_size, nr_epochs=args.nr_epochs,
                            batch_size=args.batch_size, lr=args.learning_rate, lambda_mse=args.lambda_mse,
                            lambda_kl=args.lambda_kl, lambda_ssim=args.lambda_ssim, weight_decay=args.weight_decay,
                            database_path=args.database_path, **schedule, **residual)
        elif args.method == "linear":   # cli/train_cae.py:137-138
            mt = LinearModel(batch_size=args.batch_size, nr_epochs=args.nr_epochs, lr=args.learning_rate, **schedule, **residual)
        else:
            raise SystemExit(f"--method {args.method}: cae_tools_amd implements 'conv' (ConvAEModel), 'unet' (UNET), 'var' "
                             "(VarAEModel) and 'linear' (LinearModel)")
        if args.model_id:
            mt.set_model_id(args.model_id)
        if args.layer_definitions_path:
            with open(args.layer_definitions_path) as f:
                spec = ModelSpec()
                spec.load(json.loads(f.read()))
                mt.spec = spec

    if hasattr(mt, "sync_bn"):
        mt.sync_bn = not args.local_bn
    start_time = time.time()
    print("Ready for training process")
    mt.train(args.input_variables, args.output_variable, training_ds=train_ds, testing_ds=test_ds,
             model_path=args.model_folder, training_paths=training_paths, testing_paths=test_paths,
             mask_variable_name=args.mask_variable, **augment_keywords(args))
    print(f"Time taken to train: {time.time() - start_time:.2f} seconds")


if __name__ == "__main__":
    main()
