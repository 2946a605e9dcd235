"""apply_scene — build-only command (the reference has none): apply a trained box model to a whole scene.  The input
variables are (time, channel, y, x) fields larger than the model's input box, gaps as NaN; the scene is cut into
overlapping boxes, scored on the GPU and blended back (BaseModel.apply_scene, DESIGN.md §9 'scene apply').  Takes
apply_cae's positional arguments, --model-folder, --input-variables and --prediction-variable, plus --overlap; writes the
inputs plus the prediction variable to a NetCDF file."""
import argparse
import os
import sys

import numpy as np

from ..data.arrays import open_mfdataset
from ..models.model_loader import load_model


ENSEMBLE_FLAGS = ("--ensemble-size", "--spread-variable", "--ensemble-seed", "--latent-variable")


def build_parser():
    p = argparse.ArgumentParser(description="apply a trained model to whole scenes: tile, score, blend")
    p.add_argument("data_paths", nargs="+", help="path to netcdf file(s) containing the scenes to which the model is applied")
    p.add_argument("output_path", help="path to write the netcdf file containing input data plus model outputs")
    p.add_argument("--model-folder", help="folder the trained model was saved to", required=True)
    p.add_argument("--input-variables", nargs="+", help="name of the input variable(s) in the scene data", required=False)
    p.add_argument("--prediction-variable", help="name of the prediction variable to create in output data", default="model_output")
    p.add_argument("--overlap", type=int, nargs="+", default=None, metavar="N",
                   help="overlap of neighbouring boxes in low-resolution pixels: N, or NY NX (default: a quarter of the box)")
    p.add_argument("--tile-rows", type=int, default=None, metavar="R",
                   help="score R rows of boxes at a time (default: chosen from a byte budget; the result does not depend on it)")
    p.add_argument("--gpus", type=int, default=1, help="shard the boxes over this many GPUs of the node")
    return p


def main(argv=None):
    parser = build_parser()
    asked = [a for a in (sys.argv[1:] if argv is None else argv) if a.split("=")[0] in ENSEMBLE_FLAGS]
    if asked:
        parser.error(f"{', '.join(asked)}: a scene has no ensemble or latent output (these are apply_cae's options)")
    args = parser.parse_args(argv)
    if args.overlap is not None and len(args.overlap) > 2:
        parser.error("--overlap takes N, or NY NX")
    overlap = None if args.overlap is None else (args.overlap[0] if len(args.overlap) == 1 else tuple(args.overlap))
    from ._launch import maybe_spawn_ranks
    rc = maybe_spawn_ranks("cae_tools_amd.cli.apply_scene", args.gpus, argv)    # before anything touches the GPU
    if rc is not None:
        if rc:
            raise SystemExit(rc)
        return
    from .. import dp as _dp
    _dp.select_device()
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

    scene_ds = open_mfdataset(args.data_paths, concat_dim="time", combine="nested")
    lead = int(os.environ.get("RANK", "0")) == 0
    mt.apply_scene(scene_ds, input_variable_names, args.prediction_variable, overlap=overlap, tile_rows=args.tile_rows)
    report = mt.scene_report
    plan = report["plan"]
    if lead:
        print(f"Applying model to {report['time_steps']} scenes of {plan.Y} x {plan.X}: {plan.n_y} x {plan.n_x} tiles of "
              f"{plan.h} x {plan.w} -> {plan.H} x {plan.W}, overlap ({plan.oy}, {plan.ox}), output {plan.out_shape[0]} x {plan.out_shape[1]}")
        (bad, holes) = (np.asarray(report["invalid_tiles"]), np.asarray(report["nan_pixels"]))
        print(f"invalid tiles: {int(bad.sum())} of {plan.n_tile * report['time_steps']} (per time step: {bad.tolist()})")
        print(f"NaN pixels: {int(holes.sum())} of {plan.out_shape[0] * plan.out_shape[1] * report['time_steps']} "
              f"(per time step: {holes.tolist()})")
        scene_ds.to_netcdf(args.output_path)


if __name__ == "__main__":
    main()
