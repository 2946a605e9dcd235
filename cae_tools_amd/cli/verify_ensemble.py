"""verify_ensemble - evaluate_cae with the verification of a VAE's ensemble: evaluate_cae's flags plus --ensemble-size K
(required, 2 .. 64) and --ensemble-seed S.  Besides evaluate_cae's report, per partition the K draws that
apply_cae --ensemble-size K would average are verified against the target on the GPU (cae_ensemble_verify): the file
ensemble_<partition>.json in --output-html-folder (crps, fair crps, rmse of the ensemble mean, spread, spread-skill ratio,
rank counts, per-case crps, K and seed), a per-case crps histogram beside mae / mse, and an "Ensemble verification"
section in index.html.

    python -m cae_tools_amd.cli.verify_ensemble --test-inputs test.nc --model-folder model --output-html-folder report \\
        --ensemble-size 16

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added.  It needs a VarAEModel
folder (train_cae --method var) and an output folder."""
import json
import os

from . import evaluate_cae


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with the verification of the VAE's ensemble (ensemble_<partition>.json, report section)"
    p.add_argument("--ensemble-size", type=int, required=True, help="number of latent draws per case to verify (2 .. 64)")
    p.add_argument("--ensemble-seed", type=int, default=0, help="noise seed of the draws, as apply_cae --ensemble-seed")
    return p


def ensemble_keywords(args):
    """the ModelEvaluator keywords of the two flags.  parameters.json is read here, before the GPU is touched, and anything
    but a VarAEModel folder is refused."""
    with open(os.path.join(args.model_folder, "parameters.json")) as f:
        model_type = json.load(f).get("type")
    if model_type != "VarAEModel":
        raise SystemExit("verify_ensemble needs a VarAEModel folder (the VAE, train_cae --method var): "
                         f"{args.model_folder} holds a {model_type}")
    if not 2 <= args.ensemble_size <= 64:
        raise SystemExit("--ensemble-size must be from 2 to 64")
    if not args.output_html_folder:
        raise SystemExit("verify_ensemble writes its results to --output-html-folder: give one")
    return {"ensemble_size": args.ensemble_size, "ensemble_seed": args.ensemble_seed}


def main(argv=None):
    args = build_parser().parse_args(argv)
    evaluate_cae.run(args, **ensemble_keywords(args))


if __name__ == "__main__":
    main()
