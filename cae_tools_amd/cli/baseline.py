"""baseline - evaluate_cae with the skill against interpolating the model's own input: evaluate_cae's flags plus
--baseline-variable (default: the model's first input variable) and --baseline-mode (nearest, bilinear or bicubic; default
bicubic), and besides its report (which then has a "Skill against interpolation" section) per partition a file
baseline_<partition>.json in --output-html-folder with the pooled and per-case skill 1 - model_mse / baseline_mse of channel
0, the baseline's mse and mae, the share of cases and of pixels the model wins and the pixel counts (utils/baseline.py;
the sums are one cae_case_baseline pass on the GPU, fp64, the interpolated field never stored).  One line per partition is
printed:

    baseline <partition>: <mode> of <variable>, pooled skill <x> (baseline mse <y>, model mse <z>), <k>/<n> cases better

    python -m cae_tools_amd.cli.baseline --test-inputs scored.nc --model-folder model --output-html-folder report

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
from . import evaluate_cae
from ..utils.baseline import MODES


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with the skill against interpolating the input (baseline_<partition>.json)"
    p.add_argument("--baseline-variable", help="low-resolution variable to interpolate (default: the model's first input "
                   "variable)", default=None)
    p.add_argument("--baseline-mode", choices=list(MODES), help="interpolation of the baseline", default="bicubic")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    evaluate_cae.run(args, baseline=True, baseline_variable=args.baseline_variable, baseline_mode=args.baseline_mode)


if __name__ == "__main__":
    main()
