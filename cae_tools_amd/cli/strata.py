"""strata - evaluate_cae with the error conditioned on a variable that is neither target nor prediction: evaluate_cae's flags
plus --strata-variable NAME (required: a variable of the data sets, 4-D with the case dimension first - on the target's grid
or any other over the same extent - or 1-D along the cases), --strata-channel C and one of --strata-edges E ... (finite,
ascending), --strata-classes V ... (a categorical variable: an edge midway between neighbouring classes) and --strata-count N
(N equal bins over the range of the variable's finite values, default 8; at most 64 strata in every form).  Besides the
report (which then has a "Skill by stratum" section with a table and a bar chart of bias +- rmse) it writes per partition a
file strata_<partition>.json in --output-html-folder with pixels, pairs, share, mean target and prediction, bias, mae, rmse,
correlation, sd_ratio and the share of the squared error per stratum and pooled (utils/strata.py; the counts and sums are two
cae_strata_sums passes on the GPU).  One line per partition is printed:

    strata <partition>: <variable>, <n> strata, rmse <lowest> (<label>) .. <highest> (<label>), unclassified <count>

    python -m cae_tools_amd.cli.strata --test-inputs scored.nc --model-folder model --output-html-folder report \\
        --strata-variable elevation --strata-edges 500 1000 1500

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
import argparse

from . import evaluate_cae


def _count(text):
    n = int(text)
    if not 1 <= n <= 64:
        raise argparse.ArgumentTypeError(f"1 to 64 strata expected, got {n}")
    return n


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with the skill per stratum of a third variable (strata_<partition>.json)"
    p.add_argument("--strata-variable", required=True, help="the variable of the data sets that cuts the pixels into strata")
    p.add_argument("--strata-channel", type=int, default=0, help="its channel, default 0")
    how = p.add_mutually_exclusive_group()
    how.add_argument("--strata-edges", type=float, nargs="+", help="finite, ascending edges: up to 63")
    how.add_argument("--strata-classes", type=float, nargs="+", help="the values of a categorical variable: up to 64")
    how.add_argument("--strata-count", type=_count, help="equal bins over the variable's range, 1 to 64 (default 8)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    evaluate_cae.run(args, strata=True, strata_variable=args.strata_variable, strata_channel=args.strata_channel,
                     strata_edges=args.strata_edges, strata_classes=args.strata_classes,
                     strata_count=8 if args.strata_count is None else args.strata_count)


if __name__ == "__main__":
    main()
