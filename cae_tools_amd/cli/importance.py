"""importance - evaluate_cae with the permutation importance of the model's input variables: evaluate_cae's flags plus
--importance-repeats R (1 to 64 permutations, default 5), --importance-seed S (default 0), --importance-groups G ... (each G a
comma-separated list of input-variable names forming one group; when given, only those groups are evaluated, else every
input variable on its own) and --importance-maps.  Every case is given another case's values for the variables of a group -
each permutation is a single cycle over the cases, so no case keeps its own, and the same permutations serve every group -
the batch is scored again through the model, and the growth of the error against the target is reduced on the GPU
(BaseModel.importance: cae_normalise_pack_gather and cae_case_importance; utils/importance.py).  Besides
the report (which then has an "Input importance" section with the table of the groups by rank and the bar chart of importance
+- sd) it writes per partition a file importance_<partition>.json in --output-html-folder with, per group, the pooled mse and
mae with and without the permutation per repeat, importance = mse permuted - mse with its standard deviation over the repeats,
the ratio, the sensitivity sqrt(mean (P1 - P0)^2) of the prediction, the shares of cases and pixels whose error grew, the rank
and the per-case change of the mse; with --importance-maps also importance/index.html, one map of the change of the mse per
pixel and group.  One line per partition is printed, the groups largest importance first:

    importance <partition>: <G> groups x <R> permutations of <N> cases, base mse <x>: <name> +<d> (x<ratio>), ...

    python -m cae_tools_amd.cli.importance --test-inputs scored.nc --model-folder model --output-html-folder report \\
        --importance-repeats 5 --importance-groups lowres albedo,elevation --importance-maps

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
import argparse

from . import evaluate_cae
from ..utils import importance as importance_scores


def _repeats(text):
    n = int(text)
    if not 1 <= n <= importance_scores.MAX_REPEATS:
        raise argparse.ArgumentTypeError(f"1 to {importance_scores.MAX_REPEATS} permutations expected, got {n}")
    return n


def _seed(text):
    n = int(text)
    if n < 0:
        raise argparse.ArgumentTypeError(f"a seed of 0 or more expected, got {n}")
    return n


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with the permutation importance of the input variables (importance_<partition>.json)"
    p.add_argument("--importance-repeats", type=_repeats, default=5, metavar="R", help="permutations per group, 1 to 64 (default 5)")
    p.add_argument("--importance-seed", type=_seed, default=0, metavar="S", help="seed of the permutations (default 0)")
    p.add_argument("--importance-groups", nargs="+", metavar="G",
                   help="groups of input variables, each a comma-separated list of names (default: every variable on its own)")
    p.add_argument("--importance-maps", action="store_true", help="also write importance/index.html with the per-pixel maps")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        groups = importance_scores.parse_groups(args.importance_groups)
    except ValueError as refused:
        parser.error(str(refused))
    evaluate_cae.run(args, importance=True, importance_repeats=args.importance_repeats, importance_seed=args.importance_seed,
                     importance_groups=groups, importance_maps=args.importance_maps)


if __name__ == "__main__":
    main()
