"""compare - evaluate_cae with models compared on the same cases and pixels, with bootstrap intervals: evaluate_cae's flags plus
--compare-variables V ... (up to 7 other prediction variables of the same scored files, as apply_cae --prediction-variable V
writes them from other model folders; may be empty: the model's own mse, mae and bias then get their intervals),
--compare-labels L ... (one per candidate, the folder's model first; default the variables' names), --compare-resamples B
(1 to 10^6, default 10000), --compare-seed S (default 0), --compare-confidence C (decimal text or num/den, default 0.95),
--compare-block-variable NAME (one value per case: the cases of equal value are resampled together, a block bootstrap for
boxes of one day or one location) and --compare-baseline MODE (nearest, bilinear or bicubic: also the skill against
interpolating the model's first input, with its interval).  Target and predictions are read once on the GPU over the pixels
where all of them are finite (cae_case_compare), the per-case sums are resampled there (cae_bootstrap_sums; utils/compare.py,
DESIGN.md section 9): exact, the same from run to run.  Besides the report (which then has a "Model comparison" section with
the table and the bar chart of the mse with interval whiskers) it writes per partition a file compare_<partition>.json in
--output-html-folder with, per candidate, mse, rmse, mae and bias with their intervals and, per competitor, delta_mse = its mse
minus the folder's model's, skill = 1 - mse_0 / mse_m (above 0: the folder's model is better), p_better, significant (the
interval of delta_mse excludes 0) and the shares of pixels won and tied.  One line per partition is printed:

    compare <partition>: <M> candidates, <U> units x <B> resamples at <c>: <label> mse <x> [lo, hi]; <label> delta <d> [lo, hi] (significant), ...

    python -m cae_tools_amd.cli.compare --test-inputs scored.nc --model-folder model --output-html-folder report \\
        --compare-variables unet_output linear_output --compare-labels convae unet linear

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
import argparse

from . import evaluate_cae
from ..utils import compare as compare_scores
from ..utils.baseline import MODES


def _checked(check):
    def parse(text):
        try:
            return check(int(text))
        except ValueError as refused:
            raise argparse.ArgumentTypeError(str(refused)) from None
    return parse


def _confidence(text):
    try:
        compare_scores.parse_confidence(text)
    except ValueError as refused:
        raise argparse.ArgumentTypeError(str(refused)) from None
    return text


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with models compared on the same pixels, with bootstrap intervals (compare_<partition>.json)"
    p.add_argument("--compare-variables", nargs="*", default=[], metavar="V",
                   help="other prediction variables of the scored files, up to 7 (default none: intervals for the model's own scores)")
    p.add_argument("--compare-labels", nargs="+", default=None, metavar="L", help="one label per candidate, the folder's model first")
    p.add_argument("--compare-resamples", type=_checked(compare_scores.check_resamples), default=compare_scores.DEFAULT_RESAMPLES,
                   metavar="B", help="bootstrap resamples, 1 to 10^6 (default 10000)")
    p.add_argument("--compare-seed", type=_checked(compare_scores.check_seed), default=0, metavar="S", help="seed of the resamples (default 0)")
    p.add_argument("--compare-confidence", type=_confidence, default=compare_scores.DEFAULT_CONFIDENCE, metavar="C",
                   help="confidence of the intervals as decimal text or num/den (default 0.95)")
    p.add_argument("--compare-block-variable", default=None, metavar="NAME",
                   help="a variable with one value per case: cases of equal value are resampled together")
    p.add_argument("--compare-baseline", choices=list(MODES), default=None, metavar="MODE",
                   help="also the skill against interpolating the model's first input (nearest, bilinear or bicubic), with its interval")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        compare_scores.check_candidates(args.prediction_variable or "model_output", args.compare_variables, args.compare_labels)
    except ValueError as refused:
        parser.error(str(refused))
    evaluate_cae.run(args, compare=True, compare_variables=args.compare_variables, compare_labels=args.compare_labels,
                     compare_resamples=args.compare_resamples, compare_seed=args.compare_seed,
                     compare_confidence=args.compare_confidence, compare_block_variable=args.compare_block_variable,
                     compare_baseline=args.compare_baseline)


if __name__ == "__main__":
    main()
