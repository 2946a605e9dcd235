"""fss - evaluate_cae with the neighbourhood skill of the prediction: evaluate_cae's flags plus one of --fss-thresholds V ...
(event thresholds in data units) and --fss-percentiles Q ... (percentiles of the target's distribution in the partition,
default '<5' 90 95 99), --fss-widths N ... (odd, ascending neighbourhood widths from 1 to 129, at most 8; default 1 3 5 9 17
33 65 as far as the plane allows) and --fss-gaps {strict,ignore} (strict: a window over a value that is not finite is left
out; ignore: such a pixel is a non-event and only a window without any valid pixel is left out).  A threshold token with a
leading '<' is a below-event (v < t), any other an above-event (v >= t); at most 8 thresholds.  Besides the report (which
then has a "Neighbourhood skill" section with the table of the pooled Fractions Skill Score per threshold and width and a
link) it writes per partition a file fss_<partition>.json in --output-html-folder with the threshold values used, the
pooled window sums, the pooled and per-case FSS, the event frequencies, the uniform level 0.5 + f / 2 and the skilful width
(utils/fss.py; the sums are one cae_case_fss pass on the GPU, exact integers), and fss/index.html with the FSS curves
against the width.  One line per partition is printed:

    fss <partition>: <n> cases, widths <first>..<last> (<gaps>), skilful width <label> <width|none>[, <label> <width|none> ...]

with a label like ">=q90", "<q5" or ">=291.5" per threshold.

    python -m cae_tools_amd.cli.fss --test-inputs scored.nc --model-folder model --output-html-folder report \\
        --fss-percentiles '<5' 90 95 99 --fss-widths 1 3 9 33 129 --fss-gaps ignore

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
import argparse

from . import evaluate_cae


def _event(text):
    """a threshold token: (value, side), '<' in front for a below-event"""
    below = text.startswith("<")
    try:
        value = float(text[1:] if below else text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"a number, or '<' and a number, expected, got {text!r}") from None
    if value != value or value in (float("inf"), float("-inf")):
        raise argparse.ArgumentTypeError(f"a finite number expected, got {text!r}")
    return value, "below" if below else "above"


def _width(text):
    n = int(text)
    if not 1 <= n <= 129 or n % 2 == 0:
        raise argparse.ArgumentTypeError(f"an odd width from 1 to 129 expected, got {n}")
    return n


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with the Fractions Skill Score over neighbourhood widths (fss_<partition>.json)"
    how = p.add_mutually_exclusive_group()
    how.add_argument("--fss-thresholds", type=_event, nargs="+", metavar="V", help="event thresholds in data units; '<V' for v < V")
    how.add_argument("--fss-percentiles", type=_event, nargs="+", metavar="Q",
                     help="percentiles of the target's distribution; '<Q' for a below-event (default '<5' 90 95 99)")
    p.add_argument("--fss-widths", type=_width, nargs="+", metavar="N", help="odd, ascending neighbourhood widths, 1 to 129")
    p.add_argument("--fss-gaps", choices=("strict", "ignore"), default="strict", help="what a value that is not finite does to a window")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    evaluate_cae.run(args, fss=True, fss_thresholds=args.fss_thresholds, fss_percentiles=args.fss_percentiles,
                     fss_widths=args.fss_widths, fss_gaps=args.fss_gaps)


if __name__ == "__main__":
    main()
