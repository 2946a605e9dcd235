"""distribution - evaluate_cae with the verification along value: evaluate_cae's flags plus --distribution-bins (1 to 128
coarse bins, default 128), and besides its report (which then has a "Value distribution" section) per partition a file
distribution_<partition>.json in --output-html-folder with the joint histogram of prediction against target of channel 0, the
conditional bias, mae and rmse per target bin, the reliability curve per prediction bin, the conditional slope, the
quantiles of both and their differences, the Wasserstein-1 distance, the Perkins score and the hits, misses, false alarms,
POD, FAR, CSI and frequency bias at the target's 5th, 90th, 95th and 99th percentile (utils/distribution.py; the counts and
sums are one cae_joint_hist pass on the GPU), and a page distribution/index.html with the joint density and the curves.  One
line per partition is printed:

    distribution <partition>: slope <s>, q95 bias <b>, W1 <w>, Perkins <p>, POD/FAR at q95 <x>/<y>

    python -m cae_tools_amd.cli.distribution --test-inputs scored.nc --model-folder model --output-html-folder report

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
import argparse

from . import evaluate_cae


def _bins(text):
    n = int(text)
    if not 1 <= n <= 128:
        raise argparse.ArgumentTypeError(f"1 to 128 bins expected, got {n}")
    return n


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with the value distribution of prediction against target (distribution_<partition>.json)"
    p.add_argument("--distribution-bins", type=_bins, help="coarse bins of the joint histogram, 1 to 128", default=128)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    evaluate_cae.run(args, distribution=True, distribution_bins=args.distribution_bins)


if __name__ == "__main__":
    main()
