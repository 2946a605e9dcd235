"""novelty - evaluate_cae with the novelty of every case against the training set: evaluate_cae's flags plus --novelty-k K
(1 to 32, default 5) and --novelty-reference F ... (the files of the reference set; default: the --train-inputs).  Every case is
packed and normalised as the model sees it, and its K nearest reference cases in that space are found on the GPU, exact in
fp64 (BaseModel.novelty: cae_case_neighbours; utils/novelty.py); the novelty of a case is the rms
difference per feature to its K-th nearest reference case.  The reference set measured against itself is leave-one-out: no case
names itself, and that pass gives the reference's own distribution of novelty, against whose 95th and 99th order statistics
the cases of a partition are counted as outside the training domain.  Besides the report (which then has a "Novelty of the
cases" section with the table and the bar chart of the mse per novelty quintile) it writes per partition a file
novelty_<partition>.json in --output-html-folder, adds per-case novelty and nearest_case variables beside mae / mse, and prints
one line per partition:

    novelty <partition>: <n> cases against <r> reference cases, k <K>, <D> features: median <m>, max <x>, outside p95 <s>, ...

    python -m cae_tools_amd.cli.novelty --train-inputs train.nc --test-inputs test.nc --model-folder model \\
        --output-html-folder report --novelty-k 5

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
import argparse

from . import evaluate_cae
from ..utils import novelty as novelty_scores


def _k(text):
    n = int(text)
    if not 1 <= n <= novelty_scores.MAX_K:
        raise argparse.ArgumentTypeError(f"1 to {novelty_scores.MAX_K} neighbours expected, got {n}")
    return n


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with the novelty of the cases against the training set (novelty_<partition>.json)"
    p.add_argument("--novelty-k", type=_k, default=5, metavar="K",
                   help="the novelty is the distance to the K-th nearest reference case, 1 to 32 (default 5)")
    p.add_argument("--novelty-reference", nargs="+", default=None, metavar="F",
                   help="file(s) of the reference set (default: the --train-inputs)")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.novelty_reference and not args.train_inputs:
        parser.error("novelty needs a reference set: --train-inputs, or --novelty-reference F ...")
    evaluate_cae.run(args, novelty=True, novelty_k=args.novelty_k, novelty_reference=args.novelty_reference)


if __name__ == "__main__":
    main()
