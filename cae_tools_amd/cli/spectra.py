"""spectra — evaluate_cae with the power spectra of prediction against target: exactly evaluate_cae's flags, and besides
its report (which then links them) per partition a file spectra_<partition>.json in --output-html-folder with the radially
binned power spectral density of prediction and target, their ratio, the spectral coherence, the error's share and the
effective resolution of channel 0, and the page spectra/index.html that draws them (utils/spectra.py; the sums are one
cae_case_spectra pass on the GPU).  One line per partition is printed:

    spectra <partition>: effective_resolution <x> pixels, <n_counted>/<n> cases

    python -m cae_tools_amd.cli.spectra --test-inputs scored.nc --model-folder model --output-html-folder report

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
from . import evaluate_cae


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with power spectra (spectra_<partition>.json, spectra/index.html)"
    return p


def main(argv=None):
    evaluate_cae.run(build_parser().parse_args(argv), spectra=True)


if __name__ == "__main__":
    main()
