"""ssim - evaluate_cae with the structural scores of prediction against target: exactly evaluate_cae's flags, and besides
its report (which then has a "Structural similarity" section) per partition a file ssim_<partition>.json in
--output-html-folder with the per-case SSIM, MS-SSIM (five scales, where min(h, w) > 160) and PSNR of channel 0, their
means and the window counts (utils/ssim.py; the sums are one cae_case_ssim pass on the GPU, fp64, the definition of the
`--method var` training loss).  One line per partition is printed:

    ssim <partition>: ssim <x> ms_ssim <y|none> psnr <z> dB, <n_counted>/<n> cases

    python -m cae_tools_amd.cli.ssim --test-inputs scored.nc --model-folder model --output-html-folder report

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
from . import evaluate_cae


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with SSIM, MS-SSIM and PSNR per case (ssim_<partition>.json)"
    return p


def main(argv=None):
    evaluate_cae.run(build_parser().parse_args(argv), ssim=True)


if __name__ == "__main__":
    main()
