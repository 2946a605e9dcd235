"""skill_maps — evaluate_cae with the per-pixel skill maps: exactly evaluate_cae's flags, and besides its report (which
then links them) per partition a NetCDF-3 file skill_<partition>.nc in --output-html-folder with count, bias, mae, rmse,
correlation and sd_ratio of channel 0 over the partition's cases, and the page maps/index.html that draws the six maps
(utils/skill_maps.py; the sums are one streaming pass of cae_pixel_sums on the GPU).

    python -m cae_tools_amd.cli.skill_maps --test-inputs scored.nc --model-folder model --output-html-folder report

A command of its own because evaluate_cae's flags are the reference's, to which nothing is added."""
from . import evaluate_cae


def build_parser():
    p = evaluate_cae.build_parser()
    p.description = "evaluate_cae with per-pixel skill maps (skill_<partition>.nc, maps/index.html)"
    return p


def main(argv=None):
    evaluate_cae.run(build_parser().parse_args(argv), skill_maps=True)


if __name__ == "__main__":
    main()
