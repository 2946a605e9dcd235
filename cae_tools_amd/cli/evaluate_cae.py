"""evaluate_cae — command line front end with the reference's flags (src/cae_tools/cli/evaluate_cae.py:23-55): the
metrics of a model folder on training and / or test files, an optional database row, and with --output-html-folder an
index.html report with per-case error histograms (ModelEvaluator).  With --x-coordinate, --y-coordinate and
--time-coordinate it also writes <partition>/index.html case pages linked from the report: channel 0 of the
--input-variables, the target, the prediction and their difference for --sample-count evenly spaced cases (all without
it), worst mse first; drawn by netcdf2html where that is installed, else by the package itself on the GPU
(utils/case_pages.py; value ranges and palette indices as models/model_evaluator.py defines them)."""
import argparse

from ..models.model_evaluator import ModelEvaluator


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--train-inputs", nargs="+", help="path to netcdf4 file(s) containing training data")
    p.add_argument("--test-inputs", nargs="+", help="path to netcdf4 file(s) containing test data")
    p.add_argument("--output-html-folder", help="folder to write output html to", default="")
    p.add_argument("--input-variables", nargs="*", help="input variables to plot")
    p.add_argument("--sample-count", type=int, help="fraction of cases to plot for each partition", default=None)
    p.add_argument("--model-folder", help="folder to save the trained model to", required=True)
    p.add_argument("--prediction-variable", help="name of the prediction variable to create in output data "
                   "(default: model_output, the name apply_cae writes)", default=None)
    p.add_argument("--x-coordinate", help="name of the x-coordinate", default=None)
    p.add_argument("--y-coordinate", help="name of the y-coordinate", default=None)
    p.add_argument("--time-coordinate", help="name of the time-coordinate", default=None)
    p.add_argument("--database-path", type=str, help="path to a database to store evaluation results", default=None)
    return p


def run(args, **evaluator_options):
    """the evaluator over parsed flags; evaluator_options: further ModelEvaluator keywords (cli/skill_maps.py)"""
    mt = ModelEvaluator(training_paths=args.train_inputs,
                        testing_paths=args.test_inputs,
                        output_html_folder=args.output_html_folder,
                        model_path=args.model_folder,
                        model_output_variable=args.prediction_variable or "model_output",
                        input_variables=args.input_variables,
                        sample_count=args.sample_count,
                        database_path=args.database_path,
                        x_coordinate=args.x_coordinate,
                        y_coordinate=args.y_coordinate,
                        time_coordinate=args.time_coordinate, **evaluator_options)
    mt.run()


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
