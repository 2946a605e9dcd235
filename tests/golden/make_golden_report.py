#!/usr/bin/env python3
"""Golden layout of the evaluate_cae report and the reference's evaluate_cae flag names.

Drives the reference's own Html5Builder / TableFragment (standard library only) through the sequence of headings, tables
and images that its ModelEvaluator.build_html (model_evaluator.py:162-314) writes for the fixed record below, and stores
the resulting (tag, text) items - not the reference's HTML - in report_layout.json.  The flag names of the reference's
cli/evaluate_cae.py are read from its syntax tree into evaluate_cae_flags.json.  Needs the reference's sources on the
path:

    PYTHONPATH=<reference checkout>/src python tests/golden/make_golden_report.py
"""
import ast
import html.parser
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

RECORD = {
    "metrics": {"test": {"mse": 0.0123456, "rmse": 0.111111, "mae": 0.0891, "mean_pearson_correlation": 0.98765},
                "train": {"mse": 0.0101, "rmse": 0.1004988, "mae": 0.0799, "mean_pearson_correlation": 0.9912}},
    "partitions": ["test", "train"],
    "measures": ["mae", "mse"],
    "parameters": {"type": "ConvAEModel", "model_id": "model-1", "batch_size": 10, "nr_epochs": 3, "test_interval": 1,
                   "encoded_dim_size": 4, "fc_size": 16, "lr": 0.001, "input_shape": [1, 16, 16],
                   "output_shape": [1, 256, 256], "conv_kernel_size": 3, "conv_stride": 2,
                   "conv_input_layer_count": None, "conv_output_layer_count": None},
    "history": {"nr_epochs": 3, "train_loss": [0.5, 0.25, 0.125], "test_loss": [0.6, 0.3, 0.2]},
}


class ReportItems(html.parser.HTMLParser):
    """the (tag, text) sequence of a report: title / h2 / h3 with their text, one ("tr", "cell|cell") per table row,
    ("img", "") per image"""

    TEXT = ("title", "h2", "h3", "td")

    def __init__(self):
        super().__init__(convert_charrefs=True)
        self.items = []
        self.open = None
        self.buf = []
        self.cells = []

    def handle_starttag(self, tag, attrs):
        if tag in self.TEXT:
            (self.open, self.buf) = (tag, [])
        elif tag == "tr":
            self.cells = []
        elif tag == "img":
            self.items.append(["img", ""])

    def handle_endtag(self, tag):
        if tag == self.open:
            text = " ".join("".join(self.buf).split())
            if tag == "td":
                self.cells.append(text)
            else:
                self.items.append([tag, text])
            self.open = None
        elif tag == "tr":
            self.items.append(["tr", "|".join(self.cells)])

    def handle_data(self, data):
        if self.open:
            self.buf.append(data)


def report_items(text):
    p = ReportItems()
    p.feed(text)
    p.close()
    return p.items


def reference_layout():
    from cae_tools.utils.html5.html5_builder import Html5Builder
    from cae_tools.utils.table_fragment import TableFragment
    builder = Html5Builder(language="en")
    builder.head().add_element("title").add_text("Model Evaluation")
    builder.body().add_element("h2", {"id": "heading"}).add_text("Model Metrics")
    for (label, key) in [("Test Metrics", "test"), ("Train Metrics", "train")]:
        builder.body().add_element("h3").add_text(label)
        tbl = TableFragment()
        tbl.add_row(["Metric Name", "Metric Value"])
        for (k, v) in RECORD["metrics"][key].items():
            tbl.add_row([k, f"{v:0.3f}"])
        builder.body().add_fragment(tbl)
    builder.body().add_element("h2", {"id": "heading"}).add_text("Model Evaluation Results")
    for partition in RECORD["partitions"]:
        builder.body().add_element("h3").add_text(partition)
        for _ in RECORD["measures"]:
            builder.body().add_element("img", {"src": "histogram"})
    builder.body().add_element("h2").add_text("Training Summary")
    builder.body().add_element("h2").add_text("Training Parameters")
    tbl = TableFragment()
    tbl.add_row(["Parameter Name", "Parameter Value"])
    tbl.add_row(["total epochs", str(RECORD["history"]["nr_epochs"])])
    for (k, v) in RECORD["parameters"].items():
        tbl.add_row([k, str(v)])
    builder.body().add_fragment(tbl)
    builder.body().add_element("img", {"src": "history"})
    return report_items(builder.get_html())


def reference_flags():
    origin = os.path.dirname(importlib.util.find_spec("cae_tools").origin)
    with open(os.path.join(origin, "cli", "evaluate_cae.py")) as f:
        tree = ast.parse(f.read())
    return [node.args[0].value for node in ast.walk(tree)
            if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument"]


if __name__ == "__main__":
    with open(os.path.join(HERE, "report_layout.json"), "w") as f:
        json.dump({"record": RECORD, "items": reference_layout()}, f, indent=1)
    with open(os.path.join(HERE, "evaluate_cae_flags.json"), "w") as f:
        json.dump(reference_flags(), f, indent=1)
    print("written report_layout.json, evaluate_cae_flags.json")
