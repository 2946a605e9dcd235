"""Neighbourhood skill: the Fractions Skill Score (Roberts & Lean 2008) from the integer window sums of cae_case_fss
(case_ops.fraction_skill; include/cae_hip.h).

For a threshold and a neighbourhood width n the kernel gives, over the counted n x n windows of a case, {windows, S cM, S cO,
S cM^2, S cO^2, S cM cO} with cM and cO the window's numbers of prediction and target events.  With the fractions M = cM / n^2
and O = cO / n^2 the fractions Brier score is FBS = mean (M - O)^2 and FSS = 1 - FBS / (mean M^2 + mean O^2); n^4 and the number
of windows cancel, so

    FSS = 1 - (S cM^2 - 2 S cM cO + S cO^2) / (S cM^2 + S cO^2)          NaN without a denominator

f_O = S cO / (windows n^2) is the target's event frequency over the counted windows, f_M the prediction's, frequency_bias =
f_M / f_O.  A prediction is useful at a width when FSS >= fss_uniform = 0.5 + f_O / 2 (f_O at the smallest width);
skilful_width is the smallest such width.  FSS is formed per case, and pooled from the sums added over the cases in Python
integers: a case's sum stays below 2^63, the sum over thousands of cases need not.

Host only: standard library and numpy.
"""
import math
import os
from fractions import Fraction

import numpy as np

from . import records
from .records import shown as _shown
from .report import STYLE, Document, svg_data_uri, svg_lines

DEFAULT_WIDTHS = (1, 3, 5, 9, 17, 33, 65)
(MAX_THRESHOLDS, MAX_WIDTHS, MAX_WIDTH) = (8, 8, 129)
GAPS = {"strict": 0, "ignore": 1}       # gap_rule of cae_case_fss
SIDES = {"above": 0, "below": 1}        # "above": the event is v >= t; "below": v < t
SUMS = ("windows", "S cM", "S cO", "S cM^2", "S cO^2", "S cM cO")


def default_widths(h, w):
    """the DEFAULT_WIDTHS at or below min(h, w)"""
    return [n for n in DEFAULT_WIDTHS if n <= min(int(h), int(w))]


def check_widths(widths):
    """the widths as a list of ints: 1 to 8 odd, strictly ascending widths from 1 to 129, else ValueError"""
    try:
        found = [int(n) for n in widths]
        same = all(n == v for (n, v) in zip(found, widths))
    except (TypeError, ValueError):
        raise ValueError(f"widths must be integers, got {widths!r}") from None
    if (not same or not 1 <= len(found) <= MAX_WIDTHS or any(n < 1 or n > MAX_WIDTH or n % 2 == 0 for n in found)
            or any(b <= a for (a, b) in zip(found, found[1:]))):
        raise ValueError(f"1 to {MAX_WIDTHS} odd, strictly ascending widths from 1 to {MAX_WIDTH} expected, got {list(widths)!r}")
    return found


def check_thresholds(thresholds):
    """(values, sides) of 1 to 8 thresholds, each a finite number (the event is v >= t) or a (value, "above" | "below")
    pair; sides as the integers of SIDES.  Else ValueError"""
    try:
        items = list(thresholds)
    except TypeError:
        raise ValueError(f"thresholds must be a sequence, got {thresholds!r}") from None
    if not 1 <= len(items) <= MAX_THRESHOLDS:
        raise ValueError(f"1 to {MAX_THRESHOLDS} thresholds expected, got {len(items)}")
    (values, sides) = ([], [])
    for item in items:
        (value, side) = item if isinstance(item, (tuple, list)) and len(item) == 2 else (item, "above")
        try:
            value = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"a threshold must be a number or a (number, side) pair, got {item!r}") from None
        if not math.isfinite(value):
            raise ValueError(f"the thresholds must be finite, got {value!r}")
        if not isinstance(side, str) or side not in SIDES:
            raise ValueError(f"a threshold's side must be one of {', '.join(SIDES)}, got {side!r}")
        values.append(value)
        sides.append(SIDES[side])
    return values, sides


def _fss(mm, oo, mo):
    """1 - (mm - 2 mo + oo) / (mm + oo) of Python integers, each division correctly rounded; NaN without a denominator"""
    den = mm + oo
    return 1.0 - float(Fraction(mm - 2 * mo + oo, den)) if den else float("nan")


def _div(num, den):
    return float(Fraction(num, den)) if den else float("nan")


def scores_from_sums(sums, widths):
    """The scores of an (N, T, S, 6) array of window sums over the S widths: case_fss (N, T, S) float64; pooled_sums
    [T][S][6] Python integers, the sums added over the cases; fss, f_target, f_prediction and frequency_bias [T][S] from
    them; fss_uniform [T] = 0.5 + f_target / 2 at the smallest width; skilful_width [T], the smallest width whose pooled fss
    is at or above fss_uniform, None without one.  NaN where a score has no denominator."""
    sums = np.asarray(sums)
    widths = [int(n) for n in widths]
    if sums.ndim != 4 or sums.shape[3] != 6 or sums.shape[2] != len(widths) or sums.dtype.kind not in "iu":
        raise ValueError(f"scores_from_sums: integer sums of (N, T, {len(widths)}, 6) expected, got {sums.dtype} {sums.shape}")
    (n_case, n_thr, n_width) = sums.shape[:3]
    s = sums.astype(np.int64)
    # a case: every entry is below 2^57, so the three-term numerator and the denominator stay inside int64
    (mm, oo, mo) = (s[..., 3], s[..., 4], s[..., 5])
    case_fss = 1.0 - records.ratio(mm - 2 * mo + oo, mm + oo)
    pooled = [[[sum(int(v) for v in s[:, t, k, j]) for j in range(6)] for k in range(n_width)] for t in range(n_thr)]
    (fss, f_o, f_m, bias) = ([], [], [], [])
    for t in range(n_thr):
        rows = [(p, p[0] * widths[k] * widths[k]) for (k, p) in enumerate(pooled[t])]
        fss.append([_fss(p[3], p[4], p[5]) for (p, _) in rows])
        f_o.append([_div(p[2], area) for (p, area) in rows])
        f_m.append([_div(p[1], area) for (p, area) in rows])
        bias.append([_div(p[1], p[2]) for (p, _) in rows])
    uniform = [0.5 + 0.5 * f_o[t][0] if n_width else float("nan") for t in range(n_thr)]
    skilful = []
    for t in range(n_thr):
        found = [widths[k] for k in range(n_width) if math.isfinite(uniform[t]) and fss[t][k] >= uniform[t]]
        skilful.append(found[0] if found else None)
    return {"n_cases": int(n_case), "case_fss": case_fss, "pooled_sums": pooled, "fss": fss, "f_target": f_o, "f_prediction": f_m,
            "frequency_bias": bias, "fss_uniform": uniform, "skilful_width": skilful}


def label(value, side, percentile=None):
    """a threshold as the line, the table and the plots name it: ">=q90", "<q5", ">=291.5" """
    what = f"q{100.0 * float(percentile):g}" if percentile is not None else f"{float(value):.6g}"
    return (">=" if side == "above" else "<") + what


def summary(scores, thresholds, widths, gaps, h, w, percentiles=None):
    """the scores with what names them: thresholds as check_thresholds takes them (with the percentile of the target's
    distribution a value was taken at, where it was), the widths, the gap rule and the shape of the plane"""
    (values, sides) = check_thresholds(thresholds)
    names = [name for side in sides for (name, k) in SIDES.items() if k == side]
    percentiles = list(percentiles) if percentiles is not None else [None] * len(values)
    if len(values) != len(scores["fss"]) or len(percentiles) != len(values) or any(len(row) != len(widths) for row in scores["fss"]):
        raise ValueError(f"summary: {len(values)} thresholds and {len(widths)} widths do not belong to these scores")
    if gaps not in GAPS:
        raise ValueError(f"summary: gaps must be one of {', '.join(GAPS)}, got {gaps!r}")
    return {"thresholds": [{"value": v, "side": s, "percentile": None if q is None else float(q), "label": label(v, s, q)}
                           for (v, s, q) in zip(values, names, percentiles)],
            "widths": [int(n) for n in widths], "gaps": gaps, "h": int(h), "w": int(w), "sums": list(SUMS), **scores}


def write_json(path, record):
    """fss_<partition>.json: the record as strict JSON, a score that is not finite as null; the pooled sums as integers of
    any size"""
    return records.write_json(path, records.json_record(record))


def line(partition, record):
    """fss <partition>: <n> cases, widths <first>..<last> (<gaps>), skilful width <label> <n|none>[, <label> <n|none> ...]"""
    widths = record["widths"]
    span = f"{widths[0]}..{widths[-1]}" if widths else "none"
    found = ", ".join(f"{thr['label']} {'none' if n is None else n}" for (thr, n) in zip(record["thresholds"], record["skilful_width"]))
    return f"fss {partition}: {record['n_cases']} cases, widths {span} ({record['gaps']}), skilful width {found}"


def section_rows(record):
    """the rows of the report's table: a header and one row per threshold with its value, the target's event frequency and
    the frequency bias at the smallest width, the uniform FSS, the skilful width and the pooled FSS of every width; "none" for
    a score that does not exist"""
    rows = [["Threshold", "value", "target frequency", "frequency bias", "uniform FSS", "skilful width"]
            + [f"FSS n = {n}" for n in record["widths"]]]
    for (t, thr) in enumerate(record["thresholds"]):
        first = lambda key: _shown(record[key][t][0]) if record["widths"] else "none"      # noqa: E731
        width = record["skilful_width"][t]
        rows.append([thr["label"], _shown(thr["value"]), first("f_target"), first("frequency_bias"), _shown(record["fss_uniform"][t]),
                     "none" if width is None else str(width)] + [_shown(v) for v in record["fss"][t]])
    return rows


def svg_curve(record, t, title):
    """the pooled FSS of threshold t against the width, with the level fss_uniform as a second series"""
    widths = record["widths"]
    nan = float("nan")
    number = lambda v: nan if v is None else float(v)      # noqa: E731
    return svg_lines({record["thresholds"][t]["label"]: (widths, [number(v) for v in record["fss"][t]]),
                      "uniform": (widths, [number(record["fss_uniform"][t])] * len(widths))},
                     title, "neighbourhood width (pixels)", "FSS")


def write_page(folder, partitions):
    """<folder>/index.html.  partitions: [(partition, record)] in page order.  Per partition the table of section_rows and
    one line plot per threshold: the pooled FSS against the width and the level fss_uniform."""
    os.makedirs(folder, exist_ok=True)
    doc = Document("Neighbourhood skill")
    doc.head.add("style").text(STYLE)
    body = doc.body
    body.add("h2").text("Fractions Skill Score of prediction against target")
    body.add("p").text("Channel 0; event fractions in n x n windows that lie wholly inside the image, pooled over the cases. "
                       "The placement of the events is useful from the width at which the curve passes the uniform level.")
    for (partition, record) in partitions:
        section = body.add("div", {"class": "fss", "data-partition": partition})
        section.add("h3").text(f"{partition}: {record['n_cases']} cases of {record['h']} x {record['w']}, gaps {record['gaps']}")
        section.table(section_rows(record))
        for (t, thr) in enumerate(record["thresholds"]):
            section.add("img", {"src": svg_data_uri(svg_curve(record, t, f"{partition} FSS {thr['label']}")),
                                "alt": f"{partition} fss {thr['label']}"})
    path = os.path.join(folder, "index.html")
    with open(path, "w") as f:
        f.write(doc.html())
    return path
