"""Models compared on the same pixels, with bootstrap intervals: the host side of case_ops.case_compare and
case_ops.bootstrap_sums (cae_case_compare and cae_bootstrap_sums, include/cae_hip.h).  The settings and their refusals, the
resampling units, the statistics of a table of sums and of its resamples, the interval ranks, and the writers:
compare_<partition>.json, the printed line, the rows of the report's "Model comparison" section and its bar chart of the mse
with interval whiskers.  DESIGN.md section 9 holds the definitions.

Host only: standard library and numpy.
"""
import html
import math
from fractions import Fraction

import numpy as np

from . import conformal, records
from .records import shown as _shown
from .report import _B, _H, _L, _R, _T, _W, _scale, _svg

MAX_CANDIDATES = 8
MAX_RESAMPLES = 10 ** 6
MAX_UNITS = 1 << 20
MAX_COLUMNS = 32            # of a table cae_bootstrap_sums takes; a wider one goes in column pieces with the same seed
DEFAULT_RESAMPLES = 10000
DEFAULT_CONFIDENCE = "0.95"
CANDIDATE_STATS = ("mse", "rmse", "mae", "bias")


# ---- the settings --------------------------------------------------------------------------------------------------------

def parse_confidence(text):
    """the confidence of the intervals as the exact Fraction of its text (conformal.parse_level's rule: 0 < c < 1, never
    through a float)"""
    try:
        return conformal.parse_level(text)
    except ValueError as refused:
        raise ValueError(f"compare_confidence: {refused}") from None


def check_resamples(resamples):
    if isinstance(resamples, bool) or int(resamples) != resamples or not 1 <= int(resamples) <= MAX_RESAMPLES:
        raise ValueError(f"compare_resamples must be an integer from 1 to {MAX_RESAMPLES}, got {resamples!r}")
    return int(resamples)


def check_seed(seed):
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"compare_seed must be an integer from 0 to 2^64 - 1, got {seed!r}")
    return int(seed)


def check_candidates(prediction_variable, variables, labels=None):
    """(variables, labels) of the candidates P_0 .. P_{M-1}: the evaluator's prediction variable, then the compare_variables.
    labels: None (the variables' names), or one label per candidate, P_0 included."""
    names = [str(prediction_variable)] + [str(v) for v in (variables or [])]
    if len(names) > MAX_CANDIDATES:
        raise ValueError(f"compare_variables: at most {MAX_CANDIDATES - 1} variables beside the prediction expected, got {len(names) - 1}")
    twice = [v for v in names if names.count(v) > 1]
    if twice:
        raise ValueError(f"compare_variables: {twice[0]!r} is named twice (the prediction variable is the first candidate)")
    if labels is None:
        return names, list(names)
    labels = [str(v) for v in labels]
    if len(labels) != len(names):
        raise ValueError(f"compare_labels: {len(names)} labels expected, one per candidate with the prediction first, got {len(labels)}")
    if len(set(labels)) != len(labels):
        raise ValueError("compare_labels: the labels must differ")
    return names, labels


def interval_ranks(n, confidence):
    """(k, n + 1 - k), the 1-based ranks of the two order statistics among n finite values that bound the interval at
    `confidence` (a Fraction): k = ceil(n (1 - c) / 2) in integers.  k < 1 is refused: too few resamples."""
    tail = (1 - Fraction(confidence)) / 2
    k = (int(n) * tail.numerator + tail.denominator - 1) // tail.denominator
    if k < 1:
        raise ValueError(f"too few resamples for this confidence: {int(n)} finite values at {conformal.level_text(Fraction(confidence))}")
    return k, int(n) + 1 - k


# ---- the units -----------------------------------------------------------------------------------------------------------

def units(rows, block=None):
    """The table of the resampling units from the per-case rows (N, n_col): the rows themselves, or with block - one value
    per case - the rows of the cases of equal value added in ascending case order in fp64, the units ordered by first
    appearance (values that are NaN form one unit).  Returns (table (n_unit, n_col) float64, index (N,) int64, the unit of
    every case)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2:
        raise ValueError(f"units: per-case rows (N, n_col) expected, got {rows.shape}")
    if block is None:
        return rows.copy(), np.arange(rows.shape[0], dtype=np.int64)
    block = np.asarray(block).reshape(-1)
    if block.shape[0] != rows.shape[0]:
        raise ValueError(f"units: one block value per case expected, got {block.shape[0]} for {rows.shape[0]} cases")
    (first, index) = ({}, np.empty(rows.shape[0], dtype=np.int64))
    for (i, v) in enumerate(block.tolist()):
        key = None if isinstance(v, float) and v != v else v
        index[i] = first.setdefault(key, len(first))
    table = np.zeros((len(first), rows.shape[1]), dtype=np.float64)
    for i in range(rows.shape[0]):
        table[index[i]] = table[index[i]] + rows[i]
    return table, index


def column_sums(table):
    """the column sums of a table in ascending unit order, plain fp64 adds"""
    table = np.asarray(table, dtype=np.float64)
    return np.cumsum(table, axis=0)[-1] if table.shape[0] else np.zeros(table.shape[1], dtype=np.float64)


# ---- the statistics ------------------------------------------------------------------------------------------------------

def statistics(sums):
    """The statistics of (..., 2 + 4 M) sums {n, tied, (S e, S|e|, S e^2, wins) per candidate}, one number per leading index:
    {"mse", "rmse", "mae", "bias", "win_share": (..., M); "delta_mse", "skill": (..., M) with column 0 unused (0);
    "tied_share": (...)}.  delta_mse_m = mse_m - mse_0, skill_m = 1 - mse_0 / mse_m: above 0 means candidate 0 is better.
    What has no denominator is NaN."""
    sums = np.asarray(sums, dtype=np.float64)
    m = (sums.shape[-1] - 2) // 4
    if sums.shape[-1] != 2 + 4 * m or m < 1:
        raise ValueError(f"statistics: rows of 2 + 4 M sums expected, got {sums.shape}")
    n = sums[..., :1]
    per = sums[..., 2:].reshape(sums.shape[:-1] + (m, 4))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mse = records.ratio(per[..., 2], n)
        found = {"mse": mse, "rmse": np.sqrt(mse), "mae": records.ratio(per[..., 1], n), "bias": records.ratio(per[..., 0], n),
                 "win_share": records.ratio(per[..., 3], n), "tied_share": records.ratio(sums[..., 1], sums[..., 0]),
                 "delta_mse": mse - mse[..., :1], "skill": 1.0 - records.ratio(mse[..., :1], mse)}
    return found


def _stat(point, values, confidence):
    """{"value", "interval": [lo, hi], "degenerate"}: the point value, the order statistics of interval_ranks among the finite
    resampled values (NaN without one), the number of resamples left out because their value is not finite"""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    kept = np.sort(values[np.isfinite(values)])
    interval = [float("nan"), float("nan")]
    if kept.size:
        (k, upper) = interval_ranks(kept.size, confidence)
        interval = [float(kept[k - 1]), float(kept[upper - 1])]
    return {"value": float(point), "interval": interval, "degenerate": int(values.size - kept.size)}


def _excludes_zero(stat):
    (lo, hi) = stat["interval"]
    return bool(lo == lo and hi == hi and (lo > 0.0 or hi < 0.0))


def baseline_summary(table, resampled, confidence, mode, variable):
    """the skill against interpolation with its interval, from the units' cae_case_baseline sums {n, S|b - a|, S(b - a)^2,
    S|p - a|, S(p - a)^2, n_won} and their resamples (the same seed: the same units)"""
    def stats(s):
        s = np.asarray(s, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return {"baseline_mse": records.ratio(s[..., 2], s[..., 0]), "model_mse": records.ratio(s[..., 4], s[..., 0]),
                    "skill": 1.0 - records.ratio(s[..., 4], s[..., 2])}
    (point, boot) = (stats(column_sums(table)), stats(resampled))
    found = {"mode": str(mode), "variable": str(variable), "label": f"interpolation of {variable}",
             "pixels_counted": int(column_sums(table)[0])}
    for key in ("skill", "baseline_mse", "model_mse"):
        found[key] = _stat(point[key], boot[key], confidence)
    found["significant"] = _excludes_zero(found["skill"])
    return found


def summary(table, resampled, variables, labels, confidence, resamples, seed, n_cases, plane, block_variable=None, baseline=None):
    """One partition's record.  table (n_unit, 2 + 4 M): the units' sums; resampled (B, 2 + 4 M): cae_bootstrap_sums of it;
    variables, labels: of the M candidates, the evaluator's prediction first; confidence: a Fraction.  The point values come
    from the table's column sums in ascending unit order, the intervals from the resamples by interval_ranks; a resample
    whose statistic is not finite is left out and counted in "degenerate".  Per candidate mse, rmse, mae, bias (each {value,
    interval, degenerate}) and win_share; per competitor m >= 1 delta_mse = mse_m - mse_0 and skill = 1 - mse_0 / mse_m
    likewise, p_better (the share of the resamples with mse_m > mse_0), significant (the interval of delta_mse excludes 0),
    win_share, reference_win_share and tied_share."""
    table = np.asarray(table, dtype=np.float64)
    resampled = np.asarray(resampled, dtype=np.float64)
    m = len(variables)
    if table.ndim != 2 or table.shape[1] != 2 + 4 * m or resampled.ndim != 2 or resampled.shape[1] != table.shape[1]:
        raise ValueError(f"compare.summary: a table (n_unit, {2 + 4 * m}) and resamples (B, {2 + 4 * m}) expected, got {table.shape} "
                         f"and {resampled.shape}")
    total = column_sums(table)
    (point, boot) = (statistics(total), statistics(resampled))
    record = {"variables": list(variables), "labels": list(labels), "resamples": int(resamples), "seed": int(seed),
              "confidence": conformal.level_text(Fraction(confidence)), "block_variable": block_variable,
              "n_cases": int(n_cases), "n_unit": int(table.shape[0]), "pixels_counted": int(total[0]),
              "pixels_left_out": int(n_cases) * int(plane) - int(total[0]), "pixels_tied": int(total[1]),
              "tied_share": float(point["tied_share"]), "candidates": [], "competitors": [], "baseline": baseline}
    for k in range(m):
        cand = {"variable": variables[k], "label": labels[k], "win_share": float(point["win_share"][k])}
        for key in CANDIDATE_STATS:
            cand[key] = _stat(point[key][k], boot[key][:, k], confidence)
        record["candidates"].append(cand)
    for k in range(1, m):
        delta = boot["delta_mse"][:, k]
        finite = delta[np.isfinite(delta)]
        comp = {"variable": variables[k], "label": labels[k],
                "delta_mse": _stat(point["delta_mse"][k], delta, confidence),
                "skill": _stat(point["skill"][k], boot["skill"][:, k], confidence),
                "p_better": float(np.sum(finite > 0.0)) / float(finite.size) if finite.size else float("nan"),
                "win_share": float(point["win_share"][k]), "reference_win_share": float(point["win_share"][0]),
                "tied_share": float(point["tied_share"])}
        comp["significant"] = _excludes_zero(comp["delta_mse"])
        record["competitors"].append(comp)
    return record


# ---- the writers ---------------------------------------------------------------------------------------------------------

def write_json(path, record):
    """compare_<partition>.json: the record as strict JSON, a value that is not finite as null"""
    return records.write_json(path, records.json_record(record, (dict, list, tuple)))


def _interval(stat):
    return f"[{_shown(stat['interval'][0])}, {_shown(stat['interval'][1])}]"


def line(partition, record):
    """compare <partition>: <M> candidates, <U> units x <B> resamples at <c>: <label0> mse <x> [lo, hi]; <label> delta <d>
    [lo, hi] (significant | not significant), ..."""
    first = record["candidates"][0]
    parts = [f"{first['label']} mse {_shown(first['mse']['value'])} {_interval(first['mse'])}"]
    for comp in record["competitors"]:
        parts.append(f"{comp['label']} delta {_shown(comp['delta_mse']['value'])} {_interval(comp['delta_mse'])} "
                     f"({'significant' if comp['significant'] else 'not significant'})")
    if record.get("baseline"):
        base = record["baseline"]
        parts.append(f"skill against {base['label']} {_shown(base['skill']['value'])} {_interval(base['skill'])}")
    return (f"compare {partition}: {len(record['candidates'])} candidate{'s' if len(record['candidates']) != 1 else ''}, "
            f"{record['n_unit']} units x {record['resamples']} resamples at {record['confidence']}: " + "; ".join(parts))


def heading(record):
    return (f"{len(record['candidates'])} candidate{'s' if len(record['candidates']) != 1 else ''} on {record['pixels_counted']} common "
            f"pixels, {record['n_unit']} units x {record['resamples']} resamples, confidence {record['confidence']}, seed {record['seed']}")


def section_rows(record):
    """the rows of the report's table: a header, one row per candidate, and one for the interpolation where it was asked for"""
    rows = [["Candidate", "mse", "interval", "rmse", "mae", "bias", "delta mse", "interval", "skill", "interval", "p better",
             "significant", "pixels won"]]
    by_label = {comp["label"]: comp for comp in record["competitors"]}
    for cand in record["candidates"]:
        comp = by_label.get(cand["label"]) if cand is not record["candidates"][0] else None
        rows.append([cand["label"], _shown(cand["mse"]["value"]), _interval(cand["mse"]), _shown(cand["rmse"]["value"]),
                     _shown(cand["mae"]["value"]), _shown(cand["bias"]["value"])]
                    + ([_shown(comp["delta_mse"]["value"]), _interval(comp["delta_mse"]), _shown(comp["skill"]["value"]),
                        _interval(comp["skill"]), _shown(comp["p_better"]), "yes" if comp["significant"] else "no"]
                       if comp else ["", "", "", "", "", ""]) + [_shown(cand["win_share"])])
    if record.get("baseline"):
        base = record["baseline"]
        rows.append([base["label"], _shown(base["baseline_mse"]["value"]), _interval(base["baseline_mse"]), "", "", "", "", "",
                     _shown(base["skill"]["value"]), _interval(base["skill"]), "", "yes" if base["significant"] else "no", ""])
    return rows


def svg_bars(record, title):
    """The bar chart of a record: per candidate with a finite mse one <rect class="candidate"> from 0 to its mse, carrying
    label, mse and the interval in data- attributes, and where the interval exists a whisker <line class="interval"> over it."""
    cands = [c for c in record["candidates"] if c["mse"]["value"] is not None and math.isfinite(float(c["mse"]["value"]))]
    n = len(cands)
    if not cands:
        return _svg(title, [], "candidate", "mse", (0.0, 1.0), (0.0, 1.0))
    spans = []
    for c in cands:
        (lo, hi) = c["mse"]["interval"]
        spans.append((float(lo), float(hi)) if lo is not None and hi is not None and math.isfinite(float(lo)) and math.isfinite(float(hi))
                     else None)
    y1 = max(max(float(c["mse"]["value"]) for c in cands), max((s[1] for s in spans if s), default=0.0))
    (y0, y1) = (0.0, y1 if y1 > 0.0 else 1.0)
    at = lambda v: _scale(v, y0, y1, _H - _B, _T)       # noqa: E731
    body = []
    for (k, (c, s)) in enumerate(zip(cands, spans)):
        v = float(c["mse"]["value"])
        xa = _scale(k + 0.15, 0.0, float(n), _L, _W - _R)
        xb = _scale(k + 0.85, 0.0, float(n), _L, _W - _R)
        (lo, hi) = s if s else (v, v)
        body.append(f'<rect class="candidate" data-label="{html.escape(c["label"], quote=True)}" data-mse="{v:.6g}" data-lo="{lo:.6g}" '
                    f'data-hi="{hi:.6g}" x="{xa:.2f}" y="{at(v):.2f}" width="{xb - xa:.2f}" height="{max(at(0.0) - at(v), 0.5):.2f}" '
                    'fill="steelblue"/>')
        xm = 0.5 * (xa + xb)
        if s:
            body.append(f'<line class="interval" x1="{xm:.2f}" y1="{at(lo):.2f}" x2="{xm:.2f}" y2="{at(hi):.2f}" stroke="black"/>')
        body.append(f'<text x="{xm:.2f}" y="{_H - _B + 30}" text-anchor="middle" font-size="10">{html.escape(c["label"])}</text>')
    return _svg(title, body, "candidate", "mse", (0.0, float(max(n - 1, 1))), (y0, y1))
