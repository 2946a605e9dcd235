"""Novelty of the cases against a reference set, usually the training set: the host side of BaseModel.novelty
(cae_case_neighbours, include/cae_hip.h).  The per-case record from the neighbour lists, the summary of one partition against
the reference set's own leave-one-out novelty, and the writers: novelty_<partition>.json, the printed line, the rows of the
report's "Novelty of the cases" section and its bar chart of the mse per novelty quintile.  DESIGN.md section 9 holds the
definition.

Host only: standard library and numpy.  Everything here is arithmetic on per-case arrays.
"""
import math

import numpy as np

from . import records
from .records import shown as _shown
from .report import _B, _H, _L, _R, _T, _W, _scale, _svg

MAX_K = 32
PERCENTILES = (50, 90, 95, 99)
QUINTILES = 5
MOST_NOVEL = 10


def check_k(k):
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"novelty_k must be an integer from 1 to {MAX_K}, got {k!r}")
    return int(k)


def case_record(dist2, index, count, features, reference_cases, valid_reference_cases):
    """The per-case record of BaseModel.novelty from the lists of case_neighbours.  novelty = sqrt(dist2[:, k - 1] / D), the
    rms difference per feature to the k-th nearest reference: +inf with fewer than k valid references (the slot holds +inf),
    NaN for an invalid case (count -1).  nearest: the same formula on dist2[:, 0]; nearest_case: index[:, 0]."""
    dist2 = np.asarray(dist2, dtype=np.float64)
    index = np.asarray(index, dtype=np.int32)
    count = np.asarray(count, dtype=np.int32)
    features = int(features)
    invalid = count < 0
    with np.errstate(invalid="ignore", divide="ignore"):
        novelty = np.where(invalid, np.nan, np.sqrt(dist2[:, -1] / features))
        nearest = np.where(invalid, np.nan, np.sqrt(dist2[:, 0] / features))
    return {"novelty": novelty, "nearest": nearest, "nearest_case": index[:, 0].copy(), "index": index, "dist2": dist2,
            "count": count, "k": int(dist2.shape[1]), "features": features, "reference_cases": int(reference_cases),
            "valid_reference_cases": int(valid_reference_cases)}


def order_statistic(sorted_values, percent):
    """the exact order statistic of rank ceil(n percent / 100) (1-based, an element, no interpolation) of n ascending values;
    NaN without a value"""
    n = len(sorted_values)
    if n == 0:
        return float("nan")
    rank = max(1, -(-n * int(percent) // 100))
    return float(sorted_values[rank - 1])


def average_ranks(values):
    """the ranks 1 .. n of the values, ties sharing the average of their ranks"""
    v = np.asarray(values, dtype=np.float64)
    order = np.argsort(v, kind="stable")
    ranks = np.empty(v.size, dtype=np.float64)
    i = 0
    while i < v.size:
        j = i
        while j + 1 < v.size and v[order[j + 1]] == v[order[i]]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return ranks


def spearman(a, b):
    """Spearman's rank correlation over the pairs where both are finite, ties with average ranks: Pearson's correlation of
    the ranks.  NaN with fewer than 3 such pairs or where a rank variance is zero."""
    (a, b) = (np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    both = np.isfinite(a) & np.isfinite(b)
    if int(both.sum()) < 3:
        return float("nan")
    (ra, rb) = (average_ranks(a[both]), average_ranks(b[both]))
    (da, db) = (ra - ra.mean(), rb - rb.mean())
    den = float(np.sum(da * da)) * float(np.sum(db * db))
    if den <= 0.0:
        return float("nan")
    return float(np.sum(da * db)) / math.sqrt(den)


def _mean_finite(values):
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    return float(v.mean()) if v.size else float("nan")


def quintiles(novelty, mse, mae):
    """[{"cases", "novelty_lo", "novelty_hi", "mse", "mae"}] of the five bins: the valid cases (novelty not NaN) sorted by
    (novelty, case index), the bin of rank r of m being floor(5 r / m); mse and mae are means over the bin's finite values.
    An empty bin has 0 cases and NaN everywhere."""
    novelty = np.asarray(novelty, dtype=np.float64)
    valid = np.flatnonzero(~np.isnan(novelty))
    order = valid[np.lexsort((valid, novelty[valid]))]
    m = order.size
    bins = [[] for _ in range(QUINTILES)]
    for (rank, case) in enumerate(order):
        bins[QUINTILES * rank // m].append(int(case))
    found = []
    for cases in bins:
        if not cases:
            found.append({"cases": 0, "novelty_lo": float("nan"), "novelty_hi": float("nan"), "mse": float("nan"), "mae": float("nan")})
            continue
        found.append({"cases": len(cases), "novelty_lo": float(novelty[cases[0]]), "novelty_hi": float(novelty[cases[-1]]),
                      "mse": _mean_finite(np.asarray(mse, dtype=np.float64)[cases]) if mse is not None else float("nan"),
                      "mae": _mean_finite(np.asarray(mae, dtype=np.float64)[cases]) if mae is not None else float("nan")})
    return found


def summary(case, reference=None, mse=None, mae=None):
    """The record of one partition.  case: the case_record of the partition; reference: the case_record of the reference set
    searched against itself, leave-one-out (None: none is known), whose novelty gives the exact 50th, 90th, 95th and 99th
    order statistics (np.sort, rank ceil(n p / 100)); mse, mae: the per-case errors of the partition or None.  Holds the min,
    median and max of the novelty over the valid cases, the shares of the valid cases above the reference's 95th and 99th
    ("outside the training domain"), Spearman's rank correlation of novelty with the mse, the mean mse and mae per novelty
    quintile, the ratio of the top quintile's mse to the bottom one's, the ten most novel cases with their nearest
    reference cases, and the per-case novelty, nearest and nearest_case.  What has no value is NaN (null in JSON)."""
    novelty = np.asarray(case["novelty"], dtype=np.float64)
    valid = novelty[~np.isnan(novelty)]
    record = {"n_cases": int(novelty.size), "valid_cases": int(valid.size), "k": int(case["k"]), "features": int(case["features"]),
              "reference_cases": int(case["reference_cases"]), "valid_reference_cases": int(case["valid_reference_cases"]),
              "novelty_min": float(valid.min()) if valid.size else float("nan"),
              "novelty_median": float(np.median(valid)) if valid.size else float("nan"),
              "novelty_max": float(valid.max()) if valid.size else float("nan")}
    ref = {"n": 0, **{f"p{p}": float("nan") for p in PERCENTILES}}
    if reference is not None:
        rv = np.asarray(reference["novelty"], dtype=np.float64)
        rv = np.sort(rv[~np.isnan(rv)])
        ref = {"n": int(rv.size), **{f"p{p}": order_statistic(rv, p) for p in PERCENTILES}}
    record["reference"] = ref
    for p in (95, 99):
        bound = ref[f"p{p}"]
        record[f"outside_{p}"] = float(np.mean(valid > bound)) if valid.size and not math.isnan(bound) else float("nan")
    record["spearman_mse"] = spearman(novelty, mse) if mse is not None else float("nan")
    bins = quintiles(novelty, mse, mae)
    record["quintiles"] = bins
    (lo, hi) = (bins[0]["mse"], bins[-1]["mse"])
    record["top_bottom_mse_ratio"] = hi / lo if math.isfinite(hi) and math.isfinite(lo) and lo > 0.0 else float("nan")
    cases = np.flatnonzero(~np.isnan(novelty))
    most = cases[np.lexsort((cases, -novelty[cases]))][:MOST_NOVEL]
    record["most_novel"] = [{"case": int(c), "novelty": float(novelty[c]), "nearest": float(case["nearest"][c]),
                             "nearest_case": int(case["nearest_case"][c])} for c in most]
    record["case_novelty"] = novelty
    record["case_nearest"] = np.asarray(case["nearest"], dtype=np.float64)
    record["case_nearest_case"] = np.asarray(case["nearest_case"], dtype=np.int32)
    return record


def write_json(path, record):
    """novelty_<partition>.json: the record as strict JSON, a number that is not finite as null"""
    return records.write_json(path, records.json_record(record))


def line(partition, record):
    """novelty <partition>: <n> cases against <r> reference cases, k <k>, <D> features: median <m>, max <x>, outside p95 <s>,
    p99 <s>, spearman with mse <r>, top / bottom quintile mse <q>"""
    return (f"novelty {partition}: {record['n_cases']} cases against {record['valid_reference_cases']} reference cases, k {record['k']}, "
            f"{record['features']} features: median {_shown(record['novelty_median'])}, max {_shown(record['novelty_max'])}, "
            f"outside p95 {_shown(record['outside_95'])}, p99 {_shown(record['outside_99'])}, spearman with mse "
            f"{_shown(record['spearman_mse'])}, top / bottom quintile mse {_shown(record['top_bottom_mse_ratio'])}")


def heading(record):
    return (f"{record['valid_cases']} of {record['n_cases']} cases against {record['valid_reference_cases']} reference cases, "
            f"k {record['k']}, {record['features']} features")


def section_rows(record):
    """the rows of the report's table: the scores, then one row per novelty quintile"""
    ref = record["reference"]
    rows = [["Name", "Value"],
            ["novelty min / median / max", " / ".join(_shown(record[f"novelty_{k}"]) for k in ("min", "median", "max"))],
            ["reference p50 / p90 / p95 / p99", " / ".join(_shown(ref[f"p{p}"]) for p in PERCENTILES)],
            ["share above reference p95", _shown(record["outside_95"])],
            ["share above reference p99", _shown(record["outside_99"])],
            ["spearman of novelty with mse", _shown(record["spearman_mse"])],
            ["top / bottom quintile mse", _shown(record["top_bottom_mse_ratio"])]]
    for (q, b) in enumerate(record["quintiles"]):
        rows.append([f"quintile {q + 1}: {b['cases']} cases, novelty {_shown(b['novelty_lo'])} .. {_shown(b['novelty_hi'])}",
                     f"mse {_shown(b['mse'])}, mae {_shown(b['mae'])}"])
    return rows


def svg_quintiles(record, title):
    """The bar chart of a record: per novelty quintile with a finite mse one <rect class="quintile"> from 0 to its mean mse,
    carrying the quintile, its cases and the mse in data- attributes."""
    bins = [(q, b) for (q, b) in enumerate(record["quintiles"]) if math.isfinite(float(b["mse"]))]
    if not bins:
        return _svg(title, [], "novelty quintile", "mse", (1.0, float(QUINTILES)), (0.0, 1.0))
    top = max(max(float(b["mse"]) for (_, b) in bins), 0.0)
    if not top > 0.0:
        top = 1.0
    body = []
    for (q, b) in bins:
        xa = _scale(q + 0.15, 0.0, float(QUINTILES), _L, _W - _R)
        xb = _scale(q + 0.85, 0.0, float(QUINTILES), _L, _W - _R)
        y = _scale(float(b["mse"]), 0.0, top, _H - _B, _T)
        body.append(f'<rect class="quintile" data-quintile="{q + 1}" data-cases="{b["cases"]}" data-mse="{float(b["mse"]):.6g}" '
                    f'x="{xa:.2f}" y="{y:.2f}" width="{xb - xa:.2f}" height="{max((_H - _B) - y, 0.5):.2f}" fill="steelblue"/>')
    return _svg(title, body, "novelty quintile, least novel first", "mse", (1.0, float(QUINTILES)), (0.0, top))
