"""Skill by stratum: the host side of engine.strata_sums (cae_strata_sums, include/cae_hip.h).  The edges of the strata from a
list of classes or a count of equal bins, their labels, the scores of every stratum and of all of them pooled from the
counts and the eight sums, and the writers: strata_<partition>.json, the printed line, the rows of the report's "Skill by
stratum" section and its bar chart of bias +- rmse.  DESIGN.md section 9 holds the mapping and the stratum rule.

Host only: standard library and numpy.
"""
import html
import math

import numpy as np

from . import records
from .records import ratio as _ratio, shown as _shown
from .report import _B, _H, _L, _R, _T, _W, _scale, _svg

MAX_STRATA = 64
SCORES = ("mean_target", "mean_prediction", "bias", "mae", "rmse", "correlation", "sd_ratio")


def edges_from_classes(values):
    """(edges, labels) of a categorical stratifier: the sorted distinct values listed, an edge midway between neighbours - a
    value that is not listed counts to the nearest listed class, the upper one where it lies midway - and the labels "= v" """
    v = np.unique(np.asarray(values, dtype=np.float64).reshape(-1))
    if v.size == 0 or not np.isfinite(v).all():
        raise ValueError(f"strata classes must be finite numbers, at least one, got {values!r}")
    return (0.5 * v[:-1] + 0.5 * v[1:]).tolist(), [f"= {_shown(x)}" for x in v]


def edges_from_count(lo, hi, n):
    """the n - 1 inner edges of n equal bins over [lo, hi]; no edge, one stratum, where the range is degenerate"""
    (lo, hi, n) = (float(lo), float(hi), int(n))
    if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(hi - lo) and hi > lo) or n < 2:
        return []
    edges = [lo + (hi - lo) * (k / n) for k in range(1, n)]
    return edges if all(b > a for (a, b) in zip(edges, edges[1:])) else []


def labels(edges):
    """"< e0", "[e0, e1)", ..., ">= e_last"; "all" without an edge"""
    e = [_shown(x) for x in edges]
    if not e:
        return ["all"]
    return [f"< {e[0]}"] + [f"[{a}, {b})" for (a, b) in zip(e, e[1:])] + [f">= {e[-1]}"]


def check_edges(edges):
    """the edges as a list of floats; ValueError unless they are finite, strictly ascending and at most 63"""
    e = [float(x) for x in np.asarray(edges, dtype=np.float64).reshape(-1)]
    if not all(math.isfinite(x) for x in e) or not all(b > a for (a, b) in zip(e, e[1:])):
        raise ValueError(f"strata_edges must be finite and strictly ascending, got {e}")
    if len(e) + 1 > MAX_STRATA:
        raise ValueError(f"at most {MAX_STRATA} strata expected, got {len(e) + 1}")
    return e


def stratum_means(counts, sums, shift=0.0):
    """(2, n_strata): the mean of a and of p over a stratum's pairs, from sums about `shift` (a number or (2, n_strata));
    `shift` itself where a stratum has no pair.  As the shifts of a second strata_sums call they centre its second moments."""
    s = np.asarray(sums, dtype=np.float64)
    n = np.asarray(counts["pairs"], dtype=np.float64)
    shift = np.broadcast_to(np.asarray(shift, dtype=np.float64), (2, s.shape[0]))
    means = shift + np.stack([_ratio(s[:, 3], n), _ratio(s[:, 4], n)])
    return np.where(n > 0, means, shift)


def _moments(n, sa, sp, saa, spp, sap):
    """(correlation, sd_ratio) from the count and the five sums about shifts near the means; NaN below two pairs and where
    a variance is no larger than its own rounding (utils/skill_maps.maps_from_sums has the rule)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        nn = np.where(n > 0, n, np.nan)
        va = saa - sa * sa / nn
        vp = spp - sp * sp / nn
        cov = sap - sa * sp / nn
        noise = 8.0 * n * 2.0 ** -53
        ok_a = (n >= 2) & (va > noise * saa)
        ok_p = (n >= 2) & (vp > noise * spp)
        return (np.where(ok_a & ok_p, cov / np.sqrt(va * vp), np.nan),
                np.where(ok_a, np.sqrt(np.where(vp > noise * spp, vp, 0.0) / va), np.nan))


def scores_from_sums(counts, sums, centred=None, shift=0.0, centred_shift=None):
    """The scores per stratum and pooled from engine.strata_sums' (counts, sums (n_strata, 8)) about `shift`, as a dict:
        n_strata, pixels (members + unclassified), unclassified
        members, pairs, share (pairs over all pairs), mse_share (S d^2 over the S d^2 of all strata)       per stratum
        mean_target = shift_a + S a' / n, mean_prediction likewise, bias = S d / n, mae = S|d| / n, rmse = sqrt(S d^2 / n),
        correlation = cov / sqrt(va vp), sd_ratio = sqrt(vp / va)                                          per stratum
        pooled: the same names over the pairs of all strata
    centred: the sums of a second pass about centred_shift (2, n_strata), the strata's own means (stratum_means): the
    variances and the covariance are then taken from them - the two-pass scheme of utils/skill_maps.py.  The pooled moments
    are the strata's, moved to the pooled means: S (a - M)^2 = S_k [S a'^2 + 2 (c_k - M) S a' + n_k (c_k - M)^2].
    A stratum without pairs has NaN scores."""
    s = np.asarray(sums, dtype=np.float64)
    if s.ndim != 2 or s.shape[1] != 8:
        raise ValueError(f"scores_from_sums: (n_strata, 8) sums expected, got shape {s.shape}")
    n_strata = s.shape[0]
    members = np.asarray(counts["members"], dtype=np.int64).reshape(-1)
    pairs = np.asarray(counts["pairs"], dtype=np.int64).reshape(-1)
    if members.shape != (n_strata,) or pairs.shape != (n_strata,):
        raise ValueError(f"scores_from_sums: counts of {n_strata} strata expected, got {members.shape} and {pairs.shape}")
    n = pairs.astype(np.float64)
    shift = np.broadcast_to(np.asarray(shift, dtype=np.float64), (2, n_strata))
    if centred is None:
        (c, cs) = (s, shift)
    else:
        c = np.asarray(centred, dtype=np.float64)
        cs = np.broadcast_to(np.asarray(shift if centred_shift is None else centred_shift, dtype=np.float64), (2, n_strata))
        if c.shape != s.shape:
            raise ValueError(f"scores_from_sums: centred sums of shape {s.shape} expected, got {c.shape}")
    means = np.where(n > 0, shift + np.stack([_ratio(s[:, 3], n), _ratio(s[:, 4], n)]), np.nan)
    (corr, sdr) = _moments(n, c[:, 3], c[:, 4], c[:, 5], c[:, 6], c[:, 7])
    total = int(pairs.sum())
    have = pairs > 0
    sdd = float(s[have, 2].sum())
    record = {"n_strata": n_strata, "pixels": int(members.sum()) + int(counts["unclassified"]),
              "unclassified": int(counts["unclassified"]), "members": members.tolist(), "pairs": pairs.tolist(),
              "share": _ratio(n, np.full(n_strata, float(total))).tolist(),
              "mse_share": np.where(have, _ratio(s[:, 2], np.full(n_strata, sdd)), np.nan).tolist(),
              "mean_target": means[0].tolist(), "mean_prediction": means[1].tolist(),
              "bias": _ratio(s[:, 0], n).tolist(), "mae": _ratio(s[:, 1], n).tolist(),
              "rmse": np.sqrt(_ratio(s[:, 2], n)).tolist(), "correlation": corr.tolist(), "sd_ratio": sdr.tolist()}
    pooled = {"members": int(members.sum()), "pairs": total}
    if total:
        w = n[have] / total
        (ma, mp) = (float(np.sum(w * means[0, have])), float(np.sum(w * means[1, have])))
        (da, dp) = (cs[0, have] - ma, cs[1, have] - mp)
        (k, ca) = (n[have], c[have])
        saa = float(np.sum(ca[:, 5] + 2.0 * da * ca[:, 3] + k * da * da))
        spp = float(np.sum(ca[:, 6] + 2.0 * dp * ca[:, 4] + k * dp * dp))
        sap = float(np.sum(ca[:, 7] + dp * ca[:, 3] + da * ca[:, 4] + k * da * dp))
        (sa, sp) = (float(np.sum(ca[:, 3] + k * da)), float(np.sum(ca[:, 4] + k * dp)))
        (pc, ps) = _moments(np.float64(total), np.float64(sa), np.float64(sp), np.float64(saa), np.float64(spp), np.float64(sap))
        pooled.update({"mean_target": ma, "mean_prediction": mp, "bias": float(s[have, 0].sum()) / total,
                       "mae": float(s[have, 1].sum()) / total, "rmse": math.sqrt(sdd / total), "correlation": float(pc),
                       "sd_ratio": float(ps)})
    else:
        pooled.update({name: float("nan") for name in SCORES})
    record["pooled"] = pooled
    return record


def summary(scores, variable, channel, edges, names=None, in_shape=None, out_shape=None):
    """the scores with what names them: the stratifier variable and channel, the edges, the labels of the strata and the
    shapes of the stratifier's plane and of the target's"""
    edges = [float(e) for e in edges]
    names = list(names) if names is not None else labels(edges)
    if len(names) != scores["n_strata"] or len(edges) + 1 != scores["n_strata"]:
        raise ValueError(f"summary: {scores['n_strata']} strata, {len(edges)} edges and {len(names)} labels do not belong together")
    return {"variable": variable, "channel": int(channel), "edges": edges, "labels": names,
            "in_shape": None if in_shape is None else [int(v) for v in in_shape],
            "out_shape": None if out_shape is None else [int(v) for v in out_shape], **scores}


def write_json(path, record):
    """strata_<partition>.json: the record as strict JSON, a score that is not finite as null"""
    return records.write_json(path, records.json_record(record, (dict, list, tuple)))


def _extremes(record):
    """((rmse, label) of the stratum with the lowest rmse, of the one with the highest); (NaN, "none") twice without one"""
    found = [(float(r), name) for (r, name) in zip(record["rmse"], record["labels"]) if r is not None and math.isfinite(float(r))]
    if not found:
        return (float("nan"), "none"), (float("nan"), "none")
    return min(found, key=lambda f: f[0]), max(found, key=lambda f: f[0])


def line(partition, record):
    """strata <partition>: <variable>, <n> strata, rmse <lowest> (<label>) .. <highest> (<label>), unclassified <count>"""
    (low, high) = _extremes(record)
    return (f"strata {partition}: {record['variable']}, {record['n_strata']} strata, rmse {_shown(low[0])} ({low[1]}) .. "
            f"{_shown(high[0])} ({high[1]}), unclassified {record['unclassified']}")


COLUMNS = (("mean target", "mean_target"), ("bias", "bias"), ("mae", "mae"), ("rmse", "rmse"), ("correlation", "correlation"),
           ("sd ratio", "sd_ratio"))


def section_rows(record):
    """the rows of the report's table: a header, one row per stratum and the pooled row; "none" for a score that does not exist"""
    rows = [["Stratum", "pixels", "pairs", "share"] + [title for (title, _) in COLUMNS] + ["share of the squared error"]]
    for k in range(record["n_strata"]):
        rows.append([record["labels"][k], str(record["members"][k]), str(record["pairs"][k]), _shown(record["share"][k])]
                    + [_shown(record[key][k]) for (_, key) in COLUMNS] + [_shown(record["mse_share"][k])])
    pooled = record["pooled"]
    rows.append(["all strata", str(pooled["members"]), str(pooled["pairs"]), _shown(1.0 if pooled["pairs"] else None)]
                + [_shown(pooled[key]) for (_, key) in COLUMNS] + [_shown(1.0 if pooled["pairs"] else None)])
    return rows


def svg_bars(record, title):
    """The bar chart of a record: per stratum with pairs one <rect class="stratum"> from 0 to its bias, carrying label,
    bias and rmse in data- attributes, and a whisker <line class="spread"> over bias - rmse .. bias + rmse; the zero line
    dashed."""
    n = record["n_strata"]
    bars = []
    for k in range(n):
        (b, r) = (record["bias"][k], record["rmse"][k])
        if b is not None and r is not None and math.isfinite(float(b)) and math.isfinite(float(r)):
            bars.append((k, float(b), float(r)))
    if not bars:
        return _svg(title, [], "stratum", "prediction - target", (0.0, float(max(n - 1, 1))), (0.0, 1.0))
    (y0, y1) = (min(0.0, min(b - r for (_, b, r) in bars)), max(0.0, max(b + r for (_, b, r) in bars)))
    if not y1 > y0:
        (y0, y1) = (y0 - 0.5, y1 + 0.5)
    at = lambda v: _scale(v, y0, y1, _H - _B, _T)       # noqa: E731
    body = []
    for (k, b, r) in bars:
        xa = _scale(k + 0.15, 0.0, float(n), _L, _W - _R)
        xb = _scale(k + 0.85, 0.0, float(n), _L, _W - _R)
        (top, bottom) = (min(at(b), at(0.0)), max(at(b), at(0.0)))
        body.append(f'<rect class="stratum" data-label="{html.escape(record["labels"][k], quote=True)}" data-bias="{b:.6g}" '
                    f'data-rmse="{r:.6g}" x="{xa:.2f}" y="{top:.2f}" width="{xb - xa:.2f}" height="{max(bottom - top, 0.5):.2f}" '
                    'fill="steelblue"/>')
        xm = 0.5 * (xa + xb)
        body.append(f'<line class="spread" x1="{xm:.2f}" y1="{at(b - r):.2f}" x2="{xm:.2f}" y2="{at(b + r):.2f}" stroke="black"/>')
        if n <= 16:
            body.append(f'<text x="{xm:.2f}" y="{_H - _B + 30}" text-anchor="middle" font-size="10">'
                        f'{html.escape(record["labels"][k])}</text>')
    body.append(f'<line class="zero" x1="{_L}" y1="{at(0.0):.2f}" x2="{_W - _R}" y2="{at(0.0):.2f}" stroke="black" '
                'stroke-dasharray="4 3"/>')
    return _svg(title, body, f"stratum of {record['variable']}", "bias +- rmse", (0.0, float(n - 1)), (y0, y1))
