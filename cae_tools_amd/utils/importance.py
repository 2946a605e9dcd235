"""Permutation importance of the model's input variables: the host side of BaseModel.importance (cae_normalise_pack_gather and
cae_case_importance, include/cae_hip.h).  The permutations, the groups of variables, the scores of every group from the eight
sums per group, repeat and case, and the writers: importance_<partition>.json, the printed line, the rows of the report's
"Input importance" section, its bar chart of importance +- sd and the page of the per-pixel change of the mse.  DESIGN.md
section 9 holds the definition.

Host only: standard library and numpy.
"""
import html
import math
import os

import numpy as np

from . import case_pages, records
from .records import shown as _shown
from .report import _B, _H, _L, _R, _T, _W, Document, _scale, _svg

MAX_REPEATS = 64
# the eight sums of a case: cae_case_importance's order
(N, SQ1, SQ0, AB1, AB0, DD, UP, DOWN) = range(8)


def permutations(n, repeats, seed):
    """(repeats, n) int32: row r is a single n-cycle, so no case keeps its own values, built by Sattolo's algorithm from
    numpy.random.default_rng([seed, r]): p = 0 .. n - 1, then for i = n - 1 down to 1 one draw j = rng.integers(0, i)
    (0 <= j < i) and p[i], p[j] swapped.  The same for every group of variables.  n >= 2."""
    (n, repeats, seed) = (int(n), int(repeats), int(seed))
    if n < 2:
        raise ValueError(f"permutations: at least 2 cases expected, got {n}")
    if repeats < 1:
        raise ValueError(f"permutations: at least 1 repeat expected, got {repeats}")
    out = np.empty((repeats, n), dtype=np.int32)
    for r in range(repeats):
        rng = np.random.default_rng([seed, r])
        p = np.arange(n, dtype=np.int32)
        for i in range(n - 1, 0, -1):
            j = int(rng.integers(0, i))
            (p[i], p[j]) = (p[j], p[i])
        out[r] = p
    return out


def check_repeats(repeats):
    if isinstance(repeats, bool) or int(repeats) != repeats or not 1 <= int(repeats) <= MAX_REPEATS:
        raise ValueError(f"importance_repeats must be an integer from 1 to {MAX_REPEATS}, got {repeats!r}")
    return int(repeats)


def check_groups(groups, variables=None):
    """the groups as a list of lists of names: None is every variable of `variables` on its own.  ValueError for no group,
    an empty group, a variable twice in a group and, where `variables` (the model's input variables) is given, an unknown
    one."""
    if groups is None:
        if variables is None:
            return None
        return [[name] for name in variables]
    found = [[str(v) for v in ([g] if isinstance(g, str) else g)] for g in groups]
    if not found:
        raise ValueError("importance_groups: at least one group expected")
    for g in found:
        if not g or any(not v for v in g):
            raise ValueError(f"importance_groups: a group must name at least one input variable, got {','.join(g)!r}")
        twice = sorted({v for v in g if g.count(v) > 1})
        if twice:
            raise ValueError(f"importance_groups: {twice[0]!r} is named twice in the group {','.join(g)!r}")
        if variables is not None:
            unknown = [v for v in g if v not in variables]
            if unknown:
                raise ValueError(f"importance_groups: {unknown[0]!r} is not an input variable of the model "
                                 f"({', '.join(variables)})")
    return found


def parse_groups(arguments, variables=None):
    """the --importance-groups arguments, each a comma-separated list of input-variable names forming one group, as
    check_groups returns them; None when the flag was not given"""
    if arguments is None:
        return check_groups(None, variables)
    return check_groups([[v.strip() for v in str(a).split(",")] for a in arguments], variables)


def group_name(group):
    return "+".join(group)


def _div(num, den):
    return float(num) / float(den) if den else float("nan")


def _sd(values):
    """the sample standard deviation (ddof 1) of the values that are not NaN; NaN with fewer than two"""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    return float(np.std(v, ddof=1)) if v.size >= 2 else float("nan")


def _group(name, variables, s):
    """the scores of one group from its sums s (R, n_case, 8), pooled over the pairs of all cases"""
    s = np.asarray(s, dtype=np.float64)
    per = s.sum(axis=1)                                         # (R, 8): a repeat's sums over the cases
    mse1 = [_div(t[SQ1], t[N]) for t in per]
    mse0 = [_div(t[SQ0], t[N]) for t in per]
    mae1 = [_div(t[AB1], t[N]) for t in per]
    mae0 = [_div(t[AB0], t[N]) for t in per]
    dmse = [a - b for (a, b) in zip(mse1, mse0)]
    dmae = [a - b for (a, b) in zip(mae1, mae0)]
    total = per.sum(axis=0)
    counted = s[:, :, N] > 0
    grew = (s[:, :, SQ1] > s[:, :, SQ0]) & counted              # a case's n is the same on both sides
    with np.errstate(invalid="ignore", divide="ignore"):
        case_delta = np.where(counted, (s[:, :, SQ1] - s[:, :, SQ0]) / np.where(counted, s[:, :, N], 1.0), np.nan)
    return {"name": name, "variables": list(variables), "pairs": int(total[N]),
            "mse_base": mse0, "mse_permuted": mse1, "mean_mse_base": records.stat(mse0), "mean_mse_permuted": records.stat(mse1),
            "importance": records.stat(dmse), "importance_sd": _sd(dmse),
            "ratio": _div(records.stat(mse1), records.stat(mse0)) if records.stat(mse0) == records.stat(mse0) else float("nan"),
            "mae_base": mae0, "mae_permuted": mae1, "mean_mae_base": records.stat(mae0), "mean_mae_permuted": records.stat(mae1),
            "mae_importance": records.stat(dmae), "mae_importance_sd": _sd(dmae),
            "mae_ratio": _div(records.stat(mae1), records.stat(mae0)) if records.stat(mae0) == records.stat(mae0) else float("nan"),
            "sensitivity": math.sqrt(_div(total[DD], total[N])) if total[N] else float("nan"),
            "cases_grew": _div(int(grew.sum()), int(counted.sum())),
            "pixels_grew": _div(total[UP], total[N]), "pixels_shrank": _div(total[DOWN], total[N]),
            "pixels_grew_count": int(total[UP]), "pixels_shrank_count": int(total[DOWN]),
            "case_delta_mse": [records.stat(case_delta[:, i]) for i in range(s.shape[1])]}


def summary(groups, sums, seed=0, maps=None):
    """The record of one partition.  groups: the groups as check_groups returns them; sums: (G, R, n_case, 8) float64, the
    eight sums of cae_case_importance per group, repeat and case; maps: None or (G, 3, H, W), the per-pixel {count, S e1^2,
    S e0^2} over the cases and repeats.  Per group, pooled over the pairs of all cases: mse_base and mse_permuted per repeat
    and their means, importance = mean over the repeats of mse_permuted - mse_base with the standard deviation of the
    per-repeat values (ddof 1; NaN, null in JSON, for one repeat), ratio = mean mse_permuted / mean mse_base, the same for
    the mae, sensitivity = sqrt(S (P1 - P0)^2 / n), the share of (repeat, case) whose mse grew, the shares of pixels whose
    squared error grew and shrank, the rank by importance (1 = largest; a group without a pair last) and per case the change
    of the mse averaged over the repeats.  A quotient without pairs is NaN."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim != 4 or sums.shape[0] != len(groups) or sums.shape[3] != 8:
        raise ValueError(f"importance.summary: sums of shape ({len(groups)}, R, n_case, 8) expected, got {sums.shape}")
    found = [_group(group_name(g), g, sums[k]) for (k, g) in enumerate(groups)]
    key = lambda k: (0, -found[k]["importance"], k) if found[k]["importance"] == found[k]["importance"] else (1, 0.0, k)  # noqa: E731
    order = sorted(range(len(found)), key=key)
    for (rank, k) in enumerate(order):
        found[k]["rank"] = rank + 1
    record = {"n_cases": int(sums.shape[2]), "repeats": int(sums.shape[1]), "seed": int(seed), "n_groups": len(found),
              "mse_base": found[0]["mean_mse_base"] if found else float("nan"),
              "order": [found[k]["name"] for k in order], "groups": found}
    if maps is not None:
        record["maps"] = np.asarray(maps, dtype=np.float64)
    return record


def delta_maps(record):
    """(G, H, W): per group the change of the mse per pixel, S e1^2 / count - S e0^2 / count over the cases and repeats; NaN
    where a pixel has no pair"""
    m = np.asarray(record["maps"], dtype=np.float64)
    some = m[:, 0] > 0
    den = np.where(some, m[:, 0], 1.0)
    return np.where(some, m[:, 1] / den - m[:, 2] / den, np.nan)


def write_json(path, record):
    """importance_<partition>.json: the record without its maps as strict JSON, a score that is not finite as null"""
    kept = {k: v for (k, v) in record.items() if k != "maps"}
    return records.write_json(path, records.json_record(kept, (dict, list, tuple)))


def _by_rank(record):
    return sorted(record["groups"], key=lambda g: g["rank"])


def line(partition, record):
    """importance <partition>: <G> groups x <R> permutations of <N> cases, base mse <x>: <name> +<d> (x<ratio>), ...
    the groups largest importance first"""
    parts = [f"{g['name']} {_signed(g['importance'])} (x{_shown(g['ratio'])})" for g in _by_rank(record)]
    return (f"importance {partition}: {record['n_groups']} groups x {record['repeats']} permutations of {record['n_cases']} cases, "
            f"base mse {_shown(record['mse_base'])}: " + ", ".join(parts))


def _signed(v):
    if v is None or not math.isfinite(float(v)):
        return _shown(v)
    return format(float(v), "+.6g")


COLUMNS = (("base mse", "mean_mse_base"), ("permuted mse", "mean_mse_permuted"), ("importance", "importance"),
           ("sd", "importance_sd"), ("ratio", "ratio"), ("mae importance", "mae_importance"), ("sensitivity", "sensitivity"),
           ("cases grew", "cases_grew"), ("pixels grew", "pixels_grew"))


def section_rows(record):
    """the rows of the report's table: a header and one row per group, largest importance first"""
    rows = [["Rank", "Group"] + [title for (title, _) in COLUMNS]]
    for g in _by_rank(record):
        rows.append([str(g["rank"]), g["name"]] + [_shown(g[key]) for (_, key) in COLUMNS])
    return rows


def heading(record):
    return (f"{record['n_groups']} group{'s' if record['n_groups'] != 1 else ''}, {record['repeats']} "
            f"permutation{'s' if record['repeats'] != 1 else ''} of {record['n_cases']} cases, seed {record['seed']}")


def svg_bars(record, title):
    """The bar chart of a record: per group with a finite importance one <rect class="group"> from 0 to its importance,
    carrying name, importance and sd in data- attributes, and where the sd exists a whisker <line class="spread"> over
    importance - sd .. importance + sd; the zero line dashed.  The groups in rank order."""
    groups = [g for g in _by_rank(record) if g["importance"] is not None and math.isfinite(float(g["importance"]))]
    n = len(groups)
    if not groups:
        return _svg(title, [], "group", "mse permuted - mse", (0.0, 1.0), (0.0, 1.0))
    spread = [float(g["importance_sd"]) if g["importance_sd"] is not None and math.isfinite(float(g["importance_sd"])) else 0.0
              for g in groups]
    (y0, y1) = (min(0.0, min(float(g["importance"]) - s for (g, s) in zip(groups, spread))),
                max(0.0, max(float(g["importance"]) + s for (g, s) in zip(groups, spread))))
    if not y1 > y0:
        (y0, y1) = (y0 - 0.5, y1 + 0.5)
    at = lambda v: _scale(v, y0, y1, _H - _B, _T)       # noqa: E731
    body = []
    for (k, (g, s)) in enumerate(zip(groups, spread)):
        v = float(g["importance"])
        xa = _scale(k + 0.15, 0.0, float(n), _L, _W - _R)
        xb = _scale(k + 0.85, 0.0, float(n), _L, _W - _R)
        (top, bottom) = (min(at(v), at(0.0)), max(at(v), at(0.0)))
        body.append(f'<rect class="group" data-name="{html.escape(g["name"], quote=True)}" data-importance="{v:.6g}" '
                    f'data-sd="{s:.6g}" x="{xa:.2f}" y="{top:.2f}" width="{xb - xa:.2f}" height="{max(bottom - top, 0.5):.2f}" '
                    'fill="steelblue"/>')
        xm = 0.5 * (xa + xb)
        if s > 0.0:
            body.append(f'<line class="spread" x1="{xm:.2f}" y1="{at(v - s):.2f}" x2="{xm:.2f}" y2="{at(v + s):.2f}" stroke="black"/>')
        if n <= 16:
            body.append(f'<text x="{xm:.2f}" y="{_H - _B + 30}" text-anchor="middle" font-size="10">{html.escape(g["name"])}</text>')
    body.append(f'<line class="zero" x1="{_L}" y1="{at(0.0):.2f}" x2="{_W - _R}" y2="{at(0.0):.2f}" stroke="black" '
                'stroke-dasharray="4 3"/>')
    return _svg(title, body, "group, largest importance first", "mse permuted - mse", (0.0, float(max(n - 1, 1))), (y0, y1))


def image_name(partition, k):
    return f"{partition}_group{k}.png"


def write_maps_page(folder, partitions):
    """<folder>/index.html and <folder>/<partition>_group<k>.png.  partitions: [(partition, record, lo, hi, layers)] in page
    order, layers = [(group name, scanlines)] in the record's group order with scanlines an (H, W + 1) uint8 array of
    palette indices in PNG scanline form, drawn over [lo, hi].  One table row per partition, one column per group.
    Returns the page's path."""
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "colourbar.png"), "wb") as f:
        f.write(case_pages.colour_bar())
    doc = Document("Input importance")
    doc.head.add("style").text(case_pages.STYLE)
    body = doc.body
    body.add("h2").text("Change of the mse per pixel")
    body.add("p").text("mse with the group's variables drawn from another case minus the mse as it is, over the cases and "
                       "permutations whose target and both predictions are finite at the pixel. Channel 0; transparent pixels "
                       "have no value.")
    table = body.add("table")
    for (partition, record, lo, hi, layers) in partitions:
        head = table.add("tr", {"class": "ranges", "data-partition": partition})
        head.add("th").text(f"{partition} ({heading(record)})")
        row = table.add("tr", {"class": "maps", "data-partition": partition})
        row.add("td").text(partition)
        for (k, (name, scanlines)) in enumerate(layers):
            th = head.add("th", {"class": "layer", "data-layer": name})
            th.add("div").text(name)
            th.add("img", {"class": "bar", "src": "colourbar.png", "width": case_pages.IMAGE_WIDTH, "alt": "colour bar"})
            th.add("div", {"class": "range"}).text(f"{case_pages._fmt(lo)} … {case_pages._fmt(hi)}")
            (height, pitch) = np.shape(scanlines)
            fname = image_name(partition, k)
            with open(os.path.join(folder, fname), "wb") as f:
                f.write(case_pages.png_palette(np.ascontiguousarray(scanlines), pitch - 1, height))
            row.add("td").add("img", {"src": fname, "width": case_pages.IMAGE_WIDTH, "alt": f"{partition} {name}"})
    path = os.path.join(folder, "index.html")
    with open(path, "w") as f:
        f.write(doc.html())
    return path
