"""Models blended with fitted weights: the host side of case_ops.case_error_moments and case_ops.blend_predictions
(cae_case_error_moments and cae_blend_predictions, include/cae_hip.h).  The settings and their refusals, the solver of the
weights, the fit from a table of per-unit error moments, its K-fold cross-validation and its bootstrap, and the writers:
blend.json, the printed line and the page with the error-correlation table and the bar chart of the weights with interval
whiskers.  DESIGN.md section 9, "Model blending", holds the definitions.

A row of moments for M candidates is {n, S e_0 .. S e_{M-1}, S e_i e_j for i <= j in row-major order}, e_m = P_m - a over the
common finite pixels.  With Sw = 1 the blend's error is S w_m e_m (+ c), so its mse is the quadratic form w' E w with E = S / n
(+ 2 c w' e + c^2 with e = Se / n): everything below follows from column sums of such rows.

Host only: standard library and numpy.
"""
import html
import itertools
import json
import math
from fractions import Fraction

import numpy as np

from . import compare, conformal, records
from .records import shown as _shown
from .report import _B, _H, _L, _R, _T, _W, Document, _scale, _svg, svg_data_uri

MAX_CANDIDATES = 8
MAX_RESAMPLES = 10 ** 6
MAX_UNITS = compare.MAX_UNITS
MODES = ("convex", "affine", "equal")
DEFAULT_MODE = "convex"
DEFAULT_FOLDS = 5
DEFAULT_RESAMPLES = 2000
DEFAULT_CONFIDENCE = "0.95"
DEFAULT_FILE = "blend.json"
DEFAULT_PREDICTION_VARIABLE = "blend_output"


# ---- the settings --------------------------------------------------------------------------------------------------------

def parse_confidence(text):
    """the confidence of the intervals as the exact Fraction of its text (0 < c < 1, never through a float)"""
    try:
        return conformal.parse_level(text)
    except ValueError as refused:
        raise ValueError(f"blend_confidence: {refused}") from None


def check_mode(mode):
    if mode not in MODES:
        raise ValueError(f"blend_mode must be one of {', '.join(MODES)}, got {mode!r}")
    return mode


def _integer(name, value, lo, hi, hi_text=None):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer, float)) or int(value) != value or not lo <= int(value) <= hi:
        raise ValueError(f"{name} must be an integer from {lo} to {hi_text or hi}, got {value!r}")
    return int(value)


def check_resamples(resamples):
    """0: no intervals"""
    return _integer("blend_resamples", resamples, 0, MAX_RESAMPLES)


def check_seed(seed):
    return _integer("blend_seed", seed, 0, (1 << 64) - 1, "2^64 - 1")


def check_folds(folds, n_unit=None):
    """0 switches the cross-validation off; else 2 .. n_unit folds"""
    folds = _integer("blend_folds", folds, 0, MAX_UNITS)
    if folds == 1:
        raise ValueError("blend_folds must be 0 (no cross-validation) or at least 2, got 1")
    if n_unit is not None and folds > n_unit:
        raise ValueError(f"blend_folds: {folds} folds need at least as many resampling units, there are {n_unit}")
    return folds


def check_candidates(variables, labels=None):
    """(variables, labels) of the candidates P_0 .. P_{M-1}; labels: None (the variables' names), or one label per candidate"""
    names = [str(v) for v in (variables or [])]
    if not 1 <= len(names) <= MAX_CANDIDATES:
        raise ValueError(f"blend_variables: 1 to {MAX_CANDIDATES} variables expected, got {len(names)}")
    twice = [v for v in names if names.count(v) > 1]
    if twice:
        raise ValueError(f"blend_variables: {twice[0]!r} is named twice")
    if labels is None:
        return names, list(names)
    labels = [str(v) for v in labels]
    if len(labels) != len(names):
        raise ValueError(f"blend_labels: {len(names)} labels expected, one per candidate, got {len(labels)}")
    if len(set(labels)) != len(labels):
        raise ValueError("blend_labels: the labels must differ")
    return names, labels


# ---- rows of moments -----------------------------------------------------------------------------------------------------

def width(m):
    return 1 + m + m * (m + 1) // 2


def candidates_of(n_col):
    """M of a row of n_col moments"""
    for m in range(1, MAX_CANDIDATES + 1):
        if width(m) == n_col:
            return m
    raise ValueError(f"rows of 1 + M + M (M + 1) / 2 moments with 1 <= M <= {MAX_CANDIDATES} expected, got {n_col} columns")


def unpack(sums):
    """(n (...), Se (..., M), S (..., M, M) symmetric) of (..., 1 + M + M (M + 1) / 2) sums"""
    sums = np.asarray(sums, dtype=np.float64)
    m = candidates_of(sums.shape[-1])
    (iu, ju) = np.triu_indices(m)
    full = np.zeros(sums.shape[:-1] + (m, m), dtype=np.float64)
    full[..., iu, ju] = sums[..., 1 + m:]
    full[..., ju, iu] = sums[..., 1 + m:]
    return sums[..., 0], sums[..., 1:1 + m], full


def moments(sums):
    """(E (..., M, M), e (..., M)) = (S / n, Se / n) of sums; NaN where n is 0"""
    (n, se, full) = unpack(sums)
    with np.errstate(invalid="ignore", divide="ignore"):
        return records.ratio(full, n[..., None, None]), records.ratio(se, n[..., None])


def centred(big_e, e):
    """E - e e': the matrix the weights are fitted on when an intercept is fitted with them"""
    return big_e - e[..., :, None] * e[..., None, :]


def quadratic(big_e, e, w, c=0.0):
    """the blend's mse w' E w + 2 c w' e + c^2, over any leading indices"""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.einsum("...i,...ij,...j->...", w, big_e, w) + 2.0 * c * np.einsum("...i,...i->...", w, e) + c * c


# ---- the solver ----------------------------------------------------------------------------------------------------------

def _eliminate(a, b):
    """x with a x = b for a batch a (B, k, k), b (B, k) by Gaussian elimination with partial pivoting (the first largest
    |entry| of the column), and the systems that are not singular: none of their pivots is 0 and x is finite"""
    a = a.copy()
    b = b.copy()
    (count, k) = b.shape
    rows = np.arange(count)
    ok = np.ones(count, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for col in range(k):
            at = col + np.argmax(np.abs(a[:, col:, col]), axis=1)
            (a[rows, col], a[rows, at]) = (a[rows, at], a[rows, col])
            (b[rows, col], b[rows, at]) = (b[rows, at], b[rows, col])
            pivot = a[:, col, col]
            ok &= (pivot != 0.0) & np.isfinite(pivot)
            safe = np.where(ok, pivot, 1.0)
            factor = a[:, col + 1:, col] / safe[:, None]
            a[:, col + 1:, :] = a[:, col + 1:, :] - factor[:, :, None] * a[:, None, col, :]
            b[:, col + 1:] = b[:, col + 1:] - factor * b[:, None, col]
        x = np.zeros_like(b)
        for col in range(k - 1, -1, -1):
            pivot = np.where(ok, a[:, col, col], 1.0)
            x[:, col] = (b[:, col] - np.einsum("bj,bj->b", a[:, col, col + 1:], x[:, col + 1:])) / pivot
    ok &= np.isfinite(x).all(axis=1)
    return x, ok


def _on_support(big_e, support):
    """(w (B, k), solved (B,)) minimising w' E_SS w subject to Sw = 1 on the candidates of `support`: the KKT system
    [2 E_SS 1; 1' 0] [w; l] = [0; 1]"""
    k = len(support)
    sub = big_e[:, support][:, :, support]
    a = np.zeros((big_e.shape[0], k + 1, k + 1), dtype=np.float64)
    a[:, :k, :k] = 2.0 * sub
    a[:, :k, k] = 1.0
    a[:, k, :k] = 1.0
    b = np.zeros((big_e.shape[0], k + 1), dtype=np.float64)
    b[:, k] = 1.0
    (x, ok) = _eliminate(a, b)
    return x[:, :k], ok


def supports(m):
    """the non-empty supports of m candidates by increasing size, then lexicographically"""
    return [list(s) for size in range(1, m + 1) for s in itertools.combinations(range(m), size)]


def solve(big_e, mode=DEFAULT_MODE):
    """The weights minimising w' E w, for E (M, M) or a batch (B, M, M).  "equal": 1 / M.  "affine": subject to Sw = 1, the
    KKT system of all M candidates; NaN where it is singular.  "convex": subject to Sw = 1 and w >= 0, solved exactly by
    enumerating the non-empty supports (at most 255) by increasing size, then lexicographically: each support's equality-
    constrained KKT system is solved, a singular one is skipped, a support with a weight <= 0 is infeasible, and a later
    support replaces the kept one only when its objective is strictly lower.  A candidate outside the kept support has the
    weight 0 exactly.  A matrix that is not finite gives NaN."""
    check_mode(mode)
    big_e = np.asarray(big_e, dtype=np.float64)
    single = big_e.ndim == 2
    batch = big_e[None] if single else big_e
    if batch.ndim != 3 or batch.shape[1] != batch.shape[2] or not 1 <= batch.shape[1] <= MAX_CANDIDATES:
        raise ValueError(f"solve: a matrix (M, M) or a batch (B, M, M) with 1 <= M <= {MAX_CANDIDATES} expected, got {big_e.shape}")
    (count, m) = batch.shape[:2]
    finite = np.isfinite(batch).all(axis=(1, 2))
    work = np.where(finite[:, None, None], batch, 0.0)
    if mode == "equal":
        w = np.full((count, m), 1.0 / m)
    elif mode == "affine":
        (w, ok) = _on_support(work, list(range(m)))
        w = np.where(ok[:, None], w, np.nan)
    else:
        w = np.full((count, m), np.nan)
        kept = np.full(count, np.inf)
        for support in supports(m):
            (ws, ok) = _on_support(work, support)
            ok &= (ws > 0.0).all(axis=1)
            with np.errstate(invalid="ignore", over="ignore"):
                objective = np.einsum("bi,bij,bj->b", ws, work[:, support][:, :, support], ws)
                better = ok & (objective < kept)
            if better.any():
                full = np.zeros((count, m), dtype=np.float64)
                full[:, support] = ws
                w = np.where(better[:, None], full, w)
                kept = np.where(better, objective, kept)
    w = np.where(finite[:, None], w, np.nan)
    return w[0] if single else w


# ---- the fit -------------------------------------------------------------------------------------------------------------

def fit_sums(sums, mode=DEFAULT_MODE, intercept=False):
    """(w (..., M), c (...)) fitted on (..., width) sums: E = S / n, e = Se / n; with intercept E is replaced by E - e e' and
    c = -S w_m e_m, else c = 0"""
    (big_e, e) = moments(sums)
    lead = big_e.shape[:-2]
    m = big_e.shape[-1]
    flat = (centred(big_e, e) if intercept else big_e).reshape((-1, m, m))
    w = solve(flat, mode).reshape(lead + (m,))
    c = -np.einsum("...i,...i->...", w, e) if intercept else np.zeros(lead, dtype=np.float64)
    return w, c


def mse_of(sums, w, c=0.0):
    """the mse of the blend (w, c) on sums"""
    (big_e, e) = moments(sums)
    return quadratic(big_e, e, np.asarray(w, dtype=np.float64), c)


def single_mse(sums):
    """(..., M): every candidate's own mse S e_m^2 / n"""
    (big_e, _) = moments(sums)
    return np.diagonal(big_e, axis1=-2, axis2=-1)


def fit(table, mode=DEFAULT_MODE, intercept=False):
    """The fit on a table (n_unit, width) of per-unit moments, from its column sums in ascending unit order: {"weights" (M,),
    "intercept", "mse_blend", "mse_candidates" (M,), "bias_candidates" (M,), "best_single" (the first candidate of the lowest
    mse), "mse_best_single", "gain" = 1 - mse_blend / mse_best_single}"""
    total = compare.column_sums(np.asarray(table, dtype=np.float64))
    (w, c) = fit_sums(total, mode, intercept)
    if not np.isfinite(w).all():
        raise ValueError(f"blend: the {mode} weights are not defined on these moments (no common pixel, or candidates whose "
                         "errors are alike make the system singular: use blend_mode convex)")
    each = single_mse(total)
    best = int(np.argmin(each))
    blend_mse = float(mse_of(total, w, c))
    return {"weights": w, "intercept": float(c), "mse_blend": blend_mse, "mse_candidates": each, "bias_candidates": moments(total)[1],
            "best_single": best, "mse_best_single": float(each[best]), "gain": float(1.0 - records.ratio(blend_mse, each[best]))}


def fold_of(n_unit, folds):
    """unit u, numbered by first appearance, belongs to fold u mod K"""
    return np.arange(int(n_unit), dtype=np.int64) % int(folds)


def cross_validate(table, folds, mode=DEFAULT_MODE, intercept=False):
    """K-fold cross-validation on the table: for fold f the weights are fitted on the other folds' rows (their column sums in
    ascending unit order) and scored on fold f's sums as the squared error n_f (w' E_f w + 2 c w' e_f + c^2); likewise the best
    single candidate chosen on the other folds and equal weights.  The pooled out-of-fold mse is the squared errors added
    over the folds, divided by the pixels.  Returns {"folds", "mse_blend", "mse_best_single", "mse_equal", "gain" = 1 -
    mse_blend / mse_best_single, "fold_weights" (K, M), "fold_intercepts" (K,), "fold_best_single" (K,), "fold_pixels" (K,)}"""
    table = np.asarray(table, dtype=np.float64)
    folds = check_folds(folds, table.shape[0])
    if folds == 0:
        raise ValueError("cross_validate: at least 2 folds expected")
    m = candidates_of(table.shape[1])
    member = fold_of(table.shape[0], folds)
    squared = {"blend": 0.0, "best_single": 0.0, "equal": 0.0}
    (pixels, fold_w, fold_c, fold_best, fold_n) = (0.0, [], [], [], [])
    equal = np.full(m, 1.0 / m)
    for f in range(folds):
        (train, test) = (compare.column_sums(table[member != f]), compare.column_sums(table[member == f]))
        (w, c) = fit_sums(train, mode, intercept)
        if not np.isfinite(w).all():
            raise ValueError(f"blend: the {mode} weights are not defined without fold {f} (no common pixel there, or a singular system)")
        best = int(np.argmin(single_mse(train)))
        (n_f, se_f, s_f) = unpack(test)
        squared["blend"] += float(np.einsum("i,ij,j->", w, s_f, w) + 2.0 * c * np.dot(w, se_f) + c * c * n_f)
        squared["best_single"] += float(s_f[best, best])
        squared["equal"] += float(np.einsum("i,ij,j->", equal, s_f, equal))
        pixels += float(n_f)
        fold_w.append(w), fold_c.append(float(c)), fold_best.append(best), fold_n.append(float(n_f))
    found = {"folds": folds}
    for (key, value) in squared.items():
        found["mse_" + key] = float(records.ratio(value, pixels))
    found["gain"] = float(1.0 - records.ratio(found["mse_blend"], found["mse_best_single"]))
    found.update(fold_weights=np.stack(fold_w), fold_intercepts=np.array(fold_c), fold_best_single=np.array(fold_best),
                 fold_pixels=np.array(fold_n))
    return found


def correlation(sums):
    """the correlation matrix of the candidates' errors: (E - e e')_ij / sqrt((E - e e')_ii (E - e e')_jj), NaN without a spread"""
    (big_e, e) = moments(sums)
    cov = centred(big_e, e)
    spread = np.sqrt(np.maximum(np.diagonal(cov, axis1=-2, axis2=-1), 0.0))
    return records.ratio(cov, spread[..., :, None] * spread[..., None, :])


def summary(table, resampled, variables, labels, mode, intercept, confidence, resamples, seed, folds, n_cases, plane,
            block_variable=None):
    """The record of a fit.  table (n_unit, width): the units' moments; resampled (B, width): cae_bootstrap_sums of it, or None
    without intervals; confidence: a Fraction.  The point values come from the table's column sums, the cross-validation
    from its rows, the intervals of every weight and of the gain from the fit repeated on every resample (a resample whose
    fit is not finite is left out and counted in "degenerate").  The weights and the intercept are stored as float.hex() text
    as well, so that apply uses the fitted bits."""
    table = np.asarray(table, dtype=np.float64)
    m = len(variables)
    if table.ndim != 2 or table.shape[1] != width(m) or (resampled is not None and np.shape(resampled)[1:] != (width(m),)):
        raise ValueError(f"blend.summary: a table (n_unit, {width(m)}) and resamples (B, {width(m)}) expected, got {table.shape} and "
                         f"{np.shape(resampled)}")
    total = compare.column_sums(table)
    found = fit(table, mode, intercept)
    (w, c) = (found["weights"], found["intercept"])
    none = {"interval": [float("nan"), float("nan")], "degenerate": 0}
    if resampled is not None:
        resampled = np.asarray(resampled, dtype=np.float64)
        (wb, cb) = fit_sums(resampled, mode, intercept)
        with np.errstate(invalid="ignore", divide="ignore"):
            gain_b = 1.0 - records.ratio(mse_of(resampled, wb, cb), np.min(single_mse(resampled), axis=-1))
        weight_stats = [compare._stat(w[k], wb[:, k], confidence) for k in range(m)]
        gain = compare._stat(found["gain"], gain_b, confidence)
        c_stat = compare._stat(c, cb, confidence)
    else:
        weight_stats = [dict(none, value=float(w[k])) for k in range(m)]
        gain = dict(none, value=found["gain"])
        c_stat = dict(none, value=float(c))
    record = {"variables": list(variables), "labels": list(labels), "mode": mode, "fit_intercept": bool(intercept),
              "weights": [float(v) for v in w], "weights_hex": [float(v).hex() for v in w],
              "intercept": float(c), "intercept_hex": float(c).hex(), "intercept_interval": c_stat,
              "resamples": int(resamples), "seed": int(seed), "confidence": conformal.level_text(Fraction(confidence)),
              "block_variable": block_variable, "n_cases": int(n_cases), "n_unit": int(table.shape[0]),
              "pixels_counted": int(total[0]), "pixels_left_out": int(n_cases) * int(plane) - int(total[0]),
              "candidates": [{"variable": variables[k], "label": labels[k], "mse": float(found["mse_candidates"][k]),
                              "bias": float(found["bias_candidates"][k]), "weight": weight_stats[k]} for k in range(m)],
              "error_correlation": correlation(total), "mse_blend": found["mse_blend"], "best_single": labels[found["best_single"]],
              "mse_best_single": found["mse_best_single"], "gain": gain,
              "cross_validation": cross_validate(table, folds, mode, intercept) if folds else None}
    return record


# ---- the writers ---------------------------------------------------------------------------------------------------------

def write_json(path, record):
    """blend.json: the record as strict JSON, a value that is not finite as null"""
    return records.write_json(path, records.json_record(record))


def read_json(path):
    """(variables, weights (M,) float64, intercept, record) of a blend.json: the weights and the intercept from their
    float.hex() text, the bits the fit found"""
    with open(path) as f:
        record = json.load(f)
    try:
        variables = [str(v) for v in record["variables"]]
        w = np.array([float.fromhex(t) for t in record["weights_hex"]], dtype=np.float64)
        c = float.fromhex(record["intercept_hex"])
    except (KeyError, TypeError, ValueError) as refused:
        raise ValueError(f"{path} is not a blend file: {refused!r}") from None
    if not 1 <= len(variables) <= MAX_CANDIDATES or w.shape[0] != len(variables) or not (np.isfinite(w).all() and math.isfinite(c)):
        raise ValueError(f"{path} is not a blend file: 1 to {MAX_CANDIDATES} variables with one finite weight each expected")
    return variables, w, c, record


def _interval(stat):
    return f"[{_shown(stat['interval'][0])}, {_shown(stat['interval'][1])}]"


def line(record):
    """blend: <M> candidates, <U> units, <mode>: <label> <w> [lo, hi], ...; mse <x> against <label> <y>, gain <g> [lo, hi];
    cross-validated (<K> folds) gain <g>"""
    m = len(record["candidates"])
    parts = ", ".join(f"{cand['label']} {_shown(cand['weight']['value'])} {_interval(cand['weight'])}" for cand in record["candidates"])
    text = (f"blend: {m} candidate{'s' if m != 1 else ''}, {record['n_unit']} units, {record['mode']}"
            f"{' with intercept ' + _shown(record['intercept']) if record['fit_intercept'] else ''}: {parts}; "
            f"mse {_shown(record['mse_blend'])} against {record['best_single']} {_shown(record['mse_best_single'])}, "
            f"gain {_shown(record['gain']['value'])} {_interval(record['gain'])}")
    cv = record.get("cross_validation")
    if cv:
        text += f"; cross-validated ({cv['folds']} folds) gain {_shown(cv['gain'])}"
    return text


def correlation_rows(record):
    """the rows of the page's error-correlation table: a header, then one row per candidate"""
    labels = [cand["label"] for cand in record["candidates"]]
    matrix = np.asarray(record["error_correlation"], dtype=np.float64)
    return [[""] + labels] + [[labels[i]] + [_shown(v) for v in matrix[i]] for i in range(len(labels))]


def svg_weights(record, title):
    """The bar chart of the weights: per candidate one <rect class="weight"> from 0 to its weight, carrying label, weight and
    the interval in data- attributes, and where the interval exists a whisker <line class="interval"> over it."""
    cands = record["candidates"]
    n = len(cands)
    spans = []
    for cand in cands:
        (lo, hi) = cand["weight"]["interval"]
        spans.append((float(lo), float(hi)) if lo is not None and hi is not None and math.isfinite(float(lo)) and math.isfinite(float(hi))
                     else None)
    values = [float(cand["weight"]["value"]) for cand in cands]
    y0 = min([0.0] + values + [s[0] for s in spans if s])
    y1 = max([0.0] + values + [s[1] for s in spans if s])
    if y1 <= y0:
        y1 = y0 + 1.0
    at = lambda v: _scale(v, y0, y1, _H - _B, _T)       # noqa: E731
    body = []
    for (k, (cand, v, s)) in enumerate(zip(cands, values, spans)):
        xa = _scale(k + 0.15, 0.0, float(n), _L, _W - _R)
        xb = _scale(k + 0.85, 0.0, float(n), _L, _W - _R)
        (lo, hi) = s if s else (v, v)
        (top, bottom) = (min(at(v), at(0.0)), max(at(v), at(0.0)))
        body.append(f'<rect class="weight" data-label="{html.escape(cand["label"], quote=True)}" data-weight="{v:.6g}" data-lo="{lo:.6g}" '
                    f'data-hi="{hi:.6g}" x="{xa:.2f}" y="{top:.2f}" width="{xb - xa:.2f}" height="{max(bottom - top, 0.5):.2f}" '
                    'fill="steelblue"/>')
        xm = 0.5 * (xa + xb)
        if s:
            body.append(f'<line class="interval" x1="{xm:.2f}" y1="{at(lo):.2f}" x2="{xm:.2f}" y2="{at(hi):.2f}" stroke="black"/>')
        body.append(f'<text x="{xm:.2f}" y="{_H - _B + 30}" text-anchor="middle" font-size="10">{html.escape(cand["label"])}</text>')
    return _svg(title, body, "candidate", "weight", (0.0, float(max(n - 1, 1))), (y0, y1))


def page(record):
    """blend/index.html: the fit in a paragraph, the table of the candidates, the error-correlation table and the bar chart"""
    doc = Document("Model blending")
    doc.body.add("h1").text("Model blending")
    doc.body.add("p").text(line(record))
    doc.body.add("p").text(f"{record['pixels_counted']} common pixels of {record['n_cases']} cases, {record['pixels_left_out']} left out; "
                           f"{record['n_unit']} units x {record['resamples']} resamples, confidence {record['confidence']}, seed {record['seed']}")

    def table(rows, css):
        t = doc.body.add("table", {"class": css, "border": "1"})
        for (i, row) in enumerate(rows):
            tr = t.add("tr")
            for cell in row:
                tr.add("th" if i == 0 else "td").text(str(cell))

    doc.body.add("h2").text("Candidates")
    table([["Candidate", "variable", "mse", "bias", "weight", "interval"]]
          + [[cand["label"], cand["variable"], _shown(cand["mse"]), _shown(cand["bias"]), _shown(cand["weight"]["value"]),
              _interval(cand["weight"])] for cand in record["candidates"]], "candidates")
    doc.body.add("h2").text("Error correlation")
    table(correlation_rows(record), "error-correlation")
    doc.body.add("h2").text("Weights")
    doc.body.add("img", {"src": svg_data_uri(svg_weights(record, "weights of the blend")), "alt": "weights of the blend"})
    return doc.html()
