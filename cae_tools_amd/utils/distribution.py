"""Value distributions of prediction against target: the host side of engine.joint_histogram (cae_joint_hist,
include/cae_hip.h).  From its four arrays - the joint counts over coarse bins, the two fine marginal counts, the per-bin error
sums and the outside counts - the curves a verification along value needs: the conditional bias, mae and rmse per target
bin, the reliability curve per prediction bin, the conditional slope, the quantiles of both marginals and their Q-Q
pairs, the Wasserstein-1 distance, the Perkins score and the contingency scores of four exceedance thresholds; and the
writers: distribution_<partition>.json, the printed line, the rows of the report's "Value distribution" section and
distribution/index.html.  DESIGN.md section 9 holds the bin rule.

Host only: standard library and numpy.
"""
import base64
import math
import os

import numpy as np

from . import records
from .case_pages import LEVELS, png_palette
from .records import ratio as _ratio, shown as _shown
from .report import STYLE, Document, svg_data_uri, svg_lines

QUANTILES = (0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99)
THRESHOLDS = ((0.05, "below"), (0.9, "above"), (0.95, "above"), (0.99, "above"))     # "above": at or above the edge


def _div(num, den):
    return float(num) / float(den) if den else float("nan")


def quantile_from_counts(count, lo, hi, q):
    """The q-quantile of a histogram of n_fine equal bins over [lo, hi]: with r = q * n, the first bin k with cum[k] >= r
    and count[k] > 0 holds the sample of rank ceil(r); the value is lo + w * (k + (r - cum[k - 1]) / count[k]) with the bin
    width w = (hi - lo) / n_fine, so it lies in the bin of numpy's "inverted_cdf" quantile.  NaN without a count."""
    count = np.asarray(count, dtype=np.int64).reshape(-1)
    n = int(count.sum())
    if n == 0:
        return float("nan")
    cum = np.cumsum(count)
    r = float(q) * n
    k = int(np.nonzero((cum >= r) & (count > 0))[0][0])
    before = int(cum[k - 1]) if k > 0 else 0
    w = (float(hi) - float(lo)) / count.size
    return float(lo) + w * (k + (r - before) / int(count[k]))


def contingency(joint, cond, lo, hi, q, side):
    """The exceedance table of one threshold from the joint counts joint[ia][ip]: the coarse edge e (0 .. n_bin) whose target
    non-exceedance fraction #{a-bin < e} / n is nearest to q, ties to the lower edge.  The event is "bin >= e" for side "above"
    (at or above the edge) and "bin < e" for "below".  hits: event in target and prediction; misses: in the target only;
    false_alarms: in the prediction only.  pod = h / (h + m), far = f / (h + f), csi = h / (h + m + f), frequency_bias =
    (h + f) / (h + m); tail_bias: the mean of p - a over the target's pixels in the event, from cond[0]."""
    joint = np.asarray(joint, dtype=np.int64)
    n_bin = joint.shape[0]
    n = int(joint.sum())
    target = joint.sum(axis=1)
    below = np.concatenate(([0], np.cumsum(target)))           # below[e]: target pixels in bins < e
    fraction = below / float(n) if n else np.full(n_bin + 1, np.nan)
    e = int(np.argmin(np.abs(fraction - q))) if n else 0
    (lo, hi) = (float(lo), float(hi))
    if side == "above":
        (h, m, f, c) = (joint[e:, e:].sum(), joint[e:, :e].sum(), joint[:e, e:].sum(), joint[:e, :e].sum())
        tail = slice(e, n_bin)
    else:
        (h, m, f, c) = (joint[:e, :e].sum(), joint[:e, e:].sum(), joint[e:, :e].sum(), joint[e:, e:].sum())
        tail = slice(0, e)
    (h, m, f, c) = (int(h), int(m), int(f), int(c))
    return {"q": float(q), "side": side, "edge": e, "value": lo + e * ((hi - lo) / n_bin),
            "fraction": float(fraction[e]), "hits": h, "misses": m, "false_alarms": f, "correct_negatives": c,
            "pod": _div(h, h + m), "far": _div(f, h + f), "csi": _div(h, h + m + f), "frequency_bias": _div(h + f, h + m),
            "tail_bias": _div(np.asarray(cond, dtype=np.float64)[0, tail, 0].sum(), int(target[tail].sum()))}


def curves_from_counts(joint, marg, cond, outside, lo, hi, n_pixels=None):
    """The curves from engine.joint_histogram's (joint (n_bin, n_bin), marginals (2, n_fine), cond (2, n_bin, 4), outside (4,))
    over [lo, hi], as a dict of numbers and lists:
        lo, hi, n_bin, sub, edges (n_bin + 1), centres (n_bin), pairs, pixels_left_out (n_pixels - pairs; None without
        n_pixels), outside {target_below, target_above, prediction_below, prediction_above}
        target_count, mean_target = lo + S(a - lo) / c, bias = S d / c, mae = S|d| / c, rmse = sqrt(S d^2 / c)  per target bin
        prediction_count, mean_prediction = lo + S(p - lo) / c, mean_target_given_prediction = mean_prediction - S d / c
                                                                                     per prediction bin (reliability)
        conditional_slope: the count-weighted least-squares slope of the mean prediction (mean_target + bias) on
                           mean_target over the target bins with a count; below 1, the extremes are damped
        quantile_levels, quantile_target, quantile_prediction, quantile_difference (prediction - target), qq (the pairs)
        wasserstein1 = w * S_k |cumP[k] - cumA[k]| / n over the fine bins of width w
        perkins_score = S_k min(P[k], A[k]) / n over the coarse bins, perkins_bins = n_bin
        exceedance: [contingency(...)] for THRESHOLDS
        joint, marginal_target, marginal_prediction: the counts themselves
    What has no denominator is NaN."""
    joint = np.asarray(joint, dtype=np.int64)
    marg = np.asarray(marg, dtype=np.int64)
    cond = np.asarray(cond, dtype=np.float64)
    outside = np.asarray(outside, dtype=np.int64).reshape(4)
    n_bin = int(joint.shape[0])
    n_fine = int(marg.shape[1])
    if joint.shape != (n_bin, n_bin) or marg.shape[0] != 2 or n_fine % n_bin or cond.shape != (2, n_bin, 4):
        raise ValueError(f"curves_from_counts: shapes {joint.shape}, {marg.shape} and {cond.shape} do not belong together")
    (lo, hi) = (float(lo), float(hi))
    sub = n_fine // n_bin
    n = int(joint.sum())
    width = (hi - lo) / n_bin
    edges = lo + width * np.arange(n_bin + 1)
    (ca, cp) = (joint.sum(axis=1), joint.sum(axis=0))
    mean_a = lo + _ratio(cond[0, :, 3], ca)
    bias = _ratio(cond[0, :, 0], ca)
    mean_p = lo + _ratio(cond[1, :, 3], cp)
    have = ca > 0
    slope = float("nan")
    if have.any():
        (x, y, c) = (mean_a[have], (mean_a + bias)[have], ca[have].astype(np.float64))
        (xm, ym) = (np.sum(c * x) / c.sum(), np.sum(c * y) / c.sum())
        slope = _div(np.sum(c * (x - xm) * (y - ym)), np.sum(c * (x - xm) ** 2))
    qa = [quantile_from_counts(marg[0], lo, hi, q) for q in QUANTILES]
    qp = [quantile_from_counts(marg[1], lo, hi, q) for q in QUANTILES]
    w = (hi - lo) / n_fine
    return {"lo": lo, "hi": hi, "n_bin": n_bin, "sub": sub, "edges": edges.tolist(),
            "centres": (0.5 * (edges[:-1] + edges[1:])).tolist(), "pairs": n,
            "pixels_left_out": None if n_pixels is None else int(n_pixels) - n,
            "outside": {"target_below": int(outside[0]), "target_above": int(outside[1]),
                        "prediction_below": int(outside[2]), "prediction_above": int(outside[3])},
            "target_count": ca.tolist(), "mean_target": mean_a.tolist(), "bias": bias.tolist(),
            "mae": _ratio(cond[0, :, 1], ca).tolist(), "rmse": np.sqrt(_ratio(cond[0, :, 2], ca)).tolist(),
            "prediction_count": cp.tolist(), "mean_prediction": mean_p.tolist(),
            "mean_target_given_prediction": (mean_p - _ratio(cond[1, :, 0], cp)).tolist(),
            "conditional_slope": slope,
            "quantile_levels": list(QUANTILES), "quantile_target": qa, "quantile_prediction": qp,
            "quantile_difference": [b - a for (a, b) in zip(qa, qp)], "qq": [[a, b] for (a, b) in zip(qa, qp)],
            "wasserstein1": _div(w * float(np.abs(np.cumsum(marg[1]) - np.cumsum(marg[0])).sum()), n),
            "perkins_score": _div(int(np.minimum(ca, cp).sum()), n), "perkins_bins": n_bin,
            "exceedance": [contingency(joint, cond, lo, hi, q, side) for (q, side) in THRESHOLDS],
            "joint": joint.tolist(), "marginal_target": marg[0].tolist(), "marginal_prediction": marg[1].tolist()}


def _threshold(curves, q):
    return next(t for t in curves["exceedance"] if t["q"] == q)


def summary(curves):
    """the scalars of the curves that the printed line and the report's table show: pairs, pixels_left_out, outside (the four
    counts added), conditional_slope, bias (pooled mean of p - a), q95_bias (the difference of the 0.95 quantiles),
    wasserstein1, perkins_score, perkins_bins and pod / far / csi / frequency_bias / tail_bias at the 0.95 threshold"""
    k = curves["quantile_levels"].index(0.95)
    t = _threshold(curves, 0.95)
    total = float(np.nansum(np.asarray(curves["bias"], dtype=np.float64) * np.asarray(curves["target_count"], dtype=np.float64)))
    return {"pairs": curves["pairs"], "pixels_left_out": curves["pixels_left_out"], "outside": sum(curves["outside"].values()),
            "conditional_slope": curves["conditional_slope"], "bias": _div(total, curves["pairs"]),
            "q95_bias": curves["quantile_difference"][k], "wasserstein1": curves["wasserstein1"],
            "perkins_score": curves["perkins_score"], "perkins_bins": curves["perkins_bins"], "pod_q95": t["pod"],
            "far_q95": t["far"], "csi_q95": t["csi"], "frequency_bias_q95": t["frequency_bias"], "tail_bias_q95": t["tail_bias"]}


def json_record(curves):
    """the curves as strict JSON values: a number that is not finite becomes null"""
    return records.json_record(curves, (dict, list, tuple))


def write_json(path, curves):
    """distribution_<partition>.json: the curves and, under "summary", their scalars"""
    return records.write_json(path, json_record({**curves, "summary": summary(curves)}))


def line(partition, curves):
    """distribution <partition>: slope <s>, q95 bias <b>, W1 <w>, Perkins <p>, POD/FAR at q95 <x>/<y>"""
    s = summary(curves)
    return (f"distribution {partition}: slope {_shown(s['conditional_slope'])}, q95 bias {_shown(s['q95_bias'])}, "
            f"W1 {_shown(s['wasserstein1'])}, Perkins {_shown(s['perkins_score'])}, "
            f"POD/FAR at q95 {_shown(s['pod_q95'])}/{_shown(s['far_q95'])}")


SECTION_ROWS = (("conditional slope (below 1: damped extremes)", "conditional_slope"), ("mean bias", "bias"),
                ("bias of the 0.95 quantile", "q95_bias"), ("Wasserstein-1 distance", "wasserstein1"),
                ("Perkins score", "perkins_score"), ("POD at the target's q95", "pod_q95"), ("FAR at the target's q95", "far_q95"),
                ("CSI at the target's q95", "csi_q95"), ("frequency bias at the target's q95", "frequency_bias_q95"),
                ("mean bias over the target's tail above q95", "tail_bias_q95"))


def section_rows(curves):
    """the rows of the report's table: [[name, value]] with "none" for a value that does not exist"""
    s = summary(curves)
    rows = [["Score Name", "Score Value"]] + [[label, _shown(s[key])] for (label, key) in SECTION_ROWS]
    rows.append(["bins of the Perkins score", str(s["perkins_bins"])])
    left = s["pixels_left_out"]
    rows.append(["pixel pairs / left out / outside the range", f"{s['pairs']} / {'none' if left is None else left} / {s['outside']}"])
    return rows


def density_png(joint):
    """The joint counts as a palette PNG of n_bin x n_bin pixels, target along x, prediction along y with the lowest bin
    at the bottom: a bin without a count is transparent, a count c gets the level round(254 * log(c) / log(c_max))."""
    joint = np.asarray(joint, dtype=np.int64)
    n_bin = joint.shape[0]
    top = int(joint.max()) if joint.size else 0
    level = np.zeros(joint.shape, dtype=np.float64)
    if top > 1:
        level = np.log(np.maximum(joint, 1)) / math.log(top)
    index = np.where(joint > 0, 1 + np.rint((LEVELS - 1) * level), 0).astype(np.uint8)
    rows = index.T[::-1]                    # row 0 of the picture: the highest prediction bin
    lines = np.concatenate((np.zeros((n_bin, 1), dtype=np.uint8), rows), axis=1)
    return png_palette(np.ascontiguousarray(lines), n_bin, n_bin)


def write_page(folder, partitions):
    """<folder>/index.html.  partitions: [(partition, curves)] in page order.  Per partition the joint density on a log colour
    scale, the conditional bias with bias +- rmse, the reliability curve beside the diagonal, the Q-Q pairs beside the
    diagonal and the two marginal histograms over the coarse bins."""
    os.makedirs(folder, exist_ok=True)
    doc = Document("Value distribution")
    doc.head.add("style").text(STYLE + " img.density { image-rendering: pixelated; border: 1px solid #bbb; }")
    body = doc.body
    body.add("h2").text("Value distribution of prediction against target")
    body.add("p").text("Channel 0, over the pixels where prediction and target are finite; values outside the range are "
                       "counted in the first and the last bin.")
    for (partition, curves) in partitions:
        section = body.add("div", {"class": "distribution", "data-partition": partition})
        section.add("h3").text(f"{partition}: {curves['pairs']} pixel pairs, {curves['n_bin']} bins of {curves['sub']} over "
                               f"[{_shown(curves['lo'])}, {_shown(curves['hi'])}], conditional slope "
                               f"{_shown(curves['conditional_slope'])}")
        section.add("p").text("joint density (target along x, prediction along y, log colour scale)")
        png = "data:image/png;base64," + base64.b64encode(density_png(curves["joint"])).decode("ascii")
        section.add("img", {"class": "density", "src": png, "alt": f"{partition} joint density", "width": 384, "height": 384})
        (x, bias, rmse) = (curves["mean_target"], np.asarray(curves["bias"], dtype=np.float64),
                           np.asarray(curves["rmse"], dtype=np.float64))
        (xp, qa) = (curves["mean_prediction"], curves["quantile_target"])
        plots = [("conditional bias", "target", "prediction - target",
                  {"bias": (x, bias), "bias + rmse": (x, bias + rmse), "bias - rmse": (x, bias - rmse)}),
                 ("reliability", "prediction", "mean target", {"mean target": (xp, curves["mean_target_given_prediction"]),
                                                                "diagonal": (xp, xp)}),
                 ("Q-Q", "target quantile", "prediction quantile", {"quantiles": (qa, curves["quantile_prediction"]),
                                                                    "diagonal": (qa, qa)}),
                 ("marginals", "value", "pixels", {"target": (curves["centres"], curves["target_count"]),
                                                   "prediction": (curves["centres"], curves["prediction_count"])})]
        for (title, xlabel, ylabel, series) in plots:
            section.add("img", {"src": svg_data_uri(svg_lines(series, f"{partition} {title}", xlabel, ylabel)),
                                "alt": f"{partition} {title}"})
    path = os.path.join(folder, "index.html")
    with open(path, "w") as f:
        f.write(doc.html())
    return path
