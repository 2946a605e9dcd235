"""The evaluation report of evaluate_cae: a small HTML5 writer and the two plots it embeds, drawn as SVG.

Standard library and numpy only (the reference draws its plots with seaborn / matplotlib, which are not dependencies
here).  Every text and attribute value is escaped.  The plots are embedded as inline data: URIs, so index.html stands
alone, as the reference's inlined PNGs do.
"""
import base64
import html
import math

import numpy as np

VOID = {"meta", "img", "br", "hr", "link"}


class Element:
    """one HTML element: add() appends a child element and returns it, text() appends escaped text and returns self"""

    def __init__(self, tag, attrs=None):
        self.tag = tag
        self.attrs = dict(attrs or {})
        self.children = []

    def add(self, tag, attrs=None):
        child = Element(tag, attrs)
        self.children.append(child)
        return child

    def text(self, text):
        self.children.append(str(text))
        return self

    def table(self, rows):
        """a <table> of one <tr> per row and one <td> per cell"""
        tbl = self.add("table")
        for row in rows:
            tr = tbl.add("tr")
            for cell in row:
                tr.add("td").text(cell)
        return tbl

    def render(self, out, depth=0):
        pad = "  " * depth
        attrs = "".join(f' {k}="{html.escape(str(v), quote=True)}"' for k, v in self.attrs.items() if v is not None)
        if self.tag in VOID:
            out.append(f"{pad}<{self.tag}{attrs}>")
            return
        if all(isinstance(c, str) for c in self.children):
            out.append(f"{pad}<{self.tag}{attrs}>{''.join(html.escape(c, quote=False) for c in self.children)}</{self.tag}>")
            return
        out.append(f"{pad}<{self.tag}{attrs}>")
        for c in self.children:
            if isinstance(c, str):
                out.append(pad + "  " + html.escape(c, quote=False))
            else:
                c.render(out, depth + 1)
        out.append(f"{pad}</{self.tag}>")


class Document:

    def __init__(self, title, language="en"):
        self.root = Element("html", {"lang": language})
        self.head = self.root.add("head")
        self.head.add("meta", {"charset": "utf-8"})
        self.head.add("title").text(title)
        self.body = self.root.add("body")

    def html(self):
        out = ["<!DOCTYPE html>"]
        self.root.render(out)
        return "\n".join(out) + "\n"


def svg_data_uri(svg):
    return "data:image/svg+xml;base64," + base64.b64encode(svg.encode("utf-8")).decode("ascii")


# ---- plots -----------------------------------------------------------------------------------

_W, _H = 640, 400
_L, _R, _T, _B = 70, 20, 40, 50      # plot margins


def _fmt(v):
    return f"{v:.4g}"


def _svg(title, body, xlabel, ylabel, x_range, y_range):
    """an SVG document with a title, two axes labelled at their ends, and `body` (elements in plot coordinates)"""
    (x0, x1), (y0, y1) = x_range, y_range
    (px0, px1, py0, py1) = (_L, _W - _R, _H - _B, _T)
    esc = html.escape
    parts = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{_W}" height="{_H}" viewBox="0 0 {_W} {_H}" '
             'font-family="sans-serif" font-size="12">',
             f'<rect x="0" y="0" width="{_W}" height="{_H}" fill="white"/>',
             f'<text x="{_W / 2}" y="22" text-anchor="middle" font-size="15">{esc(title)}</text>',
             f'<line x1="{px0}" y1="{py0}" x2="{px1}" y2="{py0}" stroke="black"/>',
             f'<line x1="{px0}" y1="{py0}" x2="{px0}" y2="{py1}" stroke="black"/>',
             f'<text x="{px0}" y="{py0 + 16}" text-anchor="middle">{esc(_fmt(x0))}</text>',
             f'<text x="{px1}" y="{py0 + 16}" text-anchor="middle">{esc(_fmt(x1))}</text>',
             f'<text x="{px0 - 6}" y="{py0}" text-anchor="end">{esc(_fmt(y0))}</text>',
             f'<text x="{px0 - 6}" y="{py1 + 4}" text-anchor="end">{esc(_fmt(y1))}</text>',
             f'<text x="{(px0 + px1) / 2}" y="{_H - 12}" text-anchor="middle">{esc(xlabel)}</text>',
             f'<text x="16" y="{(py0 + py1) / 2}" text-anchor="middle" '
             f'transform="rotate(-90 16 {(py0 + py1) / 2})">{esc(ylabel)}</text>']
    parts.extend(body)
    parts.append("</svg>")
    return "\n".join(parts)


def _scale(v, lo, hi, p_lo, p_hi):
    return p_lo + (p_hi - p_lo) * ((v - lo) / (hi - lo) if hi > lo else 0.5)


def histogram(values):
    """(counts, edges) of the finite values with numpy's "auto" bins (seaborn histplot's default), and how many values
    were left out as NaN / Inf"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    finite = v[np.isfinite(v)]
    if finite.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0), int(v.size)
    edges = np.histogram_bin_edges(finite, "auto")
    (counts, edges) = np.histogram(finite, bins=edges)
    return counts, edges, int(v.size - finite.size)


def svg_histogram(values, title):
    """an SVG histogram: one <rect class="bar"> per bin carrying its count in data-count, in bin order"""
    (counts, edges, dropped) = histogram(values)
    if dropped:
        title = f"{title} ({dropped} non-finite values not shown)"
    if counts.size == 0:
        return _svg(title, [], "value", "count", (0.0, 1.0), (0.0, 1.0))
    top = max(int(counts.max()), 1)
    (lo, hi) = (float(edges[0]), float(edges[-1]))
    body = []
    for k, c in enumerate(counts):
        xa = _scale(float(edges[k]), lo, hi, _L, _W - _R)
        xb = _scale(float(edges[k + 1]), lo, hi, _L, _W - _R)
        y = _scale(float(c), 0.0, float(top), _H - _B, _T)
        body.append(f'<rect class="bar" data-count="{int(c)}" x="{xa:.2f}" y="{y:.2f}" width="{max(xb - xa, 0.5):.2f}" '
                    f'height="{(_H - _B) - y:.2f}" fill="steelblue" stroke="white" stroke-width="0.5"/>')
    return _svg(title, body, "value", "count", (lo, hi), (0.0, float(top)))


def svg_rank_histogram(counts, title):
    """the rank histogram of an ensemble: one <rect class="rank"> per rank 0 .. K carrying its count in data-count, and the
    level of a flat histogram as a dashed line"""
    counts = [int(c) for c in counts]
    top = max(max(counts, default=0), 1)
    nb = max(len(counts), 1)
    body = []
    for k, c in enumerate(counts):
        xa = _scale(float(k), 0.0, float(nb), _L, _W - _R)
        xb = _scale(float(k + 1), 0.0, float(nb), _L, _W - _R)
        y = _scale(float(c), 0.0, float(top), _H - _B, _T)
        body.append(f'<rect class="rank" data-count="{c}" x="{xa:.2f}" y="{y:.2f}" width="{max(xb - xa, 0.5):.2f}" '
                    f'height="{(_H - _B) - y:.2f}" fill="seagreen" stroke="white" stroke-width="0.5"/>')
    if counts and sum(counts) > 0:
        y = _scale(sum(counts) / nb, 0.0, float(top), _H - _B, _T)
        body.append(f'<line class="flat" x1="{_L}" y1="{y:.2f}" x2="{_W - _R}" y2="{y:.2f}" stroke="black" '
                    'stroke-dasharray="4 3"/>')
    return _svg(title, body, "members below the target", "pixels", (0.0, float(nb - 1)), (0.0, float(top)))


_COLOURS = ("steelblue", "darkorange", "seagreen", "crimson")


def svg_lines(series, title, xlabel, ylabel):
    """an SVG line plot of named (x, y) series; points whose y is not finite are left out"""
    pts = {}
    for name, (xs, ys) in series.items():
        pts[name] = [(float(x), float(y)) for x, y in zip(xs, ys) if math.isfinite(float(y))]
    every = [p for ps in pts.values() for p in ps]
    if not every:
        return _svg(title, [], xlabel, ylabel, (0.0, 1.0), (0.0, 1.0))
    (x0, x1) = (min(p[0] for p in every), max(p[0] for p in every))
    (y0, y1) = (min(p[1] for p in every), max(p[1] for p in every))
    body = []
    for k, (name, ps) in enumerate(pts.items()):
        colour = _COLOURS[k % len(_COLOURS)]
        xy = " ".join(f"{_scale(x, x0, x1, _L, _W - _R):.2f},{_scale(y, y0, y1, _H - _B, _T):.2f}" for x, y in ps)
        if ps:
            body.append(f'<polyline class="series" data-name="{html.escape(name)}" data-points="{len(ps)}" '
                        f'points="{xy}" fill="none" stroke="{colour}" stroke-width="2"/>')
        body.append(f'<line x1="{_W - _R - 110}" y1="{_T + 10 + 18 * k}" x2="{_W - _R - 90}" y2="{_T + 10 + 18 * k}" '
                    f'stroke="{colour}" stroke-width="2"/>')
        body.append(f'<text x="{_W - _R - 84}" y="{_T + 14 + 18 * k}">{html.escape(name)}</text>')
    return _svg(title, body, xlabel, ylabel, (x0, x1), (y0, y1))


def svg_history(history):
    """log10 of the train and test losses against the test iteration; losses that are not positive are left out"""
    series = {}
    for name in ("train", "test"):
        losses = [float(v) for v in history.get(f"{name}_loss", [])]
        series[name] = (range(len(losses)), [math.log10(v) if v > 0 else math.nan for v in losses])
    return svg_lines(series, "history", "test_iteration", "log_loss")


# ---- the report ------------------------------------------------------------------------------

STYLE = "body { font-family: sans-serif; margin: 1em 2em; } table { border-collapse: collapse; } " \
        "td { border: 1px solid #bbb; padding: 2px 8px; } img { display: block; margin: 8px 0; }"


ENSEMBLE_ROWS = (("crps", "crps"), ("fair crps", "fair_crps"), ("mean per-case mae (deterministic)", "mae"),
                 ("rmse of the ensemble mean", "rmse_mean"), ("spread", "spread"), ("spread-skill ratio", "spread_skill"))


def _section(body, title, records, heading, rows, plots=None):
    """one optional analysis: the title, and per (partition, record) the heading "<partition>: <heading(record)>", the
    table rows(record) and one image per plot, plots being {alt text after the partition: record -> SVG}"""
    body.add("h2").text(title)
    for (partition, rec) in records:
        body.add("h3").text(f"{partition}: {heading(rec)}")
        body.table(rows(rec))
        for (alt, draw) in (plots or {}).items():
            body.add("img", {"src": svg_data_uri(draw(rec)), "alt": f"{partition} {alt}"})


def evaluation_report(metrics, measures, parameters=None, history=None, case_links=None, maps_link=None, ensemble=None,
                      spectra_link=None, ssim=None, baseline=None, distribution=None, strata=None, fss=None,
                      importance=None, novelty=None, compare=None):
    """index.html of evaluate_cae, its sections in the reference's order (model_evaluator.py:162-314).
    metrics: {"test": {...}, "train": {...}} (either may be absent); measures: [(partition, {"mae": values, "mse": values})]
    in page order; parameters: parameters.json; history: history.json; case_links: {partition: href}; maps_link: href of
    the per-pixel skill maps page (utils/skill_maps.py), linked after the partitions when given; ensemble: [(partition,
    record)] of VarAEModel.verify_ensemble's scores with "mae" (the mean per-case mae of the deterministic prediction) added:
    an "Ensemble verification" section with the ENSEMBLE_ROWS table, the rank histogram and the per-case CRPS histogram;
    spectra_link: href of the power spectra page (utils/spectra.py), linked after the skill maps when given; ssim:
    [(partition, record)] of utils/ssim.summary: a "Structural similarity" section with the table of the mean ssim, ms_ssim
    and psnr and the histogram of the per-case ssim; baseline: [(partition, record)] of utils/baseline.summary: a "Skill
    against interpolation" section with the table of the pooled and per-case skill against the interpolated input and the
    histogram of the per-case skill; distribution: ([(partition, curves)] of utils/distribution.curves_from_counts, href of
    the value distribution page): a "Value distribution" section with the table of the conditional slope, quantile bias,
    distances and exceedance scores, and the link; strata: [(partition, record)] of utils/strata.summary: a "Skill by stratum"
    section with the table of the scores per stratum and pooled and the bar chart of bias +- rmse per stratum; fss:
    ([(partition, record)] of utils/fss.summary, href of the neighbourhood skill page): a "Neighbourhood skill" section with
    the table of the pooled Fractions Skill Score per threshold and width, the uniform level and the skilful width, and the
    link; importance: ([(partition, record)] of utils/importance.summary, href of the page of per-pixel maps or None): an
    "Input importance" section with the table of the groups of input variables by rank, the bar chart of importance +- sd,
    and the link where there is one; novelty: [(partition, record)] of utils/novelty.summary: a "Novelty of the cases"
    section with the table of the scores and quintiles and the bar chart of the mse per novelty quintile; compare: [(partition,
    record)] of utils/compare.summary: a "Model comparison" section with the table of the candidates - mse, rmse, mae and bias,
    and against the first of them delta mse, skill, p better and significance - and the bar chart of the mse with the
    interval as whiskers."""
    doc = Document("Model Evaluation")
    doc.head.add("style").text(STYLE)
    body = doc.body
    body.add("h2").text("Model Metrics")
    for (label, key) in (("Test Metrics", "test"), ("Train Metrics", "train")):
        if key in metrics:
            body.add("h3").text(label)
            body.table([["Metric Name", "Metric Value"]] + [[k, f"{v:0.3f}"] for (k, v) in metrics[key].items()])
    body.add("h2").text("Model Evaluation Results")
    for (partition, values) in measures:
        body.add("h3").text(partition)
        for (measure, v) in values.items():
            body.add("img", {"src": svg_data_uri(svg_histogram(v, measure)), "alt": f"{partition} {measure} histogram"})
        if case_links and partition in case_links:
            body.add("p").add("a", {"href": case_links[partition]}).text(f"Case summary for partition {partition}")
    if maps_link:
        body.add("p").add("a", {"href": maps_link}).text("Skill maps per pixel")
    if spectra_link:
        body.add("p").add("a", {"href": spectra_link}).text("Power spectra of prediction against target")
    if ensemble:
        _section(body, "Ensemble verification", ensemble,
                 lambda rec: f"{rec['ensemble_size']} members, {rec['n']} pixels, {rec['tied']} tied",
                 lambda rec: [["Score Name", "Score Value"]] + [[label, f"{float(rec[key]):0.6g}"] for (label, key) in ENSEMBLE_ROWS],
                 {"rank histogram": lambda rec: svg_rank_histogram(rec["rank_counts"], "rank histogram"),
                  "crps histogram": lambda rec: svg_histogram(rec["case_crps"], "crps")})
    if ssim:
        from . import ssim as ssim_scores
        _section(body, "Structural similarity", ssim,
                 lambda rec: f"{rec['n_counted']} of {rec['n_cases']} cases, {len(rec['scales'])} "
                             f"scale{'s' if len(rec['scales']) != 1 else ''}",
                 ssim_scores.section_rows, {"ssim histogram": lambda rec: svg_histogram(rec["case_ssim"], "ssim")})
    if baseline:
        from . import baseline as baseline_scores
        _section(body, "Skill against interpolation", baseline,
                 lambda rec: f"{rec['mode']} interpolation of {rec['variable']}, {rec['in_shape'][0]} x {rec['in_shape'][1]} to "
                             f"{rec['out_shape'][0]} x {rec['out_shape'][1]}, {rec['n_counted']} of {rec['n_cases']} cases",
                 baseline_scores.section_rows, {"skill histogram": lambda rec: svg_histogram(rec["case_skill"], "skill")})
    if distribution:
        from . import distribution as distribution_curves
        (records, link) = distribution
        _section(body, "Value distribution", records,
                 lambda rec: f"{rec['pairs']} pixel pairs, {rec['n_bin']} bins over [{rec['lo']:.6g}, {rec['hi']:.6g}]",
                 distribution_curves.section_rows)
        if link:
            body.add("p").add("a", {"href": link}).text("Value distribution of prediction against target")
    if strata:
        from . import strata as strata_scores
        _section(body, "Skill by stratum", strata,
                 lambda rec: f"{rec['n_strata']} strata of {rec['variable']}, {rec['pooled']['pairs']} pixel pairs, "
                             f"{rec['unclassified']} pixels unclassified",
                 strata_scores.section_rows,
                 {"skill by stratum": lambda rec: strata_scores.svg_bars(rec, f"bias +- rmse by {rec['variable']}")})
    if fss:
        from . import fss as fss_scores
        (records, link) = fss
        _section(body, "Neighbourhood skill", records,
                 lambda rec: f"{len(rec['thresholds'])} threshold{'s' if len(rec['thresholds']) != 1 else ''}, widths "
                             f"{', '.join(str(n) for n in rec['widths']) or 'none'}, {rec['n_cases']} cases, gaps {rec['gaps']}",
                 fss_scores.section_rows)
        if link:
            body.add("p").add("a", {"href": link}).text("Fractions Skill Score of prediction against target")
    if importance:
        from . import importance as importance_scores
        (records, link) = importance
        _section(body, "Input importance", records, importance_scores.heading, importance_scores.section_rows,
                 {"input importance": lambda rec: importance_scores.svg_bars(rec, "importance +- sd")})
        if link:
            body.add("p").add("a", {"href": link}).text("Change of the mse per pixel by group of input variables")
    if novelty:
        from . import novelty as novelty_scores
        _section(body, "Novelty of the cases", novelty, novelty_scores.heading, novelty_scores.section_rows,
                 {"mse by novelty quintile": lambda rec: novelty_scores.svg_quintiles(rec, "mse by novelty quintile")})
    if compare:
        from . import compare as compare_scores
        _section(body, "Model comparison", compare, compare_scores.heading, compare_scores.section_rows,
                 {"mse by candidate": lambda rec: compare_scores.svg_bars(rec, "mse with bootstrap interval")})
    if parameters or history:
        body.add("h2").text("Training Summary")
    if parameters:
        body.add("h2").text("Training Parameters")
        rows = [["Parameter Name", "Parameter Value"]]
        if history:
            rows.append(["total epochs", str(history["nr_epochs"])])
        rows.extend([k, str(v)] for (k, v) in parameters.items())
        body.table(rows)
    if history:
        body.add("img", {"src": svg_data_uri(svg_history(history)), "alt": "training history", "width": 768})
    return doc.html()
