"""Per-pixel skill maps over the cases of a partition: count, bias, mae, rmse, correlation and the ratio of the standard
deviations (prediction over target), from the nine per-pixel sums engine.pixel_sums returns (cae_pixel_sums,
include/cae_hip.h); and their writers, a NetCDF-3 file skill_<partition>.nc and the page maps/index.html with one row of
six palette PNGs per partition.

Host only: standard library and numpy in fp64.  The pixels of the PNGs arrive as ready-made scanlines (the GPU renderer,
engine.render_cases) and the value ranges as engine.case_range found them; the evaluator (models/model_evaluator.py)
makes both.
"""
import os

import numpy as np

from ..data import netcdf3
from . import case_pages
from .report import Document

MAPS = ("count", "bias", "mae", "rmse", "correlation", "sd_ratio")


def pixel_means(sums, shift):
    """(2, H, W): the mean of a and of p over a pixel's pairs, from sums about `shift` (a number or (2, H, W)); `shift`
    itself where a pixel has no pair.  As the shifts of a second pixel_sums call they centre its second moments."""
    s = np.asarray(sums, dtype=np.float64)
    shift = np.broadcast_to(np.asarray(shift, dtype=np.float64), (2,) + s.shape[1:])
    with np.errstate(divide="ignore", invalid="ignore"):
        means = shift + s[4:6] / s[0]
    return np.where(s[0] > 0, means, shift)


def maps_from_sums(sums, centred=None):
    """{"count", "bias", "mae", "rmse", "correlation", "sd_ratio"}, each (H, W) float64, from the (9, H, W) sums
    {n, S d, S|d|, S d^2, S a', S p', S a'^2, S p'^2, S a'p'} of the pairs of a pixel (d = p - a, x' = x - shift):
        bias = S d / n,  mae = S|d| / n,  rmse = sqrt(S d^2 / n)
        va = S a'^2 - (S a')^2 / n,  vp = S p'^2 - (S p')^2 / n,  cov = S a'p' - S a' S p' / n
        correlation = cov / sqrt(va vp),  sd_ratio = sqrt(max(vp, 0) / va)
    Every map but count is NaN where n == 0.  correlation and sd_ratio are NaN where n < 2, and where a variance they
    divide by (va and vp; va alone for sd_ratio) is no larger than its own rounding, v <= 8 n 2^-53 S x'^2: twice the sum
    of the summation bounds of S x'^2 and (S x')^2 / n, so a constant pixel gives NaN and not the noise of a cancellation.
    By the same rule a vp no larger than its rounding is the variance of a constant prediction: sd_ratio is then 0, as a
    two-pass computation gives, not the square root of that noise.
    centred: the sums of the same cases about per-pixel shifts near the means (pixel_means); va, vp and cov are then
    taken from them.  About one common shift a variance v is known to about n 2^-53 S x'^2 only, which is a relative
    error of 1e-5 where a prediction varies by 1e-5 of its distance from the shift; centred, S x'^2 is the variance."""
    s = np.asarray(sums, dtype=np.float64)
    if s.ndim < 1 or s.shape[0] != 9:
        raise ValueError(f"maps_from_sums: nine planes of sums expected, got shape {s.shape}")
    (n, sd, sad, sdd) = s[:4]
    (sa, sp, saa, spp, sap) = s[4:] if centred is None else np.asarray(centred, dtype=np.float64)[4:]
    with np.errstate(divide="ignore", invalid="ignore"):
        nn = np.where(n > 0, n, np.nan)
        va = saa - sa * sa / nn
        vp = spp - sp * sp / nn
        cov = sap - sa * sp / nn
        noise = 8.0 * n * 2.0 ** -53
        ok_a = (n >= 2) & (va > noise * saa)
        ok_p = (n >= 2) & (vp > noise * spp)
        return {"count": n.copy(),
                "bias": sd / nn,
                "mae": sad / nn,
                "rmse": np.sqrt(sdd / nn),
                "correlation": np.where(ok_a & ok_p, cov / np.sqrt(va * vp), np.nan),
                "sd_ratio": np.where(ok_a, np.sqrt(np.where(vp > noise * spp, vp, 0.0) / va), np.nan)}


def stack_maps(maps):
    """the six maps as one (6, 1, H, W) float64 array in MAPS order: six one-channel "cases" for case_range / render_cases"""
    return np.stack([np.asarray(maps[m], dtype=np.float64) for m in MAPS])[:, None]


def map_range(name, found, n_case):
    """(lo, hi) of map `name` over the partitions.  found: one (min, max, count) of the map's finite values per
    partition (engine.case_range); n_case: the largest number of cases of a partition.  count is drawn over [0, n_case],
    bias over +-max|bias|, every other map over its finite range, a map without a finite value over (0, 0)."""
    if name == "count":
        return 0.0, float(n_case)
    found = [f for f in found if f[2] > 0]
    if not found:
        return 0.0, 0.0
    (lo, hi) = (min(f[0] for f in found), max(f[1] for f in found))
    if name == "bias":
        bound = max(abs(lo), abs(hi))
        return -bound, bound
    return lo, hi


def write_netcdf(path, maps, dims, coordinates=None):
    """skill_<partition>.nc: the six float64 maps over dims = (y dimension, x dimension) of the target, and the
    coordinate variables given as {name: (dimension, values, attrs)}"""
    (ydim, xdim) = dims
    (h, w) = np.shape(maps["count"])
    variables = {}
    for (name, (dim, values, attrs)) in (coordinates or {}).items():
        variables[name] = ((dim,), np.asarray(values), dict(attrs or {}))
    for m in MAPS:
        variables[m] = ((ydim, xdim), np.asarray(maps[m], dtype=np.float64), {})
    netcdf3.write(path, {ydim: h, xdim: w}, variables)
    return path


def image_name(partition, name):
    return f"{partition}_{name}.png"


def write_maps_page(folder, partitions):
    """<folder>/index.html and <folder>/<partition>_<map>.png.  partitions: [(partition, n_case, layers)] in page order,
    layers = [(map name, lo, hi, scanlines)] with scanlines an (H, W + 1) uint8 array of palette indices in PNG scanline
    form.  One table row per partition, one column per map with the colour bar and the printed range.  Returns the
    page's path."""
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "colourbar.png"), "wb") as f:
        f.write(case_pages.colour_bar())
    doc = Document("Skill maps")
    doc.head.add("style").text(case_pages.STYLE)
    body = doc.body
    body.add("h2").text("Skill maps per pixel")
    body.add("p").text("Over the cases of a partition whose prediction and target are both finite at the pixel. Channel 0; "
                       "transparent pixels have no value.")
    table = body.add("table")
    for (partition, n_case, layers) in partitions:
        head = table.add("tr", {"class": "ranges", "data-partition": partition})
        head.add("th").text(f"{partition} ({int(n_case)} cases)")
        row = table.add("tr", {"class": "maps", "data-partition": partition})
        row.add("td").text(partition)
        for (name, lo, hi, scanlines) in layers:
            th = head.add("th", {"class": "layer", "data-layer": name})
            th.add("div").text(name)
            th.add("img", {"class": "bar", "src": "colourbar.png", "width": case_pages.IMAGE_WIDTH, "alt": "colour bar"})
            th.add("div", {"class": "range"}).text(f"{case_pages._fmt(lo)} … {case_pages._fmt(hi)}")
            (height, pitch) = np.shape(scanlines)
            fname = image_name(partition, name)
            with open(os.path.join(folder, fname), "wb") as f:
                f.write(case_pages.png_palette(np.ascontiguousarray(scanlines), pitch - 1, height))
            row.add("td").add("img", {"src": fname, "width": case_pages.IMAGE_WIDTH, "alt": f"{partition} {name}"})
    path = os.path.join(folder, "index.html")
    with open(path, "w") as f:
        f.write(doc.html())
    return path
