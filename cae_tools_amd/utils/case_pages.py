"""The case-summary pages of evaluate_cae: per partition an index.html with one table row per case (worst mse first) and,
side by side, the input, target, prediction and error of that case as palette PNGs.

Standard library and numpy only.  The pixels are palette indices that arrive ready-made in PNG scanline form (the GPU
renderer, engine.render_cases: a filter byte 0 and one index per pixel for every row); this module only deflates them
(zlib) and wraps them in the PNG chunks, so the renderer's bytes reach the file untouched.

Index 0 is the missing-value entry (NaN), fully transparent.  Indices 1..255 are 255 levels of a cool-to-warm diverging
map, linear in sRGB from (59, 76, 192) through (221, 221, 221) at the middle level to (180, 4, 38).
"""
import os
import struct
import zlib

import numpy as np

from .report import Document

LEVELS = 255
ERROR_LAYER = "error"        # the name of the prediction - target layer
_COOL, _MID, _WARM = (59, 76, 192), (221, 221, 221), (180, 4, 38)
_HALF = (LEVELS - 1) // 2       # the middle level: 127 steps from either end


def _mix(a, b, j):
    """a + (b - a) * j / _HALF per component, rounded half up (in integers, so exactly)"""
    return tuple((2 * _HALF * ca + 2 * (cb - ca) * j + _HALF) // (2 * _HALF) for (ca, cb) in zip(a, b))


def palette():
    """the 256 (r, g, b, a) entries: entry 0 transparent, entry 1 + j the colour of level j"""
    entries = [(0, 0, 0, 0)]
    for j in range(LEVELS):
        rgb = _mix(_COOL, _MID, j) if j <= _HALF else _mix(_MID, _WARM, j - _HALF)
        entries.append(rgb + (255,))
    return entries


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


_PALETTE = palette()
_PLTE = _chunk(b"PLTE", bytes(c for entry in _PALETTE for c in entry[:3]))
_TRNS = _chunk(b"tRNS", b"\x00")        # alpha of entry 0; the entries after the last listed one are opaque
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def png_palette(scanlines, width, height):
    """a complete 8-bit palette PNG from one image's scanline bytes (height rows of a filter byte and width indices)"""
    raw = scanlines.tobytes() if hasattr(scanlines, "tobytes") else bytes(scanlines)
    if len(raw) != height * (width + 1):
        raise ValueError(f"{len(raw)} scanline bytes for a {width} x {height} image")
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 3, 0, 0, 0)
    return PNG_SIGNATURE + _chunk(b"IHDR", ihdr) + _PLTE + _TRNS + _chunk(b"IDAT", zlib.compress(raw)) + \
        _chunk(b"IEND", b"")


def colour_bar():
    """the 255 levels from low to high as a 255 x 1 palette PNG"""
    return png_palette(bytes([0]) + bytes(range(1, LEVELS + 1)), LEVELS, 1)


def select_cases(n, sample_count):
    """the cases drawn: all n of them for sample_count None, else k = min(sample_count, n) evenly spaced ones"""
    if sample_count is None:
        return list(range(n))
    k = max(0, min(int(sample_count), n))
    return [i * n // k for i in range(k)]


def case_order(cases, mse):
    """positions into `cases` by descending mse (a NaN mse counts as the worst), ties by case index"""
    def key(p):
        v = float(mse[p])
        return (0, 0.0, cases[p]) if v != v else (1, -v, cases[p])
    return sorted(range(len(cases)), key=key)


STYLE = "body { font-family: sans-serif; margin: 1em 2em; } table { border-collapse: collapse; } " \
        "td, th { border: 1px solid #bbb; padding: 2px 8px; text-align: center; } " \
        "img { image-rendering: pixelated; display: block; } img.bar { height: 12px; margin: 2px 0; }"
IMAGE_WIDTH = 250


def _fmt(v, digits=6):
    try:
        return f"{float(v):.{digits}g}"
    except (TypeError, ValueError):
        return str(v)


def image_name(case, layer):
    return f"case{int(case):06d}_{layer}.png"


def write_case_pages(folder, title, cases, layers, measures, times=None, time_units=""):
    """<folder>/index.html and <folder>/images/case{index:06d}_{layer}.png.
    cases: the selected case indices; layers: [(name, lo, hi, scanlines)] in column order, scanlines a (k, H, W + 1) uint8
    array whose image p belongs to cases[p]; measures: {"mae": (k,), "mse": (k,)} of the selected cases; times: the time
    coordinate's value per selected case, or None.  Rows go by descending mse.  Returns the page's path."""
    images = os.path.join(folder, "images")
    os.makedirs(images, exist_ok=True)
    with open(os.path.join(images, "colourbar.png"), "wb") as f:
        f.write(colour_bar())
    doc = Document(f"Case summary: {title}")
    doc.head.add("style").text(STYLE)
    body = doc.body
    body.add("h2").text(f"Case summary for partition {title}")
    body.add("p").text(f"{len(cases)} cases, worst mse first. Channel 0 of every variable; transparent pixels are missing "
                       "values.")
    table = body.add("table")
    head = table.add("tr")
    fixed = ["case"] + ([f"time ({time_units})" if time_units else "time"] if times is not None else []) + ["mae", "mse"]
    for label in fixed:
        head.add("th").text(label)
    for (name, lo, hi, _) in layers:
        th = head.add("th", {"class": "layer", "data-layer": name})
        th.add("div").text(name)
        th.add("img", {"class": "bar", "src": "images/colourbar.png", "width": IMAGE_WIDTH, "alt": "colour bar"})
        th.add("div").text(f"{_fmt(lo)} … {_fmt(hi)}")
    for p in case_order(cases, measures["mse"]):
        tr = table.add("tr", {"class": "case", "data-case": int(cases[p])})
        tr.add("td").text(int(cases[p]))
        if times is not None:
            tr.add("td").text(_fmt(times[p], 15))
        tr.add("td").text(_fmt(measures["mae"][p]))
        tr.add("td").text(_fmt(measures["mse"][p]))
        for (name, _, _, scanlines) in layers:
            (height, pitch) = scanlines.shape[1:]
            fname = image_name(cases[p], name)
            with open(os.path.join(images, fname), "wb") as f:
                f.write(png_palette(np.ascontiguousarray(scanlines[p]), pitch - 1, height))
            tr.add("td").add("img", {"src": "images/" + fname, "width": IMAGE_WIDTH, "alt": f"case {int(cases[p])} {name}"})
    path = os.path.join(folder, "index.html")
    with open(path, "w") as f:
        f.write(doc.html())
    return path
