"""Power spectra of prediction against target over radial wavenumber bins: the host side of engine.case_spectra
(cae_case_spectra, include/cae_hip.h).  The bin table and the window the kernel is given, the curves formed from its sums
- the binned power spectral density of prediction and target, their ratio, the spectral coherence, the error's share of
the target's power and the effective resolution read off the ratio - and their writers, spectra_<partition>.json and the
page spectra/index.html.  DESIGN.md section 9 holds the definition.

Host only: standard library and numpy; the table is made in Python integers, so no bin depends on a rounding.
"""
import math
import os

import numpy as np

from . import records
from .report import Document, STYLE, svg_data_uri, svg_lines

RATIO_THRESHOLD = 0.5        # effective resolution: the lowest bin whose power ratio falls below it


def bin_count(h, w):
    """M = max(1, min(h, w) // 2): the number of bins, each 1 / (2 M) cycles per pixel wide, up to the Nyquist frequency 1/2"""
    return max(1, min(int(h), int(w)) // 2)


def bin_table(h, w):
    """(h, w // 2 + 1) int32: the bin of mode (ky, kx), floor(2 M f) for f = sqrt((ky' / h)^2 + (kx / w)^2) cycles per
    pixel with ky' = min(ky, h - ky), formed in integers as isqrt((4 M^2 (ky'^2 w^2 + kx^2 h^2)) // (h^2 w^2)); -1 for
    the mean mode (0, 0) and wherever the value reaches M (f >= 1/2)."""
    (h, w) = (int(h), int(w))
    m = bin_count(h, w)
    table = np.empty((h, w // 2 + 1), dtype=np.int32)
    for ky in range(h):
        kyp = min(ky, h - ky)
        for kx in range(w // 2 + 1):
            q = kyp * kyp * w * w + kx * kx * h * h
            b = math.isqrt((4 * m * m * q) // (h * h * w * w))
            table[ky, kx] = -1 if (ky == 0 and kx == 0) or b >= m else b
    return table


def mode_weight(w):
    """(w // 2 + 1,) float64: 1 for kx == 0 and 2 kx == w, else 2 - the modes of the other half plane"""
    kx = np.arange(int(w) // 2 + 1)
    return np.where((kx == 0) | (2 * kx == int(w)), 1.0, 2.0)


def window(n):
    """the centred Hann window of n points, 1/2 - 1/2 cos(2 pi (j + 1/2) / n); a single 1 for n == 1"""
    n = int(n)
    if n == 1:
        return np.ones(1, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(n, dtype=np.float64) + 0.5) / n)


def bin_modes(h, w):
    """(M,) float64: the full-plane modes of each bin, the sum of mode_weight over its table entries"""
    table = bin_table(h, w)
    weight = np.broadcast_to(mode_weight(w), table.shape)
    keep = table >= 0
    return np.bincount(table[keep], weights=weight[keep], minlength=bin_count(h, w)).astype(np.float64)


def curves_from_sums(sums, counted, h, w):
    """The curves of one partition from engine.case_spectra's (N, M, 4) sums and (N,) counted flags, as a dict of lists
    of M numbers (NaN where a denominator is 0) and three scalars:
        modes, wavelength (2 M / (b + 1/2) pixels), psd_pred, psd_target (S / (n_counted modes S wy^2 S wx^2)),
        power_ratio PP / AA, coherence RePA / sqrt(PP AA), error_share DD / AA,
        n_cases, n_counted, effective_resolution (the wavelength of the lowest bin whose power_ratio is below 0.5, or None).
    The cases are added by numpy in case order."""
    m = bin_count(h, w)
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, m, 4)
    counted = np.asarray(counted, dtype=bool).reshape(-1)
    total = np.zeros((m, 4), dtype=np.float64)
    for c in range(sums.shape[0]):
        total += sums[c]
    n_counted = int(counted.sum())
    modes = bin_modes(h, w)
    norm = n_counted * modes * float(np.sum(window(h) ** 2)) * float(np.sum(window(w) ** 2))
    (pp, aa, pa, dd) = (total[:, 0], total[:, 1], total[:, 2], total[:, 3])
    with np.errstate(divide="ignore", invalid="ignore"):
        nan = np.full(m, np.nan)
        psd_pred = np.where(norm > 0, pp / np.where(norm > 0, norm, 1.0), nan)
        psd_target = np.where(norm > 0, aa / np.where(norm > 0, norm, 1.0), nan)
        ratio = np.where(aa != 0, pp / np.where(aa != 0, aa, 1.0), nan)
        den = np.sqrt(pp * aa)
        coherence = np.where(den != 0, pa / np.where(den != 0, den, 1.0), nan)
        share = np.where(aa != 0, dd / np.where(aa != 0, aa, 1.0), nan)
    wavelength = 2.0 * m / (np.arange(m, dtype=np.float64) + 0.5)
    below = [b for b in range(m) if ratio[b] < RATIO_THRESHOLD]
    return {"modes": modes.tolist(), "wavelength": wavelength.tolist(), "psd_pred": psd_pred.tolist(),
            "psd_target": psd_target.tolist(), "power_ratio": ratio.tolist(), "coherence": coherence.tolist(),
            "error_share": share.tolist(), "n_cases": int(sums.shape[0]), "n_counted": n_counted,
            "effective_resolution": float(wavelength[below[0]]) if below else None}


def json_record(curves, h, w):
    """the curves as strict JSON values: a number that is not finite becomes null"""
    return {**records.json_record(curves, (list,)), "h": int(h), "w": int(w)}


def write_json(path, curves, h, w):
    """spectra_<partition>.json: the curves, n_cases, n_counted, h, w and effective_resolution"""
    return records.write_json(path, json_record(curves, h, w))


def line(partition, curves):
    """spectra <partition>: effective_resolution <x|none> pixels, <n_counted>/<n> cases"""
    return (f"spectra {partition}: effective_resolution {records.shown(curves['effective_resolution'])} pixels, "
            f"{curves['n_counted']}/{curves['n_cases']} cases")


def _log10(values):
    return [math.log10(v) if v is not None and math.isfinite(v) and v > 0 else math.nan for v in values]


def write_page(folder, partitions):
    """<folder>/index.html.  partitions: [(partition, curves)] in page order.  Per partition four line plots over log10 of
    the wavelength: log10 psd of prediction and target, the power ratio, the coherence and the error share."""
    os.makedirs(folder, exist_ok=True)
    doc = Document("Power spectra")
    doc.head.add("style").text(STYLE)
    body = doc.body
    body.add("h2").text("Power spectra of prediction against target")
    body.add("p").text("Channel 0, Hann window, mean removed, radial bins of 1 / (2 M) cycles per pixel; over the cases "
                       "whose prediction and target are finite everywhere.")
    for (partition, curves) in partitions:
        er = curves["effective_resolution"]
        section = body.add("div", {"class": "spectra", "data-partition": partition})
        section.add("h3").text(f"{partition}: {curves['n_counted']} of {curves['n_cases']} cases, effective resolution "
                               + (f"{er:.4g} pixels" if er is not None else "not reached"))
        x = _log10(curves["wavelength"])
        plots = [("power spectral density", "log10 psd", {"prediction": (x, _log10(curves["psd_pred"])),
                                                          "target": (x, _log10(curves["psd_target"]))}),
                 ("power ratio", "prediction / target", {"power_ratio": (x, curves["power_ratio"])}),
                 ("coherence", "coherence", {"coherence": (x, curves["coherence"])}),
                 ("error share", "error / target", {"error_share": (x, curves["error_share"])})]
        for (title, ylabel, series) in plots:
            section.add("img", {"src": svg_data_uri(svg_lines(series, f"{partition} {title}", "log10 wavelength (pixels)", ylabel)),
                                "alt": f"{partition} {title}"})
    path = os.path.join(folder, "index.html")
    with open(path, "w") as f:
        f.write(doc.html())
    return path
