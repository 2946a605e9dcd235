"""Structural similarity of prediction against target per case: the host side of engine.case_ssim (cae_case_ssim,
include/cae_hip.h).  The window and the scale shapes the kernel works with, the scores formed from its sums - SSIM,
MS-SSIM and, from cae_case_measures' mse, PSNR - and their writers: ssim_<partition>.json and the data of the report's
"Structural similarity" section.  DESIGN.md section 9 holds the definition; it is the VAE loss's (oracle/vae_oracle.py),
so the MS-SSIM of a `--method var` model is the quantity it was trained on.

Host only: standard library and numpy.
"""
import functools

import numpy as np

from . import records

WIN_SIZE = 11
MAX_SCALES = 5
MS_MIN_SIDE = 160            # MS-SSIM is defined for min(h, w) > 160 (pytorch_msssim's condition: (11 - 1) * 2^4)

# The window is data of the definition: the eleven fp32 values of exp(-c^2 / 4.5) / sum as torch evaluates them
# (kernels_vae.h make_gauss holds the same bits), cast to double.  Recomputing them in fp64 would be another window.
_HALF = ("0x1.0d957p-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2")
# the scale weights of Wang et al. 2003 as fp32 values, cast up
MS_WEIGHTS = tuple(float(v) for v in np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=np.float32))


def window():
    """(11,) float64: the window's fp32 values cast to double"""
    half = [float.fromhex(v) for v in _HALF]
    return np.array(half + half[-2::-1], dtype=np.float64)


def pooled(side):
    """the side of the next scale: 2 x 2 pooling with padding side mod 2 on both sides"""
    side = int(side)
    return (side + 2 * (side % 2)) // 2


def scale_shapes(h, w, n_scale):
    """[(h_s, w_s)] for s in [0, n_scale)"""
    shapes = []
    for _ in range(int(n_scale)):
        shapes.append((int(h), int(w)))
        (h, w) = (pooled(h), pooled(w))
    return shapes


def default_scales(h, w):
    """5 where MS-SSIM is defined (min(h, w) > 160), else 1: SSIM alone"""
    return MAX_SCALES if min(int(h), int(w)) > MS_MIN_SIDE else 1


def scores_from_sums(sums, h, w, mse=None, vmin=0.0, vmax=1.0):
    """The per-case scores from engine.case_ssim's (N, n_scale, 3) sums {n, S ssim, S cs}, as a dict of (N,) float64 arrays:
        ssim      S ssim_0 / n_0, NaN where n_0 == 0
        ms_ssim   prod_{s<4} relu(S cs_s / n_s)^w_s * relu(S ssim_4 / n_4)^w_4 where min(h, w) > 160, the sums hold five
                  scales and all five n_s > 0; NaN otherwise
        psnr      10 log10((vmax - vmin)^2 / mse) from the per-case mse (engine.case_measures), +inf at mse == 0, NaN where
                  the mse is NaN or negative; all NaN without an mse
    and "windows", the (N, n_scale) int64 window counts."""
    sums = np.asarray(sums, dtype=np.float64)
    (n_case, n_scale) = (sums.shape[0], sums.shape[1])
    (n, s_ssim, s_cs) = (sums[:, :, 0], sums[:, :, 1], sums[:, :, 2])
    some = n > 0
    safe = np.where(some, n, 1.0)
    mean_ssim = np.where(some, s_ssim / safe, np.nan)
    mean_cs = np.where(some, s_cs / safe, np.nan)
    ssim = mean_ssim[:, 0].copy() if n_scale else np.full(n_case, np.nan)
    ms = np.full(n_case, np.nan)
    if n_scale == MAX_SCALES and min(int(h), int(w)) > MS_MIN_SIDE:
        terms = np.concatenate([mean_cs[:, :MAX_SCALES - 1], mean_ssim[:, MAX_SCALES - 1:]], axis=1)
        ok = some.all(axis=1)
        prod = np.ones(n_case)
        for s in range(MAX_SCALES):
            prod = prod * np.maximum(np.where(ok, terms[:, s], 0.0), 0.0) ** MS_WEIGHTS[s]
        ms = np.where(ok, prod, np.nan)
    psnr = np.full(n_case, np.nan)
    if mse is not None:
        mse = np.asarray(mse, dtype=np.float64).reshape(n_case)
        peak = (float(vmax) - float(vmin)) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            psnr = np.where(mse == 0, np.inf, np.where(mse > 0, 10.0 * np.log10(peak / np.where(mse > 0, mse, 1.0)), np.nan))
    return {"ssim": ssim, "ms_ssim": ms, "psnr": psnr, "windows": n.astype(np.int64)}


def summary(scores, h, w, vmin, vmax):
    """one partition's record: n_cases, h, w, vmin, vmax, the scales' shapes, n_counted (cases with an ssim) and
    n_counted_ms (cases with an ms_ssim), the means of ssim, ms_ssim and psnr over the cases that have the score, and the
    per-case arrays case_ssim, case_ms_ssim, case_psnr and windows"""
    n_scale = int(scores["windows"].shape[1])
    return {"n_cases": int(scores["ssim"].shape[0]), "h": int(h), "w": int(w), "vmin": float(vmin), "vmax": float(vmax),
            "scales": [list(s) for s in scale_shapes(h, w, n_scale)],
            "n_counted": int(np.sum(~np.isnan(scores["ssim"]))), "n_counted_ms": int(np.sum(~np.isnan(scores["ms_ssim"]))),
            "ssim": records.stat(scores["ssim"]), "ms_ssim": records.stat(scores["ms_ssim"]), "psnr": records.stat(scores["psnr"]),
            "case_ssim": scores["ssim"].tolist(), "case_ms_ssim": scores["ms_ssim"].tolist(),
            "case_psnr": scores["psnr"].tolist(), "windows": scores["windows"].tolist()}


def json_record(record):
    """the record as strict JSON values: a number that is not finite becomes null"""
    return records.json_record(record, (list, tuple))


def write_json(path, record):
    """ssim_<partition>.json"""
    return records.write_json(path, json_record(record))


_shown = functools.partial(records.shown, minus_inf="none")         # no score of this module is -inf


def line(partition, record):
    """ssim <partition>: ssim <x> ms_ssim <y|none> psnr <z> dB, <n_counted>/<n> cases"""
    return (f"ssim {partition}: ssim {_shown(record['ssim'])} ms_ssim {_shown(record['ms_ssim'])} "
            f"psnr {_shown(record['psnr'])} dB, {record['n_counted']}/{record['n_cases']} cases")


SECTION_ROWS = (("ssim", "ssim"), ("ms_ssim", "ms_ssim"), ("psnr (dB)", "psnr"))


def section_rows(record):
    """the rows of the report's table of means: [[name, value]] with "none" for a mean that does not exist"""
    return [["Score Name", "Score Value"]] + [[label, _shown(float(record[key]))] for (label, key) in SECTION_ROWS]
