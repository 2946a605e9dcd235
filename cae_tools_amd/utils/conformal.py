"""Split conformal prediction intervals (DESIGN.md section 9 'prediction intervals'): the host side of BaseModel.calibrate and
apply(interval=...).  Coverage levels as exact rationals, the rank rule, the calibration record of a model folder
(calibration.json, and calibration.nc for the pixel group) and the printed summary.  The quantiles themselves are
case_ops.score_quantiles (cae_score_quantiles, include/cae_hip.h).

Host only: standard library, numpy and the project's NetCDF-3 reader and writer.
"""
import json
import math
import os
from fractions import Fraction

import numpy as np

from . import records

GROUPS = {"pixel": 0, "pooled": 1}
MAX_LEVELS = 8
MAX_DEN = 10 ** 6
DEFAULT_LEVELS = ("0.8", "0.9", "0.95")
RECORD_FILE = "calibration.json"
MAP_FILE = "calibration.nc"


def parse_level(text):
    """One coverage level as the exact Fraction of its decimal (or "num/den") text; it never passes through a float, so 0.9
    is 9/10.  A Fraction or an int is taken as it is; a float is refused, its text is what was meant.  0 < level < 1 with a
    denominator of at most 10^6."""
    if isinstance(text, float):
        raise ValueError(f"coverage level {text!r}: give the decimal text or a Fraction, a float has already lost it")
    try:
        level = Fraction(text.strip()) if isinstance(text, str) else Fraction(text)
    except (ValueError, ZeroDivisionError, TypeError, AttributeError):
        raise ValueError(f"coverage level {text!r} is not a number") from None
    if not 0 < level < 1:
        raise ValueError(f"coverage level {text!r} is not between 0 and 1")
    if level.denominator > MAX_DEN:
        raise ValueError(f"coverage level {text!r} needs a denominator above {MAX_DEN}")
    return level


def parse_levels(texts):
    """1 to 8 strictly ascending coverage levels as Fractions (parse_level)"""
    levels = [parse_level(t) for t in ([texts] if isinstance(texts, (str, Fraction)) else list(texts))]
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f"1 to {MAX_LEVELS} coverage levels expected, got {len(levels)}")
    if any(b <= a for (a, b) in zip(levels, levels[1:])):
        raise ValueError(f"coverage levels must be strictly ascending, got {', '.join(level_text(v) for v in levels)}")
    return levels


def level_text(level):
    """a level as the record stores it: "num/den" """
    return f"{level.numerator}/{level.denominator}"


def rank(n, level):
    """the split-conformal rank ceil((n + 1) level) in integers, as the kernel forms it; the quantile is finite iff rank <= n"""
    return ((int(n) + 1) * level.numerator + level.denominator - 1) // level.denominator


def check_group(group):
    if group not in GROUPS:
        raise ValueError(f"group must be one of {', '.join(GROUPS)}, got {group!r}")
    return group


def make_record(group, levels, output_variable, scale_variable, n_cases, q, n, pooled_q, coverage=None):
    """The calibration of a model as calibration.json stores it.  q: (L, G) float64 and n: (G,) int64 of the group calibrated
    with; pooled_q: (L,) the pooled quantiles, kept for either group; coverage: None or (count (L,), n) of a held-out set."""
    n = np.asarray(n, dtype=np.int64).reshape(-1)
    q = np.asarray(q, dtype=np.float64).reshape(len(levels), -1)
    record = {"group": check_group(group), "levels": [level_text(v) for v in levels], "output_variable": output_variable,
              "scale_variable": scale_variable, "cases": int(n_cases), "groups": int(n.size),
              "n_min": int(n.min()) if n.size else 0, "n_median": float(np.median(n)) if n.size else 0.0,
              "n_max": int(n.max()) if n.size else 0,
              "finite_groups": [int(np.isfinite(row).sum()) for row in q],
              "median_q": [float(np.median(row)) if row.size else math.inf for row in q],
              "pooled_quantiles": [float(v) for v in np.asarray(pooled_q, dtype=np.float64).reshape(-1)]}
    if coverage is not None:
        (count, total) = coverage
        record["test_pairs"] = int(total)
        record["test_covered"] = [int(c) for c in count]
        record["test_coverage"] = [int(c) / int(total) if int(total) else math.nan for c in count]
    return record


def write_record(folder, record, q=None, n=None, shape=None):
    """calibration.json into the model folder, and for the pixel group calibration.nc: quantile(level, y, x) float64 with
    +inf kept and count(y, x).  A calibration.nc left by an earlier pixel calibration is removed when the group is pooled.
    Returns the paths written."""
    paths = [records.write_json(os.path.join(folder, RECORD_FILE), records.json_record(record))]
    map_path = os.path.join(folder, MAP_FILE)
    if record["group"] == "pixel":
        from ..data import netcdf3
        (h, w) = (int(shape[0]), int(shape[1]))
        levels = len(record["levels"])
        netcdf3.write(map_path, {"level": levels, "y": h, "x": w},
                      {"quantile": (("level", "y", "x"), np.asarray(q, dtype=np.float64).reshape(levels, h, w), {}),
                       "count": (("y", "x"), np.asarray(n, dtype=np.int64).reshape(h, w), {})})
        paths.append(map_path)
    elif os.path.exists(map_path):
        os.remove(map_path)
    return paths


def read_record(folder):
    """The calibration of a model folder: the record of calibration.json with "levels" as Fractions and "pooled_quantiles" as
    floats (+inf where the file has null), and for the pixel group "quantile" (L, H, W) float64 and "count" (H, W) from
    calibration.nc.  A folder without one raises FileNotFoundError."""
    path = os.path.join(folder, RECORD_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{folder} holds no {RECORD_FILE}: calibrate the model first (python -m cae_tools_amd.cli.calibrate)")
    with open(path) as f:
        record = json.load(f)
    record["levels"] = [Fraction(t) for t in record["levels"]]
    for key in ("pooled_quantiles", "median_q"):
        record[key] = [math.inf if v is None else float(v) for v in record.get(key, [])]
    if record["group"] == "pixel":
        from ..data import netcdf3
        with netcdf3.File(os.path.join(folder, MAP_FILE)) as f:
            record["quantile"] = np.array(f.variables["quantile"].data, dtype=np.float64)
            record["count"] = np.array(f.variables["count"].data, dtype=np.int64)
    return record


def interval_request(folder, interval, scale_variable=None, interval_variables=None, prediction_variable="model_output"):
    """What apply(interval=...) needs, checked against the folder's calibration on the host alone: (record, index of the level,
    (lower name, upper name)).  The level must be one that was calibrated, as an exact Fraction, and the scale variable the
    calibrated one."""
    level = parse_level(interval)
    record = read_record(folder)
    if level not in record["levels"]:
        raise ValueError(f"coverage level {level_text(level)} was not calibrated: {folder} holds "
                         f"{', '.join(level_text(v) for v in record['levels'])}")
    if scale_variable != record.get("scale_variable"):
        raise ValueError(f"scale variable {scale_variable!r} differs from the calibrated one, {record.get('scale_variable')!r}")
    if interval_variables is None:
        names = (prediction_variable + "_lower", prediction_variable + "_upper")
    else:
        names = tuple(interval_variables)
        if len(names) != 2 or names[0] == names[1] or prediction_variable in names:
            raise ValueError(f"interval_variables must be two distinct names other than the prediction's, got {interval_variables!r}")
    return record, record["levels"].index(level), names


def summary_lines(record):
    """one line per level: level, group, finite groups / groups, median q, and the held-out coverage when there is one"""
    lines = []
    for (i, level) in enumerate(record["levels"]):
        text = level if isinstance(level, str) else level_text(level)
        line = (f"calibrate {text} {record['group']}: {record['finite_groups'][i]}/{record['groups']} groups finite, "
                f"median q {records.shown(record['median_q'][i])}")
        if "test_coverage" in record:
            line += f", held-out coverage {record['test_covered'][i]}/{record['test_pairs']} = {records.shown(record['test_coverage'][i])}"
        lines.append(line)
    return lines
