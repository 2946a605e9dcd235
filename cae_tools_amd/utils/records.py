"""What the evaluation records of utils/ssim.py, baseline.py, distribution.py, spectra.py and ensemble_scores.py share: their
values as strict JSON, the file writer, the printed form of a score, and the two statistics that leave out what has no value.

Host only: standard library and numpy.
"""
import json
import math

import numpy as np


def strict(v, descend=(dict, list, tuple, np.ndarray)):
    """v as strict JSON values: a float that is not finite becomes None (JSON's null; strict JSON has no NaN token), numpy
    numbers become Python's, and the containers named in `descend` are gone through (an array as its list)."""
    if isinstance(v, descend):
        if isinstance(v, dict):
            return {k: strict(x, descend) for (k, x) in v.items()}
        return [strict(x, descend) for x in (v.tolist() if isinstance(v, np.ndarray) else v)]
    if isinstance(v, (float, np.floating)):
        return float(v) if math.isfinite(v) else None
    if isinstance(v, np.integer):
        return int(v)
    return v


def json_record(record, descend=(dict, list, tuple, np.ndarray)):
    """the values of a record made strict, key by key"""
    return {k: strict(v, descend) for (k, v) in record.items()}


def write_json(path, record):
    """the strict record as a JSON file; returns the path"""
    with open(path, "w") as f:
        json.dump(record, f, indent=1, allow_nan=False)
    return path


def shown(v, minus_inf="-inf"):
    """a score as a line or a table shows it: six significant digits, "inf", "none" for NaN and None"""
    if v is None:
        return "none"
    v = float(v)
    return format(v, ".6g") if math.isfinite(v) else ("inf" if v == math.inf else (minus_inf if v == -math.inf else "none"))


def ratio(num, den):
    """num / den, NaN where den is 0"""
    (num, den) = (np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64))
    some = den != 0
    return np.where(some, num / np.where(some, den, 1.0), np.nan)


def stat(values, fn=np.mean):
    """fn over the values that are not NaN, NaN without one"""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    return float(fn(v)) if v.size else float("nan")
