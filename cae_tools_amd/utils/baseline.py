"""Skill against interpolating the input: the host side of engine.case_baseline (cae_case_baseline, include/cae_hip.h).
The scores formed from its per-case sums - the baseline's mse and mae, the model's mse on the same pixels, the skill
1 - model_mse / baseline_mse and the share of pixels the model wins - their summary over a partition, and the writers:
baseline_<partition>.json, the printed line and the rows of the report's "Skill against interpolation" section.
DESIGN.md section 9 holds the definition of the interpolation and the counting rule.

Host only: standard library and numpy.
"""
import numpy as np

from . import records
from .records import ratio as _ratio, shown as _shown

MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}        # CAE_INTERP_* of include/cae_hip.h


def scores_from_sums(sums):
    """The per-case scores from engine.case_baseline's (N, 6) sums {n, S|b - a|, S(b - a)^2, S|p - a|, S(p - a)^2, n_won},
    as a dict of (N,) float64 arrays:
        baseline_mae   S|b - a| / n          baseline_mse   S(b - a)^2 / n
        model_mae      S|p - a| / n          model_mse      S(p - a)^2 / n      on the same pixels
        skill          1 - model_mse / baseline_mse
        win_fraction   n_won / n
    each NaN where its denominator is 0, and "pixels", the (N,) int64 counts n."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 6)
    n = sums[:, 0]
    scores = {"baseline_mae": _ratio(sums[:, 1], n), "baseline_mse": _ratio(sums[:, 2], n),
              "model_mae": _ratio(sums[:, 3], n), "model_mse": _ratio(sums[:, 4], n)}
    scores["skill"] = 1.0 - _ratio(sums[:, 4], sums[:, 2])
    scores["win_fraction"] = _ratio(sums[:, 5], n)
    scores["pixels"] = n.astype(np.int64)
    return scores


def summary(sums, mode, variable, in_shape, out_shape):
    """one partition's record from the (N, 6) sums: mode, variable, in_shape, out_shape, n_cases, n_counted (cases with a
    skill), pixels_counted and pixels_left_out, pooled_skill = 1 - SS(p - a)^2 / SS(b - a)^2 over all counted pixels, the
    pooled baseline_mse, baseline_mae and model_mse, mean_skill, median_skill and skill_positive (the share of the cases
    with a skill whose skill > 0), win_fraction (pooled), and the per-case arrays case_skill, case_baseline_mse,
    case_baseline_mae, case_model_mse, case_win_fraction and case_pixels.  What has no denominator is NaN."""
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 6)
    scores = scores_from_sums(sums)
    total = sums.sum(axis=0) if sums.shape[0] else np.zeros(6)
    pooled = scores_from_sums(total[None, :])
    skill = scores["skill"]
    have = ~np.isnan(skill)
    n_cases = int(sums.shape[0])
    plane = int(out_shape[0]) * int(out_shape[1])
    return {"mode": str(mode), "variable": str(variable), "in_shape": [int(v) for v in in_shape],
            "out_shape": [int(v) for v in out_shape], "n_cases": n_cases, "n_counted": int(have.sum()),
            "pixels_counted": int(total[0]), "pixels_left_out": n_cases * plane - int(total[0]),
            "pooled_skill": float(pooled["skill"][0]), "baseline_mse": float(pooled["baseline_mse"][0]),
            "baseline_mae": float(pooled["baseline_mae"][0]), "model_mse": float(pooled["model_mse"][0]),
            "mean_skill": records.stat(skill, np.mean), "median_skill": records.stat(skill, np.median),
            "skill_positive": float(np.sum(skill[have] > 0)) / float(have.sum()) if have.any() else float("nan"),
            "win_fraction": float(pooled["win_fraction"][0]),
            "case_skill": skill.tolist(), "case_baseline_mse": scores["baseline_mse"].tolist(),
            "case_baseline_mae": scores["baseline_mae"].tolist(), "case_model_mse": scores["model_mse"].tolist(),
            "case_win_fraction": scores["win_fraction"].tolist(), "case_pixels": scores["pixels"].tolist()}


def json_record(record):
    """the record as strict JSON values: a number that is not finite becomes null"""
    return records.json_record(record, (list, tuple))


def write_json(path, record):
    """baseline_<partition>.json"""
    return records.write_json(path, json_record(record))


def line(partition, record):
    """baseline <partition>: <mode> of <variable>, pooled skill <x> (baseline mse <y>, model mse <z>), <k>/<n> cases better"""
    better = int(np.sum(np.asarray([v for v in record["case_skill"] if v is not None], dtype=np.float64) > 0))
    return (f"baseline {partition}: {record['mode']} of {record['variable']}, pooled skill {_shown(record['pooled_skill'])} "
            f"(baseline mse {_shown(record['baseline_mse'])}, model mse {_shown(record['model_mse'])}), "
            f"{better}/{record['n_cases']} cases better")


SECTION_ROWS = (("pooled skill", "pooled_skill"), ("mean per-case skill", "mean_skill"), ("median per-case skill", "median_skill"),
                ("share of cases with skill > 0", "skill_positive"), ("baseline mse", "baseline_mse"),
                ("baseline mae", "baseline_mae"), ("model mse on the same pixels", "model_mse"),
                ("share of pixels the model wins", "win_fraction"))


def section_rows(record):
    """the rows of the report's table: [[name, value]] with "none" for a value that does not exist"""
    rows = [["Score Name", "Score Value"]] + [[label, _shown(float(record[key]))] for (label, key) in SECTION_ROWS]
    rows.append(["pixels counted / left out", f"{record['pixels_counted']} / {record['pixels_left_out']}"])
    return rows
