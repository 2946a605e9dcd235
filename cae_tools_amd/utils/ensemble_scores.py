"""Ensemble scores from the sums of cae_ensemble_verify (include/cae_hip.h): pure numpy, no GPU.

case_sums is (N, 5) float64, {n, S A, S B, S (mbar - a)^2, S s^2} per case over its counted pixels, with per pixel
A = mean_k |m_k - a| and B = (1/K^2) S_{i<j} |m_i - m_j|; rank_counts is (K + 2,) int64: the histogram of the target's rank
below = #{k: m_k < a} in bins 0 .. K (a tied pixel counted at its lowest rank) and the number of tied pixels in bin K + 1."""
import numpy as np

from . import records

SUM_NAMES = ("n", "abs_error", "pair_distance", "squared_error_of_mean", "variance")


def case_crps(case_sums):
    """per-case crps_c = (A_c - B_c) / n_c, NaN where the case has no counted pixel"""
    sums = np.asarray(case_sums, dtype=np.float64).reshape(-1, 5)
    (n, a, b) = (sums[:, 0], sums[:, 1], sums[:, 2])
    out = np.full(n.shape, np.nan)
    np.divide(a - b, n, out=out, where=n > 0)
    return out


def scores_from_sums(case_sums, rank_counts, k):
    """The scores of a K-member ensemble from the sums over all cases: a dict of
    n, crps = (A - B) / n (which is the MAE for one member), fair_crps = (A - B * K / (K - 1)) / n (unbiased in K),
    rmse_mean = sqrt(E / n) of the ensemble mean, spread = sqrt(V / n), spread_skill = sqrt((K + 1) / K) * spread / rmse_mean
    (1 for a calibrated ensemble), rank_frequencies (K + 1 values summing to 1), tied_fraction, and the per-case crps.
    With n = 0 every score is NaN."""
    k = int(k)
    if k < 2:
        raise ValueError("an ensemble has at least 2 members")
    sums = np.asarray(case_sums, dtype=np.float64).reshape(-1, 5)
    ranks = np.asarray(rank_counts, dtype=np.int64).reshape(-1)
    if ranks.size != k + 2:
        raise ValueError(f"rank_counts must hold K + 2 = {k + 2} counts, got {ranks.size}")
    (n, a, b, e, v) = (float(t) for t in sums.sum(axis=0))
    nan = float("nan")
    if n > 0:
        rmse_mean = float(np.sqrt(e / n))
        spread = float(np.sqrt(v / n))
        scores = {"crps": (a - b) / n, "fair_crps": (a - b * k / (k - 1)) / n, "rmse_mean": rmse_mean, "spread": spread,
                  "spread_skill": float(np.sqrt((k + 1) / k)) * spread / rmse_mean if rmse_mean > 0 else nan}
    else:
        scores = {"crps": nan, "fair_crps": nan, "rmse_mean": nan, "spread": nan, "spread_skill": nan}
    counted = int(ranks[:k + 1].sum())
    freq = ranks[:k + 1] / counted if counted > 0 else np.full(k + 1, np.nan)
    return {"n": int(n), "ensemble_size": k, **scores, "rank_counts": [int(c) for c in ranks[:k + 1]],
            "rank_frequencies": [float(f) for f in freq], "tied": int(ranks[k + 1]),
            "tied_fraction": int(ranks[k + 1]) / counted if counted > 0 else nan, "case_crps": case_crps(sums)}


def json_record(scores, skip=()):
    """the scores as a dict that json.dump(..., allow_nan=False) takes: arrays become lists, numpy numbers Python's, and a
    value that is not finite (every score of a partition without a counted pixel, the crps of such a case) becomes None,
    JSON's null - strict JSON has no NaN token.  Keys in `skip` are left out."""
    return records.json_record({key: v for (key, v) in scores.items() if key not in skip}, (list, tuple, np.ndarray))


def write_json(path, scores):
    """ensemble_<partition>.json"""
    return records.write_json(path, json_record(scores))
