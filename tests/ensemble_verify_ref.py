"""The fp64 numpy definition of cae_ensemble_verify (include/cae_hip.h): brute force over all pairs, no
sort, so it shares no algorithm with the kernel.  Every operation is one numpy operation, rounded on its own."""
import numpy as np


def members(y, vmin, rng):
    """m = vmin + (double)y * range: the multiply and the add each rounded on its own"""
    t = np.asarray(y, dtype=np.float32).astype(np.float64) * np.float64(rng)
    return np.float64(vmin) + t


def pixel_terms(y, a, vmin, rng):
    """y (K, P) fp32 draws and a (P,) targets of one case -> dict of per-pixel arrays (P,): counted (bool), A, B, E = (mbar -
    a)^2, V = s^2, below (int), tied (bool), and the absolute sums absA .. absV of the terms that enter each (for bounds)"""
    y = np.asarray(y, dtype=np.float32)
    a = np.asarray(a).astype(np.float64)
    k = y.shape[0]
    y64 = y.astype(np.float64)
    counted = np.isfinite(a) & np.isfinite(y64).all(axis=0)
    with np.errstate(all="ignore"):
        m = members(y, vmin, rng)
        sa = np.zeros(a.shape)
        for i in range(k):                      # ascending draw order
            sa = sa + np.abs(m[i] - a)
        sb = np.zeros(a.shape)
        for i in range(k):
            for j in range(i):
                sb = sb + np.abs(m[i] - m[j])
        (s1, s2) = (np.zeros(a.shape), np.zeros(a.shape))
        for i in range(k):
            d = y64[i] - y64[0]
            s1 = s1 + d
            s2 = s2 + d * d
        kd = np.float64(k)
        mbar = np.float64(vmin) + (y64[0] + s1 / kd) * np.float64(rng)
        var = (s2 - s1 * s1 / kd) / (kd - 1.0)
        e = (mbar - a) * (mbar - a)
        v = np.where(var < 0.0, 0.0, var) * np.float64(rng) * np.float64(rng)
        below = (m < a).sum(axis=0)
        tied = (m == a).any(axis=0)
    return {"counted": counted, "A": sa / kd, "B": sb / (kd * kd), "E": e, "V": v, "below": below, "tied": tied, "mbar": mbar}


def verify(y, a, vmin, rng):
    """y (N, K, P) fp32, a (N, P): (case_sums (N, 5), rank_counts (K + 2,) int64, terms per case)"""
    (n_case, k, _) = y.shape
    sums = np.zeros((n_case, 5))
    ranks = np.zeros(k + 2, dtype=np.int64)
    all_terms = []
    for c in range(n_case):
        t = pixel_terms(y[c], a[c], vmin, rng)
        w = t["counted"]
        sums[c] = [w.sum(), t["A"][w].sum(), t["B"][w].sum(), t["E"][w].sum(), t["V"][w].sum()]
        ranks[:k + 1] += np.bincount(t["below"][w], minlength=k + 1)
        ranks[k + 1] += int((t["tied"] & w).sum())
        all_terms.append(t)
    return sums, ranks, all_terms
