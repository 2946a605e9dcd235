"""Numpy restatement of cae_strata_sums (include/cae_hip.h) shared by test_strata_cpu.py and
test_strata_gpu.py: the source pixel of the stratifier for every target pixel, the stratum of a value, the three counts and
the eight sums of the pairs of every stratum, in fp64.

The source row of output row y is min(floor((y + 0.5) * (sh / h)), sh - 1) with the ratio divided once and the sum and the
product each rounded on their own (numpy contracts nothing), columns likewise; the stratum of a finite value is
np.searchsorted(edges, v, side="right"), the number of edges at or below it.  The addends are formed term by term - d = p - a,
a' = a - shift_a[k], p' = p - shift_p[k], then |d|, d * d, a' * a', p' * p', a' * p' - and every sum is math.fsum, the correctly
rounded sum.  With it comes the bound of any order of summation, c u S|x_i| per stratum and sum with c the stratum's pair
count and u = 2^-53: the derivation is in distribution_ref.py.  A sum with an addend that is not finite (1e300 squared) has
no bound: it is compared for equality, NaN equal to NaN."""
import math

import numpy as np

from distribution_ref import U

SUMS = 8


def source_index(n_out, n_in):
    """the source index of every output index 0 .. n_out - 1 on an axis of n_in samples"""
    ratio = np.float64(n_in) / np.float64(n_out)
    i = np.floor((np.arange(n_out, dtype=np.float64) + 0.5) * ratio).astype(np.int64)
    return np.minimum(i, n_in - 1)


def on_target_grid(s, h, w):
    """the stratifier planes s (N, sh, sw) read at the source pixel of every target pixel: (N, h, w)"""
    s = np.asarray(s)
    return s[:, source_index(h, s.shape[1])[:, None], source_index(w, s.shape[2])[None, :]]


def strata_of(v, edges):
    """the stratum of every finite value of v"""
    return np.searchsorted(np.asarray(edges, dtype=np.float64), np.asarray(v, dtype=np.float64), side="right")


def _fsum(x):
    """(the sum, S|x_i|): math.fsum of finite addends; what IEEE addition gives in any order where one is not finite"""
    if np.isfinite(x).all():
        return math.fsum(x), math.fsum(np.abs(x))
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.sum(x)), math.inf


class Reference:
    """members (n_strata,), pairs (n_strata,), unclassified, sums (n_strata, 8) and bound (n_strata, 8) of prediction p and
    target a (N, h, w) under the stratifier s (N, sh, sw) as cae_strata_sums defines them; shift: one number or (2, n_strata)"""

    def __init__(self, p, a, s, edges, shift=0.0):
        (p, a, s) = (np.asarray(p, dtype=np.float64), np.asarray(a, dtype=np.float64), np.asarray(s, dtype=np.float64))
        edges = np.asarray(edges, dtype=np.float64).reshape(-1)
        n_strata = edges.size + 1
        shift = np.broadcast_to(np.asarray(shift, dtype=np.float64), (2, n_strata))
        (n, h, w) = a.shape
        v = on_target_grid(s, h, w).reshape(-1) if n * h * w else np.zeros(0)
        (p, a) = (p.reshape(-1), a.reshape(-1))
        cls = np.isfinite(v)
        k = np.where(cls, strata_of(np.where(cls, v, 0.0), edges), -1)
        pair = cls & np.isfinite(p) & np.isfinite(a)
        self.n_strata = n_strata
        self.pixels = n * h * w
        self.unclassified = int((~cls).sum())
        self.members = np.bincount(k[cls], minlength=n_strata).astype(np.int64)
        self.pairs = np.bincount(k[pair], minlength=n_strata).astype(np.int64)
        self.sums = np.zeros((n_strata, SUMS))
        self.bound = np.zeros((n_strata, SUMS))
        for j in range(n_strata):
            at = pair & (k == j)
            with np.errstate(over="ignore", invalid="ignore"):
                d = p[at] - a[at]
                a1 = a[at] - shift[0, j]
                p1 = p[at] - shift[1, j]
                addends = (d, np.abs(d), d * d, a1, p1, a1 * a1, p1 * p1, a1 * p1)
            for (q, x) in enumerate(addends):
                (total, mag) = _fsum(x)
                self.sums[j, q] = total
                self.bound[j, q] = int(self.pairs[j]) * U * mag
