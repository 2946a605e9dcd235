"""Numpy restatement of the model comparison (include/cae_hip.h: cae_case_compare, cae_bootstrap_sums)
shared by test_compare_cpu.py and test_compare_gpu.py: the per-case sums with the bounds the kernel's results are held to,
the index generator, the sequential sums of the resamples, the units, and the statistics and interval ranks.

Comparison.  A pixel of a case is a pair when the target a and all M predictions P_m are finite.  e_m = P_m - a, q_m = e_m *
e_m in fp64, each rounded on its own.  Per case {n, tied, (S e_m, S|e_m|, S e_m^2, wins_m) per candidate}: candidate m wins
a pixel when q_m < q_j for every j != m; a pixel whose smallest q is attained more than once is tied.  n, tied and the wins
are integers, decided on the fp64 q as numpy rounds them, and are compared exactly.  Every other sum is formed here in
np.longdouble from the exact operands.

Bound on a floating-point sum of m terms t (u = 2^-53):  |got - want| <= (m + 4) u S|t|, the operation count of
importance_ref.py: a term |e| carries one rounding, a term e^2 three, adding m terms in any order m - 1 more, each at most u
of a partial sum that never exceeds S|t|; m + 4 leaves room for the second-order terms and this reference's own 2^-64
roundings.  S e is a sum of signed terms: its partial sums are bounded by S|e|, so it is held to (m + 4) u S|e| as well.  m is
the case's number of pairs.

Bootstrap.  Draw i of resample r takes unit j(r, i) = (u * n_unit) >> 32 with u the high 32 bits of output x + 1 of
splitmix64 seeded with `seed`, x = (r << 32) | i (units below).  T_r[c] starts at +0.0 and adds S[j(r, 0)][c], S[j(r, 1)][c],
... in that order with plain fp64 adds (sums below: a loop over i, vectorised over r), so the kernel's result is compared
with np.array_equal on the bits.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


class Reference:
    """the definition's sums of one operand set with their bounds, computed once and compared with many results.
    preds: a list of M arrays (N, H, W) or (N, plane), channel 0 of the predictions; actual: the target likewise"""

    def __init__(self, preds, actual):
        actual = np.asarray(actual).astype(np.float64)
        n = actual.shape[0]
        actual = actual.reshape(n, -1)
        preds = [np.asarray(p).astype(np.float64).reshape(n, -1) for p in preds]
        m = len(preds)
        pair = np.isfinite(actual)
        for p in preds:
            pair = pair & np.isfinite(p)
        z = lambda v: np.where(pair, v, 0.0)        # noqa: E731
        a = z(actual)
        ps = [z(p) for p in preds]
        with np.errstate(over="ignore", invalid="ignore"):
            q = np.stack([(p - a) * (p - a) for p in ps])            # fp64, every operation rounded on its own
        qmin = q.min(axis=0)
        hits = (q == qmin[None]).sum(axis=0)
        count = pair.sum(axis=1)
        self.pair = pair
        self.sums = np.zeros((n, 2 + 4 * m), dtype=LD)
        self.bound = np.zeros((n, 2 + 4 * m), dtype=LD)
        self.exact = [0, 1] + [5 + 4 * k for k in range(m)]
        self.sums[:, 0] = count
        self.sums[:, 1] = (pair & (hits > 1)).sum(axis=1)
        for k in range(m):
            e = ps[k].astype(LD) - a.astype(LD)
            (s_abs, s_sq) = (np.abs(e).sum(axis=1), (e * e).sum(axis=1))
            self.sums[:, 2 + 4 * k:5 + 4 * k] = np.stack([e.sum(axis=1), s_abs, s_sq], axis=1)
            self.bound[:, 2 + 4 * k:5 + 4 * k] = ((count + 4) * LD(U))[:, None] * np.stack([s_abs, s_abs, s_sq], axis=1)
            self.sums[:, 5 + 4 * k] = (pair & (hits == 1) & (q[k] == qmin)).sum(axis=1)

    def check(self, got, label="", cases=None):
        """the kernel's per-case rows against the definition (cases: the reference's cases that `got` holds, default all):
        n, tied and the wins exactly, the sums within their bounds, +0.0 in a case without a pair; prints and returns the
        largest |got - want| / bound"""
        got = np.asarray(got)
        sel = slice(None) if cases is None else cases
        (want, bound) = (self.sums[sel], self.bound[sel])
        assert got.shape == want.shape and got.dtype == np.float64, (got.shape, want.shape)
        np.testing.assert_array_equal(got[:, self.exact], want[:, self.exact].astype(np.float64), err_msg=f"{label}: counts")
        empty = want[:, 0] == 0
        assert (got[empty] == 0.0).all() and not np.signbit(got[empty]).any(), "a case without a pair holds +0.0"
        err = np.abs(got.astype(LD) - want)
        exact = bound == 0
        assert (err[exact] == 0).all(), "a sum whose bound is zero must be exact"
        ratio = float(np.max(np.where(exact, LD(0), err / np.where(exact, LD(1), bound)), initial=0.0))
        print(f"compare sums {label} {got.shape}: max |got - want| / bound = {ratio:.3e}")
        assert (err <= bound).all(), (label, ratio)
        return ratio


# ---- the bootstrap -------------------------------------------------------------------------------------------------------

def mix64(z):
    """splitmix64's output function on uint64 arrays (wrapping arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def units(n_unit, resamples, seed=0, first=0, draws=None):
    """(resamples, draws) int64: j(r, i) for r = first .. first + resamples - 1 and i = 0 .. draws - 1 (default n_unit)"""
    draws = n_unit if draws is None else draws
    r = (np.arange(resamples, dtype=np.uint64) + np.uint64(first))[:, None]
    i = np.arange(draws, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        x = (r << np.uint64(32)) | i
        z = mix64(np.uint64(seed & M64) + (x + np.uint64(1)) * np.uint64(GOLDEN))
    return ((z >> np.uint64(32)) * np.uint64(n_unit) >> np.uint64(32)).astype(np.int64)


def splitmix64(seed, count):
    """the first `count` outputs of the sequential splitmix64 generator seeded with seed, as Python ints"""
    (state, out) = (seed & M64, [])
    for _ in range(count):
        state = (state + GOLDEN) & M64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        out.append(z ^ (z >> 31))
    return out


def sums(table, resamples, seed=0, first=0):
    """(resamples, n_col) float64: T_r = S[j(r, 0)] + S[j(r, 1)] + ... from +0.0 in that order, plain fp64 adds"""
    table = np.asarray(table, dtype=np.float64)
    n_unit = table.shape[0]
    total = np.zeros((resamples, table.shape[1]), dtype=np.float64)
    r = (np.arange(resamples, dtype=np.uint64) + np.uint64(first)) << np.uint64(32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n_unit):
            z = mix64(np.uint64(seed & M64) + ((r | np.uint64(i)) + np.uint64(1)) * np.uint64(GOLDEN))
            j = ((z >> np.uint64(32)) * np.uint64(n_unit) >> np.uint64(32)).astype(np.int64)
            total = total + table[j]
    return total


# ---- units, ranks, statistics ----------------------------------------------------------------------------------------------

def block_units(rows, block):
    """the units' table: the rows of the cases of equal block value added in ascending case order, units by first appearance"""
    (order, table) = ([], {})
    for (row, v) in zip(np.asarray(rows, dtype=np.float64), list(block)):
        if v not in table:
            order.append(v)
            table[v] = np.zeros(row.shape, dtype=np.float64)
        table[v] = table[v] + row
    return np.stack([table[v] for v in order])


def ranks(n, confidence):
    """(k, n + 1 - k) with k = ceil(n (1 - c) / 2), c an exact Fraction"""
    x = n * (1 - Fraction(confidence)) / 2
    k = -((-x.numerator) // x.denominator)
    return k, n + 1 - k


def interval(values, confidence):
    """(lo, hi, degenerate): the order statistics of `ranks` among the finite values"""
    v = np.sort(np.asarray(values, dtype=np.float64)[np.isfinite(values)])
    (k, upper) = ranks(v.size, confidence)
    return float(v[k - 1]), float(v[upper - 1]), int(np.size(values) - v.size)


def mse(sums, k):
    """mse of candidate k from rows of 2 + 4 M sums"""
    sums = np.asarray(sums, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums[..., 4 + 4 * k] / sums[..., 0]
