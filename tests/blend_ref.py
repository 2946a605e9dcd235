"""Numpy restatement of the model blending (include/cae_hip.h: cae_case_error_moments, cae_blend_predictions; DESIGN.md section
9, "Model blending") shared by test_blend_cpu.py and test_blend_gpu.py: the per-case rows of moments with the bounds the
kernel's results are held to, the blend as a numpy loop, the solver of the weights in fractions.Fraction, and the bound of the
end-to-end check.

Moments.  A pixel of a case is a pair when the target a and all M predictions P_m are finite.  e_m = P_m - a in fp64.  Per case
{n, S e_m (M of them), S e_i e_j for i <= j in row-major order}.  n is an integer and is compared exactly.  Every other sum is
formed here in np.longdouble from the exact operands.

Bound on a floating-point sum of m terms t (u = 2^-53), compare_ref.py's:  |got - want| <= (m + 4) u S|t|.  A term e carries
one rounding, a term e_i e_j three, adding m terms in any order m - 1 more, each at most u of a partial sum that never exceeds
S|t|; m + 4 leaves room for the second-order terms and this reference's own 2^-64 roundings.  m is the case's number of pairs.

Blend.  y = c; for m ascending over the candidates with w_m != 0: y = y + w_m * P_m, every operation a rounded fp64 numpy
operation; NaN where such a candidate is not finite.  The kernel's field is compared with assert_array_equal.

Solver.  The package's rule in exact arithmetic: the supports by increasing size, then lexicographically; the KKT system [2 E_SS
1; 1' 0] [w; l] = [0; 1] of each; a singular one skipped; a weight <= 0 infeasible; a later support kept only when its
objective is strictly lower.
"""
import itertools
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def width(m):
    return 1 + m + m * (m + 1) // 2


def pairs(m):
    """(i, j) for i <= j in row-major order"""
    return [(i, j) for i in range(m) for j in range(i, m)]


class Reference:
    """the definition's rows of one operand set with their bounds, computed once and compared with many results.
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
        a = np.where(pair, actual, 0.0).astype(LD)
        e = [np.where(pair, p, 0.0).astype(LD) - a for p in preds]
        count = pair.sum(axis=1)
        self.pair = pair
        self.m = m
        self.sums = np.zeros((n, width(m)), dtype=LD)
        self.bound = np.zeros((n, width(m)), dtype=LD)
        self.magnitude = np.zeros((n, width(m)), dtype=LD)       # S|t| of every column
        self.sums[:, 0] = count
        scale = (count + 4) * LD(U)
        for k in range(m):
            self.sums[:, 1 + k] = e[k].sum(axis=1)
            self.magnitude[:, 1 + k] = np.abs(e[k]).sum(axis=1)
        for (col, (i, j)) in enumerate(pairs(m)):
            t = e[i] * e[j]
            self.sums[:, 1 + m + col] = t.sum(axis=1)
            self.magnitude[:, 1 + m + col] = np.abs(t).sum(axis=1)
        self.bound = scale[:, None] * self.magnitude

    def check(self, got, label="", cases=None):
        """the kernel's per-case rows against the definition (cases: the reference's cases that `got` holds, default all): n
        exactly, the sums within their bounds, +0.0 in a case without a pair; prints and returns the largest |got - want| /
        bound"""
        got = np.asarray(got)
        sel = slice(None) if cases is None else cases
        (want, bound) = (self.sums[sel], self.bound[sel])
        assert got.shape == want.shape and got.dtype == np.float64, (got.shape, want.shape)
        np.testing.assert_array_equal(got[:, 0], want[:, 0].astype(np.float64), err_msg=f"{label}: counts")
        empty = want[:, 0] == 0
        assert (got[empty] == 0.0).all() and not np.signbit(got[empty]).any(), "a case without a pair holds +0.0"
        err = np.abs(got.astype(LD) - want)
        exact = bound == 0
        assert (err[exact] == 0).all(), "a sum whose bound is zero must be exact"
        ratio = float(np.max(np.where(exact, LD(0), err / np.where(exact, LD(1), bound)), initial=0.0))
        print(f"error moments {label} {got.shape}: max |got - want| / bound = {ratio:.3e}")
        assert (err <= bound).all(), (label, ratio)
        return ratio


def compare_columns(m):
    """(columns of a row of moments, the columns of cae_case_compare's row that carry the same bits): n, S e_m, S e_m^2"""
    diagonal = [1 + m + pairs(m).index((k, k)) for k in range(m)]
    return [0] + [1 + k for k in range(m)] + diagonal, [0] + [2 + 4 * k for k in range(m)] + [4 + 4 * k for k in range(m)]


# ---- the blend -----------------------------------------------------------------------------------------------------------

def blend(preds, weights, intercept=0.0):
    """the definition as a numpy loop over arrays of one shape: float64 of that shape"""
    preds = [np.asarray(p) for p in preds]
    y = np.full(preds[0].shape, float(intercept), dtype=np.float64)
    bad = np.zeros(preds[0].shape, dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for (p, w) in zip(preds, weights):
            if float(w) != 0.0:
                p = p.astype(np.float64)
                prod = np.float64(w) * p
                y = y + prod
                bad |= ~np.isfinite(p)
    y[bad] = np.nan
    return y


# ---- the solver in fractions ------------------------------------------------------------------------------------------------

def _solve_exact(a, b):
    """x with a x = b in Fractions by Gaussian elimination, None where a is singular"""
    k = len(b)
    a = [[Fraction(v) for v in row] + [Fraction(b[i])] for (i, row) in enumerate(a)]
    for col in range(k):
        at = next((r for r in range(col, k) if a[r][col] != 0), None)
        if at is None:
            return None
        (a[col], a[at]) = (a[at], a[col])
        for r in range(k):
            if r != col and a[r][col] != 0:
                f = a[r][col] / a[col][col]
                a[r] = [x - f * y for (x, y) in zip(a[r], a[col])]
    return [a[r][k] / a[r][r] for r in range(k)]


def _kkt(big_e, support):
    k = len(support)
    a = [[2 * big_e[i][j] for j in support] + [1] for i in support] + [[1] * k + [0]]
    x = _solve_exact(a, [0] * k + [1])
    return None if x is None else x[:k]


def objective(big_e, w):
    m = len(w)
    return sum(w[i] * big_e[i][j] * w[j] for i in range(m) for j in range(m))


def solve(big_e, mode):
    """the weights as Fractions for a matrix of Fractions (or integers); None where an affine system is singular"""
    m = len(big_e)
    big_e = [[Fraction(v) for v in row] for row in big_e]
    if mode == "equal":
        return [Fraction(1, m)] * m
    if mode == "affine":
        return _kkt(big_e, list(range(m)))
    (kept, kept_objective) = (None, None)
    for size in range(1, m + 1):
        for support in itertools.combinations(range(m), size):
            ws = _kkt(big_e, list(support))
            if ws is None or any(v <= 0 for v in ws):
                continue
            w = [Fraction(0)] * m
            for (i, v) in zip(support, ws):
                w[i] = v
            value = objective(big_e, w)
            if kept is None or value < kept_objective:
                (kept, kept_objective) = (w, value)
    return kept


def moments_exact(n, se, products, intercept):
    """E as Fractions from integer sums: S / n, with intercept S / n - e e' (e = Se / n), and e"""
    m = len(se)
    full = [[None] * m for _ in range(m)]
    for (col, (i, j)) in enumerate(pairs(m)):
        full[i][j] = full[j][i] = Fraction(int(products[col]), int(n))
    e = [Fraction(int(v), int(n)) for v in se]
    if intercept:
        full = [[full[i][j] - e[i] * e[j] for j in range(m)] for i in range(m)]
    return full, e


# ---- the end-to-end bound ----------------------------------------------------------------------------------------------------

def end_to_end_bound(preds, actual, weights, intercept):
    """The bound on |mse of the blended field as cae_case_compare measures it - the record's w' E w + 2 c w' e + c^2|, to first
    order, for (N, plane) candidates and target without gaps.
    The field.  y = c + S w_m P_m in fp64 carries per pixel at most delta = (M + 2) u (|c| + S|w_m| max|P_m|): the products
    together u S|w_m P_m|, each of the M adds u of a partial sum below |c| + S|w_m| max|P_m|, one more for the second order.
    The fitted weights add to 1 only within a few u; y - a = c + S w_m e_m + (Sw - 1) a, so |Sw - 1| max|a| (Sw in exact
    arithmetic from the stored weights) is added to delta.  With e the blend's true error, mean((e + d)^2) - mean(e^2) is at
    most 2 delta mean|e| + delta^2.
    The sums.  Both mses are sums of n pixels' terms in the kernels' order, held to (n + 4) u S|t| per case; adding N cases'
    rows on the host costs N more roundings: (n + 4 + N) u of S|t| / pixels for the measured mse, and of S|w_i w_j| S|e_i e_j| +
    2 |c| S|w_m| S|e_m| (over the pixels) + c^2 for the record's.  8 u more of the record's magnitude for the host's dozen
    operations on it.  Returns (bound, the parts as a dict)."""
    actual = np.asarray(actual, dtype=np.float64)
    (n_case, plane) = actual.shape
    m = len(preds)
    w = [float(v) for v in weights]
    c = float(intercept)
    a = actual.astype(LD)
    e = [np.asarray(p, dtype=np.float64).astype(LD) - a for p in preds]
    reach = abs(c) + sum(abs(w[k]) * float(np.max(np.abs(preds[k]))) for k in range(m))
    off_one = abs(float(sum(Fraction(v) for v in w) - 1))
    delta = (m + 2) * U * reach + off_one * float(np.max(np.abs(actual)))
    blend_error = sum(LD(w[k]) * e[k] for k in range(m)) + LD(c)
    field = 2.0 * delta * float(np.mean(np.abs(blend_error))) + delta * delta
    pixels = n_case * plane
    count = (plane + 4 + n_case) * U
    measured = count * float(np.sum(blend_error * blend_error) / pixels)
    magnitude = c * c
    for i in range(m):
        magnitude += 2.0 * abs(c) * abs(w[i]) * float(np.sum(np.abs(e[i])) / pixels)
        for j in range(m):
            magnitude += abs(w[i] * w[j]) * float(np.sum(np.abs(e[i] * e[j])) / pixels)
    record = (count + 8 * U) * magnitude
    return field + measured + record, {"delta": delta, "field": field, "measured": measured, "record": record}
