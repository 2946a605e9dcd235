"""Numpy restatement of permutation importance (include/cae_hip.h: cae_normalise_pack_gather, cae_case_importance; DESIGN.md
section 9) shared by test_importance_cpu.py and test_importance_gpu.py: the permutations, the perturbed input, the eight sums
per case, the three sums per pixel, and the bounds the kernel's results are held to.

Definition.  The permutation of repeat r is a single n-cycle built by Sattolo's algorithm from numpy.random.default_rng([seed,
r]): p = 0 .. n - 1, then for i = n - 1 down to 1 one draw j = rng.integers(0, i) and p[i], p[j] swapped (sattolo below; the
package's utils/importance.permutations is held to it).  The perturbed input of a group is x1[n, ch] = x[p[n], ch] for the
group's channels and x[n, ch] otherwise, x being the normalised packed batch: (v - vmin) / range in two rounded fp32
operations, 0 where range == 0, v itself where the model does not normalise (normalise below).

Comparison.  With the fp32 scores p0 = model(x), p1 = model(x1) and the target a as stored, in fp64
    P = vmin + (double)p * range        two rounded operations, so the same bits as cae_denormalise_f64 (denormalise below)
a pixel is a pair when a, P0 and P1 are all finite; e0 = P0 - a, e1 = P1 - a; per case over its pairs
    {n, S e1^2, S e0^2, S|e1|, S|e0|, S (P1 - P0)^2, #(e1^2 > e0^2), #(e1^2 < e0^2)}
and per pixel over the cases {count, S e1^2, S e0^2}.  The two win counts compare the fp64 squares of the fp64 differences,
each rounded on its own as numpy rounds them: they, n and count are integers and are compared exactly.  Every other sum is
formed here in np.longdouble from the exact P and a.

Bound on a floating-point sum of m terms t (u = 2^-53):  |got - want| <= (m + 4) u S|t|.
Why: the kernel's e = fl(P - a) is within u |e| of the exact difference, because a rounded subtraction errs relative to its
own result.  A term |e| therefore carries one rounding.  A term e^2 carries three: two from e (the relative error of a square
is twice that of its base) and one from the rounded product.  The same holds for (P1 - P0)^2.  Adding m terms in any order
- lanes, trees and tiles included - makes m - 1 further roundings, each at most u of a partial sum that never exceeds S|t|
because all terms are positive.  To first order that is (m + 2) u S|t| for the squares and m u S|t| for the absolute values;
m + 4 leaves room for the second-order terms and for this reference's own 2^-64 roundings.  It is a count of operations, not
a fit to any result.  For a case m is its number of pairs; for a pixel of the map m is the number of cases that pair there.
"""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
NAMES = ("n", "S e1^2", "S e0^2", "S|e1|", "S|e0|", "S dP^2", "#grew", "#shrank")


def sattolo(n, repeats, seed):
    """(repeats, n) int32: the definition's permutations"""
    out = np.empty((repeats, n), dtype=np.int32)
    for r in range(repeats):
        rng = np.random.default_rng([seed, r])
        p = list(range(n))
        for i in range(n - 1, 0, -1):
            j = int(rng.integers(0, i))
            (p[i], p[j]) = (p[j], p[i])
        out[r] = p
    return out


def is_single_cycle(p):
    """True when following p from 0 visits every index before it returns"""
    (seen, k) = (0, 0)
    while True:
        k = int(p[k])
        seen += 1
        if k == 0:
            return seen == len(p)
        if seen > len(p):
            return False


def normalise(v, vmin, vmax, enable=True):
    """cae_normalise_pack's arithmetic on an fp32 array: the range formed in fp64 from python floats and rounded to fp32"""
    v = np.asarray(v, dtype=np.float32)
    if not enable:
        return v.copy()
    (lo, rng) = (np.float32(vmin), np.float32(float(vmax) - float(vmin)))
    if rng == 0:
        return np.zeros_like(v)
    return ((v - lo) / rng).astype(np.float32)


def denormalise(p, vmin, rng):
    """P = vmin + (double)p * range in fp64, two rounded operations"""
    return np.float64(vmin) + np.asarray(p, dtype=np.float32).astype(np.float64) * np.float64(rng)


class Reference:
    """the definition's sums of one operand set with their bounds, computed once and compared with many results.
    base, pert: (N, H, W) or (N, plane) fp32 scores of channel 0; actual: the target's values likewise, any float dtype"""

    def __init__(self, base, pert, actual, vmin, rng):
        actual = np.asarray(actual).astype(np.float64)
        n = actual.shape[0]
        (base, pert, actual) = (np.asarray(base).reshape(n, -1), np.asarray(pert).reshape(n, -1), actual.reshape(n, -1))
        assert base.dtype == np.float32 and pert.dtype == np.float32 and base.shape == pert.shape == actual.shape
        with np.errstate(invalid="ignore", over="ignore"):
            (P0, P1) = (denormalise(base, vmin, rng), denormalise(pert, vmin, rng))
            pair = np.isfinite(actual) & np.isfinite(P0) & np.isfinite(P1)
            z = lambda v: np.where(pair, v, 0.0)        # noqa: E731
            (a, P0, P1) = (z(actual), z(P0), z(P1))
            # the counts: fp64, every operation rounded on its own
            (q0, q1) = ((P0 - a) * (P0 - a), (P1 - a) * (P1 - a))
            grew = pair & (q1 > q0)
            shrank = pair & (q1 < q0)
            # the sums: np.longdouble from the exact P and a
            (e0, e1, d) = (P0.astype(LD) - a.astype(LD), P1.astype(LD) - a.astype(LD), P1.astype(LD) - P0.astype(LD))
        self.pair = pair
        (self.P0, self.P1) = (P0, P1)
        terms = [e1 * e1, e0 * e0, np.abs(e1), np.abs(e0), d * d]
        m = pair.sum(axis=1)
        self.sums = np.zeros((n, 8), dtype=LD)
        self.bound = np.zeros((n, 8), dtype=LD)
        self.sums[:, 0] = m
        for (k, t) in enumerate(terms):
            self.sums[:, 1 + k] = t.sum(axis=1)
            self.bound[:, 1 + k] = (m + 4) * LD(U) * t.sum(axis=1)
        self.sums[:, 6] = grew.sum(axis=1)
        self.sums[:, 7] = shrank.sum(axis=1)
        mp = pair.sum(axis=0)
        self.map = np.stack([mp.astype(LD), terms[0].sum(axis=0), terms[1].sum(axis=0)])
        self.map_bound = np.stack([np.zeros_like(self.map[0]), (mp + 4) * LD(U) * self.map[1], (mp + 4) * LD(U) * self.map[2]])

    @staticmethod
    def _ratio(got, want, bound):
        err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want)
        exact = bound == 0
        assert (err[exact] == 0).all(), "a sum whose bound is zero must be exact"
        return float(np.max(np.where(exact, LD(0), err / np.where(exact, LD(1), bound)), initial=0.0)), err

    def check(self, got, label="", cases=None):
        """the kernel's per-case sums against the definition (cases: the reference's cases that `got` holds, default all): n
        and both win counts exactly, the five sums within their bounds, +0.0 in a case without a pair; prints and returns the
        largest |got - want| / bound"""
        got = np.asarray(got)
        sel = slice(None) if cases is None else cases
        (want, bound) = (self.sums[sel], self.bound[sel])
        assert got.shape == want.shape and got.dtype == np.float64, (got.shape, want.shape)
        for k in (0, 6, 7):
            np.testing.assert_array_equal(got[:, k], want[:, k].astype(np.float64), err_msg=NAMES[k])
        empty = want[:, 0] == 0
        assert (got[empty] == 0.0).all() and not np.signbit(got[empty]).any(), "a case without a pair holds +0.0"
        (ratio, err) = self._ratio(got[:, 1:6], want[:, 1:6], bound[:, 1:6])
        print(f"importance sums {label} {got.shape}: max |got - want| / bound = {ratio:.3e}")
        assert (err <= bound[:, 1:6]).all(), (label, ratio)
        return ratio

    def check_map(self, got, label=""):
        """the kernel's per-pixel sums (3, plane) or (3, H, W), started from zeros, against the definition: the count exactly,
        the two sums within their bounds"""
        got = np.asarray(got).reshape(3, -1)
        assert got.dtype == np.float64 and got.shape == self.map.shape, (got.shape, self.map.shape)
        np.testing.assert_array_equal(got[0], self.map[0].astype(np.float64), err_msg="count")
        (ratio, err) = self._ratio(got[1:], self.map[1:], self.map_bound[1:])
        print(f"importance map {label} {got.shape}: max |got - want| / bound = {ratio:.3e}")
        assert (err <= self.map_bound[1:]).all(), (label, ratio)
        return ratio
