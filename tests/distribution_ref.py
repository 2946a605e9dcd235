"""Numpy restatement of cae_joint_hist (include/cae_hip.h) shared by test_distribution_cpu.py and
test_joint_hist_gpu.py: the fine and coarse bin of a value, the joint and marginal counts, the outside counts and the
per-bin error sums of the pairs, in fp64.

The bin of a value is formed as the kernel forms it: scale = (double)n_fine / (hi - lo), one division; t = (v - lo) * scale,
the subtraction and the product each rounded on its own (numpy contracts nothing); the comparison against 0 and n_fine in
fp64 before the conversion; the coarse bin f // sub.  The cond sums are taken with math.fsum, the correctly rounded sum,
and come with what a bound for any order of summation needs: the count c of a bin and S|x_i| of its addends.  A sum of c
addends, added in any order with every partial sum rounded, is within (c - 1) u S|x_i| of the exact sum to first order in u =
2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); fsum adds at most u / 2 of the sum, so c u S|x_i|
bounds the difference from the fsum value."""
import math

import numpy as np

U = 2.0 ** -53


def channel0(x):
    """channel 0 of an (N, C, H, W) array as (N, H * W) float64, the stored values converted exactly"""
    x = np.asarray(x)
    return np.asarray(x[:, 0], dtype=np.float64).reshape(x.shape[0], -1)


def fine_bins(v, lo, hi, n_bin, sub):
    """the fine bin of every value of v (finite values; fp64)"""
    n_fine = n_bin * sub
    scale = np.float64(n_fine) / (np.float64(hi) - np.float64(lo))
    with np.errstate(over="ignore"):
        t = (np.asarray(v, dtype=np.float64) - np.float64(lo)) * scale
    f = np.zeros(t.shape, dtype=np.int64)
    f[t >= n_fine] = n_fine - 1
    inside = (t >= 0) & (t < n_fine)
    f[inside] = t[inside].astype(np.int64)
    return f


def _bin_sums(keys, x, n_bin):
    """(fsum of x, fsum of |x|, count) per key 0 .. n_bin - 1"""
    order = np.argsort(keys, kind="stable")
    (ks, xs) = (keys[order], x[order])
    cut = np.searchsorted(ks, np.arange(n_bin + 1))
    sums = np.array([math.fsum(xs[cut[k]:cut[k + 1]]) for k in range(n_bin)])
    mags = np.array([math.fsum(np.abs(xs[cut[k]:cut[k + 1]])) for k in range(n_bin)])
    return sums, mags, np.diff(cut)


class Reference:
    """joint (n_bin, n_bin), marg (2, n_fine), cond (2, n_bin, 4), outside (4,) of prediction p against target a (arrays of
    the same shape, any values) as cae_joint_hist defines them, with pairs (the number of pairs) and bound (2, n_bin, 4): c u
    S|x_i| of every cond sum."""

    def __init__(self, p, a, lo, hi, n_bin, sub):
        (p, a) = (np.asarray(p, dtype=np.float64).reshape(-1), np.asarray(a, dtype=np.float64).reshape(-1))
        (lo, hi) = (np.float64(lo), np.float64(hi))
        pair = np.isfinite(p) & np.isfinite(a)
        (p, a) = (p[pair], a[pair])
        n_fine = n_bin * sub
        (fa, fp) = (fine_bins(a, lo, hi, n_bin, sub), fine_bins(p, lo, hi, n_bin, sub))
        (ia, ip) = (fa // sub, fp // sub)
        self.pairs = int(pair.sum())
        self.joint = np.bincount(ia * n_bin + ip, minlength=n_bin * n_bin).reshape(n_bin, n_bin).astype(np.int64)
        self.marg = np.stack([np.bincount(fa, minlength=n_fine), np.bincount(fp, minlength=n_fine)]).astype(np.int64)
        self.outside = np.array([(a < lo).sum(), (a > hi).sum(), (p < lo).sum(), (p > hi).sum()], dtype=np.int64)
        with np.errstate(over="ignore"):
            d = p - a
            addends = ((d, np.abs(d), d * d, a - lo), (d, np.abs(d), d * d, p - lo))
        self.cond = np.zeros((2, n_bin, 4))
        self.bound = np.zeros((2, n_bin, 4))
        for (k, keys) in enumerate((ia, ip)):
            for (j, x) in enumerate(addends[k]):
                (s, mag, c) = _bin_sums(keys, x, n_bin)
                self.cond[k, :, j] = s
                self.bound[k, :, j] = c * U * mag
