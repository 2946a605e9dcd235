"""Numpy restatement of the loader section of include/cae_hip.h (cae_scan_f32, cae_normalise_pack[_rows],
cae_invert_permutation, cae_denormalise_f64, cae_metric_sums, cae_bswap32), shared by test_loader_ref_cpu.py and
test_loader_kernels_gpu.py, together with the seeded inputs both files use.

Arithmetic.  Normalisation is two correctly rounded fp32 operations on the stored fp32 value: the subtraction of float32(vmin)
and the division by float32(float(vmax) - float(vmin)), the range being formed in fp64 from python floats and rounded once; a
range of 0 gives 0 for every element, of an input or of the output alike, and enable == False copies.  Denormalisation is two
correctly rounded fp64 operations, vmin + ((double)y * (vmax - vmin)): the product is rounded before the addition, so it is
NOT fma(y, range, vmin).  The metric sums use that same e, with a' = a - vmin and e' = e - vmin.

Inputs.  An implementation that divides in fp64 and rounds once, or that multiplies by the reciprocal of the range, gives the
same bits as the definition on many data sets; so does a contracted fma in the denormalisation whenever vmin and vmax are
fp32 values, because y * (vmax - vmin) is then exact in fp64 (24 + at most 25 significant bits).  wide_variable,
narrow_variable, unit_scores with ARBITRARY_F64 and fma_sensitive_scores are the inputs on which these neighbours differ
from the definition; test_loader_ref_cpu.py holds them to that.

Bound on a metric sum of N kept pixels (u = 2^-53):  |got - fsum(terms)| <= 2 N u S|term|, the terms being the fp64 addends
of metric_terms.  N - 1 additions in any order round once each, at most u of a partial sum that cannot exceed S|term| to
first order; one more rounding per addend covers a compiler that contracts acc += x * y (the product then is not rounded on
its own, so it differs from the term by at most u |term|) as well as one that does not.  A count of operations, not a fit.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
ARBITRARY_F64 = (285.123456789, 305.987654321)      # neither bound nor their difference is an fp32 value
FP32_VALUED = (288.0, 298.5)
SUM_NAMES = ("n", "S a'", "S e'", "S a'^2", "S e'^2", "S a'e'", "S|a-e|", "S(a-e)^2")


# ---- the definitions ------------------------------------------------------------------------------

def scan(x):
    """(NaN count, nanmin, nanmax) as python numbers; the extremes of an all-NaN array are not defined (None)"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    nan = np.isnan(x)
    count = int(nan.sum())
    if count == x.size:
        return count, None, None
    kept = x[~nan]
    return count, float(kept.min()), float(kept.max())


def normalise(src, vmin, vmax, enable=True):
    """fp32 array of src's shape: ((src - float32(vmin)) / float32(float(vmax) - float(vmin))), each operation rounded to
    fp32; zeros where that range is 0; src itself where enable is false"""
    src = np.asarray(src)
    assert src.dtype == np.float32
    if not enable:
        return src.copy()
    lo = np.float32(vmin)
    span = np.float32(float(vmax) - float(vmin))
    if span == 0:
        return np.zeros(src.shape, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        shifted = np.subtract(src, lo, dtype=np.float32)
        return np.divide(shifted, span, dtype=np.float32)


def pack(dst, src_norm, c_off, rows=None):
    """a copy of dst (n, c_dst, ...) with src_norm (n, c_src, ...) written to channels [c_off, c_off + c_src) of row
    rows[i] (row i when rows is None)"""
    out = np.array(dst, dtype=np.float32, copy=True)
    (n, c_src) = src_norm.shape[:2]
    assert 0 <= c_off and c_off + c_src <= out.shape[1] and out.shape[0] == n
    where = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    out.reshape(n, out.shape[1], -1)[where, c_off:c_off + c_src, :] = np.asarray(src_norm).reshape(n, c_src, -1)
    return out


def denormalise(y32, vmin, vmax):
    """fp64: vmin + (y * (vmax - vmin)), the product rounded before the sum"""
    y = np.asarray(y32).astype(np.float64)
    span = np.float64(float(vmax) - float(vmin))
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.multiply(y, span, dtype=np.float64)
        return np.add(np.float64(vmin), prod, dtype=np.float64)


def metric_terms(y, a, mask, vmin, vmax):
    """(terms, keep, e): terms (8,) + y.shape fp64, the addends {1, a', e', a'^2, e'^2, a'e', |a - e|, (a - e)^2} of every
    pixel, each operation rounded to fp64 on its own; keep = mask != 0 broadcast to y's shape (all True without a mask);
    e = denormalise(y)"""
    y = np.asarray(y)
    a = np.asarray(a)
    assert y.dtype == np.float32 and a.dtype == np.float32 and y.shape == a.shape
    keep = np.ones(y.shape, dtype=bool) if mask is None else np.broadcast_to(np.asarray(mask) != 0, y.shape)
    e = denormalise(y, vmin, vmax)
    av = a.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = av - e
        a_ = av - np.float64(vmin)
        e_ = e - np.float64(vmin)
        terms = np.stack([np.ones(y.shape), a_, e_, a_ * a_, e_ * e_, a_ * e_, np.abs(d), d * d])
    return terms, keep, e


def _fsum(values):
    values = np.asarray(values, dtype=np.float64)
    if not np.isfinite(values).all():
        with np.errstate(invalid="ignore"):
            return float(values.sum())      # NaN or an infinity, as any order of additions gives (math.fsum raises on inf - inf)
    return math.fsum(values.tolist())


def metric_sums_exact(y, a, mask, vmin, vmax, rows=None):
    """(sums, abs_sums), both (n, 8) fp64: per instance the correctly rounded sum of each column of metric_terms over the
    kept pixels (math.fsum), and the sum of the terms' magnitudes for the bound.  rows: compute these instances only, the
    others are left NaN"""
    (terms, keep, _) = metric_terms(y, a, mask, vmin, vmax)
    n = y.shape[0]
    terms = terms.reshape(8, n, -1)
    keep = keep.reshape(n, -1)
    sums = np.full((n, 8), np.nan)
    mags = np.full((n, 8), np.nan)
    for i in (range(n) if rows is None else rows):
        for k in range(8):
            t = terms[k, i][keep[i]]
            sums[i, k] = _fsum(t)
            mags[i, k] = _fsum(np.abs(t))
    return sums, mags


def metric_bound(count, abs_sums):
    """2 N u S|term| of the module docstring"""
    return 2.0 * np.asarray(count, dtype=np.float64) * U * np.asarray(abs_sums, dtype=np.float64)


# ---- neighbours of the definition: what an implementation might compute instead ------------------------------

def normalise_fp64_once(src, vmin, vmax):
    """the quotient formed in fp64 and rounded to fp32 once"""
    return ((src.astype(np.float64) - float(vmin)) / (float(vmax) - float(vmin))).astype(np.float32)


def normalise_reciprocal(src, vmin, vmax):
    """fp32 throughout, but a multiplication by the rounded reciprocal of the range"""
    span = np.float32(float(vmax) - float(vmin))
    inv = np.divide(np.float32(1.0), span, dtype=np.float32)
    return np.multiply(np.subtract(src, np.float32(vmin), dtype=np.float32), inv, dtype=np.float32)


def denormalise_fma(y32, vmin, vmax):
    """fma(y, vmax - vmin, vmin): the exact y * range + vmin rounded to fp64 once (fractions.Fraction; finite y only)"""
    span = Fraction(float(vmax) - float(vmin))
    lo = Fraction(float(vmin))
    flat = np.asarray(y32, dtype=np.float32).reshape(-1)
    out = np.array([float(Fraction(float(v)) * span + lo) for v in flat], dtype=np.float64)
    return out.reshape(np.shape(y32))


# ---- seeded inputs ---------------------------------------------------------------------------------

def wide_variable(n, seed=101):
    """exp(N(0, 3)) - 3.3 as fp32: ten orders of magnitude, so v - vmin is rounded for most elements"""
    return (np.exp(np.random.default_rng(seed).normal(0.0, 3.0, n)) - 3.3).astype(np.float32)


def narrow_variable(n, seed=102):
    """285 + 20 U[0, 1) as fp32: a temperature-like field, v - vmin exact in fp32"""
    return (285.0 + 20.0 * np.random.default_rng(seed).random(n)).astype(np.float32)


def unit_scores(n, seed=103):
    """U[0, 1) as fp32: what a model returns for a normalised target"""
    return np.random.default_rng(seed).random(n, dtype=np.float32)


def bounds_of(x):
    """(vmin, vmax) as DSDataset takes them from the scan: python floats holding fp32 values"""
    (_, lo, hi) = scan(x)
    return lo, hi


def fma_sensitive_scores(vmin, vmax, n=3000, seed=103):
    """those of unit_scores(n, seed) whose denormalised value changes when the two operations are contracted"""
    y = unit_scores(n, seed)
    return y[denormalise(y, vmin, vmax) != denormalise_fma(y, vmin, vmax)]
