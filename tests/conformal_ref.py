"""The numpy restatement of cae_score_quantiles, cae_score_counts and cae_interval_bounds (include/cae_hip.h): the scores formed
as defined - every operation a correctly rounded fp64 operation, which numpy's are - np.sort per group, integer rank.  No
tolerance belongs to it: the GPU's answers are compared with np.array_equal."""
from fractions import Fraction

import numpy as np


def scores(p, a, s=None):
    """(e, valid) of channel 0 of (N, C, H, W) operands, (N, H, W) each: e = |p - a| or |p - a| / s in fp64"""
    (p, a) = (np.asarray(p)[:, 0].astype(np.float64), np.asarray(a)[:, 0].astype(np.float64))
    valid = np.isfinite(p) & np.isfinite(a)
    with np.errstate(all="ignore"):
        e = np.abs(p - a)
        if s is not None:
            s = np.asarray(s)[:, 0].astype(np.float64)
            valid &= np.isfinite(s) & (s > 0)
            e = e / np.where(valid, s, 1.0)
    return e, valid


def rank(n, level):
    level = Fraction(level)
    return ((int(n) + 1) * level.numerator + level.denominator - 1) // level.denominator


def _group_quantiles(e, levels):
    """(q (L,), n) of one group's valid scores"""
    e = np.sort(e)
    n = e.size
    q = np.full(len(levels), np.inf)
    for (i, level) in enumerate(levels):
        k = rank(n, level)
        if k <= n:
            q[i] = e[k - 1]
    return q, n


def quantiles(p, a, levels, group, s=None):
    """(q, n): (L, H, W) float64 and (H, W) int64 for group "pixel", (L,) and () for "pooled" """
    levels = [Fraction(v) for v in levels]
    (e, valid) = scores(p, a, s)
    (_, h, w) = e.shape
    if group == "pooled":
        (q, n) = _group_quantiles(e[valid], levels)
        return q, np.int64(n)
    q = np.full((len(levels), h, w), np.inf)
    n = valid.sum(axis=0).astype(np.int64)
    if e.shape[0] == 0:
        return q, n
    ordered = np.sort(np.where(valid, e, np.nan), axis=0)       # per pixel, what is no score goes last (np.sort's place for NaN)
    for (i, level) in enumerate(levels):
        k = ((n + 1) * level.numerator + level.denominator - 1) // level.denominator
        at = np.clip(k - 1, 0, e.shape[0] - 1)
        q[i] = np.where(k <= n, np.take_along_axis(ordered, at[None], axis=0)[0], np.inf)
    return q, n


def counts(p, a, q, group, s=None, strict=False):
    """(count, n): the valid scores <= q (strict: < q) per level and group, and the valid scores"""
    (e, valid) = scores(p, a, s)
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        if group == "pooled":
            below = [(e[valid] < v) if strict else (e[valid] <= v) for v in q]
            return np.array([int(b.sum()) for b in below], dtype=np.int64), np.int64(valid.sum())
        below = [(((e < v[None]) if strict else (e <= v[None])) & valid).sum(axis=0) for v in q]
    return np.array(below, dtype=np.int64).reshape(q.shape), valid.sum(axis=0).astype(np.int64)


def bounds(p, q, s=None):
    """(lower, upper) (N, H, W) float64 of channel 0: p -+ q * s, the product and the sum rounded separately"""
    p = np.asarray(p)[:, 0].astype(np.float64)
    ok = np.isfinite(p)
    with np.errstate(all="ignore"):
        half = np.broadcast_to(np.asarray(q, dtype=np.float64), p.shape)
        if s is not None:
            s = np.asarray(s)[:, 0].astype(np.float64)
            ok &= np.isfinite(s) & (s > 0)
            half = half * s
        return np.where(ok, p - half, np.nan), np.where(ok, p + half, np.nan)
