"""The definition of cae_case_fss (include/cae_hip.h) restated in numpy, for the tests: every count is an int64 difference of
an int64 integral image, so the reference is exact, and the six sums of a case stay below 2^63 as the header derives."""
import numpy as np

SIDES = {"above": 0, "below": 1}


def threshold_list(thresholds):
    """[(value, side name)] of numbers ("above") or (value, side) pairs"""
    return [(float(t[0]), t[1]) if isinstance(t, (tuple, list)) else (float(t), "above") for t in thresholds]


def _window_counts(mask, n):
    """(N, h - n + 1, w - n + 1) int64: the set pixels of every n x n window of the (N, h, w) boolean mask"""
    (cases, h, w) = mask.shape
    table = np.zeros((cases, h + 1, w + 1), dtype=np.int64)
    table[:, 1:, 1:] = np.cumsum(np.cumsum(mask.astype(np.int64), axis=1), axis=2)
    return table[:, n:, n:] - table[:, :-n, n:] - table[:, n:, :-n] + table[:, :-n, :-n]


def reference(p, a, thresholds, widths, gaps="strict"):
    """(N, T, S, 6) int64 {windows, S cM, S cO, S cM^2, S cO^2, S cM cO} of channel-0 planes p and a (N, h, w)"""
    (p, a) = (np.asarray(p, dtype=np.float64), np.asarray(a, dtype=np.float64))
    (cases, h, w) = p.shape
    thresholds = threshold_list(thresholds)
    out = np.zeros((cases, len(thresholds), len(widths), 6), dtype=np.int64)
    pair = np.isfinite(p) & np.isfinite(a)
    with np.errstate(invalid="ignore"):
        events = [((pair & (p < t), pair & (a < t)) if side == "below" else (pair & (p >= t), pair & (a >= t)))
                  for (t, side) in thresholds]
    for (s, n) in enumerate(widths):
        if n > h or n > w:
            continue
        bad = _window_counts(~pair, n)
        counted = (bad < n * n) if gaps == "ignore" else (bad == 0)
        for (t, (ep, ea)) in enumerate(events):
            cm = np.where(counted, _window_counts(ep, n), 0)
            co = np.where(counted, _window_counts(ea, n), 0)
            total = lambda v: v.reshape(cases, -1).sum(axis=1)      # noqa: E731
            out[:, t, s] = np.stack([total(counted.astype(np.int64)), total(cm), total(co), total(cm * cm), total(co * co),
                                     total(cm * co)], axis=1)
    return out


def contingency(p, a, value, side="above"):
    """(pairs, hits, misses, false alarms) of the whole (N, h, w) planes: what width 1 must add up to under the strict rule"""
    (p, a) = (np.asarray(p, dtype=np.float64), np.asarray(a, dtype=np.float64))
    pair = np.isfinite(p) & np.isfinite(a)
    with np.errstate(invalid="ignore"):
        (ep, ea) = (pair & (p < value), pair & (a < value)) if side == "below" else (pair & (p >= value), pair & (a >= value))
    return int(pair.sum()), int((ep & ea).sum()), int((~ep & ea).sum()), int((ep & ~ea).sum())
