"""Numpy restatement of the residual target (include/cae_hip.h, cae_residual_scan / cae_residual_pack_rows /
cae_residual_restore_f64; DESIGN.md section 9, "Residual target"), given the base field b: the fp64 interpolation of the
low-resolution input that cae_case_baseline returns with field=True (case_ops.upsample), NaN where a tap is not finite.

    r = double(t) - b                                   one rounding in fp64
    scan    k = #{r not finite}; rmin, rmax = the fp64 minimum and maximum of the finite r (+inf, -inf without one)
    pack    y = float32((r - rmin) / (rmax - rmin))     subtraction and division rounded in fp64, then one rounding to fp32;
            0 at span 0; float32(r) with normalisation off; NaN where r is not finite; case i in row dst_rows[i]
    restore p = b + (rmin + double(y) * span)           product, inner sum and outer sum each rounded in fp64;
            b + double(y) with normalisation off; NaN where b or y is NaN

numpy rounds every one of these operations on its own, as the kernels do with contraction off, so the results are compared
bit for bit.  The NaN written is the canonical quiet one (0x7fc00000, 0x7ff8000000000000).

Bound.  Pack and restore see the same bits of b, so where r is finite
    |restore(pack(t)) - t| <= span * 2^-24 + 4 * 2^-53 * max(|t|, |b|, |rmin|, |rmax|):
y <= 1 is rounded to fp32 once, at most 2^-25 relative and doubled for margin, and span scales it; the four fp64 roundings
(r, r - rmin or y * span, rmin + ., b + .) act on values no larger than twice the largest of |t|, |b|, |rmin|, |rmax|, each
at most 2^-53 relative, and the division's rounding is below the fp32 one by 2^-28.
"""
import numpy as np

F32_NAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]
F64_NAN = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]


def residual(target, base):
    """r (N, H, W) fp64 of target (N, H, W) or (N, 1, H, W) fp32 and base (N, H, W) fp64"""
    t = np.asarray(target, dtype=np.float32)
    if t.ndim == 4:
        t = t[:, 0]
    with np.errstate(invalid="ignore"):
        return t.astype(np.float64) - np.asarray(base, dtype=np.float64)


def scan(target, base):
    """(k, rmin, rmax) as python numbers"""
    r = residual(target, base)
    finite = np.isfinite(r)
    return (int((~finite).sum()), float(np.min(r[finite], initial=np.inf)), float(np.max(r[finite], initial=-np.inf)))


def pack(target, base, rmin, rmax, enable=True, dst_rows=None):
    """y (N, H, W) fp32"""
    r = residual(target, base)
    finite = np.isfinite(r)
    span = np.float64(rmax) - np.float64(rmin)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if not enable:
            y = r.astype(np.float32)
        elif span == 0.0:
            y = np.zeros(r.shape, dtype=np.float32)
        else:
            y = ((r - np.float64(rmin)) / span).astype(np.float32)
    y = np.where(finite, y, F32_NAN).astype(np.float32)
    if dst_rows is None:
        return y
    out = np.empty_like(y)
    out[np.asarray(dst_rows)] = y
    return out


def restore(y, base, rmin, rmax, enable=True):
    """p (N, H, W) fp64 of the scores y (N, H, W) or (N, 1, H, W) fp32"""
    y = np.asarray(y, dtype=np.float32)
    if y.ndim == 4:
        y = y[:, 0]
    b = np.asarray(base, dtype=np.float64)
    v = y.astype(np.float64)
    span = np.float64(rmax) - np.float64(rmin)
    with np.errstate(invalid="ignore", over="ignore"):
        if enable:
            u = v * span
            w = np.float64(rmin) + u
            p = b + w
        else:
            p = b + v
    return np.where(np.isnan(b) | np.isnan(v), F64_NAN, p)


def round_trip_bound(target, base, rmin, rmax):
    """the bound above per pixel, fp64 (N, H, W)"""
    t = np.asarray(target, dtype=np.float32)
    if t.ndim == 4:
        t = t[:, 0]
    big = np.maximum(np.maximum(np.abs(t.astype(np.float64)), np.abs(base)), max(abs(rmin), abs(rmax)))
    return (rmax - rmin) * 2.0 ** -24 + 4.0 * 2.0 ** -53 * big
