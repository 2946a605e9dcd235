"""Numpy restatement of cae_case_baseline (include/cae_hip.h) shared by test_baseline_cpu.py and
test_case_baseline_gpu.py: the interpolation of the low-resolution field to the target's grid, the six per-case sums of
baseline and prediction against the target, and the bounds the kernel's results are held to.

Definition.  Channel 0 of low (h_in x w_in), pred (h_out x w_out, may be absent) and actual (h_out x w_out), taken to fp64 as
stored.  Both grids cover the same extent and are pixel-centred.  Per axis, with n_in input and n_out output samples, for
output index o, in fp64 with every operation rounded on its own (no fused multiply-add):
    s = (double)n_in / (double)n_out,   src = (o + 0.5) * s - 0.5
    nearest  (0): i = min((long)floor((o + 0.5) * s), n_in - 1); one tap, weight 1
    bilinear (1): src = max(src, 0), i0 = min((long)floor(src), n_in - 1), i1 = min(i0 + 1, n_in - 1), t = src - i0;
                  taps (i0, i1), weights (1 - t, t)
    bicubic  (2): i = floor(src), t = src - i; taps i - 1 .. i + 2 clamped to [0, n_in - 1], A = -0.75, weights
                  (c2(t + 1), c1(t), c1(1 - t), c2(2 - t)) with c1(x) = ((A + 2) x - (A + 3)) x^2 + 1 and
                  c2(x) = ((A x - 5 A) x + 8 A) x - 4 A
(torch.nn.functional.interpolate with align_corners=False: nearest-exact, bilinear, bicubic).  Here s, src, i and t are the
same fp64 operations as the kernel's and therefore the same bits; the weights are real functions of that t and are evaluated
in np.longdouble, as are all products and sums.  The interpolation is separable, along the row first: every tapped input row
j gives r_j(x) = S_k wx_k low[j][ix_k], and b = S_j wy_j r_j, taps in ascending order.
A pixel counts iff a, p (when given) and every tap read for it - 1, 2 x 2 or 4 x 4 before clamping, whatever its weight -
are finite.  Per case over the counted pixels
    sums = {n, S|b - a|, S(b - a)^2, S|p - a|, S(p - a)^2, n_won},  n_won = #{|p - a| < |b - a|}
with entries 3..5 zero without p and six zeros for a case without a counted pixel.  The field b is NaN where the taps are not
all finite.

Bound on a pixel (u = 2^-53):  |b_got - b| <= K u M,  M = S_j S_k |wy_j| |wx_k| |v_jk|,  K = 32.
Why: the kernel evaluates the weights in fp64 from the exact t in a form whose error is relative - nearest 1 (exact),
bilinear 1 - t (one rounding) and t, bicubic the factors of the same cubics, c1(t) = (1 - t)(1 + t - 1.25 t^2),
c2(t + 1) = -0.75 t (1 - t)^2 and their mirror images, where 1 - t is one rounding, the bracket is at least 0.75 with four
rounded operations on values of at most 1.25, and the products are two or three roundings: at most 8 u relative per weight.
A row value r_j is four rounded products (1 u each) and three rounded additions (each at most u of a partial sum bounded by
S_k |wx_k| |v_k|): with the weights' 8 u at most 12 u S_k |wx_k| |v_k|.  The column pass does the same to the r_j: another
12 u, 24 u M in all to first order.  K = 32 leaves a third for the second-order terms and for the reference's own 2^-64
roundings.  It is a count of operations, not a fit to any result.
Bounds on the sums, with beta the pixel's bound, d = b - a, e = p - a and S over the n counted pixels:
    S|b - a|    S (beta + u |d|)                       + n u S|d|
    S(b - a)^2  S (2 |d| beta + beta^2 + 3 u d^2)      + n u S d^2
    S|p - a|    S u |e|                                + n u S|e|
    S(p - a)^2  S 3 u e^2                              + n u S e^2
(one rounding for the difference, one for the square; a sum of n terms added in any order is within n u S|term|).  n is
compared exactly.  A pixel is undecided for n_won when | |e| - |d| | <= beta + 2 u (|d| + |e|); the test inputs have none,
so n_won is compared exactly too.
"""
import numpy as np

MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}
A = -0.75
K = 32.0
U = 2.0 ** -53
LD = np.longdouble


def channel0(x):
    return np.asarray(x)[:, 0].astype(np.float64)


def axis_taps(n_in, n_out, mode):
    """(idx (n_out, T) int64 clamped tap indices, t (n_out,) float64) of one axis: the kernel's fp64 operations"""
    mode = MODES.get(mode, mode)
    (n_in, n_out) = (int(n_in), int(n_out))
    o = np.arange(n_out, dtype=np.float64)
    s = np.float64(n_in) / np.float64(n_out)
    if mode == 0:
        i = np.minimum(np.floor((o + 0.5) * s).astype(np.int64), n_in - 1)
        return i[:, None], np.zeros(n_out)
    src = (o + 0.5) * s - 0.5
    if mode == 1:
        src = np.maximum(src, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return np.stack([i0, i1], axis=1), src - i0.astype(np.float64)
    f = np.floor(src)
    i = f.astype(np.int64)
    idx = np.clip(i[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, src - f


def axis_weights(t, mode):
    """(n_out, T) np.longdouble weights from the fp64 t"""
    mode = MODES.get(mode, mode)
    t = np.asarray(t, dtype=np.float64).astype(LD)
    if mode == 0:
        return np.ones((t.shape[0], 1), dtype=LD)
    if mode == 1:
        return np.stack([1 - t, t], axis=1)
    a = LD(A)
    c1 = lambda x: ((a + 2) * x - (a + 3)) * x * x + 1              # noqa: E731
    c2 = lambda x: ((a * x - 5 * a) * x + 8 * a) * x - 4 * a        # noqa: E731
    return np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], axis=1)


def footprint(n_in, n_out, mode):
    """(n_out, T) tap indices before clamping: what the counting rule speaks of"""
    (idx, _) = axis_taps(n_in, n_out, mode)
    return idx


def upsample(low, out_shape, mode):
    """low (N, h_in, w_in) fp64 -> (field (N, h_out, w_out) longdouble with NaN where a tap is not finite,
    magnitude M (N, h_out, w_out) longdouble, ok (N, h_out, w_out) bool)"""
    low = np.asarray(low, dtype=np.float64)
    (n, h_in, w_in) = low.shape
    (h_out, w_out) = (int(out_shape[0]), int(out_shape[1]))
    (iy, ty) = axis_taps(h_in, h_out, mode)
    (ix, tx) = axis_taps(w_in, w_out, mode)
    (wy, wx) = (axis_weights(ty, mode), axis_weights(tx, mode))
    finite = np.isfinite(low)
    v = np.where(finite, low, 0.0).astype(LD)
    field = np.zeros((n, h_out, w_out), dtype=LD)
    mag = np.zeros((n, h_out, w_out), dtype=LD)
    ok = np.ones((n, h_out, w_out), dtype=bool)
    for j in range(iy.shape[1]):
        rows = v[:, iy[:, j], :]                        # (n, h_out, w_in)
        fin = finite[:, iy[:, j], :]
        r = np.zeros((n, h_out, w_out), dtype=LD)
        m = np.zeros((n, h_out, w_out), dtype=LD)
        for k in range(ix.shape[1]):
            r = r + wx[None, None, :, k] * rows[:, :, ix[:, k]]
            m = m + np.abs(wx[None, None, :, k]) * np.abs(rows[:, :, ix[:, k]])
            ok &= fin[:, :, ix[:, k]]
        field = field + wy[None, :, j, None] * r
        mag = mag + np.abs(wy[None, :, j, None]) * m
    return np.where(ok, field, LD(np.nan)), mag, ok


class Reference:
    """the definition's field and sums of one operand set with their bounds, computed once and compared with many results.
    low (N, h_in, w_in), pred (N, h_out, w_out) or None, actual (N, h_out, w_out): fp64 values of channel 0"""

    def __init__(self, low, pred, actual, mode):
        actual = np.asarray(actual, dtype=np.float64)
        (self.n, self.h, self.w) = actual.shape
        self.mode = mode
        (field, mag, ok) = upsample(low, (self.h, self.w), mode)
        self.field = field
        self.beta = (LD(K * U) * mag)
        counted = ok & np.isfinite(actual)
        if pred is not None:
            pred = np.asarray(pred, dtype=np.float64)
            counted &= np.isfinite(pred)
        self.counted = counted
        z = LD(0)
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.where(counted, field - np.where(counted, actual, 0.0).astype(LD), z)
            e = np.where(counted, (np.where(counted, pred, 0.0).astype(LD) - np.where(counted, actual, 0.0).astype(LD)), z) \
                if pred is not None else np.zeros_like(d)
        beta = np.where(counted, self.beta, z)
        (ad, ae) = (np.abs(d), np.abs(e))
        cnt = counted.sum(axis=(1, 2)).astype(np.float64)
        s = lambda x: x.sum(axis=(1, 2))                # noqa: E731
        sums = np.zeros((self.n, 6), dtype=LD)
        bound = np.zeros((self.n, 6), dtype=LD)
        sums[:, 0] = cnt
        (sums[:, 1], sums[:, 2]) = (s(ad), s(d * d))
        bound[:, 1] = s(beta + U * ad) + cnt * U * s(ad)
        bound[:, 2] = s(2 * ad * beta + beta * beta + 3 * U * d * d) + cnt * U * s(d * d)
        self.undecided = 0
        if pred is not None:
            (sums[:, 3], sums[:, 4]) = (s(ae), s(e * e))
            bound[:, 3] = s(U * ae) + cnt * U * s(ae)
            bound[:, 4] = s(3 * U * e * e) + cnt * U * s(e * e)
            sums[:, 5] = (counted & (ae < ad)).sum(axis=(1, 2))
            self.undecided = int((counted & (np.abs(ae - ad) <= beta + 2 * U * (ad + ae))).sum())
        self.sums = sums.astype(np.float64)
        self.bound = bound.astype(np.float64)
        self.has_pred = pred is not None

    def field_ratio(self, got):
        """the largest |got - want| / bound over the pixels whose taps are finite; NaN positions must be equal"""
        got = np.asarray(got)
        assert got.shape == self.field.shape and got.dtype == np.float64, (got.shape, self.field.shape)
        nan = np.isnan(self.field)
        np.testing.assert_array_equal(np.isnan(got), nan)
        err = np.abs(np.where(nan, 0.0, got).astype(LD) - np.where(nan, LD(0), self.field))
        exact = (self.beta == 0) | nan
        assert (err[exact] == 0).all(), "a pixel whose taps are all zero must be exact"
        return float(np.max(np.where(exact, LD(0), err / np.where(exact, LD(1), self.beta)), initial=0.0)), err

    def check_field(self, got, label=""):
        (ratio, err) = self.field_ratio(got)
        print(f"baseline field {label} mode={self.mode} {self.field.shape}: max |got - want| / bound = {ratio:.3e}")
        assert (err <= np.where(np.isnan(self.field), LD(0), self.beta)).all(), (label, ratio)
        return ratio

    def ratio(self, got):
        err = np.abs(np.asarray(got, dtype=np.float64) - self.sums)
        b = self.bound
        return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0), initial=0.0))

    def check(self, got, label=""):
        """the kernel's sums against the definition: n and n_won exactly (no undecided pixel), the four sums within their
        bounds, +0.0 in what has no counted pixel or no prediction; prints and returns the largest |got - want| / bound"""
        got = np.asarray(got)
        assert got.shape == self.sums.shape and got.dtype == np.float64, (got.shape, self.sums.shape)
        assert self.undecided == 0, f"{self.undecided} pixels are undecided for n_won: pick another seed"
        np.testing.assert_array_equal(got[:, 0], self.sums[:, 0])
        np.testing.assert_array_equal(got[:, 5], self.sums[:, 5])
        empty = self.sums[:, 0] == 0
        assert (got[empty] == 0.0).all() and not np.signbit(got[empty]).any(), "a case without a counted pixel holds +0.0"
        if not self.has_pred:
            assert (got[:, 3:] == 0.0).all() and not np.signbit(got[:, 3:]).any()
        ratio = self.ratio(got)
        print(f"baseline sums {label} mode={self.mode} {self.field.shape}: max |got - want| / bound = {ratio:.3e}")
        assert (np.abs(got - self.sums)[:, 1:5] <= self.bound[:, 1:5]).all(), (label, ratio)
        return ratio
