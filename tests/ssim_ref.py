"""Numpy restatement of cae_case_ssim (include/cae_hip.h) shared by test_ssim_cpu.py and
test_case_ssim_gpu.py: the filters and the per-window terms by slicing with np.longdouble accumulation, no torch, and the
bound the sums are held to.

Definition.  For case c, channel 0 (H x W), prediction p and target a taken to fp64 as stored:
    x = (p - shift) * scale,  y = (a - shift) * scale        in fp64, the subtraction and the product each rounded
with shift = vmin, scale = 1 / (vmax - vmin).  Scale 0 is (x, y); scale s + 1 is the 2 x 2 average of scale s in fp64,
((x00 + x01) + (x10 + x11)) * 0.25, with pad = size mod 2 zeros on both sides of an axis, output side (size + 2 pad) // 2;
NaN and Inf go through it as IEEE arithmetic carries them.  These two steps are fp64 operations of the definition, so the
reference does them in fp64 too and sees the same planes as the kernel, bit for bit.
At every scale a pixel is bad when x or y is not finite there; a bad pixel enters the filters as 0 in both fields.  G is
the separable valid filter with the 11-tap window (sigma 1.5: the fp32 values of vae_oracle.gaussian_window cast to double),
along the row first, then along the column.  For every window position
    mu1 = G(x), mu2 = G(y), s11 = G(x x) - mu1^2, s22 = G(y y) - mu2^2, s12 = G(x y) - mu1 mu2
    cs = (2 s12 + C2) / (s11 + s22 + C2),  ssim = ((2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)) cs,  C1 = 1e-4, C2 = 9e-4
and the window counts iff none of the 121 pixels under it is bad.  sums[c][s] = {n, S ssim, S cs} over the counted windows;
three zeros for a scale with a side below 11 or without a counted window.

Bound.  With u = 2^-53, for the counted windows of a (case, scale):
    |got S cs   - want| <= K u S_w M2 / D2                     + n u S_w |cs|
    |got S ssim - want| <= K u S_w (M2 / D2 + M1 / D1)         + n u S_w |ssim|
    M2 = G(x^2) + G(y^2) + 2 G|x y| + C2,  D2 = s11 + s22 + C2,  M1 = G(x^2) + G(y^2) + C1,  D1 = mu1^2 + mu2^2 + C1,  K = 64.
Why: a filtered moment is two passes of eleven fused multiply-adds over rounded products, (11 + 11 + 2) u G|v| at most;
the subtraction of mu1 mu2 adds 3 u of terms that G(x^2), G(y^2) bound (mu^2 <= G(v^2), |mu1 mu2| <= (G(x^2) + G(y^2)) / 2),
so numerator and denominator of cs are each within 27 u M2 of their exact value, and since |cs| <= 1 the quotient is within
(27 + 27) u M2 / D2 to first order; the division, the product l cs and one ulp of difference in a pooled pixel (another fp64
implementation may add the four in another order: 2 u G|v| per moment) take the rest of K = 64.  The luminance factor obeys
the same rule with M1 / D1, and |l| <= 1, |cs| <= 1 make the errors of the product add.  A sum of n terms in any order is
within (n - 1) u S|t|.  The bound on a scale's mean, bound / n, is asserted to stay below 1e-9 at every shape a test uses:
dropping the window's smallest tap (1.0e-3) moves the terms by about that tap, six orders above it.
"""
import numpy as np

WIN = 11
C1, C2 = 0.01 ** 2, 0.03 ** 2
K = 64.0
U = 2.0 ** -53
MEAN_BOUND = 1e-9
MS_WEIGHTS = tuple(float(v) for v in np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], dtype=np.float32))

_HALF = ("0x1.0d957p-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2")


def window():
    half = [float.fromhex(v) for v in _HALF]
    return np.array(half + half[-2::-1], dtype=np.float64)


def channel0(x):
    return np.asarray(x)[:, 0].astype(np.float64)


def normalise(v, vmin, vmax):
    """(v - vmin) * (1 / (vmax - vmin)) in fp64, each operation rounded"""
    scale = np.float64(1.0) / (np.float64(vmax) - np.float64(vmin))
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(v, dtype=np.float64) - np.float64(vmin)) * scale


def pool(x):
    """one level of the pyramid in fp64"""
    (h, w) = x.shape
    (ph, pw) = (h % 2, w % 2)
    z = np.zeros((h + 2 * ph, w + 2 * pw), dtype=np.float64)
    z[ph:ph + h, pw:pw + w] = x
    (ho, wo) = ((h + 2 * ph) // 2, (w + 2 * pw) // 2)
    z = z[:2 * ho, :2 * wo]
    with np.errstate(invalid="ignore", over="ignore"):
        return ((z[0::2, 0::2] + z[0::2, 1::2]) + (z[1::2, 0::2] + z[1::2, 1::2])) * 0.25


def _filter(v, g):
    """rows, then columns, valid; v longdouble (H, W)"""
    (h, w) = v.shape
    rows = np.zeros((h, w - WIN + 1), dtype=np.longdouble)
    for t in range(WIN):
        rows += g[t] * v[:, t:t + w - WIN + 1]
    out = np.zeros((h - WIN + 1, w - WIN + 1), dtype=np.longdouble)
    for t in range(WIN):
        out += g[t] * rows[t:t + h - WIN + 1, :]
    return out


def scale_terms(x, y, g):
    """one scale of one case: (counted (Hv, Wv) bool, ssim, cs, M2 / D2, M1 / D1 as longdouble maps), or None where a side
    is below 11"""
    (h, w) = x.shape
    if h < WIN or w < WIN:
        return None
    bad = ~(np.isfinite(x) & np.isfinite(y))
    xl = np.where(bad, 0.0, x).astype(np.longdouble)
    yl = np.where(bad, 0.0, y).astype(np.longdouble)
    gl = np.asarray(g, dtype=np.longdouble)
    counted = _filter(bad.astype(np.longdouble), np.ones(WIN, dtype=np.longdouble)) == 0
    (mu1, mu2) = (_filter(xl, gl), _filter(yl, gl))
    (gxx, gyy, gxy) = (_filter(xl * xl, gl), _filter(yl * yl, gl), _filter(xl * yl, gl))
    (s11, s22, s12) = (gxx - mu1 * mu1, gyy - mu2 * mu2, gxy - mu1 * mu2)
    d2 = s11 + s22 + C2
    d1 = mu1 * mu1 + mu2 * mu2 + C1
    cs = (2 * s12 + C2) / d2
    ssim = ((2 * mu1 * mu2 + C1) / d1) * cs
    m2 = gxx + gyy + 2 * _filter(np.abs(xl * yl), gl) + C2
    m1 = gxx + gyy + C1
    return counted, ssim, cs, m2 / d2, m1 / d1


def case_sums(p, a, vmin, vmax, n_scale, g=None):
    """p, a: (N, H, W) arrays.  Returns (sums (N, n_scale, 3) float64, bound (N, n_scale, 3) float64)."""
    g = window() if g is None else np.asarray(g, dtype=np.float64)
    p = np.asarray(p)
    a = np.asarray(a)
    n = p.shape[0]
    sums = np.zeros((n, n_scale, 3))
    bound = np.zeros((n, n_scale, 3))
    for c in range(n):
        (x, y) = (normalise(p[c], vmin, vmax), normalise(a[c], vmin, vmax))
        for s in range(n_scale):
            terms = scale_terms(x, y, g)
            if terms is not None:
                (counted, ssim, cs, r2, r1) = terms
                k = int(counted.sum())
                if k:
                    sums[c, s] = (k, float(ssim[counted].sum()), float(cs[counted].sum()))
                    b_cs = K * U * float(r2[counted].sum())
                    b_l = K * U * float(r1[counted].sum())
                    bound[c, s, 1] = b_cs + b_l + k * U * float(np.abs(ssim[counted]).sum())
                    bound[c, s, 2] = b_cs + k * U * float(np.abs(cs[counted]).sum())
            (x, y) = (pool(x), pool(y))
    return sums, bound


def scale_shapes(h, w, n_scale):
    out = []
    for _ in range(n_scale):
        out.append((h, w))
        (h, w) = ((h + 2 * (h % 2)) // 2, (w + 2 * (w % 2)) // 2)
    return out


def scores(sums, h, w, mse=None, vmin=0.0, vmax=1.0):
    """ssim, ms_ssim, psnr per case as the issue defines them, in plain loops"""
    sums = np.asarray(sums)
    n = sums.shape[0]
    (ssim, ms, psnr) = (np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan))
    for c in range(n):
        if sums[c, 0, 0] > 0:
            ssim[c] = sums[c, 0, 1] / sums[c, 0, 0]
        if sums.shape[1] == 5 and min(h, w) > 160 and (sums[c, :, 0] > 0).all():
            v = 1.0
            for s in range(5):
                f = (sums[c, s, 2] if s < 4 else sums[c, s, 1]) / sums[c, s, 0]
                v *= max(f, 0.0) ** MS_WEIGHTS[s]
            ms[c] = v
        if mse is not None:
            m = float(mse[c])
            if m == 0:
                psnr[c] = np.inf
            elif m > 0:
                psnr[c] = 10.0 * np.log10((float(vmax) - float(vmin)) ** 2 / m)
    return ssim, ms, psnr


class Reference:
    """the definition's sums of one operand pair with their bounds, computed once and compared with many results"""

    def __init__(self, p, a, vmin, vmax, n_scale, g=None):
        p = np.asarray(p)
        (self.n, self.h, self.w) = p.shape
        self.n_scale = n_scale
        (self.sums, self.bound) = case_sums(p, a, vmin, vmax, n_scale, g)
        some = self.sums[:, :, 0] > 0
        self.mean_bound = float(np.max(np.where(some[..., None], self.bound / np.where(some, self.sums[:, :, 0], 1.0)[..., None], 0.0),
                                       initial=0.0))
        assert self.mean_bound < MEAN_BOUND, f"the bound on a scale's mean is {self.mean_bound:.3e} at {self.h} x {self.w}"

    def ratio(self, got):
        """the largest |got - want| / bound over the sums that have a bound"""
        err = np.abs(np.asarray(got, dtype=np.float64) - self.sums)[:, :, 1:]
        b = self.bound[:, :, 1:]
        return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0), initial=0.0))

    def check(self, got, label=""):
        """the kernel's sums against the definition: n exactly, the two sums within the bound, exact non-negative zeros
        where no window counts; prints and returns the largest |got - want| / bound"""
        got = np.asarray(got)
        assert got.shape == self.sums.shape and got.dtype == np.float64, (got.shape, self.sums.shape)
        np.testing.assert_array_equal(got[:, :, 0], self.sums[:, :, 0])
        empty = self.sums[:, :, 0] == 0
        assert (got[empty] == 0.0).all() and not np.signbit(got[empty]).any(), "a scale without a counted window must hold +0.0"
        ratio = self.ratio(got)
        print(f"ssim {label} {self.h}x{self.w} n={self.n} scales={self.n_scale}: max |got - want| / bound = {ratio:.3e} "
              f"(bound on a mean {self.mean_bound:.3e})")
        assert (np.abs(got - self.sums)[:, :, 1:] <= self.bound[:, :, 1:]).all(), (label, self.h, self.w, ratio)
        return ratio
