"""Numpy restatement of cae_case_spectra (include/cae_hip.h) shared by test_spectra_cpu.py and
test_case_spectra_gpu.py, with np.fft.rfft2 in fp64 in place of the kernel's direct DFT, and the bound the sums are held to.

Definition.  For case c, channel 0 (H x W), prediction p and target a taken to fp64 as stored, d = p - a per pixel.  A case
in which any pixel of p or a is not finite is not counted: zero sums, counted 0.  For each field x of {p, a, d}:
    mu = (S x) / (H W),   x'[j, i] = (x[j, i] - mu) wy[j] wx[i],   X = the DFT of x' at ky in [0, H), kx in [0, W / 2]
(S x exactly rounded, math.fsum: the rounding of a plain sum of values near 290 is as large as the bound on a small plane)
with the centred Hann window wy[j] = 1/2 - 1/2 cos(2 pi (j + 1/2) / H) (a single 1 for H == 1), wx likewise.  With
weight(kx) = 1 if kx == 0 or 2 kx == W else 2:
    sums[c][b] = {S weight |P|^2, S weight |A|^2, S weight Re(P conj A), S weight |D|^2} over the modes of bin b
    M = max(1, min(H, W) // 2) bins;  ky' = min(ky, H - ky),  bin = isqrt((4 M^2 (ky'^2 W^2 + kx^2 H^2)) // (H^2 W^2)),
    which is floor(2 M f) for f = sqrt((ky' / H)^2 + (kx / W)^2) cycles per pixel; -1 (left out) for mode (0, 0) and where
    the value reaches M.

Bound.  For the sum over bin b of fields x, y:  |got - want| <= 4 (H + W + 16) 2^-53 L1(x') L1(y') modes_b  with L1 the sum
of |x'| over the plane and modes_b the sum of the weights over the bin: each coefficient is a sum of H + W rounded
products bounded by L1; the 16 and the factor 4 cover the twiddles' ulps, the window products and the bin additions."""
import math

import numpy as np


def channel0(x):
    return np.asarray(x)[:, 0].astype(np.float64)


def window(n):
    if n == 1:
        return np.ones(1)
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * (j + 0.5) / n) for j in range(n)])


def bin_count(h, w):
    return max(1, min(h, w) // 2)


def bin_table(h, w):
    m = bin_count(h, w)
    table = np.full((h, w // 2 + 1), -1, dtype=np.int64)
    for ky in range(h):
        kyp = min(ky, h - ky)
        for kx in range(w // 2 + 1):
            if ky == 0 and kx == 0:
                continue
            b = math.isqrt((4 * m * m * (kyp * kyp * w * w + kx * kx * h * h)) // (h * h * w * w))
            if b < m:
                table[ky, kx] = b
    return table


def weights(w):
    return np.array([1.0 if kx == 0 or 2 * kx == w else 2.0 for kx in range(w // 2 + 1)])


def modes(h, w, table=None):
    table = bin_table(h, w) if table is None else table
    out = np.zeros(max(int(table.max()) + 1, bin_count(h, w)))
    wt = weights(w)
    for ky in range(h):
        for kx in range(w // 2 + 1):
            if table[ky, kx] >= 0:
                out[table[ky, kx]] += wt[kx]
    return out


def case_sums(p, a, wy=None, wx=None, table=None, n_bin=None):
    """p, a: (N, H, W) arrays.  Returns (sums (N, n_bin, 4), counted (N,) bool, l1 (N, 3): L1 of p', a', d').
    wy, wx, table, n_bin default to the definition's; the orientation test passes all-ones windows."""
    p = np.asarray(p).astype(np.float64)
    a = np.asarray(a).astype(np.float64)
    (n, h, w) = p.shape
    wy = window(h) if wy is None else np.asarray(wy, dtype=np.float64)
    wx = window(w) if wx is None else np.asarray(wx, dtype=np.float64)
    table = bin_table(h, w) if table is None else np.asarray(table)
    n_bin = bin_count(h, w) if n_bin is None else n_bin
    wt = np.broadcast_to(weights(w), table.shape)
    sums = np.zeros((n, n_bin, 4))
    counted = np.zeros(n, dtype=bool)
    l1 = np.zeros((n, 3))
    keep = (table >= 0) & (table < n_bin)
    for c in range(n):
        if not (np.isfinite(p[c]).all() and np.isfinite(a[c]).all()):
            continue
        counted[c] = True
        spec = []
        for (k, x) in enumerate((p[c], a[c], p[c] - a[c])):
            xw = (x - math.fsum(x.ravel().tolist()) / (h * w)) * wy[:, None] * wx[None, :]
            l1[c, k] = np.abs(xw).sum()
            spec.append(np.fft.rfft2(xw))
        (P, A, D) = spec
        terms = (np.abs(P) ** 2, np.abs(A) ** 2, (P * np.conj(A)).real, np.abs(D) ** 2)
        for (k, t) in enumerate(terms):
            sums[c, :, k] = np.bincount(table[keep], weights=(wt * t)[keep], minlength=n_bin)
    return sums, counted, l1


def bounds(h, w, l1, mode_count):
    """(N, n_bin, 4): the bound of every sum, from l1 (N, 3) and the bins' mode counts"""
    (lp, la, ld) = (l1[:, 0], l1[:, 1], l1[:, 2])
    pairs = np.stack([lp * lp, la * la, lp * la, ld * ld], axis=-1)                 # (N, 4)
    return 4.0 * (h + w + 16) * 2.0 ** -53 * pairs[:, None, :] * np.asarray(mode_count)[None, :, None]


class Reference:
    """the definition's sums of one operand pair with their bounds, computed once and compared with many results"""

    def __init__(self, p, a, **definition):
        p = np.asarray(p)
        (self.n, self.h, self.w) = p.shape
        (self.sums, self.counted, l1) = case_sums(p, a, **definition)
        table = definition.get("table")
        if table is not None:                   # entries outside [0, n_bin) leave their mode out
            table = np.where((np.asarray(table) >= 0) & (np.asarray(table) < self.sums.shape[1]), np.asarray(table), -1)
        self.modes = modes(self.h, self.w, table)[:self.sums.shape[1]]
        self.bound = bounds(self.h, self.w, l1, self.modes)

    def check(self, got_sums, got_counted, label=""):
        """the kernel's sums against the definition within the bound, counted exactly, exact zeros where no mode or no
        case counts; prints and returns the largest |got - want| / bound"""
        got_sums = np.asarray(got_sums)
        assert got_sums.shape == self.sums.shape and got_sums.dtype == np.float64, (got_sums.shape, self.sums.shape)
        np.testing.assert_array_equal(np.asarray(got_counted, dtype=bool), self.counted)
        err = np.abs(got_sums - self.sums)
        empty = self.bound == 0.0
        assert (got_sums[empty] == 0.0).all(), "a sum without a mode or of a case that is not counted must be an exact zero"
        ratio = float(np.max(np.where(empty, 0.0, err / np.where(empty, 1.0, self.bound)), initial=0.0))
        print(f"spectra {label} {self.h}x{self.w} n={self.n}: max |got - want| / bound = {ratio:.3e}")
        assert (err <= self.bound).all(), (label, self.h, self.w, ratio)
        return ratio


def check_case_sums(got_sums, got_counted, p, a, label="", **definition):
    return Reference(p, a, **definition).check(got_sums, got_counted, label)


def curves(ref):
    """(curves, bounds): the derived curves of DESIGN.md section 9 from a Reference's sums added in case order, as arrays
    over the bins, and what the sums' bounds allow each of them to differ by.  S = S_c sums[c]; B = S_c bound[c] plus the
    n additions' n 2^-53 |S|.  A quotient x / y with |dx| <= bx, |dy| <= by differs by at most (bx + |x / y| by) / (|y| - by)
    plus the division's own rounding; the coherence by the same rule to first order in the relative bounds, doubled.
    Where |y| <= 2 by the quotient is not constrained."""
    u = 2.0 ** -53
    S = np.zeros(ref.sums.shape[1:])
    for c in range(ref.n):
        S = S + ref.sums[c]
    B = ref.bound.sum(axis=0) + ref.n * u * np.abs(S)
    n_counted = int(ref.counted.sum())
    norm = n_counted * ref.modes * (window(ref.h) ** 2).sum() * (window(ref.w) ** 2).sum()
    (pp, aa, pa, dd) = S.T
    (bp, ba, bc, bd) = B.T
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"psd_pred": pp / norm, "psd_target": aa / norm, "power_ratio": pp / aa, "coherence": pa / np.sqrt(pp * aa),
               "error_share": dd / aa}
        # a denominator no larger than twice its own bound is not resolved: the quotient is then not constrained (inf);
        # the two psd curves hold those bins to the sums' bounds all the same
        (res_a, res_p) = (aa > 2.0 * ba, pp > 2.0 * bp)
        tol = {"psd_pred": bp / norm, "psd_target": ba / norm,
               "power_ratio": np.where(res_a, (bp + out["power_ratio"] * ba) / (aa - ba), np.inf),
               "error_share": np.where(res_a, (bd + out["error_share"] * ba) / (aa - ba), np.inf),
               "coherence": np.where(res_a & res_p, 2.0 * (bc / np.sqrt(pp * aa)
                                                           + np.abs(out["coherence"]) * 0.5 * (bp / pp + ba / aa)), np.inf)}
        for k in out:
            out[k] = np.where(norm > 0, out[k], np.nan) if k.startswith("psd") else out[k]
            tol[k] = tol[k] + 8 * u * np.abs(out[k])
    out["modes"] = ref.modes
    out["wavelength"] = 2.0 * ref.sums.shape[1] / (np.arange(ref.sums.shape[1]) + 0.5)
    return out, tol
