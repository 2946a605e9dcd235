"""What the MS-SSIM parity tests of the 'var' path share (tests/test_vae_msssim_gpu.py on the device, tests/test_vae_msssim_criterion_cpu.py
on the oracle alone): the geometries, the synthetic maps, and the per-pixel bound

    per (batch, channel) plane:  max|got - g64| <= 3 * max|g32 - g64| + 1e-5 * max|g64|

- form and constants of helpers.assert_close_as_reference - on d(lambda_ssim * (1 - MS-SSIM)) / dy, with g32 / g64 the fp32 / fp64
definition (oracle/vae_oracle.py loss_parts_and_ssim_grad) evaluated at the SAME y."""
import numpy as np
import torch

FACTOR, FLOOR_REL = 3.0, 1e-5
LAMBDAS = dict(lambda_mse=0.7, lambda_kl=0.3, lambda_ssim=1.5)
STRIP = 54      # output columns of a wave of the row-streaming kernels (kernels_vae.h kSsimCols)

# output (H, W) -> what it exercises in the row-streaming kernels
GEOMETRIES = {
    (176, 176): "smallest legal size: scale 4 is 11 x 11, its valid region 1 x 1",
    (176, 256): "scale 2 is 64 wide, valid width 54: exactly one full forward strip",
    (176, 432): "backward strips fill exactly at every scale (8, 4, 2, 1 strips; 27 < 54); last forward strip 44 columns",
    (416, 176): "forward band of 32 rows (406 valid rows: 13 bands, last workgroup one live wave, last band 22 rows); backward band 16",
    (208, 240): "forward and backward band heights differ (198 -> 8, 208 -> 16); five forward strips, the last 14 columns",
}


def band_rows(rows, forward):
    """rows of a wave's band by the map's height (kernels_vae.h ssim_band_rows)"""
    return (32 if forward else 16) if rows >= 400 else (16 if rows >= 200 else 8)


def locate(H, W, row, col):
    """where pixel (row, col) of the finest map lies in the row-streaming kernels' decomposition of scale 0"""
    (bb, fb) = (band_rows(H, False), band_rows(H - 10, True))
    (c0, c1) = (max(0, col - 10), min(col, W - 11))     # valid outputs that read this pixel
    (r0, r1) = (max(0, row - 10), min(row, H - 11))
    return (f"backward strip {col // STRIP} (lane {col % STRIP + 10}) band {row // bb} (row {row % bb} of {bb}); "
            f"read by forward strips {c0 // STRIP}..{c1 // STRIP}, forward bands {r0 // fb}..{r1 // fb} of {fb} rows")


def synthetic_pair(size, B, C, seed):
    """(y, t) of shape (B, C, H, W) in (0, 1): the target as test_vae_hip_parity._setup draws it (a sinusoid per sample + noise,
    here with a phase per channel), the output the same sinusoid damped and shifted in phase, with more noise: correlated
    with the target at every scale, as a half-trained model's output is"""
    (H, W) = size
    g = torch.Generator().manual_seed(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    t = torch.stack([torch.stack([torch.from_numpy((0.5 + 0.4 * np.sin(3 * yy * (b + 1) + 2 * xx + 0.7 * c)).astype(np.float32))
                                  for c in range(C)]) for b in range(B)])
    y = torch.stack([torch.stack([torch.from_numpy((0.5 + 0.3 * np.sin(3 * yy * (b + 1) + 2 * xx + 0.7 * c + 0.5)).astype(np.float32))
                                  for c in range(C)]) for b in range(B)])
    t = (t + 0.03 * torch.randn(t.shape, generator=g)).clamp(0, 1)
    y = (y + 0.05 * torch.randn(y.shape, generator=g)).clamp(0.02, 0.98)
    return y, t


def plane_ratios(got, g32, g64):
    """per plane of (P, H, W) arrays: (|got - g64|_max / bound, bound, the fp32 definition's own error, max|g64|)"""
    (got, g32, g64) = (np.asarray(a, dtype=np.float64) for a in (got, g32, g64))
    out = []
    for p in range(g64.shape[0]):
        scale = float(np.abs(g64[p]).max())
        own = float(np.abs(g32[p] - g64[p]).max())
        bound = FACTOR * own + FLOOR_REL * scale
        err = float(np.abs(got[p] - g64[p]).max())
        out.append((err / bound if bound > 0 else (0.0 if err == 0 else np.inf), bound, own, scale))
    return out


def assert_planes_close(got, g32, g64, what, skip=()):
    """the per-pixel bound on every plane of (P, H, W) (but `skip`); a failure names the worst pixel and where it lies.
    Returns the worst ratio |got - g64| / bound."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), f"{what}: NaN or Inf in the result"
    (H, W) = got.shape[-2:]
    worst = 0.0
    for p, (ratio, bound, own, scale) in enumerate(plane_ratios(got, g32, g64)):
        if p in skip:
            continue
        if ratio > 1.0:
            d = np.abs(got[p] - np.asarray(g64[p], dtype=np.float64))
            (r, c) = np.unravel_index(int(d.argmax()), d.shape)
            raise AssertionError(
                f"{what}: plane {p} pixel (row {r}, col {c}): got {got[p, r, c]:.9e}, fp64 {float(g64[p][r, c]):.9e}, "
                f"fp32 definition {float(g32[p][r, c]):.9e}; |got - fp64| = {d[r, c]:.3e} > bound {bound:.3e} "
                f"(fp32 definition's own error {own:.3e}, plane maximum {scale:.3e}; {int((d > bound).sum())} pixels over); "
                + locate(H, W, int(r), int(c)))
        worst = max(worst, ratio)
    return worst
