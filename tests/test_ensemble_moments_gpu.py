"""cae_ensemble_moments (include/cae_hip.h) through ctypes on synthetic fp32 draws, against numpy's fp64 mean and
std(ddof=1) of the same draws, denormalised with vmin = 288.0, range = 10.5.

Bounds, from fp64 rounding at K <= 64 with about 100x margin: mean within 1e-11 absolute, std within 1e-10 relative plus
1e-12 * range.  Every pixel class is in every case: draws spread by 0.3, 1e-3, 1e-6 and 6e-8 (one fp32 ulp) around a random
base in [0, 1], and pixels whose draws are all equal, where std must be exactly 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VMIN, RANGE = 288.0, 10.5
MEAN_ABS, STD_REL, STD_ABS = 1e-11, 1e-10, 1e-12 * RANGE
SPREADS = (0.3, 1e-3, 1e-6, 6e-8, 0.0)      # pixel p belongs to class p % 5; 0.0: all draws equal
GUARD = 8                                    # sentinel doubles on both sides of each output plane set


def _draws(n_case, k, plane, seed):
    """(n_case, k, plane) fp32 draws and the fp64 answer (mean, std), (n_case, plane) each"""
    rng = np.random.default_rng(seed)
    base = rng.random((n_case, 1, plane))
    spread = np.asarray(SPREADS)[np.arange(plane) % len(SPREADS)]
    y = (base + spread * rng.standard_normal((n_case, k, plane))).astype(np.float32)
    y64 = y.astype(np.float64)
    return y, VMIN + y64.mean(axis=1) * RANGE, y64.std(axis=1, ddof=1) * RANGE


def _place(y, offset, layout, padded):
    """the draws on the device in [case][draw] or [draw][case] order, planes tight or on a pitch that is a multiple of 4
    floats, the whole shifted by `offset` floats from a 16-byte boundary: (holder, pointer, case_stride, draw_stride)"""
    (n_case, k, plane) = y.shape
    pitch = (plane + 3) // 4 * 4 + 4 if padded else plane
    rows = y if layout == "case" else y.transpose(1, 0, 2)
    host = np.full((rows.shape[0], rows.shape[1], pitch), np.float32(np.nan))
    host[:, :, :plane] = rows
    dev = torch.empty(host.size + offset, dtype=torch.float32, device="cuda")
    dev[offset:] = torch.from_numpy(host.reshape(-1)).cuda()
    (outer, inner) = (k * pitch, pitch) if layout == "case" else (pitch, n_case * pitch)
    return dev, dev.data_ptr() + 4 * offset, outer, inner


class _Out:
    """(n_case, plane) fp64 plane between two runs of 0xAA bytes"""

    def __init__(self, n_case, plane):
        self.n = n_case * plane
        self.raw = torch.full(((self.n + 2 * GUARD) * 8,), 0xAA, dtype=torch.uint8, device="cuda")
        self.ptr = self.raw.data_ptr() + 8 * GUARD

    def read(self):
        host = self.raw.cpu().numpy()
        assert (host[:8 * GUARD] == 0xAA).all() and (host[-8 * GUARD:] == 0xAA).all(), "a guard value was overwritten"
        return host[8 * GUARD:-8 * GUARD].view(np.float64).copy()


def _run(y, offset=0, layout="draw", padded=False, parts=None):
    """mean and std (n_case, plane) of the kernel; parts: the draws delivered over several calls through the workspace"""
    from cae_tools_amd import _lib
    from cae_tools_amd._lib import check
    lib = _lib.load()
    (n_case, k, plane) = y.shape
    (keep, ptr, case_stride, draw_stride) = _place(y, offset, layout, padded)
    (mean, std) = (_Out(n_case, plane), _Out(n_case, plane))
    stream = torch.cuda.current_stream().cuda_stream
    ws = ws_ptr = None
    ws_bytes = 0
    if parts is not None:
        ws_bytes = int(lib.cae_ensemble_moments_workspace_bytes(n_case, plane))
        assert ws_bytes == n_case * plane * 20
        ws = torch.full((ws_bytes + 2 * 64,), 0xAA, dtype=torch.uint8, device="cuda")
        ws_ptr = ws.data_ptr() + 64
    done = 0
    for kc in (parts or [k]):
        check(lib.cae_ensemble_moments(ptr + 4 * done * draw_stride, case_stride, draw_stride, n_case, plane, kc, done, k,
                                       VMIN, RANGE, mean.ptr, std.ptr, ws_ptr, ws_bytes, stream))
        done += kc
    assert done == k
    torch.cuda.synchronize()
    if ws is not None:
        host = ws.cpu().numpy()
        assert (host[:64] == 0xAA).all() and (host[-64:] == 0xAA).all(), "a workspace guard value was overwritten"
    del keep
    return mean.read().reshape(n_case, plane), std.read().reshape(n_case, plane)


def _check(got, ref, what):
    ((mean, std), (ref_mean, ref_std)) = (got, ref)
    mean_err = float(np.abs(mean - ref_mean).max())
    std_excess = float((np.abs(std - ref_std) - STD_REL * ref_std).max())
    print(f"{what}: max |mean error| {mean_err:.3e} (bound {MEAN_ABS:.0e}); max |std error| - 1e-10 * std {std_excess:.3e} "
          f"(bound {STD_ABS:.2e}); max relative std error {float((np.abs(std - ref_std) / np.maximum(ref_std, 1e-300)).max()):.3e}")
    assert np.isfinite(mean).all() and np.isfinite(std).all()
    assert mean_err <= MEAN_ABS, what
    assert std_excess <= STD_ABS, what
    equal = np.arange(mean.shape[1]) % len(SPREADS) == len(SPREADS) - 1
    assert (std[:, equal] == 0.0).all(), f"{what}: equal draws must give a standard deviation of exactly 0"


@pytest.mark.parametrize("n_case", [1, 3])
@pytest.mark.parametrize("k", [2, 3, 17, 64])
@pytest.mark.parametrize("plane", [1, 3, 35, 4099, 30976])
def test_moments_match_numpy_fp64(plane, k, n_case):
    (y, ref_mean, ref_std) = _draws(n_case, k, plane, seed=plane * 131 + k * 7 + n_case)
    # offset 0 / 1 float; the engine's [draw][case] order tight, and [case][draw] on a 16-byte pitch (vector loads behind
    # a head and before a tail for every plane); tight odd planes take the scalar loads
    for (offset, layout, padded) in ((0, "draw", False), (1, "draw", False), (0, "case", True), (1, "case", True)):
        _check(_run(y, offset, layout, padded), (ref_mean, ref_std), f"plane {plane} K {k} cases {n_case} offset {offset} {layout}")


def test_all_draws_equal_is_exactly_zero():
    rng = np.random.default_rng(5)
    y = np.repeat(rng.random((3, 1, 4099)).astype(np.float32), 17, axis=1)
    (mean, std) = _run(y, offset=1)
    assert (std == 0.0).all()
    assert np.abs(mean - (VMIN + y[:, 0].astype(np.float64) * RANGE)).max() <= MEAN_ABS


@pytest.mark.parametrize("k,parts", [(5, [2, 2, 1]), (9, [4, 4, 1])])
@pytest.mark.parametrize("plane", [3, 35, 4099])
def test_split_delivery_through_the_workspace(plane, k, parts):
    (y, ref_mean, ref_std) = _draws(3, k, plane, seed=plane + k)
    for (offset, layout, padded) in ((0, "draw", False), (1, "case", True)):
        got = _run(y, offset, layout, padded, parts=parts)
        _check(got, (ref_mean, ref_std), f"plane {plane} K {k} as {parts} offset {offset} {layout}")
        whole = _run(y, offset, layout, padded)
        # the same sums in the same order, y_0 kept as the fp32 it is: the cut into calls does not change a bit
        assert all(np.array_equal(a, b) for a, b in zip(got, whole))


def test_two_runs_are_bitwise_equal():
    (y, _, _) = _draws(3, 17, 4099, seed=11)
    (a, b) = (_run(y, 1, "case", True), _run(y, 1, "case", True))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    (a, b) = (_run(y, 0, "draw", False, parts=[8, 8, 1]), _run(y, 0, "draw", False, parts=[8, 8, 1]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
