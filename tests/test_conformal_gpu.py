"""cae_score_quantiles, cae_score_counts and cae_interval_bounds on the GPU against the numpy restatement of their definition
(conformal_ref.py): the quantiles bit for bit (np.array_equal on the doubles' bit patterns), n and the counts integer for
integer, for every plane and number of cases on both sides of the first finite ranks and of 8- and 16-bit counters, every
field that stresses one end of the radix select (ties, keys that differ only in the lowest or only in the highest digits,
zeros of both signs, +inf scores, gaps), every element kind, a scale with values that take pixels out, and unaligned case
starts; the defining identities of a k-th smallest value on the GPU's own output; then train_cae -> calibrate -> apply_cae
--interval for a conv and a linear model with every stored bound recomputed, and the two commands on a unet and a var model
folder.  No tolerance anywhere.

Every check on finite data first asserts that the restatement has a finite quantile in at least half of its groups for at
least one level, so none passes on +inf alone."""
import io
import json
import os
from contextlib import redirect_stdout
from fractions import Fraction

import numpy as np
import pytest
import torch

import conformal_ref
from cae_tools_amd import _lib
from cae_tools_amd.case_ops import DeviceOperand, _args, _stream
from cae_tools_amd.engine import device_operand, interval_bounds, score_counts, score_quantiles
from cae_tools_amd.utils import conformal

pytestmark = pytest.mark.gpu

LEVELS = ["1/2", "4/5", "9/10", "19/20"]
DTYPES = {"f32": np.dtype("<f4"), "f32be": np.dtype(">f4"), "f64": np.dtype("<f8"), "f64be": np.dtype(">f8")}
KINDS = {"f32": _lib.ELEM_F32, "f32be": _lib.ELEM_F32_BE, "f64": _lib.ELEM_F64, "f64be": _lib.ELEM_F64_BE}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def ranks(n, levels):
    """k per level and group, as integers"""
    n = np.asarray(n, dtype=np.int64)
    return np.array([((n + 1) * Fraction(v).numerator + Fraction(v).denominator - 1) // Fraction(v).denominator for v in levels])


def verify(p, a, group, s=None, levels=LEVELS, finite=True, operands=None, twice=False):
    """score_quantiles and score_counts on (p, a, s) - or on `operands`, device operands that hold the same values - against
    the restatement; returns (q, n)"""
    (want_q, want_n) = conformal_ref.quantiles(p, a, levels, group, s)
    if finite:      # the check is not passed on +inf alone
        share = max(float(np.isfinite(np.atleast_1d(row)).mean()) for row in want_q) if np.size(want_q) else 0.0
        assert share >= 0.5, share
    (dp, da, dsc) = operands if operands is not None else (p, a, s)
    (q, n) = score_quantiles(dp, da, levels, group=group, scale=dsc)
    assert q.dtype == np.float64 and n.dtype == np.int64 and q.shape == want_q.shape and n.shape == np.shape(want_n)
    assert np.array_equal(n, want_n)                        # n is the pair count
    assert np.array_equal(bits(q), bits(want_q)), (int((bits(q) != bits(want_q)).sum()), q.size)
    assert (q[1:] >= q[:-1]).all()                          # non-decreasing in the level
    # the identities of a k-th smallest value, on the GPU's own output: at least k scores <= q, fewer than k scores < q
    (le, n2) = score_counts(dp, da, q, group, scale=dsc)
    (lt, _) = score_counts(dp, da, np.nextafter(q, -np.inf), group, scale=dsc)
    k = ranks(n, levels).reshape(q.shape)
    fin = np.isfinite(q)
    assert np.array_equal(n2, want_n)
    assert (le[fin] >= k[fin]).all() and (lt[fin] < k[fin]).all()
    (want_le, _) = conformal_ref.counts(p, a, q, group, s)
    (want_lt, _) = conformal_ref.counts(p, a, q, group, s, strict=True)
    assert np.array_equal(le, want_le) and np.array_equal(lt[fin], want_lt[fin])
    # where the rank is beyond n the quantile is +inf
    assert (q[k > np.broadcast_to(n, k.shape)] == np.inf).all()
    if twice:
        (q2, n3) = score_quantiles(dp, da, levels, group=group, scale=dsc)
        assert q2.tobytes() == q.tobytes() and n3.tobytes() == n.tobytes()
    return q, n


def noise(rng, n, h, w, gaps=0.05, dtype=np.float32):
    """uniform noise with a share of NaN in the target, so that n differs from pixel to pixel"""
    p = rng.random((n, 1, h, w)).astype(dtype)
    a = rng.random((n, 1, h, w)).astype(dtype)
    if gaps:
        a[rng.random(a.shape) < gaps] = np.nan
    return p, a


# ---- shapes ---------------------------------------------------------------------------------------------------------

PLANES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 65), (66, 128), (130, 193)]
CASES = [1, 2, 8, 9, 18, 19, 20, 255, 256, 257, 1000]


@pytest.mark.parametrize("n", CASES)
@pytest.mark.parametrize("plane", PLANES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pixel_shapes(plane, n):
    (h, w) = plane
    rng = np.random.default_rng(1000 * h + 7 * w + n)
    (p, a) = noise(rng, n, h, w, gaps=0.0 if h * w == 1 else 0.05)
    verify(p, a, "pixel", twice=(n in (19, 257)))


def test_pixel_past_16_bit_counters():
    n = 65537
    p = np.full((n, 1, 1, 2), 1.75, dtype=np.float32)
    a = np.full((n, 1, 1, 2), 0.5, dtype=np.float32)
    (q, cnt) = verify(p, a, "pixel")
    assert (q == 1.25).all() and (cnt == n).all()


@pytest.mark.parametrize("shape", [(1, 1, 1), (63, 1, 1), (1, 1, 64), (5, 1, 13), (17, 1, 241)], ids=lambda s: str(s[0] * s[1] * s[2]))
def test_pooled_small_totals(shape):
    (n, h, w) = shape
    rng = np.random.default_rng(n * h * w)
    (p, a) = noise(rng, n, h, w, gaps=0.0)
    verify(p, a, "pooled", twice=True)


def test_pooled_a_million_scores():
    rng = np.random.default_rng(17)
    (p, a) = noise(rng, 17, 256, 256)
    (q, n) = verify(p, a, "pooled", twice=True)
    assert 0 < n < 17 * 65536 and np.isfinite(q).all()


def test_pooled_equal_scores():
    p = np.full((70000, 1, 1, 1), -2.5)
    a = np.full((70000, 1, 1, 1), 0.25)
    (q, n) = verify(p, a, "pooled")
    assert (q == 2.75).all() and n == 70000


# ---- fields ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def circle():
    """the datagen circle pattern, the prediction rolled by a column plus small noise: (p, a), 24 cases of 256 x 256"""
    from cae_tools_amd.data import datagen
    a = np.asarray(datagen.generate("circle", 24, seed=1234)["hires"].values).astype(np.float32)
    rng = np.random.default_rng(3)
    p = (np.roll(a, 1, axis=-1) + 0.01 * rng.standard_normal(a.shape)).astype(np.float32)
    return p, a


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_circle_pattern(circle, group):
    (p, a) = circle
    verify(p, a, group, twice=True)


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_constant_field(group):
    p = np.full((40, 1, 3, 65), 288.5)
    a = np.full((40, 1, 3, 65), 288.0)
    (q, n) = verify(p, a, group)
    assert (q == 0.5).all()


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_two_values_with_the_rank_on_the_boundary(group):
    """20 scores per pixel, rank 19 for 9/10: 18 ones and 2 twos give 2, 19 ones and a two give 1"""
    a = np.zeros((20, 1, 2, 65))
    p = np.ones((20, 1, 2, 65))
    p[18:, :, 0] = 2.0
    p[19:, :, 1] = 2.0
    rng = np.random.default_rng(4)
    p = np.take_along_axis(p, np.argsort(rng.random(p.shape), axis=0), axis=0)       # the cases shuffled pixel by pixel
    (q, n) = verify(p, a, group, levels=["9/10"])
    if group == "pixel":
        assert (q[0, 0] == 2.0).all() and (q[0, 1] == 1.0).all()
    else:       # 2600 scores, rank 2341: 37 x 65 = 2405 ones
        assert q[0] == 1.0


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_keys_that_differ_in_the_lowest_digits(group):
    n = 300
    rng = np.random.default_rng(6)
    e = 1.0 + np.arange(n * 2 * 33, dtype=np.float64).reshape(n, 1, 2, 33) * 2.0 ** -52
    e = np.take_along_axis(e, np.argsort(rng.random(e.shape), axis=0), axis=0)
    (q, _) = verify(e, np.zeros_like(e), group)
    assert np.unique(bits(q)).size >= 4 and (q >= 1.0).all() and (q < 1.0 + 2.0 ** -35).all()


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_keys_that_differ_in_the_highest_digits(group):
    """2^e over the whole exponent range, subnormals included"""
    e = 2.0 ** np.arange(-1074, 1024, dtype=np.float64)
    assert e[0] == 5e-324 and np.isfinite(e[-1]) and np.unique(e).size == 2098
    rng = np.random.default_rng(7)
    p = np.stack([rng.permutation(e) for _ in range(3)], axis=1).reshape(2098, 1, 1, 3)
    sign = np.where(rng.random(p.shape) < 0.5, -1.0, 1.0)
    (q, _) = verify(p * sign, np.zeros_like(p), group)
    assert (np.frexp(q)[0] == 0.5).all()      # powers of two


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_equal_operands_and_zeros_of_both_signs(group):
    rng = np.random.default_rng(8)
    p = np.where(rng.random((30, 1, 2, 65)) < 0.5, -0.0, 0.0)
    a = np.where(rng.random((30, 1, 2, 65)) < 0.5, -0.0, 0.0)
    (q, _) = verify(p, a, group)
    assert (bits(q) == 0).all()             # +0.0, never -0.0
    v = rng.standard_normal((30, 1, 2, 65))
    (q, _) = verify(v, v.copy(), group)
    assert (bits(q) == 0).all()


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_scores_that_overflow(group):
    """+-1e308 pairs: |p - a| = +inf is a valid score above every finite one"""
    rng = np.random.default_rng(9)
    (p, a) = noise(rng, 40, 2, 65, gaps=0.0, dtype=np.float64)
    big = rng.random(p.shape) < 0.15
    p[big] = 1e308
    a[big] = -1e308
    p[:, :, 1, :8] = -1e308
    a[:, :, 1, :8] = 1e308                  # pixels whose every score is +inf
    (q, n) = verify(p, a, group)
    assert (n == (40 if group == "pixel" else 40 * 130)).all() and np.isinf(q).any()
    (le, _) = score_counts(p, a, np.full_like(q, np.inf), group)
    assert (le == n).all()                  # a score of +inf is <= +inf


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_gaps(group):
    """NaN and +-inf sprinkled, a whole pixel, a whole case; pixels with n exactly at and below the first finite rank"""
    rng = np.random.default_rng(10)
    (p, a) = noise(rng, 20, 3, 65, gaps=0.0, dtype=np.float64)
    for (arr, value) in ((p, np.nan), (a, np.inf), (p, -np.inf), (a, np.nan)):
        arr[rng.random(arr.shape) < 0.02] = value
    a[:, :, 2, 7] = np.nan                  # a pixel without a pair
    p[5] = np.inf                           # a case without a pair
    # four pixels made whole again but for the case that is out: n = 19 is the threshold of 19/20, 18 is below it; 9 and 8 of 9/10
    for (x, out) in ((0, 0), (1, 1), (2, 11), (3, 12)):     # the first `out` cases are out as well (case 5 is among 11 and 12)
        p[:, 0, 0, x] = rng.random(20)
        a[:, 0, 0, x] = rng.random(20)
        p[5, 0, 0, x] = np.inf
        a[:out, 0, 0, x] = np.nan
    (q, n) = verify(p, a, group, twice=True)
    if group == "pixel":
        assert list(n[0, :4]) == [19, 18, 9, 8] and n[2, 7] == 0 and n.max() == 19
        fin = np.isfinite(q[:, 0, :4])
        assert fin.tolist() == [[True] * 4, [True] * 4, [True, True, True, False], [True, False, False, False]]


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_scale_operand(group):
    rng = np.random.default_rng(12)
    (p, a) = noise(rng, 40, 3, 65, dtype=np.float64)
    s = 0.05 + rng.random(p.shape)
    for value in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
        s[rng.random(s.shape) < 0.02] = value
    s[:, :, 1, 3] = 0.0                     # a pixel the scale takes out
    s[3, 0, 0, 0] = 5e-324                  # a score that overflows by the division
    (q, n) = verify(p, a, group, s=s, twice=True)
    (_, n_plain) = conformal_ref.quantiles(p, a, LEVELS, group)
    assert (n <= n_plain).all() and (n < n_plain).any()
    if group == "pixel":
        assert n[1, 3] == 0


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_second_channel_is_not_read(group):
    rng = np.random.default_rng(13)
    p = rng.random((25, 2, 3, 65))
    a = rng.random((25, 3, 3, 65)).astype(np.float32)
    s = 0.5 + rng.random((25, 2, 3, 65))
    p[:, 1] = np.nan
    a[:, 1:] = np.nan
    s[:, 1] = np.nan
    (q, n) = verify(p, a, group, s=s)
    assert (n == (25 if group == "pixel" else 25 * 195)).all()


@pytest.mark.parametrize("group", ["pixel", "pooled"])
@pytest.mark.parametrize("ks", [None, "f32", "f32be", "f64", "f64be"])
@pytest.mark.parametrize("ka", list(DTYPES))
@pytest.mark.parametrize("kp", list(DTYPES))
def test_element_kinds(kp, ka, ks, group):
    rng = np.random.default_rng(14)
    (p, a) = noise(rng, 24, 2, 67, dtype=np.float64)
    s = 0.25 + rng.random(p.shape)
    s[rng.random(s.shape) < 0.03] = -1.0
    (p, a) = (np.ascontiguousarray(p.astype(DTYPES[kp])), np.ascontiguousarray(a.astype(DTYPES[ka])))
    s = np.ascontiguousarray(s.astype(DTYPES[ks])) if ks is not None else None
    ops = [device_operand(x) if x is not None else None for x in (p, a, s)]
    assert [o.kind for o in ops if o is not None] == [KINDS[k] for k in (kp, ka, ks) if k is not None]
    verify(p, a, group, s=s, operands=ops)


def strided(arr, lead, gap):
    """the cases of arr (N, 1, H, W) laid out `gap` elements apart after `lead` elements: a device operand whose case
    starts are aligned to the element and to nothing more"""
    (n, plane) = (arr.shape[0], int(np.prod(arr.shape[1:])))
    native = arr.dtype.newbyteorder("=")
    stride = plane + gap
    buf = np.full(lead + n * stride, np.nan, dtype=native)
    for i in range(n):
        buf[lead + i * stride:lead + i * stride + plane] = arr[i].reshape(-1)
    t = torch.from_numpy(buf).cuda()
    kind = _lib.ELEM_F32 if native.itemsize == 4 else _lib.ELEM_F64
    return DeviceOperand(t[lead:], kind, tuple(arr.shape), stride)


@pytest.mark.parametrize("group", ["pixel", "pooled"])
def test_unaligned_case_starts(group):
    rng = np.random.default_rng(15)
    (p, a) = noise(rng, 21, 1, 131)
    s = (0.5 + rng.random(p.shape))
    ops = [strided(p, 1, 3), strided(a, 3, 1), strided(s, 1, 2)]
    (q, n) = verify(p, a, group, s=s, operands=ops, twice=True)
    bounds_q = q[2] if group == "pixel" else q[2]
    (lo, hi) = interval_bounds(ops[0], bounds_q, group, scale=ops[2])
    (want_lo, want_hi) = conformal_ref.bounds(p, bounds_q, s)
    assert np.array_equal(bits(lo.cpu().numpy()), bits(want_lo)) and np.array_equal(bits(hi.cpu().numpy()), bits(want_hi))


# ---- the bounds -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", ["pixel", "pooled"])
@pytest.mark.parametrize("ks", [None, "f32", "f64be"])
@pytest.mark.parametrize("kp", list(DTYPES))
def test_interval_bounds(kp, ks, group):
    rng = np.random.default_rng(16)
    (n, h, w) = (7, 5, 67)
    p = (280.0 + 20.0 * rng.random((n, 2, h, w)))
    p[:, 1] = np.nan
    for value in (np.nan, np.inf, -np.inf):
        p[:, 0][rng.random((n, h, w)) < 0.03] = value
    p = np.ascontiguousarray(p.astype(DTYPES[kp]))
    s = None
    if ks is not None:
        s = 0.1 + rng.random((n, 1, h, w)) / 3.0
        for value in (0.0, -0.0, -2.0, np.nan, np.inf):
            s[rng.random(s.shape) < 0.03] = value
        s = np.ascontiguousarray(s.astype(DTYPES[ks]))
    q = rng.random((h, w)) / 7.0 if group == "pixel" else np.float64(1.0 / 3.0)
    if group == "pixel":
        q[rng.random(q.shape) < 0.1] = np.inf
        q[0, 0] = 0.0
    for each in ([q] if group == "pixel" else [q, np.float64(np.inf), np.float64(0.0)]):
        (lo, hi) = interval_bounds(p, each, group, scale=s)
        assert lo.is_cuda and lo.dtype == torch.float64 and tuple(lo.shape) == (n, h, w) == tuple(hi.shape)
        (want_lo, want_hi) = conformal_ref.bounds(p, each, s)
        (lo, hi) = (lo.cpu().numpy(), hi.cpu().numpy())
        # bit for bit but for the payload of a NaN: where one is NaN the other is
        for (got, want) in ((lo, want_lo), (hi, want_hi)):
            assert np.array_equal(np.isnan(got), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.array_equal(bits(got)[ok], bits(want)[ok])
        assert np.isnan(want_lo).any() and not np.isnan(want_lo).all()
        if np.isinf(each).any():
            assert (lo[~np.isnan(lo) & np.broadcast_to(np.isinf(each), lo.shape)] == -np.inf).all()


def test_bounds_round_product_and_sum_separately():
    """operands for which a fused multiply-add gives another answer than two rounded operations"""
    rng = np.random.default_rng(18)
    p = rng.random((64, 1, 8, 64))
    s = 1.0 + rng.random(p.shape)
    q = np.float64(1.0 / 3.0)
    (lo, hi) = interval_bounds(p, q, "pooled", scale=s)
    (want_lo, want_hi) = conformal_ref.bounds(p, q, s)
    fused = np.array([float(np.longdouble(x) + np.longdouble(q) * np.longdouble(y)) for (x, y) in zip(p.reshape(-1)[:4096], s.reshape(-1)[:4096])])
    assert (fused != want_hi.reshape(-1)[:4096]).any()      # the data can tell the two apart
    assert np.array_equal(bits(lo.cpu().numpy()), bits(want_lo)) and np.array_equal(bits(hi.cpu().numpy()), bits(want_hi))


# ---- the C entry points: outputs written whole, empty calls, refusals ---------------------------------------------------

def _levels_c(levels):
    import ctypes as C
    levels = [Fraction(v) for v in levels]
    return (C.c_int64 * len(levels))(*[v.numerator for v in levels]), (C.c_int64 * len(levels))(*[v.denominator for v in levels])


def raw_quantiles(p, a, s, n, plane, group, levels, q, cnt, ws=None, ws_bytes=None, num_den=None):
    """cae_score_quantiles as the header declares it; returns the code"""
    lib = _lib.load()
    (num, den) = num_den if num_den is not None else _levels_c(levels)
    need = int(lib.cae_score_quantiles_workspace_bytes(n, plane, group, len(levels)))
    if ws is None:
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
    with _stream(torch.device("cuda", torch.cuda.current_device())) as stream:
        return lib.cae_score_quantiles(*p, *a, *s, n, plane, group, num, den, len(levels), q.data_ptr() if q is not None else None,
                                       cnt.data_ptr() if cnt is not None else None, ws.data_ptr(),
                                       need if ws_bytes is None else ws_bytes, stream)


@pytest.mark.parametrize("group", [0, 1])
def test_outputs_are_written_whole_and_nothing_else(group):
    rng = np.random.default_rng(19)
    (p, a) = noise(rng, 30, 2, 67)
    (dp, da) = (device_operand(p), device_operand(a))
    groups = 1 if group else 134
    q = torch.full((len(LEVELS) * groups + 3,), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((groups + 3,), -7, dtype=torch.int64, device="cuda")
    assert raw_quantiles(dp.args(), da.args(), (None, 0, 0), 30, 134, group, LEVELS, q, cnt) == 0
    (want_q, want_n) = conformal_ref.quantiles(p, a, LEVELS, "pooled" if group else "pixel")
    assert np.array_equal(bits(q[:-3].cpu().numpy()), bits(want_q).reshape(-1)) and (q[-3:] == -7.0).all()
    assert np.array_equal(cnt[:-3].cpu().numpy(), np.reshape(want_n, -1)) and (cnt[-3:] == -7).all()
    lib = _lib.load()
    count = torch.full((len(LEVELS) * groups + 3,), -7, dtype=torch.int64, device="cuda")
    cnt.fill_(-7)
    with _stream(torch.device("cuda", torch.cuda.current_device())) as stream:
        assert lib.cae_score_counts(*dp.args(), *da.args(), None, 0, 0, 30, 134, group, q.data_ptr(), len(LEVELS), count.data_ptr(),
                                    cnt.data_ptr(), stream) == 0
    (want_le, _) = conformal_ref.counts(p, a, want_q, "pooled" if group else "pixel")
    assert np.array_equal(count[:-3].cpu().numpy(), want_le.reshape(-1)) and (count[-3:] == -7).all()
    assert np.array_equal(cnt[:-3].cpu().numpy(), np.reshape(want_n, -1)) and (cnt[-3:] == -7).all()


def test_empty_calls():
    some = torch.zeros(16, dtype=torch.float32, device="cuda")
    op = (some.data_ptr(), _lib.ELEM_F32, 4)
    for (n, plane, group, groups) in ((0, 4, 0, 4), (0, 4, 1, 1), (3, 0, 1, 1), (0, 0, 1, 1), (3, 0, 0, 0)):
        q = torch.full((2 * max(groups, 1) + 1,), -7.0, dtype=torch.float64, device="cuda")
        cnt = torch.full((max(groups, 1) + 1,), -7, dtype=torch.int64, device="cuda")
        assert raw_quantiles(op, op, (None, 0, 0), n, plane, group, ["1/2", "9/10"], q, cnt) == 0
        assert (q[:2 * groups] == float("inf")).all() and (q[2 * groups:] == -7.0).all()
        assert (cnt[:groups] == 0).all() and (cnt[groups:] == -7).all()
    (q, n) = score_quantiles(np.zeros((0, 1, 2, 3), dtype=np.float32), np.zeros((0, 1, 2, 3)), ["0.9"], group="pixel")
    assert q.shape == (1, 2, 3) and np.isinf(q).all() and n.shape == (2, 3) and (n == 0).all()
    (q, n) = score_quantiles(np.zeros((4, 1, 0, 3), dtype=np.float32), np.zeros((4, 1, 0, 3)), ["0.9"], group="pooled")
    assert q.shape == (1,) and np.isinf(q).all() and n == 0
    (le, n) = score_counts(np.zeros((0, 1, 2, 3)), np.zeros((0, 1, 2, 3)), np.ones((2, 2, 3)), "pixel")
    assert le.shape == (2, 2, 3) and (le == 0).all() and (n == 0).all()
    (lo, hi) = interval_bounds(np.zeros((0, 1, 2, 3)), np.ones((2, 3)), "pixel")
    assert tuple(lo.shape) == (0, 2, 3) == tuple(hi.shape)


def test_refused_calls():
    import ctypes as C
    lib = _lib.load()
    x = torch.rand(4 * 16 + 1, dtype=torch.float32, device="cuda")
    op = (x.data_ptr(), _lib.ELEM_F32, 16)
    none = (None, 0, 0)
    q = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    odd = torch.empty(64, dtype=torch.uint8, device="cuda")

    def refused(rc):
        assert rc == -1 and lib.cae_last_error()        # CAE_ERR_ARG
        assert (q == -7.0).all() and (cnt == -7).all()  # nothing written

    levels = ["1/2", "9/10"]
    refused(raw_quantiles((x.data_ptr(), 9, 16), op, none, 4, 4, 0, levels, q, cnt))               # a bad kind
    refused(raw_quantiles(op, (x.data_ptr(), -1, 16), none, 4, 4, 0, levels, q, cnt))
    refused(raw_quantiles(op, op, (x.data_ptr(), 4, 16), 4, 4, 0, levels, q, cnt))
    refused(raw_quantiles(op, op, none, -1, 4, 0, levels, q, cnt))                                 # negative sizes
    refused(raw_quantiles(op, op, none, 4, -4, 0, levels, q, cnt))
    refused(raw_quantiles(op, op, none, 4, 4, 2, levels, q, cnt))                                  # no such group
    refused(raw_quantiles((x.data_ptr(), 0, -16), op, none, 4, 4, 0, levels, q, cnt))              # a negative stride
    refused(raw_quantiles((x.data_ptr(), 0, 3), op, none, 4, 4, 0, levels, q, cnt))                # shorter than the plane
    refused(raw_quantiles(op, op, (x.data_ptr(), 0, 3), 4, 4, 0, levels, q, cnt))
    refused(raw_quantiles((None, 0, 16), op, none, 4, 4, 0, levels, q, cnt))                       # NULL
    refused(raw_quantiles(op, (None, 0, 16), none, 4, 4, 0, levels, q, cnt))
    refused(raw_quantiles(op, op, none, 4, 4, 0, levels, None, cnt))
    refused(raw_quantiles(op, op, none, 4, 4, 0, levels, q, None))
    refused(raw_quantiles((x.data_ptr() + 2, 0, 16), op, none, 4, 4, 0, levels, q, cnt))           # misaligned
    refused(raw_quantiles((x.data_ptr() + 4, _lib.ELEM_F64, 8), op, none, 4, 4, 0, levels, q, cnt))
    refused(raw_quantiles(op, op, none, 1 << 31, 4, 0, levels, q, cnt))                            # too many cases
    for bad in ((0, 2), (2, 2), (3, 2), (-1, 2), (1, 1000001), (1, 0)):                             # a level outside the rule
        pair = ((C.c_int64 * 2)(1, bad[0]), (C.c_int64 * 2)(4, bad[1]))
        refused(raw_quantiles(op, op, none, 4, 4, 0, levels, q, cnt, num_den=pair))
    for pair in (((9, 1), (10, 2)), ((1, 2), (2, 4))):                                             # descending, repeated
        refused(raw_quantiles(op, op, none, 4, 4, 1, levels, q, cnt, num_den=((C.c_int64 * 2)(*pair[0]), (C.c_int64 * 2)(*pair[1]))))
    refused(raw_quantiles(op, op, none, 4, 4, 1, [], q, cnt))                                      # no level
    refused(raw_quantiles(op, op, none, 4, 4, 1, ["1/10"] * 9, q, cnt, num_den=_levels_c([Fraction(i, 10) for i in range(1, 10)])))
    refused(raw_quantiles(op, op, none, 4, 4, 1, levels, q, cnt, ws_bytes=16632))                  # too small a workspace
    refused(raw_quantiles(op, op, none, 4, 4, 1, levels, q, cnt, ws=odd[4:]))                      # a misaligned one
    assert lib.cae_score_quantiles_workspace_bytes(4, 4, 1, 2) == 16640 and lib.cae_score_quantiles_workspace_bytes(4, 4, 0, 2) == 0
    with _stream(torch.device("cuda", torch.cuda.current_device())) as stream:
        refused(lib.cae_score_counts(*op, *op, None, 0, 0, 4, 4, 3, q.data_ptr(), 2, cnt.data_ptr(), cnt.data_ptr(), stream))
        refused(lib.cae_score_counts(*op, *op, None, 0, 0, 4, 4, 0, None, 2, cnt.data_ptr(), cnt.data_ptr(), stream))
        refused(lib.cae_score_counts(*op, *op, None, 0, 0, 4, 4, 0, q.data_ptr(), 9, cnt.data_ptr(), cnt.data_ptr(), stream))
        refused(lib.cae_score_counts(x.data_ptr(), 0, 3, *op, None, 0, 0, 4, 4, 0, q.data_ptr(), 2, cnt.data_ptr(), cnt.data_ptr(), stream))
        refused(lib.cae_interval_bounds(*op, None, 0, 0, 4, 4, cnt.data_ptr(), 2, q.data_ptr(), q.data_ptr(), stream))
        refused(lib.cae_interval_bounds(x.data_ptr(), 7, 16, None, 0, 0, 4, 4, cnt.data_ptr(), 0, q.data_ptr(), q.data_ptr(), stream))
        refused(lib.cae_interval_bounds(*op, None, 0, 0, 4, 4, None, 0, q.data_ptr(), q.data_ptr(), stream))
        refused(lib.cae_interval_bounds(*op, None, 0, 0, 4, 4, cnt.data_ptr(), 0, None, q.data_ptr(), stream))
        refused(lib.cae_interval_bounds(x.data_ptr(), 0, 3, None, 0, 0, 4, 4, cnt.data_ptr(), 0, q.data_ptr(), q.data_ptr(), stream))
    torch.cuda.synchronize()
    # the Python functions refuse what they can see
    for bad in (["0.9", "0.8"], [0.9], ["1"], []):
        with pytest.raises(ValueError):
            score_quantiles(np.zeros((2, 1, 2, 2)), np.zeros((2, 1, 2, 2)), bad)
    with pytest.raises(ValueError):
        score_quantiles(np.zeros((2, 1, 2, 2)), np.zeros((2, 1, 2, 2)), ["0.9"], group="case")
    with pytest.raises(ValueError):
        score_quantiles(np.zeros((2, 1, 2, 2)), np.zeros((3, 1, 2, 2)), ["0.9"])
    with pytest.raises(ValueError):
        score_quantiles(np.zeros((2, 1, 2, 2)), np.zeros((2, 1, 2, 2)), ["0.9"], scale=np.ones((2, 1, 2, 3)))
    with pytest.raises(ValueError):
        score_counts(np.zeros((2, 1, 2, 2)), np.zeros((2, 1, 2, 2)), np.ones((1, 2, 3)), "pixel")
    with pytest.raises(ValueError):
        interval_bounds(np.zeros((2, 1, 2, 2)), np.ones((2, 2)), "pooled")


# ---- train_cae -> calibrate -> apply_cae --interval -------------------------------------------------------------------

@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """datagen circle data: 12 training cases, 20 calibration cases (19/20 is finite from 19 on), 12 test cases; a small conv
    model and a linear one, a few epochs each"""
    from cae_tools_amd.cli import train_cae
    from cae_tools_amd.data import datagen
    root = tmp_path_factory.mktemp("conformal")
    paths = {}
    for (part, n, seed) in (("train", 12, 1234), ("calib", 20, 99), ("test", 12, 4321)):
        paths[part] = str(root / f"{part}.nc")
        datagen.generate("circle", n, seed=seed).to_netcdf(paths[part])
    models = {}
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        for (method, extra) in (("conv", ["--latent-size", "4", "--fc-size", "16"]), ("linear", [])):
            models[method] = str(root / f"model_{method}")
            train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", models[method],
                            "--input-variables", "lowres", "--output-variable", "hires", "--method", method, "--nr-epochs", "3",
                            "--batch-size", "6", *extra])
    return root, paths, models


def _folder_bytes(folder, but=()):
    out = {}
    for name in sorted(os.listdir(folder)):
        if name not in but:
            with open(os.path.join(folder, name), "rb") as f:
                out[name] = f.read()
    return out


@pytest.mark.parametrize("method", ["conv", "linear"])
def test_train_calibrate_apply(world, method):
    from cae_tools_amd.cli import apply_cae, calibrate
    from cae_tools_amd.data.arrays import open_dataset
    (root, paths, models) = world
    folder = models[method]
    plain = str(root / f"plain_{method}.nc")
    with redirect_stdout(io.StringIO()):
        apply_cae.main([paths["test"], plain, "--model-folder", folder])
        for part in ("calib", "test"):      # the scores a user could recompute: the predictions apply_cae stores
            apply_cae.main([paths[part], str(root / f"scored_{part}_{method}.nc"), "--model-folder", folder])
    before = _folder_bytes(folder)
    assert "calibration.json" not in before
    with open(plain, "rb") as f:
        plain_bytes = f.read()
    scored = {part: open_dataset(str(root / f"scored_{part}_{method}.nc")) for part in ("calib", "test")}
    (cal_p, cal_a) = (np.asarray(scored["calib"]["model_output"].values), np.asarray(scored["calib"]["hires"].values))
    (test_p, test_a) = (np.asarray(scored["test"]["model_output"].values), np.asarray(scored["test"]["hires"].values))
    assert cal_p.dtype == np.float64 and cal_p.shape == (20, 1, 256, 256)
    levels = ["4/5", "9/10", "19/20"]
    for group in ("pixel", "pooled"):
        log = io.StringIO()
        with redirect_stdout(log):
            calibrate.main(["--calibration-inputs", paths["calib"], "--model-folder", folder, "--output-variable", "hires",
                            "--group", group, "--test-inputs", paths["test"]])
        lines = [line for line in log.getvalue().splitlines() if line.startswith("calibrate ")]
        assert len(lines) == 3
        # nothing else in the folder changes
        written = {"calibration.json", "calibration.nc"} if group == "pixel" else {"calibration.json"}
        assert _folder_bytes(folder, but=("calibration.json", "calibration.nc")) == before
        assert set(os.listdir(folder)) - set(before) == written
        record = conformal.read_record(folder)
        (want_q, want_n) = conformal_ref.quantiles(cal_p, cal_a, levels, group)
        (want_pooled, _) = conformal_ref.quantiles(cal_p, cal_a, levels, "pooled")
        assert np.isfinite(want_q).all() and (np.asarray(want_n) == (20 if group == "pixel" else 20 * 65536)).all()
        assert record["levels"] == [Fraction(v) for v in levels] and record["group"] == group and record["cases"] == 20
        assert (record["output_variable"], record["scale_variable"]) == ("hires", None)
        assert np.array_equal(bits(record["pooled_quantiles"]), bits(want_pooled))
        if group == "pixel":
            assert np.array_equal(bits(record["quantile"]), bits(want_q)) and np.array_equal(record["count"], want_n)
            assert (record["n_min"], record["n_median"], record["n_max"]) == (20, 20.0, 20)
        # the printed held-out coverage is the numpy count
        (le, n) = conformal_ref.counts(test_p, test_a, want_q, group)
        covered = [int(np.sum(c)) for c in le]
        assert record["test_covered"] == covered and record["test_pairs"] == int(np.sum(n)) == 12 * 65536
        for (i, line) in enumerate(lines):
            assert line.startswith(f"calibrate {levels[i]} {group}: ") and f"held-out coverage {covered[i]}/{12 * 65536} = " in line
            print(f"{method} {line}")       # reported, not bounded: a tiny model on a tiny set
        # apply_cae --interval 0.9: the bounds in the file are prediction -+ q recomputed from the same file
        out = str(root / f"interval_{method}_{group}.nc")
        names = ["lo", "hi"] if group == "pooled" else ["model_output_lower", "model_output_upper"]
        with redirect_stdout(io.StringIO()):
            apply_cae.main([paths["test"], out, "--model-folder", folder, "--interval", "0.9"]
                           + (["--interval-variables", "lo", "hi"] if group == "pooled" else []))
        ds = open_dataset(out)
        pred = np.asarray(ds["model_output"].values)
        assert np.array_equal(bits(pred), bits(test_p))
        q = want_q[1]
        (want_lo, want_hi) = conformal_ref.bounds(pred, q)
        (lo, hi) = (np.asarray(ds[names[0]].values), np.asarray(ds[names[1]].values))
        assert lo.dtype.newbyteorder("=") == np.float64 and lo.shape == (12, 256, 256) and tuple(ds[names[0]].dims) == ("n", "model_output_y", "model_output_x")
        assert np.array_equal(bits(lo), bits(want_lo)) and np.array_equal(bits(hi), bits(want_hi))
        assert np.isfinite(lo).all() and (hi >= lo).all()
        # an uncalibrated level is refused
        with pytest.raises(SystemExit):
            apply_cae.main([paths["test"], out, "--model-folder", folder, "--interval", "0.85"])
        # without --interval the bytes are those written before the calibration
        again = str(root / f"again_{method}_{group}.nc")
        with redirect_stdout(io.StringIO()):
            apply_cae.main([paths["test"], again, "--model-folder", folder])
        with open(again, "rb") as f:
            assert f.read() == plain_bytes


def _square(path_in, path_out):
    """input and target at 64 x 64 on both sides (a UNET's decoder mirrors its encoder): the 16 x 16 input repeated 4 x 4, the
    256 x 256 target averaged over 4 x 4 blocks"""
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import open_dataset
    ds = open_dataset(path_in)
    lo = np.asarray(ds["lowres"].values)
    n = lo.shape[0]
    hi = np.asarray(ds["hires"].values).astype(np.float64)
    variables = {"lowres": (("n", "chan", "y", "x"), np.repeat(np.repeat(lo, 4, axis=2), 4, axis=3).astype(np.float32), {}),
                 "hires": (("n", "chan", "y", "x"), hi.reshape(n, 1, 64, 4, 64, 4).mean(axis=(3, 5)).astype(np.float32), {}),
                 "valid": (("n", "chan", "y", "x"), np.ones((n, 1, 64, 64), dtype=np.float32), {})}
    netcdf3.write(path_out, {"n": n, "chan": 1, "y": 64, "x": 64}, variables)


@pytest.mark.parametrize("method", ["unet", "var"])
def test_the_commands_for_the_other_model_classes(world, method):
    """calibrate and apply_cae --interval on a unet and a var model folder: the stored bounds are prediction -+ q of the record"""
    from cae_tools_amd.cli import apply_cae, calibrate, train_cae
    from cae_tools_amd.data.arrays import open_dataset
    (root, paths, _) = world
    extra = ["--latent-size", "4", "--fc-size", "16"]
    if method == "unet":
        from cae_tools_amd.models.unet import unet_layer_spec
        square = {part: str(root / f"square_{part}.nc") for part in paths}
        for part in paths:
            _square(paths[part], square[part])
        paths = square
        layers = str(root / "unet_layers.json")
        with open(layers, "w") as f:
            json.dump(unet_layer_spec(1, 1, (64, 64), [8, 16]).save(), f)
        extra = ["--layer-definitions-path", layers, "--mask-variable", "valid"]
    folder = str(root / f"model_{method}")
    out = str(root / f"interval_{method}.nc")
    torch.manual_seed(0)
    log = io.StringIO()
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", folder,
                        "--input-variables", "lowres", "--output-variable", "hires", "--method", method, "--nr-epochs", "2",
                        "--batch-size", "6"] + extra)
    with redirect_stdout(log):
        calibrate.main(["--calibration-inputs", paths["calib"], "--model-folder", folder, "--output-variable", "hires",
                        "--coverage", "0.5", "0.9", "--group", "pixel", "--test-inputs", paths["test"]])
    with redirect_stdout(io.StringIO()):
        apply_cae.main([paths["test"], out, "--model-folder", folder, "--interval", "0.9"]
                       + (["--latent-variable", "z"] if method == "var" else []))
        for part in ("calib", "test"):
            apply_cae.main([paths[part], str(root / f"scored_{part}_{method}.nc"), "--model-folder", folder])
    assert len([line for line in log.getvalue().splitlines() if line.startswith("calibrate ")]) == 2
    record = conformal.read_record(folder)
    scored = open_dataset(str(root / f"scored_calib_{method}.nc"))
    (want_q, want_n) = conformal_ref.quantiles(np.asarray(scored["model_output"].values), np.asarray(scored["hires"].values),
                                               ["1/2", "9/10"], "pixel")
    assert np.isfinite(want_q).all() and (want_n == 20).all()
    assert np.array_equal(bits(record["quantile"]), bits(want_q)) and np.array_equal(record["count"], want_n)
    ds = open_dataset(out)
    pred = np.asarray(ds["model_output"].values)
    (want_lo, want_hi) = conformal_ref.bounds(pred, want_q[1])
    assert np.array_equal(bits(np.asarray(ds["model_output_lower"].values)), bits(want_lo))
    assert np.array_equal(bits(np.asarray(ds["model_output_upper"].values)), bits(want_hi))
    plain = open_dataset(str(root / f"scored_test_{method}.nc"))
    (le, n) = conformal_ref.counts(np.asarray(plain["model_output"].values), np.asarray(plain["hires"].values), want_q, "pixel")
    assert record["test_covered"] == [int(c.sum()) for c in le] and record["test_pairs"] == int(n.sum())
    if method == "var":     # the ensemble mean is not the prediction that was calibrated
        assert "z_mu" in ds
        with pytest.raises(SystemExit):
            apply_cae.main([paths["test"], out, "--model-folder", folder, "--interval", "0.9", "--ensemble-size", "3"])


def test_calibrate_with_a_scale_variable(world):
    """the Python surface with a scale: a variable of the data set, zero in places, divides the residual and widens the bounds"""
    from cae_tools_amd.data.arrays import DataArray, open_dataset
    from cae_tools_amd.models.model_loader import load_model
    (root, paths, models) = world
    rng = np.random.default_rng(21)
    folder = str(root / "scaled")
    with redirect_stdout(io.StringIO()):
        model = load_model(models["linear"])
    ds = open_dataset(paths["calib"])
    sigma = (0.5 + rng.random((20, 1, 256, 256))).astype(np.float32)
    sigma[rng.random(sigma.shape) < 0.01] = 0.0
    ds["sigma"] = DataArray(sigma, dims=("n", "chan", "y2", "x2"))
    os.makedirs(folder)
    with redirect_stdout(io.StringIO()):
        record = model.calibrate(ds, ["lowres"], "hires", ["0.5", "0.9"], group="pooled", scale_variable="sigma", model_path=folder)
    assert "model_output" not in ds and sorted(os.listdir(folder)) == ["calibration.json"]
    with redirect_stdout(io.StringIO()):
        model.apply(ds, ["lowres"], interval="0.9", scale_variable="sigma")
    pred = np.asarray(ds["model_output"].values)
    (want_q, want_n) = conformal_ref.quantiles(pred, np.asarray(ds["hires"].values), ["1/2", "9/10"], "pooled", sigma)
    assert np.array_equal(bits(record["q"]), bits(want_q)) and record["n"] == want_n < 20 * 65536
    (want_lo, want_hi) = conformal_ref.bounds(pred, want_q[1], sigma)
    for (name, want) in (("model_output_lower", want_lo), ("model_output_upper", want_hi)):
        got = np.asarray(ds[name].values)
        assert np.array_equal(np.isnan(got), sigma[:, 0] == 0.0) and np.array_equal(bits(got)[~np.isnan(got)], bits(want)[~np.isnan(want)])
    with pytest.raises(ValueError):
        model.apply(ds, ["lowres"], interval="0.9")             # the calibrated scale is missing
    with pytest.raises(ValueError):
        model.apply(ds, ["lowres"], interval="0.8", scale_variable="sigma")
    with open(os.path.join(folder, "calibration.json")) as f:
        assert json.load(f)["scale_variable"] == "sigma"
