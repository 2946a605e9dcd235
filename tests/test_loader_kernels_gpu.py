"""The loader kernels of kernels_stateless.h (k_scan, k_normalise_pack, k_invert_perm, k_denorm_f64, k_metric_sums,
k_bswap32) with their host code (host_loader.h) and wrappers (device_ops.py) against loader_ref.py, at the sizes where each
takes another path: one lane, one wave, one workgroup and one element more, the grid caps with their second grid-stride
trip, the host fold over per-block partials, the wrapper's split of more than 65 535 instances.  Everything but the metric
sums is compared bit for bit; the metric sums are held to 2 N u S|term| against math.fsum (loader_ref's docstring), the
count column exactly.  The inputs are those test_loader_ref_cpu.py holds to telling the promised arithmetic (two rounded
fp32 operations; two rounded fp64 operations) from a quotient rounded once, a reciprocal and a contracted fma.

Largest |got - fsum| / bound per column measured on an MI355X (every check prints its running maxima before it asserts):
S a' 2.8e-3, S e' 5.2e-3, S a'^2 0.14, S e'^2 7.3e-3, S a'e' 0.25, S|a-e| 7.1e-3, S(a-e)^2 4.8e-3; the two large ones at the
4-pixel instances, 7.3e-3 at the most elsewhere.  Which test fails under which wrong arithmetic: DESIGN.md section 2, "The loader and metric-sum kernels against numpy, past one workgroup"."""
import numpy as np
import pytest
import torch

import loader_ref as ref
from cae_tools_amd import _lib
from cae_tools_amd.device_ops import (denormalise_f64, inverse_permutation, metric_sums, normalise_pack, scan_f32,
                                      upload_f32)

pytestmark = pytest.mark.gpu

# Every kernel walks its elements with the stride gridDim.x * 256; the host sizes the grid for 16, 8, 16 and 1 trips of a
# lane (elements, or 4-word groups for the swap) and caps it, so one element past a cap is one more trip of block 0, lane 0.
SCAN_CAP = 1024 * 4096          # k_scan: at most 1024 blocks, sized for 16 trips
PACK_CAP = 8192 * 2048          # k_normalise_pack, k_denorm_f64: at most 8192 blocks, sized for 8 trips
METRIC_CAP = 64 * 4096          # k_metric_sums: at most 64 chunks per instance, sized for 16 trips
BSWAP_CAP = 4096 * 256 * 4      # k_bswap32: at most 4096 blocks, one 4-word group per lane and trip


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- cae_scan_f32 -----------------------------------------------------------------------------------

def _scan_both(x):
    got = scan_f32(_cuda(x))
    want = ref.scan(x)
    assert got == want, (x.size, got, want)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, SCAN_CAP + 1])
def test_scan_against_numpy(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    _scan_both(x)
    _scan_both(ref.wide_variable(n, seed=n))
    # NaNs at both ends and on both sides of a block boundary: counted, and ignored by the extremes
    holes = sorted({i for i in (0, n - 1, 4095, 4096) if i < n})
    if len(holes) < n:
        y = x.copy()
        y[holes] = np.nan
        (count, lo, hi) = scan_f32(_cuda(y))
        assert count == len(holes) and (count, lo, hi) == ref.scan(y)
        # an extreme next to a NaN
        keep = [i for i in range(min(n, 4100)) if i not in holes]
        y[keep[0]] = 50.0
        y[keep[-1]] = -50.0
        _scan_both(y)
    # infinities are values
    z = x.copy()
    z[0] = np.inf
    z[-1] = -np.inf
    (count, lo, hi) = scan_f32(_cuda(z))
    assert count == 0 and hi == (np.inf if n > 1 else -np.inf) and lo == -np.inf
    assert (count, lo, hi) == ref.scan(z)
    # all NaN: the count alone is defined
    assert scan_f32(_cuda(np.full(n, np.nan, dtype=np.float32)))[0] == n


@pytest.mark.parametrize("n", [4097, SCAN_CAP + 1])
def test_scan_extremes_in_the_first_and_last_element(n):
    """the last element is one more trip of block 0, lane 0: the 9th at 4097 elements over two blocks, and at the capped
    size the 17th, one beyond those the grid was sized for.  Its value has to survive the lane, wave, block and host folds"""
    x = np.random.default_rng(n + 1).standard_normal(n).astype(np.float32)
    for (first, last) in ((99.5, -77.25), (-77.25, 99.5)):
        x[0] = first
        x[-1] = last
        got = scan_f32(_cuda(x))
        assert got == (0, -77.25, 99.5) and got == ref.scan(x)


# ---- cae_normalise_pack, cae_normalise_pack_rows ---------------------------------------------------------

N_ROWS = 37
ORDER = np.random.default_rng(37).permutation(N_ROWS)


def _pack_both(src, c_dst, c_off, vmin, vmax, enable, order):
    """(kernel's dst, loader_ref's dst) over a dst filled with -7, as uint32"""
    n = src.shape[0]
    fill = np.full((n, c_dst) + src.shape[2:], -7.0, dtype=np.float32)
    dst = _cuda(fill)
    rows = None if order is None else inverse_permutation(order, _dev())
    normalise_pack(_cuda(src), dst, c_off, vmin, vmax, enable=enable, dst_rows=rows)
    torch.cuda.synchronize()
    want = ref.pack(fill, ref.normalise(src, vmin, vmax, enable), c_off, None if order is None else np.argsort(order))
    return _u32(dst.cpu().numpy()), _u32(want)


@pytest.mark.parametrize("variable", ["wide", "narrow"])
@pytest.mark.parametrize("c_src", [1, 3])
@pytest.mark.parametrize("hw", [1, 3, 255, 1025])
def test_normalise_pack_against_numpy(hw, c_src, variable):
    make = ref.wide_variable if variable == "wide" else ref.narrow_variable
    src = make(N_ROWS * c_src * hw, seed=1000 * hw + c_src).reshape(N_ROWS, c_src, hw)
    (lo, hi) = ref.bounds_of(src)
    for c_off in (0, 1, 2):
        for order in (None, ORDER):
            for (vmin, vmax, enable) in ((lo, hi, True), (lo, hi, False), (lo, lo, True)):
                (got, want) = _pack_both(src, c_src + 2, c_off, vmin, vmax, enable, order)
                assert got.tobytes() == want.tobytes(), (c_off, order is not None, vmin, vmax, enable)
    # what the comparison rests on: a dst that still holds -7 outside the variable's channels, zeros at range 0
    (got, _) = _pack_both(src, c_src + 2, 1, lo, lo, True, ORDER)
    got = got.view(np.float32)
    assert (got[:, 0] == -7.0).all() and (got[:, -1] == -7.0).all() and not got[:, 1:-1].any()


def test_normalise_pack_passes_non_finite_values_as_numpy_does():
    src = ref.narrow_variable(N_ROWS * 2 * 257, seed=5).reshape(N_ROWS, 2, 257)
    (lo, hi) = ref.bounds_of(src)
    src[0, 0, 0] = src[5, 1, 256] = src[36, 1, 100] = np.nan
    src[1, 0, 1] = src[36, 1, 256] = np.inf
    src[2, 1, 2] = src[17, 0, 255] = -np.inf
    for order in (None, ORDER):
        for enable in (True, False):
            (got, want) = _pack_both(src, 3, 1, lo, hi, enable, order)
            assert np.array_equal(got, want), (order is not None, enable)
    (got, _) = _pack_both(src, 2, 0, lo, hi, True, None)
    got = got.view(np.float32)
    assert np.isnan(got[0, 0, 0]) and got[1, 0, 1] == np.inf and got[2, 1, 2] == -np.inf
    # a range of 0 gives 0 for every element, the non-finite ones included
    (got, want) = _pack_both(src, 2, 0, lo, lo, True, None)
    assert np.array_equal(got, want) and not got.any()


@pytest.mark.parametrize("shape", [(4100, 1, 64, 64), (70001, 1, 1, 1)])
def test_normalise_pack_above_the_grid_cap_and_over_many_rows(shape):
    """4100 x 64 x 64 elements are more than the 8192 x 2048 one sweep of the capped grid covers; 70 001 rows of one element
    walk a long row table"""
    count = int(np.prod(shape))
    assert shape[0] > 65535 or count > PACK_CAP
    src = ref.wide_variable(count, seed=shape[0]).reshape(shape)
    (lo, hi) = ref.bounds_of(src)
    order = np.random.default_rng(shape[0]).permutation(shape[0])
    (got, want) = _pack_both(src, 2, 1, lo, hi, True, order)
    assert got.tobytes() == want.tobytes()


# ---- cae_invert_permutation --------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_inverse_permutation_against_argsort(n):
    order = np.random.default_rng(n).permutation(n)
    inv = inverse_permutation(order, _dev())
    assert inv.dtype == torch.int32 and inv.shape == (n,)
    assert np.array_equal(inv.cpu().numpy(), np.argsort(order).astype(np.int32))


def test_invert_permutation_skips_entries_outside_the_table():
    """an entry of -1 and one of n name no row: k_invert_perm tests 0 <= p < n before it stores, so the rows they replaced
    keep what the output held and every other row is right"""
    n = 257
    order = np.random.default_rng(11).permutation(n).astype(np.int32)
    (lost_a, lost_b) = (int(order[3]), int(order[256]))
    order[3] = -1
    order[256] = n
    guard = 8
    out = torch.full((guard + n + guard,), -7, dtype=torch.int32, device="cuda")
    perm = _cuda(order)
    _lib.check(_lib.load().cae_invert_permutation(perm.data_ptr(), n, out.data_ptr() + 4 * guard, None))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:guard] == -7).all() and (host[-guard:] == -7).all()
    inv = host[guard:-guard]
    assert inv[lost_a] == -7 and inv[lost_b] == -7
    named = np.array([i for i in range(n) if i not in (3, 256)])
    assert np.array_equal(inv[order[named]], named)
    assert (inv == -7).sum() == 2


# ---- cae_denormalise_f64 ----------------------------------------------------------------------------

@pytest.mark.parametrize("params", [ref.FP32_VALUED, ref.ARBITRARY_F64], ids=["fp32-valued", "arbitrary-fp64"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049, PACK_CAP + 1])
def test_denormalise_against_numpy(n, params):
    (lo, hi) = params
    y = ref.unit_scores(n, seed=n)
    if n >= 255:
        # scores outside [0, 1] and the non-finite ones pass as in numpy
        y[0] = -0.25
        y[1] = 1.5
        y[2] = y[n - 1] = np.nan
        y[3] = y[n - 2] = np.inf
        y[4] = y[n - 3] = -np.inf
    got = denormalise_f64(_cuda(y), lo, hi)
    assert got.dtype == torch.float64 and got.shape == (n,)
    assert got.cpu().numpy().tobytes() == ref.denormalise(y, lo, hi).tobytes()


def test_denormalise_rounds_the_product_before_the_sum():
    """the scores on which a contracted fma would give other bits (loader_ref.fma_sensitive_scores)"""
    (lo, hi) = ref.ARBITRARY_F64
    y = ref.fma_sensitive_scores(lo, hi)
    assert y.size >= 20
    got = denormalise_f64(_cuda(y), lo, hi).cpu().numpy()
    assert got.tobytes() == ref.denormalise(y, lo, hi).tobytes()
    assert (got != ref.denormalise_fma(y, lo, hi)).all()


def test_importance_and_scene_blend_denormalise_with_the_same_two_roundings():
    """k_case_importance and k_scene_blend restate k_denorm_f64's arithmetic (cm_denorm of case_elem.h) and their own tests
    use fp32-valued parameters, under which a contracted fma cannot be seen.  Importance: cases of one pixel whose base score
    is fma-sensitive; S|e0| is then one rounded subtraction from P0, held to importance_ref's bound of five units in its last
    place where a contracted P0 is a unit in the last place of ~300 away.  Blend: an exact partition gives every pixel one
    tile of weight 1, so the output is the denormalised prediction, bit for bit."""
    import importance_ref
    from cae_tools_amd.engine import case_importance, scene_blend, scene_plan
    (lo, hi) = ref.ARBITRARY_F64
    (y, pert) = (ref.fma_sensitive_scores(lo, hi), ref.fma_sensitive_scores(lo, hi, seed=104))
    n = min(y.size, pert.size)
    assert n >= 20
    (y, pert) = (y[:n], pert[:n])
    a = ref.denormalise(ref.unit_scores(n, seed=105), lo, hi)
    shape = (n, 1, 1, 1)
    got = case_importance(_cuda(y.reshape(shape)), _cuda(pert.reshape(shape)), a.reshape(shape), lo, hi)
    want = importance_ref.Reference(y.reshape(n, 1), pert.reshape(n, 1), a.reshape(n, 1), lo, hi - lo)
    want.check(got, "arbitrary fp64 parameters")

    plan = scene_plan(12, 20, ((4, 5), (8, 15)), 0)
    pred = np.resize(y, (2 * plan.n_tile, 2, plan.H, plan.W))
    (out, holes) = scene_blend(_cuda(pred), _cuda(np.zeros(2 * plan.n_tile, dtype=np.int32)), plan, lo, hi, n_t=2)
    out = out.cpu().numpy()
    want = ref.denormalise(pred, lo, hi).reshape(2, plan.n_y, plan.n_x, 2, plan.H, plan.W).transpose(0, 3, 1, 4, 2, 5)
    assert out.tobytes() == np.ascontiguousarray(want.reshape(out.shape)).tobytes() and holes.cpu().tolist() == [0, 0]


# ---- cae_metric_sums --------------------------------------------------------------------------------

WORST = np.zeros(8)


def _hold_to_bound(got, want, mags, rows, what):
    """count exact; every other column within 2 N u S|term| of the exact sum, NaN where the exact sum is NaN"""
    for i in rows:
        assert got[i, 0] == want[i, 0], (what, i, got[i, 0], want[i, 0])
        bound = ref.metric_bound(want[i, 0], mags[i])
        for k in range(1, 8):
            if np.isnan(want[i, k]):
                assert np.isnan(got[i, k]), (what, i, ref.SUM_NAMES[k], got[i, k])
                continue
            err = abs(got[i, k] - want[i, k])
            if err > 0 and bound[k] > 0:
                WORST[k] = max(WORST[k], err / bound[k])
    print(f"{what}: worst |got - fsum| / bound so far " + ", ".join(f"{ref.SUM_NAMES[k]} {WORST[k]:.2e}" for k in range(1, 8)))
    for i in rows:
        bound = ref.metric_bound(want[i, 0], mags[i])
        for k in range(1, 8):
            if not np.isnan(want[i, k]):
                assert abs(got[i, k] - want[i, k]) <= bound[k], (what, i, ref.SUM_NAMES[k], got[i, k], want[i, k], bound[k])


def _metric_inputs(shape, params, seed):
    """scores in [0, 1) and fp32 targets over [vmin - 0.2 range, vmin + 1.2 range): a' takes both signs"""
    (lo, hi) = params
    count = int(np.prod(shape))
    y = ref.unit_scores(count, seed=seed).reshape(shape)
    a = (lo + (hi - lo) * (1.4 * np.random.default_rng(seed + 1).random(count) - 0.2)).astype(np.float32).reshape(shape)
    assert count < 100 or ((a < lo).any() and (a > lo).any())
    return y, a


def _metric_both(y, a, mask, params, what, rows=None):
    (lo, hi) = params
    got = metric_sums(_cuda(y), _cuda(a), None if mask is None else _cuda(mask), lo, hi)
    assert got.dtype == torch.float64 and got.shape == (y.shape[0], 8)
    got = got.cpu().numpy()
    (want, mags) = ref.metric_sums_exact(y, a, mask, lo, hi, rows=rows)
    _hold_to_bound(got, want, mags, range(y.shape[0]) if rows is None else rows, what)
    return got


@pytest.mark.parametrize("params", [ref.FP32_VALUED, ref.ARBITRARY_F64], ids=["fp32-valued", "arbitrary-fp64"])
@pytest.mark.parametrize("elems", [1, 255, 256, 257, 4097, METRIC_CAP + 1])
def test_metric_sums_against_fsum(elems, params):
    (y, a) = _metric_inputs((3, elems), params, seed=elems)
    rng = np.random.default_rng(elems + 2)
    masks = {"no mask": None,
             "0/1 mask": (rng.random((3, elems)) < 0.5).astype(np.float32),
             "non-binary mask": np.array([0.0, 0.5, -1.0, 2.0], dtype=np.float32)[rng.integers(0, 4, (3, elems))]}
    for (name, mask) in masks.items():
        _metric_both(y, a, mask, params, f"{elems} elements, {name}")


def test_metric_sums_see_the_two_roundings_of_e():
    """instances of one pixel whose score is one of loader_ref.fma_sensitive_scores: the bound is two units in the last
    place of each term, and e from a contracted fma is a unit in the last place of ~300 away from a difference of ~10"""
    params = ref.ARBITRARY_F64
    y = ref.fma_sensitive_scores(*params).reshape(-1, 1)
    (_, a) = _metric_inputs(y.shape, params, seed=9)
    got = _metric_both(y, a, None, params, "one sensitive pixel per instance")
    (terms, _, _) = ref.metric_terms(y, a, None, *params)
    assert got.tobytes() == np.ascontiguousarray(terms.reshape(8, -1).T).tobytes()      # one term: no rounding to allow for


def test_metric_sums_masked_instance_and_nan_under_the_mask():
    params = ref.ARBITRARY_F64
    (y, a) = _metric_inputs((3, 4097), params, seed=21)
    mask = (np.random.default_rng(22).random((3, 4097)) < 0.5).astype(np.float32)
    mask[1] = 0.0
    mask[0, 0] = mask[0, 4096] = mask[2, 255] = mask[2, 256] = 0.0
    y[0, 0] = a[0, 4096] = y[2, 255] = a[2, 256] = np.nan       # hidden by the mask
    y[1, 7] = a[1, 4000] = np.nan                                   # in the fully masked instance
    got = _metric_both(y, a, mask, params, "one instance fully masked, NaN under zeros")
    assert got[1].tobytes() == np.zeros(8).tobytes()
    assert np.isfinite(got).all()


def test_metric_sums_nan_under_a_kept_pixel_stays_in_its_instance():
    params = ref.FP32_VALUED
    (y, a) = _metric_inputs((3, 4097), params, seed=31)
    mask = np.ones((3, 4097), dtype=np.float32)
    mask[:, ::3] = 0.0
    (y[0, 4096], a[2, 1]) = (np.nan, np.nan)
    assert mask[0, 4096] != 0 and mask[2, 1] != 0
    got = _metric_both(y, a, mask, params, "NaN under a kept pixel")
    assert np.isnan(got[0, [2, 4, 5, 6, 7]]).all() and np.isfinite(got[0, [0, 1, 3]]).all()     # a NaN score: e', a - e
    assert np.isnan(got[2, [1, 3, 5, 6, 7]]).all() and np.isfinite(got[2, [0, 2, 4]]).all()     # a NaN target: a', a - e
    assert np.isfinite(got[1]).all()


@pytest.mark.parametrize("kind", ["bool", "float64"])
def test_metric_sums_cast_and_broadcast_the_mask(kind):
    """a mask of (n, 1, h, w) against scores of (n, c, h, w), as DSDataset.device_mask hands it over"""
    params = ref.ARBITRARY_F64
    (y, a) = _metric_inputs((3, 2, 17, 19), params, seed=41)
    rng = np.random.default_rng(42)
    mask = rng.random((3, 1, 17, 19)) < 0.6
    if kind == "float64":
        mask = np.where(mask, rng.choice([0.5, -1.0, 2.0], mask.shape), 0.0)
    assert mask.dtype == np.dtype(kind)
    got = _metric_both(y, a, mask, params, f"{kind} mask broadcast over the channels")
    assert np.array_equal(got[:, 0], 2 * (mask != 0).reshape(3, -1).sum(axis=1))


def test_metric_sums_over_more_instances_than_one_launch_takes():
    """65 541 instances of 4 pixels: the wrapper's second call starts at instance 65 535"""
    params = ref.ARBITRARY_F64
    n = 65541
    (y, a) = _metric_inputs((n, 4), params, seed=51)
    mask = (np.random.default_rng(52).random((n, 4)) < 0.7).astype(np.float32)
    got = _metric_both(y, a, mask, params, "65 541 instances", rows=[0, 65534, 65535, 65540])
    assert np.array_equal(got[:, 0], (mask != 0).sum(axis=1))


# ---- cae_bswap32 ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 1023, 1024, 1025, BSWAP_CAP + 1031])
def test_bswap32_against_byteswap(n):
    guard = 8
    words = np.random.default_rng(n).integers(0, 2 ** 32, n + guard, dtype=np.uint32)
    buf = _cuda(words.view(np.int32))
    assert buf.data_ptr() % 16 == 0
    lib = _lib.load()
    _lib.check(lib.cae_bswap32(buf.data_ptr(), n, None))
    torch.cuda.synchronize()
    once = _u32(buf.cpu().numpy())
    assert np.array_equal(once[:n], words[:n].byteswap()) and np.array_equal(once[n:], words[n:])
    _lib.check(lib.cae_bswap32(buf.data_ptr(), n, None))
    torch.cuda.synchronize()
    assert np.array_equal(_u32(buf.cpu().numpy()), words)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025, BSWAP_CAP + 1031])
def test_upload_of_a_big_endian_slab(n):
    """any bit pattern, NaN payloads included, arrives as the native float of the same value"""
    words = np.random.default_rng(n + 1).integers(0, 2 ** 32, n, dtype=np.uint32)
    slab = words.astype(">u4").view(">f4")
    got = upload_f32(slab, _dev())
    assert got.dtype == torch.float32 and got.shape == (n,)
    assert np.array_equal(_u32(got.view(torch.int32).cpu().numpy()), words)


# ---- a constant output variable ------------------------------------------------------------------------

def test_constant_output_variable_normalises_to_zero_and_comes_back():
    """Deliberately not the reference: its DSDataset guards a range of 0 for the inputs only, so a constant output variable
    is 0 / 0 = NaN there.  Here inputs and output go through the same kernel, which writes 0 at range 0: training targets
    0, and denormalising any score gives the constant back."""
    from cae_tools_amd.data.arrays import DataArray, Dataset
    from cae_tools_amd.models.ds_dataset import DSDataset
    rng = np.random.default_rng(61)
    ds = Dataset()
    ds["lowres"] = DataArray((288 + 10 * rng.random((5, 1, 6, 4))).astype(np.float32), dims=("n", "c", "y", "x"))
    ds["flat"] = DataArray(np.full((5, 2, 6, 4), 3.25, dtype=np.float32), dims=("n", "c2", "y", "x"))
    ds["hires"] = DataArray(np.full((5, 1, 12, 8), 291.75, dtype=np.float32), dims=("n", "c", "Y", "X"))
    d = DSDataset(ds, ["lowres", "flat"], "hires")
    (mins, maxs, omin, omax) = d.get_normalisation_parameters()
    assert omin == omax == 291.75 and mins["flat"] == maxs["flat"] == 3.25
    t = d.device_outputs().cpu().numpy()
    assert t.shape == (5, 1, 12, 8) and t.tobytes() == np.zeros_like(t).tobytes()
    assert not d.device_inputs().cpu().numpy()[:, 1:].any()
    (_, t_rows) = d.device_batches(np.random.default_rng(62).permutation(5))
    assert not t_rows.cpu().numpy().any()
    assert not d[3][1].any()
    scores = _cuda(np.concatenate([ref.unit_scores(93), np.array([-2.0, 0.0, 1.0], dtype=np.float32)]))
    for back in (denormalise_f64(scores, omin, omax), d.denormalise_device(scores)):
        assert (back.cpu().numpy() == 291.75).all()
