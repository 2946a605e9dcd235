"""The stateless evaluation kernels past their grid caps.  Every entry point sizes its grid with ceil_capped(n, per, cap)
(csrc/stateless_host.h); past per * cap items the kernel changes regime: a wave of k_joint_hist and k_strata_sums walks `per`
> 1 consecutive items into the same LDS table, the workgroups of every other kernel come round for a second grid-stride trip.
Each test here makes the smallest call past a cap, and the boundary call just under it where that call is named in SHAPES,
and holds it to the restatement the kernel's own module uses (distribution_ref, strata_ref, ensemble_verify_ref, importance_ref,
compare_ref, conformal_ref, scene_ref, neighbours_ref, the numpy helpers of test_case_pages_gpu and test_ensemble_moments_gpu)
under that module's bound, unchanged.  Where a restatement built on math.fsum or np.longdouble is too slow for the shape (11.2
million pixels for the histogram and the strata, 4 and 19 million for the importance and comparison sums), the inputs lie on
a dyadic grid - multiples of 2^-6 in [0, 16) - so that every addend is a multiple of 2^-12 below 2^8 and every partial sum
of fewer than 2^33 of them is exact in fp64 in any order: the reference is np.bincount or np.sum and every sum is compared
with ==.  Each such test asserts that precondition on its own inputs.

A test proves its regime: from the workgroup count the library gives away through its workspace size (cae_joint_hist,
cae_strata_sums, cae_ensemble_verify), else from CAPS below, which test_grid_caps_cpu.py holds to the host code: a changed
cap, or a new capped launch, fails there.  Wrappers that cut a call into groups of cases (case_compare, render_cases) are
asserted to hold the whole call in one group.

Of the folds whose caps are cheap to pass, k_pixel_fold and k_baseline_fold are driven at the end of the module.
Out of scope, by size: cae_ensemble_verify capped with more than one chunk a case (over 33 million pixels times K), the
map variant of cae_case_importance and the pixel mode of the quantiles (2^20 tiles), cae_bootstrap_sums unstaged (4 million
resamples of 5200 draws); test_grid_caps_cpu.py lists them with the other launches this module does not drive.

Largest |got - want| / bound measured on an MI355X (each check prints its figure before it asserts) and the wall time of each
test: DESIGN.md section 2, "The evaluation kernels past their grid caps"."""
import numpy as np
import pytest
import torch

import baseline_ref
import compare_ref
import conformal_ref
import distribution_ref
import ensemble_verify_ref
import importance_ref
import neighbours_ref
import scene_ref
import skill_maps_ref
import strata_ref
import test_ensemble_moments_gpu as moments
import test_ensemble_verify_gpu as verify_mod
from cae_tools_amd import _lib, case_ops
from cae_tools_amd.engine import (bootstrap_sums, case_baseline, case_compare, case_importance, case_neighbours, device_operand, interval_bounds,
                                  joint_histogram, normalise_pack, pack_gather, pixel_sums, render_cases, scene_plan, scene_tiles, strata_sums)
from test_case_pages_gpu import np_scanlines, np_values
from test_compare_gpu import _fields as compare_fields, _shape as compare_shape
from test_conformal_gpu import LEVELS, bits, noise, raw_quantiles, verify as conformal_verify
from test_importance_gpu import _scores as importance_scores
from test_joint_hist_gpu import _check as hist_check, _nchw as hist_nchw, _sprinkle as hist_sprinkle
from test_neighbours_gpu import grid_rows, same as same_neighbours
from test_scene_gpu import _packed_on_the_host
from test_strata_gpu import _compare as strata_compare, _edges, _nchw as strata_nchw, _sprinkle as strata_sprinkle

pytestmark = pytest.mark.gpu

# kernel: (per, cap) - the items a workgroup takes in one trip and the most workgroups of a launch, as the host code sizes
# the grid: ceil_capped(items, per, cap).  test_grid_caps_cpu.py reads both from csrc/host_*.h and compares.
CAPS = {
    "k_joint_hist": (4, 1024),
    "k_strata_sums": (4, 1024),
    "k_ensemble_verify": (1, 8192),
    "k_ensemble_moments": (4, 65536),
    "k_case_importance": (4, 16384),
    "k_importance_fold": (4, 8192),
    "k_case_compare": (4, 16384),
    "k_compare_fold": (4, 8192),
    "k_quantile_pool_count": (16, 2048),
    "k_score_counts_pool": (16, 2048),
    "k_interval_bounds": (1024, 8192),
    "k_quantile_fill": (256, 4096),
    "k_bootstrap_sums staged": (256, 2048),
    "k_scene_gather": (1024, 8192),
    "k_normalise_pack_gather": (2048, 8192),
    "k_render_cases": (4, 8192),
    "k_nb_valid": (4, 8192),
    "k_pixel_fold": (256, 8192),
    "k_baseline_fold": (256, 4096),
}


def _ensemble_chunks(n_case, plane):
    """ensemble_chunks of host_ensemble.h: chunks of 64 .. 1024 4-pixel groups, about 4096 wave items a call"""
    groups = (plane + 3) // 4
    chunk = min(max((n_case * groups // 4096 + 63) // 64 * 64, 64), 1024)
    return -(-groups // chunk)


def _scene_total(Y, X, box, n_t):
    """elements of a gather of one variable of one channel: overlap 0, square boxes"""
    return n_t * len(scene_ref.origins(Y, box, 0)) * len(scene_ref.origins(X, box, 0)) * box * box


# kernel: the items of a call of that shape, as the host code counts them
ITEMS = {
    "k_joint_hist": lambda n, plane: n * -(-plane // 4096),
    "k_strata_sums": lambda n, plane: n * -(-plane // 4096),
    "k_ensemble_verify": lambda n, plane, k: n * _ensemble_chunks(n, plane),
    "k_ensemble_moments": lambda n, plane, k: n * _ensemble_chunks(n, plane),
    "k_case_importance": lambda n, plane: -(-plane // 64) * -(-n // 8),
    "k_importance_fold": lambda n, plane: n,
    "k_case_compare": lambda n, plane: -(-plane // 64) * -(-n // 8),
    "k_compare_fold": lambda n, plane: n,
    "k_quantile_pool_count": lambda n, plane: -(-n * plane // 64),
    "k_score_counts_pool": lambda n, plane: -(-n * plane // 64),
    "k_interval_bounds": lambda n, plane: n * plane,
    "k_quantile_fill": lambda plane, levels: plane * levels,
    "k_bootstrap_sums staged": lambda n_unit, n_col, resamples: resamples * -(-n_col // 4),       # the wide lanes: 4 columns each
    "k_scene_gather": _scene_total,
    "k_normalise_pack_gather": lambda n_dst, c, hw: n_dst * c * hw,
    "k_render_cases": lambda n_sel, h, w: n_sel * max(1, -(-(h * (w + 1) // 4) // 1024)),
    "k_nb_valid": lambda rows: rows,
    "k_pixel_fold": lambda n, plane: 9 * plane,                # the nine sums of every pixel
    "k_baseline_fold": lambda n: 6 * n,                        # the six sums of every case
}

# kernel: (the shapes past the cap that this module runs, the boundary shapes: the last calls the cap does not touch)
SHAPES = {
    "k_joint_hist": ([(4097, 5), (8193, 1), (1366, 8195)], [(4096, 5)]),
    "k_strata_sums": ([(4097, 5), (8193, 1), (1366, 8195)], [(4096, 5)]),
    "k_ensemble_verify": ([(8193, 3, 3), (20000, 5, 2), (8200, 1, 64)], [(8192, 3, 3)]),
    "k_ensemble_moments": ([(262145, 1, 2), (262145, 3, 3)], [(262144, 1, 2)]),
    "k_case_importance": ([(1, 64 * 65536 + 1), (9, 64 * 32768 + 1)], [(1, 64 * 65536), (9, 64 * 32768)]),
    "k_importance_fold": ([(32769, 1), (32769, 65)], [(32768, 1)]),
    "k_case_compare": ([(1, 64 * 65536 + 1), (9, 64 * 32768 + 1)], [(1, 64 * 65536), (9, 64 * 32768)]),
    "k_compare_fold": ([(32769, 1), (32769, 65)], [(32768, 1)]),
    # 2 097 152 scores are no three cases of a plane: the boundary is four cases of 524 288
    "k_quantile_pool_count": ([(3, 699051)], [(4, 524288)]),
    "k_score_counts_pool": ([(3, 699051)], [(4, 524288)]),
    "k_interval_bounds": ([(3, 2796203)], [(2, 4194304)]),
    "k_quantile_fill": ([(262145, 4)], [(262144, 4)]),
    "k_bootstrap_sums staged": ([(5, 32, 65537)], [(5, 32, 65536)]),
    "k_scene_gather": ([(1500, 1500, 64, 4)], [(2048, 4096, 64, 1)]),
    "k_normalise_pack_gather": ([(4100, 1, 4096)], [(4096, 1, 4096)]),
    "k_render_cases": ([(32769, 1, 3)], [(32768, 1, 3)]),
    "k_nb_valid": ([(32769,)], [(32768,)]),
    "k_pixel_fold": ([(3, 233017)], [(3, 233016)]),
    "k_baseline_fold": ([(174763,)], [(174762,)]),
}

VERIFY_SHAPES = SHAPES["k_ensemble_verify"][1] + SHAPES["k_ensemble_verify"][0]
HIST_SHAPES = SHAPES["k_joint_hist"][1] + SHAPES["k_joint_hist"][0][:2]


def trips(kernel, shape):
    """the grid-stride trips of the busiest workgroup (for k_joint_hist and k_strata_sums: the items of the busiest wave)"""
    (per, cap) = CAPS[kernel]
    return -(-ITEMS[kernel](*shape) // (per * cap))


def _past(kernel, shape):
    assert shape in SHAPES[kernel][0] and trips(kernel, shape) >= 2, (kernel, shape)


def _under(kernel, shape):
    assert shape in SHAPES[kernel][1] and trips(kernel, shape) == 1, (kernel, shape)


def _dyadic(rng, shape, dtype=np.float32):
    """multiples of 2^-6 in [0, 16): exact in fp32"""
    return (rng.integers(0, 1024, size=shape) / 64.0).astype(dtype)


def _assert_exact(count, *addends):
    """the precondition of the == comparisons: every addend a multiple of 2^-12, and `count` of the largest below 2^53 / 2^12"""
    for x in addends:
        scaled = np.asarray(x, dtype=np.float64) * 4096.0
        assert np.array_equal(scaled, np.rint(scaled))
        assert count * float(np.abs(scaled).max(initial=0.0)) < 2.0 ** 53


def _misaligned(x4, off):
    """an fp32 (N, C, h, w) array as a CUDA tensor that starts `off` floats after a 16-byte boundary"""
    flat = torch.empty(x4.size + off, dtype=torch.float32, device="cuda")
    flat[off:] = torch.from_numpy(np.ascontiguousarray(x4).reshape(-1)).cuda()
    t = flat[off:].view(x4.shape)
    assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
    return t


# ---- 1. cae_joint_hist and cae_strata_sums: a wave walks `per` items ---------------------------------------------------------

def _hist_regime(n, plane, n_bin, sub):
    """(workgroups, items a wave walks) of a cae_joint_hist call, the workgroups from the workspace size"""
    groups = int(_lib.load().cae_joint_hist_workspace_bytes(n, plane, n_bin, sub)) // (2 * n_bin * 4 * 8)
    items = ITEMS["k_joint_hist"](n, plane)
    assert groups == min(-(-items // 4), CAPS["k_joint_hist"][1])
    return groups, -(-items // (4 * groups))


def _strata_regime(n, h, w, n_strata):
    groups = int(_lib.load().cae_strata_sums_workspace_bytes(n, h, w, n_strata)) // (n_strata * 8 * 8)
    items = ITEMS["k_strata_sums"](n, h * w)
    assert groups == min(-(-items // 4), CAPS["k_strata_sums"][1])
    return groups, -(-items // (4 * groups))


@pytest.mark.parametrize("shape", HIST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_joint_hist_at_and_past_the_cap(shape):
    """(4096, 5): 4096 items, the last call with an item a wave.  (4097, 5): two items a wave, waves 2049 .. 4095 and
    workgroups 513 .. 1023 idle, their all-zero partials in the fold.  (8193, 1): three items a wave, the last run short.
    Then the same values as misaligned fp32 tensors of two channels: the case starts go through every 16-byte phase, so the
    head and tail lanes run between the items of a wave."""
    (n, plane) = shape
    (n_bin, sub, hi) = (128, 8, 16.0)
    (groups, per) = _hist_regime(n, plane, n_bin, sub)
    assert (groups, per) == (1024, trips("k_joint_hist", shape)) and per == {4096: 1, 4097: 2, 8193: 3}[n]
    (_under if per == 1 else _past)("k_joint_hist", shape)
    rng = np.random.default_rng(n * 10 + plane)
    a = rng.uniform(0.0, hi, (n, plane))
    p = 0.5 * hi + 0.7 * (a - 0.5 * hi) + 0.01 * hi * rng.standard_normal(a.shape)
    hist_sprinkle(rng, p, a, hi, n_bin)
    got = joint_histogram(hist_nchw(p, 1, plane), hist_nchw(a, 1, plane), 0.0, hi, n_bin=n_bin, sub=sub)
    ref = distribution_ref.Reference(p, a, 0.0, hi, n_bin, sub)
    hist_check(f"{n} cases of {plane}, {per} items a wave", got, ref, n_bin, sub)
    assert ref.outside.sum() > 0 and ref.pairs < n * plane
    with np.errstate(over="ignore"):
        (p4, a4) = (hist_nchw(p, 1, plane, 2, np.float32), hist_nchw(a, 1, plane, 2, np.float32))
    got = joint_histogram(_misaligned(p4, 1), _misaligned(a4, 3), 0.0, hi, n_bin=n_bin, sub=sub)
    ref = distribution_ref.Reference(distribution_ref.channel0(p4), distribution_ref.channel0(a4), 0.0, hi, n_bin, sub)
    hist_check(f"{n} cases of {plane}, {per} items a wave, misaligned", got, ref, n_bin, sub)


def _big_fields(seed):
    """(1366, 8195) prediction and target on the dyadic grid, the prediction within 1 of the target, a few values not finite"""
    (n, plane) = SHAPES["k_joint_hist"][0][2]
    rng = np.random.default_rng(seed)
    a = _dyadic(rng, (n, plane))
    p = np.clip(a + (rng.integers(-64, 65, size=(n, plane)) / 64.0).astype(np.float32), 0.0, 1023.0 / 64.0).astype(np.float32)
    for (x, v) in ((p, np.nan), (a, np.inf), (p, -np.inf), (a, np.nan)):
        x.reshape(-1)[rng.integers(0, x.size, 50)] = v
    return rng, p, a


def test_joint_hist_exact_when_runs_straddle_cases():
    """1366 cases of 8195 pixels: three chunks a case, 4098 items, two a wave, so every other wave's run lies in two cases.
    Inputs on the dyadic grid, lo 0, hi 16, 128 x 8 bins (scale 64): every count and every sum compared with =="""
    (n, plane) = shape = SHAPES["k_joint_hist"][0][2]
    (n_bin, sub, hi) = (128, 8, 16.0)
    _past("k_joint_hist", shape)
    (groups, per) = _hist_regime(n, plane, n_bin, sub)
    assert (groups, per) == (1024, 2) and -(-plane // 4096) % per != 0          # a case is no whole number of runs
    (_, p, a) = _big_fields(1)
    got = joint_histogram(hist_nchw(p, 1, plane, 1, np.float32), hist_nchw(a, 1, plane, 1, np.float32), 0.0, hi, n_bin=n_bin, sub=sub)
    (p, a) = (p.astype(np.float64).reshape(-1), a.astype(np.float64).reshape(-1))
    pair = np.isfinite(p) & np.isfinite(a)
    (p, a) = (p[pair], a[pair])
    assert 0 < pair.size - p.size <= 200
    (fa, fp) = (distribution_ref.fine_bins(a, 0.0, hi, n_bin, sub), distribution_ref.fine_bins(p, 0.0, hi, n_bin, sub))
    assert np.array_equal(fa, (a * 64.0).astype(np.int64))                      # the scale is a power of two
    (ia, ip) = (fa // sub, fp // sub)
    d = p - a
    addends = ((d, np.abs(d), d * d, a), (d, np.abs(d), d * d, p))
    _assert_exact(p.size, *addends[0], *addends[1])
    (joint, marg, cond, outside) = got
    assert np.array_equal(joint, np.bincount(ia * n_bin + ip, minlength=n_bin * n_bin).reshape(n_bin, n_bin))
    assert np.array_equal(marg, np.stack([np.bincount(fa, minlength=n_bin * sub), np.bincount(fp, minlength=n_bin * sub)]))
    assert not outside.any() and int(joint.sum()) == p.size
    for (k, keys) in enumerate((ia, ip)):
        for (j, x) in enumerate(addends[k]):
            assert np.array_equal(cond[k, :, j], np.bincount(keys, weights=x, minlength=n_bin)), (k, j)
    assert (joint.sum(axis=1) > 0).all()                                        # the data spreads over the bins


@pytest.mark.parametrize("shape", HIST_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_strata_sums_at_and_past_the_cap(shape):
    """the shapes of test_joint_hist_at_and_past_the_cap, six edges, the stratifier on a coarser grid where the plane has
    room for one; then the same values as misaligned fp32 tensors of two channels"""
    (n, w) = shape
    sw = 2 if w > 1 else 1
    edges = _edges(6)
    (groups, per) = _strata_regime(n, 1, w, len(edges) + 1)
    assert (groups, per) == (1024, trips("k_strata_sums", shape)) and per == {4096: 1, 4097: 2, 8193: 3}[n]
    (_under if per == 1 else _past)("k_strata_sums", shape)
    rng = np.random.default_rng(n * 10 + w + 1)
    a = rng.random((n, 1, w))
    p = 0.5 + 0.7 * (a - 0.5) + 0.01 * rng.standard_normal(a.shape)
    s = rng.random((n, 1, sw))
    for x in (p, a, s):
        strata_sprinkle(rng, x, [np.nan, np.inf, -np.inf, 1e300, -0.0, 2.5, -1.0] * 3)
    shift = rng.random((2, len(edges) + 1))
    got = strata_sums(strata_nchw(p), strata_nchw(a), strata_nchw(s), edges, shift)
    ref = strata_ref.Reference(p, a, s, edges, shift)
    strata_compare(f"{n} cases of 1 x {w}, {per} items a wave", got, ref)
    assert ref.unclassified > 0 and (ref.pairs > 0).all() and int(ref.pairs.sum()) < n * w
    with np.errstate(over="ignore"):
        arrays = [strata_nchw(x, 2, np.float32) for x in (p, a, s)]
    stored = [np.asarray(x[:, 0], dtype=np.float64) for x in arrays]
    got = strata_sums(*[device_operand(_misaligned(x, off)) for (x, off) in zip(arrays, (1, 3, 2))], edges, shift)
    strata_compare(f"{n} cases of 1 x {w}, {per} items a wave, misaligned", got, strata_ref.Reference(*stored, edges, shift))


def test_strata_sums_exact_when_runs_straddle_cases():
    """1366 cases of 1 x 8195 pixels under a stratifier of 1 x 745, seven edges, per-stratum shifts: the operands, the
    stratifier and the shifts on the dyadic grid, every count and every sum compared with =="""
    (n, w) = shape = SHAPES["k_strata_sums"][0][2]
    sw = 745
    edges = [2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0]
    n_strata = len(edges) + 1
    _past("k_strata_sums", shape)
    (groups, per) = _strata_regime(n, 1, w, n_strata)
    assert (groups, per) == (1024, 2) and -(-w // 4096) % per != 0
    (rng, p, a) = _big_fields(2)
    s = _dyadic(rng, (n, 1, sw))
    s.reshape(-1)[rng.integers(0, s.size, 40)] = np.nan
    shift = rng.integers(0, 1024, size=(2, n_strata)) / 64.0
    got = strata_sums(strata_nchw(p.reshape(n, 1, w), 1, np.float32), strata_nchw(a.reshape(n, 1, w), 1, np.float32),
                      strata_nchw(s, 1, np.float32), edges, shift)
    v = strata_ref.on_target_grid(s.astype(np.float64), 1, w).reshape(-1)
    (p, a) = (p.astype(np.float64).reshape(-1), a.astype(np.float64).reshape(-1))
    cls = np.isfinite(v)
    k = np.where(cls, strata_ref.strata_of(np.where(cls, v, 0.0), edges), -1)
    pair = cls & np.isfinite(p) & np.isfinite(a)
    (kk, pp, aa) = (k[pair], p[pair], a[pair])
    (d, a1, p1) = (pp - aa, aa - shift[0][kk], pp - shift[1][kk])
    addends = (d, np.abs(d), d * d, a1, p1, a1 * a1, p1 * p1, a1 * p1)
    _assert_exact(pp.size, *addends)
    (counts, sums) = got
    assert np.array_equal(counts["members"], np.bincount(k[cls], minlength=n_strata))
    assert np.array_equal(counts["pairs"], np.bincount(kk, minlength=n_strata))
    assert counts["unclassified"] == int((~cls).sum()) > 0 and int(counts["members"].sum()) + counts["unclassified"] == n * w
    assert (counts["pairs"] > 0).all() and int(counts["pairs"].sum()) < int(counts["members"].sum())
    for (q, x) in enumerate(addends):
        assert np.array_equal(sums[:, q], np.bincount(kk, weights=x, minlength=n_strata)), q


# ---- 2. cae_ensemble_verify: a workgroup's rank counters carried over its items ------------------------------------------

def _verify_data(n_case, plane, k, seed):
    """(y (n_case, k, plane) fp32, target (n_case, plane) fp64): per pixel at random the target below all members (bin 0),
    above all (bin K), inside, equal to member 0 (a tie), NaN, or one draw NaN; spreads from 0.3 down to all draws equal"""
    rng = np.random.default_rng(seed)
    base = 0.25 + 0.5 * rng.random((n_case, 1, plane))
    spread = rng.choice([0.3, 1e-3, 6e-8, 0.0], size=(n_case, 1, plane))
    y = (base + spread * rng.standard_normal((n_case, k, plane))).astype(np.float32)
    m = ensemble_verify_ref.members(y, verify_mod.VMIN, verify_mod.RANGE)
    (lo, hi) = (m.min(axis=1), m.max(axis=1))
    kind = rng.integers(0, 8, size=(n_case, plane))
    a = 0.5 * (lo + hi) + 0.25 * (hi - lo) * (rng.random((n_case, plane)) - 0.5)
    a = np.where(kind == 0, lo - 0.5 - rng.random((n_case, plane)), a)
    a = np.where(kind == 1, hi + 0.5 + rng.random((n_case, plane)), a)
    a = np.where(kind == 2, m[:, 0], a)
    a = np.where(kind == 3, np.nan, a)
    (cs, px) = np.nonzero(kind == 4)
    y[cs, rng.integers(0, k, size=cs.size), px] = np.nan
    return y, a


def _verify_check(label, got, y, a):
    """test_ensemble_verify_gpu's _check with the cases side by side: the rank counts, the tie count and n per case exactly,
    the four sums within c 2^-53 S|terms| of ensemble_verify_ref's terms added in pixel order"""
    (sums, ranks) = got
    (n_case, k, plane) = y.shape
    t = ensemble_verify_ref.pixel_terms(y.transpose(1, 0, 2).reshape(k, -1), a.reshape(-1), verify_mod.VMIN, verify_mod.RANGE)
    w = t["counted"]
    want_ranks = np.zeros(k + 2, dtype=np.int64)
    want_ranks[:k + 1] = np.bincount(t["below"][w], minlength=k + 1)
    want_ranks[k + 1] = int((t["tied"] & w).sum())
    assert np.array_equal(ranks, want_ranks), f"{label}: rank counts {ranks} != {want_ranks}"
    assert np.array_equal(sums[:, 0], w.reshape(n_case, plane).sum(axis=1)), label
    adds = (plane * k, plane * k * (k - 1) // 2, plane * (k + 3), plane * (2 * k + 3))
    for (q, name) in enumerate("ABEV"):
        term = np.where(w, t[name], 0.0).reshape(n_case, plane)
        want = np.zeros(n_case)
        for j in range(plane):
            want = want + term[:, j]
        bound = adds[q] * verify_mod.U * np.abs(term).sum(axis=1)
        err = np.abs(sums[:, 1 + q] - want)
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
        print(f"{label} S{name}: max |got - want| / bound = {worst:.3e} over {n_case} cases ({adds[q]} additions)")
        assert (err <= bound).all(), f"{label} S{name}"
    return want_ranks


@pytest.mark.parametrize("shape", VERIFY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ensemble_verify_carries_its_counters_over_items(shape):
    """One chunk a case, so the cases are the items and a workgroup is one wave.  (8192, 3, 3): an item each.  (8193, 3, 3):
    workgroup 0 takes items 0 and 8192.  (20000, 5, 2): two to three items a workgroup, the head and tail lanes with their
    __syncthreads between the items.  (8200, 1, 64): bin 64, which a wave-uniform counter keeps, carried over two items.
    (The capped call with more than one chunk a case takes over 33 million pixels times K: out of scope.)"""
    (n_case, plane, k) = shape
    assert _ensemble_chunks(n_case, plane) == 1
    lib = _lib.load()
    blocks = int(lib.cae_ensemble_verify_workspace_bytes(n_case, plane, k)) // ((k + 2) * 8)
    assert blocks == min(n_case, CAPS["k_ensemble_verify"][1]) and -(-n_case // blocks) == trips("k_ensemble_verify", shape)
    (_under if n_case == 8192 else _past)("k_ensemble_verify", shape)
    (y, a) = _verify_data(n_case, plane, k, seed=n_case + k)
    got = verify_mod._run(y, a, verify_mod.F64, offset=1 if plane == 5 else 0)
    ranks = _verify_check(f"{n_case} cases of {plane}, K {k}", got, y, a)
    assert ranks[0] > 0 and ranks[k] > 0 and ranks[k + 1] > 0 and ranks.sum() - ranks[k + 1] < n_case * plane


# ---- 3. cae_ensemble_moments ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES["k_ensemble_moments"][1] + SHAPES["k_ensemble_moments"][0], ids=lambda s: "x".join(map(str, s)))
def test_ensemble_moments_past_the_cap(shape):
    """65536 workgroups of 4 (case, chunk) items: 262 144 cases of one pixel are the last call without a second trip.  numpy's
    fp64 mean and std(ddof=1) under the bounds of test_ensemble_moments_gpu, equal draws exactly 0, and the draws delivered
    as [1, 1] / [2, 1] through the workspace bitwise equal to one call"""
    (n_case, plane, k) = shape
    assert _ensemble_chunks(n_case, plane) == 1
    (_under if n_case == 262144 else _past)("k_ensemble_moments", shape)
    rng = np.random.default_rng(n_case + plane)
    spread = np.asarray(moments.SPREADS)[np.arange(n_case * plane) % len(moments.SPREADS)].reshape(n_case, 1, plane)
    y = (rng.random((n_case, 1, plane)) + spread * rng.standard_normal((n_case, k, plane))).astype(np.float32)
    y64 = y.astype(np.float64)
    (ref_mean, ref_std) = (moments.VMIN + y64.mean(axis=1) * moments.RANGE, y64.std(axis=1, ddof=1) * moments.RANGE)
    whole = moments._run(y, 1, "draw", False)
    split = moments._run(y, 1, "draw", False, parts=[k - 1, 1])
    (mean, std) = whole
    mean_err = float(np.abs(mean - ref_mean).max())
    std_excess = float((np.abs(std - ref_std) - moments.STD_REL * ref_std).max())
    print(f"{shape}: max |mean error| / bound {mean_err / moments.MEAN_ABS:.3e}; max (|std error| - 1e-10 std) / bound "
          f"{std_excess / moments.STD_ABS:.3e}")
    assert np.isfinite(mean).all() and np.isfinite(std).all()
    assert mean_err <= moments.MEAN_ABS and std_excess <= moments.STD_ABS
    equal = (spread == 0.0).reshape(n_case, plane)
    assert equal.any() and (std[equal] == 0.0).all() and (std[~equal] > 0.0).any()
    assert np.array_equal(bits(split[0]), bits(mean)) and np.array_equal(bits(split[1]), bits(std))


# ---- 4. cae_case_importance (no map) and cae_case_compare ---------------------------------------------------------------

def _importance_rows(base, pert, a):
    """the eight sums per case with vmin 0 and range 1 (P is the score itself), plain fp64: exact on the dyadic grid"""
    rows = []
    for (b, q, t) in zip(base, pert, a):
        (P0, P1, A) = (b.astype(np.float64), q.astype(np.float64), t.astype(np.float64))
        pair = np.isfinite(A) & np.isfinite(P0) & np.isfinite(P1)
        (P0, P1, A) = (P0[pair], P1[pair], A[pair])
        (e0, e1, d) = (P0 - A, P1 - A, P1 - P0)
        (q0, q1) = (e0 * e0, e1 * e1)
        _assert_exact(A.size, q0, q1, d * d)
        rows.append([A.size, q1.sum(), q0.sum(), np.abs(e1).sum(), np.abs(e0).sum(), (d * d).sum(), (q1 > q0).sum(), (q1 < q0).sum()])
    return np.array(rows, dtype=np.float64)


def _compare_rows(preds, a):
    """{n, tied, (S e, S|e|, S e^2, wins) per candidate} per case, plain fp64: exact on the dyadic grid"""
    rows = []
    for c in range(a.shape[0]):
        A = a[c].astype(np.float64)
        P = [p[c].astype(np.float64) for p in preds]
        pair = np.isfinite(A)
        for p in P:
            pair &= np.isfinite(p)
        e = [p[pair] - A[pair] for p in P]
        q = np.stack([x * x for x in e])
        _assert_exact(q.shape[1], *q)
        qmin = q.min(axis=0)
        hits = (q == qmin[None]).sum(axis=0)
        row = [q.shape[1], (hits > 1).sum()]
        for (m, x) in enumerate(e):
            row += [x.sum(), np.abs(x).sum(), q[m].sum(), ((hits == 1) & (q[m] == qmin)).sum()]
        rows.append(row)
    return np.array(rows, dtype=np.float64)


def _dyadic_scores(shape):
    """base, pert and target (n, plane) fp32 on the dyadic grid: a tenth of the perturbed scores equal to the unperturbed, a
    few values that are not finite, and the last pixel of the last case - the item of the second trip - a pair"""
    rng = np.random.default_rng(shape[1])
    (base, pert, a) = (_dyadic(rng, shape), _dyadic(rng, shape), _dyadic(rng, shape))
    same = rng.random(shape) < 0.1
    pert[same] = base[same]                                     # neither grew nor shrank; a tie of two candidates
    for (x, v) in ((a, np.nan), (base, np.inf), (pert, np.nan), (a, -np.inf)):
        x.reshape(-1)[rng.integers(0, x.size, 20)] = v
    (a[-1, -1], base[-1, -1], pert[-1, -1]) = (3.0, 1.0, 6.5)
    return base, pert, a


@pytest.mark.parametrize("shape", SHAPES["k_case_importance"][0], ids=lambda s: f"{s[0]}x{s[1]}")
def test_importance_main_kernel_comes_round_again(shape):
    """(1, 64 * 65536 + 1): 65 537 tiles, the last one, of one pixel, is the second trip of workgroup 0.  (9, 64 * 32768 + 1):
    two runs of cases per tile, 65 538 items.  vmin 0, range 1 and operands on the dyadic grid: every sum compared with =="""
    (n, plane) = shape
    _past("k_case_importance", shape)
    (base, pert, a) = _dyadic_scores(shape)
    nchw = (n, 1, 1, plane)
    got = case_importance(torch.from_numpy(base.reshape(nchw)).cuda(), torch.from_numpy(pert.reshape(nchw)).cuda(), a.reshape(nchw), 0.0, 1.0)
    want = _importance_rows(base, pert, a)
    assert got.dtype == np.float64 and np.array_equal(got, want), np.nonzero(got != want)
    assert (want[:, 6] > 0).all() and (want[:, 7] > 0).all() and want[:, 0].sum() < n * plane


@pytest.mark.parametrize("shape", SHAPES["k_case_compare"][0], ids=lambda s: f"{s[0]}x{s[1]}")
def test_compare_main_kernel_comes_round_again(shape):
    """the shapes and operands of test_importance_main_kernel_comes_round_again, two candidates, every sum compared with =="""
    (n, plane) = shape
    _past("k_case_compare", shape)
    (base, pert, a) = _dyadic_scores(shape)
    nchw = (n, 1, 1, plane)
    assert case_ops._COMPARE_BYTES // int(_lib.load().cae_case_compare_workspace_bytes(1, plane, 2)) >= n       # one call
    got = case_compare([base.reshape(nchw), pert.reshape(nchw)], a.reshape(nchw))
    want = _compare_rows([base, pert], a)
    assert got.dtype == np.float64 and np.array_equal(got, want), np.nonzero(got != want)
    assert (want[:, 1] > 0).all() and (want[:, 5] > 0).all() and (want[:, 9] > 0).all()


@pytest.mark.parametrize("shape", SHAPES["k_importance_fold"][0], ids=lambda s: f"{s[0]}x{s[1]}")
def test_importance_fold_comes_round_again(shape):
    """32 769 cases: 8192 fold workgroups of four waves, and case 32 768 is the second trip of workgroup 0, wave 0; at 65
    pixels a lane of the fold adds a second tile.  The module's own reference and bound"""
    (n, plane) = shape
    _past("k_importance_fold", shape)
    rng = np.random.default_rng(n + plane)
    (base, pert, a) = importance_scores(rng, n, plane)
    a.reshape(-1)[rng.integers(0, a.size, 30)] = np.nan
    a[n - 2] = np.nan                                           # a case without a pair next to the last one
    nchw = (n, 1, 1, plane)
    got = case_importance(torch.from_numpy(base.reshape(nchw)).cuda(), torch.from_numpy(pert.reshape(nchw)).cuda(), a.reshape(nchw),
                          288.0, 298.0)
    importance_ref.Reference(base, pert, a, 288.0, 10.0).check(got, f"fold past the cap, {n} cases of {plane}")
    assert got[n - 1, 0] > 0 and got[n - 2, 0] == 0


@pytest.mark.parametrize("shape", SHAPES["k_compare_fold"][0], ids=lambda s: f"{s[0]}x{s[1]}")
def test_compare_fold_comes_round_again(shape):
    """the shapes of test_importance_fold_comes_round_again, three candidates, the module's own reference and bound"""
    (n, plane) = shape
    _past("k_compare_fold", shape)
    rng = np.random.default_rng(n + plane + 1)
    (preds, target) = compare_fields(rng, 3, n, plane)
    target.reshape(-1)[rng.integers(0, target.size, 30)] = np.nan
    target[n - 2] = np.nan
    assert case_ops._COMPARE_BYTES // int(_lib.load().cae_case_compare_workspace_bytes(1, plane, 3)) >= n       # one call
    got = case_compare([compare_shape(p) for p in preds], compare_shape(target))
    compare_ref.Reference(preds, target).check(got, f"fold past the cap, {n} cases of {plane}, M 3")
    assert got[n - 1, 0] > 0 and got[n - 2, 0] == 0


# ---- 5. pooled quantiles and counts, the bounds, the fill of an empty call ---------------------------------------------------

def test_pooled_quantiles_and_counts_past_the_cap():
    """2 097 153 scores in 3 cases: 32 769 chunks of 64 for 2048 workgroups of 16, so wave 0 of workgroup 0 comes round
    again in all eight passes and in the counts.  The module's verify(): bit-for-bit quantiles, exact counts, the
    identities of a k-th smallest value, two runs.  2 097 152 scores are the last call without the second trip."""
    for kernel in ("k_quantile_pool_count", "k_score_counts_pool"):
        _past(kernel, SHAPES[kernel][0][0])
        _under(kernel, SHAPES[kernel][1][0])
        assert ITEMS[kernel](*SHAPES[kernel][1][0]) * 64 == 2097152 == 64 * CAPS[kernel][0] * CAPS[kernel][1]
    (n, plane) = SHAPES["k_quantile_pool_count"][0][0]
    assert n * plane == 2097153
    rng = np.random.default_rng(21)
    (p, a) = noise(rng, n, 1, plane)
    # the scores of the second trip are the largest of all: every level's count would miss them
    (p[n - 1, 0, 0, -1], a[n - 1, 0, 0, -1]) = (5.0, 0.0)
    (q, count) = conformal_verify(p, a, "pooled", twice=True)
    assert 0 < count < n * plane and np.isfinite(q).all()


def test_interval_bounds_past_the_cap():
    """8 388 609 elements for 8192 workgroups of 1024: pooled, an fp32 scale, bit for bit against conformal_ref.bounds"""
    (n, plane) = shape = SHAPES["k_interval_bounds"][0][0]
    _past("k_interval_bounds", shape)
    _under("k_interval_bounds", SHAPES["k_interval_bounds"][1][0])
    rng = np.random.default_rng(22)
    p = 280.0 + 20.0 * rng.random((n, 1, 1, plane))
    s = (0.1 + rng.random((n, 1, 1, plane)) / 3.0).astype(np.float32)
    for (x, values) in ((p, (np.nan, np.inf, -np.inf)), (s, (0.0, -0.0, -2.0, np.nan, np.inf))):
        for v in values:
            x.reshape(-1)[rng.integers(0, x.size, 1000)] = v
    (p[n - 1, 0, 0, -1], s[n - 1, 0, 0, -1]) = (291.5, 0.25)    # the element of the second trip has an answer
    q = np.float64(1.0 / 3.0)
    (lo, hi) = interval_bounds(p, q, "pooled", scale=s)
    (want_lo, want_hi) = conformal_ref.bounds(p, q, s)
    for (got, want) in ((lo.cpu().numpy(), want_lo), (hi.cpu().numpy(), want_hi)):
        assert got.shape == want.shape == (n, 1, plane)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        assert ok[n - 1, 0, -1] and np.array_equal(bits(got)[ok], bits(want)[ok])
    assert np.isnan(want_lo).any()


def test_quantile_fill_past_the_cap():
    """an empty pixel-mode call over a plane of 262 145 with four levels: 1 048 580 values of +inf from 4096 workgroups of 256,
    the words behind them untouched, the counts 0"""
    (plane, levels) = shape = SHAPES["k_quantile_fill"][0][0]
    _past("k_quantile_fill", shape)
    _under("k_quantile_fill", SHAPES["k_quantile_fill"][1][0])
    assert levels == len(LEVELS)
    some = torch.zeros(16, dtype=torch.float32, device="cuda")
    op = (some.data_ptr(), _lib.ELEM_F32, plane)
    q = torch.full((levels * plane + 3,), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((plane + 3,), -7, dtype=torch.int64, device="cuda")
    assert raw_quantiles(op, op, (None, 0, 0), 0, plane, 0, LEVELS, q, cnt) == 0
    torch.cuda.synchronize()
    assert bool((q[:levels * plane] == float("inf")).all()) and bool((q[levels * plane:] == -7.0).all())
    assert bool((cnt[:plane] == 0).all()) and bool((cnt[plane:] == -7).all())


# ---- 6. cae_bootstrap_sums, the table staged in LDS ------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES["k_bootstrap_sums staged"][1] + SHAPES["k_bootstrap_sums staged"][0], ids=lambda s: "x".join(map(str, s)))
def test_bootstrap_sums_staged_past_the_cap(shape):
    """5 units of 32 columns fit the LDS; 65 537 resamples of 8 column groups are 524 296 wide lanes for 2048 workgroups of
    256.  Every row against compare_ref.sums with ==.  (Unstaged, the cap takes 4 million resamples of 5200 draws: out of
    scope.)"""
    (n_unit, n_col, b) = shape
    (_under if b == 65536 else _past)("k_bootstrap_sums staged", shape)
    assert n_unit * n_col * 8 <= 160 * 1024 and b * -(-n_col // 4) >= 1 << 17       # staged, and a lane takes 4 columns
    rng = np.random.default_rng(b)
    table = rng.gamma(2.0, 1.0, (n_unit, n_col)) * rng.choice([-1.0, 1.0], (n_unit, n_col))
    got = bootstrap_sums(table, b, seed=9)
    assert got.shape == (b, n_col) and got.dtype == np.float64
    assert np.array_equal(bits(got), bits(compare_ref.sums(table, b, seed=9)))


# ---- 7. the traffic kernels ------------------------------------------------------------------------------------------------

def test_scene_gather_past_the_cap():
    """a 1500 x 1500 scene in boxes of 64 x 64 without overlap, 4 time steps of one variable: 2304 tiles, 9 437 184 elements
    for 8192 workgroups of 1024.  The batch as bytes against normalise_pack of the boxes sliced on the host, the flags exact,
    one NaN in a tile the second trip covers"""
    (Y, X, box, n_t) = shape = SHAPES["k_scene_gather"][0][0]
    _past("k_scene_gather", shape)
    _under("k_scene_gather", SHAPES["k_scene_gather"][1][0])
    plan = scene_plan(Y, X, ((box, box), (box, box)), 0)
    assert n_t * plan.n_tile * box * box == ITEMS["k_scene_gather"](*shape)
    rng = np.random.default_rng(31)
    var = (280.0 + 10.0 * rng.random((n_t, 1, Y, X))).astype(np.float32)
    first_trip = CAPS["k_scene_gather"][0] * CAPS["k_scene_gather"][1] // (box * box)     # whole tiles of the first trip
    tile = first_trip + 5
    (t, ky, kx) = (tile // plan.n_tile, tile % plan.n_tile // plan.n_x, tile % plan.n_x)
    (y0, x0) = (scene_ref.origins(Y, box, 0)[ky], scene_ref.origins(X, box, 0)[kx])
    assert t == n_t - 1 and 0 < ky < plan.n_y - 1 and 0 < kx < plan.n_x - 1        # an inner tile: no other box holds the pixel
    var[t, 0, y0 + 7, x0 + 9] = np.nan
    norms = [(280.0, 290.0)]
    (x, invalid) = scene_tiles([var], plan, norms)
    assert tuple(x.shape) == (n_t * plan.n_tile, 1, box, box)
    assert x.cpu().numpy().tobytes() == _packed_on_the_host([var], plan, norms, True).tobytes()
    flags = invalid.cpu().numpy()
    assert np.array_equal(flags, scene_ref.invalid_tiles([var], box, box, 0, 0)) and flags[tile] == 1 and flags.sum() == 1


def test_pack_gather_past_the_cap():
    """4100 destination rows of one channel of 4096 pixels: 16 793 600 elements for 8192 workgroups of 2048.  As bytes against
    importance_ref's arithmetic on the rows gathered in numpy, and against normalise_pack of them"""
    (n_dst, c, hw) = shape = SHAPES["k_normalise_pack_gather"][0][0]
    _past("k_normalise_pack_gather", shape)
    _under("k_normalise_pack_gather", SHAPES["k_normalise_pack_gather"][1][0])
    rng = np.random.default_rng(32)
    n_src = 7
    src = (280.0 + 20.0 * rng.random((n_src, c, hw, 1))).astype(np.float32)
    rows = rng.integers(0, n_src, n_dst).astype(np.int32)
    rows[-1] = n_src - 1                                       # the rows of the second trip come from the last source row
    got = torch.full((n_dst, c + 2, hw, 1), -7.0, dtype=torch.float32, device="cuda")
    pack_gather(torch.from_numpy(src).cuda(), got, 1, torch.from_numpy(rows).cuda(), 280.0, 300.0)
    want = torch.full((n_dst, c + 2, hw, 1), -7.0, dtype=torch.float32, device="cuda")
    normalise_pack(torch.from_numpy(src[rows]).cuda(), want, 1, 280.0, 300.0)
    got = got.cpu().numpy()
    assert got.tobytes() == want.cpu().numpy().tobytes()
    assert got[:, 1:1 + c].tobytes() == importance_ref.normalise(src[rows], 280.0, 300.0).tobytes()
    assert (got[:, 0] == -7.0).all() and (got[:, c + 1] == -7.0).all()


def test_render_cases_past_the_cap():
    """32 769 images of 1 x 3 pixels, four bytes each, in one call: an item an image, 8192 workgroups of 4"""
    (n_sel, h, w) = shape = SHAPES["k_render_cases"][0][0]
    _past("k_render_cases", shape)
    _under("k_render_cases", SHAPES["k_render_cases"][1][0])
    assert case_ops._RENDER_BYTES // (h * (w + 1)) >= n_sel     # the wrapper's group holds the call
    rng = np.random.default_rng(33)
    a = rng.random((n_sel, 1, h, w)).astype(np.float32)
    a.reshape(-1)[rng.integers(0, a.size, 100)] = np.nan
    a[n_sel - 1, 0, 0] = [0.125, np.nan, 0.9]                   # the image of the second trip: the lowest level, NaN, the highest
    got = render_cases(a, 0.125, 0.9)
    want = np_scanlines(np_values(a), 0.125, 0.9)
    assert got.shape == (n_sel, h, w + 1) and np.array_equal(got, want) and list(got[n_sel - 1, 0]) == [0, 1, 0, 255]


def test_neighbours_validity_past_the_cap():
    """k_nb_valid, a wave a row, 8192 workgroups of 4: 32 769 queries against one reference, and one query against 32 769
    references.  Row 32 768, the one of the second trip, is invalid in one call and the valid one beside an invalid row
    in the next: a flag that was never written could pass one of the two by what the workspace happened to hold, not both"""
    _past("k_nb_valid", SHAPES["k_nb_valid"][0][0])
    _under("k_nb_valid", SHAPES["k_nb_valid"][1][0])
    n = SHAPES["k_nb_valid"][0][0][0]
    rng = np.random.default_rng(34)
    for bad in (n - 1, n - 2):
        (q, r) = (grid_rows(rng, n, 1), grid_rows(rng, 1, 1))
        q[bad] = np.nan
        got = case_neighbours(q, r, 1)
        same_neighbours(got, neighbours_ref.neighbours(q, r, 1))
        assert got[2][bad] == -1 and got[2].sum() == n - 2
    # all references invalid but row 5, and in the second call row 32 768 as well
    for last in (np.inf, 2.0):
        (q, r) = (np.zeros((1, 1), dtype=np.float32), np.full((n, 1), np.inf, dtype=np.float32))
        r[5] = 1.0
        r[n - 1] = last
        got = case_neighbours(q, r, 2)
        same_neighbours(got, neighbours_ref.neighbours(q, r, 2))
        assert got[2][0] == (1 if last == np.inf else 2) and got[1][0, 0] == 5


# ---- the folds the issue leaves to the time they take ----------------------------------------------------------------------

def test_pixel_fold_past_the_cap():
    """k_pixel_fold adds the chunks' partials of nine sums a pixel, 8192 workgroups of 256: three cases of 233 017 pixels in
    chunks of one case.  Operands and shift on the dyadic grid: skill_maps_ref's terms added over the cases, compared with =="""
    (n, plane) = shape = SHAPES["k_pixel_fold"][0][0]
    _past("k_pixel_fold", shape)
    _under("k_pixel_fold", SHAPES["k_pixel_fold"][1][0])
    assert int(_lib.load().cae_pixel_sums_workspace_bytes(n, plane, 1)) == n * 9 * plane * 8        # a partial per case: folded
    rng = np.random.default_rng(41)
    (p, a) = (_dyadic(rng, (n, 1, 1, plane)), _dyadic(rng, (n, 1, 1, plane), np.float64))
    p.reshape(-1)[rng.integers(0, p.size, 50)] = np.nan
    a[1, 0, 0, -1] = np.inf                                     # the last pixel, the one of the second trip, has two pairs
    got = pixel_sums(p, a, 7.25, 1)
    t = skill_maps_ref.terms(p[:, 0], a[:, 0], 7.25)
    _assert_exact(n, *t[1:])
    want = t.sum(axis=1)
    assert got.shape == want.shape == (9, 1, plane) and got.dtype == np.float64
    assert np.array_equal(got, want) and got[0, 0, -1] == 2 and got[0].min() >= 1


def test_baseline_fold_past_the_cap():
    """k_baseline_fold, 4096 workgroups of 256 over six sums a case: 174 763 cases of 1 x 1 pixel against 1 x 1.  The
    module's own reference and bounds (a sum of one term)"""
    (n,) = shape = SHAPES["k_baseline_fold"][0][0]
    _past("k_baseline_fold", shape)
    _under("k_baseline_fold", SHAPES["k_baseline_fold"][1][0])
    rng = np.random.default_rng(42)
    low = 280.0 + 10.0 * rng.random((n, 1, 1, 1))
    a = low + rng.standard_normal(low.shape)
    p = a + 0.5 * rng.standard_normal(low.shape)
    for x in (low, a, p):
        x.reshape(-1)[rng.integers(0, n - 1, 30)] = np.nan
    got = case_baseline(low, p, a, mode="bilinear")
    ref = baseline_ref.Reference(low[:, 0], p[:, 0], a[:, 0], "bilinear")
    ref.check(got, f"fold past the cap, {n} cases")
    assert got[n - 1, 0] == 1 and 0 < got[:, 5].sum() < got[:, 0].sum() < n
