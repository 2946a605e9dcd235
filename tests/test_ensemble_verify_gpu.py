"""cae_ensemble_verify (include/cae_hip.h) through ctypes on synthetic fp32 draws, against the fp64 numpy definition of
tests/ensemble_verify_ref.py (all pairs, no sort), with members vmin + y * range, vmin = 288.0, range = 10.5.

Integers are exact: the rank counts, the tie count and n per case equal the definition's.  The four sums are held to
c * 2^-53 * S|terms|, c the number of additions that enter the output: the terms are non-negative and formed from the
same members by the same operations as the definition's, so what differs is the order of at most c additions, and each
addition's rounding error is at most 2^-53 of a partial sum that never exceeds S|terms|.  c is plane * K for S A,
plane * K (K - 1) / 2 for S B, plane * (K + 3) for S (mbar - a)^2 and plane * (2 K + 3) for S s^2 (a derived worst-case
bound, not a measured one; the observed errors are printed beside it).

Every pixel class is in every case whose plane has room for it (pixel p has class p % 8): target below all members, above
all, strictly inside at spreads 0.3 and 1e-3, a spread of one fp32 ulp, all members equal, a NaN target, one NaN draw."""
import numpy as np
import pytest
import torch

import ensemble_verify_ref as ref

pytestmark = pytest.mark.gpu

VMIN, RANGE = 288.0, 10.5
GUARD = 64                  # bytes of 0xAA on both sides of every output and of the workspace
CLASSES = 8
F32, F32_BE, F64 = 0, 1, 2
U = 2.0 ** -53


def _case_data(n_case, k, plane, seed):
    """(y (n_case, k, plane) fp32, target (n_case, plane) fp64) with the pixel classes of the module docstring"""
    rng = np.random.default_rng(seed)
    cls = np.arange(plane) % CLASSES
    spread = np.select([cls == 0, cls == 1, cls == 2, cls == 3, cls == 4, cls == 5], [0.3, 1e-3, 0.3, 1e-3, 6e-8, 0.0], 0.05)
    base = 0.25 + 0.5 * rng.random((n_case, 1, plane))
    y = (base + spread * rng.standard_normal((n_case, k, plane))).astype(np.float32)
    m = ref.members(y, VMIN, RANGE)
    (lo, hi) = (m.min(axis=1), m.max(axis=1))
    a = 0.5 * (lo + hi) + 0.25 * (hi - lo) * (rng.random((n_case, plane)) - 0.5)
    a = np.where(cls == 0, lo - 0.5 - rng.random((n_case, plane)), a)
    a = np.where(cls == 1, hi + 0.5 + rng.random((n_case, plane)), a)
    a = np.where(cls == 5, lo + 0.125, a)
    a = np.where(cls == 6, np.nan, a)
    nan_draw = rng.integers(0, k, size=(n_case, plane))
    for c in range(n_case):
        cols = np.nonzero(cls == 7)[0]
        y[c, nan_draw[c, cols], cols] = np.nan
    return y, a


def _place_draws(y, offset, layout, padded):
    """the draws on the device in [case][draw] or [draw][case] order, planes tight or on a pitch that is a multiple of 4
    floats, the whole shifted by `offset` floats from a 16-byte boundary: (holder, pointer, case_stride, draw_stride)"""
    (n_case, k, plane) = y.shape
    pitch = (plane + 3) // 4 * 4 + 4 if padded else plane
    rows = y if layout == "case" else y.transpose(1, 0, 2)
    host = np.full((rows.shape[0], rows.shape[1], pitch), np.float32(np.inf))
    host[:, :, :plane] = rows
    dev = torch.empty(host.size + offset, dtype=torch.float32, device="cuda")
    dev[offset:] = torch.from_numpy(host.reshape(-1)).cuda()
    (case_stride, draw_stride) = (k * pitch, pitch) if layout == "case" else (pitch, n_case * pitch)
    return dev, dev.data_ptr() + 4 * offset, case_stride, draw_stride


def _stored(a, kind):
    """the target as its kind stores it, back in float64"""
    return a.astype(np.float32).astype(np.float64) if kind in (F32, F32_BE) else a.astype(np.float64)


def _place_target(a, kind, stride, offset):
    """the target of kind `kind` on the device, case c at element offset + c * stride: (holder, pointer)"""
    (n_case, plane) = a.shape
    dtype = {F32: "<f4", F32_BE: ">f4", F64: "<f8"}[kind]
    host = np.full(offset + n_case * stride, 7.0, dtype=dtype)
    for c in range(n_case):
        host[offset + c * stride:offset + c * stride + plane] = a[c]
    dev = torch.from_numpy(host.view(np.uint8).copy()).cuda()
    return dev, dev.data_ptr() + offset * host.itemsize


class _Guarded:
    """nbytes of device memory between two runs of 0xAA bytes, `fill` (a byte) inside"""

    def __init__(self, nbytes, fill):
        self.nbytes = nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        self.raw[GUARD:GUARD + nbytes] = fill
        self.ptr = self.raw.data_ptr() + GUARD

    def read(self, dtype):
        host = self.raw.cpu().numpy()
        assert (host[:GUARD] == 0xAA).all() and (host[GUARD + self.nbytes:] == 0xAA).all(), "a guard value was overwritten"
        return host[GUARD:GUARD + self.nbytes].view(dtype).copy()


def _run(y, a, kind=F32, offset=0, layout="draw", padded=False, a_stride=None, a_offset=0, ranks=None, vmin=VMIN, rng=RANGE):
    """(case_sums (n_case, 5), rank_counts (K + 2,)) of one call; `ranks`: a _Guarded to add into (None: a zeroed one)"""
    from cae_tools_amd import _lib
    lib = _lib.load()
    (n_case, k, plane) = y.shape
    (keep_y, yp, case_stride, draw_stride) = _place_draws(y, offset, layout, padded)
    (keep_a, ap) = _place_target(a, kind, a_stride or plane, a_offset)
    sums = _Guarded(n_case * 5 * 8, 0xAA)
    ranks = ranks or _Guarded((k + 2) * 8, 0)
    need = int(lib.cae_ensemble_verify_workspace_bytes(n_case, plane, k))
    assert need >= (k + 2) * 8
    ws = _Guarded(need, 0xAA)
    _lib.check(lib.cae_ensemble_verify(yp, case_stride, draw_stride, ap, kind, a_stride or plane, n_case, plane, k, vmin, rng,
                                       sums.ptr, ranks.ptr, ws.ptr, need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ws.read(np.uint8)
    del keep_y, keep_a
    return sums.read(np.float64).reshape(n_case, 5), ranks.read(np.int64)


def _check(got, want, k, what):
    """got: the kernel's (sums, ranks); want: ensemble_verify_ref.verify's (sums, ranks, terms)"""
    ((sums, ranks), (ref_sums, ref_ranks, terms)) = (got, want)
    plane = terms[0]["counted"].size
    assert np.array_equal(ranks, ref_ranks), f"{what}: rank counts {ranks} != {ref_ranks}"
    assert np.array_equal(sums[:, 0], ref_sums[:, 0]), f"{what}: n per case {sums[:, 0]} != {ref_sums[:, 0]}"
    adds = (plane * k, plane * k * (k - 1) // 2, plane * (k + 3), plane * (2 * k + 3))
    for c in range(sums.shape[0]):
        w = terms[c]["counted"]
        for (q, name) in enumerate("ABEV"):
            total = float(np.abs(terms[c][name][w]).sum())
            bound = adds[q] * U * total
            err = abs(sums[c, 1 + q] - ref_sums[c, 1 + q])
            print(f"{what} case {c} S{name}: error {err:.3e}, bound {bound:.3e} ({adds[q]} additions, S|terms| {total:.6e})")
            assert err <= bound, f"{what} case {c} S{name}: error {err:.3e} above {bound:.3e}"


# offset of the draws in floats, their order, padded pitch; target kind, extra elements on its case stride, its offset
PLACEMENTS = ((0, "draw", False, F32, 0, 0), (1, "draw", False, F64, 1, 1), (0, "case", True, F32_BE, 3, 1),
              (1, "case", True, F64, 0, 0))


@pytest.mark.parametrize("n_case", [1, 3])
@pytest.mark.parametrize("k", [2, 3, 17, 64])
@pytest.mark.parametrize("plane", [1, 3, 35, 4099])
def test_sums_and_ranks_match_the_definition(plane, k, n_case):
    (y, a) = _case_data(n_case, k, plane, seed=plane * 131 + k * 7 + n_case)
    want = {wide: ref.verify(y, _stored(a, F64 if wide else F32), VMIN, RANGE) for wide in (False, True)}
    if plane >= CLASSES:
        (sums, ranks, terms) = want[True]
        skipped = (np.arange(plane) % CLASSES >= 6).sum()
        assert (sums[:, 0] == plane - skipped).all() and ranks[0] > 0 and ranks[k] > 0 and ranks[1:k].sum() > 0
    for (offset, layout, padded, kind, extra, a_offset) in PLACEMENTS:
        got = _run(y, _stored(a, kind), kind, offset, layout, padded, a_stride=plane + extra, a_offset=a_offset)
        _check(got, want[kind == F64], k, f"plane {plane} K {k} cases {n_case} offset {offset} {layout} kind {kind}")


def test_chunks_of_more_than_one_block():
    """3 cases of 360 007 pixels: the library cuts them into chunks of 128 groups, two 256-pixel blocks per wave item, and folds
    704 chunks per case"""
    (n_case, k, plane) = (3, 3, 360007)
    (y, a) = _case_data(n_case, k, plane, seed=77)
    want = ref.verify(y, _stored(a, F32), VMIN, RANGE)
    for (offset, layout, padded) in ((1, "draw", False), (0, "case", True)):
        _check(_run(y, _stored(a, F32), F32, offset, layout, padded), want, k, f"plane {plane} K {k} offset {offset} {layout}")


def test_skipped_pixels_change_nothing_else():
    """the NaN targets and NaN draws replaced by pixels that are not there at all: the same sums, bit for bit"""
    (y, a) = _case_data(3, 5, 4096, seed=3)
    keep = np.arange(4096) % CLASSES < 6
    (y2, a2) = (y.copy(), a.copy())
    y2[:, :, ~keep] = 0.5
    a2[:, ~keep] = VMIN + 0.5 * RANGE
    (sums, ranks) = _run(y, a, F64)
    (sums2, ranks2) = _run(y2, a2, F64)
    n_skipped = int((~keep).sum())
    assert (sums[:, 0] == keep.sum()).all() and (sums2[:, 0] == 4096).all()
    # the replacement pixels have all members equal to the target: A = B = E = V = 0, rank 0, tied
    assert np.array_equal(sums[:, 1:], sums2[:, 1:])
    assert ranks2[0] == ranks[0] + 3 * n_skipped and np.array_equal(ranks2[1:-1], ranks[1:-1])
    assert ranks2[-1] == ranks[-1] + 3 * n_skipped


@pytest.mark.parametrize("k", [2, 5, 64])
def test_ties_are_counted_at_their_lowest_rank(k):
    """vmin 0, range 1: the members are the fp32 draws themselves, the target is the fp32 value of one chosen member"""
    (n_case, plane) = (2, 777)
    rng = np.random.default_rng(k)
    y = rng.random((n_case, k, plane)).astype(np.float32)
    y[:, :, ::3] = y[:, :1, ::3]                             # every third pixel: all members equal
    y[:, 1, 1::3] = y[:, 0, 1::3]                            # the next: two members equal
    pick = rng.integers(0, k, size=(n_case, plane))
    a = np.take_along_axis(y, pick[:, None, :], axis=1)[:, 0, :]
    want = ref.verify(y, a.astype(np.float64), 0.0, 1.0)
    assert want[1][k + 1] == n_case * plane                  # every pixel is tied
    below = (y < a[:, None, :]).sum(axis=1)
    assert np.array_equal(want[1][:k + 1], np.bincount(below.reshape(-1), minlength=k + 1))
    for kind in (F32, F64):
        got = _run(y, a.astype(np.float64), kind, offset=1, layout="case", padded=True, vmin=0.0, rng=1.0)
        _check(got, want, k, f"ties K {k} kind {kind}")
    # tied pixels with all members equal: A = B = 0 exactly
    (sums, ranks) = _run(y[:, :, ::3].copy(), a[:, ::3].astype(np.float64), F32, vmin=0.0, rng=1.0)
    assert (sums[:, 1:] == 0.0).all() and ranks[0] == ranks[k + 1] == sums[:, 0].sum()


def test_rank_counts_accumulate_across_calls():
    (y, a) = _case_data(3, 9, 4099, seed=21)
    (whole_sums, whole_ranks) = _run(y, a, F64)
    ranks = _Guarded((9 + 2) * 8, 0)
    (s0, _) = _run(y[:2], a[:2], F64, ranks=ranks)
    (s1, both) = _run(y[2:], a[2:], F64, ranks=ranks)
    assert np.array_equal(both, whole_ranks)
    # (calls this small are all cut into 64-group chunks, so the cases' sums are the same bits as well)
    assert np.array_equal(np.concatenate([s0, s1]), whole_sums)


def test_two_runs_are_bitwise_equal():
    (y, a) = _case_data(3, 17, 12301, seed=11)
    for args in ((F32, 1, "case", True), (F64, 0, "draw", False)):
        (r0, r1) = (_run(y, _stored(a, args[0]), *args), _run(y, _stored(a, args[0]), *args))
        assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1])


def test_bad_arguments_are_refused_and_write_nothing():
    from cae_tools_amd import _lib
    lib = _lib.load()
    (n_case, k, plane) = (3, 4, 4099)
    (y, a) = _case_data(n_case, k, plane, seed=2)
    (keep_y, yp, cs, ds) = _place_draws(y, 0, "draw", False)
    (keep_a, ap) = _place_target(a, F64, plane, 0)
    need = int(lib.cae_ensemble_verify_workspace_bytes(n_case, plane, k))
    (sums, ranks, ws) = (_Guarded(n_case * 5 * 8, 0xAA), _Guarded((k + 2) * 8, 0xAA), _Guarded(need, 0xAA))
    good = dict(y=yp, cs=cs, ds=ds, a=ap, kind=F64, a_stride=plane, n=n_case, plane=plane, k=k, vmin=VMIN, rng=RANGE,
                sums=sums.ptr, ranks=ranks.ptr, ws=ws.ptr, ws_bytes=need)

    def call(**change):
        v = dict(good, **change)
        return lib.cae_ensemble_verify(v["y"], v["cs"], v["ds"], v["a"], v["kind"], v["a_stride"], v["n"], v["plane"], v["k"],
                                       v["vmin"], v["rng"], v["sums"], v["ranks"], v["ws"], v["ws_bytes"], None)

    bad = [dict(kind=4), dict(kind=-1), dict(n=-1), dict(plane=-1), dict(k=1), dict(k=65), dict(cs=-plane), dict(ds=-1),
           dict(a_stride=-plane), dict(a_stride=plane - 1), dict(cs=plane - 1), dict(ds=n_case * plane - 1),
           dict(cs=2 ** 62), dict(ds=2 ** 62), dict(cs=2 ** 62, ds=2 ** 62), dict(a_stride=2 ** 62),
           dict(rng=-1.0), dict(rng=float("inf")), dict(rng=float("nan")), dict(vmin=float("nan")), dict(vmin=float("-inf")),
           dict(ws_bytes=need - 8), dict(ws=None), dict(ws=ws.ptr + 4), dict(y=yp + 2), dict(a=ap + 4), dict(sums=sums.ptr + 4),
           dict(ranks=ranks.ptr + 4), dict(y=None), dict(a=None), dict(sums=None), dict(ranks=None)]
    for change in bad:
        assert call(**change) == -1, f"{change} was not refused"           # CAE_ERR_ARG
    torch.cuda.synchronize()
    for g in (sums, ranks, ws):
        assert (g.read(np.uint8) == 0xAA).all()
    # no case or no pixel: accepted, nothing written
    assert call(n=0) == 0 and call(plane=0) == 0
    torch.cuda.synchronize()
    for g in (sums, ranks, ws):
        assert (g.read(np.uint8) == 0xAA).all()
    del keep_y, keep_a


def test_python_wrapper_matches_the_definition():
    from cae_tools_amd import engine as eng
    (n_case, k, h, w) = (3, 6, 13, 17)
    (y, a) = _case_data(n_case, k, h * w, seed=8)
    want = ref.verify(y, a, VMIN, RANGE)
    target = np.stack([a.reshape(n_case, h, w), np.zeros((n_case, h, w))], axis=1)      # channel 1 is ignored
    for (layout, draws) in (("case", y.reshape(n_case, k, h, w)), ("draw", y.transpose(1, 0, 2).reshape(k, n_case, h, w))):
        for d in (draws, torch.from_numpy(np.ascontiguousarray(draws)).cuda()):
            (sums, ranks) = eng.ensemble_verify(d, target, VMIN, VMIN + RANGE, layout=layout)
            _check((sums, ranks), want, k, f"wrapper {layout}")
