"""cae_case_fss on the GPU through engine.fraction_skill, against the numpy restatement of the definition (fss_ref.py): all six
integers of every (case, threshold, width) with np.array_equal - there is no tolerance anywhere, every sum is an integer -
for planes around the word and row boundaries (130 x 193: a 129-wide window starts at every bit offset and crosses three
word boundaries), neighbourhood widths 1 to 129 with widths larger than a side, 1 to 17 cases, 1 to 8 thresholds of mixed
sides, both gap rules, smooth, noisy and constant fields, values on a threshold, -0.0, +-1e300, values that are not finite
sprinkled and as a whole row and column, a case without a pair, a second channel, every element kind, misaligned case
starts, a call cut into case groups; two runs byte for byte, outputs overwritten whole, empty and refused calls; then
train_cae -> fss with the files it writes.  Every smooth and noise check first asserts that the restatement itself has
S cM cO > 0 and S cM^2 != S cO^2 somewhere, so none passes on zeros, and every check holds the identities of the definition
on the GPU's own output."""
import ctypes as C
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from cae_tools_amd import _lib, case_ops
from cae_tools_amd.engine import device_operand, fraction_skill
from cae_tools_amd.utils import fss as fss_scores
from fss_ref import contingency, reference, threshold_list

pytestmark = pytest.mark.gpu

ERR_ARG = -1        # CAE_ERR_ARG of include/cae_hip.h
WIDTHS = [1, 3, 63, 65, 127, 129]
# heights from {1, 2, 3, 65, 66, 129, 130}, widths from {1, 63, 64, 65, 127, 128, 129, 130, 193}; with each the number of cases,
# the number of thresholds and the columns the prediction is rolled by
PLANES = [(1, 1, 17, 1, 0), (1, 63, 17, 3, 1), (2, 64, 3, 8, 1), (3, 65, 17, 3, 5), (65, 127, 3, 8, 5), (66, 128, 1, 3, 1),
          (129, 129, 3, 1, 5), (130, 130, 1, 8, 5), (130, 193, 3, 3, 5), (65, 193, 1, 1, 1), (3, 193, 17, 8, 0), (129, 64, 3, 3, 1)]
SIDES8 = ["below", "above", "above", "below", "above", "above", "below", "above"]


@pytest.fixture(scope="module")
def pattern():
    """17 cases of the datagen circle pattern in [0, 1]: hires (17, 65536), (v - 288) / 10"""
    from cae_tools_amd.data import datagen
    ds = datagen.generate("circle", 17, seed=99)
    return (np.asarray(ds["hires"].values, dtype=np.float64)[:, 0].reshape(17, -1) - 288.0) / 10.0


def _pair(pattern, rng, n, h, w, roll=1):
    """target: h * w consecutive pixels across the ring of n pattern cases; prediction: the target rolled by `roll` columns,
    with small noise"""
    a = pattern[:n, 100 * 256:100 * 256 + h * w].reshape(n, h, w).copy()
    p = np.roll(a, roll, axis=2) + 0.01 * rng.standard_normal(a.shape)
    return p, a


def _thresholds(a, n_thr=3):
    """n_thr thresholds of mixed sides: the 0.1, 0.5 and 0.9 quantiles of the finite target values of this very input for three
    (below, above, above), the 0.1 .. 0.9 quantiles in equal steps otherwise"""
    finite = a[np.isfinite(a)]
    levels = [0.1, 0.5, 0.9] if n_thr == 3 else [0.5] if n_thr == 1 else list(np.linspace(0.1, 0.9, n_thr))
    sides = SIDES8[:n_thr] if n_thr > 1 else ["above"]
    return [(float(np.quantile(finite, q)), side) for (q, side) in zip(levels, sides)]


def _nchw(x, channels=1, dtype=np.float64, channel=0):
    """(N, h, w) values as channel `channel` of an (N, C, h, w) array whose other channels are NaN"""
    out = np.full((x.shape[0], channels) + x.shape[1:], np.nan, dtype=dtype)
    out[:, channel] = x
    return out


def _sprinkle(rng, x, values):
    flat = x.reshape(-1)
    for v in values:
        flat[int(rng.integers(flat.size))] = v
    return x


def _identities(label, got, p, a, thresholds, widths, gaps):
    """the identities of the definition on the GPU's own output"""
    (h, w) = p.shape[1:]
    for (t, (value, side)) in enumerate(threshold_list(thresholds)):
        for (s, n) in enumerate(widths):
            if n == 1 and gaps == "strict":
                for c in range(p.shape[0]):
                    (pairs, hits, misses, alarms) = contingency(p[c:c + 1], a[c:c + 1], value, side)
                    assert got[c, t, s].tolist() == [pairs, hits + alarms, hits + misses, hits + alarms, hits + misses, hits], label
            if n == h == w:
                one = got[:, t, s]
                assert ((one[:, 0] == 0) | (one[:, 0] == 1)).all(), label
                assert (one[:, 3] == one[:, 1] ** 2).all() and (one[:, 4] == one[:, 2] ** 2).all() and (one[:, 5] == one[:, 1] * one[:, 2]).all()
            if n > min(h, w):
                assert not got[:, t, s].any(), label


def _check(label, p, a, thresholds, widths=WIDTHS, gaps="strict", ops=None, nonzero=True):
    """engine.fraction_skill against the restatement, integer for integer; returns (got, ref)"""
    ref = reference(p, a, thresholds, widths, gaps)
    if nonzero:         # the restatement itself: no check passes on zeros
        assert (ref[..., 5] > 0).any() and (ref[..., 3] != ref[..., 4]).any(), label
    (pd, ad) = ops if ops is not None else (_nchw(p), _nchw(a))
    got = fraction_skill(pd, ad, thresholds, widths=widths, gaps=gaps)
    assert got.dtype == np.int64 and got.shape == (p.shape[0], len(thresholds), len(widths), 6), label
    print(f"{label}: {int(ref[..., 0].sum())} windows, S cM cO = {int(ref[..., 5].sum())}, "
          f"{int((got != ref).sum())} of {ref.size} integers differ")
    assert np.array_equal(got, ref), label
    _identities(label, got, p, a, thresholds, widths, gaps)
    return got, ref


# ---- planes, widths, cases, thresholds, gap rules -------------------------------------------------

@pytest.mark.parametrize("shape", PLANES, ids=str)
def test_planes_around_the_word_and_row_boundaries(pattern, shape):
    (h, w, n, n_thr, roll) = shape
    rng = np.random.default_rng(h * 1000 + w)
    (p, a) = _pair(pattern, rng, n, h, w, roll)
    thresholds = _thresholds(a, n_thr)
    big = h * w >= 64
    (got, ref) = _check(f"{h} x {w} strict", p, a, thresholds)
    assert np.array_equal(fraction_skill(_nchw(p), _nchw(a), thresholds, widths=WIDTHS, gaps="ignore"), got)    # every pixel a pair
    if big:             # a few gaps, so that the two rules part
        _sprinkle(rng, p, [np.nan, np.inf])
        _sprinkle(rng, a, [np.nan, -np.inf])
        ignore = _check(f"{h} x {w} ignore", p, a, thresholds, gaps="ignore")[0]
        strict = _check(f"{h} x {w} strict with gaps", p, a, thresholds, nonzero=False)[0]
        # at width 1 a window is a pixel and both rules count the pairs; from width 3 on the ignore rule keeps more
        assert (ignore[..., 0] >= strict[..., 0]).all() and np.array_equal(ignore[:, :, 0], strict[:, :, 0])
        assert min(h, w) < 3 or (ignore[..., 0] > strict[..., 0]).any()


def test_default_widths_and_plain_thresholds(pattern):
    rng = np.random.default_rng(2)
    (p, a) = _pair(pattern, rng, 3, 40, 70, 5)
    t = [float(np.quantile(a, 0.9)), float(np.quantile(a, 0.5))]
    got = fraction_skill(_nchw(p), _nchw(a), t)
    assert got.shape == (3, 2, 6, 6) and np.array_equal(got, reference(p, a, t, [1, 3, 5, 9, 17, 33]))
    scores = fss_scores.scores_from_sums(got, [1, 3, 5, 9, 17, 33])
    assert all(b >= a for (a, b) in zip(scores["fss"][0], scores["fss"][0][1:]))       # a displacement: skill grows with the width
    same = fraction_skill(_nchw(a), _nchw(a), t)
    perfect = fss_scores.scores_from_sums(same, [1, 3, 5, 9, 17, 33])["case_fss"]
    assert ((perfect == 1.0) | np.isnan(perfect)).all() and (perfect == 1.0).any()      # exactly 1 wherever it is defined


def test_noise_and_a_constant_field():
    rng = np.random.default_rng(3)
    (p, a) = (rng.random((3, 66, 130)), rng.random((3, 66, 130)))
    for gaps in ("strict", "ignore"):
        _check(f"noise {gaps}", p, a, _thresholds(a), gaps=gaps)
    c = np.full((3, 66, 130), 0.25)
    for (thresholds, events) in (([0.25], 1), ([(0.25, "below")], 0), ([0.5, (0.5, "below")], None)):
        (got, ref) = _check(f"constant {thresholds}", c, c, thresholds, nonzero=False)
        if events is not None:          # every window is full of events, or empty
            assert (got[:, 0, 1] == np.array([64 * 128, 9 * 64 * 128, 9 * 64 * 128, 81 * 64 * 128, 81 * 64 * 128, 81 * 64 * 128])
                    * np.array([1, events, events, events, events, events])).all()


# ---- special values ----------------------------------------------------------------------------------

def test_values_on_a_threshold_signed_zero_and_huge_values():
    rng = np.random.default_rng(5)
    grid = rng.integers(-2, 3, size=(3, 20, 70)) / 4.0          # many values exactly on -0.5, 0.0 and 0.5
    (p, a) = (grid.copy(), np.roll(grid, 1, axis=2))
    p[0, :, ::3] = -0.0
    a[1, ::2, :] = -0.0
    _sprinkle(rng, p, [1e300, -1e300, 1e300])
    _sprinkle(rng, a, [-1e300, 1e300])
    thresholds = [0.0, (0.0, "below"), (-0.0, "above"), 0.5, (-0.5, "below"), (1e300, "above"), (-1e300, "below")]
    for gaps in ("strict", "ignore"):
        (got, ref) = _check(f"on the thresholds {gaps}", p, a, thresholds, widths=[1, 3, 5, 19], gaps=gaps)
        assert np.array_equal(got[:, 0], got[:, 2])             # -0.0 compares as 0.0, as a threshold too
        assert got[:, 5, 0, 2].sum() == int((a >= 1e300).sum()) > 0 and got[:, 6, 0, 1:].sum() == 0     # nothing is below -1e300
        # above and below 0.0 part the pairs
        assert np.array_equal(got[:, 0, 0, 1] + got[:, 1, 0, 1], got[:, 0, 0, 0])


def test_values_that_are_not_finite(pattern):
    rng = np.random.default_rng(7)
    (p, a) = _pair(pattern, rng, 3, 66, 130, 5)
    thresholds = _thresholds(a)
    _sprinkle(rng, p, [np.nan, np.inf, -np.inf, np.nan])
    _sprinkle(rng, a, [np.nan, np.inf, -np.inf])
    for gaps in ("strict", "ignore"):
        _check(f"sprinkled {gaps}", p, a, thresholds, gaps=gaps)
    # a whole row and a whole column of gaps, in either operand
    (p, a) = _pair(pattern, rng, 3, 40, 70, 1)
    thresholds = _thresholds(a)
    p[:, 3, :] = np.nan
    a[:, :, 3] = np.inf
    widths = [1, 5, 9]
    strict = _check("row and column strict", p, a, thresholds, widths=widths)[0]
    ignore = _check("row and column ignore", p, a, thresholds, widths=widths, gaps="ignore")[0]
    # strict: a window of width 5 fits only below the row and right of the column; ignore: every window holds a pair
    assert (strict[:, :, 1, 0] == (40 - 5 + 1 - 4) * (70 - 5 + 1 - 4)).all() and (ignore[:, :, 1, 0] == 36 * 66).all()
    assert (strict[:, :, 0, 0] == 39 * 69).all() and (ignore[:, :, 0, 0] == 39 * 69).all()


def test_a_case_without_a_pair_and_a_second_channel(pattern):
    rng = np.random.default_rng(9)
    (p, a) = _pair(pattern, rng, 3, 33, 65, 1)
    thresholds = _thresholds(a)
    p[1] = np.nan
    a[1, ::2] = np.inf
    for gaps in ("strict", "ignore"):
        (got, ref) = _check(f"no pair {gaps}", p, a, thresholds, widths=[1, 3, 33], gaps=gaps)
        assert not got[1].any() and got[0].any() and got[2].any()
    (p, a) = _pair(pattern, rng, 3, 33, 65, 1)
    ops = (device_operand(_nchw(p, 2)), device_operand(_nchw(a, 3)))        # case strides of two and three planes
    _check("a second channel", p, a, thresholds, widths=[1, 3, 33], ops=ops)


@pytest.mark.parametrize("kinds", [(kp, ka) for kp in ("f4", ">f4", "f8", ">f8") for ka in ("f4", ">f4", "f8", ">f8")], ids=str)
def test_element_kinds(pattern, kinds):
    (n, h, w) = (3, 17, 131)
    rng = np.random.default_rng(23)
    (p, a) = _pair(pattern, rng, n, h, w, 5)
    for x in (p, a):
        _sprinkle(rng, x, [np.nan, np.inf, 1e300, -0.0])
    with np.errstate(over="ignore"):        # 1e300 is Inf in fp32
        arrays = [_nchw(x, 2, np.dtype(k)) for (x, k) in zip((p, a), kinds)]
    ops = [device_operand(x) for x in arrays]
    want = {"f4": _lib.ELEM_F32, "f8": _lib.ELEM_F64, ">f4": _lib.ELEM_F32_BE, ">f8": _lib.ELEM_F64_BE}
    assert [op.kind for op in ops] == [want[k] for k in kinds]
    stored = [np.asarray(x[:, 0], dtype=np.float64) for x in arrays]
    finite = stored[1][np.isfinite(stored[1])]
    thresholds = [(float(np.quantile(finite, 0.1)), "below"), float(np.quantile(finite, 0.5)), float(np.quantile(finite, 0.9))]
    _check(f"kinds {kinds}", *stored, thresholds, widths=[1, 3, 17, 65], gaps="ignore", ops=ops)


@pytest.mark.parametrize("offsets", [(1, 1), (1, 3), (2, 0), (3, 2)], ids=str)
def test_misaligned_device_tensors(pattern, offsets):
    """fp32 tensors that start 4, 8 or 12 bytes after a 16-byte boundary, two channels: the case stride is twice the plane"""
    (n, h, w) = (5, 3, 193)
    rng = np.random.default_rng(29)
    (p, a) = _pair(pattern, rng, n, h, w, 5)
    tensors = []
    for (x, off) in zip((p, a), offsets):
        x4 = _nchw(x, 2, np.float32)
        flat = torch.empty(x4.size + off, dtype=torch.float32, device="cuda")
        flat[off:] = torch.from_numpy(x4.reshape(-1)).cuda()
        t = flat[off:].view(x4.shape)
        assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
        tensors.append(t)
    stored = [np.asarray(x, dtype=np.float32).astype(np.float64) for x in (p, a)]
    _check(f"offsets {offsets}", *stored, _thresholds(stored[1]), widths=[1, 3, 65, 129], ops=[device_operand(t) for t in tensors])


def test_a_call_cut_into_case_groups(pattern, monkeypatch):
    (n, h, w) = (17, 20, 70)
    rng = np.random.default_rng(11)
    (p, a) = _pair(pattern, rng, n, h, w, 5)
    thresholds = _thresholds(a)
    uncut = _check("uncut", p, a, thresholds, widths=[1, 3, 19])[0]
    per_case = int(_lib.load().cae_case_fss_workspace_bytes(1, h, w, 3))
    assert per_case == 7 * 20 * 2 * 8
    monkeypatch.setattr(case_ops, "_FSS_PLANE_BYTES", 3 * per_case + 8)     # groups of three cases: six calls, the last of two
    cut = fraction_skill(_nchw(p), _nchw(a), thresholds, widths=[1, 3, 19])
    monkeypatch.setattr(case_ops, "_FSS_PLANE_BYTES", 1)                    # one case a call
    single = fraction_skill(_nchw(p), _nchw(a), thresholds, widths=[1, 3, 19])
    assert np.array_equal(cut, uncut) and np.array_equal(single, uncut)


def test_segments_of_window_rows(pattern):
    """one case of 256 x 256: the walk is cut into segments of 64 window rows (four at width 1, one and a rest at 129), whose
    sums the atomics add"""
    rng = np.random.default_rng(13)
    a = pattern[:1].reshape(1, 256, 256).copy()
    p = np.roll(a, 9, axis=2) + 0.01 * rng.standard_normal(a.shape)
    _sprinkle(rng, p, [np.nan, np.nan])
    for gaps in ("strict", "ignore"):
        _check(f"256 x 256 {gaps}", p, a, _thresholds(a), widths=[1, 9, 65, 129], gaps=gaps)


# ---- the call itself ---------------------------------------------------------------------------------------

def _raw(p, a, n, h, w, thresholds, widths, gap_rule=0, fill=0x5A, change=()):
    """cae_case_fss itself on an output filled with garbage; returns (code, sums) as numpy"""
    change = dict(change)
    lib = _lib.load()
    dev = p.tensor.device
    pairs = threshold_list(thresholds)
    (n_thr, n_width) = (len(pairs), len(widths))
    sums = torch.full((max(n, 1), n_thr, n_width, 6), fill, dtype=torch.int64, device=dev)
    need = int(lib.cae_case_fss_workspace_bytes(n, h, w, n_thr))
    ws = torch.full((max(need, 1 << 16),), 0xFF, dtype=torch.uint8, device=dev)    # set bits: a word read before it is written shows
    thr = (C.c_double * n_thr)(*[v for (v, _) in pairs])
    side = (C.c_int * n_thr)(*[change.pop("side", 1 if s == "below" else 0) for (_, s) in pairs])
    wid = (C.c_int * n_width)(*widths)
    args = dict(n=n, h=h, w=w, n_thr=n_thr, n_width=n_width, gap_rule=gap_rule, bytes=max(need, 1 << 16))
    args.update(change)
    rc = lib.cae_case_fss(*p.args(), *a.args(), args["n"], args["h"], args["w"], thr, side, args["n_thr"], wid, args["n_width"],
                          args["gap_rule"], sums.data_ptr(), ws.data_ptr(), args["bytes"], torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc, sums.cpu().numpy()


def test_two_runs_garbage_empty_and_refused_calls(pattern):
    (n, h, w) = (17, 20, 130)
    rng = np.random.default_rng(31)
    (p, a) = _pair(pattern, rng, n, h, w, 5)
    for x in (p, a):
        _sprinkle(rng, x, [np.nan, np.inf, -np.inf])
    thresholds = _thresholds(a)
    widths = [1, 3, 19, 65]
    (pd, ad) = (device_operand(_nchw(p)), device_operand(_nchw(a)))
    first = _raw(pd, ad, n, h, w, thresholds, widths, gap_rule=1)
    second = _raw(pd, ad, n, h, w, thresholds, widths, gap_rule=1, fill=0x33)
    assert first[0] == 0 and second[0] == 0
    assert first[1].tobytes() == second[1].tobytes()            # whatever the buffers held
    ref = reference(p, a, thresholds, widths, "ignore")
    assert (ref[..., 5] > 0).any() and (ref[..., 3] != ref[..., 4]).any()
    assert np.array_equal(first[1], ref)
    assert np.array_equal(fraction_skill(pd, ad, thresholds, widths=widths, gaps="ignore"), ref)
    # no case: nothing is written; no pixel: zeros over the garbage
    assert _raw(pd, ad, n, h, w, thresholds, widths, change=dict(n=0))[0] == 0
    for change in (dict(h=0), dict(w=0), dict(h=0, w=0)):
        empty = _raw(pd, ad, n, h, w, thresholds, widths, change=change)
        assert empty[0] == 0 and not empty[1].any(), change
    assert fraction_skill(np.zeros((0, 1, 4, 4)), np.zeros((0, 2, 4, 4)), [0.5]).shape == (0, 1, 2, 6)
    assert fraction_skill(np.zeros((3, 1, 0, 5)), np.zeros((3, 1, 0, 5)), [0.5, 0.7]).shape == (3, 2, 0, 6)
    assert not fraction_skill(np.zeros((3, 1, 0, 5)), np.zeros((3, 1, 0, 5)), [0.5], widths=[1, 3]).any()
    # a refused call writes nothing
    lib = _lib.load()
    for (thr, wid, kw) in ((thresholds, widths, dict(n_thr=0)), (thresholds, widths, dict(n_thr=9)), (thresholds, widths, dict(n_width=9)),
                           (thresholds, widths, dict(gap_rule=2)), (thresholds, widths, dict(h=16385)), (thresholds, widths, dict(side=2)),
                           ([float("nan")], widths, {}), ([float("inf")], widths, {}), (thresholds, [2], {}), (thresholds, [3, 1], {}),
                           (thresholds, [131], {}), (thresholds, [0], {}), (thresholds, widths, dict(bytes=8)),
                           (thresholds, widths, dict(w=131))):
        refused = _raw(pd, ad, n, h, w, thr, wid, fill=5, change=kw)
        assert refused[0] == ERR_ARG and lib.cae_last_error().decode().startswith("cae_case_fss: "), (thr, wid, kw)
        assert (refused[1] == 5).all(), (thr, wid, kw)


def test_argument_errors_name_the_function():
    (x, y) = (np.zeros((2, 1, 4, 4), dtype=np.float32), np.zeros((2, 1, 4, 5), dtype=np.float32))
    for (args, kw) in (((x, y, [0.5]), {}), ((x, x[0], [0.5]), {}), ((x, x, []), {}), ((x, x, [0.0] * 9), {}), ((x, x, [float("nan")]), {}),
                       ((x, x, [(0.5, "over")]), {}), ((x, x, [0.5]), dict(widths=[2])), ((x, x, [0.5]), dict(widths=[3, 1])),
                       ((x, x, [0.5]), dict(widths=[131])), ((x, x, [0.5]), dict(widths=[])), ((x, x, [0.5]), dict(gaps="lenient")),
                       ((x, x, [0.5]), dict(gaps=None))):
        with pytest.raises(ValueError, match="fraction_skill: "):
            fraction_skill(*args, **kw)


# ---- train_cae -> fss --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 circle cases per partition, the smallest set datagen makes"""
    from cae_tools_amd.data import datagen
    root = tmp_path_factory.mktemp("fss")
    paths = {}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        paths[part] = str(root / f"{part}.nc")
        datagen.generate("circle", 12, seed=seed).to_netcdf(paths[part])
    return root, paths


def test_train_fss(data):
    from cae_tools_amd.cli import fss as cli, train_cae
    from cae_tools_amd.data.arrays import open_mfdataset
    (root, paths) = data
    model = str(root / "model")
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                        "--input-variables", "lowres", "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"])
    out = str(root / "report")
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["--test-inputs", paths["test"], "--model-folder", model, "--output-html-folder", out, "--fss-percentiles", "<5", "90",
                  "--fss-widths", "1", "9", "129", "--fss-gaps", "ignore"])
    assert sorted(f for f in os.listdir(out) if f.startswith("fss")) == ["fss", "fss_test.json"]
    with open(os.path.join(out, "fss_test.json")) as f:
        rec = json.load(f, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert (rec["widths"], rec["gaps"], rec["h"], rec["w"], rec["n_cases"]) == ([1, 9, 129], "ignore", 256, 256, 12)
    assert [(t["side"], t["percentile"], t["label"]) for t in rec["thresholds"]] == [("below", 0.05, "<q5"), ("above", 0.9, ">=q90")]
    # the values are percentiles of the target (the pattern holds many equal values, so an event's frequency need not be the
    # percentile's): the events counted at width 1 are the target's under the values in the file
    target = np.asarray(open_mfdataset([paths["test"]])["hires"].values, dtype=np.float64)[:, 0]
    assert 0.0 < rec["f_target"][0][0] < 0.2 and 0.0 < rec["f_target"][1][0] < 0.3 and rec["thresholds"][0]["value"] < rec["thresholds"][1]["value"]
    assert rec["pooled_sums"][0][0][0] == 12 * 256 * 256 and rec["pooled_sums"][0][2][0] == 12 * 128 * 128
    for (t, thr) in enumerate(rec["thresholds"]):
        event = target < thr["value"] if thr["side"] == "below" else target >= thr["value"]
        assert rec["pooled_sums"][t][0][2] == int(event.sum())          # S cO at width 1: the target's events
    assert np.asarray(rec["case_fss"], dtype=object).shape == (12, 2, 3)
    lines = [ln for ln in log.getvalue().splitlines() if ln.startswith("fss ")]
    assert lines == [fss_scores.line("test", rec)] and lines[0].startswith("fss test: 12 cases, widths 1..129 (ignore), skilful width <q5 ")
    with open(os.path.join(out, "index.html")) as f:
        page = f.read()
    assert page.count("<h2>Neighbourhood skill</h2>") == 1 and page.count('href="fss/index.html"') == 1
    assert "test: 2 thresholds, widths 1, 9, 129, 12 cases, gaps ignore" in page
    with open(os.path.join(out, "fss", "index.html")) as f:
        curves = f.read()
    assert curves.count('alt="test fss ') == 2 and "test: 12 cases of 256 x 256, gaps ignore" in curves
