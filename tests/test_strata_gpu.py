"""cae_strata_sums on the GPU through engine.strata_sums, against the numpy restatement of the definition (strata_ref.py):
members, pairs and unclassified integer for integer, every sum within c 2^-53 S|x_i| of the math.fsum value - the bound of any
order of summation, derived in distribution_ref.py - for planes around the wave and chunk sizes, 1 to 17 cases, 0 to 63
edges, stratifier grids equal to, coarser and finer than the target's and one value per case, smooth, constant and noisy
fields, values on the edges, -0.0, +-1e300 and values that are not finite in every operand, a second channel, every element
kind, misaligned case starts, a call cut into several workgroups and per-stratum shifts; two runs byte for byte, outputs
overwritten whole, empty and refused calls; then train_cae -> strata with the files it writes.  Every check also holds the
two identities: members + unclassified is the number of pixels, and one stratum over a finite stratifier gives the sums
of pixel_sums added over the pixels.

Largest |got - fsum| / bound measured on an MI355X (each check prints its figure before it asserts): 0.35 over the planes,
cases and simple grids (plane 1 x 1, 3 cases, one value per case), 0.47 over the coarser and finer grids (9 x 9 -> 4 x 4, 63
edges: a pair or two per stratum), 0.050 smooth, 2.8e-4 constant, 0.039 noise, 0.0093 with the special values, 0.0038 on the
second channel, 0.15 over the element kinds, 6.7e-4 with misaligned case starts, 2.8e-4 over nine workgroups, 2.2e-4 about
per-stratum shifts, 2.7e-4 over garbage, 0.34 in the one-stratum calls of the second identity; every count exact."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from cae_tools_amd import _lib
from cae_tools_amd.engine import device_operand, pixel_sums, strata_sums
from cae_tools_amd.utils import strata as strata_scores
from strata_ref import Reference, on_target_grid, strata_of

pytestmark = pytest.mark.gpu

ERR_ARG = -1        # CAE_ERR_ARG of include/cae_hip.h
PLANES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 4099), (33, 65)]
CASES = [1, 3, 17]
N_EDGE = [0, 1, 6, 63]


@pytest.fixture(scope="module")
def pattern():
    """17 cases of the datagen circle pattern in [0, 1]: hires (17, 65536) and lowres (17, 16, 16), (v - 288) / 10"""
    from cae_tools_amd.data import datagen
    ds = datagen.generate("circle", 17, seed=99)
    hires = (np.asarray(ds["hires"].values, dtype=np.float64)[:, 0].reshape(17, -1) - 288.0) / 10.0
    low = (np.asarray(ds["lowres"].values, dtype=np.float64)[:, 0] - 288.0) / 10.0
    return hires, low


def _edges(n_edge):
    """n_edge ascending edges inside (0, 1): equal bins, multiples of 1/64 for 63"""
    return [(k + 1) / 64.0 for k in range(n_edge)] if n_edge == 63 else [(k + 1) / (n_edge + 1.0) for k in range(n_edge)]


def _pair(pattern, rng, n, h, w):
    """target: h * w consecutive pixels across the ring of n pattern cases; prediction: damped, with noise"""
    a = pattern[0][:n, 100 * 256:100 * 256 + h * w].reshape(n, h, w).copy()
    p = 0.5 + 0.7 * (a - 0.5) + 0.01 * rng.standard_normal(a.shape)
    return p, a


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


def _compare(label, got, ref):
    """counts integer for integer, the first identity, every sum within its bound; prints the worst |got - fsum| / bound"""
    (counts, sums) = got
    assert counts["members"].dtype == np.int64 and counts["pairs"].dtype == np.int64 and isinstance(counts["unclassified"], int)
    assert sums.dtype == np.float64 and sums.shape == (ref.n_strata, 8)
    assert np.array_equal(counts["members"], ref.members), label
    assert np.array_equal(counts["pairs"], ref.pairs), label
    assert counts["unclassified"] == ref.unclassified, label
    assert int(counts["members"].sum()) + counts["unclassified"] == ref.pixels, label
    bounded = np.isfinite(ref.bound)
    with np.errstate(invalid="ignore"):
        err = np.abs(sums - ref.sums)
        worst = float(np.max(np.where(bounded & (ref.bound > 0), err / np.where(ref.bound > 0, ref.bound, 1.0), 0.0), initial=0.0))
        print(f"{label}: {int(ref.pairs.sum())} pairs in {int((ref.pairs > 0).sum())} of {ref.n_strata} strata, "
              f"{ref.unclassified} unclassified, max |sum - fsum| / bound = {worst:.3e}")
        same = (sums == ref.sums) | (np.isnan(sums) & np.isnan(ref.sums))
        assert np.where(bounded, err <= ref.bound, same).all(), label


def _check(label, p, a, s, edges, shift=0.0, ops=None, channel=0):
    """strata_sums of (N, h, w) p and a under the stratifier s ((N, sh, sw) or (N,)) against the reference, and the second
    identity: one stratum over a finite stratifier against pixel_sums added over the pixels.  ops: the three operands as
    the call takes them, where they are not the plain fp64 arrays"""
    (pd, ad, sd) = ops if ops is not None else (device_operand(_nchw(p)), device_operand(_nchw(a)),
                                                 device_operand(s if s.ndim == 1 else _nchw(s)))
    got = strata_sums(pd, ad, sd, edges, shift, channel=channel)
    ref = Reference(p, a, s.reshape(-1, 1, 1) if s.ndim == 1 else s, edges, shift)
    _compare(label, got, ref)
    one = strata_sums(pd, ad, np.zeros(p.shape[0]), [], 0.25)
    whole = Reference(p, a, np.zeros((p.shape[0], 1, 1)), [], 0.25)
    _compare(label + ", one stratum", one, whole)
    if p.size:
        with np.errstate(invalid="ignore", over="ignore"):
            nine = pixel_sums(pd, ad, 0.25).reshape(9, -1).sum(axis=1)
        assert int(nine[0]) == int(one[0]["pairs"][0]) == int(whole.pairs[0]), label
        bounded = np.isfinite(whole.bound[0])
        with np.errstate(invalid="ignore"):
            same = (nine[1:] == whole.sums[0]) | (np.isnan(nine[1:]) & np.isnan(whole.sums[0]))
            assert np.where(bounded, np.abs(nine[1:] - whole.sums[0]) <= whole.bound[0], same).all(), label
    return got, ref


@pytest.mark.parametrize("plane", PLANES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_planes_cases_edges_and_the_simple_grids(pattern, plane):
    """every plane with 1, 3 and 17 cases; the grids identity, (1, 1) and (N,) and the four edge counts go round"""
    (h, w) = plane
    rng = np.random.default_rng(1000 * h + w)
    for (turn, n) in enumerate(CASES):
        for (j, grid) in enumerate(("identity", "one", "per case")):
            n_edge = N_EDGE[(turn + j + w) % 4]
            (p, a) = _pair(pattern, rng, n, h, w)
            s = a.copy() if grid == "identity" else (rng.uniform(0.0, 1.0, (n, 1, 1)) if grid == "one" else rng.uniform(0.0, 1.0, n))
            for x in (p, a, s):
                _sprinkle(rng, x, [np.nan, np.inf] if x.size > 8 else [])
            _check(f"plane {h} x {w}, {n} cases, {grid}, {n_edge} edges", p, a, s, _edges(n_edge))


@pytest.mark.parametrize("grids", [((4, 4), (33, 65)), ((3, 5), (7, 11)), ((9, 9), (4, 4))], ids=str)
@pytest.mark.parametrize("n_edge", N_EDGE)
def test_coarser_and_finer_grids(pattern, grids, n_edge):
    """ratios that are no integers, two axes that differ, and a stratifier finer than the target"""
    ((sh, sw), (h, w)) = grids
    rng = np.random.default_rng(7 * sh + n_edge)
    (p, a) = _pair(pattern, rng, 3, h, w)
    s = pattern[1][:3, 2:2 + sh, 3:3 + sw].copy()
    s[1, sh - 1, sw - 1] = np.nan
    (got, ref) = _check(f"{sh} x {sw} -> {h} x {w}, {n_edge} edges", p, a, s, _edges(n_edge))
    assert ref.unclassified > 0 or (sh, sw) == (9, 9)


@pytest.mark.parametrize("field", ["smooth", "constant", "noise"])
def test_smooth_constant_and_noise(pattern, field):
    (n, h, w) = (3, 33, 65)
    rng = np.random.default_rng(17)
    (p, a) = _pair(pattern, rng, n, h, w)
    if field == "smooth":                   # the 16 x 16 input under the target: a wave meets one or two strata
        s = pattern[1][:n].copy()
    elif field == "constant":               # one round per 64 pixels
        s = np.full((n, h, w), 0.3)
    else:                                   # per-pixel noise over 64 strata: some 41 distinct among a wave's 64 pixels
        s = rng.uniform(0.0, 1.0, (n, h, w))
    (got, ref) = _check(field, p, a, s, _edges(63))
    occupied = int((ref.members > 0).sum())
    assert occupied == (1 if field == "constant" else occupied) and (field != "noise" or occupied == 64)


def test_edges_signed_zero_huge_and_missing_values(pattern):
    (n, h, w) = (3, 33, 65)
    rng = np.random.default_rng(19)
    edges = [-1.0, 0.0, 0.25, 0.5, 1.0, 1e300]
    for where in ("s", "p", "a", "all"):
        (p, a) = _pair(pattern, rng, n, h, w)
        s = rng.integers(-8, 9, (n, h, w)) / 4.0                # every value on an edge or a quarter of the way
        _sprinkle(rng, s, [-0.0] * 40 + [1e300, -1e300, np.nextafter(0.25, 0.0), np.nextafter(0.25, 1.0)])
        special = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, 1e300, -1e300, -0.0]
        for (name, x) in (("s", s), ("p", p), ("a", a)):
            if where in (name, "all"):
                _sprinkle(rng, x, special)
        if where == "all":                  # and at one pixel in all three
            p[0, 5, 5] = a[0, 5, 5] = s[0, 5, 5] = np.nan
            p[1, 6, 6] = a[1, 6, 6] = 1e300
        (got, ref) = _check(f"special values in {where}", p, a, s, edges)
        zero = (s == 0.0) & np.isfinite(s)
        assert np.signbit(s[zero]).any() and ref.members[2] >= zero.sum()      # -0.0 lies at or above the edge 0.0
        assert ref.members[6] >= 1 and ref.members[0] >= 1


def test_a_second_channel(pattern):
    (n, h, w) = (3, 17, 31)
    rng = np.random.default_rng(21)
    (p, a) = _pair(pattern, rng, n, h, w)
    s = pattern[1][:n, :4, :5].copy()
    s4 = _nchw(s, channels=3, channel=1)
    s4[:, 0] = 0.9                          # what channel 0 would give: everything in one stratum
    ops = (device_operand(_nchw(p, 2)), device_operand(_nchw(a, 3)), device_operand(s4))
    (got, ref) = _check("channel 1", p, a, s, _edges(6), ops=ops, channel=1)
    assert (ref.members > 0).sum() > 1


@pytest.mark.parametrize("kinds", [("f4", "f4", "f4"), ("f8", ">f4", ">f8"), (">f4", ">f8", "f4"), (">f8", "f8", ">f4"),
                                   ("f4", ">f8", "f8")], ids=str)
def test_element_kinds(pattern, kinds):
    (n, h, w) = (3, 17, 31)
    rng = np.random.default_rng(23)
    (p, a) = _pair(pattern, rng, n, h, w)
    s = pattern[1][:n, :6, :7].copy()
    for x in (p, a, s):
        _sprinkle(rng, x, [np.nan, np.inf, 1e300, -0.0])
    with np.errstate(over="ignore"):        # 1e300 is Inf in fp32
        arrays = [_nchw(x, 2, np.dtype(k)) for (x, k) in zip((p, a, s), kinds)]
    ops = [device_operand(x) for x in arrays]
    want = {"f4": _lib.ELEM_F32, "f8": _lib.ELEM_F64, ">f4": _lib.ELEM_F32_BE, ">f8": _lib.ELEM_F64_BE}
    assert [op.kind for op in ops] == [want[k] for k in kinds]
    stored = [np.asarray(x[:, 0], dtype=np.float64) for x in arrays]
    _check(f"kinds {kinds}", *stored, _edges(6), ops=ops)


@pytest.mark.parametrize("offsets", [(1, 1, 1), (1, 3, 2), (2, 0, 3), (3, 3, 0)], ids=str)
def test_misaligned_device_tensors(pattern, offsets):
    """fp32 tensors that start 4, 8 or 12 bytes after a 16-byte boundary"""
    (n, h, w) = (5, 1, 4099)
    rng = np.random.default_rng(29)
    (p, a) = _pair(pattern, rng, n, h, w)
    s = pattern[1][:n, :1, :13].copy()
    tensors = []
    for (x, off) in zip((p, a, s), offsets):
        x4 = _nchw(x, 2, np.float32)
        flat = torch.empty(x4.size + off, dtype=torch.float32, device="cuda")
        flat[off:] = torch.from_numpy(x4.reshape(-1)).cuda()
        t = flat[off:].view(x4.shape)
        assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
        tensors.append(t)
    stored = [np.asarray(x, dtype=np.float32).astype(np.float64) for x in (p, a, s)]
    _check(f"offsets {offsets}", *stored, _edges(6), ops=[device_operand(t) for t in tensors])


def test_a_call_of_several_workgroups_and_the_second_pass(pattern):
    """17 cases of 4099 pixels are 34 (case, chunk) items: nine workgroups, whose partials the fold adds; then the sums about
    each stratum's own means, from which the variances come without the cancellation"""
    (n, h, w, n_edge) = (17, 1, 4099, 6)
    groups = int(_lib.load().cae_strata_sums_workspace_bytes(n, h, w, n_edge + 1)) // ((n_edge + 1) * 8 * 8)
    assert groups == 9
    rng = np.random.default_rng(3)
    (p, a) = _pair(pattern, rng, n, h, w)
    (p, a) = (288.0 + 10.0 * p, 288.0 + 10.0 * a)
    s = pattern[1][:n, 3:4, :].copy()
    (got, ref) = _check("nine workgroups", p, a, s, _edges(n_edge), shift=293.0)
    assert (ref.pairs > 0).sum() >= 3
    means = strata_scores.stratum_means(*got, 293.0)
    assert means.shape == (2, n_edge + 1) and (means[:, ref.pairs == 0] == 293.0).all()
    (centred, ref2) = _check("per-stratum shifts", p, a, s, _edges(n_edge), shift=means)
    scores = strata_scores.scores_from_sums(got[0], got[1], centred[1], shift=293.0, centred_shift=means)
    v = strata_of(on_target_grid(s, h, w), _edges(n_edge))
    for k in np.nonzero(ref.pairs > 1)[0]:
        (pk, ak) = (p[v == k], a[v == k])
        assert abs(scores["correlation"][k] - np.corrcoef(pk, ak)[0, 1]) < 1e-9
        assert abs(scores["rmse"][k] - np.sqrt(np.mean((pk - ak) ** 2))) < 1e-11
    assert abs(scores["pooled"]["correlation"] - np.corrcoef(p.reshape(-1), a.reshape(-1))[0, 1]) < 1e-9


def _raw(p, a, s, n, h, w, sh, sw, edges, fill=0x5A, change=()):
    """cae_strata_sums itself on output buffers filled with garbage; returns (code, counts, sums) as numpy"""
    import ctypes as C
    change = dict(change)
    lib = _lib.load()
    dev = p.tensor.device
    n_strata = len(edges) + 1
    counts = torch.full((2 * n_strata + 1,), fill, dtype=torch.int64, device=dev)
    sums = torch.full((n_strata, 8), -7.0 - fill, dtype=torch.float64, device=dev)
    need = int(lib.cae_strata_sums_workspace_bytes(n, h, w, n_strata))
    ws = torch.full((max(need, 1 << 16),), 0xFF, dtype=torch.uint8, device=dev)    # NaN bits: a partial read before it is written shows
    e = (C.c_double * max(len(edges), 1))(*edges)
    z = (C.c_double * n_strata)(*([change.pop("shift", 0.0)] * n_strata))
    args = dict(n=n, h=h, w=w, sh=sh, sw=sw, n_edge=len(edges), bytes=max(need, 1 << 16))
    args.update(change)
    rc = lib.cae_strata_sums(*p.args(), *a.args(), *s.args(), args["n"], args["h"], args["w"], args["sh"], args["sw"], e, args["n_edge"],
                             z, z, counts.data_ptr(), sums.data_ptr(), ws.data_ptr(), args["bytes"],
                             torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy(), sums.cpu().numpy()


def test_two_runs_garbage_empty_and_refused_calls(pattern):
    (n, h, w, sh, sw) = (17, 1, 4099, 1, 16)
    rng = np.random.default_rng(31)
    (p, a) = _pair(pattern, rng, n, h, w)
    s = pattern[1][:n, 5:6, :].copy()
    for x in (p, a, s):
        _sprinkle(rng, x, [np.nan, np.inf, -np.inf])
    edges = _edges(6)
    (pd, ad, sd) = (device_operand(_nchw(p)), device_operand(_nchw(a)), device_operand(_nchw(s)))
    first = _raw(pd, ad, sd, n, h, w, sh, sw, edges)
    second = _raw(pd, ad, sd, n, h, w, sh, sw, edges, fill=0x33)
    assert first[0] == 0 and second[0] == 0
    assert first[1].tobytes() == second[1].tobytes() and first[2].tobytes() == second[2].tobytes()     # whatever the buffers held
    ref = Reference(p, a, s, edges)
    got = ({"members": first[1][:7], "pairs": first[1][7:14], "unclassified": int(first[1][14])}, first[2])
    _compare("over garbage", got, ref)
    wrapped = strata_sums(pd, ad, sd, edges)
    assert wrapped[1].tobytes() == first[2].tobytes() and np.array_equal(wrapped[0]["pairs"], got[0]["pairs"])
    # no case, or no pixel: zeros over the garbage
    for change in (dict(n=0), dict(h=0), dict(w=0), dict(n=0, h=0, w=0)):
        empty = _raw(pd, ad, sd, n, h, w, sh, sw, edges, change=change)
        assert empty[0] == 0 and not empty[1].any() and not empty[2].any(), change
    (counts, sums) = strata_sums(np.zeros((0, 1, 4, 4)), np.zeros((0, 2, 4, 4)), np.zeros((0, 1, 2, 2)), [0.5])
    assert counts["members"].shape == (2,) and not counts["pairs"].any() and counts["unclassified"] == 0 and sums.shape == (2, 8)
    assert not strata_sums(np.zeros((3, 1, 0, 5)), np.zeros((3, 1, 0, 5)), np.zeros(3), [])[1].any()
    # a refused call writes nothing
    lib = _lib.load()
    for (bad, kw) in ((edges, dict(n_edge=64)), (edges, dict(n_edge=-1)), (edges, dict(sh=0)), (edges, dict(h=(1 << 30) + 1)),
                      ([0.5, 0.5], {}), ([0.5, 0.25], {}), ([float("nan")], {}), ([float("inf")], {}),
                      (edges, dict(shift=float("nan"))), (edges, dict(bytes=8)), (edges, dict(sw=17))):
        refused = _raw(pd, ad, sd, n, h, w, sh, sw, bad, fill=5, change=kw)
        assert refused[0] == ERR_ARG and lib.cae_last_error().decode().startswith("cae_strata_sums: "), (bad, kw)
        assert (refused[1] == 5).all() and (refused[2] == -12.0).all(), (bad, kw)


def test_argument_errors_name_the_function():
    (x, y, s) = (np.zeros((2, 1, 4, 4), dtype=np.float32), np.zeros((2, 1, 4, 5), dtype=np.float32), np.zeros((2, 2, 2, 2)))
    for (args, kw) in (((x, y, s, []), {}), ((x, x, s[:1], []), {}), ((x, x, s[0], []), {}), ((x, x, s, [1.0, 1.0]), {}),
                       ((x, x, s, [float("nan")]), {}), ((x, x, s, list(range(64))), {}), ((x, x, s, [0.5]), dict(channel=2)),
                       ((x, x, s, [0.5]), dict(channel=0.5)), ((x, x, s, [0.5]), dict(shift=[1.0, 2.0])),
                       ((x, x, s, [0.5]), dict(shift=float("inf"))), ((x, x, np.zeros(3), []), {})):
        with pytest.raises(ValueError, match="strata_sums: "):
            strata_sums(*args, **kw)


# ---- train_cae -> strata ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 circle cases per partition, the smallest set datagen makes"""
    from cae_tools_amd.data import datagen
    root = tmp_path_factory.mktemp("strata")
    paths = {}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        paths[part] = str(root / f"{part}.nc")
        datagen.generate("circle", 12, seed=seed).to_netcdf(paths[part])
    return root, paths


def test_train_strata(data, monkeypatch):
    from cae_tools_amd.cli import evaluate_cae, strata as cli, train_cae
    (root, paths) = data
    model = str(root / "model")
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                        "--input-variables", "lowres", "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"])
    seen = []

    class Recording(evaluate_cae.ModelEvaluator):
        def build_html(self, case_dimension, train_ds, test_ds, model_metrics):
            super().build_html(case_dimension, train_ds, test_ds, model_metrics)
            seen.append(np.asarray(test_ds["mse"].values, dtype=np.float64))

    monkeypatch.setattr(evaluate_cae, "ModelEvaluator", Recording)
    out = str(root / "report")
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["--test-inputs", paths["test"], "--model-folder", model, "--output-html-folder", out,
                  "--strata-variable", "lowres", "--strata-count", "4"])
    monkeypatch.undo()
    assert sorted(f for f in os.listdir(out) if f.startswith("strata")) == ["strata_test.json"]
    with open(os.path.join(out, "strata_test.json")) as f:
        rec = json.load(f, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert (rec["variable"], rec["channel"], rec["n_strata"]) == ("lowres", 0, 4) and len(rec["edges"]) == 3
    assert (rec["in_shape"], rec["out_shape"]) == ([16, 16], [256, 256])
    assert sum(rec["pairs"]) == 12 * 256 * 256 == rec["pooled"]["pairs"] == sum(rec["members"]) and rec["unclassified"] == 0
    assert all(m % 256 == 0 for m in rec["members"])            # a source pixel covers 16 x 16 target pixels
    number = lambda v: float("nan") if v is None else float(v)      # noqa: E731
    assert abs(np.nansum([number(v) for v in rec["share"]]) - 1.0) < 1e-12
    assert abs(np.nansum([number(v) for v in rec["mse_share"]]) - 1.0) < 1e-12
    assert abs(rec["pooled"]["rmse"] ** 2 - float(np.mean(seen[0]))) <= 1e-9 * float(np.mean(seen[0]))
    lines = [ln for ln in log.getvalue().splitlines() if ln.startswith("strata ")]
    finite = [(r, name) for (r, name) in zip(rec["rmse"], rec["labels"]) if r is not None]
    (low, high) = (min(finite), max(finite))
    assert lines == [f"strata test: lowres, 4 strata, rmse {low[0]:.6g} ({low[1]}) .. {high[0]:.6g} ({high[1]}), unclassified 0"]
    with open(os.path.join(out, "index.html")) as f:
        page = f.read()
    assert page.count("<h2>Skill by stratum</h2>") == 1 and page.count('alt="test skill by stratum"') == 1
    assert f"test: 4 strata of lowres, {12 * 256 * 256} pixel pairs, 0 pixels unclassified" in page
    assert f"<td>{rec['pooled']['rmse']:.6g}</td>" in page
