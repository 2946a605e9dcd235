"""cae_normalise_pack_gather and cae_case_importance on the GPU: the gathered batch against normalise_pack on the
numpy-gathered source, byte for byte; the eight per-case sums and the three per-pixel sums against the numpy restatement of
the definition (importance_ref.py, np.longdouble) - n, both win counts and the map's count exactly, every floating-point sum
of m terms within (m + 4) 2^-53 S|t| - for every plane, number of cases, target kind, alignment and non-finite value; the
independence of a case's sums from the call and of the map from the cut of the cases, byte for byte; then train_cae ->
apply_cae -> importance with every number of importance_test.json compared.

Largest |got - want| / bound measured on an MI355X (each check prints its figure before it asserts): the per-case sums 0.20
(plane 1, 65 cases: one term, where the three roundings of a square stand against a bound of five), 4.7e-4 at plane 4097 and
1.6e-4 at plane 3 * 4096 + 5; the map 0.36 (plane 4097, three cases: again a handful of terms) and 0.13 over 65 cases; the
target kinds 8.3e-3 (sums) and 0.31 (map); unaligned case starts 1.4e-3 and 0.34; NaN, +-Inf and an all-NaN case 6.3e-4 and
0.31; end to end the pooled mse and mae per repeat 3.6e-5, the sensitivity 3.7e-6, the per-case change of the mse 1.3e-5 and
the base mse against case_measures 2.7e-5 of their bounds.  n, the win counts and the map's count are exact everywhere."""
import io
import json
import math
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import importance_ref
from importance_ref import Reference
from cae_tools_amd import _lib
from cae_tools_amd.engine import (case_importance, case_measures, denormalise_f64, device_operand, normalise_pack, operand_cases,
                                  pack_gather)
from cae_tools_amd.utils import importance

pytestmark = pytest.mark.gpu

(VMIN, RANGE) = (288.0, 10.0)
KINDS = {"f32": _lib.ELEM_F32, "f32be": _lib.ELEM_F32_BE, "f64": _lib.ELEM_F64, "f64be": _lib.ELEM_F64_BE}


# ---- cae_normalise_pack_gather --------------------------------------------------------------------

def _gathered(src, rows, c_dst, c_off, vmin, vmax, enable, hw):
    """(pack_gather's dst, the same rows by normalise_pack of the numpy-gathered source), both over a dst filled with -7"""
    (n_dst, c_src) = (len(rows), src.shape[1])
    raw = torch.from_numpy(src).cuda()
    got = torch.full((n_dst, c_dst, hw, 1), -7.0, dtype=torch.float32, device="cuda")
    pack_gather(raw, got, c_off, torch.from_numpy(np.asarray(rows, dtype=np.int32)).cuda(), vmin, vmax, enable=enable)
    valid = np.array([0 <= r < src.shape[0] for r in rows])
    picked = np.stack([src[r] if ok else np.zeros_like(src[0]) for (r, ok) in zip(rows, valid)])
    want = torch.full((n_dst, c_dst, hw, 1), -7.0, dtype=torch.float32, device="cuda")
    normalise_pack(torch.from_numpy(picked).cuda(), want, c_off, vmin, vmax, enable=enable)
    torch.cuda.synchronize()
    return got.cpu().numpy(), want.cpu().numpy(), valid


@pytest.mark.parametrize("hw", [1, 255, 256, 1025])
@pytest.mark.parametrize("c_src", [1, 3])
def test_pack_gather_against_normalise_pack(hw, c_src):
    rng = np.random.default_rng(hw * 7 + c_src)
    n_src = 6
    src = (280.0 + 20.0 * rng.random((n_src, c_src, hw, 1))).astype(np.float32)
    tables = {"identity": list(range(n_src)), "cycle": [1, 2, 3, 4, 5, 0], "repeated": [2, 2, 0, 5, 5, 5],
              "fewer": [4, 1], "more": [0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 0, 3]}
    for (name, rows) in tables.items():
        for (vmin, vmax, enable) in ((280.0, 300.0, True), (280.0, 300.0, False), (285.5, 285.5, True)):
            (got, want, valid) = _gathered(src, rows, c_src + 2, 1, vmin, vmax, enable, hw)
            assert valid.all()
            assert got.tobytes() == want.tobytes(), (name, vmin, vmax, enable)
            assert (got[:, 0] == -7.0).all() and (got[:, c_src + 1] == -7.0).all()      # the other channels are untouched
            if enable and vmax > vmin:
                assert np.array_equal(got[:, 1:1 + c_src], importance_ref.normalise(src[rows], vmin, vmax))


def test_pack_gather_does_not_follow_an_index_outside_the_source():
    """an index of -1 and one of n_src give NaN rows; the rest stay right.  k_normalise_pack_gather tests 0 <= row < n_src
    before it forms the source address, and the destination index does not depend on the row table."""
    rng = np.random.default_rng(3)
    (n_src, c_src, hw) = (5, 3, 255)
    src = (280.0 + 20.0 * rng.random((n_src, c_src, hw, 1))).astype(np.float32)
    rows = [3, -1, 0, n_src, 4, 2 ** 31 - 1, -2 ** 31]
    (got, want, valid) = _gathered(src, rows, c_src + 1, 0, 280.0, 300.0, True, hw)
    assert valid.tolist() == [True, False, True, False, True, False, False]
    assert got[valid].tobytes() == want[valid].tobytes()
    assert np.isnan(got[~valid][:, :c_src]).all()
    assert (got[:, c_src] == -7.0).all()


# ---- cae_case_importance against the reference ---------------------------------------------------------

def _scores(rng, n, plane):
    """seeded scores in [0, 1] and a target around their denormalised values: base, pert fp32 (n, plane), a fp64 (n, plane)"""
    base = rng.random((n, plane)).astype(np.float32)
    pert = np.clip(base + 0.2 * rng.standard_normal((n, plane)), 0, 1).astype(np.float32)
    a = VMIN + RANGE * rng.random((n, plane))
    return base, pert, a


def _raw(base, b_off, bs, pert, p_off, ps, a, ak, a_off, as_, n, plane, with_map=False, start=None):
    """cae_case_importance on element offsets into flat device buffers (case starts of any alignment), with -7.0 doubles
    around sums_dev and map_dev and behind the workspace checked.  Returns (sums (n, 8), map (3, plane) or None)"""
    lib = _lib.load()
    eb = 4 if ak in (0, 1) else 8
    guard = 8
    out = torch.full((guard + n * 8 + guard,), -7.0, dtype=torch.float64, device="cuda")
    fld = torch.full((guard + 3 * plane + guard,), -7.0, dtype=torch.float64, device="cuda")
    fld[guard:guard + 3 * plane] = 0.0 if start is None else torch.from_numpy(np.asarray(start).reshape(-1)).cuda()
    need = int(lib.cae_case_importance_workspace_bytes(n, plane))
    assert need == n * ((plane + 63) // 64) * 64
    ws = torch.full((need // 8 + guard,), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.cae_case_importance(base.data_ptr() + 4 * b_off, bs, pert.data_ptr() + 4 * p_off, ps, a.data_ptr() + eb * a_off,
                                       ak, as_, n, plane, VMIN, RANGE, out.data_ptr() + 8 * guard,
                                       fld.data_ptr() + 8 * guard if with_map else None, ws.data_ptr(), need, None))
    torch.cuda.synchronize()
    (host, fh) = (out.cpu().numpy(), fld.cpu().numpy())
    assert (host[:guard] == -7.0).all() and (host[-guard:] == -7.0).all()
    assert (fh[:guard] == -7.0).all() and (fh[-guard:] == -7.0).all()
    assert (ws.cpu().numpy()[need // 8:] == -7.0).all()
    return host[guard:-guard].reshape(n, 8).copy(), fh[guard:-guard].reshape(3, plane).copy() if with_map else None


def _flat(x):
    return torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()


_CASES = {}


def _case(n, plane):
    """one operand set and its Reference per (n, plane), shared by the checks that use the same values"""
    if (n, plane) not in _CASES:
        (base, pert, a) = _scores(np.random.default_rng(1000 * n + plane), n, plane)
        _CASES[(n, plane)] = (base, pert, a, Reference(base, pert, a, VMIN, RANGE))
    return _CASES[(n, plane)]


@pytest.mark.parametrize("n_case", [1, 2, 3, 65])
@pytest.mark.parametrize("plane", [1, 63, 64, 65, 4097, 3 * 4096 + 5])
def test_planes_and_cases(plane, n_case):
    (base, pert, a, ref) = _case(n_case, plane)
    (sums, field) = _raw(_flat(base), 0, plane, _flat(pert), 0, plane, _flat(a), _lib.ELEM_F64, 0, plane, n_case, plane, with_map=True)
    ref.check(sums, f"plane {plane} n {n_case}")
    ref.check_map(field, f"plane {plane} n {n_case}")
    # the denormalised values are cae_denormalise_f64's bits
    den = denormalise_f64(torch.from_numpy(base).cuda(), VMIN, VMIN + RANGE).cpu().numpy()
    assert np.array_equal(den, importance_ref.denormalise(base, VMIN, RANGE))
    # the wrapper, through the operand vocabulary
    shape = (n_case, 1, 1, plane)
    got = case_importance(torch.from_numpy(base.reshape(shape)).cuda(), torch.from_numpy(pert.reshape(shape)).cuda(),
                          a.reshape(shape), VMIN, VMIN + RANGE)
    assert got.tobytes() == sums.tobytes()


def test_every_target_kind(tmp_path):
    """the target as fp32, fp64 and as the big-endian slabs of a NetCDF-3 file, read back the way the loader hands them on"""
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import as_numpy, open_dataset
    (n, h, w) = (3, 5, 31)
    (base, pert, a) = _scores(np.random.default_rng(5), n, h * w)
    path = str(tmp_path / "kinds.nc")
    netcdf3.write(path, {"n": n, "c": 1, "y": h, "x": w},
                  {"t32": (("n", "c", "y", "x"), a.reshape(n, 1, h, w).astype(np.float32), {}),
                   "t64": (("n", "c", "y", "x"), a.reshape(n, 1, h, w), {})})
    ds = open_dataset(path)
    slabs = {"f32be": as_numpy(ds["t32"]), "f64be": as_numpy(ds["t64"])}
    assert all(v.dtype.byteorder == ">" for v in slabs.values())
    slabs["f32"] = a.reshape(n, 1, h, w).astype(np.float32)
    slabs["f64"] = a.reshape(n, 1, h, w)
    (b4, p4) = (torch.from_numpy(base.reshape(n, 1, h, w)).cuda(), torch.from_numpy(pert.reshape(n, 1, h, w)).cuda())
    refs = {4: Reference(base, pert, a.astype(np.float32), VMIN, RANGE), 8: Reference(base, pert, a, VMIN, RANGE)}
    found = {}
    for (kind, slab) in slabs.items():
        op = device_operand(slab)
        assert op.kind == KINDS[kind]
        maps = torch.zeros((3, h, w), dtype=torch.float64, device="cuda")
        found[kind] = case_importance(b4, p4, op, VMIN, VMIN + RANGE, maps=maps)
        refs[op.elem_bytes].check(found[kind], kind)
        refs[op.elem_bytes].check_map(maps.cpu().numpy(), kind)
        # a piece of the operand: the cases 1 .. 2 alone
        part = case_importance(b4[1:], p4[1:], operand_cases(op, 1, 3), VMIN, VMIN + RANGE)
        assert part.tobytes() == found[kind][1:].tobytes()
    assert found["f32"].tobytes() == found["f32be"].tobytes() and found["f64"].tobytes() == found["f64be"].tobytes()


@pytest.mark.parametrize("offsets", [(0, 1, 3), (1, 3, 2), (3, 2, 1)])
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_unaligned_case_starts_and_strides(offsets, kind):
    """cases that start at odd element offsets with strides longer than the plane"""
    (n, plane) = (4, 23 * 67)
    rng = np.random.default_rng(sum(offsets) * 3 + len(kind))
    (bo, po, ao) = offsets
    (sb, sp, sa) = (plane + 1, plane + 5, plane + 3)
    bf = rng.random(bo + n * sb).astype(np.float32)
    pf = rng.random(po + n * sp).astype(np.float32)
    af = (VMIN + RANGE * rng.random(ao + n * sa)).astype(np.float32 if kind == "f32" else np.float64)
    cases = lambda buf, off, st: np.stack([buf[off + k * st: off + k * st + plane] for k in range(n)])     # noqa: E731
    ref = Reference(cases(bf, bo, sb), cases(pf, po, sp), cases(af, ao, sa), VMIN, RANGE)
    (sums, field) = _raw(_flat(bf), bo, sb, _flat(pf), po, sp, _flat(af), KINDS[kind], ao, sa, n, plane, with_map=True)
    ref.check(sums, f"raw {kind} {offsets}")
    ref.check_map(field, f"raw {kind} {offsets}")
    # the same cases laid out densely from aligned starts: the same bytes, whatever the alignment
    dense = _raw(_flat(cases(bf, bo, sb)), 0, plane, _flat(cases(pf, po, sp)), 0, plane, _flat(cases(af, ao, sa)), KINDS[kind], 0,
                 plane, n, plane)[0]
    assert dense.tobytes() == sums.tobytes()


def test_values_that_are_not_finite():
    rng = np.random.default_rng(12)
    (n, plane) = (7, 32 * 70)
    (base, pert, a) = _scores(rng, n, plane)
    a[0, 5] = np.nan
    a[1, 70] = np.inf
    a[1, 71] = -np.inf
    a[2, :] = np.nan                    # a case without a pair
    base[3, 9] = np.nan
    base[3, 10] = np.inf
    pert[4, 11] = np.nan
    pert[4, 12] = -np.inf
    pert[5, 13] = np.float32(3e38)      # finite as fp32 and as P
    a[6, plane - 1] = np.nan
    ref = Reference(base, pert, a, VMIN, RANGE)
    assert ref.sums[:, 0].astype(int).tolist() == [plane - 1, plane - 2, 0, plane - 2, plane - 2, plane, plane - 1]
    (sums, field) = _raw(_flat(base), 0, plane, _flat(pert), 0, plane, _flat(a), _lib.ELEM_F64, 0, plane, n, plane, with_map=True)
    ref.check(sums, "non-finite")
    ref.check_map(field, "non-finite")
    assert np.isfinite(sums).all() and np.isfinite(field).all()


def test_pert_is_base_gives_zeros_exactly():
    (base, _, a, _) = _case(3, 4097)
    b = _flat(base)
    (sums, field) = _raw(b, 0, 4097, b, 0, 4097, _flat(a), _lib.ELEM_F64, 0, 4097, 3, 4097, with_map=True)
    assert (sums[:, 5] == 0.0).all() and (sums[:, 6] == 0.0).all() and (sums[:, 7] == 0.0).all()
    assert sums[:, 1].tobytes() == sums[:, 2].tobytes() and sums[:, 3].tobytes() == sums[:, 4].tobytes()
    assert field[1].tobytes() == field[2].tobytes()
    Reference(base, base, a, VMIN, RANGE).check(sums, "pert is base")
    # the per-case base mse is cae_case_measures' on the denormalised prediction, within the bound
    den = importance_ref.denormalise(base, VMIN, RANGE).reshape(3, 1, 1, 4097)
    mse = case_measures(den, a.reshape(3, 1, 1, 4097))[:, 1]
    ref = Reference(base, base, a, VMIN, RANGE)
    assert (np.abs(mse.astype(importance_ref.LD) - ref.sums[:, 2] / 4097) <= ref.bound[:, 2] / 4097).all()


# ---- independence --------------------------------------------------------------------------------------

def test_a_case_does_not_depend_on_the_call_and_the_map_not_on_the_cut():
    (n, plane) = (65, 4097)
    (base, pert, a, ref) = _case(n, plane)
    (b, p, t) = (_flat(base), _flat(pert), _flat(a))
    (whole, field) = _raw(b, 0, plane, p, 0, plane, t, _lib.ELEM_F64, 0, plane, n, plane, with_map=True)
    # two identical runs give identical bytes
    (again, field2) = _raw(b, 0, plane, p, 0, plane, t, _lib.ELEM_F64, 0, plane, n, plane, with_map=True)
    assert again.tobytes() == whole.tobytes() and field2.tobytes() == field.tobytes()
    # the sums with and without a map are the same bytes
    (plain, none) = _raw(b, 0, plane, p, 0, plane, t, _lib.ELEM_F64, 0, plane, n, plane)
    assert none is None and plain.tobytes() == whole.tobytes()
    # case i of the call of 65 has the bits of a call with that case alone, with and without a map
    for i in (0, 1, 31, 64):
        for with_map in (False, True):
            alone = _raw(b, i * plane, plane, p, i * plane, plane, t, _lib.ELEM_F64, i * plane, plane, 1, plane, with_map=with_map)[0]
            assert alone.tobytes() == whole[i:i + 1].tobytes(), (i, with_map)
    # the map after one call of 65 cases equals the map after calls of 1 + 7 + 57 cases
    carried = None
    pieces = []
    for (c0, c1) in ((0, 1), (1, 8), (8, 65)):
        (s, carried) = _raw(b, c0 * plane, plane, p, c0 * plane, plane, t, _lib.ELEM_F64, c0 * plane, plane, c1 - c0, plane,
                            with_map=True, start=carried)
        pieces.append(s)
    assert carried.tobytes() == field.tobytes()
    assert np.concatenate(pieces).tobytes() == whole.tobytes()
    ref.check(whole, "65 cases")
    ref.check_map(field, "65 cases")


def test_bad_arguments_write_nothing():
    """the refusals with real buffers: CAE_ERR_ARG, the text, and sums, map and workspace untouched"""
    lib = _lib.load()
    (n, plane) = (3, 70)
    (base, pert, a) = _scores(np.random.default_rng(2), n, plane)
    (b, p, t) = (_flat(base), _flat(pert), _flat(a))
    out = torch.full((n * 8,), -7.0, dtype=torch.float64, device="cuda")
    fld = torch.full((3 * plane,), -7.0, dtype=torch.float64, device="cuda")
    need = int(lib.cae_case_importance_workspace_bytes(n, plane))
    ws = torch.full((need // 8,), -7.0, dtype=torch.float64, device="cuda")
    good = dict(base=b.data_ptr(), bs=plane, pert=p.data_ptr(), ps=plane, a=t.data_ptr(), ak=_lib.ELEM_F64, as_=plane, n=n, plane=plane,
                vmin=VMIN, rng=RANGE, sums=out.data_ptr(), map=fld.data_ptr(), ws=ws.data_ptr(), wsb=need, stream=None)
    bad = [(dict(ak=4), "bad argument"), (dict(n=-1), "bad argument"), (dict(bs=-1), "negative stride"),
           (dict(vmin=math.nan), "vmin and range must be finite"), (dict(rng=math.inf), "vmin and range must be finite"),
           (dict(pert=None), "null pointer"), (dict(sums=None), "null pointer"), (dict(as_=plane - 1), "shorter than the plane"),
           (dict(ps=1 << 59), "reaches 2^60"), (dict(a=t.data_ptr() + 4), "aligned"), (dict(ws=ws.data_ptr() + 8), "aligned"),
           (dict(wsb=need - 1), f"needs a workspace of {need} bytes"), (dict(ws=None), f"needs a workspace of {need} bytes")]
    for (change, text) in bad:
        args = dict(good, **change)
        rc = lib.cae_case_importance(*args.values())
        assert rc == -1 and text in lib.cae_last_error().decode(), (change, lib.cae_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (fld == -7.0).all() and (ws == -7.0).all()
    for change in (dict(n=0), dict(plane=0)):
        assert lib.cae_case_importance(*dict(good, **change).values()) == 0
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (fld == -7.0).all() and (ws == -7.0).all()


# ---- train_cae -> apply_cae -> importance --------------------------------------------------------------

VARIABLES = ["lowres", "noise", "fixed"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 circle cases per partition, the smallest set datagen makes, with two more input variables: noise (seeded, per
    case) and fixed (one field repeated for every case)"""
    from cae_tools_amd.data import datagen, netcdf3
    root = tmp_path_factory.mktemp("importance")
    paths = {}
    fixed = np.random.default_rng(99).random((1, 1, 16, 16)).astype(np.float32)
    for (part, seed) in (("train", 1234), ("test", 4321)):
        ds = datagen.generate("circle", 12, seed=seed)
        variables = {name: (tuple(da.dims), np.asarray(da.values), {}) for (name, da) in ds.data_vars.items()}
        variables["noise"] = (("n", "chan", "y1", "x1"), np.random.default_rng(seed).random((12, 1, 16, 16)).astype(np.float32), {})
        variables["fixed"] = (("n", "chan", "y1", "x1"), np.repeat(fixed, 12, axis=0), {})
        paths[part] = str(root / f"{part}.nc")
        netcdf3.write(paths[part], {d: int(k) for (d, k) in ds.dims.items()}, variables)
    return root, paths


def _number(v):
    return math.nan if v is None else v


def _permuted_scores(model, ds, group, perm):
    """the scores the test makes itself: _score_all on the numpy-permuted, numpy-normalised inputs"""
    (lo, hi) = (model.normalisation_parameters[0], model.normalisation_parameters[1])
    planes = []
    for name in model.get_input_variable_names():
        v = np.asarray(ds[name].values).astype(np.float32)
        if name in group:
            v = v[perm]
        planes.append(importance_ref.normalise(v, lo[name], hi[name], enable=model.normalise_input))
    x = torch.from_numpy(np.concatenate(planes, axis=1)).cuda()
    return model._score_all(x).cpu().numpy()


def _close(got, want, tol, what):
    err = abs(importance_ref.LD(_number(got)) - want)
    print(f"importance end to end {what}: |got - want| / bound = {float(err / tol) if tol > 0 else 0.0:.3e}")
    assert err <= tol, (what, got, want, tol)


def test_train_apply_importance(data):
    from cae_tools_amd.cli import apply_cae, evaluate_cae, importance as cli, train_cae
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.models.model_loader import load_model
    (root, paths) = data
    model_dir = str(root / "model")
    scored = str(root / "scored_test.nc")
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model_dir,
                        "--input-variables", *VARIABLES, "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"])
        apply_cae.main([paths["test"], scored, "--model-folder", model_dir])
    flags = ["--test-inputs", scored, "--model-folder", model_dir, "--importance-repeats", "3", "--importance-maps"]
    (out1, out2, out3) = (str(root / "report_1"), str(root / "report_2"), str(root / "report_3"))
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(flags + ["--output-html-folder", out1])
    with redirect_stdout(io.StringIO()):
        cli.main(flags + ["--output-html-folder", out2])
        cli.main(flags + ["--output-html-folder", out3, "--importance-groups", "lowres,noise,fixed", "noise"])
    with open(os.path.join(out1, "importance_test.json"), "rb") as f:
        text = f.read()
    with open(os.path.join(out2, "importance_test.json"), "rb") as f:
        assert f.read() == text                 # the same command twice writes the same bytes
    rec = json.loads(text)
    assert sorted(f for f in os.listdir(out1) if f.startswith("importance_")) == ["importance_test.json"]

    # the reference, fed with scores the test makes itself
    ds = open_dataset(scored)
    model = load_model(model_dir)
    (target, stored) = (np.asarray(ds["hires"].values)[:, 0], np.asarray(ds["model_output"].values))
    (n, h, w) = target.shape
    assert (n, h, w) == (12, 256, 256)
    (vmin, vmax) = (float(model.normalisation_parameters[2]), float(model.normalisation_parameters[3]))
    rng_ = vmax - vmin
    perms = importance_ref.sattolo(n, 3, 0)
    assert np.array_equal(importance.permutations(n, 3, 0), perms)
    with redirect_stdout(io.StringIO()):
        base = _permuted_scores(model, ds, [], None)[:, 0]
    # P0 is the bits apply_cae stored
    assert np.array_equal(importance_ref.denormalise(base, vmin, rng_), stored[:, 0])
    assert (rec["n_cases"], rec["repeats"], rec["seed"], rec["n_groups"]) == (n, 3, 0, 3)
    assert [g["name"] for g in rec["groups"]] == VARIABLES and sorted(rec["order"]) == sorted(VARIABLES)
    u = importance_ref.LD(importance_ref.U)
    measured = case_measures(stored, np.asarray(ds["hires"].values))[:, 1]
    refs = {}
    for (k, name) in enumerate(VARIABLES):
        g = rec["groups"][k]
        per = []
        for r in range(3):
            with redirect_stdout(io.StringIO()):
                pert = _permuted_scores(model, ds, [name], perms[r])[:, 0]
            per.append(Reference(base, pert, target, vmin, rng_))
        refs[name] = per
        assert g["pairs"] == 3 * n * h * w and g["variables"] == [name]
        for (r, ref) in enumerate(per):
            m = importance_ref.LD(n * h * w)
            for (key, col) in (("mse_permuted", 1), ("mse_base", 2), ("mae_permuted", 3), ("mae_base", 4)):
                # a pooled mean: the cases' sums within their bounds, n - 1 additions and one division
                tol = ref.bound[:, col].sum() / m + (n + 1) * u * ref.sums[:, col].sum() / m
                _close(g[key][r], ref.sums[:, col].sum() / m, tol, f"{name} {key}[{r}]")
        # what the record derives from those per-repeat values is held to them exactly, by the formulas of DESIGN.md section 9
        for kind in ("mse", "mae"):
            (b0, b1) = (np.array(g[f"{kind}_base"]), np.array(g[f"{kind}_permuted"]))
            assert g[f"mean_{kind}_base"] == float(np.mean(b0)) and g[f"mean_{kind}_permuted"] == float(np.mean(b1))
            prefix = "" if kind == "mse" else "mae_"
            assert g[prefix + "importance"] == float(np.mean(b1 - b0))
            assert g[prefix + "importance_sd"] == float(np.std(b1 - b0, ddof=1))
            assert g[prefix + "ratio"] == float(np.mean(b1)) / float(np.mean(b0))
        # the sensitivity: the root of a pooled sum over all repeats, half its relative bound and the roundings of the pooling
        (dd, dd_bound) = (sum(ref.sums[:, 5].sum() for ref in per), sum(ref.bound[:, 5].sum() for ref in per))
        want_sens = np.sqrt(dd / (3 * n * h * w))
        _close(g["sensitivity"], want_sens, (dd_bound / dd / 2 + (3 * n + 4) * u) * want_sens if dd > 0 else 0, f"{name} sensitivity")
        assert g["pixels_grew_count"] == int(sum(ref.sums[:, 6].sum() for ref in per))
        assert g["pixels_shrank_count"] == int(sum(ref.sums[:, 7].sum() for ref in per))
        assert g["pixels_grew"] == g["pixels_grew_count"] / g["pairs"] and g["pixels_shrank"] == g["pixels_shrank_count"] / g["pairs"]
        # a case's mse grew where S e1^2 > S e0^2; the two sums differ by far more than their bounds wherever they differ
        grew = np.stack([ref.sums[:, 1] > ref.sums[:, 2] for ref in per])
        assert all((np.abs(ref.sums[:, 1] - ref.sums[:, 2]) > ref.bound[:, 1] + ref.bound[:, 2])[ref.sums[:, 1] != ref.sums[:, 2]].all()
                   for ref in per)
        assert g["cases_grew"] == float(grew.sum()) / (3 * n)
        # per case the change of the mse, averaged over the repeats: both sums within their bounds, then a subtraction, a
        # division and the mean of three
        got_delta = np.array([_number(v) for v in g["case_delta_mse"]]).astype(importance_ref.LD)
        want_delta = sum((ref.sums[:, 1] - ref.sums[:, 2]) / (h * w) for ref in per) / 3
        tol_delta = sum((ref.bound[:, 1] + ref.bound[:, 2] + 6 * u * (ref.sums[:, 1] + ref.sums[:, 2])) / (h * w) for ref in per) / 3
        ratio = np.max(np.where(tol_delta > 0, np.abs(got_delta - want_delta) / np.where(tol_delta > 0, tol_delta, 1), 0))
        print(f"importance end to end {name} case_delta_mse: max |got - want| / bound = {float(ratio):.3e}")
        assert (np.abs(got_delta - want_delta) <= tol_delta).all()
        # the per-case base mse agrees with case_measures on the prediction apply_cae stored, within the bound
        for ref in per:
            err = np.abs(measured.astype(importance_ref.LD) - ref.sums[:, 2] / (h * w))
            print(f"importance end to end {name} base mse against case_measures: max |got - want| / bound = "
                  f"{float(np.max(err / (ref.bound[:, 2] / (h * w)))):.3e}")
            assert (err <= ref.bound[:, 2] / (h * w)).all()
    ranks = sorted(rec["groups"], key=lambda g: g["rank"])
    assert [g["name"] for g in ranks] == rec["order"] and [g["rank"] for g in ranks] == [1, 2, 3]
    assert all(a["importance"] >= b["importance"] for (a, b) in zip(ranks, ranks[1:]))

    # fixed is the same field in every case: permuting it changes nothing
    fixed = rec["groups"][2]
    assert fixed["importance"] == 0.0 and fixed["sensitivity"] == 0.0 and fixed["mae_importance"] == 0.0
    assert fixed["pixels_grew_count"] == 0 and fixed["pixels_shrank_count"] == 0 and fixed["cases_grew"] == 0.0
    assert fixed["mse_permuted"] == fixed["mse_base"] and all(v == 0.0 for v in fixed["case_delta_mse"])
    assert rec["groups"][1]["sensitivity"] >= 0.0

    # a group of all three variables equals scoring the whole permuted batch; a group listed alone equals itself
    with open(os.path.join(out3, "importance_test.json")) as f:
        rec3 = json.load(f)
    assert [g["name"] for g in rec3["groups"]] == ["lowres+noise+fixed", "noise"]
    assert rec3["groups"][1]["mse_permuted"] == rec["groups"][1]["mse_permuted"]
    everything = rec3["groups"][0]
    for r in range(3):
        with redirect_stdout(io.StringIO()):
            pert = _permuted_scores(model, ds, VARIABLES, perms[r])[:, 0]
        # every channel permuted: case i is scored exactly as case perm[i]
        assert np.array_equal(pert, base[perms[r]])
        ref = Reference(base, pert, target, vmin, rng_)
        m = importance_ref.LD(n * h * w)
        tol = ref.bound[:, 1].sum() / m + (n + 1) * u * ref.sums[:, 1].sum() / m
        _close(everything["mse_permuted"][r], ref.sums[:, 1].sum() / m, tol, f"all variables mse_permuted[{r}]")

    # the line, the report and the map page
    shown = lambda v: format(v, ".6g")              # noqa: E731
    parts = [f"{g['name']} {format(g['importance'], '+.6g')} (x{shown(g['ratio'])})" for g in ranks]
    line = f"importance test: 3 groups x 3 permutations of {n} cases, base mse {shown(rec['mse_base'])}: " + ", ".join(parts)
    assert line in log.getvalue().splitlines()
    with open(os.path.join(out1, "index.html")) as f:
        page = f.read()
    assert page.count("<h2>Input importance</h2>") == 1 and page.count('alt="test input importance"') == 1
    assert f"test: 3 groups, 3 permutations of {n} cases, seed 0" in page
    assert 'href="importance/index.html"' in page
    with open(os.path.join(out1, "importance", "index.html")) as f:
        maps_page = f.read()
    for (k, name) in enumerate(VARIABLES):
        assert f'data-layer="{name}"' in maps_page
        with open(os.path.join(out1, "importance", f"test_group{k}.png"), "rb") as f:
            assert f.read(8) == b"\x89PNG\r\n\x1a\n"

    # evaluate_cae itself on the same input: no importance file, no section, and the page it has always written
    out4 = str(root / "report_plain")
    plain_log = io.StringIO()
    with redirect_stdout(plain_log):
        evaluate_cae.main(["--test-inputs", scored, "--model-folder", model_dir, "--output-html-folder", out4])
    assert not [f for f in os.listdir(out4) if f.startswith("importance")]
    assert "importance" not in plain_log.getvalue()
    with open(os.path.join(out4, "index.html")) as f:
        plain = f.read()
    start = page.index("<h2>Input importance</h2>")
    end = page.index("<h2>Training Summary</h2>")
    assert page[:start] + page[end:] == plain


def test_the_python_api_of_another_model_class(data):
    """--method linear through BaseModel.importance with groups, maps and pieces of cases: the record does not depend on
    case_chunk, and the map's count is the number of repeats times the cases"""
    from cae_tools_amd.cli import train_cae
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.models.model_loader import load_model
    (root, paths) = data
    model_dir = str(root / "linear_model")
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model_dir,
                        "--input-variables", *VARIABLES, "--output-variable", "hires", "--method", "linear", "--nr-epochs", "2",
                        "--batch-size", "6"])
        model = load_model(model_dir)
        ds = open_dataset(paths["test"])
        groups = [["lowres", "noise"], ["fixed"]]
        one = model.importance(ds, VARIABLES, "hires", groups=groups, repeats=2, seed=7, maps=True)
        cut = model.importance(ds, VARIABLES, "hires", groups=groups, repeats=2, seed=7, maps=True, case_chunk=5)
    assert type(model).__name__ == "LinearModel"
    assert [g["name"] for g in one["groups"]] == ["lowres+noise", "fixed"]
    assert one["maps"].shape == (2, 3, 256, 256) and (one["maps"][:, 0] == 2 * 12).all()
    assert one["maps"].tobytes() == cut["maps"].tobytes()
    strip = lambda rec: json.dumps({k: v for (k, v) in rec.items() if k != "maps"}, sort_keys=True)        # noqa: E731
    assert strip(one) == strip(cut)
    assert one["groups"][1]["importance"] == 0.0 and one["groups"][1]["sensitivity"] == 0.0
    assert one["groups"][0]["sensitivity"] > 0.0
    with pytest.raises(ValueError, match="'albedo' is not an input variable of the model"):
        model.importance(ds, VARIABLES, "hires", groups=[["albedo"]])
    with pytest.raises(ValueError, match="importance_repeats must be an integer from 1 to 64, got 65"):
        model.importance(ds, VARIABLES, "hires", repeats=65)


def _square(path_in, path_out):
    """the three inputs and the target at 64 x 64 on both sides (a UNET's decoder mirrors its encoder): the 16 x 16 inputs
    repeated 4 x 4, the 256 x 256 target averaged over 4 x 4 blocks"""
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import open_dataset
    ds = open_dataset(path_in)
    variables = {name: (("n", "chan", "y", "x"), np.repeat(np.repeat(np.asarray(ds[name].values), 4, axis=2), 4, axis=3).astype(np.float32),
                        {}) for name in VARIABLES}
    hi = np.asarray(ds["hires"].values).astype(np.float64)
    variables["hires"] = (("n", "chan", "y", "x"), hi.reshape(12, 1, 64, 4, 64, 4).mean(axis=(3, 5)).astype(np.float32), {})
    variables["valid"] = (("n", "chan", "y", "x"), np.ones((12, 1, 64, 64), dtype=np.float32), {})     # three inputs, one output
    netcdf3.write(path_out, {"n": 12, "chan": 1, "y": 64, "x": 64}, variables)


@pytest.mark.parametrize("method", ["unet", "var", "linear"])
def test_the_command_for_every_other_model_class(data, method):
    """the command on a unet, var and linear model folder and an unscored test file: the JSON, the report section and, with
    --importance-maps, the map page; `fixed` moves nothing in any of them"""
    from cae_tools_amd.cli import importance as cli, train_cae
    (root, paths) = data
    extra = []
    if method == "unet":       # a UNET's layers come from a definitions file
        from cae_tools_amd.models.unet import unet_layer_spec
        paths = {part: str(root / f"square_{part}.nc") for part in ("train", "test")}
        for part in paths:
            _square(data[1][part], paths[part])
        layers = str(root / "unet_layers.json")
        with open(layers, "w") as f:
            json.dump(unet_layer_spec(3, 1, (64, 64), [8, 16]).save(), f)
        extra = ["--layer-definitions-path", layers, "--mask-variable", "valid"]
    model_dir = str(root / f"model_{method}")
    out = str(root / f"report_{method}")
    torch.manual_seed(0)
    log = io.StringIO()
    with redirect_stdout(log):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model_dir,
                        "--input-variables", *VARIABLES, "--output-variable", "hires", "--method", method, "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"] + extra)
        cli.main(["--test-inputs", paths["test"], "--model-folder", model_dir, "--output-html-folder", out, "--importance-repeats", "2",
                  "--importance-seed", "3", "--importance-groups", "lowres,noise", "fixed", "--importance-maps"])
    with open(os.path.join(out, "importance_test.json")) as f:
        rec = json.load(f)
    side = 64 if method == "unet" else 256
    assert (rec["n_cases"], rec["repeats"], rec["seed"], rec["n_groups"]) == (12, 2, 3, 2)
    (both, fixed) = rec["groups"]
    assert both["name"] == "lowres+noise" and both["pairs"] == 2 * 12 * side * side and both["sensitivity"] > 0.0
    assert fixed["importance"] == 0.0 and fixed["sensitivity"] == 0.0 and fixed["pixels_grew_count"] == 0
    assert fixed["pixels_shrank_count"] == 0 and fixed["mse_permuted"] == fixed["mse_base"] == both["mse_base"]
    assert [line for line in log.getvalue().splitlines() if line.startswith("importance test: 2 groups x 2 permutations of 12 cases")]
    with open(os.path.join(out, "index.html")) as f:
        assert f.read().count("<h2>Input importance</h2>") == 1
    assert os.path.exists(os.path.join(out, "importance", "index.html")) and os.path.exists(os.path.join(out, "importance", "test_group1.png"))
