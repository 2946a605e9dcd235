"""cae_case_baseline on the GPU: the six per-case sums and the interpolated field against the numpy restatement of the
definition (baseline_ref.py, np.longdouble) - n and n_won exactly, the field within 32 2^-53 S|w||v| per pixel, the sums
within the bounds derived from that - for every mode, shape, band and strip cut, element kind, alignment and non-finite
value; then train_cae -> apply_cae -> baseline with every output compared.

Largest |got - want| / bound measured on an MI355X (each check prints its figure before it asserts): the field 0.17 (bicubic,
(200, 150) -> (65, 129)), 0.099 bilinear, 0 nearest; the sums 0.13 at (3, 3) -> (3, 3) in every mode (b = low exactly there:
the accumulation alone), 1.9e-3 with unaligned case starts, 1.7e-3 with NaN, +-Inf and an all-NaN case; end to end the
per-case skill 2.9e-5 and baseline_mse 7.5e-5 of their bounds.  n and n_won are exact everywhere."""
import io
import json
import math
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import baseline_ref
from baseline_ref import Reference, channel0
from cae_tools_amd import _lib
from cae_tools_amd.engine import case_baseline, device_operand, upsample
from cae_tools_amd.utils import baseline

pytestmark = pytest.mark.gpu

ERR_ARG = -1        # CAE_ERR_ARG of include/cae_hip.h
MODES = ("nearest", "bilinear", "bicubic")


def _netcdf_slabs(tmp_path, name, low, p, a):
    """the three written to a NetCDF-3 file and read back as the big-endian views of its mapping that the loader hands on"""
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import as_numpy, open_dataset
    dims = {"n": p.shape[0], "cl": low.shape[1], "yl": low.shape[2], "xl": low.shape[3], "c": p.shape[1], "ca": a.shape[1],
            "y": p.shape[2], "x": p.shape[3]}
    path = str(tmp_path / f"{name}.nc")
    netcdf3.write(path, dims, {"low": (("n", "cl", "yl", "xl"), low, {}), "pred": (("n", "c", "y", "x"), p, {}),
                               "target": (("n", "ca", "y", "x"), a, {})})
    ds = open_dataset(path)
    out = [as_numpy(ds[k]) for k in ("low", "pred", "target")]
    assert all(v.dtype.byteorder == ">" for v in out)
    return out


def _operands(rng, n, in_shape, out_shape, channels=(1, 1, 1)):
    """seeded continuous fields around 290 K: low (N, cl, h, w), a (N, ca, H, W) and p = a + noise (N, cp, H, W), fp64"""
    low = 290.0 + 5.0 * rng.random((n, channels[0]) + in_shape)
    a = 290.0 + 5.0 * rng.random((n, channels[2]) + out_shape)
    p = a[:, :1] + 2.0 * rng.standard_normal((n, 1) + out_shape)
    if channels[1] > 1:
        p = np.concatenate([p, rng.random((n, channels[1] - 1) + out_shape)], axis=1)
    return low, p, a


_REFS = {}


def _ref(key, low, p, a, mode):
    """one Reference per (key, mode), shared by the checks that use the same values"""
    if (key, mode) not in _REFS:
        _REFS[(key, mode)] = Reference(channel0(low), None if p is None else channel0(p), channel0(a), mode)
    return _REFS[(key, mode)]


SHAPES = [((1, 1), (1, 1)), ((1, 1), (3, 5)), ((2, 3), (7, 5)), ((3, 3), (3, 3)), ((4, 4), (64, 64)), ((5, 7), (33, 130)),
          ((63, 64), (127, 129)), ((9, 9), (4, 4))]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_case", [1, 3])
@pytest.mark.parametrize("shapes", SHAPES)
def test_shapes_and_modes(shapes, n_case, mode):
    (i, o) = shapes
    rng = np.random.default_rng(i[0] * 1000 + o[1] * 10 + n_case)
    (low, p, a) = _operands(rng, n_case, i, o)
    ref = Reference(channel0(low), channel0(p), channel0(a), mode)
    (sums, field) = case_baseline(low, p, a, mode=mode, field=True)
    ref.check(sums, f"{i}->{o}")
    ref.check_field(field, f"{i}->{o}")
    assert case_baseline(low, p, a, mode=mode).tobytes() == sums.tobytes()         # the field output changes no sum
    if i == o:                                  # identity: the field is low, and pred = low never wins
        assert field.tobytes() == channel0(low).tobytes()
        same = case_baseline(low, low, a, mode=mode)
        assert (same[:, 5] == 0).all() and np.array_equal(same[:, 1], same[:, 3]) and np.array_equal(same[:, 2], same[:, 4])
        assert upsample(low, o, mode).tobytes() == channel0(low).tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_benchmark_shape(mode):
    rng = np.random.default_rng(17)            # seed 16 has an fp32 pixel with |p - a| == |b - a|: undecided
    (low, p, a) = _operands(rng, 1, (16, 16), (256, 256))
    (low32, p32, a32) = (low.astype(np.float32), p.astype(np.float32), a.astype(np.float32))
    ref = Reference(channel0(low32), channel0(p32), channel0(a32), mode)
    (sums, field) = case_baseline(torch.from_numpy(low32).cuda(), torch.from_numpy(p32).cuda(), torch.from_numpy(a32).cuda(),
                                  mode=mode, field=True)
    ref.check(sums, "16x16->256x256 fp32")
    ref.check_field(field, "16x16->256x256 fp32")
    assert upsample(low32, (256, 256), mode).tobytes() == field.tobytes()


# output sizes on both sides of the band cut (64 output rows) and of the strip cuts (64 and 128 output columns), the input
# small (every ring slot refreshed a few times per band) and large (a downscale: every row refreshes the whole ring)
@pytest.mark.parametrize("shapes", [((3, 5), (63, 63)), ((3, 5), (64, 64)), ((3, 5), (65, 65)), ((7, 3), (128, 64)),
                                    ((7, 3), (129, 128)), ((200, 150), (65, 129)), ((70, 2), (66, 1)), ((2, 70), (1, 193))])
def test_band_and_strip_cuts(shapes):
    (i, o) = shapes
    rng = np.random.default_rng(i[0] * 7 + o[1])
    (low, p, a) = _operands(rng, 2, i, o)
    (ld, pd, ad) = (device_operand(low), device_operand(p), device_operand(a))
    for mode in MODES:
        ref = Reference(channel0(low), channel0(p), channel0(a), mode)
        (sums, field) = case_baseline(ld, pd, ad, mode=mode, field=True)
        ref.check(sums, f"cuts {i}->{o}")
        ref.check_field(field, f"cuts {i}->{o}")


@pytest.mark.parametrize("mode", MODES)
def test_every_operand_in_every_kind(tmp_path, mode):
    """each operand independently as fp32, fp64, big-endian fp32 and fp64 NetCDF-3 slabs and torch device tensors; channel 0 of
    operands with more channels"""
    rng = np.random.default_rng(8)
    (low64, p64, a64) = _operands(rng, 3, (5, 7), (33, 70), channels=(2, 3, 2))
    (low32, p32, a32) = (low64.astype(np.float32), p64.astype(np.float32), a64.astype(np.float32))
    (low64be, p64be, a64be) = _netcdf_slabs(tmp_path, "f64", low64, p64, a64)
    (low32be, p32be, a32be) = _netcdf_slabs(tmp_path, "f32", low32, p32, a32)
    dev = torch.device("cuda")
    t = lambda x: torch.from_numpy(x).to(dev)           # noqa: E731
    lows = {"f64": (low64, low64), "f32": (low32, low32), "f64be": (low64be, low64), "f32be": (low32be, low32), "t32": (t(low32), low32)}
    preds = {"f64": (p64, p64), "f32": (p32, p32), "f64be": (p64be, p64), "f32be": (p32be, p32), "t64": (t(p64), p64)}
    acts = {"f64": (a64, a64), "f32": (a32, a32), "f64be": (a64be, a64), "f32be": (a32be, a32), "t32": (t(a32), a32)}
    base = ("f64", "f32", "f32be")
    combos = [(k, base[1], base[2]) for k in lows] + [(base[0], k, base[2]) for k in preds] + [(base[0], base[1], k) for k in acts]
    combos += [("f32be", "f64be", "f64be"), ("t32", "t64", "t32")]
    for (kl, kp, ka) in combos:
        ((lo, lv), (p, pv), (a, av)) = (lows[kl], preds[kp], acts[ka])
        ref = _ref((id(lv), id(pv), id(av)), lv, pv, av, mode)
        (sums, field) = case_baseline(lo, p, a, mode=mode, field=True)
        ref.check(sums, f"{kl}/{kp}/{ka}")
        ref.check_field(field, f"{kl}/{kp}/{ka}")


def _raw(low, lk, l_off, ls, in_shape, p, pk, p_off, ps, a, ak, a_off, as_, n, out_shape, mode, with_field=True):
    """cae_case_baseline on element offsets into flat device buffers (case starts of any alignment), with -7.0 doubles
    around sums_dev, field_dev and behind the workspace checked"""
    lib = _lib.load()
    eb = lambda k: 4 if k in (0, 1) else 8              # noqa: E731
    guard = 8
    (h, w) = out_shape
    out = torch.full((guard + n * 6 + guard,), -7.0, dtype=torch.float64, device="cuda")
    fld = torch.full((guard + n * h * w + guard,), -7.0, dtype=torch.float64, device="cuda")
    need = int(lib.cae_case_baseline_workspace_bytes(n, h, w))
    assert need > 0 and need % 8 == 0
    ws = torch.full((need // 8 + guard,), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.cae_case_baseline(low.data_ptr() + l_off * eb(lk), lk, ls, in_shape[0], in_shape[1],
                                     p.data_ptr() + p_off * eb(pk) if p is not None else None, pk, ps,
                                     a.data_ptr() + a_off * eb(ak), ak, as_, n, h, w, baseline.MODES[mode],
                                     out.data_ptr() + 8 * guard, fld.data_ptr() + 8 * guard if with_field else None,
                                     ws.data_ptr(), need, None))
    (host, fh) = (out.cpu().numpy(), fld.cpu().numpy())
    assert (host[:guard] == -7.0).all() and (host[-guard:] == -7.0).all()
    assert (fh[:guard] == -7.0).all() and (fh[-guard:] == -7.0).all()
    assert (ws.cpu().numpy()[need // 8:] == -7.0).all()
    if not with_field:
        assert (fh == -7.0).all()
    return host[guard:-guard].reshape(n, 6), fh[guard:-guard].reshape(n, h, w)


@pytest.mark.parametrize("offsets", [(0, 1, 3), (1, 3, 2), (3, 2, 1)])
def test_unaligned_case_starts_and_strides(offsets):
    """cases that start at odd element offsets with strides larger than the plane, fp32 and fp64 operands"""
    (n, i, o) = (4, (5, 6), (23, 67))
    (pl_in, pl) = (i[0] * i[1], o[0] * o[1])
    rng = np.random.default_rng(sum(offsets))
    (lo_, po, ao) = offsets
    (sl, sp, sa) = (pl_in + 1, pl + 5, pl + 3)
    lf = (290 + 5 * rng.random(lo_ + n * sl)).astype(np.float32)
    pf = 290 + 5 * rng.random(po + n * sp)
    af = (290 + 5 * rng.random(ao + n * sa)).astype(np.float32)
    cases = lambda buf, off, st, shape: np.stack([buf[off + k * st: off + k * st + shape[0] * shape[1]]     # noqa: E731
                                                  for k in range(n)]).reshape((n,) + shape).astype(np.float64)
    (ld, pd, ad) = (torch.from_numpy(lf).cuda(), torch.from_numpy(pf).cuda(), torch.from_numpy(af).cuda())
    for mode in MODES:
        ref = Reference(cases(lf, lo_, sl, i), cases(pf, po, sp, o), cases(af, ao, sa, o), mode)
        (sums, field) = _raw(ld, _lib.ELEM_F32, lo_, sl, i, pd, _lib.ELEM_F64, po, sp, ad, _lib.ELEM_F32, ao, sa, n, o, mode)
        ref.check(sums, "raw")
        ref.check_field(field, "raw")
        (again, _) = _raw(ld, _lib.ELEM_F32, lo_, sl, i, pd, _lib.ELEM_F64, po, sp, ad, _lib.ELEM_F32, ao, sa, n, o, mode,
                          with_field=False)
        assert again.tobytes() == sums.tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_values_that_are_not_finite(mode):
    rng = np.random.default_rng(12)
    (i, o) = ((8, 9), (32, 70))
    (low, p, a) = _operands(rng, 7, i, o)
    clean = case_baseline(low, p, a, mode=mode)
    (low, p, a) = (low.copy(), p.copy(), a.copy())
    (a[0, 0, 3, 4], a[0, 0, 31, 69], p[0, 0, 0, 0], p[0, 0, 5, 5]) = (np.nan, np.inf, -np.inf, np.nan)
    low[1, 0, 0, 0] = np.nan                    # a corner
    low[2, 0, 7, 4] = np.nan                    # an edge
    low[3, 0, 4, 3] = np.nan                    # the interior
    low[4] = np.nan                             # a case that is all NaN
    low[5, 0, 2, 2] = np.inf
    ref = Reference(channel0(low), channel0(p), channel0(a), mode)
    (sums, field) = case_baseline(low.astype(">f8"), p, a.astype(">f8"), mode=mode, field=True)
    ref.check(sums, "not finite")
    ref.check_field(field, "not finite")
    plane = o[0] * o[1]
    assert sums[0, 0] == plane - 4 and sums[6, 0] == plane and (sums[1:4, 0] < plane).all() and (sums[1:4, 0] > 0).all()
    assert (sums[4] == 0.0).all() and not np.signbit(sums[4]).any() and np.isnan(field[4]).all()
    assert np.isfinite(sums).all()
    assert sums[6].tobytes() == clean[6].tobytes()      # the neighbours are untouched, bit for bit
    # without a prediction: entries 3..5 are +0.0, the first three what they are with one wherever p is finite
    (none, f2) = case_baseline(low, None, a, mode=mode, field=True)
    Reference(channel0(low), None, channel0(a), mode).check(none, "no prediction")
    assert f2.tobytes() == field.tobytes()
    assert none[1:, :3].tobytes() == sums[1:, :3].tobytes() and none[0, 0] == plane - 2


def test_two_runs_and_two_cuts_agree_bit_for_bit():
    rng = np.random.default_rng(11)
    (low, p, a) = _operands(rng, 7, (6, 9), (70, 130))
    (ld, pd, ad) = (torch.from_numpy(low).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(a.astype(np.float32)).cuda())
    for mode in MODES:
        (first, f1) = case_baseline(ld, pd, ad, mode=mode, field=True)
        (second, f2) = case_baseline(ld.clone(), pd.clone(), ad.clone(), mode=mode, field=True)
        assert first.tobytes() == second.tobytes() and f1.tobytes() == f2.tobytes()
        head = case_baseline(ld[:3], pd[:3], ad[:3], mode=mode)
        tail = case_baseline(ld[3:], pd[3:], ad[3:], mode=mode)
        assert first.tobytes() == np.concatenate([head, tail]).tobytes()


def test_bad_arguments_write_nothing():
    lib = _lib.load()
    (n, hi, wi, h, w) = (3, 4, 5, 23, 70)
    (pl_in, plane) = (hi * wi, h * w)
    low = torch.rand(n * pl_in + 4, dtype=torch.float32, device="cuda")
    p = torch.rand(n * plane + 4, dtype=torch.float32, device="cuda")
    a = torch.rand(n * plane + 4, dtype=torch.float64, device="cuda")
    out = torch.full((16 + n * 6,), -7.0, dtype=torch.float64, device="cuda")
    fld = torch.full((16 + n * plane,), -7.0, dtype=torch.float64, device="cuda")
    need = int(lib.cae_case_baseline_workspace_bytes(n, h, w))
    assert need == n * 1 * 2 * 6 * 8            # one band, two strips
    ws = torch.full((need // 8 + 2,), -7.0, dtype=torch.float64, device="cuda")
    good = dict(low=low.data_ptr(), lk=_lib.ELEM_F32, ls=pl_in, hi=hi, wi=wi, p=p.data_ptr(), pk=_lib.ELEM_F32, ps=plane,
                a=a.data_ptr(), ak=_lib.ELEM_F64, as_=plane, n=n, h=h, w=w, mode=2, out=out.data_ptr() + 64,
                fld=fld.data_ptr() + 64, ws=ws.data_ptr(), ws_bytes=need)

    def call(**change):
        v = {**good, **change}
        return lib.cae_case_baseline(v["low"], v["lk"], v["ls"], v["hi"], v["wi"], v["p"], v["pk"], v["ps"], v["a"], v["ak"],
                                     v["as_"], v["n"], v["h"], v["w"], v["mode"], v["out"], v["fld"], v["ws"], v["ws_bytes"], None)

    big = 1 << 60
    for change in (dict(lk=4), dict(lk=-1), dict(pk=4), dict(pk=-1), dict(ak=4), dict(ak=-1), dict(mode=3), dict(mode=-1),
                   dict(n=-1), dict(hi=0), dict(wi=0), dict(hi=-2), dict(h=0), dict(w=0), dict(h=-3), dict(w=-1),
                   dict(h=(1 << 30) + 1), dict(wi=(1 << 30) + 1), dict(ls=-1), dict(ps=-1), dict(as_=-1),
                   dict(ls=pl_in - 1), dict(ps=plane - 1), dict(as_=plane - 1), dict(ls=big), dict(ps=big), dict(as_=big),
                   dict(ws_bytes=need - 8), dict(ws_bytes=0), dict(low=None), dict(a=None), dict(out=None), dict(ws=None),
                   dict(low=good["low"] + 2), dict(p=good["p"] + 2), dict(a=good["a"] + 4), dict(out=good["out"] + 4),
                   dict(fld=good["fld"] + 4), dict(ws=good["ws"] + 4)):
        assert call(**change) == ERR_ARG, change
    torch.cuda.synchronize()
    for t in (out, fld, ws):
        assert (t.cpu().numpy() == -7.0).all()
    # no case: nothing written, no pointer needed
    _lib.check(call(n=0))
    _lib.check(lib.cae_case_baseline(None, 0, 0, hi, wi, None, 0, 0, None, 0, 0, 0, h, w, 0, None, None, None, 0, None))
    torch.cuda.synchronize()
    for t in (out, fld, ws):
        assert (t.cpu().numpy() == -7.0).all()
    # and the same call with good arguments writes the sums and the field whole and nothing around them
    _lib.check(call())
    (host, fh) = (out.cpu().numpy(), fld.cpu().numpy())
    assert (host[:8] == -7.0).all() and (host[8 + n * 6:] == -7.0).all() and (ws.cpu().numpy()[need // 8:] == -7.0).all()
    assert (fh[:8] == -7.0).all() and (fh[8 + n * plane:] == -7.0).all()
    cut = lambda t, k, shape: t.cpu().numpy()[:n * k].reshape((n,) + shape).astype(np.float64)      # noqa: E731
    ref = Reference(cut(low, pl_in, (hi, wi)), cut(p, plane, (h, w)), cut(a, plane, (h, w)), "bicubic")
    ref.check(host[8:8 + n * 6].reshape(n, 6), "after the refusals")
    ref.check_field(fh[8:8 + n * plane].reshape(n, h, w), "after the refusals")


def test_wrapper_refusals():
    x = np.zeros((2, 1, 4, 4), dtype=np.float32)
    y = np.zeros((2, 1, 8, 8), dtype=np.float32)
    with pytest.raises(ValueError):
        case_baseline(x, y, y, mode="lanczos")
    with pytest.raises(ValueError):
        case_baseline(x, y[:1], y)
    with pytest.raises(ValueError):
        case_baseline(x[:1], y, y)
    with pytest.raises(ValueError):
        upsample(x, (0, 4))
    assert case_baseline(x[:0], None, y[:0]).shape == (0, 6)
    assert upsample(x, (8, 8), "nearest").shape == (2, 8, 8)


# ---- train_cae -> apply_cae -> baseline --------------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 circle cases per partition, the smallest set datagen makes"""
    from cae_tools_amd.data import datagen
    root = tmp_path_factory.mktemp("baseline")
    paths = {}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        paths[part] = str(root / f"{part}.nc")
        datagen.generate("circle", 12, seed=seed).to_netcdf(paths[part])
    return root, paths


def _number(v):
    return math.nan if v is None else v


def test_train_apply_baseline(data, monkeypatch):
    from cae_tools_amd.cli import apply_cae, baseline as cli, evaluate_cae, train_cae
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.models.model_evaluator import ModelEvaluator
    (root, paths) = data
    model = str(root / "model")
    scored = str(root / "scored_test.nc")
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                        "--input-variables", "lowres", "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"])
        apply_cae.main([paths["test"], scored, "--model-folder", model])
    seen = []

    class Recording(ModelEvaluator):
        def build_html(self, case_dimension, train_ds, test_ds, model_metrics):
            super().build_html(case_dimension, train_ds, test_ds, model_metrics)
            seen.append({k: np.asarray(test_ds[k].values) for k in ("baseline_mse", "skill", "mse")})

    monkeypatch.setattr(evaluate_cae, "ModelEvaluator", Recording)
    out1 = str(root / "report_scored")
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["--test-inputs", scored, "--model-folder", model, "--output-html-folder", out1, "--baseline-mode", "bilinear"])
    monkeypatch.undo()
    variables = seen[0]

    ds = open_dataset(scored)
    (low, pred, target) = (np.asarray(ds["lowres"].values), np.asarray(ds["model_output"].values), np.asarray(ds["hires"].values))
    (n, h, w) = (pred.shape[0], pred.shape[2], pred.shape[3])
    assert (n, h, w) == (12, 256, 256) and low.shape[2:] == (16, 16)
    ref = Reference(channel0(low), channel0(pred), channel0(target), "bilinear")
    assert ref.undecided == 0
    want = baseline.summary(ref.sums, "bilinear", "lowres", (16, 16), (h, w))
    assert sorted(f for f in os.listdir(out1) if f.startswith("baseline_")) == ["baseline_test.json"]
    with open(os.path.join(out1, "baseline_test.json")) as f:
        rec = json.load(f)
    for k in ("mode", "variable", "in_shape", "out_shape", "n_cases", "n_counted", "pixels_counted", "pixels_left_out", "case_pixels"):
        assert rec[k] == want[k], k
    assert rec["pixels_counted"] == n * h * w
    # a quotient of two sums moves by at most the sum of their relative bounds (and a rounding or two)
    rel = lambda k: ref.bound[:, k] / ref.sums[:, k] + 4 * baseline_ref.U         # noqa: E731
    got_skill = np.array([_number(v) for v in rec["case_skill"]])
    got_bmse = np.array([_number(v) for v in rec["case_baseline_mse"]])
    want_skill = np.asarray(want["case_skill"])
    tol_skill = (rel(2) + rel(4)) * np.abs(1.0 - want_skill) + 4 * baseline_ref.U
    print(f"baseline end to end: max |skill - want| / bound = {float(np.max(np.abs(got_skill - want_skill) / tol_skill)):.3e}, "
          f"max |baseline_mse - want| / bound = "
          f"{float(np.max(np.abs(got_bmse - want['case_baseline_mse']) / (rel(2) * np.asarray(want['case_baseline_mse'])))):.3e}")
    assert (np.abs(got_skill - want_skill) <= tol_skill).all()
    assert (np.abs(got_bmse - want["case_baseline_mse"]) <= rel(2) * np.asarray(want["case_baseline_mse"])).all()
    pooled_tol = (ref.bound[:, 2].sum() / ref.sums[:, 2].sum() + ref.bound[:, 4].sum() / ref.sums[:, 4].sum() + 64 * baseline_ref.U) \
        * abs(1.0 - want["pooled_skill"]) + 4 * baseline_ref.U
    assert abs(rec["pooled_skill"] - want["pooled_skill"]) <= pooled_tol
    assert rec["case_win_fraction"] == want["case_win_fraction"] and rec["win_fraction"] == want["win_fraction"]
    assert rec["mean_skill"] == float(np.mean(got_skill)) and rec["median_skill"] == float(np.median(got_skill))
    assert rec["skill_positive"] == float(np.mean(got_skill > 0))
    assert np.array_equal(variables["skill"], got_skill) and np.array_equal(variables["baseline_mse"], got_bmse)
    # the model's mse on the same pixels is the evaluator's mse where every pixel counts
    assert np.allclose(rec["case_model_mse"], variables["mse"], rtol=1e-12, atol=0)
    better = int(np.sum(got_skill > 0))
    line = (f"baseline test: bilinear of lowres, pooled skill {rec['pooled_skill']:.6g} (baseline mse {rec['baseline_mse']:.6g}, "
            f"model mse {rec['model_mse']:.6g}), {better}/{n} cases better")
    assert line in log.getvalue().splitlines()
    with open(os.path.join(out1, "index.html")) as f:
        page = f.read()
    assert page.count("Skill against interpolation") == 1
    assert f"test: bilinear interpolation of lowres, 16 x 16 to 256 x 256, {n} of {n} cases" in page
    assert page.count('alt="test skill histogram"') == 1
    for v in (rec["pooled_skill"], rec["mean_skill"], rec["baseline_mse"]):
        assert f"<td>{v:.6g}</td>" in page

    # a variable that is not in the data set is named
    with pytest.raises(ValueError, match="no_such_variable"):
        with redirect_stdout(io.StringIO()):
            cli.main(["--test-inputs", scored, "--model-folder", model, "--output-html-folder", str(root / "report_bad"),
                      "--baseline-variable", "no_such_variable"])

    # evaluate_cae itself on the same input: no baseline file, no section, and the page it has always written
    out2 = str(root / "report_plain")
    plain_log = io.StringIO()
    with redirect_stdout(plain_log):
        evaluate_cae.main(["--test-inputs", scored, "--model-folder", model, "--output-html-folder", out2])
    assert not [f for f in os.listdir(out2) if f.startswith("baseline_")]
    assert "baseline" not in plain_log.getvalue()
    with open(os.path.join(out2, "index.html")) as f:
        plain = f.read()
    assert "Skill against interpolation" not in plain and "skill histogram" not in plain
    # the page with the option is the plain page plus the section
    start = page.index("<h2>Skill against interpolation</h2>")
    end = page.index("<h2>Training Summary</h2>")
    assert page[:start] + page[end:] == plain
