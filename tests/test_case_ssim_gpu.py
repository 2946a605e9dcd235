"""cae_case_ssim on the GPU: {n, S ssim, S cs} per case and scale against the numpy restatement of the definition
(ssim_ref.py, np.longdouble) - n exactly, the sums within the derived bound 64 2^-53 S_w (M2 / D2 [+ M1 / D1]) + n 2^-53 S|t| -
for every element kind, plane shape, band and strip cut, alignment and non-finite value; exact ones for identical operands;
then train_cae -> apply_cae -> ssim with every output compared.

Largest |got - want| / bound measured on an MI355X (each check prints its figure before it asserts): 2.9e-2 at
11 x 11 and 23 x 22, 1.2e-2 at 45 x 47 (1.1e-2 with NaN, +-Inf and an all-NaN case), 1.3e-2 at 161 x 161 and 177 x 161,
2.1e-3 at 256 x 256, at most 5.6e-3 at the strip and band cuts, 4.9e-3 with unaligned case starts; end to end 6.0e-3 (ssim)
and 7.1e-3 (ms_ssim).  The bound on a scale's mean was at most 6.4e-12 (256 x 256, scale 4)."""
import io
import json
import math
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import ssim_ref
from ssim_ref import Reference, channel0
from cae_tools_amd import _lib
from cae_tools_amd.engine import case_ssim
from cae_tools_amd.utils import ssim

pytestmark = pytest.mark.gpu

ERR_ARG = -1        # CAE_ERR_ARG of include/cae_hip.h
(VMIN, VMAX) = (290.0, 295.0)


def _netcdf_slabs(tmp_path, name, p, a):
    """p and a written to a NetCDF-3 file and read back as the big-endian views of its mapping that the loader hands on"""
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import as_numpy, open_dataset
    dims = {"n": p.shape[0], "c": p.shape[1], "ca": a.shape[1], "y": p.shape[2], "x": p.shape[3]}
    path = str(tmp_path / f"{name}.nc")
    netcdf3.write(path, dims, {"pred": (("n", "c", "y", "x"), p, {}), "target": (("n", "ca", "y", "x"), a, {})})
    ds = open_dataset(path)
    (pb, ab) = (as_numpy(ds["pred"]), as_numpy(ds["target"]))
    assert pb.dtype.byteorder == ">" and ab.dtype.byteorder == ">"
    return pb, ab


def _operands(rng, n, shape, eps):
    """290 + 5 U fp32 targets (two channels), p = a + 5 eps N(0, 1) in fp64 (one channel) and their fp32 / fp64 partners:
    normalised over [290, 295] the fields lie in about [0, 1]"""
    a32 = (VMIN + (VMAX - VMIN) * rng.random((n, 2) + shape)).astype(np.float32)
    p64 = a32[:, :1].astype(np.float64) + (VMAX - VMIN) * eps * rng.standard_normal((n, 1) + shape)
    (p32, a64) = (p64.astype(np.float32), a32.astype(np.float64) + 1e-3 * rng.random(a32.shape))
    return p64, p32, a64, a32


def _ref(p, a, n_scale):
    return Reference(channel0(p), channel0(a), VMIN, VMAX, n_scale)


@pytest.mark.parametrize("eps", [0.1, 1e-6])
@pytest.mark.parametrize("n_case", [1, 3, 7])
@pytest.mark.parametrize("shape,n_scale", [((10, 30), 1), ((11, 11), 1), ((12, 27), 1), ((23, 22), 2), ((45, 47), 3)])
def test_every_kind_matches_the_definition(tmp_path, shape, n_scale, n_case, eps):
    rng = np.random.default_rng(shape[0] * 100 + n_case)
    (p64, p32, a64, a32) = _operands(rng, n_case, shape, eps)
    (p64be, a32be) = _netcdf_slabs(tmp_path, "p64_a32", p64, a32)
    (p32be, a64be) = _netcdf_slabs(tmp_path, "p32_a64", p32, a64)
    dev = torch.device("cuda")
    refs = {}
    for (p, a, pn, an) in [(p64, a32, p64, a32), (p32, a64, p32, a64), (p64be, a32be, p64, a32), (p32be, a64be, p32, a64),
                           (p64be, a64, p64, a64), (p32, a32be, p32, a32),
                           (torch.from_numpy(p64).to(dev), a32be, p64, a32),
                           (torch.from_numpy(p32).to(dev), torch.from_numpy(a32).to(dev), p32, a32)]:
        key = (id(pn), id(an))
        if key not in refs:
            refs[key] = _ref(pn, an, n_scale)
        sums = case_ssim(p, a, VMIN, VMAX, n_scale=n_scale)
        assert sums.shape == (n_case, n_scale, 3)
        refs[key].check(sums, f"eps={eps}")
        want_n = [max(h - 10, 0) * max(w - 10, 0) for (h, w) in ssim.scale_shapes(*shape, n_scale)]
        assert (sums[:, :, 0] == np.array(want_n, dtype=np.float64)).all()
        if shape == (10, 30):                   # no window: exact zeros
            assert (sums == 0.0).all() and not np.signbit(sums).any()


# widths on both sides of the strip cuts (54 and 108 outputs), heights on both sides of the band cuts (12 output rows below
# 200 rows, 23 below 400, 34 above: 12, 9 * 23 = 207 and 12 * 34 = 408 outputs) and of the two thresholds themselves
@pytest.mark.parametrize("shape", [(12, 64), (12, 65), (12, 118), (12, 119), (22, 11), (23, 12), (199, 11), (200, 12),
                                   (217, 11), (218, 12), (399, 11), (400, 12), (418, 11), (419, 12), (35, 130)])
def test_strip_and_band_cuts(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    (p64, p32, a64, a32) = _operands(rng, 2, shape, 0.1)
    _ref(p32, a32, 2).check(case_ssim(torch.from_numpy(p32).cuda(), torch.from_numpy(a32).cuda(), VMIN, VMAX, n_scale=2), "fp32")
    _ref(p64, a32, 2).check(case_ssim(p64, a32, VMIN, VMAX, n_scale=2), "fp64/fp32")


@pytest.mark.parametrize("shape,n_case,eps", [((161, 161), 2, 0.1), ((177, 161), 2, 1e-6), ((256, 256), 1, 0.1)])
def test_five_scales(shape, n_case, eps):
    rng = np.random.default_rng(shape[0])
    (p64, p32, a64, a32) = _operands(rng, n_case, shape, eps)
    ref = _ref(p32, a64, 5)
    sums = case_ssim(p32, a64, VMIN, VMAX)      # n_scale None: five where min(h, w) > 160
    assert sums.shape == (n_case, 5, 3)
    ref.check(sums, f"five scales eps={eps}")
    if shape == (161, 161):
        assert (sums[:, 4, 0] == 1).all()       # exactly one window at the last scale
    got = ssim.scores_from_sums(sums, *shape)
    (_, ms, _) = ssim_ref.scores(ref.sums, *shape)
    # every factor f^w with w < 1 moves by at most w df / f: the product by the sum of those
    tol = np.zeros(n_case)
    for s in range(5):
        k = 2 if s < 4 else 1
        tol += ssim.MS_WEIGHTS[s] * ref.bound[:, s, k] / np.abs(ref.sums[:, s, k])
    assert (np.abs(got["ms_ssim"] - ms) <= (tol + 16 * ssim_ref.U) * ms).all()
    assert case_ssim(p32[:, :, :160], a64[:, :, :160], VMIN, VMAX).shape == (n_case, 1, 3)      # 160: ssim alone


@pytest.mark.parametrize("kind", ["fp32", "fp64", "fp32/fp64be"])
def test_identical_operands_give_exact_ones(kind):
    rng = np.random.default_rng(21)
    (p64, p32, a64, a32) = _operands(rng, 3, (177, 161), 0.1)
    if kind == "fp32":
        (p, a) = (torch.from_numpy(p32).cuda(), torch.from_numpy(p32.copy()).cuda())
    elif kind == "fp64":
        (p, a) = (p64, p64.copy())
    else:                                       # the same values in two kinds: fp32 is exact in fp64
        (p, a) = (p32, p32.astype(">f8"))
    sums = case_ssim(p, a, VMIN, VMAX)
    want_n = np.array([(h - 10) * (w - 10) for (h, w) in ssim.scale_shapes(177, 161, 5)], dtype=np.float64)
    assert (sums[:, :, 0] == want_n).all()
    assert (sums[:, :, 1] == sums[:, :, 0]).all() and (sums[:, :, 2] == sums[:, :, 0]).all()
    scores = ssim.scores_from_sums(sums, 177, 161)
    assert (scores["ssim"] == 1.0).all() and (scores["ms_ssim"] == 1.0).all()


def test_missing_data():
    rng = np.random.default_rng(5)
    (h, w) = (45, 47)
    (p64, p32, a64, a32) = _operands(rng, 6, (h, w), 0.1)
    (p, a) = (p64.copy(), a32.copy())
    p[1, 0, 20, 30] = np.nan                # inside
    a[3, 0, 44, 46] = np.inf                # the corner
    a[2, 1, 0, 0] = np.nan                  # channel 1 is not read
    p[4, 0] = np.nan                        # a case that is all NaN
    sums = case_ssim(p, a, VMIN, VMAX, n_scale=3)
    ref = _ref(p, a, 3)
    ref.check(sums, "missing data")
    full = [35 * 37, 13 * 14, 2 * 2]
    assert sums[[0, 2, 5], :, 0].tolist() == [full] * 3
    # scale 1 (23 x 24) holds the NaN in pixel (10, 15): 11 x 9 of the 13 x 14 positions; scale 2 (12 x 12) in pixel (5, 7),
    # under all four.  The Inf at the corner: one window at scale 0, pixel (22, 23) at scale 1, (11, 11) at scale 2
    assert sums[1, :, 0].tolist() == [35 * 37 - 121, 13 * 14 - 11 * 9, 0]
    assert sums[3, :, 0].tolist() == [35 * 37 - 1, 13 * 14 - 1, 3]
    assert (sums[4] == 0.0).all() and not np.signbit(sums[4]).any() and np.isfinite(sums).all()
    assert (sums[1, 2] == 0.0).all() and not np.signbit(sums[1, 2]).any()
    # the other cases are what they are without the bad ones, bit for bit
    clean = case_ssim(p[[0, 2, 5]], a[[0, 2, 5]], VMIN, VMAX, n_scale=3)
    assert sums[[0, 2, 5]].tobytes() == clean.tobytes()
    # -Inf in the prediction, big-endian slab kinds
    q = p32.copy()
    q[5, 0, 0, 0] = -np.inf
    sums = case_ssim(q.astype(">f4"), a64.astype(">f8"), VMIN, VMAX, n_scale=3)
    _ref(q, a64, 3).check(sums, "-inf, big-endian")
    assert sums[5, :, 0].tolist() == [35 * 37 - 1, 13 * 14 - 1, 3]


def _raw(p_dev, pk, p_off, ps, a_dev, ak, a_off, as_, n, h, w, n_scale):
    """cae_case_ssim on element offsets into flat device buffers (case starts of any alignment), with -7.0 doubles around
    sums_dev and behind the workspace checked"""
    lib = _lib.load()
    (pe, ae) = (4 if pk in (0, 1) else 8, 4 if ak in (0, 1) else 8)
    guard = 8
    dev = p_dev.device
    out = torch.full((guard + n * n_scale * 3 + guard,), -7.0, dtype=torch.float64, device=dev)
    need = int(lib.cae_case_ssim_workspace_bytes(n, h, w, n_scale))
    assert need > 0 and need % 8 == 0
    ws = torch.full((need // 8 + guard,), -7.0, dtype=torch.float64, device=dev)
    win = (_lib.C.c_double * 11)(*ssim.window().tolist())
    _lib.check(lib.cae_case_ssim(p_dev.data_ptr() + p_off * pe, pk, ps, a_dev.data_ptr() + a_off * ae, ak, as_, n, h, w, n_scale,
                                 VMIN, 1.0 / (VMAX - VMIN), win, out.data_ptr() + 8 * guard, ws.data_ptr(), need, None))
    host = out.cpu().numpy()
    assert (host[:guard] == -7.0).all() and (host[-guard:] == -7.0).all()
    assert (ws.cpu().numpy()[need // 8:] == -7.0).all()
    return host[guard:-guard].reshape(n, n_scale, 3)


@pytest.mark.parametrize("offsets", [(0, 1), (1, 3), (2, 2), (3, 0)])
@pytest.mark.parametrize("strides", [(1, 5), (5, 1)])
def test_unaligned_case_starts_and_strides(offsets, strides):
    """fp32 cases that start at element offsets 0 - 3 with strides plane + 1 and plane + 5, against fp32 and fp64 targets"""
    (h, w, n) = (23, 66, 5)
    plane = h * w
    rng = np.random.default_rng(offsets[0] * 4 + offsets[1])
    (po, ao) = offsets
    (sp, sa) = (plane + strides[0], plane + strides[1])
    pf = (VMIN + 5 * rng.random(po + n * sp)).astype(np.float32)
    af = (VMIN + 5 * rng.random(ao + n * sa)).astype(np.float32)
    a64 = VMIN + 5 * rng.random(ao + n * sa)
    cases = lambda buf, off, st: np.stack([buf[off + k * st: off + k * st + plane] for k in range(n)]).reshape(n, h, w)  # noqa: E731
    (pd, ad, a64d) = (torch.from_numpy(pf).cuda(), torch.from_numpy(af).cuda(), torch.from_numpy(a64).cuda())
    for (adev, ak, abuf) in ((ad, _lib.ELEM_F32, af), (a64d, _lib.ELEM_F64, a64)):
        sums = _raw(pd, _lib.ELEM_F32, po, sp, adev, ak, ao, sa, n, h, w, 2)
        Reference(cases(pf, po, sp), cases(abuf, ao, sa), VMIN, VMAX, 2).check(sums, "raw")


def test_bad_arguments_write_nothing():
    lib = _lib.load()
    (n, h, w, n_scale) = (3, 23, 30, 2)
    plane = h * w
    p = torch.rand(n * plane + 4, dtype=torch.float32, device="cuda")
    a = torch.rand(n * plane + 4, dtype=torch.float64, device="cuda")
    out = torch.full((16 + n * n_scale * 3,), -7.0, dtype=torch.float64, device="cuda")
    need = int(lib.cae_case_ssim_workspace_bytes(n, h, w, n_scale))
    # the planes of scale 1 (12 x 15, two fields) and one partial of three doubles per (case, scale, band, strip)
    assert need == n * (2 * 12 * 15 + 3 * (2 * 1 + 1 * 1)) * 8
    ws = torch.full((need // 8 + 2,), -7.0, dtype=torch.float64, device="cuda")
    win = (_lib.C.c_double * 11)(*ssim.window().tolist())
    good = dict(p=p.data_ptr(), pk=_lib.ELEM_F32, ps=plane, a=a.data_ptr(), ak=_lib.ELEM_F64, as_=plane, n=n, h=h, w=w,
                n_scale=n_scale, shift=0.0, scale=1.0, win=win, out=out.data_ptr() + 64, ws=ws.data_ptr(), ws_bytes=need)

    def call(**change):
        v = {**good, **change}
        return lib.cae_case_ssim(v["p"], v["pk"], v["ps"], v["a"], v["ak"], v["as_"], v["n"], v["h"], v["w"], v["n_scale"],
                                 v["shift"], v["scale"], v["win"], v["out"], v["ws"], v["ws_bytes"], None)

    for change in (dict(pk=4), dict(pk=-1), dict(ak=4), dict(ak=-1), dict(n=-1), dict(h=0), dict(h=-3), dict(w=0), dict(w=-1),
                   dict(h=16385), dict(w=16385), dict(n_scale=0), dict(n_scale=6), dict(n_scale=-1),
                   dict(shift=math.nan), dict(shift=math.inf), dict(scale=math.nan), dict(scale=-math.inf),
                   dict(ws_bytes=need - 8), dict(ws_bytes=0), dict(ps=plane - 1), dict(as_=plane - 1),
                   dict(p=None), dict(a=None), dict(win=None), dict(out=None), dict(ws=None),
                   dict(p=good["p"] + 2), dict(a=good["a"] + 4), dict(out=good["out"] + 4), dict(ws=good["ws"] + 4)):
        assert call(**change) == ERR_ARG, change
    for bad in ((0, h, w, 2), (-1, h, w, 2), (n, 0, w, 2), (n, h, 0, 2), (n, 16385, w, 2), (n, h, w, 0), (n, h, w, 6)):
        assert lib.cae_case_ssim_workspace_bytes(*bad) == 0
    assert lib.cae_case_ssim_workspace_bytes(n, 10, 30, 1) == 0         # no window, one scale: nothing to keep
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (ws.cpu().numpy() == -7.0).all()
    # no case: nothing written, no pointer needed
    _lib.check(call(n=0))
    _lib.check(lib.cae_case_ssim(None, 0, plane, None, 0, plane, 0, h, w, 2, 0.0, 1.0, None, None, None, 0, None))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (ws.cpu().numpy() == -7.0).all()
    # and the same call with good arguments writes the sums whole and nothing around them
    _lib.check(call())
    host = out.cpu().numpy()
    assert (host[:8] == -7.0).all() and (host[8 + n * n_scale * 3:] == -7.0).all() and (ws.cpu().numpy()[need // 8:] == -7.0).all()
    Reference(p.cpu().numpy()[:n * plane].reshape(n, h, w), a.cpu().numpy()[:n * plane].reshape(n, h, w), 0.0, 1.0, 2).check(
        host[8:8 + n * n_scale * 3].reshape(n, n_scale, 3), "after the refusals")
    # a plane without a window and one scale needs no workspace: NULL is taken and the zeros are written
    _lib.check(call(h=10, ps=plane, as_=plane, n_scale=1, ws=None, ws_bytes=0))
    host = out.cpu().numpy()
    assert (host[8:8 + n * 3] == 0.0).all() and (host[:8] == -7.0).all()


def test_two_runs_and_two_cuts_agree_bit_for_bit():
    rng = np.random.default_rng(11)
    (p64, p32, a64, a32) = _operands(rng, 7, (45, 130), 0.1)
    (p, a) = (torch.from_numpy(p64).cuda(), torch.from_numpy(a32).cuda())
    first = case_ssim(p, a, VMIN, VMAX, n_scale=3)
    second = case_ssim(p.clone(), a.clone(), VMIN, VMAX, n_scale=3)
    assert first.tobytes() == second.tobytes()
    head = case_ssim(p[:3], a[:3], VMIN, VMAX, n_scale=3)
    tail = case_ssim(p[3:], a[3:], VMIN, VMAX, n_scale=3)
    assert first.tobytes() == np.concatenate([head, tail]).tobytes()


def test_wrapper_refuses_a_range_without_width():
    x = np.zeros((1, 1, 12, 12), dtype=np.float32)
    with pytest.raises(ValueError):
        case_ssim(x, x, 1.0, 1.0)
    with pytest.raises(ValueError):
        case_ssim(x, x, 0.0, 1.0, n_scale=6)
    assert case_ssim(x[:0], x[:0], 0.0, 1.0).shape == (0, 1, 3)


# ---- train_cae -> apply_cae -> ssim ----------------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 circle cases per partition, the smallest set datagen makes"""
    from cae_tools_amd.data import datagen
    root = tmp_path_factory.mktemp("ssim")
    paths = {}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        paths[part] = str(root / f"{part}.nc")
        datagen.generate("circle", 12, seed=seed).to_netcdf(paths[part])
    return root, paths


def _number(v):
    return math.nan if v is None else v


def test_train_apply_ssim(data, monkeypatch):
    from cae_tools_amd.cli import apply_cae, evaluate_cae, ssim as cli, train_cae
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
            seen.append(({k: np.asarray(test_ds[k].values) for k in ("ssim", "ms_ssim", "psnr", "mse")},
                         [float(v) for v in self.model.normalisation_parameters[2:4]]))

    monkeypatch.setattr(evaluate_cae, "ModelEvaluator", Recording)
    out1 = str(root / "report_scored")
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["--test-inputs", scored, "--model-folder", model, "--output-html-folder", out1])
    monkeypatch.undo()
    (variables, (vmin, vmax)) = seen[0]

    ds = open_dataset(scored)
    (pred, target) = (np.asarray(ds["model_output"].values), np.asarray(ds["hires"].values))
    (n, h, w) = (pred.shape[0], pred.shape[2], pred.shape[3])
    assert (n, h, w) == (12, 256, 256)
    ref = Reference(channel0(pred), channel0(target), vmin, vmax, 5)
    mse = np.mean((channel0(pred) - channel0(target)) ** 2, axis=(1, 2))
    (want_ssim, want_ms, want_psnr) = ssim_ref.scores(ref.sums, h, w, mse=mse, vmin=vmin, vmax=vmax)
    assert sorted(f for f in os.listdir(out1) if f.startswith("ssim_")) == ["ssim_test.json"]
    with open(os.path.join(out1, "ssim_test.json")) as f:
        rec = json.load(f)
    assert (rec["n_cases"], rec["h"], rec["w"], rec["vmin"], rec["vmax"]) == (n, h, w, vmin, vmax)
    assert rec["scales"] == [list(s) for s in ssim_ref.scale_shapes(h, w, 5)]
    assert (rec["n_counted"], rec["n_counted_ms"]) == (n, n)
    assert rec["windows"] == ref.sums[:, :, 0].astype(np.int64).tolist()
    got_ssim = np.array([_number(v) for v in rec["case_ssim"]])
    got_ms = np.array([_number(v) for v in rec["case_ms_ssim"]])
    got_psnr = np.array([_number(v) for v in rec["case_psnr"]])
    cnt = ref.sums[:, :, 0]
    tol_ssim = ref.bound[:, 0, 1] / cnt[:, 0] + 4 * ssim_ref.U
    tol_ms = np.zeros(n)
    for s in range(5):
        k = 2 if s < 4 else 1
        assert (ref.sums[:, s, k] > 0).all()
        tol_ms += ssim.MS_WEIGHTS[s] * ref.bound[:, s, k] / ref.sums[:, s, k]
    tol_ms = (tol_ms + 16 * ssim_ref.U) * want_ms
    print(f"ssim end to end: max |ssim - want| / bound = {float(np.max(np.abs(got_ssim - want_ssim) / tol_ssim)):.3e}, "
          f"max |ms_ssim - want| / bound = {float(np.max(np.abs(got_ms - want_ms) / tol_ms)):.3e}")
    assert (np.abs(got_ssim - want_ssim) <= tol_ssim).all() and (np.abs(got_ms - want_ms) <= tol_ms).all()
    # the mse is a mean of 65536 squares in fp64: 2^-53 times their number bounds any order of the additions
    assert (np.abs(got_psnr - want_psnr) <= 10.0 / math.log(10.0) * (h * w + 8) * ssim_ref.U + 8 * ssim_ref.U * np.abs(want_psnr)).all()
    for (key, case) in (("ssim", got_ssim), ("ms_ssim", got_ms), ("psnr", got_psnr)):
        assert rec[key] == float(np.mean(case))
        assert np.array_equal(variables[key], case)             # the data set's variables are the file's arrays
    assert np.array_equal(got_psnr, 10.0 * np.log10((vmax - vmin) ** 2 / variables["mse"]))
    line = (f"ssim test: ssim {rec['ssim']:.6g} ms_ssim {rec['ms_ssim']:.6g} psnr {rec['psnr']:.6g} dB, {n}/{n} cases")
    assert line in log.getvalue().splitlines()
    with open(os.path.join(out1, "index.html")) as f:
        page = f.read()
    assert page.count("Structural similarity") == 1 and f"test: {n} of {n} cases, 5 scales" in page
    assert page.count('alt="test ssim histogram"') == 1
    for v in (rec["ssim"], rec["ms_ssim"], rec["psnr"]):
        assert f"<td>{v:.6g}</td>" in page

    # evaluate_cae itself on the same input: no ssim file, no section
    out2 = str(root / "report_plain")
    with redirect_stdout(io.StringIO()):
        evaluate_cae.main(["--test-inputs", scored, "--model-folder", model, "--output-html-folder", out2])
    assert not [f for f in os.listdir(out2) if f.startswith("ssim_")]
    with open(os.path.join(out2, "index.html")) as f:
        plain = f.read()
    assert "Structural similarity" not in plain and "ssim histogram" not in plain
