"""cae_case_spectra on the GPU: the four binned spectral sums per case against the numpy restatement of the definition
(spectra_ref.py, np.fft.rfft2 in fp64) within the derived bound 4 (H + W + 16) 2^-53 L1(x') L1(y') modes_b, with counted
exact, for every element kind, plane shape, band cut, alignment and non-finite value; then train_cae -> apply_cae ->
spectra with every file it writes compared.

Largest |got - want| / bound measured on an MI355X (each check prints its figure before it asserts): 1.8e-2 at 3 x 5,
7.1e-4 at 17 x 19, 1.7e-4 at 16 x 64, 1.5e-5 at 33 x 128 and 81 x 81, 4.6e-7 at 256 x 256, 8.5e-7 at 2048 x 6."""
import io
import json
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import spectra_ref
from spectra_ref import Reference, channel0
from cae_tools_amd import _lib
from cae_tools_amd.engine import case_spectra
from cae_tools_amd.utils import spectra

pytestmark = pytest.mark.gpu

ERR_ARG = -1        # CAE_ERR_ARG of include/cae_hip.h


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
    """290 + 5 U fp32 targets (two channels), p = a + eps N(0, 1) in fp64 (one channel) and their fp32 / fp64 partners"""
    a32 = (290 + 5 * rng.random((n, 2) + shape)).astype(np.float32)
    p64 = a32[:, :1].astype(np.float64) + eps * rng.standard_normal((n, 1) + shape)
    (p32, a64) = (p64.astype(np.float32), a32.astype(np.float64) + 1e-3 * rng.random(a32.shape))
    return p64, p32, a64, a32


@pytest.mark.parametrize("eps", [0.5, 1e-6])
@pytest.mark.parametrize("n_case", [1, 3, 7])
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 5), (17, 19), (16, 64), (64, 16), (33, 128)])
def test_every_kind_matches_the_definition(tmp_path, shape, n_case, eps):
    rng = np.random.default_rng(shape[0] * 100 + n_case)
    (p64, p32, a64, a32) = _operands(rng, n_case, shape, eps)
    (p64be, a32be) = _netcdf_slabs(tmp_path, "p64_a32", p64, a32)
    (p32be, a64be) = _netcdf_slabs(tmp_path, "p32_a64", p32, a64)
    dev = torch.device("cuda")
    refs = {}
    m = max(1, min(shape) // 2)
    for (p, a, pn, an) in [(p64, a32, p64, a32), (p32, a64, p32, a64), (p64be, a32be, p64, a32), (p32be, a64be, p32, a64),
                           (p64be, a64, p64, a64), (p32, a32be, p32, a32),
                           (torch.from_numpy(p64).to(dev), a32be, p64, a32),
                           (torch.from_numpy(p32).to(dev), torch.from_numpy(a32).to(dev), p32, a32)]:
        key = (id(pn), id(an))
        if key not in refs:
            refs[key] = Reference(channel0(pn), channel0(an))
        (sums, counted) = case_spectra(p, a)
        assert sums.shape == (n_case, m, 4) and counted.shape == (n_case,) and counted.dtype == bool
        refs[key].check(sums, counted, f"eps={eps}")
        assert counted.all()
        if shape in ((1, 1), (2, 2)):           # every mode is left out
            assert (sums == 0.0).all() and not np.signbit(sums).any()


# the band and LDS limits: 256 x 256 (one pass of 256 ky, 4 columns a band, the staging in the tile's place); more than one
# pass (300), two columns a band (600) and one (2048, the largest tile, above the 64 KiB a kernel gets without asking);
# the widest plane (2048 columns, 257 bands); 81 x 81, odd on both sides
@pytest.mark.parametrize("shape,eps", [((256, 256), 0.5), ((256, 256), 1e-6), ((81, 81), 0.5), ((300, 12), 0.5),
                                       ((600, 10), 1e-6), ((2048, 6), 0.5), ((6, 2048), 1e-6)])
def test_band_and_lds_limits(shape, eps):
    rng = np.random.default_rng(shape[0])
    (p64, p32, a64, a32) = _operands(rng, 1, shape, eps)
    Reference(channel0(p32), channel0(a32)).check(*case_spectra(torch.from_numpy(p32).cuda(), torch.from_numpy(a32).cuda()),
                                                 f"fp32 eps={eps}")
    Reference(channel0(p64), channel0(a32)).check(*case_spectra(p64, a32), f"fp64/fp32 eps={eps}")


def _raw(p_dev, pk, p_off, ps, a_dev, ak, a_off, as_, n, h, w, wy, wx, table, n_bin):
    """cae_case_spectra on element offsets into flat device buffers (case starts of any alignment), with -7.0 doubles
    around sums_dev and 0xAA bytes around counted_dev checked"""
    lib = _lib.load()
    (pe, ae) = (4 if pk in (0, 1) else 8, 4 if ak in (0, 1) else 8)
    guard = 8
    dev = p_dev.device
    out = torch.full((guard + n * n_bin * 4 + guard,), -7.0, dtype=torch.float64, device=dev)
    cnt = torch.full((guard + n + guard,), 0xAA, dtype=torch.uint8, device=dev).repeat_interleave(4).view(torch.int32)
    need = int(lib.cae_case_spectra_workspace_bytes(n, h, w, n_bin))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    wyd = torch.from_numpy(np.ascontiguousarray(wy, dtype=np.float64)).to(dev)
    wxd = torch.from_numpy(np.ascontiguousarray(wx, dtype=np.float64)).to(dev)
    tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(dev)
    _lib.check(lib.cae_case_spectra(p_dev.data_ptr() + p_off * pe, pk, ps, a_dev.data_ptr() + a_off * ae, ak, as_, n, h, w,
                                    wyd.data_ptr(), wxd.data_ptr(), tab.data_ptr(), n_bin, out.data_ptr() + 8 * guard,
                                    cnt.data_ptr() + 4 * guard, ws.data_ptr(), need, None))
    host = out.cpu().numpy()
    chost = cnt.cpu().numpy()
    filler = np.frombuffer(b"\xaa" * 4, dtype=np.int32)[0]
    assert (host[:guard] == -7.0).all() and (host[-guard:] == -7.0).all()
    assert (chost[:guard] == filler).all() and (chost[-guard:] == filler).all()
    return host[guard:-guard].reshape(n, n_bin, 4), chost[guard:-guard]


@pytest.mark.parametrize("shape,mode", [((16, 64), (3, 5)), ((64, 16), (5, 3))])
def test_orientation(shape, mode):
    """one plane wave under an all-ones window: all power lies in the bin the table gives (ky, kx), which is not the bin
    of (kx, ky) - a ky / kx or H / W swap puts it elsewhere"""
    (h, w) = shape
    (ky, kx) = mode
    (j, i) = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    plane = np.cos(2.0 * np.pi * (ky * j / h + kx * i / w))[None]
    table = spectra.bin_table(h, w)
    m = spectra.bin_count(h, w)
    assert 0 <= table[ky, kx] != table[kx, ky] >= 0
    dev = torch.from_numpy(plane.reshape(-1)).cuda()
    ones = dict(wy=np.ones(h), wx=np.ones(w))
    (sums, counted) = _raw(dev, _lib.ELEM_F64, 0, h * w, dev, _lib.ELEM_F64, 0, h * w, 1, h, w, ones["wy"], ones["wx"], table, m)
    assert counted.tolist() == [1]
    ref = Reference(plane, plane, **ones)
    ref.check(sums, counted, "plane wave")
    power = 2.0 * (h * w / 2.0) ** 2
    for k in range(3):
        assert abs(sums[0, table[ky, kx], k] - power) <= ref.bound[0, table[ky, kx], k] + 1e-12 * power
        others = np.delete(sums[0, :, k], table[ky, kx])
        assert (np.abs(others) <= np.delete(ref.bound[0, :, k], table[ky, kx]) + 1e-20 * power).all()
    assert (sums[0, :, 3] == 0.0).all()           # d = 0 exactly


@pytest.mark.parametrize("offsets", [(0, 1), (1, 3), (2, 2), (3, 0)])
@pytest.mark.parametrize("strides", [(1, 5), (5, 1)])
def test_unaligned_case_starts_and_strides(offsets, strides):
    """fp32 cases that start at element offsets 0 - 3 with strides plane + 1 and plane + 5, against fp32 and fp64 targets;
    a table entry that is no bin (>= n_bin) is left out like -1 and not indexed with"""
    (h, w, n) = (17, 19, 5)
    plane = h * w
    rng = np.random.default_rng(offsets[0] * 4 + offsets[1])
    (po, ao) = offsets
    (sp, sa) = (plane + strides[0], plane + strides[1])
    pf = (290 + 5 * rng.random(po + n * sp)).astype(np.float32)
    af = (290 + 5 * rng.random(ao + n * sa)).astype(np.float32)
    a64 = 290 + 5 * rng.random(ao + n * sa)
    cases = lambda buf, off, st: np.stack([buf[off + k * st: off + k * st + plane] for k in range(n)]).reshape(n, h, w)  # noqa: E731
    (pd, ad, a64d) = (torch.from_numpy(pf).cuda(), torch.from_numpy(af).cuda(), torch.from_numpy(a64).cuda())
    table = spectra.bin_table(h, w)
    m = spectra.bin_count(h, w)
    wild = table.copy()
    wild[5, 3] = m
    wild[9, 9] = 2 ** 31 - 1
    wild[2, 0] = -5
    for (adev, ak, abuf) in ((ad, _lib.ELEM_F32, af), (a64d, _lib.ELEM_F64, a64)):
        for tab in (table, wild):
            (sums, counted) = _raw(pd, _lib.ELEM_F32, po, sp, adev, ak, ao, sa, n, h, w, spectra.window(h), spectra.window(w), tab, m)
            Reference(cases(pf, po, sp), cases(abuf, ao, sa), table=tab, n_bin=m).check(sums, counted, "raw")
            assert counted.tolist() == [1] * n


def test_bad_arguments_write_nothing():
    lib = _lib.load()
    (n, h, w) = (3, 17, 19)
    plane = h * w
    m = spectra.bin_count(h, w)
    p = torch.rand(n * plane + 4, dtype=torch.float32, device="cuda")
    a = torch.rand(n * plane + 4, dtype=torch.float64, device="cuda")
    wy = torch.from_numpy(spectra.window(h)).cuda()
    wx = torch.from_numpy(spectra.window(w)).cuda()
    tab = torch.from_numpy(spectra.bin_table(h, w)).cuda()
    out = torch.full((16 + n * m * 4,), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((16 + n,), -7, dtype=torch.int32, device="cuda")
    need = int(lib.cae_case_spectra_workspace_bytes(n, h, w, m))
    assert need >= (2 * (h + w) + 4 * n + n * m * 4) * 8
    ws = torch.full((need // 8 + 2,), -7.0, dtype=torch.float64, device="cuda")
    good = dict(p=p.data_ptr(), pk=_lib.ELEM_F32, ps=plane, a=a.data_ptr(), ak=_lib.ELEM_F64, as_=plane, n=n, h=h, w=w,
                wy=wy.data_ptr(), wx=wx.data_ptr(), tab=tab.data_ptr(), m=m, out=out.data_ptr() + 64, cnt=cnt.data_ptr() + 32,
                ws=ws.data_ptr(), ws_bytes=need)

    def call(**change):
        v = {**good, **change}
        return lib.cae_case_spectra(v["p"], v["pk"], v["ps"], v["a"], v["ak"], v["as_"], v["n"], v["h"], v["w"], v["wy"], v["wx"],
                                    v["tab"], v["m"], v["out"], v["cnt"], v["ws"], v["ws_bytes"], None)

    for change in (dict(pk=4), dict(pk=-1), dict(ak=4), dict(ak=-1), dict(n=-1), dict(h=0), dict(h=2049), dict(w=0),
                   dict(w=2049), dict(h=-3), dict(m=0), dict(m=-2), dict(ws_bytes=need - 8), dict(ws_bytes=0),
                   dict(ps=plane - 1), dict(as_=plane - 1),
                   dict(p=None), dict(a=None), dict(wy=None), dict(wx=None), dict(tab=None), dict(out=None), dict(cnt=None),
                   dict(ws=None),
                   dict(p=good["p"] + 2), dict(a=good["a"] + 4), dict(wy=good["wy"] + 4), dict(wx=good["wx"] + 4),
                   dict(tab=good["tab"] + 2), dict(out=good["out"] + 4), dict(cnt=good["cnt"] + 2), dict(ws=good["ws"] + 8)):
        assert call(**change) == ERR_ARG, change
    for bad in ((0, h, w, m), (n, 0, w, m), (n, 2049, w, m), (n, h, 0, m), (n, h, 2049, m), (n, h, w, 0)):
        assert lib.cae_case_spectra_workspace_bytes(*bad) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (cnt.cpu().numpy() == -7).all() and (ws.cpu().numpy() == -7.0).all()
    # no case: nothing written, no pointer needed
    _lib.check(call(n=0))
    _lib.check(lib.cae_case_spectra(None, 0, plane, None, 0, plane, 0, h, w, None, None, None, m, None, None, None, 0, None))
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (cnt.cpu().numpy() == -7).all() and (ws.cpu().numpy() == -7.0).all()
    # and the same call with good arguments writes both outputs whole and nothing around them
    _lib.check(call())
    (host, chost) = (out.cpu().numpy(), cnt.cpu().numpy())
    assert (host[:8] == -7.0).all() and (host[8 + n * m * 4:] == -7.0).all()
    assert (chost[:8] == -7).all() and (chost[8 + n:] == -7).all() and (ws.cpu().numpy()[need // 8:] == -7.0).all()
    Reference(p.cpu().numpy()[:n * plane].reshape(n, h, w), a.cpu().numpy()[:n * plane].reshape(n, h, w)).check(
        host[8:8 + n * m * 4].reshape(n, m, 4), chost[8:8 + n], "after the refusals")


def test_non_finite_cases_are_not_counted():
    rng = np.random.default_rng(5)
    (p64, p32, a64, a32) = _operands(rng, 5, (17, 19), 0.5)
    (p, a) = (p64.copy(), a32.copy())
    p[1, 0, 10, 3] = np.nan
    a[3, 0, 16, 18] = np.inf
    a[2, 1, 0, 0] = np.nan                  # channel 1 is not read
    (sums, counted) = case_spectra(p, a)
    assert counted.tolist() == [True, False, True, False, True]
    assert (sums[[1, 3]] == 0.0).all() and not np.signbit(sums[[1, 3]]).any() and np.isfinite(sums).all()
    Reference(channel0(p), channel0(a)).check(sums, counted, "non-finite")
    # the other cases are what they are without the bad ones, bit for bit
    (clean, counted_clean) = case_spectra(p[[0, 2, 4]], a[[0, 2, 4]])
    assert counted_clean.all() and sums[[0, 2, 4]].tobytes() == clean.tobytes()
    # -Inf in the prediction, big-endian slab kinds and fp32 alike
    q = p32.copy()
    q[4, 0, 0, 0] = -np.inf
    (sums, counted) = case_spectra(q.astype(">f4"), a64.astype(">f8"))
    assert counted.tolist() == [True, True, True, True, False] and (sums[4] == 0.0).all()


def test_two_runs_and_two_cuts_agree_bit_for_bit():
    rng = np.random.default_rng(11)
    (p64, p32, a64, a32) = _operands(rng, 7, (33, 128), 0.5)
    (p, a) = (torch.from_numpy(p64).cuda(), torch.from_numpy(a32).cuda())
    (first, counted) = case_spectra(p, a)
    (second, _) = case_spectra(p.clone(), a.clone())
    assert first.tobytes() == second.tobytes() and counted.all()
    (head, _) = case_spectra(p[:3], a[:3])
    (tail, _) = case_spectra(p[3:], a[3:])
    assert first.tobytes() == np.concatenate([head, tail]).tobytes()


# ---- train_cae -> apply_cae -> spectra ---------------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 circle cases per partition, the smallest set datagen makes"""
    from cae_tools_amd.data import datagen
    root = tmp_path_factory.mktemp("spectra")
    paths = {}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        paths[part] = str(root / f"{part}.nc")
        datagen.generate("circle", 12, seed=seed).to_netcdf(paths[part])
    return root, paths


def _check_outputs(folder, held_by, log):
    """the files of one spectra run against the definition.  held_by: {partition: (prediction, target)}, (N, C, H, W) arrays"""
    with open(os.path.join(folder, "index.html")) as f:
        assert f.read().count('href="spectra/index.html"') == 1
    with open(os.path.join(folder, "spectra", "index.html")) as f:
        page = f.read()
    assert sorted(f for f in os.listdir(folder) if f.startswith("spectra_")) == sorted(f"spectra_{p}.json" for p in held_by)
    for (partition, (pred, target)) in held_by.items():
        with open(os.path.join(folder, f"spectra_{partition}.json")) as f:
            rec = json.load(f)
        (n, h, w) = (pred.shape[0], pred.shape[2], pred.shape[3])
        assert (rec["n_cases"], rec["n_counted"], rec["h"], rec["w"]) == (n, n, h, w)
        (want, tol) = spectra_ref.curves(Reference(channel0(pred), channel0(target)))
        for name in ("modes", "wavelength"):
            assert rec[name] == want[name].tolist()
        for name in ("psd_pred", "psd_target", "power_ratio", "coherence", "error_share"):
            got = np.array([np.nan if v is None else v for v in rec[name]])
            assert np.isnan(got).tolist() == np.isnan(want[name]).tolist(), name
            ok = ~np.isnan(got)
            excess = float(np.max(np.abs(got - want[name])[ok] / tol[name][ok]))
            loose = int(ok.sum() - np.isfinite(tol[name][ok]).sum())
            print(f"spectra end to end {partition} {name}: max |got - want| / bound = {excess:.3e} over {int(ok.sum())} bins"
                  + (f", {loose} of them not constrained (denominator below twice its bound)" if loose else ""))
            assert (np.abs(got - want[name])[ok] <= tol[name][ok]).all(), (partition, name, excess)
        # the ratio is the quotient of the two psd curves in every bin, whatever the bound resolves: PP / AA against
        # (PP / norm) / (AA / norm) differ by the three roundings of the latter and the one of the former
        (rp, ra, rr) = (np.array([np.nan if v is None else v for v in rec[k]]) for k in ("psd_pred", "psd_target", "power_ratio"))
        ok = ~np.isnan(rr)
        assert (np.abs(rr[ok] - rp[ok] / ra[ok]) <= 4 * 2.0 ** -53 * np.abs(rr[ok])).all()
        below = [b for (b, r) in enumerate(rec["power_ratio"]) if r is not None and r < 0.5]
        er = rec["wavelength"][below[0]] if below else None
        assert rec["effective_resolution"] == er
        shown = "none" if er is None else format(er, ".6g")
        assert f"spectra {partition}: effective_resolution {shown} pixels, {n}/{n} cases" in log.splitlines()
        assert f'data-partition="{partition}"' in page
    assert page.count("<img") == 4 * len(held_by)


def test_train_apply_spectra(data):
    from cae_tools_amd.cli import apply_cae, evaluate_cae, spectra as cli, train_cae
    from cae_tools_amd.data.arrays import open_dataset
    (root, paths) = data
    model = str(root / "model")
    scored = str(root / "scored_test.nc")
    torch.manual_seed(0)
    with redirect_stdout(io.StringIO()):
        train_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                        "--input-variables", "lowres", "--output-variable", "hires", "--method", "conv", "--nr-epochs", "2",
                        "--batch-size", "6", "--latent-size", "4", "--fc-size", "16"])
        apply_cae.main([paths["test"], scored, "--model-folder", model])
    arrays = lambda ds: tuple(np.asarray(ds[v].values) for v in ("model_output", "hires"))      # noqa: E731

    out1 = str(root / "report_scored")
    log = io.StringIO()
    with redirect_stdout(log):
        cli.main(["--test-inputs", scored, "--model-folder", model, "--output-html-folder", out1])
    _check_outputs(out1, {"test": arrays(open_dataset(scored))}, log.getvalue())

    # evaluate_cae itself on the same input: no spectra files, no page, no link
    out2 = str(root / "report_plain")
    with redirect_stdout(io.StringIO()):
        evaluate_cae.main(["--test-inputs", scored, "--model-folder", model, "--output-html-folder", out2])
    assert not os.path.exists(os.path.join(out2, "spectra"))
    assert not [f for f in os.listdir(out2) if f.startswith("spectra_")]
    with open(os.path.join(out2, "index.html")) as f:
        plain = f.read()
    with open(os.path.join(out1, "index.html")) as f:
        linked = f.read()
    assert "spectra/index.html" not in plain and len(linked.splitlines()) == len(plain.splitlines()) + 3
