"""cae_pixel_sums on the GPU: the nine per-pixel sums over the cases against an exactly rounded numpy oracle
(skill_maps_ref.fsum_sums: every term in fp64, each pixel summed with math.fsum) within the derived bound
|got - want| <= 2 n 2^-53 S|term| and with equal counts, for every element kind, alignment, chunking and non-finite
value; then train_cae -> apply_cae -> skill_maps with every file it writes compared."""
import io
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from skill_maps_ref import MAPS, assert_maps_close, channel0, check_sums, decode_png, np_scanlines, range_rule, two_pass_maps
from cae_tools_amd import _lib
from cae_tools_amd.engine import pixel_sums

pytestmark = pytest.mark.gpu

SHIFT = 292.5


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


@pytest.mark.parametrize("n_case,case_chunk", [(1, 8), (7, 8), (37, 8), (37, 0)])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (17, 19)])
def test_every_kind_matches_the_oracle(tmp_path, shape, n_case, case_chunk):
    rng = np.random.default_rng(shape[0] * 100 + n_case)
    (n, channels) = (n_case, 2)
    a32 = (290 + 5 * rng.random((n, channels) + shape)).astype(np.float32)
    p64 = a32.astype(np.float64) + 0.1 + 0.5 * rng.standard_normal(a32.shape)
    (p32, a64) = (p64.astype(np.float32), a32.astype(np.float64) + 1e-3 * rng.random(a32.shape))
    (p64be, a32be) = _netcdf_slabs(tmp_path, "p64_a32", p64, a32)
    (p32be, a64be) = _netcdf_slabs(tmp_path, "p32_a64", p32, a64)
    dev = torch.device("cuda")
    for (p, a, pn, an) in [(p64, a32, p64, a32), (p32, a64, p32, a64), (p64be, a32be, p64, a32), (p32be, a64be, p32, a64),
                           (p64be, a64, p64, a64), (p32, a32be, p32, a32),
                           (torch.from_numpy(p64).to(dev), a32be, p64, a32),
                           (torch.from_numpy(p32).to(dev), torch.from_numpy(a32).to(dev), p32, a32)]:
        got = pixel_sums(p, a, SHIFT, case_chunk)
        assert got.shape == (9,) + shape and got.dtype == np.float64
        check_sums(got, channel0(pn), channel0(an), SHIFT)
        assert (got[0] == n).all()
        # the same about per-pixel shifts (cae_pixel_sums_about)
        shifts = 290 + 5 * rng.random((2,) + shape)
        check_sums(pixel_sums(p, a, shifts, case_chunk), channel0(pn), channel0(an), shifts)


def _raw_sums(p_dev, pk, p_off, ps, a_dev, ak, a_off, as_, n, plane, shift, case_chunk):
    """cae_pixel_sums on element offsets into flat device buffers (case starts of any alignment), guard doubles around
    the nine planes checked"""
    lib = _lib.load()
    (pe, ae) = (4 if pk in (0, 1) else 8, 4 if ak in (0, 1) else 8)
    guard = 8
    out = torch.full((guard + 9 * plane + guard,), -7.0, dtype=torch.float64, device=p_dev.device)
    need = int(lib.cae_pixel_sums_workspace_bytes(n, plane, case_chunk))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=p_dev.device)
    _lib.check(lib.cae_pixel_sums(p_dev.data_ptr() + p_off * pe, pk, ps, a_dev.data_ptr() + a_off * ae, ak, as_, n, plane,
                                  shift, case_chunk, out.data_ptr() + 8 * guard, ws.data_ptr(), need, None))
    host = out.cpu().numpy()
    assert (host[:guard] == -7.0).all() and (host[-guard:] == -7.0).all()
    return host[guard:-guard].reshape(9, plane)


@pytest.mark.parametrize("plane,stride_p,stride_a", [(323, 324, 328), (4099, 4101, 4103), (5, 7, 6)])
@pytest.mark.parametrize("offsets", [(1, 3), (0, 1), (2, 2)])
def test_unaligned_case_starts(plane, stride_p, stride_a, offsets):
    """fp32 cases that start at every 4-byte phase of a 16-byte line, against fp32 and fp64 partners: strides that keep a
    common 16-byte phase (with a head and a tail at (2, 2), none at (1, 3)) and strides that do not"""
    rng = np.random.default_rng(plane + offsets[0])
    n = 11
    (po, ao) = offsets
    pf = rng.random(po + n * stride_p).astype(np.float32)
    af = rng.random(ao + n * stride_a).astype(np.float32)
    a64 = rng.random(ao + n * stride_a)
    cases = lambda buf, off, st: np.stack([buf[off + i * st: off + i * st + plane] for i in range(n)])  # noqa: E731
    (pd, ad, a64d) = (torch.from_numpy(pf).cuda(), torch.from_numpy(af).cuda(), torch.from_numpy(a64).cuda())
    for (adev, ak, abuf) in ((ad, _lib.ELEM_F32, af), (a64d, _lib.ELEM_F64, a64)):
        for case_chunk in (0, 4):
            got = _raw_sums(pd, _lib.ELEM_F32, po, stride_p, adev, ak, ao, stride_a, n, plane, 0.5, case_chunk)
            check_sums(got, cases(pf, po, stride_p), cases(abuf, ao, stride_a), 0.5)


def test_non_finite_values_stay_in_their_pixel():
    rng = np.random.default_rng(5)
    p = rng.random((7, 1, 17, 19))
    a = rng.random((7, 1, 17, 19)).astype(np.float32)
    clean = (p.copy(), a.copy())
    p[1, 0, 10, 3] = np.nan
    a[3, 0, 16, 18] = np.inf
    p[5, 0, 0, 0] = np.inf
    a[5, 0, 0, 0] = np.inf
    p[6, 0, 8, 9] = -np.inf
    p[:, 0, 2, 2] = np.nan                  # no pair at all
    touched = np.zeros((17, 19), dtype=bool)
    touched[[10, 16, 0, 8, 2], [3, 18, 0, 9, 2]] = True
    for case_chunk in (0, 3):
        got = pixel_sums(p, a, 0.5, case_chunk)
        check_sums(got, channel0(p), channel0(a), 0.5)
        assert got[0, 10, 3] == 6 and got[0, 16, 18] == 6 and got[0, 0, 0] == 6 and got[0, 8, 9] == 6
        assert (got[:, 2, 2] == 0.0).all() and not np.signbit(got[:, 2, 2]).any()
        assert np.isfinite(got).all()
        # the other pixels are what they are without the non-finite values, bit for bit
        untouched = pixel_sums(clean[0], clean[1], 0.5, case_chunk)
        assert got[:, ~touched].tobytes() == untouched[:, ~touched].tobytes()
        assert (got[0][~touched] == 7).all()
        # per-pixel shifts that differ for a and p: a case that is no pair still adds nothing, to d either
        shifts = rng.random((2, 17, 19))
        about = pixel_sums(p, a, shifts, case_chunk)
        check_sums(about, channel0(p), channel0(a), shifts)
        assert (about[:, 2, 2] == 0.0).all() and np.isfinite(about).all()
        assert about[:4].tobytes() == got[:4].tobytes()        # n and the sums of d do not depend on the shifts


def test_seventy_thousand_cases():
    """case indices past 65 535 and the library's own cut: many chunks on a tiny plane"""
    rng = np.random.default_rng(70000)
    p = 290 + 5 * rng.random((70000, 1, 1, 4))
    a = (290 + 5 * rng.random((70000, 2, 1, 4))).astype(np.float32)
    assert _lib.load().cae_pixel_sums_workspace_bytes(70000, 4, 0) > 1000 * 9 * 4 * 8
    got = pixel_sums(p, a, SHIFT)
    assert (got[0] == 70000).all()
    check_sums(got, channel0(p), channel0(a), SHIFT)


@pytest.mark.parametrize("case_chunk", [0, 8])
def test_two_runs_agree_bit_for_bit(case_chunk):
    rng = np.random.default_rng(11)
    p = torch.from_numpy(rng.random((40, 1, 256, 256))).cuda()
    a = torch.from_numpy(rng.random((40, 1, 256, 256)).astype(np.float32)).cuda()
    first = pixel_sums(p, a, 0.5, case_chunk)
    second = pixel_sums(p.clone(), a.clone(), 0.5, case_chunk)
    assert first.tobytes() == second.tobytes()
    assert (first[0] == 40).all()


def test_bad_arguments_write_nothing():
    lib = _lib.load()
    (n, plane) = (20, 40)
    p = torch.rand(n * plane, dtype=torch.float64, device="cuda")
    a = torch.rand(n * plane, dtype=torch.float32, device="cuda")
    out = torch.full((16 + 9 * plane,), -7.0, dtype=torch.float64, device="cuda")
    need = int(lib.cae_pixel_sums_workspace_bytes(n, plane, 8))
    assert need == 3 * 9 * plane * 8
    ws = torch.full((need // 8,), -7.0, dtype=torch.float64, device="cuda")
    call = lambda pk, pl, ws_bytes, chunk=8, shift=0.5: lib.cae_pixel_sums(                # noqa: E731
        p.data_ptr(), pk, plane, a.data_ptr(), _lib.ELEM_F32, plane, n, pl, shift, chunk, out.data_ptr() + 64,
        ws.data_ptr(), ws_bytes, None)
    assert call(_lib.ELEM_F64, plane, need - 8) < 0          # a workspace that is too small
    assert call(4, plane, need) < 0                           # an unknown kind
    assert call(-1, plane, need) < 0
    assert call(_lib.ELEM_F64, -1, need) < 0                  # a negative plane
    assert call(_lib.ELEM_F64, plane, need, chunk=-1) < 0
    assert call(_lib.ELEM_F64, plane, need, shift=float("nan")) < 0
    assert lib.cae_pixel_sums(p.data_ptr(), _lib.ELEM_F64, plane, a.data_ptr(), _lib.ELEM_F32, plane, -1, plane, 0.5, 8,
                              out.data_ptr() + 64, ws.data_ptr(), need, None) < 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (ws.cpu().numpy() == -7.0).all()
    # and the same call with good arguments writes the nine planes and nothing around them
    _lib.check(call(_lib.ELEM_F64, plane, need))
    host = out.cpu().numpy()
    assert (host[:8] == -7.0).all() and (host[8 + 9 * plane:] == -7.0).all()
    check_sums(host[8:8 + 9 * plane].reshape(9, plane), p.cpu().numpy().reshape(n, plane), a.cpu().numpy().reshape(n, plane), 0.5)
    # no case: nine planes of zeros
    _lib.check(lib.cae_pixel_sums(None, _lib.ELEM_F64, plane, None, _lib.ELEM_F32, plane, 0, plane, 0.5, 0,
                                  out.data_ptr() + 64, None, 0, None))
    host = out.cpu().numpy()
    assert (host[8:8 + 9 * plane] == 0.0).all() and (host[:8] == -7.0).all() and (host[8 + 9 * plane:] == -7.0).all()


# ---- train_cae -> apply_cae -> skill_maps -----------------------------------------------------

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """12 circle cases per partition with a time variable over the case dimension and ascending y / x coordinates"""
    from cae_tools_amd.data import datagen
    from cae_tools_amd.data.arrays import DataArray
    root = tmp_path_factory.mktemp("skill_maps")
    paths = {}
    for (part, seed) in (("train", 1234), ("test", 4321)):
        ds = datagen.generate("circle", 12, seed=seed)
        ds["time"] = DataArray(np.arange(12, dtype=np.float64) * 0.5 + 100.0, dims=("n",), attrs={"units": "days since 2000-01-01"})
        ds["y"] = DataArray(np.linspace(50.0, 60.0, 256), dims=("y2",))
        ds["x"] = DataArray(np.linspace(-5.0, 5.0, 256), dims=("x2",))
        paths[part] = str(root / f"{part}.nc")
        ds.to_netcdf(paths[part])
    return root, paths


def _check_outputs(folder, held_by):
    """the files of one skill_maps run against numpy.  held_by: {partition: (prediction, target)}, (N, C, H, W) arrays"""
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.utils.case_pages import _fmt
    scored = held_by
    with open(os.path.join(folder, "index.html")) as f:
        assert f.read().count('href="maps/index.html"') == 1
    with open(os.path.join(folder, "maps", "index.html")) as f:
        page = f.read()
    held = {}
    n_case = 0
    for (partition, (pred, target)) in held_by.items():
        assert pred.dtype.itemsize == 8 and target.dtype.itemsize == 4
        n_case = max(n_case, pred.shape[0])
        sk = open_dataset(os.path.join(folder, f"skill_{partition}.nc"))
        held[partition] = {m: np.asarray(sk[m].values).astype(np.float64) for m in MAPS}
        for m in MAPS:
            assert tuple(sk[m].dims) == ("y2", "x2") and np.asarray(sk[m].values).dtype.itemsize == 8
        assert_maps_close(held[partition], two_pass_maps(channel0(pred), channel0(target)), rtol=1e-12)
        assert (held[partition]["count"] == pred.shape[0]).all()
        np.testing.assert_array_equal(np.asarray(sk["y"].values), np.linspace(50.0, 60.0, 256))
        np.testing.assert_array_equal(np.asarray(sk["x"].values), np.linspace(-5.0, 5.0, 256))
    assert sorted(f for f in os.listdir(folder) if f.startswith("skill_")) == sorted(f"skill_{p}.nc" for p in scored)
    # every PNG: the palette restatement of the map the file holds, under the range rule over the partitions; y ascends
    for m in MAPS:
        (lo, hi) = range_rule(m, list(held.values()), n_case)
        assert page.count(f"{_fmt(lo)} … {_fmt(hi)}") >= len(scored), m
        for partition in scored:
            name = f"{partition}_{m}.png"
            assert f'src="{name}"' in page
            with open(os.path.join(folder, "maps", name), "rb") as f:
                (w, h, raw) = decode_png(f.read())
            assert (h, w) == (256, 256)
            assert raw == np_scanlines(held[partition][m], lo, hi, True).tobytes(), (partition, m)
    assert len(os.listdir(os.path.join(folder, "maps"))) == 6 * len(scored) + 2       # the colour bar and the page
    assert re.findall(r'<tr class="maps" data-partition="([a-z]+)"', page) == [p for p in ("test", "train") if p in scored]


def test_train_apply_skill_maps(data, monkeypatch):
    from cae_tools_amd.cli import apply_cae, evaluate_cae, skill_maps, train_cae
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
    coords = ["--x-coordinate", "x", "--y-coordinate", "y", "--time-coordinate", "time", "--sample-count", "2",
              "--input-variables", "lowres"]
    arrays = lambda ds: tuple(np.asarray(ds[v].values) for v in ("model_output", "hires"))      # noqa: E731

    # the scored file: the prediction is read from it
    out1 = str(root / "report_scored")
    with redirect_stdout(io.StringIO()):
        skill_maps.main(["--test-inputs", scored, "--model-folder", model, "--output-html-folder", out1] + coords)
    _check_outputs(out1, {"test": arrays(open_dataset(scored))})

    # both partitions unscored: the evaluator applies the model and sums the prediction where it lies on the GPU; the
    # data sets it leaves hold the host copy of that prediction
    seen = []

    class Recording(ModelEvaluator):
        def build_html(self, case_dimension, train_ds, test_ds, model_metrics):
            super().build_html(case_dimension, train_ds, test_ds, model_metrics)
            seen.append({"test": arrays(test_ds), "train": arrays(train_ds)})

    monkeypatch.setattr(evaluate_cae, "ModelEvaluator", Recording)
    out2 = str(root / "report_apply")
    log = io.StringIO()
    with redirect_stdout(log):
        skill_maps.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                         "--output-html-folder", out2] + coords)
    assert "Applying model to generate train scores" in log.getvalue() and len(seen) == 1
    _check_outputs(out2, seen[0])
    monkeypatch.undo()

    # evaluate_cae itself on the same inputs: no maps, no skill files, no link
    out3 = str(root / "report_plain")
    with redirect_stdout(io.StringIO()):
        evaluate_cae.main(["--train-inputs", paths["train"], "--test-inputs", paths["test"], "--model-folder", model,
                           "--output-html-folder", out3] + coords)
    assert not os.path.exists(os.path.join(out3, "maps"))
    assert not [f for f in os.listdir(out3) if f.startswith("skill_")]
    with open(os.path.join(out3, "index.html")) as f:
        assert "maps/index.html" not in f.read()
    with open(os.path.join(out2, "index.html")) as f:
        linked = f.read()
    with open(os.path.join(out3, "index.html")) as f:
        assert len(linked.splitlines()) == len(f.read().splitlines()) + 3
