"""Scene apply on the GPU (cae_scene_gather, cae_scene_blend; DESIGN.md §9 'scene apply').  Model-free first, the
"predictions" seeded random fp32 values: the gathered batch is the bytes of normalise_pack on the same boxes sliced on the host,
for every element kind, and the invalid flags are exact; the blended scene is within the fold-order bound
(m + 2) 2^-53 (|vmin| + |range| S w|p| / S w) of scene_ref.py's np.longdouble value at every pixel; the cases with an exact
answer are compared as bytes; the result does not depend on how the tile rows are cut into pieces, nor on the run.  Then a
LinearModel is trained and the apply_scene command line is compared, pixel by pixel, with the reference fed by the model's own
scores of the gathered tiles.

Largest |got - want| / bound measured on an MI355X (every check prints its figure before it asserts): 0.24 over the shapes
without invalid tiles ((40, 70) scene, 16 x 16 -> 64 x 64 boxes, overlap 4; 0.21 at (7, 8) with 3 x 3 -> 6 x 9 boxes, 0.15 at the
triple cover of (7, 9) with 4 x 4 boxes, 0 at overlap 0 and for the scene of one pixel), 0.30 with invalid tiles, 0.23 blended in
pieces, 0.31 end to end through the command line.  The gathered batches, the exact cases and the pieces are equal as bytes;
the counts are exact."""
import io
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import scene_ref
from cae_tools_amd._lib import CaeError
from cae_tools_amd.engine import (denormalise_f64, normalise_pack, scene_apply, scene_blend, scene_plan, scene_tiles,
                                  upload_f32)

pytestmark = pytest.mark.gpu

(VMIN, VMAX) = (270.5, 310.25)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _plan(scene, box, out_box, overlap):
    return scene_plan(scene[0], scene[1], (box, out_box), overlap)


def _args(plan):
    """the plan as scene_ref takes it"""
    return (plan.Y, plan.X, plan.h, plan.w, plan.oy, plan.ox)


# ---- gather -------------------------------------------------------------------------------------------------------

def _as_kind(tmp_path, kind, arrays):
    """the arrays as fp32 / fp64 numpy arrays, or written to a NetCDF-3 file and read back as the big-endian views of its
    mapping that the loader hands on"""
    dtype = np.float32 if kind.startswith("f32") else np.float64
    arrays = [np.ascontiguousarray(a, dtype=dtype) for a in arrays]
    if not kind.endswith("be"):
        return arrays, arrays
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import as_numpy, open_dataset
    (dims, variables) = ({}, {})
    for (i, a) in enumerate(arrays):
        names = tuple(f"d{i}_{j}" for j in range(a.ndim))
        dims.update(dict(zip(names, a.shape)))
        variables[f"v{i}"] = (names, a, {})
    path = str(tmp_path / f"{kind}.nc")
    netcdf3.write(path, dims, variables)
    ds = open_dataset(path, mask_and_scale=False)
    slabs = [as_numpy(ds[f"v{i}"]) for i in range(len(arrays))]
    assert all(s.dtype.byteorder == ">" for s in slabs)
    return slabs, arrays


def _packed_on_the_host(native, plan, norms, enable):
    """normalise_pack of the same boxes, sliced on the host"""
    boxes = [np.ascontiguousarray(scene_ref.boxes(v, plan.h, plan.w, plan.oy, plan.ox)) for v in native]
    dst = torch.empty((boxes[0].shape[0], sum(b.shape[1] for b in boxes), plan.h, plan.w), dtype=torch.float32, device=_dev())
    off = 0
    for (b, (lo, hi)) in zip(boxes, norms):
        normalise_pack(upload_f32(b, _dev()), dst, off, lo, hi, enable=enable)
        off += b.shape[1]
    return dst.cpu().numpy()


GATHER_SCENES = [((7, 9), (4, 4), 2), ((5, 7), (2, 3), (1, 2)), ((16, 33), (8, 8), 0), ((1, 1), (1, 1), 0)]


@pytest.mark.parametrize("kind", ["f32", "f32be", "f64", "f64be"])
@pytest.mark.parametrize("scene", GATHER_SCENES)
def test_gather_is_normalise_pack_of_the_sliced_boxes(tmp_path, scene, kind):
    ((Y, X), box, overlap) = scene
    plan = _plan((Y, X), box, box, overlap)
    rng = np.random.default_rng(Y * 100 + X)
    one = 280.0 + 10.0 * rng.random((2, 1, Y, X))
    two = 1e3 * rng.standard_normal((2, 2, Y, X))
    one[0, 0, 0, 0] = np.nan
    two[1, 1, Y - 1, X // 2] = -np.inf
    (given, native) = _as_kind(tmp_path, kind, [one, two])
    want_flags = scene_ref.invalid_tiles(native, plan.h, plan.w, plan.oy, plan.ox)
    for (norms, enable) in (([(280.0, 290.0), (-3e3, 3e3)], True), ([(280.0, 290.0), (5.0, 5.0)], True),     # range == 0
                            ([(280.0, 290.0), (-3e3, 3e3)], False)):
        (x, invalid) = scene_tiles(given, plan, norms, normalise=enable)
        assert tuple(x.shape) == (2 * plan.n_tile, 3, plan.h, plan.w)
        assert x.cpu().numpy().tobytes() == _packed_on_the_host(native, plan, norms, enable).tobytes()
        assert np.array_equal(invalid.cpu().numpy(), want_flags)
    # a time range and a tile-row range are the same tiles
    (whole, flags) = scene_tiles(given, plan, [(280.0, 290.0), (-3e3, 3e3)])
    whole = whole.view(2, plan.n_y, plan.n_x, 3, plan.h, plan.w)
    for (t0, n_t, k0, n_k) in ((1, 1, 0, plan.n_y), (0, 2, plan.n_y - 1, 1), (1, 1, plan.n_y // 2, 1)):
        (part, pf) = scene_tiles(given, plan, [(280.0, 290.0), (-3e3, 3e3)], t0, n_t, k0, n_k)
        assert part.cpu().numpy().tobytes() == whole[t0:t0 + n_t, k0:k0 + n_k].contiguous().cpu().numpy().tobytes()
        assert torch.equal(pf, flags.view(2, plan.n_y, plan.n_x)[t0:t0 + n_t, k0:k0 + n_k].reshape(-1))


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_invalid_flags_are_exact(value):
    plan = _plan((7, 9), (4, 4), (4, 4), 2)                # origins y 0, 2, 3 and x 0, 2, 4, 5
    rng = np.random.default_rng(3)
    clean = [rng.random((2, 1, 7, 9)).astype(np.float32), rng.random((2, 2, 7, 9))]
    norms = [(0.0, 1.0), (0.0, 1.0)]
    assert int(scene_tiles(clean, plan, norms)[1].sum()) == 0
    # a corner pixel (one tile), the last channel of the last variable, and a pixel four tiles share
    for ((var, t, c, y, x), n_flagged) in (((0, 0, 0, 0, 0), 1), ((1, 1, 1, 6, 8), 1), ((0, 1, 0, 2, 2), 4), ((1, 0, 1, 3, 5), 9)):
        dirty = [a.copy() for a in clean]
        dirty[var][t, c, y, x] = value
        want = scene_ref.invalid_tiles(dirty, 4, 4, 2, 2)
        assert int(want.sum()) == n_flagged and int(want.reshape(2, -1)[1 - t].sum()) == 0
        assert np.array_equal(scene_tiles(dirty, plan, norms)[1].cpu().numpy(), want)
    big = [clean[0], clean[1].copy()]
    big[1][0, 0, 6, 0] = 1e300                              # finite as fp64, not as the fp32 the model is given
    assert np.array_equal(scene_tiles(big, plan, norms)[1].cpu().numpy(), scene_ref.invalid_tiles(big, 4, 4, 2, 2))
    assert int(scene_ref.invalid_tiles(big, 4, 4, 2, 2).sum()) == 1


# ---- blend against the reference --------------------------------------------------------------------------------------

BLEND_SCENES = [((1, 1), (1, 1), (1, 1), 0), ((5, 7), (2, 3), (2, 3), (1, 2)), ((7, 8), (3, 3), (6, 9), 0),
                ((7, 8), (3, 3), (6, 9), 1), ((7, 8), (3, 3), (6, 9), 2), ((7, 9), (4, 4), (4, 4), 2),
                ((40, 70), (16, 16), (64, 64), 4)]


def _blend(pred, invalid, plan, n_t):
    (out, holes) = scene_blend(torch.from_numpy(pred).to(_dev()), torch.from_numpy(np.asarray(invalid, dtype=np.int32)).to(_dev()),
                               plan, VMIN, VMAX, n_t=n_t)
    return out.cpu().numpy(), holes.cpu().numpy()


@pytest.mark.parametrize("c_out", [1, 2])
@pytest.mark.parametrize("n_t", [1, 3])
@pytest.mark.parametrize("scene", BLEND_SCENES)
def test_blend_within_the_fold_order_bound(scene, n_t, c_out):
    (yx, box, out_box, overlap) = scene
    plan = _plan(yx, box, out_box, overlap)
    rng = np.random.default_rng(yx[0] * 1000 + yx[1] * 10 + n_t + c_out)
    pred = rng.standard_normal((n_t * plan.n_tile, c_out, plan.H, plan.W)).astype(np.float32)
    invalid = np.zeros(n_t * plan.n_tile, dtype=np.int32)
    ref = scene_ref.Reference(pred, invalid, *_args(plan), VMIN, VMAX)
    (got, holes) = _blend(pred, invalid, plan, n_t)
    ref.check(got, f"{yx} {box}->{out_box} overlap {overlap} T {n_t} Co {c_out}")
    assert holes.tolist() == [0] * n_t and not ref.hole.any()
    # a pixel under one tile is that tile's value, denormalised: the same bytes
    den = denormalise_f64(torch.from_numpy(pred).to(_dev()), VMIN, VMAX).cpu().numpy()
    canvas = np.full(got.shape, np.nan)
    tile = 0
    for t in range(n_t):
        for y in plan.ys:
            for x in plan.xs:
                canvas[t, :, y * plan.sy:y * plan.sy + plan.H, x * plan.sx:x * plan.sx + plan.W] = den[tile]
                tile += 1
    single = np.broadcast_to((ref.valid == 1)[:, None], got.shape)
    assert got[single].tobytes() == canvas[single].tobytes()


@pytest.mark.parametrize("scene", [((7, 9), (4, 4), (4, 4), 2), ((40, 70), (16, 16), (64, 64), 4), ((7, 8), (3, 3), (6, 9), 1)])
def test_blend_with_invalid_tiles(scene):
    (yx, box, out_box, overlap) = scene
    plan = _plan(yx, box, out_box, overlap)
    rng = np.random.default_rng(yx[1])
    n_t = 3
    pred = (5.0 * rng.standard_normal((n_t * plan.n_tile, 2, plan.H, plan.W))).astype(np.float32)
    invalid = (rng.random(n_t * plan.n_tile) < 0.4).astype(np.int32)
    invalid[:plan.n_tile][:plan.n_x + 1] = 1                # the first tile row and one more: a corner without a valid tile
    invalid[2 * plan.n_tile:] = 1                           # a time step without a valid tile
    pred[invalid != 0] = np.nan                             # what an invalid tile scores is never read into a sum
    ref = scene_ref.Reference(pred, invalid, *_args(plan), VMIN, VMAX)
    (got, holes) = _blend(pred, invalid, plan, n_t)
    ref.check(got, f"{yx} {box}->{out_box} with invalid tiles")
    assert holes.tolist() == ref.nan_pixels.tolist()        # the counts are exact
    assert holes[0] > 0 and holes[2] == plan.out_shape[0] * plan.out_shape[1] and np.isnan(got[2]).all()


def test_exact_partition_is_the_per_box_layout():
    plan = _plan((12, 20), (4, 5), (8, 15), 0)
    rng = np.random.default_rng(5)
    (n_t, c_out) = (2, 2)
    pred = rng.standard_normal((n_t * plan.n_tile, c_out, plan.H, plan.W)).astype(np.float32)
    (got, holes) = _blend(pred, np.zeros(n_t * plan.n_tile, dtype=np.int32), plan, n_t)
    den = denormalise_f64(torch.from_numpy(pred).to(_dev()), VMIN, VMAX).cpu().numpy()
    want = den.reshape(n_t, plan.n_y, plan.n_x, c_out, plan.H, plan.W).transpose(0, 3, 1, 4, 2, 5).reshape(got.shape)
    assert got.tobytes() == want.tobytes() and holes.tolist() == [0, 0]


def test_one_valid_and_one_invalid_tile():
    plan = _plan((4, 6), (4, 4), (8, 8), 2)                # two tiles side by side, origins x 0 and 2: output columns 4..7 shared
    rng = np.random.default_rng(6)
    pred = rng.standard_normal((2, 1, 8, 8)).astype(np.float32)
    den = denormalise_f64(torch.from_numpy(pred).to(_dev()), VMIN, VMAX).cpu().numpy()
    (got, holes) = _blend(pred, [0, 1], plan, 1)
    assert got[0, 0, :, :8].tobytes() == den[0, 0].tobytes()            # shared pixels: the valid tile alone
    assert np.isnan(got[0, 0, :, 8:]).all() and holes.tolist() == [8 * 4]
    (got, holes) = _blend(pred, [1, 0], plan, 1)
    assert got[0, 0, :, 4:].tobytes() == den[1, 0].tobytes() and np.isnan(got[0, 0, :, :4]).all() and holes.tolist() == [32]
    (got, holes) = _blend(pred, [1, 1], plan, 1)
    assert np.isnan(got).all() and holes.tolist() == [8 * 12]


def test_blend_refuses_rows_whose_tiles_are_missing():
    plan = _plan((7, 9), (4, 4), (4, 4), 2)
    pred = torch.zeros((plan.n_x, 1, 4, 4), dtype=torch.float32, device=_dev())
    flags = torch.zeros(plan.n_x, dtype=torch.int32, device=_dev())
    with pytest.raises(CaeError, match="tile row 0"):
        scene_blend(pred, flags, plan, VMIN, VMAX, k0=1)            # rows 2.. of tile row 1 alone: tile row 0 covers row 2 too
    with pytest.raises(ValueError):
        scene_blend(pred[:, :, :3], flags, plan, VMIN, VMAX)


# ---- pieces and repeatability -------------------------------------------------------------------------------------------

def _score(plan, c_out):
    """a stand-in model, element by element: what it returns for a tile does not depend on the batch the tile comes in"""
    def score(x):
        up = x[:, :1].repeat_interleave(plan.sy, dim=2).repeat_interleave(plan.sx, dim=3)
        ramp = torch.linspace(0.0, 0.3, plan.H * plan.W, device=x.device).view(1, 1, plan.H, plan.W)      # tiles differ where they overlap
        return torch.cat([up * (0.75 + 0.5 * c) + ramp for c in range(c_out)], dim=1).contiguous()
    return score


@pytest.mark.parametrize("scene", [((7, 9), (4, 4), (4, 4), 2, 2), ((7, 8), (3, 3), (6, 9), 1, 1), ((40, 70), (16, 16), (64, 64), 4, 2),
                                   ((23, 9), (4, 4), (8, 4), 3, 1)])
def test_pieces_and_runs_give_the_same_bytes(scene):
    (yx, box, out_box, overlap, c_out) = scene
    plan = _plan(yx, box, out_box, overlap)
    rng = np.random.default_rng(yx[0])
    field = rng.random((3, 1) + yx).astype(np.float32)
    field[1, 0, yx[0] // 2, yx[1] // 2] = np.nan
    field[2, 0, 0, 0] = np.inf
    norms = [(0.0, 1.0)]
    score = _score(plan, c_out)
    runs = {rows: scene_apply([field], norms, plan, score, c_out, VMIN, VMAX, tile_rows=rows) for rows in (None, 1, 2, plan.n_y)}
    again = scene_apply([field], norms, plan, score, c_out, VMIN, VMAX)
    (out, bad, holes) = runs[None]
    base = out.cpu().numpy().tobytes()
    for (rows, (o, b, n)) in list(runs.items()) + [("again", again)]:
        assert o.cpu().numpy().tobytes() == base, rows
        assert b.tolist() == bad.tolist() and n.tolist() == holes.tolist(), rows
    (x, invalid) = scene_tiles([field], plan, norms)
    ref = scene_ref.Reference(score(x).cpu().numpy(), invalid.cpu().numpy(), *_args(plan), VMIN, VMAX)
    ref.check(out.cpu().numpy(), f"{yx} {box}->{out_box} in pieces")
    assert bad.tolist() == ref.invalid_tiles.tolist() and holes.tolist() == ref.nan_pixels.tolist()
    assert bad[0] == 0 and bad[1] > 0 and bad[2] == 1


# ---- end to end ---------------------------------------------------------------------------------------------------------

def _boxes_data(n, seed):
    from cae_tools_amd.data.arrays import DataArray, Dataset
    rng = np.random.default_rng(seed)
    lo = (280 + 10 * rng.random((n, 1, 8, 8))).astype(np.float32)
    hi = np.repeat(np.repeat(lo, 4, axis=2), 4, axis=3) + rng.standard_normal((n, 1, 32, 32)).astype(np.float32) * 0.1
    ds = Dataset()
    ds["lowres"] = DataArray(lo, dims=("n", "chan", "y", "x"))
    ds["hires"] = DataArray(hi.astype(np.float32), dims=("n", "chan", "y2", "x2"))
    return ds


@pytest.fixture(scope="module")
def model_folder(tmp_path_factory):
    """a LinearModel on 8 x 8 -> 32 x 32 boxes, two epochs"""
    from cae_tools_amd.models.linear_model import LinearModel
    folder = str(tmp_path_factory.mktemp("scene") / "model")
    torch.manual_seed(4)
    model = LinearModel(batch_size=4, nr_epochs=2, test_interval=1)
    with redirect_stdout(io.StringIO()):
        model.train(["lowres"], "hires", _boxes_data(11, 1), _boxes_data(5, 2), model_path=folder)
    return folder


def test_apply_scene_command_line(model_folder, tmp_path):
    from cae_tools_amd.cli import apply_scene
    from cae_tools_amd.data import netcdf3
    from cae_tools_amd.data.arrays import open_dataset
    from cae_tools_amd.models.model_loader import load_model
    rng = np.random.default_rng(9)
    scene = (280 + 10 * rng.random((1, 1, 20, 28))).astype(np.float32)         # 2.5 x 3.5 boxes
    scene[0, 0, 9:11, 13:15] = np.nan                                         # one gap
    (path, scored) = (str(tmp_path / "scene.nc"), str(tmp_path / "scored.nc"))
    netcdf3.write(path, {"time": 1, "chan": 1, "y": 20, "x": 28}, {"lowres": (("time", "chan", "y", "x"), scene, {})})
    log = io.StringIO()
    with redirect_stdout(log):
        apply_scene.main([path, scored, "--model-folder", model_folder, "--overlap", "2"])
    ds = open_dataset(scored)
    got = np.asarray(ds["model_output"].values)
    assert got.dtype == np.float64 and got.shape == (1, 1, 80, 112)
    assert tuple(ds["model_output"].dims) == ("time", "model_output_channel", "model_output_y", "model_output_x")
    assert np.asarray(ds["lowres"].values).tobytes() == scene.tobytes()

    model = load_model(model_folder)
    with redirect_stdout(io.StringIO()):
        plan = scene_plan(20, 28, (model.input_shape, model.output_shape), 2)
        (min_in, max_in, min_out, max_out) = model.normalisation_parameters
        (x, invalid) = scene_tiles([scene], plan, [(min_in["lowres"], max_in["lowres"])])
        y = model._score_device(x)
    assert (plan.n_y, plan.n_x) == (3, 5)
    ref = scene_ref.Reference(y.cpu().numpy(), invalid.cpu().numpy(), 20, 28, 8, 8, 2, 2, min_out, max_out)
    ref.check(got, "apply_scene command line")
    assert ref.invalid_tiles.tolist() == [2] and ref.nan_pixels.tolist() == [640]
    lines = log.getvalue().splitlines()
    assert "Applying model to 1 scenes of 20 x 28: 3 x 5 tiles of 8 x 8 -> 32 x 32, overlap (2, 2), output 80 x 112" in lines
    assert "invalid tiles: 2 of 15 (per time step: [2])" in lines
    assert "NaN pixels: 640 of 8960 (per time step: [640])" in lines
    # --overlap NY NX and --tile-rows are taken
    with redirect_stdout(io.StringIO()):
        apply_scene.main([path, str(tmp_path / "rows.nc"), "--model-folder", model_folder, "--overlap", "2", "2", "--tile-rows", "3"])
    assert np.asarray(open_dataset(str(tmp_path / "rows.nc"))["model_output"].values).tobytes() == got.tobytes()


def test_a_scene_of_one_box_is_apply(model_folder):
    from cae_tools_amd.models.model_loader import load_model
    model = load_model(model_folder)
    (a, b) = (_boxes_data(3, 7), _boxes_data(3, 7))
    with redirect_stdout(io.StringIO()):
        model.apply(a, ["lowres"])
        out = model.apply_scene(b, ["lowres"])
    assert np.asarray(b["model_output"].values).tobytes() == np.asarray(a["model_output"].values).tobytes()
    assert out.cpu().numpy().tobytes() == np.asarray(a["model_output"].values).tobytes()
    assert tuple(b["model_output"].dims) == ("n", "model_output_channel", "model_output_y", "model_output_x")
    assert model.scene_report["invalid_tiles"].tolist() == [0, 0, 0] and model.scene_report["nan_pixels"].tolist() == [0, 0, 0]
    from cae_tools_amd.data.arrays import DataArray, Dataset
    small = Dataset()
    small["lowres"] = DataArray(np.asarray(a["lowres"].values)[:, :, :7], dims=("n", "chan", "y", "x"))
    with pytest.raises(ValueError, match="smaller"):
        model.apply_scene(small, ["lowres"])
