"""Scene apply without a GPU: engine.scene_plan against the definition (DESIGN.md §9 'scene apply'), its refusals, the pieces
scene_apply cuts a scene into, the numpy restatement (scene_ref.py) against a plain triple loop, and the command line's
refusal of apply_cae's ensemble options."""
import math

import numpy as np
import pytest

import scene_ref
from cae_tools_amd.engine import scene_chunks, scene_plan


def _plan_1d(Y, h, o):
    return scene_plan(Y, h, ((h, h), (h, h)), (o, o))


def test_origins_of_the_definition():
    assert _plan_1d(7, 4, 2).ys == (0, 2, 3)                # the shifted last tile: triple cover
    assert _plan_1d(7, 4, 2).xs == (0,)
    p = scene_plan(9, 5, ((1, 9, 5), (2, 18, 20)))
    assert (p.ys, p.xs, p.n_y, p.n_x, p.n_tile) == ((0,), (0,), 1, 1, 1)       # Y = h: one tile
    assert (p.sy, p.sx, p.oy, p.ox, p.out_shape) == (2, 4, 2, 1, (18, 20))     # the default overlap is a quarter of the box
    p = scene_plan(12, 20, ((4, 5), (8, 5)), 0)
    assert p.ys == (0, 4, 8) and p.xs == (0, 5, 10, 15)     # overlap 0, a multiple of the box: an exact partition
    assert scene_plan(40, 70, ((16, 16), (64, 64)), 4).ys == (0, 12, 24) and scene_plan(40, 70, ((16, 16), (64, 64)), 4).n_x == 6


def test_cover_for_every_small_case():
    for h in range(1, 9):
        for o in range(h):
            s = h - o
            for Y in range(h, 40):
                ys = _plan_1d(Y, h, o).ys
                assert list(ys) == scene_ref.origins(Y, h, o)
                assert len(ys) == 1 + math.ceil((Y - h) / s) and ys[0] == 0 and ys[-1] == Y - h
                assert all(b > a for a, b in zip(ys, ys[1:]))
                c = scene_ref.cover(Y, h, o)
                assert c.min() >= 1 and c.max() <= math.ceil(h / s) + 1, (h, o, Y)


def test_rows_done_and_first_row_over():
    p = scene_plan(7, 9, ((4, 4), (8, 4)), 2)              # sy = 2; origins 0, 2, 3
    assert [p.rows_done(k) for k in range(4)] == [0, 4, 6, 14]
    assert [p.first_row_over(r) for r in (0, 7, 8, 11, 12, 13)] == [0, 0, 1, 1, 2, 2]
    for k1 in range(1, p.n_y):                              # a tile row at or after k1 touches no finished row
        assert all(y * p.sy >= p.rows_done(k1) for y in p.ys[k1:])


def test_refusals():
    with pytest.raises(ValueError, match=r"\(1, 24, 25\).*\(1, 8, 8\)"):
        scene_plan(20, 20, ((1, 8, 8), (1, 24, 25)))         # a ratio that is no integer: both shapes are named
    with pytest.raises(ValueError, match="multiple"):
        scene_plan(20, 20, ((8, 8), (4, 8)))
    for overlap in (8, (0, 8), (-1, 0)):
        with pytest.raises(ValueError, match="overlap"):
            scene_plan(20, 20, ((8, 8), (8, 8)), overlap)
    for (Y, X) in ((7, 20), (20, 7)):
        with pytest.raises(ValueError, match="smaller"):
            scene_plan(Y, X, ((8, 8), (8, 8)))
    with pytest.raises(ValueError, match="2\\^29"):
        scene_plan(4096, 8192, ((4096, 8192), (8192, 16384)))          # 4 H W = 2^29
    assert scene_plan(4096, 8192, ((4096, 8192), (8192, 8192)), 0).n_tile == 1          # 2^28: taken


def test_chunks_cover_every_tile_row_once():
    p = scene_plan(40, 70, ((16, 16), (64, 64)), 4)
    assert scene_chunks(p, 3, 1, tile_rows=1) == [(t, 1, k, 1) for t in range(3) for k in range(3)]
    assert scene_chunks(p, 3, 1, tile_rows=2) == [(t, 1, k, n) for t in range(3) for (k, n) in ((0, 2), (2, 1))]
    assert scene_chunks(p, 3, 2) == [(0, 3, 0, 3)]          # a small scene: all time steps in one piece
    big = scene_plan(1000, 4000, ((16, 16), (256, 256)), 4)
    chunks = scene_chunks(big, 2, 1)
    for t in range(2):
        assert [k for (t0, _, k0, n) in chunks if t0 == t for k in range(k0, k0 + n)] == list(range(big.n_y))
    assert all(n_t == 1 for (_, n_t, _, _) in chunks)
    assert 1 < max(n for (_, _, _, n) in chunks) <= (256 << 20) // (big.n_x * 256 * 256 * 4)
    with pytest.raises(ValueError):
        scene_chunks(p, 1, 1, tile_rows=0)


@pytest.mark.parametrize("case", [((5, 4), (2, 3), (4, 3), (1, 2), 2, 2), ((7, 5), (4, 4), (4, 4), (2, 0), 1, 1)])
def test_reference_against_the_triple_loop(case):
    ((Y, X), (h, w), (H, W), (oy, ox), T, Co) = case
    rng = np.random.default_rng(Y * 10 + X)
    n_tile = len(scene_ref.origins(Y, h, oy)) * len(scene_ref.origins(X, w, ox))
    pred = rng.standard_normal((T * n_tile, Co, H, W)).astype(np.float32)
    invalid = np.zeros(T * n_tile, dtype=np.int32)
    invalid[[0, n_tile - 1]] = 1
    if T > 1:
        invalid[n_tile:] = 1                                # a time step without a valid tile: all NaN
    ref = scene_ref.Reference(pred, invalid, Y, X, h, w, oy, ox, 270.5, 310.25)
    want = scene_ref.pixel_by_pixel(pred, invalid, Y, X, h, w, oy, ox, 270.5, 310.25)
    assert np.array_equal(np.isnan(want), np.isnan(ref.want)) and np.isnan(want).any() and not np.isnan(want).all()
    assert np.array_equal(want[~np.isnan(want)], ref.want[~np.isnan(want)])         # the same adds in the same order
    assert ref.nan_pixels.tolist() == [int(np.isnan(want[t, 0]).sum()) for t in range(T)]
    assert ref.ratio(ref.want.astype(np.float64)) <= 1.0 and (ref.bound > 0).all()
    if (Y, h, oy) == (7, 4, 2):
        assert scene_ref.cover(7, 4, 2).max() == 3 and ref.valid.max() > 2      # the triple cover along y is there


def test_command_line_refuses_the_ensemble_options(capsys):
    from cae_tools_amd.cli import apply_scene
    for flags in (["--ensemble-size", "4"], ["--spread-variable", "sd"], ["--latent-variable=z"], ["--ensemble-seed", "1"]):
        with pytest.raises(SystemExit) as ex:
            apply_scene.main(["in.nc", "out.nc", "--model-folder", "m"] + flags)
        assert ex.value.code == 2 and "no ensemble or latent output" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        apply_scene.main(["in.nc", "out.nc", "--model-folder", "m", "--overlap", "1", "2", "3"])
