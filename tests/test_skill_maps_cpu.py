"""The per-pixel skill maps without a GPU: maps_from_sums against a two-pass numpy computation, where it must give NaN,
the workspace size of cae_pixel_sums, the skill_maps command's flags, the report with and without the maps link, and the
NetCDF-3 file and the maps page fed synthetic scanlines."""
import json
import os
import re

import numpy as np
import pytest

from golden.make_golden_report import report_items
from skill_maps_ref import MAPS, assert_maps_close, chunked_sums, decode_png, range_rule, two_pass_maps
from cae_tools_amd import _lib
from cae_tools_amd.utils import report, skill_maps

HERE = os.path.dirname(os.path.abspath(__file__))


def _cases(seed=37):
    """37 cases x 13 pixels: float32 targets 290 + 5 rand, fp64 predictions target + 0.1 + 0.5 randn, with a NaN, both
    infinities, one pixel without a pair and one pixel whose target is constant"""
    rng = np.random.default_rng(seed)
    a = (290 + 5 * rng.random((37, 13))).astype(np.float32)
    a[:, 9] = np.float32(291.25)            # a constant target
    p = a.astype(np.float64) + 0.1 + 0.5 * rng.standard_normal((37, 13))
    p[3, 1] = np.nan
    a[5, 2] = np.inf
    p[7, 4] = -np.inf
    p[:, 6] = np.nan                        # no pair at all
    return p, a


@pytest.mark.parametrize("chunk", [8, 37, 1])
def test_maps_from_sums_match_two_pass(chunk):
    (p, a) = _cases()
    sums = chunked_sums(p, a, 292.5, chunk)
    got = skill_maps.maps_from_sums(sums)
    want = two_pass_maps(p, a)
    assert set(got) == set(MAPS)
    assert want["count"].tolist() == [37, 36, 36, 37, 36, 37, 0, 37, 37, 37, 37, 37, 37]
    assert_maps_close(got, want, rtol=1e-12)
    # the pixel without a pair: count 0, everything else NaN
    assert got["count"][6] == 0 and all(np.isnan(got[m][6]) for m in MAPS[1:])
    # the constant target: no correlation and no ratio, the error maps as everywhere
    assert np.isnan(got["correlation"][9]) and np.isnan(got["sd_ratio"][9]) and np.isfinite(got["rmse"][9])
    assert np.isfinite(got["correlation"][[0, 1, 2, 3, 4, 5, 7, 8, 10, 11, 12]]).all()


def test_one_case_has_no_correlation():
    (p, a) = _cases()
    got = skill_maps.maps_from_sums(chunked_sums(p[:1], a[:1], 292.5, 8))
    want = two_pass_maps(p[:1], a[:1])
    assert_maps_close(got, want)
    assert np.isnan(got["correlation"]).all() and np.isnan(got["sd_ratio"]).all()
    assert got["count"].tolist() == [1] * 6 + [0] + [1] * 6
    assert np.isfinite(np.delete(got["bias"], 6)).all() and np.isnan(got["bias"][6])


def test_constant_pixels_of_many_cases_stay_nan():
    """a variance no larger than its own rounding is no variance: a constant pixel far from the shift, whose sums cancel
    only to rounding, gives NaN and not a correlation of noise"""
    rng = np.random.default_rng(2)
    n = 5000
    a = np.full((n, 4), 293.75)
    p = 290 + 5 * rng.random((n, 4))
    p[:, 1] = 288.25                        # both constant
    a[:, 2] = 290 + 5 * rng.random(n)       # neither constant
    a[:, 3] = 290 + 5 * rng.random(n)       # a constant prediction of a varying target
    p[:, 3] = 288.25
    got = skill_maps.maps_from_sums(chunked_sums(p, a, 1.0, 64))
    assert np.isnan(got["correlation"][:2]).all() and np.isnan(got["sd_ratio"][:2]).all()
    assert np.isfinite(got["correlation"][2]) and np.isfinite(got["sd_ratio"][2])
    assert np.isnan(got["correlation"][3]) and got["sd_ratio"][3] == 0.0
    want = two_pass_maps(p, a)              # the shift is far off on purpose: the same places, not the same digits
    for m in MAPS:
        np.testing.assert_array_equal(np.isnan(got[m]), np.isnan(want[m]), err_msg=m)
    np.testing.assert_allclose(got["sd_ratio"][2:], want["sd_ratio"][2:], rtol=1e-6)
    with pytest.raises(ValueError):
        skill_maps.maps_from_sums(np.zeros((8, 3)))


def test_centred_sums_resolve_a_small_variance():
    """a prediction that varies by 1e-5 of its distance from the common shift: about that shift its variance is known to
    1e-5 only, about the pixel's own means (the evaluator's second pass) to rounding"""
    rng = np.random.default_rng(4)
    (n, px) = (12, 50)
    a = np.where(rng.random((n, px)) < 0.4, 4.0, 0.0).astype(np.float32)
    a[:, 7] = 0.0
    p = 2.0 + 0.1 * rng.random(px) + 2e-5 * rng.standard_normal((n, px))
    p[:, 9] = 2.03125                       # a constant prediction
    p[3, 11] = np.nan
    sums = chunked_sums(p, a, 0.25, 8)
    means = skill_maps.pixel_means(sums, 0.25)
    assert means.shape == (2, px)
    np.testing.assert_allclose(means[1], np.nanmean(p, axis=0), rtol=1e-14)
    centred = chunked_sums(p, a, means, 8)
    want = two_pass_maps(p, a)
    assert_maps_close(skill_maps.maps_from_sums(sums, centred), want, rtol=1e-12)
    assert np.isnan(want["correlation"][[7, 9]]).all() and want["sd_ratio"][9] == 0.0 and np.isnan(want["sd_ratio"][7])
    plain = skill_maps.maps_from_sums(sums)
    ok = np.isfinite(want["correlation"]) & np.isfinite(plain["correlation"])
    assert np.abs(plain["correlation"][ok] / want["correlation"][ok] - 1).max() > 1e-9     # what the second pass is for
    # a pixel without a pair keeps the shift
    sums[:, 0] = 0.0
    assert (skill_maps.pixel_means(sums, 0.25)[:, 0] == 0.25).all()


def test_workspace_bytes_without_a_gpu():
    lib = _lib.load()
    assert lib.cae_pixel_sums_workspace_bytes(37, 323, 37) == 0
    assert lib.cae_pixel_sums_workspace_bytes(37, 323, 100) == 0
    assert lib.cae_pixel_sums_workspace_bytes(37, 323, 8) == 5 * 9 * 323 * 8
    assert lib.cae_pixel_sums_workspace_bytes(7, 1, 1) == 7 * 9 * 8
    assert lib.cae_pixel_sums_workspace_bytes(1, 65536, 0) == 0
    assert lib.cae_pixel_sums_workspace_bytes(0, 5, 0) == 0 and lib.cae_pixel_sums_workspace_bytes(5, 0, 0) == 0
    # the library's own cut: whole chunks of at least 8 cases, and a tiny plane with many cases is still cut
    for (n, plane) in ((2000, 65536), (70000, 4), (37, 323), (9, 4)):
        need = lib.cae_pixel_sums_workspace_bytes(n, plane, 0)
        assert need % (9 * plane * 8) == 0
        n_chunk = need // (9 * plane * 8)
        assert n_chunk == 0 or 2 <= n_chunk <= -(-n // 8)
    assert lib.cae_pixel_sums_workspace_bytes(70000, 4, 0) > 1000 * 9 * 4 * 8


def test_cli_flags_equal_evaluate_cae():
    from cae_tools_amd.cli import evaluate_cae, skill_maps as cli
    flags = lambda parser: [(a.option_strings, a.dest, a.nargs, a.default, a.required, a.type)   # noqa: E731
                            for a in parser._actions if a.option_strings and a.dest != "help"]
    assert flags(cli.build_parser()) == flags(evaluate_cae.build_parser())
    with open(os.path.join(HERE, "golden", "evaluate_cae_flags.json")) as f:
        assert [a[0][0] for a in flags(cli.build_parser())] == json.load(f)


def test_report_is_unchanged_without_the_maps_link():
    with open(os.path.join(HERE, "golden", "report_layout.json")) as f:
        fixture = json.load(f)
    rec = fixture["record"]
    rng = np.random.default_rng(7)
    measures = [(p, {m: rng.random(20) for m in rec["measures"]}) for p in rec["partitions"]]
    page = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"])
    assert report_items(page) == fixture["items"]
    assert page == report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], None, None)
    assert "maps/index.html" not in page
    linked = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], maps_link="maps/index.html")
    assert linked.count('href="maps/index.html"') == 1
    # the link is one paragraph more and nothing else
    extra = [line for line in linked.splitlines() if line not in page.splitlines()]
    assert len(linked.splitlines()) == len(page.splitlines()) + 3 and any("maps/index.html" in line for line in extra)


def test_netcdf_round_trip(tmp_path):
    from cae_tools_amd.data.arrays import open_dataset
    (p, a) = _cases()
    maps = skill_maps.maps_from_sums(chunked_sums(p, a, 292.5, 8).reshape(9, 1, 13))
    y = np.array([55.5])
    x = np.linspace(-5.0, 5.0, 13)
    path = skill_maps.write_netcdf(str(tmp_path / "skill_test.nc"), maps, ("lat", "lon"),
                                   {"y": ("lat", y, {"units": "degrees_north"}), "x": ("lon", x, {})})
    ds = open_dataset(path)
    for m in MAPS:
        v = np.asarray(ds[m].values)
        assert v.dtype.itemsize == 8 and tuple(ds[m].dims) == ("lat", "lon") and v.shape == (1, 13)
        np.testing.assert_array_equal(v, maps[m])
    np.testing.assert_array_equal(np.asarray(ds["y"].values), y)
    np.testing.assert_array_equal(np.asarray(ds["x"].values), x)
    assert tuple(ds["x"].dims) == ("lon",) and ds["y"].attrs["units"] == "degrees_north"


def test_range_rule():
    found = {"a": (1.5, 4.0, 10), "b": (-7.0, 2.0, 3), "none": (np.inf, -np.inf, 0)}
    assert skill_maps.map_range("count", [found["a"], found["b"]], 37) == (0.0, 37.0)
    assert skill_maps.map_range("bias", [found["a"], found["b"]], 37) == (-7.0, 7.0)
    assert skill_maps.map_range("rmse", [found["a"], found["b"], found["none"]], 37) == (-7.0, 4.0)
    assert skill_maps.map_range("correlation", [found["none"], found["none"]], 37) == (0.0, 0.0)
    assert skill_maps.map_range("bias", [found["none"]], 37) == (0.0, 0.0)
    # the same rule as the tests' restatement
    (p, a) = _cases()
    parts = [skill_maps.maps_from_sums(chunked_sums(p[:k], a[:k], 292.5, 8)) for k in (37, 20)]
    for m in MAPS:
        spans = []
        for maps in parts:
            v = maps[m][np.isfinite(maps[m])]
            spans.append((v.min(), v.max(), v.size) if v.size else (np.inf, -np.inf, 0))
        assert skill_maps.map_range(m, spans, 37) == range_rule(m, parts, 37)


def test_maps_page(tmp_path):
    rng = np.random.default_rng(3)
    (h, w) = (5, 7)
    parts = []
    rows = {}
    for (partition, n) in (("test", 12), ("train", 20)):
        layers = []
        for (k, m) in enumerate(MAPS):
            sl = rng.integers(0, 256, size=(h, w + 1), dtype=np.uint8)
            sl[:, 0] = 0
            rows[partition, m] = sl
            layers.append((m, -1.5 * k, 0.25 + k, sl))
        parts.append((partition, n, layers))
    folder = str(tmp_path / "maps")
    path = skill_maps.write_maps_page(folder, parts)
    assert path == os.path.join(folder, "index.html")
    with open(path) as f:
        page = f.read()
    assert sorted(os.listdir(folder)) == sorted(["index.html", "colourbar.png"] + [f"{p}_{m}.png" for p in ("test", "train")
                                                                                 for m in MAPS])
    for partition in ("test", "train"):
        assert re.findall(rf'<img src="({partition}_[a-z_]+\.png)"', page) == [f"{partition}_{m}.png" for m in MAPS]
        for m in MAPS:
            with open(os.path.join(folder, f"{partition}_{m}.png"), "rb") as f:
                assert decode_png(f.read()) == (w, h, rows[partition, m].tobytes())
    assert re.findall(r'data-layer="([^"]+)"', page) == list(MAPS) * 2
    assert "test (12 cases)" in page and "train (20 cases)" in page
    for k in range(len(MAPS)):
        assert page.count(f"{-1.5 * k:.6g} … {0.25 + k:.6g}") == 2
