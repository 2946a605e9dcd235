"""utils/spectra.py without a GPU: the bin table against its float restatement and hand-listed tables, the window, the
curves and the effective resolution from sums the numpy reference makes (spectra_ref.py), the writers, the CLI's flags and
the report, which stays what it is without the spectra link."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import spectra_ref
from cae_tools_amd.utils import report, spectra

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (2, 2), (3, 5), (4, 4), (17, 19), (16, 64), (64, 16), (33, 128), (81, 81)]


def test_hand_listed_tables():
    np.testing.assert_array_equal(spectra.bin_table(3, 5), [[-1, 0, 0], [0, 0, -1], [0, 0, -1]])
    np.testing.assert_array_equal(spectra.bin_table(4, 4), [[-1, 1, -1], [1, 1, -1], [-1, -1, -1], [1, 1, -1]])
    assert spectra.bin_table(1, 1).tolist() == [[-1]]
    assert (spectra.bin_table(2, 2) == -1).all()
    assert spectra.bin_table(4, 4).dtype == np.int32


@pytest.mark.parametrize("shape", SHAPES)
def test_table_against_the_float_rule(shape):
    (h, w) = shape
    m = spectra.bin_count(h, w)
    assert m == max(1, min(h, w) // 2)
    table = spectra.bin_table(h, w)
    assert table.shape == (h, w // 2 + 1)
    assert table.min() >= -1 and table.max() < m and table[0, 0] == -1
    np.testing.assert_array_equal(table, spectra_ref.bin_table(h, w))
    checked = 0
    for ky in range(h):
        for kx in range(w // 2 + 1):
            v = 2.0 * m * math.sqrt((min(ky, h - ky) / h) ** 2 + (kx / w) ** 2)
            if abs(v - round(v)) < 1e-9:            # on an edge: the integer rule decides, not a rounding
                continue
            want = -1 if (ky, kx) == (0, 0) or math.floor(v) >= m else math.floor(v)
            assert table[ky, kx] == want, (ky, kx, v)
            checked += 1
    assert checked > 0 or h * w <= 4
    # the modes of the bins: every kept mode of the full plane once
    full = sum(1 for ky in range(h) for kx in range(w) if table[ky, min(kx, w - kx)] >= 0)
    modes = spectra.bin_modes(h, w)
    assert modes.shape == (m,) and modes.sum() == full
    np.testing.assert_array_equal(modes, spectra_ref.modes(h, w))


def test_window():
    assert spectra.window(1).tolist() == [1.0]
    for n in (2, 3, 16, 81):
        # an argument near 2 pi carries half an ulp(2 pi) = 4 * 2^-53 per rounding, two roundings, halved by the 1/2 and
        # taken twice where two entries are compared: 8 * 2^-53, and as much again for cos and the subtraction
        win = spectra.window(n)
        assert win.dtype == np.float64 and win.shape == (n,)
        np.testing.assert_allclose(win, spectra_ref.window(n), rtol=0, atol=16 * 2.0 ** -53)
        np.testing.assert_allclose(win, win[::-1], rtol=0, atol=16 * 2.0 ** -53)       # centred
        assert (win > 0).all() and win.max() <= 1.0
    np.testing.assert_allclose(spectra.window(2), [0.5, 0.5], atol=1e-16)


def _blur(a):
    """the 3 x 3 box mean, periodic"""
    return sum(np.roll(np.roll(a, dy, axis=-2), dx, axis=-1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0


def _blur_gain(h, w):
    """the box mean's power transfer in every radial bin: the mean of |T|^2 over the bin's modes"""
    table = spectra_ref.bin_table(h, w)
    ty = (1.0 + 2.0 * np.cos(2.0 * np.pi * np.arange(h) / h)) / 3.0
    tx = (1.0 + 2.0 * np.cos(2.0 * np.pi * np.arange(w // 2 + 1) / w)) / 3.0
    gain = (ty[:, None] * tx[None, :]) ** 2 * spectra_ref.weights(w)[None, :]
    keep = table >= 0
    m = spectra_ref.bin_count(h, w)
    return np.bincount(table[keep], weights=gain[keep], minlength=m) / np.maximum(spectra_ref.modes(h, w), 1.0)      # bin 0 is empty


def test_curves_of_a_blurred_prediction():
    (n, h, w) = (6, 32, 32)
    rng = np.random.default_rng(3)
    a = 290.0 + 5.0 * rng.random((n, h, w))
    p = _blur(a)
    (sums, counted, _) = spectra_ref.case_sums(p, a)
    curves = spectra.curves_from_sums(sums, counted, h, w)
    m = spectra.bin_count(h, w)
    assert set(curves) == {"modes", "wavelength", "psd_pred", "psd_target", "power_ratio", "coherence", "error_share",
                           "n_cases", "n_counted", "effective_resolution"}
    assert all(len(curves[k]) == m for k in curves if isinstance(curves[k], list))
    assert (curves["n_cases"], curves["n_counted"]) == (n, n)
    assert curves["wavelength"] == [2.0 * m / (b + 0.5) for b in range(m)]
    ratio = np.array(curves["power_ratio"])
    gain = _blur_gain(h, w)
    # white noise under a Hann window: the ratio follows the box mean's transfer, which falls from 1 to 0 at f = 1/3
    third = int(2 * m / 3)
    assert np.isfinite(ratio[1:]).all() and ratio[1] > 0.95 and (np.diff(ratio[1:third]) < 0).all() and ratio[third] < 0.02
    np.testing.assert_allclose(ratio[1:], gain[1:], atol=0.03)
    expected = 1 + int(np.argmax(gain[1:] < 0.5))
    assert abs(gain[expected] - 0.5) > 0.03 and abs(gain[expected - 1] - 0.5) > 0.03       # not a marginal bin
    assert curves["effective_resolution"] == 2.0 * m / (expected + 0.5)
    # psd: the sums over what they are normalised by
    norm = n * np.array(curves["modes"]) * (spectra_ref.window(h) ** 2).sum() * (spectra_ref.window(w) ** 2).sum()
    np.testing.assert_allclose(np.array(curves["psd_target"])[1:], sums[:, 1:, 1].sum(axis=0) / norm[1:], rtol=1e-14)
    np.testing.assert_allclose(np.array(curves["psd_pred"])[1:], sums[:, 1:, 0].sum(axis=0) / norm[1:], rtol=1e-14)
    coherence = np.array(curves["coherence"])[1:]
    assert (np.abs(coherence) <= 1.0 + 1e-12).all() and coherence[0] > 0.99
    # the error's share is 1 where the prediction has lost the scale
    assert abs(curves["error_share"][third] - 1.0) < 0.2 and curves["error_share"][1] < 0.01


def test_no_effective_resolution_for_a_perfect_prediction():
    rng = np.random.default_rng(4)
    a = rng.random((3, 17, 19))
    (sums, counted, _) = spectra_ref.case_sums(a, a)
    curves = spectra.curves_from_sums(sums, counted, 17, 19)
    assert curves["effective_resolution"] is None
    assert curves["power_ratio"] == [1.0] * 8 and curves["coherence"] == pytest.approx([1.0] * 8, abs=1e-15)
    assert curves["error_share"] == [0.0] * 8


def test_uncounted_cases_and_empty_bins(tmp_path):
    rng = np.random.default_rng(5)
    a = rng.random((4, 4, 4))
    p = a + 0.1 * rng.random(a.shape)
    p[2, 1, 1] = np.nan
    (sums, counted, _) = spectra_ref.case_sums(p, a)
    assert counted.tolist() == [True, True, False, True] and (sums[2] == 0.0).all()
    curves = spectra.curves_from_sums(sums, counted, 4, 4)
    assert (curves["n_cases"], curves["n_counted"]) == (4, 3)
    # bin 0 of a 4 x 4 plane holds no mode: NaN in the curves, null in the file
    assert curves["modes"] == [0.0, 8.0]
    assert all(math.isnan(curves[k][0]) for k in ("psd_pred", "psd_target", "power_ratio", "coherence", "error_share"))
    path = spectra.write_json(str(tmp_path / "spectra_test.json"), curves, 4, 4)
    with open(path) as f:
        rec = json.load(f)
    assert rec["power_ratio"][0] is None and rec["power_ratio"][1] == curves["power_ratio"][1]
    assert (rec["h"], rec["w"], rec["n_cases"], rec["n_counted"], rec["effective_resolution"]) == (4, 4, 4, 3, None)
    # no case counted: every curve is NaN, nothing raises
    none = spectra.curves_from_sums(np.zeros((2, 2, 4)), [False, False], 4, 4)
    assert none["n_counted"] == 0 and all(math.isnan(v) for v in none["psd_pred"]) and none["effective_resolution"] is None
    page = spectra.write_page(str(tmp_path / "spectra"), [("test", curves), ("train", none)])
    with open(page) as f:
        text = f.read()
    assert text.count('class="spectra"') == 2 and text.count("<img") == 8
    assert "test: 3 of 4 cases, effective resolution not reached" in text


def test_cli_flags_equal_evaluate_cae():
    from cae_tools_amd.cli import evaluate_cae, spectra as cli
    flags = lambda parser: [(a.option_strings, a.dest, a.nargs, a.default, a.required, a.type)   # noqa: E731
                            for a in parser._actions if a.option_strings and a.dest != "help"]
    assert flags(cli.build_parser()) == flags(evaluate_cae.build_parser())


# sha256 of evaluation_report's page for the record below, taken before the spectra link existed
REPORT_SHA256 = "0a26c705f2bab559c1df1dee37ad957c941d84ce2aa0652d349c3549845789f1"


def test_report_is_unchanged_without_the_spectra_link():
    with open(os.path.join(HERE, "golden", "report_layout.json")) as f:
        rec = json.load(f)["record"]
    rng = np.random.default_rng(7)
    measures = [(p, {m: rng.random(20) for m in rec["measures"]}) for p in rec["partitions"]]
    page = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"])
    assert hashlib.sha256(page.encode("utf-8")).hexdigest() == REPORT_SHA256
    assert page == report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], spectra_link=None)
    assert "spectra/index.html" not in page
    linked = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], spectra_link="spectra/index.html")
    assert linked.count('href="spectra/index.html"') == 1
    lines = linked.splitlines()
    extra = [k for (k, line) in enumerate(lines) if "spectra/index.html" in line]
    assert len(extra) == 1 and lines[:extra[0] - 1] + lines[extra[0] + 2:] == page.splitlines()
