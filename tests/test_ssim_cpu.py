"""The host side of the SSIM evaluator without a GPU: the numpy restatement of the definition (ssim_ref.py) against the
oracle's per_scale_terms and ms_ssim in fp64 within the derived bound, the rules of utils/ssim.scores_from_sums, the strict
JSON, the command's flags, the report's section, and a mutant of the reference that must miss the bound.

Largest |oracle fp64 - reference| / bound measured (each check prints its figure): 9.6e-3 (177 x 161, eps 1e-6), 7.1e-3 at
161 x 161; the oracle filters columns first and pools with torch's own order of the four additions, both inside the bound's
allowance.  The mutant misses the bound by factors of 1.7e9 and more."""
import hashlib
import json
import math
import os

import numpy as np
import pytest

import ssim_ref
from ssim_ref import Reference
from cae_tools_amd.utils import report, ssim

HERE = os.path.dirname(os.path.abspath(__file__))
(VMIN, VMAX) = (290.0, 295.0)


def _pair(rng, shape, eps, n=1):
    """targets 290 + 5 U, predictions a + 5 eps N(0, 1): normalised fields in about [0, 1]"""
    a = VMIN + (VMAX - VMIN) * rng.random((n,) + shape)
    p = a + (VMAX - VMIN) * eps * rng.standard_normal((n,) + shape)
    return p, a


def test_window_and_weights_are_the_oracles():
    from oracle import vae_oracle as vo
    import torch
    want = vo.gaussian_window(torch.float32).numpy()
    assert want.dtype == np.float32
    for w in (ssim.window(), ssim_ref.window()):
        assert w.dtype == np.float64 and w.shape == (11,) and w.tobytes() == want.astype(np.float64).tobytes()
    assert ssim.MS_WEIGHTS == ssim_ref.MS_WEIGHTS == tuple(vo.scale_weights(torch.float64).reshape(-1).tolist())
    assert (ssim.WIN_SIZE, ssim.MAX_SCALES) == (vo.WIN_SIZE, len(vo.MS_WEIGHTS))
    assert (ssim_ref.C1, ssim_ref.C2) == (vo.K1 ** 2, vo.K2 ** 2)


@pytest.mark.parametrize("eps", [0.1, 1e-6])
@pytest.mark.parametrize("shape", [(161, 161), (177, 161)])
def test_reference_against_the_oracle_in_fp64(shape, eps):
    from oracle import vae_oracle as vo
    import torch
    rng = np.random.default_rng(shape[0] + int(eps * 10))
    (p, a) = _pair(rng, shape, eps, n=2)
    ref = Reference(p, a, VMIN, VMAX, 5)
    assert [int(v) for v in ref.sums[0, :, 0]] == [(h - 10) * (w - 10) for (h, w) in ssim_ref.scale_shapes(*shape, 5)]
    if shape == (161, 161):
        assert ref.sums[0, 4, 0] == 1           # exactly one window at the last scale
    x = torch.from_numpy(ssim_ref.normalise(p, VMIN, VMAX))[:, None]
    y = torch.from_numpy(ssim_ref.normalise(a, VMIN, VMAX))[:, None]
    terms = vo.per_scale_terms(x, y).numpy()[:, :, 0]              # (5, N): mean cs of scales 0..3, mean ssim of scale 4
    n = ref.sums[:, :, 0]
    worst = 0.0
    for s in range(5):
        k = 2 if s < 4 else 1
        (want, bound) = (ref.sums[:, s, k] / n[:, s], ref.bound[:, s, k] / n[:, s])
        worst = max(worst, float(np.max(np.abs(terms[s] - want) / bound)))
        print(f"oracle fp64 vs reference {shape} eps={eps} scale {s}: |diff| {np.max(np.abs(terms[s] - want)):.3e}, "
              f"bound {np.max(bound):.3e}")
        assert (np.abs(terms[s] - want) <= bound).all(), (shape, eps, s)
    print(f"oracle fp64 vs reference {shape} eps={eps}: max |got - want| / bound = {worst:.3e}")
    # ms_ssim: the oracle's batch mean against the mean of the reference's per-case products; every factor f^w with
    # f in (0, 1] and w < 1 moves by at most w df / f, so the product by the sum of those
    (_, ms, _) = ssim_ref.scores(ref.sums, *shape)
    scored = ssim.scores_from_sums(ref.sums, *shape)
    assert (np.abs(scored["ms_ssim"] - ms) <= 8 * ssim_ref.U * ms).all()       # five powers and four products, each rounded
    assert np.array_equal(scored["ssim"], ref.sums[:, 0, 1] / n[:, 0])
    got = float(vo.ms_ssim(x, y))
    tol = 0.0
    for c in range(2):
        f = [ref.sums[c, s, 2 if s < 4 else 1] / n[c, s] for s in range(5)]
        assert min(f) > 0
        tol += sum(ssim.MS_WEIGHTS[s] * (ref.bound[c, s, 2 if s < 4 else 1] / n[c, s]) / f[s] for s in range(5)) * ms[c] / 2
    tol += 16 * ssim_ref.U * float(np.mean(ms))
    print(f"oracle ms_ssim {shape} eps={eps}: |diff| {abs(got - float(np.mean(ms))):.3e}, bound {tol:.3e}")
    assert abs(got - float(np.mean(ms))) <= tol


def test_scores_from_sums_rules():
    sums = np.zeros((4, 5, 3))
    sums[0] = [[100, 90, 95], [50, 40, 45], [20, 18, 19], [10, 9, 9.5], [1, 0.5, 0.75]]
    sums[1] = sums[0]
    sums[1, 2] = 0                              # a scale without a counted window: no ms_ssim
    sums[2] = sums[0]
    sums[2, 1] = [50, 40, -5]                   # a negative mean cs: the relu makes the product 0
    sums[3] = 0                                 # no window at all
    mse = np.array([0.25, 0.0, np.nan, 1e-4])
    s = ssim.scores_from_sums(sums, 161, 200, mse=mse, vmin=290.0, vmax=295.0)
    w = ssim.MS_WEIGHTS
    want = 0.95 ** w[0] * 0.9 ** w[1] * 0.95 ** w[2] * 0.95 ** w[3] * 0.5 ** w[4]
    assert s["ssim"][:3].tolist() == [0.9, 0.9, 0.9] and math.isnan(s["ssim"][3])
    assert abs(s["ms_ssim"][0] - want) <= 4 * 2.0 ** -53 and math.isnan(s["ms_ssim"][1]) and s["ms_ssim"][2] == 0.0
    assert math.isnan(s["ms_ssim"][3])
    assert s["psnr"][0] == 10.0 * np.log10(25.0 / 0.25) == 20.0 and s["psnr"][1] == math.inf and math.isnan(s["psnr"][2])
    assert abs(s["psnr"][3] - 10.0 * math.log10(25.0 / 1e-4)) < 1e-12
    assert s["windows"].dtype == np.int64 and s["windows"][0].tolist() == [100, 50, 20, 10, 1]
    # the 160 / 161 rule: pytorch_msssim's condition is on the smaller side
    assert math.isnan(ssim.scores_from_sums(sums, 160, 400)["ms_ssim"][0])
    assert math.isnan(ssim.scores_from_sums(sums, 400, 160)["ms_ssim"][0])
    assert ssim.scores_from_sums(sums, 161, 161)["ms_ssim"][0] == s["ms_ssim"][0]
    assert (ssim.default_scales(160, 400), ssim.default_scales(161, 161)) == (1, 5)
    # fewer than five scales: ssim alone, and no psnr without an mse
    one = ssim.scores_from_sums(sums[:, :1], 400, 400)
    assert np.isnan(one["ms_ssim"]).all() and one["ssim"][0] == 0.9 and np.isnan(one["psnr"]).all()
    assert ssim.scale_shapes(177, 161, 5) == ssim_ref.scale_shapes(177, 161, 5) == [(177, 161), (89, 81), (45, 41), (23, 21), (12, 11)]
    assert ssim.scale_shapes(23, 22, 2) == [(23, 22), (12, 11)]


def test_json_is_strict_and_the_line(tmp_path):
    sums = np.zeros((3, 1, 3))
    sums[0, 0] = [4, 3, 3.5]
    sums[1, 0] = [2, 2, 2]
    scores = ssim.scores_from_sums(sums, 20, 30, mse=np.array([1.0, 0.0, np.nan]), vmin=0.0, vmax=2.0)
    rec = ssim.summary(scores, 20, 30, 0.0, 2.0)
    path = ssim.write_json(str(tmp_path / "ssim_test.json"), rec)
    text = open(path).read()
    assert "NaN" not in text and "Infinity" not in text
    back = json.loads(text, parse_constant=lambda name: pytest.fail(f"not strict JSON: {name}"))
    assert (back["n_cases"], back["h"], back["w"], back["vmin"], back["vmax"]) == (3, 20, 30, 0.0, 2.0)
    assert back["scales"] == [[20, 30]] and (back["n_counted"], back["n_counted_ms"]) == (2, 0)
    assert back["ssim"] == 0.875 and back["ms_ssim"] is None and back["psnr"] is None      # the mean of {6.02.., inf}
    assert back["case_ssim"] == [0.75, 1.0, None] and back["case_ms_ssim"] == [None, None, None]
    assert abs(back["case_psnr"][0] - 10.0 * math.log10(4.0)) < 1e-12 and back["case_psnr"][1:] == [None, None]
    assert back["windows"] == [[4], [2], [0]]
    assert ssim.line("test", rec) == "ssim test: ssim 0.875 ms_ssim none psnr inf dB, 2/3 cases"
    rec2 = ssim.summary(ssim.scores_from_sums(sums[:1], 20, 30, mse=np.array([1.0]), vmin=0.0, vmax=2.0), 20, 30, 0.0, 2.0)
    assert ssim.line("train", rec2) == "ssim train: ssim 0.75 ms_ssim none psnr 6.0206 dB, 1/1 cases"


def test_cli_flags_equal_evaluate_cae():
    from cae_tools_amd.cli import evaluate_cae, ssim as cli
    flags = lambda parser: [(a.option_strings, a.dest, a.nargs, a.default, a.required, a.type)   # noqa: E731
                            for a in parser._actions if a.option_strings and a.dest != "help"]
    assert flags(cli.build_parser()) == flags(evaluate_cae.build_parser())


# sha256 of evaluation_report's page for the golden record, as test_spectra_cpu.py holds it
REPORT_SHA256 = "0a26c705f2bab559c1df1dee37ad957c941d84ce2aa0652d349c3549845789f1"


def test_report_section_is_off_by_default():
    with open(os.path.join(HERE, "golden", "report_layout.json")) as f:
        rec = json.load(f)["record"]
    rng = np.random.default_rng(7)
    measures = [(p, {m: rng.random(20) for m in rec["measures"]}) for p in rec["partitions"]]
    page = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"])
    assert hashlib.sha256(page.encode("utf-8")).hexdigest() == REPORT_SHA256
    assert page == report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], ssim=None)
    assert "Structural similarity" not in page
    sums = np.zeros((3, 1, 3))
    sums[:, 0] = [[4, 3, 3.5], [2, 2, 2], [0, 0, 0]]
    record = ssim.summary(ssim.scores_from_sums(sums, 20, 30, mse=np.array([1.0, 0.5, 2.0]), vmin=0.0, vmax=2.0), 20, 30, 0.0, 2.0)
    with_section = report.evaluation_report(rec["metrics"], measures, rec["parameters"], rec["history"], ssim=[("test", record)])
    assert with_section.count("Structural similarity") == 1 and "test: 2 of 3 cases, 1 scale" in with_section
    assert with_section.count('alt="test ssim histogram"') == 1
    for cell in ("<td>ssim</td>", "<td>0.875</td>", "<td>ms_ssim</td>", "<td>none</td>", "<td>psnr (dB)</td>"):
        assert cell in with_section, cell
    assert with_section.count("<img") == page.count("<img") + 1


@pytest.mark.parametrize("shape,n_scale", [((11, 11), 1), ((45, 47), 3)])
def test_a_window_without_its_first_tap_misses_the_bound(shape, n_scale):
    rng = np.random.default_rng(3)
    (p, a) = _pair(rng, shape, 0.1, n=2)
    ref = Reference(p, a, VMIN, VMAX, n_scale)
    assert ref.ratio(ref.sums) == 0.0
    g = ssim_ref.window()
    g[0] = 0.0
    (mutant, _) = ssim_ref.case_sums(p, a, VMIN, VMAX, n_scale, g)
    np.testing.assert_array_equal(mutant[:, :, 0], ref.sums[:, :, 0])
    err = np.abs(mutant - ref.sums)[:, :, 1:]
    print(f"mutant {shape}: least |mutant - want| / bound = {float(np.min(err / ref.bound[:, :, 1:])):.3e}")
    assert (err > ref.bound[:, :, 1:]).all()
    with pytest.raises(AssertionError):
        ref.check(mutant, "mutant")


def test_missing_data_rule_of_the_reference():
    """a NaN loses exactly the windows over it, at the scale it is at and at the pooled pixel's below; the rest of the case
    is untouched"""
    rng = np.random.default_rng(9)
    (p, a) = _pair(rng, (45, 47), 0.1, n=1)
    clean = Reference(p, a, VMIN, VMAX, 3)
    q = p.copy()
    q[0, 20, 30] = np.nan
    holed = Reference(q, a, VMIN, VMAX, 3)
    # scale 0: 11 x 11 windows over (20, 30), all inside; scale 1 (23 x 24, pad 1 on both axes: pixel ((20 + 1) // 2,
    # (30 + 1) // 2) = (10, 15)): rows 0..10 and columns 5..13 of 13 x 14 positions; scale 2 (12 x 12): pixel (5, 7), both
    # positions of either axis that hold it
    assert clean.sums[0, :, 0].tolist() == [35 * 37, 13 * 14, 2 * 2]
    assert holed.sums[0, :, 0].tolist() == [35 * 37 - 121, 13 * 14 - 11 * 9, 0]
    assert (holed.sums[0, 2] == 0).all() and np.isfinite(holed.sums).all()
