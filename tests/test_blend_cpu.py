"""The host side of the model blending without a GPU: the solver of the weights held to the same rule in fractions.Fraction
(blend_ref.py), its corner cases, the cross-validation against a direct loop, the record's round trip through blend.json, the
refusals of the settings and of both sub-commands with the GPU library unreachable, and the CAE_ERR_ARG refusals of
cae_case_error_moments and cae_blend_predictions with made-up addresses that are never dereferenced."""
import ctypes as C
import json
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import blend_ref
from cae_tools_amd import _lib
from cae_tools_amd.cli import blend as cli
from cae_tools_amd.utils import blend, compare

MODES = ("convex", "affine", "equal")


# ---- the solver ------------------------------------------------------------------------------------------------------------

def _integer_sums(rng, m, n=60):
    """(the row of moments of n integer-valued error vectors, as float64; n, Se, the products as Python integers): the errors
    share a part and have parts of their own of growing size, and the matrix S / n - with and without its mean taken out - has
    a condition number of at most 10^4"""
    while True:
        e = rng.integers(-6, 7, (n, 1)) + rng.integers(-4, 5, (n, m)) * (1 + np.arange(m) % 3) + rng.integers(-2, 3, (1, m))
        s = e.T @ e
        se = e.sum(axis=0)
        mean = se / n
        if max(np.linalg.cond(s / n), np.linalg.cond(s / n - np.outer(mean, mean))) <= 1e4:
            products = [int(s[i, j]) for (i, j) in blend_ref.pairs(m)]
            return np.array([n] + se.tolist() + products, dtype=np.float64), n, [int(v) for v in se], products


@pytest.mark.parametrize("intercept", [False, True], ids=["plain", "intercept"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m", range(1, 9))
def test_solve_against_the_fraction_solver(m, mode, intercept):
    """integer-valued sums, condition number <= 10^4: cond u is about 10^-12, the tolerance 100 times that, relative to the
    largest weight"""
    rng = np.random.default_rng(100 * m + 10 * MODES.index(mode) + intercept)
    for _ in range(3):
        (row, n, se, products) = _integer_sums(rng, m)
        (exact_e, exact_mean) = blend_ref.moments_exact(n, se, products, intercept)
        want = blend_ref.solve(exact_e, mode)
        (got, c) = blend.fit_sums(row, mode, intercept)
        (big_e, mean) = blend.moments(row)
        direct = blend.solve(blend.centred(big_e, mean) if intercept else big_e, mode)
        assert np.array_equal(got, direct) and got.shape == (m,)
        want_f = np.array([float(v) for v in want])
        worst = float(np.max(np.abs(got - want_f)) / np.max(np.abs(want_f)))
        print(f"M {m} {mode} intercept {intercept}: max |w - exact| / max |exact| = {worst:.3e}")
        assert worst <= 1e-10
        assert abs(float(np.sum(got)) - 1.0) <= 1e-12
        want_c = float(-sum(w * e for (w, e) in zip(want, exact_mean))) if intercept else 0.0
        assert abs(c - want_c) <= 1e-10 * max(1.0, abs(want_c))
        if mode == "convex":
            assert ((got == 0.0) == np.array([v == 0 for v in want])).all()      # the same support, zeros exact
            # never above the best diagonal entry, nor above equal weights; the mse is the quadratic form
            fitted = float(np.einsum("i,ij,j->", got, np.array([[float(v) for v in r] for r in exact_e]), got))
            assert fitted <= min(float(exact_e[k][k]) for k in range(m)) * (1 + 1e-12)
            assert abs(fitted - float(blend_ref.objective(exact_e, want))) <= 1e-10 * fitted


def test_a_batch_is_solved_matrix_by_matrix():
    rng = np.random.default_rng(7)
    batch = []
    for _ in range(20):
        x = rng.normal(0.0, 1.0, (30, 4)) + rng.normal(0.0, 1.0, (30, 1))
        batch.append(x.T @ x / 30)
    batch = np.stack(batch)
    batch[3] = np.nan                                                       # a resample without a pixel
    for mode in MODES:
        got = blend.solve(batch, mode)
        assert got.shape == (20, 4) and np.isnan(got[3]).all()
        for k in (0, 5, 19):
            assert np.array_equal(got[k], blend.solve(batch[k], mode))


def test_two_identical_candidates_give_the_first_the_weight():
    """the support {0, 1} is singular and skipped; {1} is not strictly lower than {0}"""
    big_e = np.array([[2.0, 2.0], [2.0, 2.0]])
    assert blend.solve(big_e, "convex").tolist() == [1.0, 0.0]
    assert blend_ref.solve([[2, 2], [2, 2]], "convex") == [1, 0]
    assert np.isnan(blend.solve(big_e, "affine")).all() and blend_ref.solve([[2, 2], [2, 2]], "affine") is None
    three = np.array([[3.0, 3.0, 1.0], [3.0, 3.0, 1.0], [1.0, 1.0, 2.0]])
    got = blend.solve(three, "convex")
    want = blend_ref.solve([[3, 3, 1], [3, 3, 1], [1, 1, 2]], "convex")
    assert got[1] == 0.0 and want[1] == 0 and np.allclose(got, [float(v) for v in want], rtol=1e-14, atol=0)
    # through fit: the table of a duplicated candidate
    row = np.array([10.0, 1.0, 1.0, 20.0, 20.0, 20.0])
    assert blend.fit(row[None], "convex")["weights"].tolist() == [1.0, 0.0]
    with pytest.raises(ValueError, match="the affine weights are not defined"):
        blend.fit(row[None], "affine")


def test_a_candidate_whose_optimum_is_negative_gets_exactly_zero():
    """candidate 1 is candidate 0 with more of the same error: the affine optimum extrapolates away from it"""
    big_e = np.array([[1.0, 1.5], [1.5, 4.0]])
    affine = blend.solve(big_e, "affine")
    assert affine[1] < 0.0 and abs(affine.sum() - 1.0) < 1e-15
    assert [float(v) for v in blend_ref.solve([[2, 3], [3, 8]], "affine")] == [1.25, -0.25] and np.allclose(affine, [1.25, -0.25], rtol=1e-14, atol=0)
    convex = blend.solve(big_e, "convex")
    assert convex.tolist() == [1.0, 0.0] and not np.signbit(convex[1])
    assert blend.solve(big_e, "equal").tolist() == [0.5, 0.5]


def test_convex_never_exceeds_the_best_diagonal_entry():
    rng = np.random.default_rng(11)
    for m in range(1, 9):
        for _ in range(10):
            x = rng.normal(0.0, 1.0, (m + 3, m)) * rng.gamma(2.0, 1.0, m)
            big_e = x.T @ x / (m + 3)
            w = blend.solve(big_e, "convex")
            assert (w >= 0.0).all() and abs(w.sum() - 1.0) < 1e-12
            assert float(w @ big_e @ w) <= float(np.min(np.diag(big_e))) * (1 + 1e-12)
    with pytest.raises(ValueError, match="blend_mode must be one of convex, affine, equal"):
        blend.solve(np.eye(2), "ridge")
    with pytest.raises(ValueError, match="a matrix"):
        blend.solve(np.eye(9), "convex")


# ---- the cross-validation ----------------------------------------------------------------------------------------------------

def _table(rng, n_unit, m, pixels=50):
    rows = []
    for _ in range(n_unit):
        e = rng.normal(0.0, 1.0, (pixels, 1)) + rng.normal(0.1, 1.0, (pixels, m)) * (1.0 + 0.5 * np.arange(m))
        s = e.T @ e
        rows.append([pixels] + e.sum(axis=0).tolist() + [s[i, j] for (i, j) in blend_ref.pairs(m)])
    return np.array(rows, dtype=np.float64)


@pytest.mark.parametrize("intercept", [False, True], ids=["plain", "intercept"])
def test_folds_and_out_of_fold_sums_against_a_direct_loop(intercept):
    assert blend.fold_of(7, 3).tolist() == [0, 1, 2, 0, 1, 2, 0]
    rng = np.random.default_rng(5)
    (m, n_unit, folds) = (3, 11, 4)
    table = _table(rng, n_unit, m)
    found = blend.cross_validate(table, folds, "convex", intercept)
    (sq_blend, sq_best, sq_equal, pixels) = (0.0, 0.0, 0.0, 0.0)
    for f in range(folds):
        train = np.zeros(table.shape[1])
        test = np.zeros(table.shape[1])
        for u in range(n_unit):                     # ascending unit order, plain adds
            if u % folds == f:
                test = test + table[u]
            else:
                train = train + table[u]
        (w, c) = blend.fit_sums(train, "convex", intercept)
        assert np.array_equal(found["fold_weights"][f], w) and found["fold_intercepts"][f] == c
        (n_f, se_f, s_f) = blend.unpack(test)
        best = int(np.argmin([train[1 + m + blend_ref.pairs(m).index((k, k))] / train[0] for k in range(m)]))
        assert found["fold_best_single"][f] == best and found["fold_pixels"][f] == n_f
        sq_blend += float(w @ s_f @ w + 2.0 * c * (w @ se_f) + c * c * n_f)
        sq_best += float(s_f[best, best])
        sq_equal += float(np.full(m, 1 / 3) @ s_f @ np.full(m, 1 / 3))
        pixels += float(n_f)
    assert found["folds"] == folds and pixels == 11 * 50
    assert math.isclose(found["mse_blend"], sq_blend / pixels, rel_tol=1e-14)
    assert math.isclose(found["mse_best_single"], sq_best / pixels, rel_tol=1e-14)
    assert math.isclose(found["mse_equal"], sq_equal / pixels, rel_tol=1e-14)
    assert found["gain"] == 1.0 - found["mse_blend"] / found["mse_best_single"]
    for bad in (1, 12, -1, 2.5):
        with pytest.raises(ValueError, match="blend_folds"):
            blend.cross_validate(table, bad)


# ---- the record ------------------------------------------------------------------------------------------------------------

def test_summary_and_the_json_round_trip(tmp_path):
    rng = np.random.default_rng(9)
    table = _table(rng, 12, 3)
    j = rng.integers(0, 12, (200, 12))
    resampled = table[j].sum(axis=1)
    rec = blend.summary(table, resampled, ["p0", "p1", "p2"], ["a", "b", "c"], "convex", True, Fraction(19, 20), 200, 4, 3,
                        n_cases=12, plane=50)
    found = blend.fit(table, "convex", True)
    assert rec["weights"] == found["weights"].tolist() and rec["intercept"] == found["intercept"] != 0.0
    assert rec["pixels_counted"] == 600 and rec["pixels_left_out"] == 0 and (rec["n_cases"], rec["n_unit"]) == (12, 12)
    assert rec["mse_blend"] <= rec["mse_best_single"] == min(c["mse"] for c in rec["candidates"]) and rec["best_single"] == "a"
    assert rec["gain"]["value"] == 1.0 - rec["mse_blend"] / rec["mse_best_single"] >= 0.0
    assert rec["gain"]["interval"][0] <= rec["gain"]["interval"][1] and rec["gain"]["degenerate"] == 0
    corr = np.asarray(rec["error_correlation"])
    assert corr.shape == (3, 3) and np.allclose(np.diag(corr), 1.0) and np.allclose(corr, corr.T) and (np.abs(corr) <= 1 + 1e-12).all()
    for (k, cand) in enumerate(rec["candidates"]):
        total = compare.column_sums(table)
        assert cand["bias"] == total[1 + k] / total[0] and cand["weight"]["value"] == rec["weights"][k]
        (wb, _) = blend.fit_sums(resampled, "convex", True)
        (lo, hi) = cand["weight"]["interval"]
        kept = np.sort(wb[:, k])
        (rank_lo, rank_hi) = compare.interval_ranks(200, Fraction(19, 20))
        assert (lo, hi) == (kept[rank_lo - 1], kept[rank_hi - 1])
    assert rec["cross_validation"]["folds"] == 3 and rec["cross_validation"]["fold_weights"].shape == (3, 3)
    path = blend.write_json(str(tmp_path / "blend.json"), dict(rec, extra=math.nan))
    with open(path) as f:
        stored = json.loads(f.read(), parse_constant=lambda name: pytest.fail(f"{name} is not strict JSON"))
    assert stored["extra"] is None and stored["weights"] == rec["weights"]
    for (text, w) in zip(stored["weights_hex"], found["weights"]):
        assert float.fromhex(text) == w
    assert float.fromhex(stored["intercept_hex"]) == found["intercept"]
    (variables, w, c, again) = blend.read_json(path)
    assert variables == ["p0", "p1", "p2"] and np.array_equal(w, found["weights"]) and c == found["intercept"] and again == stored
    text = blend.line(rec)
    assert text.startswith("blend: 3 candidates, 12 units, convex with intercept ") and "; cross-validated (3 folds) gain " in text
    assert " against a " in text
    page = blend.page(rec)
    assert page.count("<h2>Error correlation</h2>") == 1 and page.count('alt="weights of the blend"') == 1
    svg = blend.svg_weights(rec, "weights")
    assert svg.count('class="weight"') == 3 and svg.count('class="interval"') == 3
    rows = blend.correlation_rows(rec)
    assert rows[0] == ["", "a", "b", "c"] and [r[0] for r in rows[1:]] == ["a", "b", "c"] and rows[1][1] == "1"
    # without resamples and folds: no intervals, no cross-validation
    bare = blend.summary(table, None, ["p0", "p1", "p2"], ["a", "b", "c"], "equal", False, Fraction(19, 20), 0, 0, 0, n_cases=12, plane=50)
    assert bare["weights"] == [1 / 3] * 3 and bare["intercept"] == 0.0 and bare["cross_validation"] is None
    assert all(math.isnan(v) for v in bare["gain"]["interval"]) and blend.svg_weights(bare, "w").count('class="interval"') == 0
    for (broken, text) in (({"variables": ["a"]}, "is not a blend file"), ({"variables": ["a"], "weights_hex": ["x"], "intercept_hex": "0x0p+0"},
                                                                       "is not a blend file"),
                           ({"variables": ["a", "b"], "weights_hex": ["0x1p+0"], "intercept_hex": "0x0p+0"}, "one finite weight each")):
        with open(tmp_path / "broken.json", "w") as f:
            json.dump(broken, f)
        with pytest.raises(ValueError, match=text):
            blend.read_json(str(tmp_path / "broken.json"))


# ---- the settings and the command, with the GPU library unreachable ------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    def unreachable(*args, **kwargs):
        pytest.fail("the GPU library was loaded before the refusal")
    monkeypatch.setattr(_lib, "load", unreachable)


@pytest.mark.parametrize("call, text", [
    (lambda: blend.check_mode("ridge"), "blend_mode must be one of convex, affine, equal, got 'ridge'"),
    (lambda: blend.check_resamples(-1), "blend_resamples must be an integer from 0 to 1000000, got -1"),
    (lambda: blend.check_resamples(10 ** 6 + 1), "blend_resamples must be an integer from 0 to 1000000, got 1000001"),
    (lambda: blend.check_resamples(2.5), "blend_resamples must be an integer from 0 to 1000000, got 2.5"),
    (lambda: blend.check_resamples(True), "blend_resamples must be an integer from 0 to 1000000, got True"),
    (lambda: blend.check_seed(-1), "blend_seed must be an integer from 0 to 2^64 - 1, got -1"),
    (lambda: blend.check_seed(1 << 64), f"blend_seed must be an integer from 0 to 2^64 - 1, got {1 << 64}"),
    (lambda: blend.check_folds(1), "blend_folds must be 0 (no cross-validation) or at least 2, got 1"),
    (lambda: blend.check_folds(-2), "blend_folds must be an integer from 0 to 1048576, got -2"),
    (lambda: blend.check_folds(5, 4), "blend_folds: 5 folds need at least as many resampling units, there are 4"),
    (lambda: blend.parse_confidence("1.0"), "blend_confidence: coverage level '1.0' is not between 0 and 1"),
    (lambda: blend.parse_confidence(0.95), "blend_confidence: coverage level 0.95: give the decimal text or a Fraction, a float has already lost it"),
    (lambda: blend.check_candidates([]), "blend_variables: 1 to 8 variables expected, got 0"),
    (lambda: blend.check_candidates(list("abcdefghi")), "blend_variables: 1 to 8 variables expected, got 9"),
    (lambda: blend.check_candidates(["a", "a"]), "blend_variables: 'a' is named twice"),
    (lambda: blend.check_candidates(["a", "b"], ["x"]), "blend_labels: 2 labels expected, one per candidate, got 1"),
    (lambda: blend.check_candidates(["a", "b"], ["x", "x"]), "blend_labels: the labels must differ"),
])
def test_refusals_of_the_settings(no_library, call, text):
    with pytest.raises(ValueError) as refused:
        call()
    assert str(refused.value) == text


def test_the_settings_that_pass():
    assert blend.check_candidates(["a", "b"]) == (["a", "b"], ["a", "b"]) and blend.check_candidates(["a"], ["x"]) == (["a"], ["x"])
    assert (blend.check_folds(0), blend.check_folds(2, 2), blend.check_resamples(0), blend.check_seed((1 << 64) - 1)) == (0, 2, 0, (1 << 64) - 1)
    assert blend.parse_confidence("9/10") == Fraction(9, 10)
    assert [blend.width(m) for m in (1, 2, 8)] == [3, 6, 45] and blend.candidates_of(45) == 8
    with pytest.raises(ValueError, match="rows of 1"):
        blend.candidates_of(7)
    assert blend.supports(3) == [[0], [1], [2], [0, 1], [0, 2], [1, 2], [0, 1, 2]] and len(blend.supports(8)) == 255


def test_cli_parser(no_library):
    parser = cli.build_parser()
    args = parser.parse_args(["fit", "--inputs", "a.nc", "b.nc", "--output-variable", "hires", "--blend-variables", "u", "v"])
    assert (args.inputs, args.output_variable, args.blend_variables, args.blend_labels) == (["a.nc", "b.nc"], "hires", ["u", "v"], None)
    assert (args.blend_mode, args.blend_intercept, args.blend_block_variable, args.blend_folds, args.blend_resamples) == ("convex", False, None, 5, 2000)
    assert (args.blend_seed, args.blend_confidence, args.blend_file, args.output_html_folder) == (0, "0.95", "blend.json", None)
    args = parser.parse_args(["fit", "--inputs", "a.nc", "--output-variable", "hires", "--blend-variables", "u", "--blend-labels", "x",
                              "--blend-mode", "affine", "--blend-intercept", "--blend-block-variable", "day", "--blend-folds", "0",
                              "--blend-resamples", "0", "--blend-seed", "7", "--blend-confidence", "9/10", "--blend-file", "w.json",
                              "--output-html-folder", "report"])
    assert (args.blend_mode, args.blend_intercept, args.blend_block_variable, args.blend_folds, args.blend_resamples) == ("affine", True, "day", 0, 0)
    assert (args.blend_seed, args.blend_confidence, args.blend_file, args.output_html_folder, args.blend_labels) == (7, "9/10", "w.json", "report", ["x"])
    args = parser.parse_args(["apply", "a.nc", "b.nc", "out.nc", "--blend-file", "w.json"])
    assert (args.data_paths, args.output_path, args.blend_file, args.prediction_variable) == (["a.nc", "b.nc"], "out.nc", "w.json", "blend_output")
    fit = ["fit", "--inputs", "a.nc", "--output-variable", "hires", "--blend-variables", "u"]
    for bad in (fit + ["--blend-mode", "ridge"], fit + ["--blend-folds", "1"], fit + ["--blend-folds", "x"], fit + ["--blend-resamples", "-1"],
                fit + ["--blend-resamples", "1000001"], fit + ["--blend-seed", "-1"], fit + ["--blend-confidence", "1"],
                fit + ["--blend-confidence", "abc"], fit + ["--blend-labels"], fit[:-2], ["fit", "--inputs", "a.nc", "--blend-variables", "u"],
                ["apply", "a.nc", "out.nc"], ["apply", "out.nc", "--blend-file", "w.json"], ["blend"], []):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)


@pytest.fixture
def scored(tmp_path):
    from cae_tools_amd.data import netcdf3
    path = str(tmp_path / "scored.nc")
    field = np.zeros((4, 1, 6, 5), dtype=np.float32)
    netcdf3.write(path, {"n": 4, "c": 1, "c2": 2, "y": 6, "x": 5, "y2": 3},
                  {"hires": (("n", "c", "y", "x"), field, {}), "u": (("n", "c", "y", "x"), field, {}), "v": (("n", "c", "y", "x"), field, {}),
                   "two": (("n", "c2", "y", "x"), np.zeros((4, 2, 6, 5), dtype=np.float32), {}),
                   "small": (("n", "c", "y2", "x"), field[:, :, :3], {}), "day": (("n",), np.array([1.0, 1.0, 2.0, 2.0]), {}),
                   "row": (("y",), np.arange(6.0), {})})
    return path


def test_fit_refuses_before_the_gpu_library_is_loaded(no_library, scored, tmp_path):
    base = ["fit", "--inputs", scored, "--output-variable", "hires", "--blend-file", str(tmp_path / "never.json")]
    for (flags, text) in ((["--blend-variables", "u", "u"], "'u' is named twice"),
                          (["--blend-variables", *"abcdefghi"], "1 to 8 variables expected, got 9"),
                          (["--blend-variables", "u", "v", "--blend-labels", "only"], "2 labels expected"),
                          (["--blend-variables", "u", "v", "--blend-labels", "a", "a"], "the labels must differ"),
                          (["--blend-variables", "u", "hires"], "'hires' is the target"),
                          (["--blend-variables", "u", "absent"], "needs the variable 'absent'"),
                          (["--blend-variables", "u", "small"], "do not match"),
                          (["--blend-variables", "u", "day"], "do not match"),
                          (["--blend-variables", "u", "--blend-block-variable", "row"], "is not a variable of the data set with one value per case"),
                          (["--blend-variables", "u", "--blend-block-variable", "absent"], "is not a variable of the data set with one value per case"),
                          (["--blend-variables", "u", "--blend-folds", "5"], "5 folds need at least as many resampling units, there are 4"),
                          (["--blend-variables", "u", "--blend-block-variable", "day", "--blend-folds", "3"], "there are 2")):
        with pytest.raises(ValueError, match=text):
            cli.main(base + flags)
    with pytest.raises(ValueError, match="needs the variable 'absent'"):
        cli.main(["fit", "--inputs", scored, "--output-variable", "absent", "--blend-variables", "u"])
    assert not (tmp_path / "never.json").exists()
    # more than 2^20 units without a block variable: refused from the shapes alone
    from cae_tools_amd.data.arrays import DataArray, Dataset
    many = (1 << 20) + 1
    wide = np.broadcast_to(np.zeros((1, 1, 1, 1), dtype=np.float32), (many, 1, 1, 1))
    ds = Dataset({"hires": DataArray(wide, dims=("n", "c", "y", "x")), "u": DataArray(wide, dims=("n", "c", "y", "x"))})
    with pytest.raises(ValueError, match="at most 1048576 resampling units expected, the data set has 1048577 cases; name a blend_block_variable"):
        cli.check_fit_files(ds, "hires", ["u"], None, 5)


def test_apply_refuses_before_the_gpu_library_is_loaded(no_library, scored, tmp_path):
    def record(variables, weights, intercept=0.0):
        path = str(tmp_path / "w.json")
        with open(path, "w") as f:
            json.dump({"variables": variables, "weights_hex": [float(w).hex() for w in weights], "intercept_hex": float(intercept).hex()}, f)
        return path
    out = str(tmp_path / "out.nc")
    for (variables, weights, flags, text) in ((["u", "v"], [0.5, 0.5], ["--prediction-variable", "u"], "already holds a variable 'u'"),
                                              (["u", "absent"], [0.5, 0.5], [], "needs the variable 'absent'"),
                                              (["u", "two"], [0.5, 0.5], [], "differ in shape"),
                                              (["u", "small"], [0.5, 0.5], [], "differ in shape"),
                                              (["day", "u"], [0.5, 0.5], [], "differ in shape")):
        with pytest.raises(ValueError, match=text):
            cli.main(["apply", scored, out, "--blend-file", record(variables, weights)] + flags)
    with pytest.raises(ValueError, match="is not a blend file"):
        cli.main(["apply", scored, out, "--blend-file", record(["u"], [math.inf])])
    with pytest.raises(FileNotFoundError):
        cli.main(["apply", scored, out, "--blend-file", str(tmp_path / "absent.json")])
    # a candidate whose weight is 0 is not read and need not be there
    from cae_tools_amd.data.arrays import open_mfdataset
    (kept, w) = cli.check_apply_files(open_mfdataset([scored]), ["u", "absent", "v"], [0.25, 0.0, 0.75], "blend_output")
    assert kept == ["u", "v"] and w.tolist() == [0.25, 0.75]
    assert not (tmp_path / "out.nc").exists()


def test_the_wrappers_refuse_before_the_gpu(no_library):
    from cae_tools_amd.case_ops import blend_predictions, case_error_moments, moments_width
    field = np.zeros((2, 1, 3, 3))
    with pytest.raises(ValueError, match="1 to 8 predictions expected"):
        case_error_moments([], field)
    with pytest.raises(ValueError, match="1 to 8 predictions expected"):
        case_error_moments([field] * 9, field)
    with pytest.raises(ValueError, match="1 to 8 predictions expected"):
        blend_predictions([], [])
    with pytest.raises(ValueError, match="one weight per prediction"):
        blend_predictions([field, field], [1.0])
    with pytest.raises(ValueError, match="must be finite"):
        blend_predictions([field], [math.nan])
    with pytest.raises(ValueError, match="must be finite"):
        blend_predictions([field], [1.0], intercept=math.inf)
    assert [moments_width(m) for m in (1, 3, 8)] == [3, 10, 45]


# ---- the entry points' host side -------------------------------------------------------------------------------------------

def test_workspace_rule():
    size = _lib.load().cae_case_error_moments_workspace_bytes
    assert size(0, 64, 2) == 0 and size(3, 0, 2) == 0 and size(3, 64, 0) == 0 and size(3, 64, 9) == 0 and size(-1, 64, 1) == 0
    # the row of 3, 6, 10, 15 and 45 moments at an even pitch
    assert size(1, 1, 1) == 4 * 8 and size(3, 64, 2) == 3 * 6 * 8 and size(3, 65, 3) == 3 * 2 * 10 * 8 and size(2, 64, 4) == 2 * 16 * 8
    assert size(9, 4099, 8) == 9 * 65 * 46 * 8 and size(1 << 40, 1 << 30, 1) == 0


no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the refusal tables run without a GPU only: their addresses are made up")
(P0, P1, A, SUMS, WS, OUT) = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000)
MOMENTS_CALL = dict(ptrs=[P0, P1], pred_kind=2, strides=[80, 80], n_pred=2, actual=A, actual_kind=2, actual_stride=80, n_case=3, plane=70,
                    sums=SUMS, workspace=WS, workspace_bytes=1 << 20, stream=None)
MOMENTS_TABLE = [
    ("bad argument", [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(n_pred=0), dict(n_pred=9), dict(n_case=-1),
                      dict(plane=-1)]),
    ("null list of predictions", [dict(ptrs=None), dict(strides=None)]),
    ("negative stride", [dict(strides=[80, -1]), dict(actual_stride=-80)]),
    ("null pointer", [dict(ptrs=[P0, None]), dict(actual=None), dict(sums=None)]),
    ("a case stride is shorter than the plane", [dict(strides=[69, 80]), dict(strides=[80, 69]), dict(actual_stride=69)]),
    ("an operand reaches 2^60 elements from its pointer", [dict(strides=[80, 1 << 59]), dict(actual_stride=1 << 59),
                                                          dict(n_case=1 << 31, plane=1 << 30, strides=[1 << 30, 1 << 30],
                                                               actual_stride=1 << 30)]),
    ("pointers must be aligned to their element size, the workspace to 16 bytes",
     [dict(ptrs=[P0, P1 + 4]), dict(actual=A + 4), dict(actual=A + 2, actual_kind=0), dict(sums=SUMS + 4), dict(workspace=WS + 8)]),
    ("needs a workspace of 288 bytes", [dict(workspace=None), dict(workspace_bytes=287)]),
]


def _lists(args):
    n = len(args["ptrs"]) if args["ptrs"] is not None else 0
    ptrs = (C.c_void_p * n)(*args["ptrs"]) if args["ptrs"] is not None else None
    strides = (C.c_int64 * len(args["strides"]))(*args["strides"]) if args["strides"] is not None else None
    return ptrs, strides


def _moments_call(lib, args):
    (ptrs, strides) = _lists(args)
    return lib.cae_case_error_moments(ptrs, args["pred_kind"], strides, args["n_pred"], args["actual"], args["actual_kind"],
                                      args["actual_stride"], args["n_case"], args["plane"], args["sums"], args["workspace"],
                                      args["workspace_bytes"], args["stream"])


@no_gpu
@pytest.mark.parametrize("row", [(text, change) for (text, changes) in MOMENTS_TABLE for change in changes],
                         ids=lambda r: r[0][:24] + ":" + ",".join(r[1]))
def test_case_error_moments_refusal(row):
    """the call is answered by the host, with CAE_ERR_ARG and this text"""
    (text, change) = row
    lib = _lib.load()
    assert _moments_call(lib, dict(MOMENTS_CALL, **change)) == -1
    message = lib.cae_last_error().decode()
    assert message.startswith("cae_case_error_moments: ") and text in message


@no_gpu
def test_case_error_moments_empty_calls_succeed_on_the_host():
    lib = _lib.load()
    for change in (dict(n_case=0), dict(plane=0), dict(n_case=0, actual=None, sums=None, workspace=None, workspace_bytes=0)):
        assert _moments_call(lib, dict(MOMENTS_CALL, **change)) == 0


BLEND_CALL = dict(ptrs=[P0, P1], pred_kind=2, strides=[80, 80], n_pred=2, weights=[0.5, 0.5], intercept=0.0, n_case=3, case_elems=70,
                  out=OUT, out_stride=70, stream=None)
BLEND_TABLE = [
    ("bad argument", [dict(pred_kind=4), dict(pred_kind=-1), dict(n_pred=0), dict(n_pred=9), dict(n_case=-1), dict(case_elems=-1)]),
    ("null list of predictions or weights", [dict(ptrs=None), dict(strides=None), dict(weights=None)]),
    ("negative stride", [dict(strides=[80, -1]), dict(out_stride=-70)]),
    ("the weights and the intercept must be finite", [dict(weights=[0.5, math.nan]), dict(weights=[math.inf, 0.5]), dict(intercept=math.nan),
                                                     dict(intercept=-math.inf)]),
    ("null pointer", [dict(ptrs=[P0, None]), dict(ptrs=[None, P1], weights=[0.0, 1.0]), dict(out=None)]),
    ("a case stride is shorter than the case", [dict(strides=[69, 80]), dict(strides=[80, 69]), dict(out_stride=69)]),
    ("an operand reaches 2^60 elements from its pointer", [dict(strides=[80, 1 << 59]), dict(out_stride=1 << 59),
                                                          dict(n_case=1 << 31, case_elems=1 << 30, strides=[1 << 30, 1 << 30],
                                                               out_stride=1 << 30)]),
    ("pointers must be aligned to their element size", [dict(ptrs=[P0, P1 + 4]), dict(ptrs=[P0 + 2, P1], pred_kind=0), dict(out=OUT + 4)]),
]


def _blend_call(lib, args):
    (ptrs, strides) = _lists(args)
    weights = (C.c_double * len(args["weights"]))(*args["weights"]) if args["weights"] is not None else None
    return lib.cae_blend_predictions(ptrs, args["pred_kind"], strides, args["n_pred"], weights, args["intercept"], args["n_case"],
                                     args["case_elems"], args["out"], args["out_stride"], args["stream"])


@no_gpu
@pytest.mark.parametrize("row", [(text, change) for (text, changes) in BLEND_TABLE for change in changes],
                         ids=lambda r: r[0][:24] + ":" + ",".join(r[1]))
def test_blend_predictions_refusal(row):
    (text, change) = row
    lib = _lib.load()
    assert _blend_call(lib, dict(BLEND_CALL, **change)) == -1
    message = lib.cae_last_error().decode()
    assert message.startswith("cae_blend_predictions: ") and text in message


@no_gpu
def test_blend_predictions_empty_calls_succeed_on_the_host():
    lib = _lib.load()
    for change in (dict(n_case=0), dict(case_elems=0), dict(n_case=0, ptrs=[None, None], out=None)):
        assert _blend_call(lib, dict(BLEND_CALL, **change)) == 0
