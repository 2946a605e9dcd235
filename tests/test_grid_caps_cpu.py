"""test_grid_caps_gpu.py's table of grid caps against the host code, without a GPU.  csrc/host_*.h and stateless_host.h are
read as text: every ceil_capped(items, per, cap) call site and the caps that have a name of their own (JH_MAX_GROUPS,
ST_MAX_GROUPS, EV_MAX_BLOCKS, quantile_pool_groups, the 2^20 tile caps) must be known here by the kernel they size, and each
kernel is either in the GPU module's CAPS with the same per and cap or in NOT_DRIVEN with the reason.  A new capped launch, or
a changed cap, fails here instead of leaving a loop untested.  Then every shape of the GPU module's SHAPES really exceeds per *
cap, its boundary partner is the last call that does not, and the workgroup counts the library gives away through its
workspace sizes are the ones the GPU tests assert."""
import glob
import os
import re

import pytest

import test_grid_caps_gpu as gpu
from cae_tools_amd import _lib

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cae_tools_amd", "csrc")

# (file, items as written, per as written) of every ceil_capped call: the kernel it sizes; two kernels where the cap is
# `condition ? a : b`, the one of the true branch first
SITES = {
    ("host_loader.h", "n", "256 * 16"): "k_scan",
    ("host_loader.h", "total", "256 * 8"): "k_normalise_pack",
    ("host_loader.h", "n", "256 * 8"): "k_denorm_f64",
    ("host_loader.h", "inst_elems", "256 * 16"): "k_metric_sums",
    ("host_loader.h", "n / 4", "256"): "k_bswap32",
    ("host_case_measures.h", "items", "CM_WAVES"): "k_case_measures",
    ("host_case_measures.h", "n_case", "256"): "k_case_fold",
    ("host_ensemble.h", "a.items", "CM_WAVES"): "k_ensemble_moments",
    ("host_ensemble.h", "n_case * EV_SUMS", "256"): "k_verify_fold",
    ("host_case_pages.h", "n_case * case_chunks(plane)", "CM_WAVES"): "k_case_range",
    ("host_case_pages.h", "items", "CM_WAVES"): "k_render_cases",
    ("host_pixel_sums.h", "n", "256"): "k_pixel_fold",
    ("host_spectra.h", "n_case * n_bin * 4", "256"): "k_spectra_fold",
    ("host_ssim.h", "n_case * per", "256"): "k_ssim_pool",
    ("host_ssim.h", "n_case * n_scale * 3", "256"): "k_ssim_fold",
    ("host_baseline.h", "n_case * BL_SUMS", "256"): "k_baseline_fold",
    ("host_scene.h", "a.total", "256 * 4"): "k_scene_gather",
    ("host_hist.h", "n_case * case_chunks(plane)", "JH_WAVES"): "k_joint_hist",
    ("host_strata.h", "(int64_t)items", "ST_WAVES"): "k_strata_sums",
    ("host_fss.h", "b.words", "FS_WAVES * FS_AHEAD"): "k_fss_bits",
    ("host_fss.h", "g.items", "FS_WAVES"): "k_fss_windows",
    ("host_importance.h", "total", "256 * 8"): "k_normalise_pack_gather",
    ("host_importance.h", "a.items", "IM_WAVES"): ("k_case_importance map", "k_case_importance"),
    ("host_importance.h", "n_case", "IM_WAVES"): "k_importance_fold",
    ("host_quantile.h", "(total + 63) / 64", "4 * QT_AHEAD"): ("k_quantile_pool_count", "k_score_counts_pool"),      # one function, two launches
    ("host_quantile.h", "groups * n_level", "256"): "k_quantile_fill",
    ("host_quantile.h", "b.total", "256 * 4"): "k_interval_bounds",
    ("host_neighbours.h", "n_query", "4"): "k_nb_valid",
    ("host_neighbours.h", "n_ref", "4"): "k_nb_valid",
    ("host_compare.h", "a.items", "CP_WAVES"): "k_case_compare",
    ("host_compare.h", "n_case", "CP_WAVES"): "k_compare_fold",
    ("host_compare.h", "a.items", "BS_THREADS"): ("k_bootstrap_sums staged", "k_bootstrap_sums unstaged"),
}

# the capped launches test_grid_caps_gpu.py does not drive, and why
NOT_DRIVEN = {
    "k_scan": "held past its cap by test_loader_kernels_gpu.py",
    "k_normalise_pack": "held past its cap by test_loader_kernels_gpu.py",
    "k_denorm_f64": "held past its cap by test_loader_kernels_gpu.py",
    "k_metric_sums": "held past its cap by test_loader_kernels_gpu.py",
    "k_bswap32": "held past its cap by test_loader_kernels_gpu.py",
    "k_case_measures": "held past its cap by test_evaluator_gpu.py, 70 000 cases",
    "k_case_range": "held past its cap by test_case_pages_gpu.py, 70 000 cases",
    "k_case_fold": "out of reach: more than 4096 x 256 cases of more than one chunk, over 4 x 10^9 pixels",
    "k_verify_fold": "out of reach: more than one chunk a case past EV_MAX_BLOCKS takes over 33 million pixels times K",
    "k_spectra_fold": "not driven: more than 524 288 (case, bin) pairs of a transform each",
    "k_ssim_pool": "out of reach: more than 65536 x 256 pooled pixels a scale",
    "k_ssim_fold": "out of reach: more than 349 525 cases of 11 x 11 pixels at the least",
    "k_fss_bits": "out of reach: more than 4096 x 16 x 64 x 64 thresholded pixels",
    "k_fss_windows": "out of reach: 2^20 workgroups",
    "k_case_importance map": "out of reach: 2^20 tiles, a plane of 2^26 pixels",
    "k_quantile_pixel": "out of reach: 2^20 tiles, a plane of 2^26 pixels",
    "k_score_counts_pixel": "out of reach: 2^20 tiles, a plane of 2^26 pixels",
    "k_bootstrap_sums unstaged": "out of reach: 4 million resamples of a table of 5200 units",
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constants():
    """every `constexpr <integer type> NAME = expression;` of csrc/*.h, as text"""
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h"))):
        with open(path) as f:
            for m in re.finditer(r"constexpr\s+(?:int|int64_t|long long|unsigned|size_t)\s+(\w+)\s*=\s*([^;]+);", f.read()):
                found[m.group(1)] = m.group(2)
    return found


CONSTANTS = _constants()


def _value(expr):
    """a C integer expression over literals and the constants above"""
    expr = re.sub(r"\((?:int64_t|long long|int|size_t)\)", "", expr)
    expr = re.sub(r"\b(\d+)(?:ull|ll|u|l)\b", r"\1", expr, flags=re.IGNORECASE)
    expr = re.sub(r"\b[A-Za-z_]\w*\b", lambda m: str(_value(CONSTANTS[m.group(0)])), expr)
    assert re.fullmatch(r"[\d\s()*+\-<]+", expr), expr
    return int(eval(expr, {"__builtins__": {}}))       # digits, brackets, * + - and << alone


def _call_sites():
    """(file, [items, per, cap] as written) of every ceil_capped call in the host files, the definition left out"""
    sites = []
    for name in sorted(os.listdir(CSRC)):
        if not (re.fullmatch(r"host_\w+\.h", name) or name == "stateless_host.h"):
            continue
        text = _read(name)
        for m in re.finditer(r"\bceil_capped\(", text):
            (depth, i, args, start) = (1, m.end(), [], m.end())
            while depth:
                c = text[i]
                depth += (c == "(") - (c == ")")
                if (c == "," and depth == 1) or depth == 0:
                    args.append(" ".join(text[start:i].split()))
                    start = i + 1
                i += 1
            if args[0].startswith("int64_t "):
                continue                    # the definition
            assert len(args) == 3, (name, args)
            sites.append((name, args))
    return sites


def _caps_of(cap):
    """the values of a cap as written: one, or (true branch, false branch) of `condition ? a : b`"""
    m = re.fullmatch(r"\w+ \? (.+) : (.+)", cap)
    return (_value(m.group(1)), _value(m.group(2))) if m else (_value(cap),)


def test_every_capped_launch_is_in_a_table():
    sites = _call_sites()
    assert len(sites) >= 30
    seen = {}
    for (name, (items, per, cap)) in sites:
        key = (name, items, per)
        assert key in SITES, f"a ceil_capped call this test does not know: {name}: ceil_capped({items}, {per}, {cap})"
        kernels = SITES[key]
        caps = _caps_of(cap)
        if isinstance(kernels, str):
            kernels = (kernels,) * len(caps)
        elif len(caps) == 1:
            caps = caps * len(kernels)
        assert len(kernels) == len(caps), (key, cap)
        for (kernel, value) in zip(kernels, caps):
            assert seen.setdefault(kernel, (_value(per), value)) == (_value(per), value), kernel
    assert set(SITES) == {(name, a[0], a[1]) for (name, a) in sites}, "a call site listed here is gone"
    # the caps that do not go through ceil_capped
    assert re.search(r"return items < EV_MAX_BLOCKS \? items : EV_MAX_BLOCKS;", _read("host_ensemble.h"))
    seen["k_ensemble_verify"] = (1, _value("EV_MAX_BLOCKS"))
    quantile = _read("host_quantile.h")
    assert quantile.count("quantile_pool_groups(g.total)") == 2 and quantile.count("g.n_tile < ((int64_t)1 << 20)") == 2
    seen["k_quantile_pixel"] = seen["k_score_counts_pixel"] = (1, 1 << 20)
    assert seen["k_joint_hist"][1] == _value("JH_MAX_GROUPS") and seen["k_strata_sums"][1] == _value("ST_MAX_GROUPS")
    assert "ST_WAVES * ST_MAX_GROUPS ? ST_MAX_GROUPS" in _read("host_strata.h")
    assert seen["k_case_importance map"][1] == seen["k_fss_windows"][1] == 1 << 20
    for (kernel, per_cap) in seen.items():
        if kernel in gpu.CAPS:
            assert kernel not in NOT_DRIVEN and gpu.CAPS[kernel] == per_cap, (kernel, gpu.CAPS[kernel], per_cap)
        else:
            assert NOT_DRIVEN.get(kernel), f"{kernel} is capped at {per_cap} and neither driven past it nor listed with a reason"
    assert set(gpu.CAPS) <= set(seen) and set(NOT_DRIVEN) <= set(seen)


@pytest.mark.parametrize("kernel", sorted(gpu.CAPS))
def test_every_shape_is_in_the_regime_it_claims(kernel):
    assert set(gpu.SHAPES) == set(gpu.CAPS) == set(gpu.ITEMS)
    (per, cap) = gpu.CAPS[kernel]
    (past, boundary) = gpu.SHAPES[kernel]
    assert past and boundary
    for shape in past:
        assert gpu.ITEMS[kernel](*shape) > per * cap and gpu.trips(kernel, shape) >= 2, shape
    for shape in boundary:
        items = gpu.ITEMS[kernel](*shape)
        assert per * cap - items < 16 and gpu.trips(kernel, shape) == 1, shape      # the last call under the cap


def test_workgroup_counts_from_the_workspace_sizes():
    """the library loads without a GPU: the three size functions give the workgroups of the shapes of points 1 and 2"""
    lib = _lib.load()
    for (n, plane) in gpu.SHAPES["k_joint_hist"][1] + gpu.SHAPES["k_joint_hist"][0]:
        items = gpu.ITEMS["k_joint_hist"](n, plane)
        assert int(lib.cae_joint_hist_workspace_bytes(n, plane, 128, 8)) // (2 * 128 * 4 * 8) == 1024 == min(-(-items // 4), 1024)
        assert int(lib.cae_strata_sums_workspace_bytes(n, 1, plane, 7)) // (7 * 8 * 8) == 1024
        assert -(-items // 4096) == gpu.trips("k_joint_hist", (n, plane)) == gpu.trips("k_strata_sums", (n, plane))
    assert [gpu.trips("k_joint_hist", s) for s in gpu.SHAPES["k_joint_hist"][0]] == [2, 3, 2]
    assert int(lib.cae_joint_hist_workspace_bytes(4092, 5, 128, 8)) // (2 * 128 * 4 * 8) == 1023
    for (n, plane, k) in gpu.VERIFY_SHAPES:
        assert gpu._ensemble_chunks(n, plane) == 1
        assert int(lib.cae_ensemble_verify_workspace_bytes(n, plane, k)) // ((k + 2) * 8) == min(n, 8192)
    # the restatement of ensemble_chunks against the library where a case has more than one chunk: 3 cases of 360 007 pixels
    # are 704 chunks a case (test_ensemble_verify_gpu.py), whose partials the workspace holds ahead of the rank counts
    assert gpu._ensemble_chunks(3, 360007) == 704
    assert int(lib.cae_ensemble_verify_workspace_bytes(3, 360007, 3)) == 3 * 704 * 5 * 8 + 2112 * 5 * 8
