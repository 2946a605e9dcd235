"""What the host side of the stateless entry points refuses, frozen: the return code and the exact cae_last_error() text of
one bad call per check of cae_case_measures, cae_pixel_sums, cae_pixel_sums_about, cae_case_range, cae_render_cases,
cae_case_spectra, cae_case_ssim, cae_case_baseline, cae_ensemble_verify and cae_scene_gather, and the calls without a case
that return CAE_OK before they look at a pointer.

The addresses are made-up integers that no call here dereferences: every row is answered by the host before a launch.  The
module is skipped where a GPU is present, so that a row that slipped past the checks ends in HIP's no-device error and never
in a launch with those addresses; on the GPU the *_gpu.py tests cover the refusals with real buffers.  The shapes are 3 cases
of 5 x 7 (plane 35); a row that needs a workspace says how it gets one (a plane above one chunk, case_chunk 1, two scales).
"""
import ctypes as C
import math

import pytest
import torch

from cae_tools_amd import _lib

if torch.cuda.is_available():
    pytest.skip("the refusal table runs without a GPU only: its addresses are made up", allow_module_level=True)

(OK, ARG) = (0, -1)
# 16-byte aligned, far apart
(P, A, L, OUT, WS, AUX, AUX2, AUX3) = (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000)
BIG = 1 << 59       # as a case stride of 3 cases: 2 * 2^59 + plane elements from the pointer, above 2^60
NAN = math.nan

GEOM = dict(Y=10, X=14, h=5, w=7, oy=1, ox=2, sy=1, sx=1)       # 3 x 3 tiles

# entry point -> (argument names in the order of include/cae_hip.h, a call that passes every check)
CALLS = {
    "cae_case_measures": (
        "pred pred_kind pred_stride actual actual_kind actual_stride n_case plane out workspace workspace_bytes stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, n_case=3, plane=35, out=OUT,
             workspace=None, workspace_bytes=0, stream=None)),
    "cae_pixel_sums": (
        "pred pred_kind pred_stride actual actual_kind actual_stride n_case plane shift case_chunk sums workspace "
        "workspace_bytes stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, n_case=3, plane=35, shift=0.0,
             case_chunk=0, sums=OUT, workspace=None, workspace_bytes=0, stream=None)),
    "cae_pixel_sums_about": (
        "pred pred_kind pred_stride actual actual_kind actual_stride n_case plane shifts case_chunk sums workspace "
        "workspace_bytes stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, n_case=3, plane=35, shifts=AUX,
             case_chunk=0, sums=OUT, workspace=None, workspace_bytes=0, stream=None)),
    "cae_case_range": (
        "src src_kind src_stride sub sub_kind sub_stride n_case plane out workspace workspace_bytes stream",
        dict(src=P, src_kind=0, src_stride=35, sub=A, sub_kind=3, sub_stride=35, n_case=3, plane=35, out=OUT, workspace=WS,
             workspace_bytes=24, stream=None)),
    "cae_render_cases": (
        "src src_kind src_stride sub sub_kind sub_stride cases n_sel n_case height width lo hi flip_y out stream",
        dict(src=P, src_kind=0, src_stride=35, sub=A, sub_kind=3, sub_stride=35, cases=AUX, n_sel=2, n_case=3, height=5,
             width=7, lo=0.0, hi=1.0, flip_y=0, out=OUT, stream=None)),
    "cae_case_spectra": (
        "pred pred_kind pred_stride actual actual_kind actual_stride n_case h w wy wx bin n_bin sums counted workspace "
        "workspace_bytes stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, n_case=3, h=5, w=7, wy=AUX, wx=AUX2,
             bin=AUX3, n_bin=4, sums=OUT, counted=L, workspace=WS, workspace_bytes=672, stream=None)),
    "cae_case_ssim": (
        "pred pred_kind pred_stride actual actual_kind actual_stride n_case h w n_scale shift scale window sums workspace "
        "workspace_bytes stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, n_case=3, h=5, w=7, n_scale=2,
             shift=0.0, scale=1.0, window=AUX, sums=OUT, workspace=WS, workspace_bytes=576, stream=None)),
    "cae_case_baseline": (
        "low low_kind low_stride h_in w_in pred pred_kind pred_stride actual actual_kind actual_stride n_case h_out w_out mode "
        "sums field workspace workspace_bytes stream",
        dict(low=L, low_kind=1, low_stride=12, h_in=3, w_in=4, pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2,
             actual_stride=35, n_case=3, h_out=5, w_out=7, mode=2, sums=OUT, field=AUX, workspace=WS, workspace_bytes=144,
             stream=None)),
    "cae_ensemble_verify": (
        "draws case_stride draw_stride actual actual_kind actual_stride n_case plane k_total vmin range case_sums rank_counts "
        "workspace workspace_bytes stream",
        dict(draws=P, case_stride=4 * 35, draw_stride=35, actual=A, actual_kind=2, actual_stride=35, n_case=3, plane=35,
             k_total=4, vmin=288.0, range=10.5, case_sums=OUT, rank_counts=AUX, workspace=WS, workspace_bytes=144, stream=None)),
    "cae_scene_gather": (
        "geom src src_kind n_t c_src t0 n_t_call ky0 n_ky dst c_dst c_off vmin range enable invalid stream",
        dict(geom=GEOM, src=P, src_kind=2, n_t=3, c_src=1, t0=0, n_t_call=3, ky0=0, n_ky=3, dst=OUT, c_dst=2, c_off=1, vmin=0.0,
             range=1.0, enable=1, invalid=AUX, stream=None)),
}

NO_CASE = dict(pred=None, actual=None, sums=None, workspace=None, workspace_bytes=0)
_PAIR_NULLS = dict(pred=None, actual=None)

# the ladder cae_pixel_sums and cae_pixel_sums_about share (pixel_sums_run names both "cae_pixel_sums")
_PIXEL_SUMS = [
    (ARG, "cae_pixel_sums: bad argument",
     [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1), dict(plane=-1),
      dict(case_chunk=-1), dict(pred=None), dict(actual=None)]),
    (OK, "", [dict(plane=0, **NO_CASE), dict(plane=0, n_case=0, **NO_CASE)]),
    (ARG, "cae_pixel_sums: sums_dev must be an 8-byte aligned pointer",
     [dict(sums=None), dict(sums=OUT + 2), dict(n_case=0, **NO_CASE)]),
    (ARG, "cae_pixel_sums: a case stride is shorter than the plane", [dict(pred_stride=34), dict(actual_stride=34)]),
    (ARG, "cae_pixel_sums: pointers must be aligned to their element size", [dict(pred=P + 2), dict(actual=A + 2)]),
    # case_chunk 1: three chunks of one case, 3 * 9 * 35 doubles of partials
    (ARG, "cae_pixel_sums: needs a workspace of 7560 bytes (cae_pixel_sums_workspace_bytes)",
     [dict(case_chunk=1), dict(case_chunk=1, workspace=WS, workspace_bytes=7559),
      dict(case_chunk=1, workspace=WS + 2, workspace_bytes=7560)]),
]

# entry point -> [(return code, cae_last_error() text, [changes to the passing call, one bad call each])]
TABLE = {
    "cae_case_measures": [
        (ARG, "cae_case_measures: bad argument",
         [dict(pred=None), dict(actual=None), dict(out=None), dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4),
          dict(actual_kind=-1), dict(n_case=0), dict(plane=0), dict(n_case=0, pred=None, actual=None, out=None)]),
        (ARG, "cae_case_measures: a case stride is shorter than the plane", [dict(pred_stride=34), dict(actual_stride=34)]),
        (ARG, "cae_case_measures: pointers must be aligned to their element size",
         [dict(pred=P + 2), dict(actual=A + 2), dict(out=OUT + 2)]),
        # a plane of two chunks: 3 * 2 * 2 doubles of partials
        (ARG, "cae_case_measures: needs a workspace of 96 bytes (cae_case_measures_workspace_bytes)",
         [dict(plane=4097, pred_stride=4097, actual_stride=4097),
          dict(plane=4097, pred_stride=4097, actual_stride=4097, workspace=WS, workspace_bytes=95),
          dict(plane=4097, pred_stride=4097, actual_stride=4097, workspace=WS + 2, workspace_bytes=96)]),
    ],
    "cae_pixel_sums": _PIXEL_SUMS + [(ARG, "cae_pixel_sums: bad argument", [dict(shift=NAN), dict(shift=math.inf)])],
    "cae_pixel_sums_about": _PIXEL_SUMS + [
        (ARG, "cae_pixel_sums_about: shifts_dev must be an 8-byte aligned pointer", [dict(shifts=None), dict(shifts=AUX + 2)]),
        (OK, "", [dict(plane=0, shifts=None, **NO_CASE)]),
        (ARG, "cae_pixel_sums: sums_dev must be an 8-byte aligned pointer", [dict(n_case=0, shifts=None, **NO_CASE)]),
    ],
    "cae_case_range": [
        (ARG, "cae_case_range: bad argument",
         [dict(out=None), dict(out=OUT + 2), dict(n_case=0), dict(plane=0), dict(src=None), dict(src_kind=4), dict(src_kind=-1),
          dict(sub_kind=4), dict(sub_kind=-1), dict(n_case=0, src=None, sub=None, out=None, workspace=None)]),
        (ARG, "cae_case_range: a case stride is shorter than the plane", [dict(src_stride=34), dict(sub_stride=34)]),
        (ARG, "cae_case_range: pointers must be aligned to their element size", [dict(src=P + 2), dict(sub=A + 2)]),
        (ARG, "cae_case_range: needs a workspace of 24 bytes (cae_case_range_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=23), dict(workspace=WS + 2)]),
    ],
    "cae_render_cases": [
        (ARG, "cae_render_cases: bad argument",
         [dict(out=None), dict(n_sel=0), dict(n_case=0), dict(height=0), dict(width=0), dict(cases=AUX + 2), dict(src=None),
          dict(src_kind=4), dict(src_kind=-1), dict(sub_kind=4), dict(sub_kind=-1),
          dict(n_case=0, src=None, sub=None, cases=None, out=None)]),
        (ARG, "cae_render_cases: image too large (height * (width + 1) must stay below 2^31)",
         [dict(height=1 << 16, width=1 << 15)]),
        (ARG, "cae_render_cases: lo, hi and hi - lo must be finite", [dict(lo=NAN), dict(hi=math.inf)]),
        (ARG, "cae_render_cases: a case stride is shorter than the plane", [dict(src_stride=34), dict(sub_stride=34)]),
        (ARG, "cae_render_cases: pointers must be aligned to their element size", [dict(src=P + 2), dict(sub=A + 2)]),
    ],
    "cae_case_spectra": [
        (ARG, "cae_case_spectra: bad argument (CAE_ELEM_* kinds, n_case >= 0, 1 <= h, w <= 2048, n_bin >= 1)",
         [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1), dict(h=0),
          dict(w=2049), dict(n_bin=0)]),
        (OK, "", [dict(n_case=0, pred=None, actual=None, wy=None, wx=None, bin=None, sums=None, counted=None, workspace=None,
                       workspace_bytes=0)]),
        (ARG, "cae_case_spectra: null pointer",
         [dict(pred=None), dict(actual=None), dict(wy=None), dict(wx=None), dict(bin=None), dict(sums=None), dict(counted=None),
          dict(workspace=None)]),
        (ARG, "cae_case_spectra: a case stride is shorter than the plane", [dict(pred_stride=34), dict(actual_stride=34)]),
        (ARG, "cae_case_spectra: an operand reaches 2^60 elements from its pointer", [dict(pred_stride=BIG), dict(actual_stride=BIG)]),
        (ARG, "cae_case_spectra: pointers must be aligned to their element size, the workspace to 16 bytes",
         [dict(pred=P + 2), dict(actual=A + 2), dict(wy=AUX + 2), dict(wx=AUX2 + 2), dict(bin=AUX3 + 2), dict(sums=OUT + 2),
          dict(counted=L + 2), dict(workspace=WS + 8)]),
        (ARG, "cae_case_spectra: needs a workspace of 672 bytes (cae_case_spectra_workspace_bytes)", [dict(workspace_bytes=671)]),
    ],
    "cae_case_ssim": [
        (ARG, "cae_case_ssim: bad argument (CAE_ELEM_* kinds, n_case >= 0, 1 <= h, w <= 16384, 1 <= n_scale <= 5)",
         [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1), dict(h=0),
          dict(w=16385), dict(n_scale=0), dict(n_scale=6)]),
        (ARG, "cae_case_ssim: shift and scale must be finite", [dict(shift=NAN), dict(scale=math.inf)]),
        (OK, "", [dict(n_case=0, pred=None, actual=None, window=None, sums=None, workspace=None, workspace_bytes=0)]),
        (ARG, "cae_case_ssim: null pointer", [dict(pred=None), dict(actual=None), dict(window=None), dict(sums=None)]),
        (ARG, "cae_case_ssim: a case stride is shorter than the plane", [dict(pred_stride=34), dict(actual_stride=34)]),
        (ARG, "cae_case_ssim: an operand reaches 2^60 elements from its pointer", [dict(pred_stride=BIG), dict(actual_stride=BIG)]),
        (ARG, "cae_case_ssim: pointers must be aligned to their element size, the workspace to 8 bytes",
         [dict(pred=P + 2), dict(actual=A + 2), dict(sums=OUT + 2), dict(workspace=WS + 2)]),
        # two scales: the pooled 3 x 4 planes of x and y for 3 cases
        (ARG, "cae_case_ssim: needs a workspace of 576 bytes (cae_case_ssim_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=575)]),
    ],
    "cae_case_baseline": [
        (ARG, "cae_case_baseline: bad argument (CAE_ELEM_* kinds, a CAE_INTERP_* mode, n_case >= 0, sides of 1 to 2^30)",
         [dict(low_kind=4), dict(low_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(pred_kind=4), dict(pred_kind=-1),
          dict(mode=-1), dict(mode=3), dict(h_in=0), dict(w_in=(1 << 30) + 1), dict(n_case=-1), dict(h_out=0)]),
        (ARG, "cae_case_baseline: negative stride", [dict(low_stride=-1), dict(actual_stride=-1), dict(pred_stride=-1)]),
        (OK, "", [dict(n_case=0, low=None, pred=None, actual=None, sums=None, field=None, workspace=None, workspace_bytes=0)]),
        (ARG, "cae_case_baseline: null pointer", [dict(low=None), dict(actual=None), dict(sums=None)]),
        (ARG, "cae_case_baseline: a case stride is shorter than the plane",
         [dict(low_stride=11), dict(actual_stride=34), dict(pred_stride=34)]),
        (ARG, "cae_case_baseline: an operand reaches 2^60 elements from its pointer",
         [dict(low_stride=BIG), dict(actual_stride=BIG), dict(pred_stride=BIG)]),
        (ARG, "cae_case_baseline: pointers must be aligned to their element size, the workspace to 8 bytes",
         [dict(low=L + 2), dict(actual=A + 2), dict(pred=P + 2), dict(sums=OUT + 2), dict(field=AUX + 2), dict(workspace=WS + 2)]),
        (ARG, "cae_case_baseline: needs a workspace of 144 bytes (cae_case_baseline_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=143)]),
    ],
    "cae_ensemble_verify": [
        (ARG, "cae_ensemble_verify: bad argument (n_case >= 0, plane >= 0, 2 <= k_total <= 64, a CAE_ELEM_* kind)",
         [dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1), dict(plane=-1), dict(k_total=1), dict(k_total=65)]),
        (ARG, "cae_ensemble_verify: negative stride", [dict(case_stride=-1), dict(draw_stride=-1), dict(actual_stride=-1)]),
        (ARG, "cae_ensemble_verify: vmin must be finite, range finite and not negative",
         [dict(vmin=NAN), dict(range=math.inf), dict(range=-1.0)]),
        (OK, "", [dict(n_case=0, draws=None, actual=None, case_sums=None, rank_counts=None, workspace=None, workspace_bytes=0),
                  dict(plane=0, draws=None, actual=None, case_sums=None, rank_counts=None, workspace=None, workspace_bytes=0)]),
        (ARG, "cae_ensemble_verify: null pointer",
         [dict(draws=None), dict(actual=None), dict(case_sums=None), dict(rank_counts=None)]),
        (ARG, "cae_ensemble_verify: an operand reaches 2^60 elements from its pointer",
         [dict(case_stride=BIG), dict(actual_stride=BIG)]),
        (ARG, "cae_ensemble_verify: the strides make planes overlap", [dict(draw_stride=34), dict(case_stride=4 * 35 - 1)]),
        (ARG, "cae_ensemble_verify: the target's case stride is shorter than the plane", [dict(actual_stride=34)]),
        (ARG, "cae_ensemble_verify: pointers must be aligned to their element size",
         [dict(draws=P + 2), dict(actual=A + 2), dict(case_sums=OUT + 2), dict(rank_counts=AUX + 2)]),
        # one chunk a case: 3 blocks of 4 + 2 rank bins
        (ARG, "cae_ensemble_verify: needs a workspace of 144 bytes (cae_ensemble_verify_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=143), dict(workspace=WS + 2)]),
    ],
    "cae_scene_gather": [
        (ARG, "cae_scene_gather: null geometry", [dict(geom=None)]),
        (ARG, "cae_scene_gather: a scene of 4 x 14 pixels does not hold a box of 5 x 7 (sides up to 2^30)", [dict(geom=dict(GEOM, Y=4))]),
        (ARG, "cae_scene_gather: the overlap (5, 2) must be at least 0 and below the box (5, 7)", [dict(geom=dict(GEOM, oy=5))]),
        (ARG, "cae_scene_gather: bad argument (a CAE_ELEM_* kind, the time range inside the variable, the channels inside the batch)",
         [dict(src_kind=4), dict(src_kind=-1), dict(n_t=-1), dict(c_src=0), dict(c_off=2), dict(t0=1), dict(n_t_call=-1),
          dict(ky0=-1), dict(n_ky=-1)]),
        (ARG, "cae_scene_gather: tile rows 1 .. 4 of 3", [dict(ky0=1)]),
        (OK, "", [dict(n_t_call=0, src=None, dst=None, invalid=None), dict(n_ky=0, src=None, dst=None, invalid=None)]),
        (ARG, "cae_scene_gather: null pointer", [dict(src=None), dict(dst=None), dict(invalid=None)]),
        (ARG, "cae_scene_gather: pointers must be aligned to their element size",
         [dict(src=P + 2), dict(dst=OUT + 2), dict(invalid=AUX + 2)]),
    ],
}

ROWS = [(fn, rc, text, change) for (fn, groups) in TABLE.items() for (rc, text, changes) in groups for change in changes]


def _row_id(row):
    (fn, _, _, change) = row
    return fn[4:] + "-" + ",".join(f"{k}={sorted(set(v.items()) - set(GEOM.items())) if isinstance(v, dict) else v}" for (k, v) in change.items())


def test_the_table_names_all_ten_entry_points():
    assert sorted(TABLE) == sorted(CALLS) and len(CALLS) == 10
    assert len(set(map(_row_id, ROWS))) == len(ROWS)


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_refusal(row):
    """the call is answered by the host, with this code and this text"""
    (fn, rc, text, change) = row
    lib = _lib.load()
    (names, base) = CALLS[fn]
    args = dict(base, **change)
    assert set(change) <= set(base) and names.split() == list(base)
    geom = None
    if isinstance(args.get("geom"), dict):
        geom = _lib.SceneGeomC(**args["geom"])
        args["geom"] = C.byref(geom)
    got = getattr(lib, fn)(*(args[n] for n in names.split()))
    message = lib.cae_last_error().decode() if got != OK else ""
    print(f"{_row_id(row)}: {got} {message!r}")
    assert (got, message) == (rc, text)
