"""What the host side of the stateless entry points refuses, frozen: the return code and the exact cae_last_error() text of
one bad call per check of cae_case_measures, cae_pixel_sums, cae_pixel_sums_about, cae_case_range, cae_render_cases,
cae_case_spectra, cae_case_ssim, cae_case_baseline, cae_ensemble_verify, cae_scene_gather, cae_ensemble_moments,
cae_scene_blend, cae_joint_hist, cae_strata_sums, cae_case_fss, cae_normalise_pack_gather, cae_case_importance,
cae_score_quantiles, cae_score_counts, cae_interval_bounds and cae_case_neighbours, and the calls without a case that return
CAE_OK before they look at a pointer.

The addresses are made-up integers that no call here dereferences: every row is answered by the host before a launch.  The
module is skipped where a GPU is present, so that a row that slipped past the checks ends in HIP's no-device error and never
in a launch with those addresses; on the GPU the *_gpu.py tests cover the refusals with real buffers.  The shapes are 3 cases
of 5 x 7 (plane 35); a row that needs a workspace says how it gets one (a plane above one chunk, case_chunk 1, two scales).
The arrays the library reads on the host (HOST_ARRAYS) stand in the table as tuples and reach the call as ctypes arrays.  The
empty calls that zero or fill outputs on the device (cae_joint_hist, cae_strata_sums, cae_case_fss, cae_score_quantiles and
cae_score_counts without a case or a pixel) are not here: they make HIP calls, and the *_gpu.py tests cover them.
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
    "cae_ensemble_moments": (
        "draws case_stride draw_stride n_case plane k_call k_done k_total vmin range mean std workspace workspace_bytes stream",
        dict(draws=P, case_stride=4 * 35, draw_stride=35, n_case=3, plane=35, k_call=4, k_done=0, k_total=4, vmin=288.0,
             range=10.5, mean=OUT, std=AUX, workspace=None, workspace_bytes=0, stream=None)),
    "cae_scene_blend": (
        "geom pred invalid k0 n_k carry_pred carry_invalid carry_k0 carry_n_k n_t_call c_out row0 row1 vmin range out "
        "out_t_stride nan_pixels stream",
        dict(geom=GEOM, pred=P, invalid=AUX, k0=0, n_k=3, carry_pred=None, carry_invalid=None, carry_k0=0, carry_n_k=0,
             n_t_call=2, c_out=1, row0=0, row1=10, vmin=0.0, range=1.0, out=OUT, out_t_stride=140, nan_pixels=AUX2, stream=None)),
    "cae_joint_hist": (
        "pred pred_kind pred_stride actual actual_kind actual_stride n_case plane lo hi n_bin sub joint marg cond outside "
        "workspace workspace_bytes stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, n_case=3, plane=35, lo=0.0, hi=1.0,
             n_bin=4, sub=2, joint=OUT, marg=AUX, cond=AUX2, outside=AUX3, workspace=WS, workspace_bytes=256, stream=None)),
    "cae_strata_sums": (
        "pred pred_kind pred_stride actual actual_kind actual_stride strata strata_kind strata_stride n_case h w sh sw edges "
        "n_edge shift_a shift_p counts sums workspace workspace_bytes stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, strata=L, strata_kind=1,
             strata_stride=12, n_case=3, h=5, w=7, sh=3, sw=4, edges=(0.5, 1.5), n_edge=2, shift_a=(0.0, 0.0, 0.0),
             shift_p=(0.0, 0.0, 0.0), counts=OUT, sums=AUX, workspace=WS, workspace_bytes=192, stream=None)),
    "cae_case_fss": (
        "pred pred_kind pred_stride actual actual_kind actual_stride n_case h w thresholds sides n_thr widths n_width gap_rule "
        "sums workspace workspace_bytes stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, n_case=3, h=5, w=7,
             thresholds=(0.5, 1.0), sides=(0, 1), n_thr=2, widths=(1, 3), n_width=2, gap_rule=0, sums=OUT, workspace=WS,
             workspace_bytes=600, stream=None)),
    "cae_normalise_pack_gather": (
        "src n_src c_src hw dst n_dst c_dst c_off vmin range enable row stream",
        dict(src=P, n_src=3, c_src=1, hw=35, dst=OUT, n_dst=4, c_dst=2, c_off=1, vmin=0.0, range=1.0, enable=1, row=AUX,
             stream=None)),
    "cae_case_importance": (
        "base base_stride pert pert_stride actual actual_kind actual_stride n_case plane vmin range sums map workspace "
        "workspace_bytes stream",
        dict(base=P, base_stride=35, pert=L, pert_stride=35, actual=A, actual_kind=2, actual_stride=35, n_case=3, plane=35,
             vmin=288.0, range=10.5, sums=OUT, map=AUX, workspace=WS, workspace_bytes=192, stream=None)),
    "cae_score_quantiles": (
        "pred pred_kind pred_stride actual actual_kind actual_stride scale scale_kind scale_stride n_case plane group num den "
        "n_level q n workspace workspace_bytes stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, scale=L, scale_kind=1,
             scale_stride=35, n_case=3, plane=35, group=1, num=(1, 9), den=(2, 10), n_level=2, q=OUT, n=AUX, workspace=WS,
             workspace_bytes=16640, stream=None)),
    "cae_score_counts": (
        "pred pred_kind pred_stride actual actual_kind actual_stride scale scale_kind scale_stride n_case plane group q n_level "
        "count n stream",
        dict(pred=P, pred_kind=0, pred_stride=35, actual=A, actual_kind=2, actual_stride=35, scale=L, scale_kind=1,
             scale_stride=35, n_case=3, plane=35, group=1, q=OUT, n_level=2, count=AUX, n=AUX2, stream=None)),
    "cae_interval_bounds": (
        "pred pred_kind pred_stride scale scale_kind scale_stride n_case plane q group lower upper stream",
        dict(pred=P, pred_kind=0, pred_stride=35, scale=L, scale_kind=3, scale_stride=35, n_case=3, plane=35, q=AUX, group=0,
             lower=OUT, upper=AUX2, stream=None)),
    "cae_case_neighbours": (
        "query n_query query_stride ref n_ref ref_stride dim k ref_base self_offset merge dist2 index count workspace "
        "workspace_bytes stream",
        dict(query=P, n_query=3, query_stride=35, ref=A, n_ref=5, ref_stride=35, dim=35, k=2, ref_base=0, self_offset=-1,
             merge=0, dist2=OUT, index=AUX, count=AUX2, workspace=WS, workspace_bytes=104, stream=None)),
}

# the arrays the library reads on the host: a tuple in the table, an array of this type in the call
HOST_ARRAYS = dict(edges=C.c_double, shift_a=C.c_double, shift_p=C.c_double, thresholds=C.c_double, sides=C.c_int,
                   widths=C.c_int, num=C.c_int64, den=C.c_int64)

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
    "cae_ensemble_moments": [
        (ARG, "cae_ensemble_moments: bad argument (k_total >= 2, 1 <= k_call, k_done + k_call <= k_total)",
         [dict(draws=None), dict(mean=None), dict(n_case=0), dict(plane=0), dict(k_total=1), dict(k_call=0), dict(k_done=-1),
          dict(k_done=1)]),
        (ARG, "cae_ensemble_moments: negative stride", [dict(case_stride=-1), dict(draw_stride=-1)]),
        (ARG, "cae_ensemble_moments: the strides make planes overlap", [dict(draw_stride=34), dict(case_stride=4 * 35 - 1)]),
        (ARG, "cae_ensemble_moments: pointers must be aligned to their element size",
         [dict(draws=P + 2), dict(mean=OUT + 2), dict(std=AUX + 2)]),
        # two of four draws in a call: the running sums of 3 * 35 pixels, two doubles and a float each
        (ARG, "cae_ensemble_moments: draws delivered over several calls need a workspace of 2100 bytes "
              "(cae_ensemble_moments_workspace_bytes)",
         [dict(k_call=2), dict(k_call=2, k_done=2), dict(k_call=2, workspace=WS, workspace_bytes=2099),
          dict(k_call=2, workspace=WS + 2, workspace_bytes=2100)]),
        # 2^48 groups of 4 pixels in chunks of 1024
        (ARG, "cae_ensemble_moments: plane too large", [dict(n_case=1, plane=1 << 50, draw_stride=1 << 50, case_stride=1 << 52)]),
    ],
    "cae_scene_blend": [
        (ARG, "cae_scene_blend: null geometry", [dict(geom=None)]),
        (ARG, "cae_scene_blend: a scene of 4 x 14 pixels does not hold a box of 5 x 7 (sides up to 2^30)", [dict(geom=dict(GEOM, Y=4))]),
        (ARG, "cae_scene_blend: the overlap (5, 2) must be at least 0 and below the box (5, 7)", [dict(geom=dict(GEOM, oy=5))]),
        (ARG, "cae_scene_blend: the scale (0, 1) must be at least 1", [dict(geom=dict(GEOM, sy=0))]),
        (ARG, "cae_scene_blend: 4 H W must stay below 2^29 (the weights times an fp32 value are then exact in fp64)",
         [dict(geom=dict(GEOM, sy=1 << 12, sx=1 << 12))]),
        (ARG, "cae_scene_blend: an output of 2147483648 x 14 pixels (sides up to 2^30)", [dict(geom=dict(GEOM, Y=1 << 30, sy=2))]),
        (ARG, "cae_scene_blend: bad argument (tile rows inside the scene's 3, output rows inside its 10, a time stride of at least "
              "a scene)",
         [dict(n_t_call=-1), dict(c_out=0), dict(k0=-1), dict(n_k=-1), dict(k0=1), dict(carry_n_k=-1), dict(carry_k0=-1),
          dict(carry_k0=4), dict(row0=-1), dict(row1=11), dict(row0=5, row1=4), dict(out_t_stride=-1), dict(out_t_stride=139)]),
        (ARG, "cae_scene_blend: the carried tile rows must come before the new ones", [dict(carry_n_k=1)]),
        (OK, "", [dict(n_t_call=0, pred=None, invalid=None, out=None, nan_pixels=None),
                  dict(row0=4, row1=4, pred=None, invalid=None, out=None, nan_pixels=None)]),
        (ARG, "cae_scene_blend: more than 65535 (time step, channel) planes in a call", [dict(c_out=32768, out_t_stride=32768 * 140)]),
        (ARG, "cae_scene_blend: null pointer",
         [dict(pred=None), dict(invalid=None), dict(out=None), dict(nan_pixels=None),
          dict(k0=1, n_k=2, carry_n_k=1, carry_invalid=AUX3), dict(k0=1, n_k=2, carry_n_k=1, carry_pred=L)]),
        (ARG, "cae_scene_blend: pointers must be aligned to their element size",
         [dict(pred=P + 2), dict(invalid=AUX + 2), dict(carry_pred=L + 2), dict(carry_invalid=AUX3 + 2), dict(out=OUT + 2),
          dict(nan_pixels=AUX2 + 2)]),
        # boxes of 2 x 2 that overlap by 1: the tiles of two time steps hold 2^61 values, the two scenes 2^59
        (ARG, "cae_scene_blend: an operand reaches 2^60 elements from its pointer",
         [dict(geom=dict(GEOM, Y=1 << 29, X=1 << 29, h=2, w=2, oy=1, ox=1), n_k=(1 << 29) - 1, out_t_stride=1 << 58),
          dict(out_t_stride=1 << 60)]),
        (ARG, "cae_scene_blend: output rows 0 .. 10 need tile row 0, which the call does not bring", [dict(k0=1, n_k=2)]),
    ],
    "cae_joint_hist": [
        (ARG, "cae_joint_hist: bad argument (CAE_ELEM_* kinds, n_case >= 0, plane >= 0, 1 <= n_bin <= 128, 1 <= sub <= 32, "
              "n_case * plane < 2^40)",
         [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1), dict(plane=-1),
          dict(n_bin=0), dict(n_bin=129), dict(sub=0), dict(sub=33), dict(n_case=1 << 20, plane=1 << 20)]),
        (ARG, "cae_joint_hist: lo and hi must be finite, hi > lo, and n_bin * sub / (hi - lo) finite and not zero",
         [dict(lo=NAN), dict(hi=math.inf), dict(hi=0.0), dict(hi=5e-324), dict(lo=-1e308, hi=1e308)]),
        (ARG, "cae_joint_hist: negative stride", [dict(pred_stride=-1), dict(actual_stride=-1)]),
        (ARG, "cae_joint_hist: the outputs must be 8-byte aligned",
         [dict(joint=OUT + 2), dict(marg=AUX + 2), dict(cond=AUX2 + 2), dict(outside=AUX3 + 2)]),
        (ARG, "cae_joint_hist: null pointer",
         [dict(pred=None), dict(actual=None), dict(joint=None), dict(marg=None), dict(cond=None), dict(outside=None)]),
        (ARG, "cae_joint_hist: a case stride is shorter than the plane", [dict(pred_stride=34), dict(actual_stride=34)]),
        (ARG, "cae_joint_hist: an operand reaches 2^60 elements from its pointer", [dict(pred_stride=BIG), dict(actual_stride=BIG)]),
        (ARG, "cae_joint_hist: pointers must be aligned to their element size", [dict(pred=P + 2), dict(actual=A + 2)]),
        # one workgroup: the conditional sums of 2 * 4 bins, 4 doubles each
        (ARG, "cae_joint_hist: needs a workspace of 256 bytes (cae_joint_hist_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=255), dict(workspace=WS + 2)]),
    ],
    "cae_strata_sums": [
        (ARG, "cae_strata_sums: bad argument (CAE_ELEM_* kinds, n_case >= 0, target sides of 0 to 2^30, stratifier sides of 1 to "
              "2^30, 0 <= n_edge <= 63)",
         [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(strata_kind=4),
          dict(strata_kind=-1), dict(n_edge=-1), dict(n_edge=64), dict(n_case=-1), dict(h=-1), dict(w=(1 << 30) + 1), dict(sh=0),
          dict(sw=(1 << 30) + 1)]),
        (ARG, "cae_strata_sums: negative stride", [dict(pred_stride=-1), dict(actual_stride=-1), dict(strata_stride=-1)]),
        (ARG, "cae_strata_sums: the outputs must be 8-byte aligned", [dict(counts=OUT + 2), dict(sums=AUX + 2)]),
        (ARG, "cae_strata_sums: null pointer",
         [dict(pred=None), dict(actual=None), dict(strata=None), dict(counts=None), dict(sums=None), dict(edges=None),
          dict(shift_a=None), dict(shift_p=None)]),
        (ARG, "cae_strata_sums: the edges must be finite and strictly ascending",
         [dict(edges=(1.5, 0.5)), dict(edges=(0.5, 0.5)), dict(edges=(NAN, 1.5)), dict(edges=(0.5, math.inf))]),
        (ARG, "cae_strata_sums: the shifts must be finite", [dict(shift_a=(0.0, NAN, 0.0)), dict(shift_p=(0.0, 0.0, math.inf))]),
        (ARG, "cae_strata_sums: a case stride is shorter than the plane",
         [dict(pred_stride=34), dict(actual_stride=34), dict(strata_stride=11)]),
        (ARG, "cae_strata_sums: an operand reaches 2^60 elements from its pointer",
         [dict(pred_stride=BIG), dict(actual_stride=BIG), dict(strata_stride=BIG)]),
        (ARG, "cae_strata_sums: pointers must be aligned to their element size", [dict(pred=P + 2), dict(actual=A + 2), dict(strata=L + 2)]),
        # one workgroup: 3 strata of 8 sums
        (ARG, "cae_strata_sums: needs a workspace of 192 bytes (cae_strata_sums_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=191), dict(workspace=WS + 2)]),
    ],
    "cae_case_fss": [
        (ARG, "cae_case_fss: bad argument (CAE_ELEM_* kinds, 0 <= n_case <= 2^40, sides of 0 to 16384, 1 <= n_thr <= 8, "
              "1 <= n_width <= 8, gap_rule 0 or 1)",
         [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1),
          dict(n_case=(1 << 40) + 1), dict(h=-1), dict(w=16385), dict(n_thr=0), dict(n_thr=9), dict(n_width=0), dict(n_width=9),
          dict(gap_rule=2), dict(gap_rule=-1)]),
        (ARG, "cae_case_fss: negative stride", [dict(pred_stride=-1), dict(actual_stride=-1)]),
        (ARG, "cae_case_fss: the output must be 8-byte aligned", [dict(sums=OUT + 2)]),
        (ARG, "cae_case_fss: null pointer",
         [dict(pred=None), dict(actual=None), dict(thresholds=None), dict(sides=None), dict(widths=None), dict(sums=None)]),
        (ARG, "cae_case_fss: the thresholds must be finite", [dict(thresholds=(NAN, 1.0)), dict(thresholds=(0.5, math.inf))]),
        (ARG, "cae_case_fss: a side must be 0 (above) or 1 (below)", [dict(sides=(0, 2)), dict(sides=(-1, 1))]),
        (ARG, "cae_case_fss: the widths must be odd, from 1 to 129 and strictly ascending",
         [dict(widths=(2, 3)), dict(widths=(-1, 3)), dict(widths=(1, 131)), dict(widths=(3, 1)), dict(widths=(3, 3))]),
        (ARG, "cae_case_fss: a case stride is shorter than the plane", [dict(pred_stride=34), dict(actual_stride=34)]),
        (ARG, "cae_case_fss: an operand reaches 2^60 elements from its pointer", [dict(pred_stride=BIG), dict(actual_stride=BIG)]),
        (ARG, "cae_case_fss: pointers must be aligned to their element size", [dict(pred=P + 2), dict(actual=A + 2)]),
        # the validity plane and two planes per threshold: 3 cases of 5 rows of one 64-bit word
        (ARG, "cae_case_fss: needs a workspace of 600 bytes (cae_case_fss_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=599), dict(workspace=WS + 2)]),
    ],
    "cae_normalise_pack_gather": [
        (ARG, "cae_normalise_pack_gather: bad argument (n_src >= 0, n_dst >= 0, c_src >= 1, hw >= 0, 0 <= c_off <= c_dst - c_src)",
         [dict(n_src=-1), dict(n_dst=-1), dict(c_src=0), dict(hw=-1), dict(c_off=-1), dict(c_off=2)]),
        (ARG, "cae_normalise_pack_gather: more than 2^31 - 1 rows", [dict(n_src=1 << 31), dict(n_dst=1 << 31)]),
        (OK, "", [dict(n_dst=0, src=None, dst=None, row=None), dict(hw=0, src=None, dst=None, row=None)]),
        (ARG, "cae_normalise_pack_gather: null pointer", [dict(src=None), dict(dst=None), dict(row=None)]),
        (ARG, "cae_normalise_pack_gather: an operand reaches 2^60 elements from its pointer",
         [dict(n_src=(1 << 31) - 1, hw=1 << 30), dict(n_dst=(1 << 31) - 1, hw=1 << 30)]),
        (ARG, "cae_normalise_pack_gather: pointers must be 4-byte aligned", [dict(src=P + 2), dict(dst=OUT + 2), dict(row=AUX + 2)]),
    ],
    "cae_case_importance": [
        (ARG, "cae_case_importance: bad argument (a CAE_ELEM_* kind, n_case >= 0, plane >= 0)",
         [dict(actual_kind=4), dict(actual_kind=-1), dict(n_case=-1), dict(plane=-1)]),
        (ARG, "cae_case_importance: negative stride", [dict(base_stride=-1), dict(pert_stride=-1), dict(actual_stride=-1)]),
        (ARG, "cae_case_importance: vmin and range must be finite", [dict(vmin=NAN), dict(range=math.inf)]),
        (OK, "", [dict(n_case=0, base=None, pert=None, actual=None, sums=None, map=None, workspace=None, workspace_bytes=0),
                  dict(plane=0, base=None, pert=None, actual=None, sums=None, map=None, workspace=None, workspace_bytes=0)]),
        (ARG, "cae_case_importance: null pointer", [dict(base=None), dict(pert=None), dict(actual=None), dict(sums=None)]),
        (ARG, "cae_case_importance: a case stride is shorter than the plane",
         [dict(base_stride=34), dict(pert_stride=34), dict(actual_stride=34)]),
        (ARG, "cae_case_importance: an operand reaches 2^60 elements from its pointer",
         [dict(base_stride=BIG), dict(pert_stride=BIG), dict(actual_stride=BIG)]),
        (ARG, "cae_case_importance: pointers must be aligned to their element size, the workspace to 16 bytes",
         [dict(base=P + 2), dict(pert=L + 2), dict(actual=A + 2), dict(sums=OUT + 2), dict(map=AUX + 2), dict(workspace=WS + 8)]),
        # one tile of 64 pixels a case: 3 * 8 doubles of partials
        (ARG, "cae_case_importance: needs a workspace of 192 bytes (cae_case_importance_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=191)]),
    ],
    "cae_score_quantiles": [
        (ARG, "cae_score_quantiles: bad argument (CAE_ELEM_* kinds, 0 <= n_case < 2^31, plane >= 0, at most 2^40 scores, group 0 or "
              "1, 1 <= n_level <= 8)",
         [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(scale_kind=4), dict(scale_kind=-1),
          dict(n_case=-1), dict(n_case=1 << 31), dict(plane=-1), dict(plane=(1 << 40) + 1), dict(n_case=1 << 20, plane=(1 << 20) + 1),
          dict(group=2), dict(group=-1), dict(n_level=0), dict(n_level=9)]),
        (ARG, "cae_score_quantiles: negative stride", [dict(pred_stride=-1), dict(actual_stride=-1), dict(scale_stride=-1)]),
        (ARG, "cae_score_quantiles: null pointer", [dict(num=None), dict(den=None), dict(q=None), dict(n=None)]),
        (ARG, "cae_score_quantiles: the levels must be num / den with 0 < num < den <= 10^6, strictly ascending",
         [dict(num=(0, 9)), dict(num=(2, 9)), dict(den=(2, 1000001)), dict(num=(9, 1), den=(10, 2)), dict(num=(1, 2), den=(2, 4))]),
        (ARG, "cae_score_quantiles: the outputs must be 8-byte aligned", [dict(q=OUT + 2), dict(n=AUX + 2)]),
        (ARG, "cae_score_quantiles: null pointer", [dict(pred=None), dict(actual=None)]),
        (ARG, "cae_score_quantiles: a case stride is shorter than the plane",
         [dict(pred_stride=34), dict(actual_stride=34), dict(scale_stride=34)]),
        (ARG, "cae_score_quantiles: an operand reaches 2^60 elements from its pointer",
         [dict(pred_stride=BIG), dict(actual_stride=BIG), dict(scale_stride=BIG)]),
        (ARG, "cae_score_quantiles: pointers must be aligned to their element size", [dict(pred=P + 2), dict(actual=A + 2), dict(scale=L + 2)]),
        # pooled: 32 words of state and a table of 256 bins for each of the 8 levels a call may have
        (ARG, "cae_score_quantiles: needs a workspace of 16640 bytes (cae_score_quantiles_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=16639), dict(workspace=WS + 2)]),
    ],
    "cae_score_counts": [
        (ARG, "cae_score_counts: bad argument (CAE_ELEM_* kinds, 0 <= n_case < 2^31, plane >= 0, at most 2^40 scores, group 0 or 1, "
              "1 <= n_level <= 8)",
         [dict(pred_kind=4), dict(pred_kind=-1), dict(actual_kind=4), dict(actual_kind=-1), dict(scale_kind=4), dict(scale_kind=-1),
          dict(n_case=-1), dict(n_case=1 << 31), dict(plane=-1), dict(plane=(1 << 40) + 1), dict(n_case=1 << 20, plane=(1 << 20) + 1),
          dict(group=2), dict(group=-1), dict(n_level=0), dict(n_level=9)]),
        (ARG, "cae_score_counts: negative stride", [dict(pred_stride=-1), dict(actual_stride=-1), dict(scale_stride=-1)]),
        (ARG, "cae_score_counts: null pointer", [dict(count=None), dict(n=None)]),
        (ARG, "cae_score_counts: q and the outputs must be 8-byte aligned", [dict(q=OUT + 2), dict(count=AUX + 2), dict(n=AUX2 + 2)]),
        (ARG, "cae_score_counts: null pointer", [dict(q=None), dict(pred=None), dict(actual=None)]),
        (ARG, "cae_score_counts: a case stride is shorter than the plane",
         [dict(pred_stride=34), dict(actual_stride=34), dict(scale_stride=34)]),
        (ARG, "cae_score_counts: an operand reaches 2^60 elements from its pointer",
         [dict(pred_stride=BIG), dict(actual_stride=BIG), dict(scale_stride=BIG)]),
        (ARG, "cae_score_counts: pointers must be aligned to their element size", [dict(pred=P + 2), dict(actual=A + 2), dict(scale=L + 2)]),
    ],
    "cae_interval_bounds": [
        (ARG, "cae_interval_bounds: bad argument (CAE_ELEM_* kinds, 0 <= n_case < 2^31, plane >= 0, at most 2^40 pixels, group 0 or 1)",
         [dict(pred_kind=4), dict(pred_kind=-1), dict(scale_kind=4), dict(scale_kind=-1), dict(n_case=-1), dict(n_case=1 << 31),
          dict(plane=-1), dict(plane=(1 << 40) + 1), dict(n_case=1 << 20, plane=(1 << 20) + 1), dict(group=2), dict(group=-1)]),
        (ARG, "cae_interval_bounds: negative stride", [dict(pred_stride=-1), dict(scale_stride=-1)]),
        (OK, "", [dict(n_case=0, pred=None, scale=None, q=None, lower=None, upper=None),
                  dict(plane=0, pred=None, scale=None, q=None, lower=None, upper=None)]),
        (ARG, "cae_interval_bounds: null pointer", [dict(pred=None), dict(q=None), dict(lower=None), dict(upper=None)]),
        (ARG, "cae_interval_bounds: a case stride is shorter than the plane", [dict(pred_stride=34), dict(scale_stride=34)]),
        (ARG, "cae_interval_bounds: an operand reaches 2^60 elements from its pointer", [dict(pred_stride=BIG), dict(scale_stride=BIG)]),
        (ARG, "cae_interval_bounds: pointers must be aligned to their element size",
         [dict(pred=P + 2), dict(scale=L + 4), dict(q=AUX + 2), dict(lower=OUT + 2), dict(upper=AUX2 + 2)]),
    ],
    "cae_case_neighbours": [
        (ARG, "cae_case_neighbours: bad argument (0 <= n_query, n_ref < 2^31, 1 <= k <= 32, 0 <= ref_base, ref_base + n_ref < 2^31, "
              "self_offset >= -1, merge 0 or 1)",
         [dict(n_query=-1), dict(n_query=1 << 31), dict(n_ref=-1), dict(n_ref=1 << 31), dict(k=0), dict(k=33), dict(ref_base=-1),
          dict(ref_base=(1 << 31) - 5), dict(self_offset=-2), dict(merge=2), dict(merge=-1)]),
        (ARG, "cae_case_neighbours: dim must be at least 1 while rows exist", [dict(dim=0), dict(dim=0, n_query=0), dict(dim=0, n_ref=0)]),
        # asked before the operands are looked at: a null operand does not hide it
        (ARG, "cae_case_neighbours: a row stride is shorter than dim",
         [dict(query_stride=34), dict(ref_stride=34), dict(query=None, query_stride=34), dict(ref=None, ref_stride=34)]),
        (ARG, "cae_case_neighbours: null output", [dict(dist2=None), dict(index=None), dict(count=None)]),
        (ARG, "cae_case_neighbours: null operand with rows to read", [dict(query=None), dict(ref=None)]),
        (ARG, "cae_case_neighbours: an operand reaches 2^60 elements from its pointer", [dict(query_stride=BIG), dict(ref_stride=1 << 58)]),
        (ARG, "cae_case_neighbours: pointers must be aligned to their element size",
         [dict(query=P + 2), dict(ref=A + 2), dict(dist2=OUT + 2), dict(index=AUX + 2), dict(count=AUX2 + 2)]),
        (OK, "", [dict(n_query=0, query=None, workspace=None, workspace_bytes=0),
                  dict(n_query=0, n_ref=0, dim=0, query=None, ref=None, workspace=None, workspace_bytes=0)]),
        # one split: 3 * 2 distances, as many indices, and the validity of 3 + 5 rows
        (ARG, "cae_case_neighbours: needs a workspace of 104 bytes (cae_case_neighbours_workspace_bytes)",
         [dict(workspace=None), dict(workspace_bytes=103), dict(workspace=WS + 2)]),
        (OK, "", [dict(n_ref=0, ref=None, merge=1)]),
    ],
}

ROWS = [(fn, rc, text, change) for (fn, groups) in TABLE.items() for (rc, text, changes) in groups for change in changes]


def _row_id(row):
    (fn, _, _, change) = row
    return fn[4:] + "-" + ",".join(f"{k}={sorted(set(v.items()) - set(GEOM.items())) if isinstance(v, dict) else v}" for (k, v) in change.items())


def test_the_table_names_all_21_entry_points():
    assert sorted(TABLE) == sorted(CALLS) and len(CALLS) == 21
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
    for (name, ctype) in HOST_ARRAYS.items():
        if isinstance(args.get(name), tuple):
            args[name] = (ctype * len(args[name]))(*args[name])
    got = getattr(lib, fn)(*(args[n] for n in names.split()))
    message = lib.cae_last_error().decode() if got != OK else ""
    print(f"{_row_id(row)}: {got} {message!r}")
    assert (got, message) == (rc, text)
