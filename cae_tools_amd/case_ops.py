"""The case kernels of libcae_hip (include/cae_hip.h) as functions, no engine needed: measures, per-pixel sums, spectra, SSIM,
interpolation baseline, value distributions, skill by stratum, neighbourhood skill, permutation importance, prediction
intervals, novelty against a reference set, model comparison and its bootstrap, the error moments of a blend of models, ensemble
verification, value range and rendered pages of channel 0 of (N, C, H, W) operands; and the blended field over all channels."""
import ctypes as C
import math
from contextlib import contextmanager
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._engine_base import require_gpu
from ._lib import check
from .device_ops import _is_big_endian_slab, _upload_raw

_TORCH_KINDS = {torch.float32: _lib.ELEM_F32, torch.float64: _lib.ELEM_F64}
# cases per call, which bounds the workspace (for SSIM the pooled planes); a case's sums do not depend on the cut
(_SPECTRA_CASES, _SSIM_CASES) = (512, 256)
_BASELINE_FIELD_BYTES = 256 << 20       # of fp64 field per cae_case_baseline call when the field is asked for
_RENDER_BYTES = 64 << 20                # of rendered pages per group of cae_render_cases calls
_FSS_PLANE_BYTES = 256 << 20            # of bit-planes per cae_case_fss call (one case at least)
_COMPARE_BYTES = 256 << 20              # of per-tile partials per cae_case_compare call (one case at least)


@dataclass(frozen=True, eq=False)
class DeviceOperand:
    """One operand of the case kernels on the device: what device_operand returns, and takes again without another upload"""

    tensor: torch.Tensor        # kept alive; the raw bytes of a big-endian slab, else the array itself
    kind: int                   # _lib.ELEM_*
    shape: tuple                # of the array
    stride: int                 # from one case to the next, in elements

    @property
    def elem_bytes(self):
        return 4 if self.kind in (_lib.ELEM_F32, _lib.ELEM_F32_BE) else 8

    def args(self, case0=0):
        """(pointer to case case0, element kind, case stride): the three C arguments of an operand"""
        return self.tensor.data_ptr() + case0 * self.stride * self.elem_bytes, self.kind, self.stride


def _args(op, case0=0):
    """op.args(case0), or the C arguments of an optional operand that is not there (the caller keeps op alive over the call)"""
    return op.args(case0) if op is not None else (None, 0, 0)


def device_operand(x, device=None):
    """x (numpy array, raw NetCDF-3 slab or CUDA tensor) on the device, ready for the case kernels.  A CUDA tensor is used in
    place; a C-contiguous big-endian >f4 / >f8 numpy array (a NetCDF-3 slab) goes up as its raw bytes and is swapped inside
    the kernel; any other array is uploaded in its native fp32 / fp64 form.  An operand made earlier is handed through, so
    one upload serves several calls."""
    if isinstance(x, DeviceOperand):
        return x
    device = _case_device(device, x)
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            x = x.numpy()
        else:
            if x.dtype not in _TORCH_KINDS:
                x = x.to(torch.float64)
            x = x.contiguous()
            return DeviceOperand(x, _TORCH_KINDS[x.dtype], tuple(x.shape), int(x.stride(0)))
    arr = np.asarray(x)
    for (dtype, kind) in ((">f4", _lib.ELEM_F32_BE), (">f8", _lib.ELEM_F64_BE)):
        if _is_big_endian_slab(arr, dtype):
            return DeviceOperand(_upload_raw(arr, device), kind, arr.shape, int(np.prod(arr.shape[1:])))
    if arr.dtype.newbyteorder("=") != np.dtype(np.float32):
        arr = arr.astype(np.float64)
    t = torch.from_numpy(np.ascontiguousarray(arr, dtype=arr.dtype.newbyteorder("="))).to(device)
    return DeviceOperand(t, _TORCH_KINDS[t.dtype], tuple(t.shape), int(np.prod(t.shape[1:])))


def device_operands(xs, device=None):
    """(device, the operands xs on it): the device given, else that of a device-resident operand, else the current one"""
    device = _case_device(device, *xs)
    return device, [device_operand(x, device) for x in xs]


def _case_device(device, *operands):
    """the device the case kernels run on: the one given, else that of a device-resident operand, else the current one"""
    if device is None:
        for x in operands:
            if isinstance(x, DeviceOperand):
                x = x.tensor
            if isinstance(x, torch.Tensor) and x.is_cuda:
                return x.device
        require_gpu()
        device = torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _pair(name, pred, actual, device):
    """(device, prediction, target, N, H, W) of a function over pairs of cases: (N, C, H, W) operands with N, H and W in common"""
    (device, (p, a)) = device_operands((pred, actual), device)
    if len(p.shape) != 4 or len(a.shape) != 4:
        raise ValueError(f"{name}: (N, C, H, W) arrays expected, got {p.shape} and {a.shape}")
    if p.shape[0] != a.shape[0] or p.shape[2:] != a.shape[2:]:
        raise ValueError(f"{name}: prediction {p.shape} and target {a.shape} do not match")
    return device, p, a, int(p.shape[0]), int(p.shape[2]), int(p.shape[3])


def _workspace(device, size_fn, *args, least=8):
    """(uint8 CUDA tensor, the bytes size_fn(*args) asks for): the workspace of a call, allocated with at least `least` bytes"""
    need = int(size_fn(*args))
    return torch.empty(max(need, least), dtype=torch.uint8, device=device), need


@contextmanager
def _stream(device):
    """the current stream of `device` as the C argument, with the device current"""
    with torch.cuda.device(device):
        yield torch.cuda.current_stream(device).cuda_stream


def case_measures(pred, actual, device=None):
    """Per-case (mae, mse) of channel 0, the reference's ModelEvaluator.compute_measure (model_evaluator.py:87-95)
    for every case at once: mean |p - a| and mean (p - a)^2 over [i, 0, :, :] in fp64.  pred / actual: (N, C, H, W) numpy
    arrays or CUDA tensors (fp32 or fp64; C may differ).  One streaming pass of cae_case_measures.  Returns an (N, 2)
    float64 numpy array."""
    (device, p, a, n, h, w) = _pair("case_measures", pred, actual, device)
    plane = h * w
    out = torch.empty((n, 2), dtype=torch.float64, device=device)
    if n == 0:
        return np.zeros((0, 2), dtype=np.float64)
    if plane == 0:
        return np.full((n, 2), np.nan)      # np.mean of an empty plane
    lib = _lib.load()
    (ws, need) = _workspace(device, lib.cae_case_measures_workspace_bytes, n, plane)
    with _stream(device) as stream:
        check(lib.cae_case_measures(*p.args(), *a.args(), n, plane, out.data_ptr(), ws.data_ptr(), need, stream))
        sums = out.cpu().numpy()
    return sums / float(plane)


def pixel_sums(pred, actual, shift=0.0, case_chunk=0, device=None):
    """The nine per-pixel sums of channel 0 over the cases (cae_pixel_sums, include/cae_hip.h): a (9, H, W) float64 numpy
    array {n, S d, S|d|, S d^2, S a', S p', S a'^2, S p'^2, S a'p'} with d = p - a, a' = a - shift, p' = p - shift over the
    cases whose two values at the pixel are finite.  Operands as case_measures takes them; case_chunk 0 leaves the cut
    of the cases to the library.  shift: one number, or a (2, H, W) array of per-pixel shifts for a and p
    (cae_pixel_sums_about).  utils/skill_maps.maps_from_sums turns the sums into the skill maps."""
    (device, p, a, n, h, w) = _pair("pixel_sums", pred, actual, device)
    plane = h * w
    about = np.ndim(shift) != 0
    if about and np.shape(shift) != (2, h, w):
        raise ValueError(f"pixel_sums: per-pixel shifts of shape (2, {h}, {w}) expected, got {np.shape(shift)}")
    if n == 0 or plane == 0:
        return np.zeros((9, h, w), dtype=np.float64)
    lib = _lib.load()
    (ws, need) = _workspace(device, lib.cae_pixel_sums_workspace_bytes, n, plane, int(case_chunk))
    out = torch.empty((9, h, w), dtype=torch.float64, device=device)
    with _stream(device) as stream:
        shifts = torch.from_numpy(np.ascontiguousarray(shift, dtype=np.float64)).to(device) if about else None
        (fn, by) = (lib.cae_pixel_sums_about, shifts.data_ptr()) if about else (lib.cae_pixel_sums, float(shift))
        check(fn(*p.args(), *a.args(), n, plane, by, int(case_chunk), out.data_ptr(), ws.data_ptr(), need, stream))
        return out.cpu().numpy()


def case_spectra(pred, actual, device=None):
    """The four binned spectral sums of channel 0 per case (cae_case_spectra, include/cae_hip.h): (sums (N, n_bin, 4) float64
    {S w|P|^2, S w|A|^2, S w Re(P conj A), S w|D|^2}, counted (N,) bool) for the Hann-windowed, mean-free prediction P,
    target A and error D = (p - a) over the radial bins of utils/spectra.bin_table(H, W).  A case with a value that is
    not finite is not counted and has zero sums.  Operands as pixel_sums takes them.
    utils/spectra.curves_from_sums turns the sums into the spectra, their ratio, the coherence and the error share."""
    from .utils import spectra
    (device, p, a, n, h, w) = _pair("case_spectra", pred, actual, device)
    if not (1 <= h <= 2048 and 1 <= w <= 2048):
        raise ValueError(f"case_spectra: planes of 1 to 2048 pixels a side expected, got {h} x {w}")
    table = spectra.bin_table(h, w)
    n_bin = spectra.bin_count(h, w)
    if table.shape != (h, w // 2 + 1) or table.min() < -1 or table.max() >= n_bin:
        raise ValueError("case_spectra: the bin table does not fit its bins")
    if n == 0:
        return np.zeros((0, n_bin, 4), dtype=np.float64), np.zeros(0, dtype=bool)
    lib = _lib.load()
    sums = torch.empty((n, n_bin, 4), dtype=torch.float64, device=device)
    counted = torch.empty(n, dtype=torch.int32, device=device)
    (wy, wx) = (torch.from_numpy(spectra.window(side)).to(device) for side in (h, w))
    bins = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(device)
    (ws, need) = _workspace(device, lib.cae_case_spectra_workspace_bytes, min(n, _SPECTRA_CASES), h, w, n_bin, least=16)
    with _stream(device) as stream:
        for lo in range(0, n, _SPECTRA_CASES):
            g = min(n, lo + _SPECTRA_CASES) - lo
            check(lib.cae_case_spectra(*p.args(lo), *a.args(lo), g, h, w, wy.data_ptr(), wx.data_ptr(), bins.data_ptr(), n_bin,
                                       sums[lo:].data_ptr(), counted[lo:].data_ptr(), ws.data_ptr(), need, stream))
        return sums.cpu().numpy(), counted.cpu().numpy() != 0


def case_ssim(pred, actual, vmin, vmax, n_scale=None, device=None):
    """The SSIM sums of channel 0 per case and scale (cae_case_ssim, include/cae_hip.h): an (N, n_scale, 3) float64 numpy
    array {n, S ssim, S cs} over the counted 11 x 11 windows of scale s, for x = (p - vmin) * (1 / (vmax - vmin)) and y
    likewise (data_range 1, the VAE loss's definition).  A window over a value that is not finite is left out, for that case
    and scale only.  n_scale None: 5 where min(H, W) > 160 (MS-SSIM is defined), else 1.  Operands as case_spectra takes them.
    utils/ssim.scores_from_sums turns the sums into ssim, ms_ssim and psnr."""
    from .utils import ssim
    (device, p, a, n, h, w) = _pair("case_ssim", pred, actual, device)
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError(f"case_ssim: planes of 1 to 16384 pixels a side expected, got {h} x {w}")
    n_scale = ssim.default_scales(h, w) if n_scale is None else int(n_scale)
    if not 1 <= n_scale <= ssim.MAX_SCALES:
        raise ValueError(f"case_ssim: n_scale must be 1 to {ssim.MAX_SCALES}, got {n_scale}")
    (shift, scale) = (float(vmin), 1.0 / (float(vmax) - float(vmin)) if float(vmax) != float(vmin) else math.inf)
    if not (math.isfinite(shift) and math.isfinite(scale)):
        raise ValueError(f"case_ssim: vmin and 1 / (vmax - vmin) must be finite, got vmin {vmin!r} and vmax {vmax!r}")
    if n == 0:
        return np.zeros((0, n_scale, 3), dtype=np.float64)
    lib = _lib.load()
    sums = torch.empty((n, n_scale, 3), dtype=torch.float64, device=device)
    win = (C.c_double * ssim.WIN_SIZE)(*ssim.window().tolist())
    (ws, need) = _workspace(device, lib.cae_case_ssim_workspace_bytes, min(n, _SSIM_CASES), h, w, n_scale)
    with _stream(device) as stream:
        for lo in range(0, n, _SSIM_CASES):
            g = min(n, lo + _SSIM_CASES) - lo
            check(lib.cae_case_ssim(*p.args(lo), *a.args(lo), g, h, w, n_scale, shift, scale, win, sums[lo:].data_ptr(),
                                    ws.data_ptr(), need, stream))
        return sums.cpu().numpy()


def case_baseline(low, pred, actual, mode="bicubic", field=False, device=None):
    """Skill against interpolating the input (cae_case_baseline, include/cae_hip.h): channel 0 of low (N, C, h, w) is
    interpolated to the grid of actual (N, C, H, W) - mode "nearest", "bilinear" or "bicubic", the formulas of
    torch.nn.functional.interpolate with align_corners=False - inside the kernel that compares it: an (N, 6) float64 numpy
    array {n, S|b - a|, S(b - a)^2, S|p - a|, S(p - a)^2, n_won} per case over the pixels where a, p and every tap of b
    are finite.  pred None: entries 3..5 are zero.  field=True returns (sums, b) with b the (N, H, W) float64 interpolated
    field, NaN where a tap is not finite.  Operands as case_ssim takes them.  utils/baseline.scores_from_sums turns the
    sums into baseline_mse, skill and win_fraction."""
    from .utils import baseline
    if mode not in baseline.MODES:
        raise ValueError(f"case_baseline: mode must be one of {', '.join(baseline.MODES)}, got {mode!r}")
    device = _case_device(device, low, pred, actual)
    (lo, a) = (device_operand(low, device), device_operand(actual, device))
    if len(lo.shape) != 4 or len(a.shape) != 4 or lo.shape[0] != a.shape[0]:
        raise ValueError(f"case_baseline: (N, C, h, w) and (N, C, H, W) arrays expected, got {lo.shape} and {a.shape}")
    p = device_operand(pred, device) if pred is not None else None
    if p is not None and (len(p.shape) != 4 or p.shape[0] != a.shape[0] or p.shape[2:] != a.shape[2:]):
        raise ValueError(f"case_baseline: prediction {p.shape} and target {a.shape} do not match")     # _pair's rule, one text
    (n, h_in, w_in, h, w) = (int(a.shape[0]), int(lo.shape[2]), int(lo.shape[3]), int(a.shape[2]), int(a.shape[3]))
    if min(h_in, w_in, h, w) < 1:
        raise ValueError(f"case_baseline: planes of at least one pixel expected, got {h_in} x {w_in} and {h} x {w}")
    if n == 0:
        empty = np.zeros((0, 6), dtype=np.float64)
        return (empty, np.zeros((0, h, w), dtype=np.float64)) if field else empty
    lib = _lib.load()
    group = max(1, min(n, _BASELINE_FIELD_BYTES // (8 * h * w))) if field else n
    sums = torch.empty((n, 6), dtype=torch.float64, device=device)
    (ws, need) = _workspace(device, lib.cae_case_baseline_workspace_bytes, group, h, w)
    out = np.empty((n, h, w), dtype=np.float64) if field else None
    with _stream(device) as stream:
        for c0 in range(0, n, group):
            g = min(n, c0 + group) - c0
            b = torch.empty((g, h, w), dtype=torch.float64, device=device) if field else None
            check(lib.cae_case_baseline(*lo.args(c0), h_in, w_in, *_args(p, c0), *a.args(c0),
                                        g, h, w, baseline.MODES[mode], sums[c0:].data_ptr(), b.data_ptr() if field else None,
                                        ws.data_ptr(), need, stream))
            if field:
                out[c0:c0 + g] = b.cpu().numpy()
        sums = sums.cpu().numpy()
    return (sums, out) if field else sums


def joint_histogram(pred, actual, lo, hi, n_bin=128, sub=8, device=None):
    """The value distributions of channel 0 (cae_joint_hist, include/cae_hip.h) over the pixels where prediction p and
    target a are both finite: (joint (n_bin, n_bin) int64 with joint[ia][ip] the count of the coarse bin pair, marginals
    (2, n_bin * sub) int64 fine counts of a and of p, cond (2, n_bin, 4) float64 {S d, S|d|, S d^2, S (a - lo)} keyed by
    the bin of a and {S d, S|d|, S d^2, S (p - lo)} keyed by the bin of p with d = p - a, outside (4,) int64
    {a < lo, a > hi, p < lo, p > hi}).  n_bin coarse bins of `sub` fine bins each over [lo, hi]; a value outside goes to
    the nearest bin, hi itself to the last.  Operands as case_baseline takes them.  utils/distribution.curves_from_counts
    turns the arrays into the conditional bias, reliability, quantiles and exceedance scores."""
    (device, p, a, n, h, w) = _pair("joint_histogram", pred, actual, device)
    (lo, hi) = (float(lo), float(hi))
    if int(n_bin) != n_bin or not 1 <= int(n_bin) <= 128:
        raise ValueError(f"joint_histogram: n_bin must be an integer from 1 to 128, got {n_bin!r}")
    if int(sub) != sub or not 1 <= int(sub) <= 32:
        raise ValueError(f"joint_histogram: sub must be an integer from 1 to 32, got {sub!r}")
    (n_bin, sub) = (int(n_bin), int(sub))
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo and math.isfinite(hi - lo) and math.isfinite(n_bin * sub / (hi - lo))):
        raise ValueError(f"joint_histogram: lo and hi must be finite with hi > lo and n_bin * sub / (hi - lo) finite, got {lo!r} and {hi!r}")
    plane = h * w
    if n * plane >= 1 << 40:
        raise ValueError(f"joint_histogram: fewer than 2^40 pixels a call expected, got {n} x {plane}")
    joint = torch.empty((n_bin, n_bin), dtype=torch.int64, device=device)
    marg = torch.empty((2, n_bin * sub), dtype=torch.int64, device=device)
    cond = torch.empty((2, n_bin, 4), dtype=torch.float64, device=device)
    outside = torch.empty(4, dtype=torch.int64, device=device)
    lib = _lib.load()
    (ws, need) = _workspace(device, lib.cae_joint_hist_workspace_bytes, n, plane, n_bin, sub)
    with _stream(device) as stream:
        check(lib.cae_joint_hist(*p.args(), *a.args(), n, plane, lo, hi, n_bin, sub, joint.data_ptr(), marg.data_ptr(),
                                 cond.data_ptr(), outside.data_ptr(), ws.data_ptr(), need, stream))
        return joint.cpu().numpy(), marg.cpu().numpy(), cond.cpu().numpy(), outside.cpu().numpy()


def strata_sums(pred, actual, strata, edges, shift=0.0, channel=0, device=None):
    """The error sums of channel 0 conditioned on a third field (cae_strata_sums, include/cae_hip.h): (counts, sums) with
    counts = {"members": (n_strata,) int64 pixels of the target grid per stratum, "pairs": (n_strata,) int64 of them with
    prediction and target finite, "unclassified": int pixels whose stratifier is not finite} and sums (n_strata, 8) float64
    {S d, S|d|, S d^2, S a', S p', S a'^2, S p'^2, S a'p'} over the pairs with d = p - a, a' = a - shift_a[k], p' = p -
    shift_p[k].  strata: (N, C, sh, sw), whose plane `channel` covers the target's extent - the nearest source pixel is
    taken by cae_case_baseline's "nearest" rule - or (N,) for one value per case.  edges: up to 63 finite, strictly
    ascending numbers; the stratum of a value is the number of edges at or below it.  shift: one number, or a
    (2, n_strata) array of per-stratum shifts for a and p.  Operands as case_baseline takes them.
    utils/strata.scores_from_sums turns the sums into the scores per stratum."""
    (device, p, a, n, h, w) = _pair("strata_sums", pred, actual, device)
    s = device_operand(strata, device)
    if len(s.shape) not in (1, 4) or s.shape[0] != n:
        raise ValueError(f"strata_sums: a stratifier of (N, C, sh, sw) or (N,) with N = {n} expected, got {tuple(s.shape)}")
    (c, sh, sw) = (int(s.shape[1]), int(s.shape[2]), int(s.shape[3])) if len(s.shape) == 4 else (1, 1, 1)
    if int(channel) != channel or not 0 <= int(channel) < c:
        raise ValueError(f"strata_sums: channel must be an integer from 0 to {c - 1}, got {channel!r}")
    try:
        edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"strata_sums: edges must be numbers, got {edges!r}") from None
    if edges.size > 63 or not np.isfinite(edges).all() or not (np.diff(edges) > 0).all():
        raise ValueError(f"strata_sums: at most 63 finite, strictly ascending edges expected, got {edges.tolist()}")
    n_strata = int(edges.size) + 1
    if np.ndim(shift) != 0 and np.shape(shift) != (2, n_strata):
        raise ValueError(f"strata_sums: per-stratum shifts of shape (2, {n_strata}) expected, got {np.shape(shift)}")
    shifts = np.ascontiguousarray(np.broadcast_to(np.asarray(shift, dtype=np.float64), (2, n_strata)))
    if not np.isfinite(shifts).all():
        raise ValueError("strata_sums: the shifts must be finite")
    empty = {"members": np.zeros(n_strata, dtype=np.int64), "pairs": np.zeros(n_strata, dtype=np.int64), "unclassified": 0}
    if n == 0 or h * w == 0:
        return empty, np.zeros((n_strata, 8), dtype=np.float64)
    if sh * sw == 0:
        raise ValueError(f"strata_sums: a stratifier plane of at least one pixel expected, got {sh} x {sw}")
    counts = torch.empty(2 * n_strata + 1, dtype=torch.int64, device=device)
    sums = torch.empty((n_strata, 8), dtype=torch.float64, device=device)
    lib = _lib.load()
    (ws, need) = _workspace(device, lib.cae_strata_sums_workspace_bytes, n, h, w, n_strata)
    (s_ptr, s_kind, s_stride) = s.args()
    as_c = lambda v: v.ctypes.data_as(C.c_void_p)      # noqa: E731
    with _stream(device) as stream:
        check(lib.cae_strata_sums(*p.args(), *a.args(), s_ptr + int(channel) * sh * sw * s.elem_bytes, s_kind, s_stride, n, h, w,
                                  sh, sw, as_c(edges) if edges.size else None, int(edges.size), as_c(shifts[0]), as_c(shifts[1]),
                                  counts.data_ptr(), sums.data_ptr(), ws.data_ptr(), need, stream))
        counts = counts.cpu().numpy()
        sums = sums.cpu().numpy()
    return {"members": counts[:n_strata].copy(), "pairs": counts[n_strata:2 * n_strata].copy(),
            "unclassified": int(counts[2 * n_strata])}, sums


def fraction_skill(pred, actual, thresholds, widths=None, gaps="strict", device=None):
    """The window sums of the Fractions Skill Score of channel 0 (cae_case_fss, include/cae_hip.h): an (N, T, S, 6) int64
    numpy array {windows, S cM, S cO, S cM^2, S cO^2, S cM cO} per case, threshold and width over the counted n x n windows
    that lie wholly inside the image, cM and cO being the window's numbers of prediction and target events among the pixels
    where both are finite.  thresholds: 1 to 8 numbers (the event is v >= t) or (value, "above" | "below") pairs ("below":
    v < t).  widths: up to 8 odd, ascending widths from 1 to 129; None: the DEFAULT widths of utils/fss.py at or below
    min(H, W).  gaps "strict": a window over a pixel where a value is not finite is left out; "ignore": such a pixel is a
    non-event in both fields and a window is left out only where it holds no pair at all.  Exact integers, the same from run
    to run.  Operands as case_ssim takes them; the cases go in groups that bound the workspace, and a case's sums do not
    depend on the cut.  utils/fss.scores_from_sums turns the sums into FSS, frequencies and the skilful width."""
    from .utils import fss
    (device, p, a, n, h, w) = _pair("fraction_skill", pred, actual, device)
    if not (0 <= h <= 16384 and 0 <= w <= 16384):
        raise ValueError(f"fraction_skill: planes of up to 16384 pixels a side expected, got {h} x {w}")
    try:
        (values, sides) = fss.check_thresholds(thresholds)
        widths = fss.default_widths(h, w) if widths is None else fss.check_widths(widths)    # no default for a plane without a pixel
        rule = fss.GAPS[gaps]
    except (KeyError, TypeError):
        raise ValueError(f"fraction_skill: gaps must be one of {', '.join(fss.GAPS)}, got {gaps!r}") from None
    except ValueError as refused:
        raise ValueError(f"fraction_skill: {refused}") from None
    (n_thr, n_width) = (len(values), len(widths))
    if n == 0 or h * w == 0 or n_width == 0:     # n_width 0: the default widths of a plane without a pixel
        return np.zeros((n, n_thr, n_width, 6), dtype=np.int64)
    lib = _lib.load()
    group = max(1, min(n, _FSS_PLANE_BYTES // int(lib.cae_case_fss_workspace_bytes(1, h, w, n_thr))))
    sums = torch.empty((n, n_thr, n_width, 6), dtype=torch.int64, device=device)
    (ws, need) = _workspace(device, lib.cae_case_fss_workspace_bytes, group, h, w, n_thr)
    (thr_c, side_c, width_c) = ((C.c_double * n_thr)(*values), (C.c_int * n_thr)(*sides), (C.c_int * n_width)(*widths))
    with _stream(device) as stream:
        for c0 in range(0, n, group):
            g = min(n, c0 + group) - c0
            check(lib.cae_case_fss(*p.args(c0), *a.args(c0), g, h, w, thr_c, side_c, n_thr, width_c, n_width, rule,
                                   sums[c0:].data_ptr(), ws.data_ptr(), need, stream))
        return sums.cpu().numpy()


def operand_cases(op, c0, c1):
    """the cases c0 .. c1 - 1 of a device operand as an operand of its own: no copy, the tensor is a view of op's"""
    (c0, c1) = (int(c0), int(c1))
    if not 0 <= c0 <= c1 <= int(op.shape[0]):
        raise IndexError(f"operand_cases: cases [{c0}, {c1}) are not within [0, {int(op.shape[0])})")
    if op.tensor.dim() == 1 and op.tensor.dtype == torch.uint8:     # the raw bytes of a big-endian slab
        per = op.stride * op.elem_bytes
        view = op.tensor[c0 * per:c1 * per]
    else:
        view = op.tensor[c0:c1]
    return DeviceOperand(view, op.kind, (c1 - c0,) + tuple(op.shape[1:]), op.stride)


def pack_gather(raw, dst, c_off, rows, vmin, vmax, enable=True):
    """dst[i, c_off:c_off + Cv] = normalise(raw[rows[i]]) on the device (cae_normalise_pack_gather, include/cae_hip.h): the
    arithmetic of device_ops.normalise_pack bit for bit, the source row of every destination row read from rows, an int32
    CUDA tensor of dst.shape[0] entries in any order, repeats allowed.  raw: (n_src, Cv, h, w) fp32 CUDA tensor; dst:
    (n_dst, C, h, w) fp32 CUDA tensor, whose other channels are not touched.  A row index outside 0 .. n_src - 1 is not
    followed: that row of dst gets NaN."""
    for (name, t) in (("raw", raw), ("dst", dst)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() >= 2 and t.is_contiguous()):
            raise ValueError(f"pack_gather: {name} must be a contiguous float32 CUDA tensor of at least 2 dimensions")
    if not (isinstance(rows, torch.Tensor) and rows.dtype == torch.int32 and rows.device == raw.device and rows.dim() == 1
            and rows.is_contiguous() and rows.numel() == int(dst.shape[0])) or dst.device != raw.device:
        raise ValueError("pack_gather: rows must be a contiguous int32 tensor of one entry per row of dst on the data's device")
    (n_src, c_src) = (int(raw.shape[0]), int(raw.shape[1]))
    hw = int(np.prod(raw.shape[2:]))
    if int(np.prod(dst.shape[2:])) != hw:
        raise ValueError(f"pack_gather: planes of raw {tuple(raw.shape)} and dst {tuple(dst.shape)} do not match")
    rng = float(vmax) - float(vmin)
    lib = _lib.load()
    with _stream(raw.device) as stream:
        check(lib.cae_normalise_pack_gather(raw.data_ptr(), n_src, c_src, hw, dst.data_ptr(), int(dst.shape[0]), int(dst.shape[1]),
                                            int(c_off), C.c_float(float(np.float32(vmin))), C.c_float(float(np.float32(rng))),
                                            1 if enable else 0, rows.data_ptr(), stream))


def dihedral_rows(src, dst, codes, rows=None, group=8):
    """dst[i] = g(codes[i]) applied to src[rows[i]] on the device, every channel, as 32-bit words (cae_dihedral_rows,
    include/cae_hip.h; utils/augment.apply is the numpy definition of a code).  src: (n_src, C, h, w) and dst: (n_dst, C, h, w)
    contiguous float32 CUDA tensors that do not overlap; codes: an int32 CUDA tensor of n_dst entries; rows: likewise, in any
    order, repeats allowed, or None for row i.  group 4 takes the codes 0 .. 3 on any plane, group 8 all eight on square
    planes.  A row index outside 0 .. n_src - 1 or a code outside the group is not followed: that row of dst gets NaN."""
    for (name, t) in (("src", src), ("dst", dst)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()):
            raise ValueError(f"dihedral_rows: {name} must be a contiguous float32 CUDA tensor (N, C, h, w)")
    if dst.device != src.device or tuple(dst.shape[1:]) != tuple(src.shape[1:]):
        raise ValueError(f"dihedral_rows: rows of src {tuple(src.shape)} and dst {tuple(dst.shape)} do not match, or their devices")
    if group not in (4, 8):
        raise ValueError(f"dihedral_rows: group must be 4 or 8, got {group!r}")
    (n_src, n_dst, c, h, w) = (int(src.shape[0]), int(dst.shape[0]), int(src.shape[1]), int(src.shape[2]), int(src.shape[3]))
    if group == 8 and h != w:
        raise ValueError(f"dihedral_rows: group 8 transposes, which needs square planes, got {h} x {w}")
    for (name, t) in (("codes", codes),) + ((("rows", rows),) if rows is not None else ()):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == src.device and t.dim() == 1
                and t.is_contiguous() and t.numel() == n_dst):
            raise ValueError(f"dihedral_rows: {name} must be a contiguous int32 tensor of one entry per row of dst on the data's device")
    if c < 1:
        raise ValueError("dihedral_rows: at least one channel expected")
    lib = _lib.load()
    with _stream(src.device) as stream:
        check(lib.cae_dihedral_rows(src.data_ptr(), n_src, c, h, w, dst.data_ptr(), n_dst, rows.data_ptr() if rows is not None else None,
                                    codes.data_ptr(), int(group), stream))


def ensemble_moments(draws, vmin, vmax, want_std=True):
    """The per-pixel mean and sample standard deviation of K >= 2 members (cae_ensemble_moments, include/cae_hip.h, all draws in
    one call): draws is a contiguous float32 CUDA tensor (K, N, ...) - [draw][case], normalised scores - and the result (mean,
    std) float64 CUDA tensors (N, ...), mean = vmin + (y_0 + S (y_k - y_0) / K) (vmax - vmin) and std (None unless want_std)
    the ddof = 1 deviation times |vmax - vmin|.  A pixel is summed by one lane in draw order: a case's result does not depend
    on the other cases of the call."""
    if not (isinstance(draws, torch.Tensor) and draws.is_cuda and draws.dtype == torch.float32 and draws.dim() >= 3
            and draws.is_contiguous()):
        raise ValueError("ensemble_moments: draws must be a contiguous float32 CUDA tensor (K, N, ...)")
    (k, n) = (int(draws.shape[0]), int(draws.shape[1]))
    if k < 2:
        raise ValueError(f"ensemble_moments: at least 2 draws expected, got {k}")
    plane = int(np.prod(draws.shape[2:]))
    mean = torch.empty(tuple(draws.shape[1:]), dtype=torch.float64, device=draws.device)
    std = torch.empty_like(mean) if want_std else None
    if n and plane:
        lib = _lib.load()
        with _stream(draws.device) as stream:
            check(lib.cae_ensemble_moments(draws.data_ptr(), plane, n * plane, n, plane, k, 0, k, float(vmin), float(vmax) - float(vmin),
                                           mean.data_ptr(), std.data_ptr() if want_std else None, None, 0, stream))
    return mean, std


def case_importance(base, pert, actual, vmin, vmax, maps=None, device=None):
    """The eight sums of permutation importance per case (cae_case_importance, include/cae_hip.h): an (N, 8) float64 numpy
    array {n, S e1^2, S e0^2, S|e1|, S|e0|, S (P1 - P0)^2, #(e1^2 > e0^2), #(e1^2 < e0^2)} of channel 0 with P = vmin +
    (double)p * (vmax - vmin) for the unperturbed scores base and the perturbed scores pert - fp32 CUDA tensors (N, C, H, W)
    as the model wrote them - and e = P - a against the target actual as stored, over the pixels where a, P0 and P1 are all
    finite.  actual as case_measures takes it.  maps: None, or a (3, H, W) float64 CUDA tensor {count, S e1^2, S e0^2} per
    pixel that is CARRIED: the call adds its cases to it in place, the caller clears it before the first call; the map after
    a run of calls over consecutive cases is the same bits as after one call.  A case's sums do not depend on the other
    cases of the call or on maps.  utils/importance.summary turns the sums into the scores."""
    device = _case_device(device, base, pert, actual)
    for (name, t) in (("base", base), ("pert", pert)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.device == device):
            raise ValueError(f"case_importance: {name} must be a float32 CUDA tensor (N, C, H, W) on the device of the call")
    if tuple(base.shape) != tuple(pert.shape):
        raise ValueError(f"case_importance: base {tuple(base.shape)} and pert {tuple(pert.shape)} do not match")
    (base, pert) = (base.contiguous(), pert if pert is base else pert.contiguous())
    a = device_operand(actual, device)
    if len(a.shape) != 4 or a.shape[0] != base.shape[0] or tuple(a.shape[2:]) != tuple(base.shape[2:]):
        raise ValueError(f"case_importance: scores {tuple(base.shape)} and target {tuple(a.shape)} do not match")
    (n, h, w) = (int(base.shape[0]), int(base.shape[2]), int(base.shape[3]))
    plane = h * w
    if maps is not None and not (isinstance(maps, torch.Tensor) and maps.is_cuda and maps.dtype == torch.float64
                                 and tuple(maps.shape) == (3, h, w) and maps.is_contiguous() and maps.device == device):
        raise ValueError(f"case_importance: maps must be a contiguous float64 CUDA tensor (3, {h}, {w}) on the device of the call")
    (vmin, rng) = (float(vmin), float(vmax) - float(vmin))
    if not (math.isfinite(vmin) and math.isfinite(rng)):
        raise ValueError(f"case_importance: vmin and vmax - vmin must be finite, got vmin {vmin!r} and vmax {vmax!r}")
    if n == 0 or plane == 0:
        return np.zeros((n, 8), dtype=np.float64)
    lib = _lib.load()
    sums = torch.empty((n, 8), dtype=torch.float64, device=device)
    (ws, need) = _workspace(device, lib.cae_case_importance_workspace_bytes, n, plane, least=16)
    with _stream(device) as stream:
        check(lib.cae_case_importance(base.data_ptr(), int(base.stride(0)), pert.data_ptr(), int(pert.stride(0)), *a.args(), n, plane,
                                      vmin, rng, sums.data_ptr(), maps.data_ptr() if maps is not None else None, ws.data_ptr(), need,
                                      stream))
        return sums.cpu().numpy()


def case_compare(preds, actual, device=None):
    """Up to 8 predictions against one target on the same pixels (cae_case_compare, include/cae_hip.h): an (N, 2 + 4 M) float64
    numpy array {n, tied, (S e_m, S|e_m|, S e_m^2, wins_m) for m = 0 .. M - 1} per case of channel 0, with e_m = P_m - a in
    fp64 over the pixels where the target and every prediction are finite; candidate m wins a pixel when its squared error is
    strictly the smallest, a pixel whose smallest squared error is shared counts as tied.  preds: a list of 1 to 8 (N, C, H,
    W) operands as case_measures takes them (C may differ); they go to the kernel in one element kind, so where their kinds
    differ those that are not native fp64 are converted to it on the device, which changes no value.  The cases go in chunks
    that bound the workspace, and a case's sums do not depend on the cut.  utils/compare.summary turns the sums, and their
    bootstrap resamples (bootstrap_sums), into the scores."""
    preds = list(preds)
    if not 1 <= len(preds) <= 8:
        raise ValueError(f"case_compare: 1 to 8 predictions expected, got {len(preds)}")
    (device, ops) = device_operands(preds + [actual], device)
    (ps, a) = (ops[:-1], ops[-1])
    for p in ps:
        if len(p.shape) != 4 or len(a.shape) != 4:
            raise ValueError(f"case_compare: (N, C, H, W) arrays expected, got {p.shape} and {a.shape}")
        if p.shape[0] != a.shape[0] or p.shape[2:] != a.shape[2:]:
            raise ValueError(f"case_compare: prediction {p.shape} and target {a.shape} do not match")
    (n, h, w, m) = (int(a.shape[0]), int(a.shape[2]), int(a.shape[3]), len(ps))
    (plane, width) = (h * w, 2 + 4 * len(ps))
    if n == 0 or plane == 0:
        return np.zeros((n, width), dtype=np.float64)
    if len({p.kind for p in ps}) > 1:
        ps = [p if p.kind == _lib.ELEM_F64 else _as_f64(p) for p in ps]
    lib = _lib.load()
    group = max(1, min(n, _COMPARE_BYTES // int(lib.cae_case_compare_workspace_bytes(1, plane, m))))
    sums = torch.empty((n, width), dtype=torch.float64, device=device)
    (ws, need) = _workspace(device, lib.cae_case_compare_workspace_bytes, group, plane, m, least=16)
    strides = (C.c_int64 * m)(*[p.stride for p in ps])
    with _stream(device) as stream:
        for c0 in range(0, n, group):
            g = min(n, c0 + group) - c0
            ptrs = (C.c_void_p * m)(*[p.args(c0)[0] for p in ps])
            check(lib.cae_case_compare(ptrs, ps[0].kind, strides, m, *a.args(c0), g, plane, sums[c0:].data_ptr(), ws.data_ptr(),
                                       need, stream))
        return sums.cpu().numpy()


def _as_f64(op):
    """channel 0 of a device operand as a native fp64 operand (N, 1, H, W), converted on the device: exact for every kind"""
    if op.kind == _lib.ELEM_F32:
        t = op.tensor[:, :1].to(torch.float64)
    else:       # a big-endian slab: its raw bytes, swapped as integers
        (n, per, wide) = (int(op.shape[0]), int(op.shape[2]) * int(op.shape[3]), op.elem_bytes)
        raw = op.tensor.view(n, op.stride * wide)[:, :per * wide].reshape(n, per, wide).flip(2).contiguous()
        t = raw.view(torch.float32 if wide == 4 else torch.float64).reshape(n, 1, int(op.shape[2]), int(op.shape[3])).to(torch.float64)
    t = t.contiguous()
    return DeviceOperand(t, _lib.ELEM_F64, tuple(t.shape), int(t.stride(0)))


def _all_as_f64(op):
    """every channel of a device operand as a native fp64 operand of the same shape, converted on the device: exact for every kind"""
    if op.kind == _lib.ELEM_F64:
        return op
    if op.kind == _lib.ELEM_F32:
        t = op.tensor.to(torch.float64)
    else:       # a big-endian slab: its raw bytes, swapped as integers
        wide = op.elem_bytes
        raw = op.tensor.view(-1, wide).flip(1).contiguous()
        t = raw.view(torch.float32 if wide == 4 else torch.float64).reshape(op.shape).to(torch.float64)
    t = t.contiguous()
    return DeviceOperand(t, _lib.ELEM_F64, tuple(t.shape), int(np.prod(t.shape[1:])))


def moments_width(m):
    """the width of a row of case_error_moments for m candidates: n, m sums of errors, m (m + 1) / 2 sums of products"""
    return 1 + m + m * (m + 1) // 2


def case_error_moments(preds, actual, device=None):
    """The error moments a blend of up to 8 predictions is fitted from (cae_case_error_moments, include/cae_hip.h): an (N, 1 + M +
    M (M + 1) / 2) float64 numpy array {n, S e_0 .. S e_{M-1}, S e_i e_j for i <= j in row-major order} per case of channel 0,
    with e_m = P_m - a in fp64 over the pixels where the target and every prediction are finite.  n, S e_m and S e_m^2 carry the
    bits of case_compare's columns 0, 2 + 4 m and 4 + 4 m.  preds and actual as case_compare takes them: predictions of mixed
    kinds are converted to native fp64 on the device, which changes no value; the cases go in chunks that bound the workspace,
    and a case's row does not depend on the cut.  utils/blend.fit turns the sums into weights."""
    preds = list(preds)
    if not 1 <= len(preds) <= 8:
        raise ValueError(f"case_error_moments: 1 to 8 predictions expected, got {len(preds)}")
    (device, ops) = device_operands(preds + [actual], device)
    (ps, a) = (ops[:-1], ops[-1])
    for p in ps:
        if len(p.shape) != 4 or len(a.shape) != 4:
            raise ValueError(f"case_error_moments: (N, C, H, W) arrays expected, got {p.shape} and {a.shape}")
        if p.shape[0] != a.shape[0] or p.shape[2:] != a.shape[2:]:
            raise ValueError(f"case_error_moments: prediction {p.shape} and target {a.shape} do not match")
    (n, h, w, m) = (int(a.shape[0]), int(a.shape[2]), int(a.shape[3]), len(ps))
    (plane, width) = (h * w, moments_width(m))
    if n == 0 or plane == 0:
        return np.zeros((n, width), dtype=np.float64)
    if len({p.kind for p in ps}) > 1:
        ps = [p if p.kind == _lib.ELEM_F64 else _as_f64(p) for p in ps]
    lib = _lib.load()
    group = max(1, min(n, _COMPARE_BYTES // int(lib.cae_case_error_moments_workspace_bytes(1, plane, m))))
    sums = torch.empty((n, width), dtype=torch.float64, device=device)
    (ws, need) = _workspace(device, lib.cae_case_error_moments_workspace_bytes, group, plane, m, least=16)
    strides = (C.c_int64 * m)(*[p.stride for p in ps])
    with _stream(device) as stream:
        for c0 in range(0, n, group):
            g = min(n, c0 + group) - c0
            ptrs = (C.c_void_p * m)(*[p.args(c0)[0] for p in ps])
            check(lib.cae_case_error_moments(ptrs, ps[0].kind, strides, m, *a.args(c0), g, plane, sums[c0:].data_ptr(), ws.data_ptr(),
                                             need, stream))
        return sums.cpu().numpy()


def blend_predictions(preds, weights, intercept=0.0, device=None):
    """The blended field of up to 8 predictions (cae_blend_predictions, include/cae_hip.h): the (N, C, H, W) float64 numpy array
    y = intercept, then y = y + weights[m] * preds[m] for m ascending over the weights that are not 0, product and sum rounded
    separately in fp64; NaN where a prediction with a weight other than 0 is not finite.  A prediction whose weight is exactly 0
    is not read.  preds: (N, C, H, W) operands of one shape as case_compare takes them; where their kinds differ those that
    are not native fp64 are converted to it on the device, which changes no value.  One streaming launch."""
    preds = list(preds)
    if not 1 <= len(preds) <= 8:
        raise ValueError(f"blend_predictions: 1 to 8 predictions expected, got {len(preds)}")
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != len(preds):
        raise ValueError(f"blend_predictions: one weight per prediction expected, got {w.shape[0]} for {len(preds)}")
    intercept = float(intercept)
    if not (np.isfinite(w).all() and math.isfinite(intercept)):
        raise ValueError("blend_predictions: the weights and the intercept must be finite")
    (device, ps) = device_operands(preds, device)
    for p in ps:
        if len(p.shape) != 4 or tuple(p.shape) != tuple(ps[0].shape):
            raise ValueError(f"blend_predictions: (N, C, H, W) predictions of one shape expected, got {ps[0].shape} and {p.shape}")
    shape = tuple(int(v) for v in ps[0].shape)
    (n, per, m) = (shape[0], shape[1] * shape[2] * shape[3], len(ps))
    if n == 0 or per == 0:
        return np.zeros(shape, dtype=np.float64)
    if len({p.kind for p in ps}) > 1:
        ps = [_all_as_f64(p) for p in ps]
    lib = _lib.load()
    out = torch.empty(shape, dtype=torch.float64, device=device)
    strides = (C.c_int64 * m)(*[p.stride for p in ps])
    ptrs = (C.c_void_p * m)(*[p.args()[0] for p in ps])
    with _stream(device) as stream:
        check(lib.cae_blend_predictions(ptrs, ps[0].kind, strides, m, (C.c_double * m)(*w.tolist()), intercept, n, per,
                                        out.data_ptr(), per, stream))
        return out.cpu().numpy()


def bootstrap_sums(table, resamples, seed=0, first=0, device=None):
    """The paired bootstrap of a table of per-unit sums on the device (cae_bootstrap_sums, include/cae_hip.h): table (n_unit,
    n_col) float64 with 1 <= n_col <= 32 and 1 <= n_unit <= 2^20; returns the (resamples, n_col) float64 numpy array whose row k
    is the sum of the n_unit rows drawn with replacement for resample first + k, added in draw order with plain fp64 adds.  The
    draws are a counter-based function of (seed, resample, draw) alone: exact, the same bits from run to run, resamples cut
    into consecutive calls give the bits of one call, and two tables of the same n_unit resampled with the same seed are
    resampled alike.  tests/compare_ref.py restates it in numpy."""
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.ndim != 2 or not 1 <= table.shape[0] <= 1 << 20 or not 1 <= table.shape[1] <= 32:
        raise ValueError(f"bootstrap_sums: a table (n_unit, n_col) with 1 <= n_unit <= 2^20 and 1 <= n_col <= 32 expected, got {table.shape}")
    (b, first, seed) = (int(resamples), int(first), int(seed))
    if b < 0 or first < 0 or first + b > 1 << 32:
        raise ValueError(f"bootstrap_sums: resamples [{first}, {first + b}) must lie within [0, 2^32)")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"bootstrap_sums: seed must be an integer from 0 to 2^64 - 1, got {seed}")
    (n_unit, n_col) = table.shape
    if b == 0:
        return np.zeros((0, n_col), dtype=np.float64)
    device = _case_device(device)
    lib = _lib.load()
    out = torch.empty((b, n_col), dtype=torch.float64, device=device)
    with _stream(device) as stream:
        t = torch.from_numpy(table).to(device)
        check(lib.cae_bootstrap_sums(t.data_ptr(), n_unit, n_col, first, b, seed, out.data_ptr(), stream))
        return out.cpu().numpy()


_BOOTSTRAP_COLUMNS = 32             # of a table cae_bootstrap_sums takes
_BOOTSTRAP_RESAMPLES = 1 << 18      # resamples per cae_bootstrap_sums call


def bootstrap_table(table, resamples, seed, device=None):
    """cae_bootstrap_sums of a table of any width: column pieces of at most 32 with the same seed - the units of a resample
    depend on (seed, resample, n_unit) alone, so the pieces are resampled alike - and resamples in consecutive pieces"""
    pieces = []
    for c0 in range(0, table.shape[1], _BOOTSTRAP_COLUMNS):
        part = np.ascontiguousarray(table[:, c0:c0 + _BOOTSTRAP_COLUMNS])
        pieces.append(np.concatenate([bootstrap_sums(part, min(_BOOTSTRAP_RESAMPLES, resamples - r0), seed=seed, first=r0, device=device)
                                      for r0 in range(0, resamples, _BOOTSTRAP_RESAMPLES)]))
    return np.concatenate(pieces, axis=1)


def _score_operands(name, pred, actual, scale, device):
    """(device, p, a, s or None, N, H, W) of the three interval functions: _pair, and a scale shaped like the target's cases"""
    (device, p, a, n, h, w) = _pair(name, pred, actual, device)
    s = device_operand(scale, device) if scale is not None else None
    if s is not None and (len(s.shape) != 4 or s.shape[0] != n or tuple(s.shape[2:]) != (h, w)):
        raise ValueError(f"{name}: scale {tuple(s.shape)} and target {tuple(a.shape)} do not match")
    if n >= 1 << 31 or n * h * w > 1 << 40:
        raise ValueError(f"{name}: fewer than 2^31 cases and at most 2^40 scores a call expected, got {n} x {h * w}")
    return device, p, a, s, n, h, w


def _group_code(name, group):
    from .utils import conformal
    try:
        return conformal.GROUPS[group]
    except (KeyError, TypeError):
        raise ValueError(f"{name}: group must be one of {', '.join(conformal.GROUPS)}, got {group!r}") from None


def score_quantiles(pred, actual, levels, group="pooled", scale=None, device=None):
    """Exact split-conformal quantiles of the absolute residual of channel 0 (cae_score_quantiles, include/cae_hip.h): (q, n)
    with q (L, H, W) float64 for group "pixel" or (L,) for "pooled", and n (H, W) or () int64, the valid scores of the group.
    The score is |p - a|, or |p - a| / s with a scale s, over the cases where p and a are finite (and s finite and > 0); for
    a level num/den the rank is k = ceil((n + 1) num / den) and q the k-th smallest score of the group, +inf where k > n.
    levels: 1 to 8 ascending coverage levels as utils/conformal.parse_levels takes them (decimal text or Fractions, never
    floats).  All cases go in one call: a quantile cannot be folded over pieces.  Exact, the same bits from run to run.
    Operands as case_measures takes them."""
    from .utils import conformal
    try:
        levels = conformal.parse_levels(levels)
    except ValueError as refused:
        raise ValueError(f"score_quantiles: {refused}") from None
    code = _group_code("score_quantiles", group)
    (device, p, a, s, n, h, w) = _score_operands("score_quantiles", pred, actual, scale, device)
    (plane, n_level) = (h * w, len(levels))
    groups = 1 if code else plane
    if groups == 0:     # a pixel group of a plane without a pixel
        return np.zeros((n_level, h, w), dtype=np.float64), np.zeros((h, w), dtype=np.int64)
    q = torch.empty((n_level, groups), dtype=torch.float64, device=device)
    count = torch.empty(groups, dtype=torch.int64, device=device)
    lib = _lib.load()
    (ws, need) = _workspace(device, lib.cae_score_quantiles_workspace_bytes, n, plane, code, n_level)
    num = (C.c_int64 * n_level)(*[v.numerator for v in levels])
    den = (C.c_int64 * n_level)(*[v.denominator for v in levels])
    with _stream(device) as stream:
        check(lib.cae_score_quantiles(*p.args(), *a.args(), *_args(s), n, plane, code, num, den, n_level, q.data_ptr(),
                                      count.data_ptr(), ws.data_ptr(), need, stream))
        (q, count) = (q.cpu().numpy(), count.cpu().numpy())
    return (q.reshape(n_level), count.reshape(())) if code else (q.reshape(n_level, h, w), count.reshape(h, w))


def score_counts(pred, actual, q, group, scale=None, device=None):
    """(count, n) of cae_score_counts (include/cae_hip.h): count (L, H, W) or (L,) int64, the valid scores <= q of the group
    per level (a score of +inf is <= +inf), and n (H, W) or () int64, the valid scores.  q: (L, H, W) for group "pixel",
    (L,) for "pooled", float64 as score_quantiles returns it, 1 <= L <= 8.  Operands and scores as score_quantiles.
    Held-out coverage is count.sum() / n.sum() of a level."""
    code = _group_code("score_counts", group)
    (device, p, a, s, n, h, w) = _score_operands("score_counts", pred, actual, scale, device)
    plane = h * w
    q = np.ascontiguousarray(q, dtype=np.float64)
    if q.ndim != (1 if code else 3) or not 1 <= q.shape[0] <= 8 or (not code and q.shape[1:] != (h, w)):
        raise ValueError(f"score_counts: q of shape {'(L,)' if code else f'(L, {h}, {w})'} with 1 <= L <= 8 expected, got {q.shape}")
    n_level = int(q.shape[0])
    groups = 1 if code else plane
    if groups == 0:
        return np.zeros((n_level, h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
    count = torch.empty((n_level, groups), dtype=torch.int64, device=device)
    total = torch.empty(groups, dtype=torch.int64, device=device)
    lib = _lib.load()
    with _stream(device) as stream:
        q_dev = torch.from_numpy(q.reshape(n_level, groups)).to(device)
        check(lib.cae_score_counts(*p.args(), *a.args(), *_args(s), n, plane, code, q_dev.data_ptr(), n_level,
                                   count.data_ptr(), total.data_ptr(), stream))
        (count, total) = (count.cpu().numpy(), total.cpu().numpy())
    return (count.reshape(n_level), total.reshape(())) if code else (count.reshape(n_level, h, w), total.reshape(h, w))


def interval_bounds(pred, q, group, scale=None, device=None):
    """(lower, upper) of cae_interval_bounds (include/cae_hip.h): float64 CUDA tensors (N, H, W), lower = p - q * s and upper =
    p + q * s of channel 0 of pred with the product and the sum rounded separately (p -+ q without a scale).  q: one number
    for group "pooled", an (H, W) array for "pixel".  NaN where p is not finite or s is not finite or <= 0; q = +inf gives
    -inf / +inf.  Operands as score_quantiles."""
    code = _group_code("interval_bounds", group)
    device = _case_device(device, pred, scale)
    p = device_operand(pred, device)
    if len(p.shape) != 4:
        raise ValueError(f"interval_bounds: an (N, C, H, W) prediction expected, got {tuple(p.shape)}")
    (n, h, w) = (int(p.shape[0]), int(p.shape[2]), int(p.shape[3]))
    s = device_operand(scale, device) if scale is not None else None
    if s is not None and (len(s.shape) != 4 or s.shape[0] != n or tuple(s.shape[2:]) != (h, w)):
        raise ValueError(f"interval_bounds: scale {tuple(s.shape)} and prediction {tuple(p.shape)} do not match")
    if n >= 1 << 31 or n * h * w > 1 << 40:
        raise ValueError(f"interval_bounds: fewer than 2^31 cases and at most 2^40 pixels a call expected, got {n} x {h * w}")
    q = np.asarray(q, dtype=np.float64)
    if q.shape != (() if code else (h, w)):
        raise ValueError(f"interval_bounds: q of shape {() if code else (h, w)} expected for group {group!r}, got {q.shape}")
    lower = torch.empty((n, h, w), dtype=torch.float64, device=device)
    upper = torch.empty((n, h, w), dtype=torch.float64, device=device)
    if n * h * w == 0:
        return lower, upper
    lib = _lib.load()
    with _stream(device) as stream:
        q_dev = torch.from_numpy(np.ascontiguousarray(q).reshape(-1)).to(device)
        check(lib.cae_interval_bounds(*p.args(), *_args(s), n, h * w, q_dev.data_ptr(), code, lower.data_ptr(), upper.data_ptr(), stream))
    return lower, upper


def _rows(name, x, device):
    """x (numpy array or CUDA tensor of shape (n, ...)) as a contiguous float32 CUDA tensor (n, D), one row per case"""
    if isinstance(x, torch.Tensor):
        t = x.to(device)
    else:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    if t.dim() < 1:
        raise ValueError(f"case_neighbours: {name} must have a case axis, got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"case_neighbours: {name} must be float32, got {t.dtype}")
    n = int(t.shape[0])
    return t.reshape(n, -1).contiguous() if n else t.reshape(0, int(np.prod(t.shape[1:])))


def case_neighbours(query, reference, k, ref_base=0, self_offset=None, merge_into=None, device=None):
    """The k nearest references of every query row, exact in fp64 (cae_case_neighbours, include/cae_hip.h): (dist2 (n_q, k)
    float64 ascending, index (n_q, k) int32 global reference indices ref_base + j, count (n_q,) int32).  query and reference:
    float32 CUDA tensors or numpy arrays of shape (n, ...), flattened per case, with the same number D of features.  d2 is
    S_d (q_d - r_d)^2 in the difference form, d ascending; a row with a value that is not finite is invalid: such a reference
    is never a neighbour, such a query has count -1, dist2 +inf and index -1.  Candidates are ordered by (d2, index), so ties
    go to the smaller index.  Unused slots hold +inf / -1.  self_offset i0: query i never takes the reference with global
    index i0 + i (leave-one-out).  merge_into: the (dist2, index, count) of earlier calls with the same queries and k over
    other references; the result is the k smallest of the union, the same bits as one call over all references."""
    device = _case_device(device, query, reference)
    (q, r) = (_rows("query", query, device), _rows("reference", reference, device))
    (n_q, n_r) = (int(q.shape[0]), int(r.shape[0]))
    dim = int(q.shape[1]) if n_q else int(r.shape[1])
    if n_q and n_r and int(r.shape[1]) != int(q.shape[1]):
        raise ValueError(f"case_neighbours: queries of {int(q.shape[1])} and references of {int(r.shape[1])} features do not match")
    if int(k) != k or not 1 <= int(k) <= 32:
        raise ValueError(f"case_neighbours: k must be an integer from 1 to 32, got {k!r}")
    k = int(k)
    (ref_base, self_offset) = (int(ref_base), -1 if self_offset is None else int(self_offset))
    if ref_base < 0 or ref_base + n_r > 0x7fffffff or self_offset < -1 or n_q > 0x7fffffff:
        raise ValueError(f"case_neighbours: ref_base {ref_base} and self_offset {self_offset} must not be negative and indices must stay below 2^31")
    if (n_q or n_r) and dim < 1:
        raise ValueError("case_neighbours: rows of at least one feature expected")
    if merge_into is None:
        dist2 = torch.full((n_q, k), math.inf, dtype=torch.float64, device=device)
        index = torch.full((n_q, k), -1, dtype=torch.int32, device=device)
        count = torch.zeros(n_q, dtype=torch.int32, device=device)
    else:
        (d0, i0, c0) = merge_into
        if np.shape(d0) != (n_q, k) or np.shape(i0) != (n_q, k) or np.shape(c0) != (n_q,):
            raise ValueError(f"case_neighbours: merge_into must hold arrays of shape ({n_q}, {k}), ({n_q}, {k}) and ({n_q},)")
        dist2 = torch.from_numpy(np.ascontiguousarray(d0, dtype=np.float64)).to(device)
        index = torch.from_numpy(np.ascontiguousarray(i0, dtype=np.int32)).to(device)
        count = torch.from_numpy(np.ascontiguousarray(c0, dtype=np.int32)).to(device)
    if n_q == 0:
        return np.zeros((0, k), dtype=np.float64), np.zeros((0, k), dtype=np.int32), np.zeros(0, dtype=np.int32)
    lib = _lib.load()
    (ws, need) = _workspace(device, lib.cae_case_neighbours_workspace_bytes, n_q, n_r, k)
    with _stream(device) as stream:
        check(lib.cae_case_neighbours(q.data_ptr(), n_q, dim, r.data_ptr() if n_r else None, n_r, dim, dim, k, ref_base, self_offset,
                                      0 if merge_into is None else 1, dist2.data_ptr(), index.data_ptr(), count.data_ptr(),
                                      ws.data_ptr(), need, stream))
        return dist2.cpu().numpy(), index.cpu().numpy(), count.cpu().numpy()


def upsample(low, out_shape, mode="bicubic", device=None):
    """Channel 0 of low (N, C, h, w) interpolated to out_shape = (H, W) as case_baseline does it: an (N, H, W) float64 numpy
    array, NaN where a tap is not finite (the field output of cae_case_baseline against a target of zeros)."""
    device = _case_device(device, low)
    op = device_operand(low, device)
    if len(op.shape) != 4:
        raise ValueError(f"upsample: an (N, C, h, w) array expected, got {tuple(op.shape)}")
    (h, w) = (int(out_shape[0]), int(out_shape[1]))
    if min(h, w) < 1:
        raise ValueError(f"upsample: an output of at least one pixel expected, got {h} x {w}")
    zeros = torch.zeros((int(op.shape[0]), 1, h, w), dtype=torch.float32, device=device)
    return case_baseline(op, None, zeros, mode=mode, field=True, device=device)[1]


def ensemble_verify(draws, actual, vmin, vmax, layout="case", device=None):
    """cae_ensemble_verify (include/cae_hip.h) on the K draws of every case at once: draws is a float32 numpy array or CUDA
    tensor (N, K, H, W) or (N, K, C, H, W) for layout "case", (K, N, H, W) or (K, N, C, H, W) for layout "draw" - the
    normalised decoder output, channel 0 is verified - and actual an (N, C, H, W) target in physical units as case_measures
    takes it.  The members are vmin + y * (vmax - vmin).  Returns (case_sums (N, 5) float64 {n, S A, S B, S (mbar - a)^2,
    S s^2}, rank_counts (K + 2,) int64); utils/ensemble_scores.scores_from_sums turns them into the scores."""
    if layout not in ("case", "draw"):
        raise ValueError(f"ensemble_verify: layout must be 'case' or 'draw', got {layout!r}")
    device = _case_device(device, draws, actual)
    if not isinstance(draws, torch.Tensor):
        draws = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.float32))
    if draws.dtype != torch.float32 or draws.dim() not in (4, 5):
        raise ValueError(f"ensemble_verify: float32 draws of 4 or 5 dimensions expected, got {draws.dtype} {tuple(draws.shape)}")
    y = draws.to(device).contiguous()
    a = device_operand(actual, device)
    (n, k) = (int(y.shape[0]), int(y.shape[1])) if layout == "case" else (int(y.shape[1]), int(y.shape[0]))
    if len(a.shape) != 4 or a.shape[0] != n or tuple(a.shape[2:]) != tuple(y.shape[-2:]):
        raise ValueError(f"ensemble_verify: draws {tuple(y.shape)} ({layout} major) and target {tuple(a.shape)} do not match")
    if not 2 <= k <= 64:
        raise ValueError(f"ensemble_verify: 2 to 64 draws expected, got {k}")
    plane = int(y.shape[-2] * y.shape[-1])
    field = plane * (int(y.shape[2]) if y.dim() == 5 else 1)
    (case_stride, draw_stride) = (k * field, field) if layout == "case" else (field, n * field)
    sums = torch.zeros((n, 5), dtype=torch.float64, device=device)
    ranks = torch.zeros(k + 2, dtype=torch.int64, device=device)
    if n and plane:
        lib = _lib.load()
        (ws, need) = _workspace(device, lib.cae_ensemble_verify_workspace_bytes, n, plane, k)
        with _stream(device) as stream:
            check(lib.cae_ensemble_verify(y.data_ptr(), case_stride, draw_stride, *a.args(), n, plane, k, float(vmin),
                                          float(vmax) - float(vmin), sums.data_ptr(), ranks.data_ptr(), ws.data_ptr(), need, stream))
    return sums.cpu().numpy(), ranks.cpu().numpy()


def _case_pair(name, arr, sub, device):
    """(device, source, subtracted operand or None, N, H, W) of case_range / render_cases: _pair with texts of its own"""
    device = _case_device(device, arr, sub)
    src = device_operand(arr, device)
    other = device_operand(sub, device) if sub is not None else None
    shape = src.shape
    if len(shape) != 4:
        raise ValueError(f"{name}: an (N, C, H, W) array expected, got {tuple(shape)}")
    if other is not None and (len(other.shape) != 4 or other.shape[0] != shape[0] or tuple(other.shape[2:]) != tuple(shape[2:])):
        raise ValueError(f"{name}: {tuple(shape)} and the subtracted {tuple(other.shape)} do not match")
    return device, src, other, int(shape[0]), int(shape[2]), int(shape[3])


def case_range(arr, sub=None, device=None):
    """(min, max, count) of the finite values of channel 0 of arr (N, C, H, W), or of arr - sub formed in fp64: what
    np.nanmin / np.nanmax of the fp64 copy give where nothing is infinite, in one streaming pass of cae_case_range over
    the array as stored.  Operands as case_measures takes them.  (inf, -inf, 0) when no value is finite."""
    (device, src, other, n, h, w) = _case_pair("case_range", arr, sub, device)
    if n * h * w == 0:
        return float("inf"), float("-inf"), 0
    lib = _lib.load()
    (ws, need) = _workspace(device, lib.cae_case_range_workspace_bytes, n, h * w, least=0)
    out = torch.empty(3, dtype=torch.float64, device=device)
    with _stream(device) as stream:
        check(lib.cae_case_range(*src.args(), *_args(other), n, h * w, out.data_ptr(), ws.data_ptr(), need, stream))
        (lo, hi, count) = out.cpu().tolist()
    return lo, hi, int(count)


def render_cases(arr, lo, hi, cases=None, sub=None, flip_y=False, device=None):
    """Channel 0 of the selected cases of arr (N, C, H, W), or of arr - sub in fp64, as palette indices in PNG scanline
    form (cae_render_cases, include/cae_hip.h): a (k, H, W + 1) uint8 numpy array whose rows start with the filter byte 0.
    cases: case indices in any order, repeats allowed (None: all).  Rendered in groups of cases, so that at most about
    _RENDER_BYTES of output are on the device and in pinned host memory at a time."""
    (device, src, other, n, h, w) = _case_pair("render_cases", arr, sub, device)
    sel = np.arange(n, dtype=np.int32) if cases is None else np.asarray(cases, dtype=np.int64).reshape(-1)
    if sel.size and (sel.min() < 0 or sel.max() >= n):
        raise IndexError(f"render_cases: case indices must lie in [0, {n})")
    result = np.empty((sel.size, h, w + 1), dtype=np.uint8)
    if result.size == 0:
        return result
    if w == 0:
        result[:] = 0
        return result
    lib = _lib.load()
    size = h * (w + 1)
    group = max(1, min(sel.size, _RENDER_BYTES // size))
    sel_dev = torch.from_numpy(sel.astype(np.int32)).to(device)
    out = torch.empty(group * size, dtype=torch.uint8, device=device)
    stage = torch.empty(group * size, dtype=torch.uint8).pin_memory()
    flat = result.reshape(-1)
    with _stream(device) as stream:
        for k0 in range(0, sel.size, group):
            k = min(group, sel.size - k0)
            check(lib.cae_render_cases(*src.args(), *_args(other), sel_dev.data_ptr() + 4 * k0, k, n, h, w, float(lo), float(hi),
                                       1 if flip_y else 0, out.data_ptr(), stream))
            stage[:k * size].copy_(out[:k * size], non_blocking=False)
            flat[k0 * size:(k0 + k) * size] = stage.numpy()[:k * size]
    return result
