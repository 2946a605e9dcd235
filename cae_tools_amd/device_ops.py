"""The loader's kernels of libcae_hip (include/cae_hip.h) as functions on torch CUDA tensors, no engine needed: scan,
normalise and pack, permutation, denormalise, the residual target (scan, pack, restore), metric sums, upload."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import CaeError, check


def scan_f32(x):
    """(nan_count, nanmin, nanmax) of an fp32 CUDA tensor as python numbers (ds_dataset.py:43-58)"""
    lib = _lib.load()
    x = x.contiguous()
    out = (C.c_double * 3)()
    torch.cuda.synchronize(x.device)
    check(lib.cae_scan_f32(x.data_ptr(), x.numel(), None, out))
    return int(out[0]), float(out[1]), float(out[2])


def normalise_pack(src, dst, c_off, vmin, vmax, enable=True, dst_rows=None):
    """dst[row(i), c_off:c_off+Cv] = normalise(src[i]) on the device (ds_dataset.py:99-113,137-147).
    The range is formed in fp64 from python floats and rounded to fp32, as numpy does.
    dst_rows: int32 CUDA tensor, row(i) = dst_rows[i] (inverse_permutation() of a frozen sample order: the samples land in
    batch order, which is the DataLoader + collate stacking of conv_ae_model.py:291-292,315-325); None: row(i) = i."""
    lib = _lib.load()
    (n, c_src) = (int(src.shape[0]), int(src.shape[1]))
    hw = int(np.prod(src.shape[2:]))
    rng = float(vmax) - float(vmin)
    if dst_rows is not None:
        if dst_rows.dtype != torch.int32 or dst_rows.device != src.device or dst_rows.numel() != n or int(dst.shape[0]) != n:
            raise CaeError("normalise_pack: dst_rows must be an int32 tensor of one entry per sample on the data's device")
    with torch.cuda.device(src.device):
        check(lib.cae_normalise_pack_rows(src.data_ptr(), n, c_src, hw, dst.data_ptr(), int(dst.shape[1]), int(c_off),
                                          C.c_float(float(np.float32(vmin))), C.c_float(float(np.float32(rng))),
                                          1 if enable else 0, dst_rows.data_ptr() if dst_rows is not None else None,
                                          torch.cuda.current_stream(src.device).cuda_stream))


def inverse_permutation(order, device):
    """int32 CUDA tensor inv with inv[order[i]] = i (cae_invert_permutation): where each sample goes when the data set is
    laid out in the frozen order `order` (host sequence of sample indices, every index exactly once)."""
    lib = _lib.load()
    order = np.ascontiguousarray(np.asarray(order, dtype=np.int32))
    n = int(order.size)
    if n < 1 or not np.array_equal(np.sort(order), np.arange(n, dtype=np.int32)):
        raise CaeError("inverse_permutation: `order` must hold every sample index 0..n-1 exactly once")
    perm = torch.from_numpy(order).to(device)
    inv = torch.empty(n, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(lib.cae_invert_permutation(perm.data_ptr(), n, inv.data_ptr(), torch.cuda.current_stream(device).cuda_stream))
    torch.cuda.synchronize(device)
    return inv


def denormalise_f64(y, vmin, vmax):
    """float64 CUDA tensor min + y*(max-min) (ds_dataset.py:131-135 on base_model.py:123's fp64 array)"""
    lib = _lib.load()
    y = y.contiguous()
    out = torch.empty(y.shape, dtype=torch.float64, device=y.device)
    check(lib.cae_denormalise_f64(y.data_ptr(), y.numel(), float(vmin), float(vmax) - float(vmin), out.data_ptr(),
                                  torch.cuda.current_stream(y.device).cuda_stream))
    return out


def _residual_operands(name, low, other, mode):
    """(lib, low as a case operand, the fp32 tensor `other` contiguous, N, h, w, H, W, mode code) of a residual_* call:
    low (N, C, h, w) in any form case_ops.device_operand takes, other a float32 CUDA tensor (N, 1, H, W) or (N, H, W)"""
    from .case_ops import device_operand
    from .utils.baseline import MODES
    if mode not in MODES:
        raise ValueError(f"{name}: mode must be one of {', '.join(MODES)}, got {mode!r}")
    if not (isinstance(other, torch.Tensor) and other.is_cuda and other.dtype == torch.float32 and other.dim() in (3, 4)):
        raise CaeError(f"{name}: a float32 CUDA tensor (N, 1, H, W) expected beside the low-resolution variable")
    if other.dim() == 4 and int(other.shape[1]) != 1:
        raise ValueError(f"{name}: the residual is defined for an output of one channel, got {int(other.shape[1])}")
    lo = device_operand(low, other.device)
    if len(lo.shape) != 4 or int(lo.shape[0]) != int(other.shape[0]):
        raise ValueError(f"{name}: (N, C, h, w) beside (N, 1, H, W) expected, got {tuple(lo.shape)} and {tuple(other.shape)}")
    (h_in, w_in, h, w) = (int(lo.shape[2]), int(lo.shape[3]), int(other.shape[-2]), int(other.shape[-1]))
    if min(h_in, w_in, h, w) < 1:
        raise ValueError(f"{name}: planes of at least one pixel expected, got {h_in} x {w_in} and {h} x {w}")
    return _lib.load(), lo, other.contiguous(), int(other.shape[0]), h_in, w_in, h, w, MODES[mode]


def residual_scan(low, target, mode="bicubic"):
    """(k, rmin, rmax) of r = double(target) - b as python numbers (cae_residual_scan, include/cae_hip.h): b is channel 0 of
    low interpolated to the target's grid, the field of case_ops.upsample, formed in registers; k counts the r that are not
    finite, rmin and rmax are the exact fp64 minimum and maximum of the others (+inf, -inf without one)."""
    (lib, lo, t, n, h_in, w_in, h, w, code) = _residual_operands("residual_scan", low, target, mode)
    out = (C.c_double * 3)()
    need = int(lib.cae_residual_scan_workspace_bytes(n, h, w))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=t.device)
    with torch.cuda.device(t.device):
        check(lib.cae_residual_scan(*lo.args(), h_in, w_in, t.data_ptr(), n, h, w, code, ws.data_ptr(), need,
                                    torch.cuda.current_stream(t.device).cuda_stream, out))
    return int(out[0]), float(out[1]), float(out[2])


def residual_pack(low, target, dst, rmin, rmax, mode="bicubic", enable=True, dst_rows=None):
    """dst[row(i)] = float32((r - rmin) / (rmax - rmin)) on the device (cae_residual_pack_rows): the residual target a
    model trains on, 0 at span 0, float32(r) when not enabled, NaN where r is not finite.  dst: a contiguous float32 CUDA
    tensor shaped like target; dst_rows as normalise_pack takes it.  The span is formed in fp64 from python floats."""
    (lib, lo, t, n, h_in, w_in, h, w, code) = _residual_operands("residual_pack", low, target, mode)
    if dst.dtype != torch.float32 or dst.device != t.device or tuple(dst.shape) != tuple(target.shape) or not dst.is_contiguous():
        raise CaeError("residual_pack: dst must be a contiguous float32 tensor shaped like the target on its device")
    if dst_rows is not None:
        if dst_rows.dtype != torch.int32 or dst_rows.device != t.device or dst_rows.numel() != n:
            raise CaeError("residual_pack: dst_rows must be an int32 tensor of one entry per sample on the data's device")
    with torch.cuda.device(t.device):      # (no case: a defined no-op of the entry point)
        check(lib.cae_residual_pack_rows(*lo.args(), h_in, w_in, t.data_ptr(), n, h, w, code, float(rmin),
                                         float(rmax) - float(rmin), 1 if enable else 0,
                                         dst_rows.data_ptr() if dst_rows is not None else None, dst.data_ptr(),
                                         torch.cuda.current_stream(t.device).cuda_stream))


def residual_restore(low, y, rmin, rmax, mode="bicubic", enable=True):
    """float64 CUDA tensor b + (rmin + double(y) * (rmax - rmin)), shaped like the scores y (cae_residual_restore_f64): the
    prediction of a residual model, b + double(y) when not enabled, NaN where b or y is."""
    (lib, lo, yc, n, h_in, w_in, h, w, code) = _residual_operands("residual_restore", low, y, mode)
    out = torch.empty(yc.shape, dtype=torch.float64, device=yc.device)
    with torch.cuda.device(yc.device):
        check(lib.cae_residual_restore_f64(*lo.args(), h_in, w_in, yc.data_ptr(), n, h, w, code, float(rmin),
                                           float(rmax) - float(rmin), 1 if enable else 0, out.data_ptr(),
                                           torch.cuda.current_stream(yc.device).cuda_stream))
    return out


def metric_sums(y, actual, mask, vmin, vmax):
    """cae_metric_sums: per-instance fp64 sums (n, 8) of the denormalised scores `vmin + y*(vmax-vmin)` against
    `actual` over the pixels where `mask` (same shape, or None = all) is non-zero.  CUDA fp32 tensors (n, ...)."""
    lib = _lib.load()
    y, actual = y.contiguous(), actual.contiguous()
    if y.shape != actual.shape:
        raise ValueError("The shapes of 'actual' and 'estimates' must match.")
    n = int(y.shape[0])
    elems = y.numel() // max(n, 1)
    if mask is not None:
        mask = mask.to(device=y.device, dtype=torch.float32).expand(y.shape).contiguous()
    out = torch.empty((n, 8), dtype=torch.float64, device=y.device)
    stream = torch.cuda.current_stream(y.device).cuda_stream
    for lo in range(0, n, 65535):
        hi = min(n, lo + 65535)
        check(lib.cae_metric_sums(y[lo:hi].data_ptr(), actual[lo:hi].data_ptr(),
                                  mask[lo:hi].data_ptr() if mask is not None else None, hi - lo, elems,
                                  float(vmin), float(vmax) - float(vmin), out[lo:hi].data_ptr(), stream))
    return out


_STAGE_BYTES = 64 << 20


def _upload_raw(arr, device):
    """the bytes of a C-contiguous numpy array, unchanged, in a new uint8 CUDA tensor: copied through a pinned staging
    buffer in pieces of at most _STAGE_BYTES"""
    src = arr.reshape(-1).view(np.uint8)
    nbytes = src.size
    out = torch.empty(nbytes, dtype=torch.uint8, device=device)
    stage = torch.empty(min(nbytes, _STAGE_BYTES), dtype=torch.uint8).pin_memory()
    stage_np = stage.numpy()
    for lo in range(0, nbytes, _STAGE_BYTES):
        hi = min(nbytes, lo + _STAGE_BYTES)
        stage_np[:hi - lo] = src[lo:hi]
        out[lo:hi].copy_(stage[:hi - lo], non_blocking=False)
    return out


def _is_big_endian_slab(arr, dtype):
    return arr.dtype == np.dtype(dtype) and arr.dtype.byteorder == ">" and arr.flags.c_contiguous and arr.size > 0


def upload_f32(arr, device):
    """numpy (N,...) array -> fp32 CUDA tensor.  A C-contiguous big-endian float32 array (a NetCDF-3 slab, usually a
    view of the file mapping) is copied as raw bytes through a pinned staging buffer and byte-swapped on the GPU
    (cae_bswap32); anything else is converted by numpy first."""
    arr = np.asarray(arr)
    if not _is_big_endian_slab(arr, ">f4"):
        return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(device)
    lib = _lib.load()
    words = _upload_raw(arr, device).view(torch.int32)
    check(lib.cae_bswap32(words.data_ptr(), words.numel(), torch.cuda.current_stream(device).cuda_stream))
    return words.view(torch.float32).view(arr.shape)
