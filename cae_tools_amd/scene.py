"""A box model applied to a whole scene (cae_scene_gather, cae_scene_blend; include/cae_hip.h): the scene is cut into the
model's boxes on the GPU, the boxes are scored by a callable, and the scores are blended back.  No engine needed."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import CaeError, check
from .case_ops import device_operands

_SCENE_PRED_BYTES = 256 << 20       # of fp32 tile predictions scored per chunk of a scene


class ScenePlan(namedtuple("ScenePlan", "Y X h w H W sy sx oy ox ys xs")):
    """The tiling of a (Y, X) scene by a model's boxes (scene_plan): pure Python, nothing here needs a GPU.
    ys / xs are the tile origins in low-resolution pixels; tiles are numbered (k_y, k_x) row-major within a time step."""

    __slots__ = ()

    n_y = property(lambda self: len(self.ys))
    n_x = property(lambda self: len(self.xs))
    n_tile = property(lambda self: len(self.ys) * len(self.xs))
    out_shape = property(lambda self: (self.Y * self.sy, self.X * self.sx))

    def rows_done(self, k1):
        """the output rows [0, rows_done) that no tile row k >= k1 touches: complete once the tile rows below k1 are in"""
        return self.ys[k1] * self.sy if k1 < self.n_y else self.Y * self.sy

    def first_row_over(self, row):
        """the first tile row that covers output row `row`"""
        return next(k for k, y in enumerate(self.ys) if (y + self.h) * self.sy > row)

    def geom(self):
        return _lib.SceneGeomC(self.Y, self.X, self.h, self.w, self.oy, self.ox, self.sy, self.sx)


def _origins(extent, box, overlap):
    stride = box - overlap
    n = 1 + -(-(extent - box) // stride)
    return tuple(min(k * stride, extent - box) for k in range(n))


def scene_plan(Y, X, box, overlap=None):
    """How a (Y, X) scene of low-resolution pixels is cut into a model's boxes.  box = (input shape, output shape), each
    (channels, rows, columns) or (rows, columns); overlap = None for (h // 4, w // 4), one number for both axes, or (oy, ox)
    in low-resolution pixels.  Along y the stride is h - oy and the origins are min(k * stride, Y - h) for
    k = 0 .. ceil((Y - h) / stride): every tile is a full box, the last one shifted inward.  ValueError for output sides
    that are no whole multiple of the input's, an overlap outside [0, box), a scene smaller than a box, or 4 H W >= 2^29."""
    (in_shape, out_shape) = (tuple(int(v) for v in box[0]), tuple(int(v) for v in box[1]))
    ((h, w), (H, W)) = (in_shape[-2:], out_shape[-2:])
    if min(h, w, H, W) < 1 or H % h or W % w:
        raise ValueError(f"scene_plan: the output box {out_shape} must be a whole multiple of the input box {in_shape} along y and x")
    if overlap is None:
        overlap = (h // 4, w // 4)
    elif np.ndim(overlap) == 0:
        overlap = (overlap, overlap)
    (oy, ox) = (int(v) for v in overlap)
    if not (0 <= oy < h and 0 <= ox < w):
        raise ValueError(f"scene_plan: the overlap ({oy}, {ox}) must be at least 0 and below the input box ({h}, {w})")
    (Y, X) = (int(Y), int(X))
    if Y < h or X < w:
        raise ValueError(f"scene_plan: a scene of {Y} x {X} pixels is smaller than the input box {h} x {w}")
    if 4 * H * W >= 1 << 29:
        raise ValueError(f"scene_plan: an output box of {H} x {W} is too large (4 H W must stay below 2^29)")
    return ScenePlan(Y, X, h, w, H, W, H // h, W // w, oy, ox, _origins(Y, h, oy), _origins(X, w, ox))


def _scene_operands(variables, plan, device):
    """(device, the scene's variables on it), each (time, channel, Y, X)"""
    (device, ops) = device_operands(variables, device)
    for op in ops:
        if len(op.shape) != 4 or tuple(op.shape[2:]) != (plan.Y, plan.X):
            raise ValueError(f"scene variables must be (time, channel, {plan.Y}, {plan.X}); got {tuple(op.shape)}")
    return device, ops


def scene_tiles(variables, plan, norms, t0=0, n_t=None, ky0=0, n_ky=None, normalise=True, device=None):
    """The boxes of a scene as the model's input batch (cae_scene_gather).  variables: the scene's input variables, each
    (T, Cv, Y, X) as case_measures takes operands (NetCDF-3 slabs go up as stored); norms: (vmin, vmax) per variable.
    Returns (x, invalid) for the time steps t0 .. t0 + n_t - 1 and the tile rows ky0 .. ky0 + n_ky - 1: x the normalised fp32
    CUDA batch (n_t * n_ky * n_x, C, h, w), tiles in (time, k_y, k_x) order, channels in variable order; invalid an int32
    CUDA tensor, 1 for a tile whose box holds a value that is not finite."""
    (device, ops) = _scene_operands(variables, plan, device)
    T = int(ops[0].shape[0])
    if any(int(op.shape[0]) != T for op in ops):
        raise ValueError(f"scene variables differ in their first dimension: {[tuple(op.shape) for op in ops]}")
    n_t = T - t0 if n_t is None else int(n_t)
    n_ky = plan.n_y - ky0 if n_ky is None else int(n_ky)
    if not (0 <= t0 and 0 <= n_t and t0 + n_t <= T and 0 <= ky0 and 0 <= n_ky and ky0 + n_ky <= plan.n_y):
        raise ValueError(f"scene_tiles: time steps {t0}..{t0 + n_t} of {T}, tile rows {ky0}..{ky0 + n_ky} of {plan.n_y}")
    channels = int(sum(op.shape[1] for op in ops))
    n_tile = n_t * n_ky * plan.n_x
    x = torch.empty((n_tile, channels, plan.h, plan.w), dtype=torch.float32, device=device)
    invalid = torch.zeros(n_tile, dtype=torch.int32, device=device)
    if n_tile == 0:
        return x, invalid
    lib = _lib.load()
    geom = plan.geom()
    off = 0
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        for (op, (vmin, vmax)) in zip(ops, norms):
            rng = float(vmax) - float(vmin)
            check(lib.cae_scene_gather(C.byref(geom), op.tensor.data_ptr(), op.kind, T, int(op.shape[1]), int(t0), n_t, int(ky0), n_ky,
                                       x.data_ptr(), channels, off, C.c_float(float(np.float32(vmin))),
                                       C.c_float(float(np.float32(rng))), 1 if normalise else 0, invalid.data_ptr(), stream))
            off += int(op.shape[1])
    return x, invalid


def scene_blend(pred, invalid, plan, vmin, vmax, n_t=1, k0=0, carry=None, rows=None, out=None, nan_pixels=None):
    """Scored boxes folded back into the scene (cae_scene_blend).  pred: fp32 CUDA (n_t * n_k * n_x, Co, H, W), the tile rows
    k0 .. k0 + n_k - 1 of n_t time steps in scene_tiles' order, with their invalid flags; carry: None or (pred, invalid, k0) of
    earlier tile rows that the output rows still need.  rows = (row0, row1): the output rows to write; None: the rows the
    tile rows complete, plan.rows_done(k0) .. plan.rows_done(k0 + n_k).  out: float64 CUDA (n_t, Co, Y sy, X sx) to write
    into (None: a new one, NaN outside the rows); nan_pixels: int64 CUDA (n_t) to add the pixels without a valid tile to.
    Per pixel (S w p) / S w over the valid covering tiles in ascending tile number, then vmin + v * (vmax - vmin).
    Returns (out, nan_pixels)."""
    device = pred.device
    pred = pred.contiguous()
    (Co, n_t) = (int(pred.shape[1]), int(n_t))
    if pred.dtype != torch.float32 or tuple(pred.shape[2:]) != (plan.H, plan.W) or n_t < 1 or int(pred.shape[0]) % (n_t * plan.n_x):
        raise ValueError(f"scene_blend: fp32 predictions (n_t * n_k * {plan.n_x}, Co, {plan.H}, {plan.W}) expected, got "
                         f"{tuple(pred.shape)} {pred.dtype} for {n_t} time steps")
    n_k = int(pred.shape[0]) // (n_t * plan.n_x)
    if invalid.dtype != torch.int32 or invalid.numel() != pred.shape[0] or invalid.device != device:
        raise ValueError("scene_blend: one int32 invalid flag per tile expected, on the predictions' device")
    (cp, ci, ck0, cnk) = (None, None, 0, 0)
    if carry is not None:
        (cp, ci, ck0) = (carry[0].contiguous(), carry[1].contiguous(), int(carry[2]))
        if cp.dtype != torch.float32 or tuple(cp.shape[1:]) != tuple(pred.shape[1:]) or int(cp.shape[0]) % (n_t * plan.n_x) or \
                ci.dtype != torch.int32 or ci.numel() != cp.shape[0]:
            raise ValueError("scene_blend: the carried tile rows must be laid out as the new ones")
        cnk = int(cp.shape[0]) // (n_t * plan.n_x)
    (Ys, Xs) = plan.out_shape
    (row0, row1) = (plan.rows_done(k0) if k0 else 0, plan.rows_done(k0 + n_k)) if rows is None else (int(rows[0]), int(rows[1]))
    if out is None:
        out = torch.full((n_t, Co, Ys, Xs), math.nan, dtype=torch.float64, device=device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n_t, Co, Ys, Xs) or out.device != device or \
            not out[0].is_contiguous():
        raise ValueError(f"scene_blend: out must be a float64 tensor ({n_t}, {Co}, {Ys}, {Xs}) on the predictions' device")
    if nan_pixels is None:
        nan_pixels = torch.zeros(n_t, dtype=torch.int64, device=device)
    lib = _lib.load()
    geom = plan.geom()
    with torch.cuda.device(device):
        check(lib.cae_scene_blend(C.byref(geom), pred.data_ptr(), invalid.data_ptr(), int(k0), n_k,
                                  cp.data_ptr() if cnk else None, ci.data_ptr() if cnk else None, ck0, cnk, n_t, Co, row0, row1,
                                  float(vmin), float(vmax) - float(vmin), out.data_ptr(), int(out.stride(0)), nan_pixels.data_ptr(),
                                  torch.cuda.current_stream(device).cuda_stream))
    return out, nan_pixels


def scene_chunks(plan, T, c_out, tile_rows=None):
    """The (t0, n_t, k0, n_k) pieces scene_apply scores one after the other: whole tile rows, tile_rows of them at a time.
    None: as many as keep a piece's fp32 predictions within _SCENE_PRED_BYTES, and whole time steps, several at a time,
    once a time step fits.  Pure Python."""
    row_bytes = plan.n_x * c_out * plan.H * plan.W * 4
    n_t = 1
    if tile_rows is None:
        tile_rows = max(1, min(plan.n_y, _SCENE_PRED_BYTES // row_bytes))
        if tile_rows == plan.n_y:
            n_t = max(1, min(T, _SCENE_PRED_BYTES // (row_bytes * plan.n_y), 65535 // c_out))
    tile_rows = int(tile_rows)
    if tile_rows < 1:
        raise ValueError(f"scene_apply: tile_rows must be at least 1, got {tile_rows}")
    return [(t0, min(n_t, T - t0), k0, min(tile_rows, plan.n_y - k0))
            for t0 in range(0, T, n_t) for k0 in range(0, plan.n_y, tile_rows)]


def scene_apply(variables, norms, plan, score, c_out, vmin, vmax, tile_rows=None, normalise=True, device=None):
    """A box model over a whole scene: scene_tiles -> score -> scene_blend in pieces of whole tile rows (scene_chunks), so that
    the tile predictions of a large scene are never all resident.  score: callable, the fp32 CUDA batch (n, C, h, w) -> the fp32
    CUDA scores (n, c_out, H, W).  The tile rows a later piece's output rows still need are carried (the previous piece's
    scores are kept, not copied), so the result does not depend on tile_rows, bit for bit.
    Returns (out float64 CUDA (T, c_out, Y sy, X sx), invalid_tiles (T,) int64 numpy, nan_pixels (T,) int64 numpy)."""
    (device, ops) = _scene_operands(variables, plan, device)
    T = int(ops[0].shape[0])
    c_out = int(c_out)
    out = torch.empty((T, c_out) + plan.out_shape, dtype=torch.float64, device=device)
    invalid_tiles = torch.zeros(T, dtype=torch.int64, device=device)
    nan_pixels = torch.zeros(T, dtype=torch.int64, device=device)
    carry = None
    for (t0, n_t, k0, n_k) in scene_chunks(plan, T, c_out, tile_rows):
        (x, inv) = scene_tiles(ops, plan, norms, t0, n_t, k0, n_k, normalise=normalise, device=device)
        y = score(x)
        if y.dtype != torch.float32 or tuple(y.shape) != (int(x.shape[0]), c_out, plan.H, plan.W):
            raise CaeError(f"scene_apply: the model returned {tuple(y.shape)} {y.dtype} for {tuple(x.shape)}; fp32 "
                           f"({int(x.shape[0])}, {c_out}, {plan.H}, {plan.W}) expected")
        invalid_tiles[t0:t0 + n_t] += inv.view(n_t, -1).sum(dim=1)
        scene_blend(y, inv, plan, vmin, vmax, n_t=n_t, k0=k0, carry=carry, out=out[t0:t0 + n_t], nan_pixels=nan_pixels[t0:t0 + n_t])
        k1 = k0 + n_k
        if k1 == plan.n_y:
            carry = None
            continue
        # what the next piece's output rows need of the tile rows seen so far (a piece of part of a time step has n_t == 1)
        keep = plan.first_row_over(plan.rows_done(k1))
        if keep >= k0:
            carry = (y[(keep - k0) * plan.n_x:], inv[(keep - k0) * plan.n_x:], keep)
        else:                   # pieces thinner than the cover: the older rows are copied on
            skip = (keep - carry[2]) * plan.n_x
            carry = (torch.cat([carry[0][skip:], y]), torch.cat([carry[1][skip:], inv]), keep)
    return out, invalid_tiles.cpu().numpy(), nan_pixels.cpu().numpy()
