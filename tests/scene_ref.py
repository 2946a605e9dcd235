"""Scene apply restated in numpy (DESIGN.md §9 'scene apply'; include/cae_hip.h, cae_scene_gather / cae_scene_blend): the
tiling, the integer tent weights, the validity of a tile and the blended, denormalised value per pixel in np.longdouble,
with the bound the fold order gives.  Nothing here imports the package: the tests compare the package against it.

A model maps an input box (h, w) to an output box (H, W), sy = H / h, sx = W / w.  With the overlap (oy, ox) the stride
along y is s = h - oy and the origins are y_k = min(k s, Y - h), k = 0 .. ceil((Y - h) / s); along x likewise.  On the
output grid, row r of a tile has m = min(r, H - 1 - r) and w_y(r) = min(2 m + 1, 2 oy sy), or 1 when oy = 0; w = w_y w_x.
    v = (S_t w_t p_t) / S_t w_t   over the valid covering tiles t in ascending tile number,   out = vmin + v * range
and NaN where no valid tile covers the pixel.  A tile is invalid when a value of its input box is not finite as fp32.

Bound: w p is exact in fp64 (w < 2^29, p fp32); the m - 1 adds of the numerator each err by at most 2^-53 of a partial sum
<= S w|p|; the division, the product with range and the sum with vmin round once each.  To first order
    |got - want| <= (m + 2) 2^-53 (|vmin| + |range| S w|p| / S w),    m = the valid covering tiles of the pixel."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def origins(extent, box, overlap):
    stride = box - overlap
    n = 1 + -(-(extent - box) // stride)
    return [min(k * stride, extent - box) for k in range(n)]


def tent(side, cap):
    """the integer weights along one axis of an output box: min(2 m + 1, 2 cap), or ones when cap == 0"""
    r = np.arange(side)
    m = np.minimum(r, side - 1 - r)
    return np.minimum(2 * m + 1, 2 * cap).astype(np.int64) if cap > 0 else np.ones(side, dtype=np.int64)


def cover(extent, box, overlap):
    """how many tiles cover each pixel along one axis"""
    c = np.zeros(extent, dtype=np.int64)
    for o in origins(extent, box, overlap):
        c[o:o + box] += 1
    return c


def boxes(var, h, w, oy, ox):
    """the boxes of a (T, Cv, Y, X) variable sliced on the host, in (time, k_y, k_x) order: (n_tile, Cv, h, w) as stored"""
    (T, _, Y, X) = var.shape
    return np.stack([var[t, :, y:y + h, x:x + w] for t in range(T) for y in origins(Y, h, oy) for x in origins(X, w, ox)])


def invalid_tiles(variables, h, w, oy, ox):
    """1 for a tile whose box holds, in any variable and channel, a value that is not finite as fp32"""
    bad = None
    for var in variables:
        with np.errstate(over="ignore"):
            b = ~np.isfinite(boxes(np.asarray(var), h, w, oy, ox).astype(np.float32))
        b = b.reshape(b.shape[0], -1).any(axis=1)
        bad = b if bad is None else (bad | b)
    return bad.astype(np.int32)


class Reference:
    """pred: fp32 (T * n_y * n_x, Co, H, W) in (time, k_y, k_x) order; invalid: (T * n_y * n_x,) flags.  want is the blended scene
    (T, Co, Y sy, X sx) in np.longdouble, bound the per-pixel bound, valid the count of valid covering tiles (T, Y sy, X sx)."""

    def __init__(self, pred, invalid, Y, X, h, w, oy, ox, vmin, vmax):
        pred = np.asarray(pred)
        assert pred.dtype == np.float32
        (Co, H, W) = pred.shape[1:]
        (sy, sx) = (H // h, W // w)
        assert (sy * h, sx * w) == (H, W)
        (ys, xs) = (origins(Y, h, oy), origins(X, w, ox))
        n_tile = len(ys) * len(xs)
        T = pred.shape[0] // n_tile
        assert pred.shape[0] == T * n_tile and len(invalid) == T * n_tile
        rng = float(vmax) - float(vmin)         # the fp64 range the kernel is given
        wgt = np.outer(tent(H, oy * sy), tent(W, ox * sx))
        num = np.zeros((T, Co, Y * sy, X * sx), dtype=LD)
        mag = np.zeros_like(num)
        den = np.zeros((T, Y * sy, X * sx), dtype=np.int64)
        valid = np.zeros_like(den)
        tile = 0
        for t in range(T):
            for y in ys:
                for x in xs:
                    if not invalid[tile]:
                        (r, c) = (slice(y * sy, y * sy + H), slice(x * sx, x * sx + W))
                        p = pred[tile].astype(LD)
                        num[t, :, r, c] += wgt * p
                        mag[t, :, r, c] += wgt * np.abs(p)
                        den[t, r, c] += wgt
                        valid[t, r, c] += 1
                    tile += 1
        hole = den == 0
        d = np.where(hole, 1, den).astype(LD)[:, None]
        self.want = np.where(hole[:, None], LD(np.nan), LD(vmin) + (num / d) * LD(rng))
        self.bound = (valid[:, None] + 2) * U * (abs(float(vmin)) + abs(rng) * (mag / d).astype(np.float64))
        (self.valid, self.hole) = (valid, hole)
        self.nan_pixels = hole.reshape(T, -1).sum(axis=1)
        self.invalid_tiles = np.asarray(invalid).reshape(T, -1).sum(axis=1)

    def ratio(self, got):
        """the largest |got - want| / bound over the pixels a valid tile covers; the holes must be NaN"""
        got = np.asarray(got)
        assert got.dtype == np.float64 and got.shape == self.want.shape, (got.dtype, got.shape, self.want.shape)
        hole = np.broadcast_to(self.hole[:, None], got.shape)
        assert np.isnan(got[hole]).all() and not np.isnan(got[~hole]).any()
        if hole.all():
            return 0.0
        err = np.abs(got[~hole].astype(LD) - self.want[~hole]).astype(np.float64)
        return float(np.max(err / self.bound[~hole]))

    def check(self, got, what):
        r = self.ratio(got)
        print(f"scene blend {what}: max |got - want| / bound = {r:.3e}")
        assert r <= 1.0, (what, r)
        return r


def pixel_by_pixel(pred, invalid, Y, X, h, w, oy, ox, vmin, vmax):
    """the definition as three plain loops (time, pixel, tile), np.longdouble: the restatement Reference is checked against"""
    pred = np.asarray(pred)
    (Co, H, W) = pred.shape[1:]
    (sy, sx) = (H // h, W // w)
    tiles = [(y * sy, x * sx) for y in origins(Y, h, oy) for x in origins(X, w, ox)]
    T = pred.shape[0] // len(tiles)
    (wy, wx) = (tent(H, oy * sy), tent(W, ox * sx))
    rng = float(vmax) - float(vmin)
    out = np.full((T, Co, Y * sy, X * sx), np.nan, dtype=LD)
    for t in range(T):
        for c in range(Co):
            for r in range(Y * sy):
                for q in range(X * sx):
                    (num, den) = (LD(0), 0)
                    for (k, (ty, tx)) in enumerate(tiles):
                        if ty <= r < ty + H and tx <= q < tx + W and not invalid[t * len(tiles) + k]:
                            wt = int(wy[r - ty]) * int(wx[q - tx])
                            num += LD(wt) * LD(pred[t * len(tiles) + k, c, r - ty, q - tx])
                            den += wt
                    if den:
                        out[t, c, r, q] = LD(vmin) + (num / LD(den)) * LD(rng)
    return out
