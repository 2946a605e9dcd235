"""Numpy restatements shared by test_skill_maps_cpu.py and test_pixel_sums_gpu.py: the nine per-pixel sums of
cae_pixel_sums (include/cae_hip.h) term by term, their exactly rounded sums with the derived error bound, the two-pass
skill maps, the range rule of the maps page and the palette index of cae_render_cases."""
import math
import struct
import zlib

import numpy as np

MAPS = ("count", "bias", "mae", "rmse", "correlation", "sd_ratio")


def channel0(x):
    return np.asarray(x)[:, 0].astype(np.float64)


def terms(p, a, shift):
    """(9, N, ...) float64: per case and pixel the nine terms {1, d, |d|, d^2, a', p', a'^2, p'^2, a'p'} of a pair, zeros
    where the two values are not both finite.  p, a: (N, ...) arrays, taken to fp64 first; shift: one number, or a
    (2, ...) array of per-pixel shifts for a and for p (cae_pixel_sums_about)."""
    p = np.asarray(p).astype(np.float64)
    a = np.asarray(a).astype(np.float64)
    (shift_a, shift_p) = (shift[0], shift[1]) if np.ndim(shift) else (shift, shift)
    pair = np.isfinite(p) & np.isfinite(a)
    p = np.where(pair, p, 0.0)
    a = np.where(pair, a, 0.0)
    d = p - a
    (sa, sp) = (a - shift_a, p - shift_p)
    t = np.stack([np.ones_like(d), d, np.abs(d), d * d, sa, sp, sa * sa, sp * sp, sa * sp])
    return np.where(pair[None], t, 0.0)


def chunked_sums(p, a, shift, chunk):
    """the sums as the kernel orders them: one running sum per chunk of `chunk` cases in case order, the chunks' partials
    added in chunk order"""
    t = terms(p, a, shift)
    total = np.zeros(t.shape[:1] + t.shape[2:])
    for c0 in range(0, t.shape[1], chunk):
        part = np.zeros_like(total)
        for c in range(c0, min(c0 + chunk, t.shape[1])):
            part = part + t[:, c]
        total = total + part
    return total


def fsum_sums(p, a, shift):
    """(want, bound), both (9, ...): every sum exactly rounded (math.fsum) and |got - want| <= 2 n 2^-53 S|term| with n
    the pixel's pairs: at most one rounding per product (a fused multiply-add may or may not keep it), n - 1 additions
    in any order, and the oracle's final rounding"""
    t = terms(p, a, shift)
    flat = t.reshape(9, t.shape[1], -1)
    want = np.array([[math.fsum(col) for col in flat[k].T.tolist()] for k in range(9)]).reshape(t.shape[:1] + t.shape[2:])
    bound = 2.0 * t[0].sum(axis=0) * 2.0 ** -53 * np.abs(t).sum(axis=1)
    return want, bound


def check_sums(got, p, a, shift):
    (want, bound) = fsum_sums(p, a, shift)
    got = np.asarray(got).reshape(want.shape)
    np.testing.assert_array_equal(got[0], want[0])
    err = np.abs(got - want)
    assert (err <= bound).all(), (float((err / np.maximum(bound, 1e-300)).max()), np.argwhere(err > bound)[:5])


def two_pass_maps(p, a):
    """the six maps per pixel by the textbook two-pass formulas over the pairs (isfinite on both), mean-centred; NaN where
    the definition has no value: n == 0, and for correlation / sd_ratio n < 2 or a variance that is exactly zero"""
    p = np.asarray(p).astype(np.float64)
    a = np.asarray(a).astype(np.float64)
    shape = p.shape[1:]
    (p, a) = (p.reshape(p.shape[0], -1), a.reshape(a.shape[0], -1))
    out = {m: np.full(p.shape[1], np.nan) for m in MAPS}
    for x in range(p.shape[1]):
        ok = np.isfinite(p[:, x]) & np.isfinite(a[:, x])
        (px, ax) = (p[ok, x], a[ok, x])
        n = int(ok.sum())
        out["count"][x] = n
        if n == 0:
            continue
        d = px - ax
        out["bias"][x] = d.mean()
        out["mae"][x] = np.abs(d).mean()
        out["rmse"][x] = math.sqrt((d * d).mean())
        if n < 2:
            continue
        (ca, cp) = (ax - ax.mean(), px - px.mean())
        (va, vp, cov) = ((ca * ca).sum(), (cp * cp).sum(), (ca * cp).sum())
        if va > 0.0:
            out["sd_ratio"][x] = math.sqrt(vp / va)
            if vp > 0.0:
                out["correlation"][x] = cov / math.sqrt(va * vp)
    return {m: v.reshape(shape) for (m, v) in out.items()}


def assert_maps_close(got, want, rtol=1e-12):
    for m in MAPS:
        (g, w) = (np.asarray(got[m]), np.asarray(want[m]))
        assert g.shape == w.shape, m
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=m)
        np.testing.assert_allclose(g, w, rtol=rtol, atol=0, err_msg=m)


def range_rule(name, partitions, n_case):
    """(lo, hi) of map `name` over the partitions' maps: count over [0, largest n_case], bias over +-max|bias|, every other
    map over its finite range, (0, 0) without a finite value"""
    if name == "count":
        return 0.0, float(n_case)
    v = np.concatenate([np.asarray(maps[name]).reshape(-1) for maps in partitions])
    v = v[np.isfinite(v)]
    if v.size == 0:
        return 0.0, 0.0
    if name == "bias":
        bound = float(np.abs(v).max())
        return -bound, bound
    return float(v.min()), float(v.max())


def np_scanlines(v, lo, hi, flip_y=False):
    """(H, W) values -> (H, W + 1) PNG scanlines of palette indices as cae_render_cases defines them: 0 for NaN, else
    1 + (int)(clamp((v - lo) / (hi - lo), 0, 1) * 254.0 + 0.5), the middle level for all when hi <= lo"""
    v = np.asarray(v, dtype=np.float64)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore", over="ignore"):
        if hi > lo:
            t = np.minimum(np.maximum((np.where(nan, lo, v) - lo) / (hi - lo), 0.0), 1.0)
        else:
            t = np.full(v.shape, 0.5)
        scaled = t * 254.0
        idx = np.where(nan, 0, 1 + (scaled + 0.5).astype(np.int64)).astype(np.uint8)
    if flip_y:
        idx = idx[::-1]
    out = np.zeros((idx.shape[0], idx.shape[1] + 1), dtype=np.uint8)
    out[:, 1:] = idx
    return out


def decode_png(data):
    """(width, height, scanline bytes) of an 8-bit palette PNG; every chunk's CRC is checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    (at, chunks) = (8, {})
    while at < len(data):
        (length,) = struct.unpack_from(">I", data, at)
        (kind, body) = (data[at + 4:at + 8], data[at + 8:at + 8 + length])
        assert struct.unpack_from(">I", data, at + 8 + length)[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks[kind] = body
        at += 12 + length
    (width, height, depth, colour) = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (depth, colour) == (8, 3) and len(chunks[b"PLTE"]) == 768 and chunks[b"tRNS"][0] == 0
    return width, height, zlib.decompress(chunks[b"IDAT"])
