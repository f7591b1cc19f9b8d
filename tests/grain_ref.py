"""Host reference of the grain (``sn_yuv_grain``, csrc/sn_grain.hip), numpy only: the white field from the hash, the separable 5-tap filter, the level
curve at the luma code and the rounding, each float32 product and sum rounded separately, in the order include/shiftnet_hip.h states.  It knows no
tiles: a plane's field is made whole, with a halo of 2 from the hash.  Levels are given in the user's unit (sigma of 8-bit R'G'B' codes) and converted
by the package's own ``grain.luma_knots``."""
from __future__ import annotations

import numpy as np

import yuv_ref as R
from shiftnet_amd import degrade, grain

f32 = np.float32
u32 = np.uint32
FLAT = [10.0] * 16
BUMPY = [12.0, 3.0, 9.0, 20.0, 1.0, 6.0, 15.0, 4.0, 11.0, 2.0, 18.0, 7.0, 13.0, 5.0, 8.0, 0.0]      # not monotonic, ending in a zero knot


def white_field(seed: int, f: int, plane: int, ys, xs) -> np.ndarray:
    """float32 [len(ys), len(xs)]: g_plane(f, y, x) for any integer rows and columns (negative ones wrap as uint32)."""
    y = (np.asarray(ys, np.int64) & 0xFFFFFFFF).astype(u32)[:, None]
    x = (np.asarray(xs, np.int64) & 0xFFFFFFFF).astype(u32)[None, :]
    with np.errstate(over="ignore"):
        k = (y * u32(0x9E3779B1)) ^ (x * u32(0x85EBCA77)) ^ u32((f * 0xC2B2AE3D) & 0xFFFFFFFF) ^ u32((plane * 0x27D4EB2F) & 0xFFFFFFFF) ^ u32(seed & 0xFFFFFFFF)
        k ^= k >> u32(16)
        k = k * u32(0x85EBCA6B)
        k ^= k >> u32(13)
        k = k * u32(0xC2B2AE35)
        k ^= k >> u32(16)
    return degrade.gauss_table()[k >> u32(16)]


def _fir(a, axis: int, taps) -> np.ndarray:
    """(((w2 a[-2] + w1 a[-1]) + w0 a[0]) + w1 a[+1]) + w2 a[+2] along ``axis``; the result is 4 shorter."""
    w0, w1, w2 = (f32(t) for t in taps)
    n = a.shape[axis] - 4
    s = [np.take(a, np.arange(k, k + n), axis=axis) for k in range(5)]
    out = (((w2 * s[0] + w1 * s[1]) + w0 * s[2]) + w1 * s[3]) + w2 * s[4]
    assert out.dtype == f32
    return out


def field(seed: int, f: int, plane: int, h: int, w: int, taps) -> np.ndarray:
    """float32 [h, w]: the correlated field c_plane(f, y, x), y < h, x < w."""
    g = white_field(seed, f, plane, np.arange(-2, h + 2), np.arange(-2, w + 2))
    return _fir(_fir(g, 1, taps), 0, taps)


def level(Y: np.ndarray, knots_luma, fmt: R.Fmt) -> np.ndarray:
    """float32, the shape of Y: the curve (luma code units) at the luma codes Y, with sn_yuv_degrade's interpolation."""
    k = np.asarray(knots_luma, f32)
    c = R.constants(fmt)
    lo, hi = c["ylo"], c["yhi"]
    sc = f32(16.0 / (float(hi) - float(lo)))
    u = np.minimum(np.maximum((Y.astype(f32) - f32(lo)) * sc - f32(0.5), f32(0)), f32(15))
    i = np.minimum(np.floor(u).astype(np.int64), 14)
    s = k[i] + (u - i.astype(f32)) * (k[i + 1] - k[i])
    assert s.dtype == f32
    return s


def _add(C: np.ndarray, s: np.ndarray, c: np.ndarray, lo: int, hi: int) -> np.ndarray:
    q = np.rint(C.astype(f32) + s * c).astype(np.int64)
    return np.minimum(np.maximum(q, np.minimum(lo, C)), np.maximum(hi, C))


def grain_picture(Y, U, V, fmt: R.Fmt, knots, taps, chroma: float, seed: int, f: int):
    """One picture's planes (int64; the whole frame, or a rectangle's) -> its planes with grain, frame number f."""
    k = grain.luma_knots(knots, fmt)
    c = R.constants(fmt)
    h, w = Y.shape
    Yn = _add(Y, level(Y, k, fmt), field(seed, f, 6, h, w, taps), c["ylo"], c["yhi"])
    if chroma == 0:
        return Yn, U, V
    if fmt.chroma == R.C444:
        Ym = Y
    else:
        r0, c0 = 2 * np.arange(U.shape[0]), 2 * np.arange(U.shape[1])
        r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
        Ym = (Y[r0][:, c0] + Y[r0][:, c1] + Y[r1][:, c0] + Y[r1][:, c1] + 2) >> 2
    s = f32(chroma) * level(Ym, k, fmt)
    ch, cw = U.shape
    return Yn, _add(U, s, field(seed, f, 7, ch, cw, taps), c["clo"], c["chi"]), _add(V, s, field(seed, f, 8, ch, cw, taps), c["clo"], c["chi"])


def grain_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, knots, taps, chroma: float, seed: int, t0: int, rect=None) -> np.ndarray:
    """uint8 [T, frame_bytes], frames t0 .. t0 + T - 1 of their clip -> uint8 [T, frame_bytes].  ``knots``: 16 levels in 8-bit R'G'B' code units.
    ``rect=(x0, y0, w, h)``: the rectangle is the picture; every sample outside stays."""
    out = []
    for t, p in enumerate(np.ascontiguousarray(payloads)):
        Y, U, V = (a.copy() for a in R.split_planes(p, fmt, H, W))
        if rect is None:
            Y, U, V = grain_picture(Y, U, V, fmt, knots, taps, chroma, seed, t0 + t)
        else:
            x0, y0, w, h = rect
            sub = fmt.chroma != R.C444
            cx0, cy0, cw, ch = (x0 >> 1, y0 >> 1, (w + 1) >> 1, (h + 1) >> 1) if sub else (x0, y0, w, h)
            ys, cs = (slice(y0, y0 + h), slice(x0, x0 + w)), (slice(cy0, cy0 + ch), slice(cx0, cx0 + cw))
            Y[ys], U[cs], V[cs] = grain_picture(Y[ys], U[cs], V[cs], fmt, knots, taps, chroma, seed, t0 + t)
        out.append(R.join_planes(Y, U, V, fmt))
    return np.stack(out)
