"""Host reference of ``sn_yuv_ssim_sums``, numpy only: the definition in include/shiftnet_hip.h restated in float64 -- separable 11-tap Gaussian, the
border replicated at the picture's edge, constants that follow 2^bits - 1, every position counted, the map summed per 32 x 32 tile.  It differs from the
reference implementation's ``_ssim_cly`` in the order of its sums only (separable here, one 11 x 11 correlation there), and from the kernel in
precision: the kernel forms the map in float32."""
from __future__ import annotations

import math

import numpy as np

import picture_ref as P
import yuv_ref as R
from shiftnet_amd import fullref as F

TILE = 32                                                      # SN_SSIM_TILE


def _filter(x: np.ndarray, g: np.ndarray) -> np.ndarray:
    """G * x: rows, then columns, float64, replicated border."""
    h, w = x.shape
    r = len(g) // 2
    cols = np.clip(np.arange(-r, w + r), 0, w - 1)
    rows = np.clip(np.arange(-r, h + r), 0, h - 1)
    xr = x[:, cols]
    hx = sum(g[k] * xr[:, k:k + w] for k in range(len(g)))
    hr = hx[rows, :]
    return sum(g[k] * hr[k:k + h, :] for k in range(len(g)))


def ssim_map_ref(Ya: np.ndarray, Yb: np.ndarray, bits: int) -> np.ndarray:
    """float64 [h, w]: the SSIM map of two luma planes of codes."""
    a, b = np.asarray(Ya, np.float64), np.asarray(Yb, np.float64)
    g = F.ssim_taps()
    c1, c2 = F.ssim_constants(bits)
    mua, mub = _filter(a, g), _filter(b, g)
    saa, sbb, sab = _filter(a * a, g) - mua * mua, _filter(b * b, g) - mub * mub, _filter(a * b, g) - mua * mub
    return ((2 * mua * mub + c1) * (2 * sab + c2)) / ((mua * mua + mub * mub + c1) * (saa + sbb + c2))


def tile_counts(h: int, w: int) -> np.ndarray:
    """float64 [nty, ntx]: the positions of every tile."""
    ys = np.minimum(TILE, h - TILE * np.arange(-(-h // TILE)))
    xs = np.minimum(TILE, w - TILE * np.arange(-(-w // TILE)))
    return np.outer(ys, xs).astype(np.float64)


def tiles_of_map(m: np.ndarray) -> np.ndarray:
    h, w = m.shape
    nty, ntx = -(-h // TILE), -(-w // TILE)
    return np.array([[math.fsum(m[i * TILE:(i + 1) * TILE, j * TILE:(j + 1) * TILE].reshape(-1)) for j in range(ntx)] for i in range(nty)], np.float64)


def ssim_sums_ref(a: np.ndarray, b: np.ndarray, fmt: R.Fmt, H: int, W: int, rect=None) -> np.ndarray:
    """a, b: uint8 [T, frame_bytes] -> float64 [T, nty, ntx], the tile sums of the map of every pair's luma planes (of the rectangle, or the frame)."""
    a, b = (np.ascontiguousarray(x) for x in (a, b))
    if rect is not None:
        a, b = P.crop_payloads(a, fmt, H, W, rect), P.crop_payloads(b, fmt, H, W, rect)
        H, W = rect[3], rect[2]
    return np.stack([tiles_of_map(ssim_map_ref(R.split_planes(x, fmt, H, W)[0], R.split_planes(y, fmt, H, W)[0], fmt.bits)) for x, y in zip(a, b)])
