"""Host reference of the sums of ``sn_yuv_niqe_sums``, numpy only, float64 throughout: restated from the definition in include/shiftnet_hip.h -- the same
crop, clamp, wrap and order of the sums -- and sharing nothing with shiftnet_amd/niqe.py.  The kernel computes the map values in float32, so it equals
this to a tolerance, and its counts differ where a value and its float64 twin lie on both sides of zero.
``tests/yuv_ref.py`` supplies the payload layout and ``tests/picture_ref.py`` the planes of a rectangle."""
from __future__ import annotations

import numpy as np

import picture_ref as P
import yuv_ref as R

BLOCK, MAPS, SUMS = 96, 5, 5                                   # SN_NIQE_BLOCK, SN_NIQE_MAPS, SN_NIQE_SUMS
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))                     # (dy, dx) of maps 1 .. 4


def values(Y: np.ndarray, fmt: R.Fmt) -> np.ndarray:
    """Luma codes -> the 16 .. 235 scale.  The full-range constant is the kernel's: a float64 expression rounded once to float32."""
    Y = np.asarray(Y, np.float64)
    if fmt.range == R.FULL:
        return 16.0 + Y * np.float64(np.float32(219.0 / ((1 << fmt.bits) - 1)))
    return Y / (1 << (fmt.bits - 8))


def sum7(p: list) -> np.ndarray:
    return (((p[0] + p[6]) + (p[1] + p[5])) + (p[2] + p[4])) + p[3]


def filter7(I: np.ndarray, g: np.ndarray) -> np.ndarray:
    """Rows, then columns, indices clamped to the array."""
    h, w = I.shape
    a = np.pad(I, ((0, 0), (3, 3)), mode="edge")
    r = sum7([g[i] * a[:, i:i + w] for i in range(7)])
    a = np.pad(r, ((3, 3), (0, 0)), mode="edge")
    return sum7([g[j] * a[j:j + h, :] for j in range(7)])


def coefficients(I: np.ndarray, g: np.ndarray) -> np.ndarray:
    mu, m2 = filter7(I, g), filter7(I * I, g)
    return (I - mu) / (np.sqrt(np.abs(m2 - mu * mu)) + 1.0)


def map_sums(block: np.ndarray) -> np.ndarray:
    """One B x B block of coefficients -> [5, 5]: per map the count and the sum of squares of the negative values, the same of the positive values,
    the sum of the magnitudes."""
    block = np.asarray(block, np.float64)
    out = np.zeros((MAPS, SUMS))
    for k, m in enumerate([block] + [block * np.roll(block, s, axis=(0, 1)) for s in SHIFTS]):
        neg, pos = m[m < 0], m[m > 0]
        out[k] = [neg.size, (neg * neg).sum(), pos.size, (pos * pos).sum(), np.abs(m).sum()]
    return out


def sums_of_luma(Y: np.ndarray, fmt: R.Fmt, g) -> np.ndarray:
    """Y: [h, w] luma codes of the picture; g: the 7 taps as the kernel gets them -> float64 [2, nbh, nbw, 5, 5]."""
    g = np.asarray(g, np.float64)
    h, w = Y.shape
    nbh, nbw = h // BLOCK, w // BLOCK
    I = values(Y[:BLOCK * nbh, :BLOCK * nbw], fmt)
    out = np.zeros((2, nbh, nbw, MAPS, SUMS))
    for s in range(2):
        if s == 1:
            I = 0.25 * ((I[0::2, 0::2] + I[0::2, 1::2]) + (I[1::2, 0::2] + I[1::2, 1::2]))
        n, B = coefficients(I, g), BLOCK >> s
        for by in range(nbh):
            for bx in range(nbw):
                out[s, by, bx] = map_sums(n[by * B:(by + 1) * B, bx * B:(bx + 1) * B])
    return out


def niqe_sums_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, g, rect=None) -> np.ndarray:
    """uint8 [T, frame_bytes] -> float64 [T, 2, nbh, nbw, 5, 5]."""
    payloads = np.ascontiguousarray(payloads)
    if rect is not None:
        payloads = P.crop_payloads(payloads, fmt, H, W, rect)
        H, W = rect[3], rect[2]
    return np.stack([sums_of_luma(R.split_planes(p, fmt, H, W)[0], fmt, g) for p in payloads])
