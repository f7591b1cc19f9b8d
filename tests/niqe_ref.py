"""Host references of the sums of ``sn_yuv_niqe_sums``, numpy only, sharing nothing with shiftnet_amd/niqe.py.  Two of them:

  * ``plain_sums_of_luma``: the formula of include/shiftnet_hip.h as one would write it down -- the values themselves, no pivot, the model's float64
    taps -- in ``np.longdouble`` throughout.  It says what the right answer is.
  * ``sums_of_luma`` / ``niqe_sums_ref``: the kernel's arithmetic restated rounding for rounding: float64 from the codes on, per block the deviations
    from the block's own first sample filtered, the block's halo included, in the header's order.  Every numpy operation here is one correctly
    rounded float64 operation, as every operation of the kernel is, so with the kernel's taps (``kernel_taps``: the float32 taps widened, over their
    sum) the coefficients are the kernel's bit for bit and the counts are equal; the sums differ by the order in which the block's values are added.
    With the model's float64 taps it is the same arithmetic without what the float32 taps cost, and equals the plain reference to 3e-12.

``tests/yuv_ref.py`` supplies the payload layout and ``tests/picture_ref.py`` the planes of a rectangle."""
from __future__ import annotations

import numpy as np

import picture_ref as P
import yuv_ref as R

BLOCK, MAPS, SUMS = 96, 5, 5                                   # SN_NIQE_BLOCK, SN_NIQE_MAPS, SN_NIQE_SUMS
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))                     # (dy, dx) of maps 1 .. 4


def values(Y: np.ndarray, fmt: R.Fmt, dtype=np.float64) -> np.ndarray:
    """Luma codes -> the 16 .. 235 scale.  The full-range constant is the kernel's: a float64 expression rounded once to float32.  Code times
    constant has 34 significant bits at most, so the values are exact in float64."""
    Y = np.asarray(Y, dtype)
    if fmt.range == R.FULL:
        return dtype(16.0) + Y * dtype(np.float32(219.0 / ((1 << fmt.bits) - 1)))
    return Y / dtype(1 << (fmt.bits - 8))


def halve(I: np.ndarray) -> np.ndarray:
    """Scale 2: the mean of every 2 x 2 samples (exact in float64)."""
    return I.dtype.type(0.25) * ((I[0::2, 0::2] + I[0::2, 1::2]) + (I[1::2, 0::2] + I[1::2, 1::2]))


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
    """The header's n of a whole picture of one scale from the values themselves, in the precision of I and g."""
    mu, m2 = filter7(I, g), filter7(I * I, g)
    return (I - mu) / (np.sqrt(np.abs(m2 - mu * mu)) + 1)


def block_coefficients(padded: np.ndarray, by: int, bx: int, B: int, g: np.ndarray) -> np.ndarray:
    """The kernel's n of block (by, bx): ``padded`` is the picture of one scale with 3 replicated samples on every side, float64; g 7 float64 taps.
    J = I - p, p the block's own sample (0, 0), over the block and its halo; rows, then columns."""
    win = padded[by * B:by * B + B + 6, bx * B:bx * B + B + 6]
    J = win - win[3, 3]
    JJ = J * J
    r1 = sum7([g[i] * J[:, i:i + B] for i in range(7)])
    r2 = sum7([g[i] * JJ[:, i:i + B] for i in range(7)])
    mu = sum7([g[j] * r1[j:j + B, :] for j in range(7)])
    m2 = sum7([g[j] * r2[j:j + B, :] for j in range(7)])
    return (J[3:3 + B, 3:3 + B] - mu) / (np.sqrt(np.abs(m2 - mu * mu)) + 1.0)


def block_maps(block: np.ndarray) -> list:
    """The five maps of one B x B block of coefficients: n and its products with four neighbours, the wrap inside the block."""
    return [block] + [block * np.roll(block, s, axis=(0, 1)) for s in SHIFTS]


def map_sums(block: np.ndarray) -> np.ndarray:
    """One B x B block of coefficients -> [5, 5]: per map the count and the sum of squares of the negative values, the same of the positive values,
    the sum of the magnitudes.  A longdouble block is summed in longdouble; anything else in float64."""
    block = np.asarray(block, np.longdouble if np.asarray(block).dtype == np.longdouble else np.float64)
    out = np.zeros((MAPS, SUMS))
    for k, m in enumerate(block_maps(block)):
        neg, pos = m[m < 0], m[m > 0]
        out[k] = [neg.size, (neg * neg).sum(), pos.size, (pos * pos).sum(), np.abs(m).sum()]
    return out


def kernel_taps(g) -> np.ndarray:
    """The 7 taps as the kernel uses them: rounded to float32 (what the binding hands over), widened to float64 and divided by their own 7-tap sum."""
    w = np.asarray(g).astype(np.float32).astype(np.float64)
    return w / sum7(list(w))


def coefficient_blocks(Y: np.ndarray, fmt: R.Fmt, g):
    """Yields (scale index, by, bx, the block's float64 coefficients as the kernel forms them) over the whole blocks of the picture Y; g: 7 float64
    taps, used as they are (``kernel_taps`` makes the kernel's)."""
    g = np.asarray(g, np.float64)
    h, w = Y.shape
    nbh, nbw = h // BLOCK, w // BLOCK
    I = values(Y[:BLOCK * nbh, :BLOCK * nbw], fmt)
    for s in range(2):
        if s == 1:
            I = halve(I)
        padded, B = np.pad(I, 3, mode="edge"), BLOCK >> s
        for by in range(nbh):
            for bx in range(nbw):
                yield s, by, bx, block_coefficients(padded, by, bx, B, g)


def sums_of_luma(Y: np.ndarray, fmt: R.Fmt, g) -> np.ndarray:
    """Y: [h, w] luma codes of the picture; g: 7 float64 taps, used as they are -> float64 [2, nbh, nbw, 5, 5]."""
    out = np.zeros((2, Y.shape[0] // BLOCK, Y.shape[1] // BLOCK, MAPS, SUMS))
    for s, by, bx, n in coefficient_blocks(Y, fmt, g):
        out[s, by, bx] = map_sums(n)
    return out


def plain_sums_of_luma(Y: np.ndarray, fmt: R.Fmt, g) -> np.ndarray:
    """The same sums from the formula as the header states it for the values themselves, in longdouble: no pivot, g the model's float64 taps unrounded,
    the picture of each scale filtered as a whole.  -> float64 [2, nbh, nbw, 5, 5] (each sum rounded once at the end)."""
    g = np.asarray(g, np.longdouble)
    h, w = Y.shape
    nbh, nbw = h // BLOCK, w // BLOCK
    I = values(Y[:BLOCK * nbh, :BLOCK * nbw], fmt, np.longdouble)
    out = np.zeros((2, nbh, nbw, MAPS, SUMS))
    for s in range(2):
        if s == 1:
            I = halve(I)
        n, B = coefficients(I, g), BLOCK >> s
        assert n.dtype == np.longdouble
        for by in range(nbh):
            for bx in range(nbw):
                out[s, by, bx] = map_sums(n[by * B:(by + 1) * B, bx * B:(bx + 1) * B])
    return out


def niqe_sums_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, g, rect=None, sums=sums_of_luma) -> np.ndarray:
    """uint8 [T, frame_bytes] -> float64 [T, 2, nbh, nbw, 5, 5]; ``sums``: sums_of_luma (the restatement) or plain_sums_of_luma."""
    payloads = np.ascontiguousarray(payloads)
    if rect is not None:
        payloads = P.crop_payloads(payloads, fmt, H, W, rect)
        H, W = rect[3], rect[2]
    return np.stack([sums(R.split_planes(p, fmt, H, W)[0], fmt, g) for p in payloads])
