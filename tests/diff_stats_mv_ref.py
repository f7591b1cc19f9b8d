"""Host reference of the method-noise sums along block motion vectors, numpy only: what ``sn_yuv_diff_stats_mv`` must equal word for word, restated in
int64 from the definition in include/shiftnet_hip.h.  ``tests/nlf_ref.py`` supplies the luma plane of a payload (of a rectangle of it).  ``split=False``
measures on every 2 x 2 block instead of the measuring half: it exists to pin this restatement against ``tests/diff_stats_ref.py`` (all vectors zero,
even h and w: every sample counts) and is nothing the kernel does."""
from __future__ import annotations

import numpy as np

import nlf_ref as F
import yuv_ref as R

WORDS = 8                                                      # SN_DIFF_STATS_MV
BLOCK = 8                                                      # 2 x 2 blocks per side of a vector block


def sums_of_pair(a0, b0, a1, b1, mv, split: bool = True) -> list:
    """The 8 words of one pair from its luma planes [h, w] (what came in and what was written, of payload p and of payload p + 1) and the pair's
    vectors int8 [nby, nbx, 2], which may hold any int8."""
    a0, b0, a1, b1 = (np.asarray(x, np.int64) for x in (a0, b0, a1, b1))
    h, w = a0.shape
    hb, wb = h // 2, w // 2
    if hb == 0 or wb == 0:
        return [0] * WORDS
    i, j = np.mgrid[0:hb, 0:wb]
    vec = np.asarray(mv).astype(np.int64)[i // BLOCK, j // BLOCK]
    dy, dx = vec[..., 0], vec[..., 1]
    ok = (2 * i + dy >= 0) & (2 * i + dy + 2 <= h) & (2 * j + dx >= 0) & (2 * j + dx + 2 <= w)      # the displaced block lies wholly inside the picture
    if split:
        ok &= ((i + j) & 1) == 1                                # measuring blocks
    i, j, dy, dx = i[ok], j[ok], dy[ok], dx[ok]
    out = [0] * WORDS
    for r in (0, 1):
        for c in (0, 1):
            y, x = 2 * i + r, 2 * j + c
            d0 = b0[y, x] - a0[y, x]
            d1 = b1[y + dy, x + dx] - a1[y + dy, x + dx]
            g = b1[y + dy, x + dx] - b0[y, x]
            out[0] += int(y.size)
            out[1] += int(d0.sum())
            out[2] += int((d0 * d0).sum())
            out[3] += int(d1.sum())
            out[4] += int((d1 * d1).sum())
            out[5] += int((d0 * d1).sum())
            out[6] += int((g * g).sum())
            out[7] += int(((dy != 0) | (dx != 0)).sum())
    return out


def diff_stats_mv_ref(a: np.ndarray, b: np.ndarray, mv: np.ndarray, fmt: R.Fmt, H: int, W: int, rect=None, split: bool = True) -> np.ndarray:
    """a (what came in), b (what was written): uint8 [T, frame_bytes]; mv: int8 [T - 1, nby, nbx, 2] -> int64 [T - 1, 8].  Samples are taken as stored."""
    a, b = (np.ascontiguousarray(x) for x in (a, b))
    assert a.shape == b.shape and a.shape[1] == R.frame_bytes(fmt, H, W) and len(a) >= 2
    A = [F.luma_of(p, fmt, H, W, rect) for p in a]
    B = [F.luma_of(p, fmt, H, W, rect) for p in b]
    out = np.zeros((len(a) - 1, WORDS), np.int64)
    for p in range(len(a) - 1):
        out[p] = sums_of_pair(A[p], B[p], A[p + 1], B[p + 1], mv[p], split)
    return out
