"""Host reference of the method-noise sums, numpy only: what ``sn_yuv_diff_stats`` must equal word for word, restated in int64 from the definition
in include/shiftnet_hip.h.  ``tests/yuv_ref.py`` supplies the payload layout and ``tests/picture_ref.py`` the planes of a rectangle."""
from __future__ import annotations

import numpy as np

import picture_ref as P
import yuv_ref as R

WORDS = 16                                                     # SN_DIFF_STATS


def sums_of_planes(dY: np.ndarray, bY: np.ndarray, dU: np.ndarray, dV: np.ndarray, edge: int, dY_next=None) -> list:
    """The 16 words of one frame from its planes (int64): dY = b - a of the luma [h, w], bY the written luma, dU and dV of the chroma planes;
    dY_next: the next frame's dY, or None for a launch's last frame."""
    dY, bY, dU, dV = (np.asarray(x, np.int64) for x in (dY, bY, dU, dV))
    h, w = dY.shape
    right = bY[:, np.minimum(np.arange(w) + 1, w - 1)]
    below = bY[np.minimum(np.arange(h) + 1, h - 1), :]
    e = np.abs(right - bY) + np.abs(below - bY)
    is_edge = e >= edge
    sq = dY * dY
    out = [h * w, dY.sum(), sq.sum(),
           h * (w - 1), (dY[:, :-1] * dY[:, 1:]).sum(),
           (h - 1) * w, (dY[:-1, :] * dY[1:, :]).sum(),
           0 if dY_next is None else (dY * np.asarray(dY_next, np.int64)).sum(),
           is_edge.sum(), sq[is_edge].sum(),
           dU.size, dU.sum(), (dU * dU).sum(), dV.sum(), (dV * dV).sum(), 0]
    return [int(v) for v in out]


def diff_stats_ref(a: np.ndarray, b: np.ndarray, fmt: R.Fmt, H: int, W: int, rect=None, edge: int = 0) -> np.ndarray:
    """a (what came in), b (what was written): uint8 [T, frame_bytes] -> int64 [T, 16].  Samples are taken as stored: a 10-bit payload's words may
    hold anything up to 65535 (products reach 65535^2 < 2^32, sums of them fit int64 with room to spare)."""
    a, b = (np.ascontiguousarray(x) for x in (a, b))
    assert a.shape == b.shape and a.shape[1] == R.frame_bytes(fmt, H, W)
    if rect is not None:
        a, b = P.crop_payloads(a, fmt, H, W, rect), P.crop_payloads(b, fmt, H, W, rect)
        H, W = rect[3], rect[2]
    planes = [[np.asarray(pb, np.int64) - np.asarray(pa, np.int64) for pa, pb in zip(R.split_planes(x, fmt, H, W), R.split_planes(y, fmt, H, W))]
              for x, y in zip(a, b)]
    out = np.zeros((len(a), WORDS), np.int64)
    for t in range(len(a)):
        bY = R.split_planes(b[t], fmt, H, W)[0]
        nxt = planes[t + 1][0] if t + 1 < len(a) else None
        out[t] = sums_of_planes(planes[t][0], bY, planes[t][1], planes[t][2], edge, nxt)
    return out
