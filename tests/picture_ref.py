"""Host references of the active-picture path, numpy only: the cropped stream of a picture rectangle and its inverse, the row and column sums
``sn_yuv_rowcol_sums`` must equal exactly, and the letterboxed clip of the restorer's tests.  ``tests/yuv_ref.py`` supplies the payload layout."""
from __future__ import annotations

import numpy as np

import yuv_ref as R


def chroma_rect(fmt: R.Fmt, rect):
    """(column, row, width, height) of the rectangle in the chroma planes."""
    x0, y0, w, h = rect
    return (x0, y0, w, h) if fmt.chroma == R.C444 else (x0 // 2, y0 // 2, (w + 1) // 2, (h + 1) // 2)


def crop_payloads(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, rect) -> np.ndarray:
    """uint8 [T, frame_bytes(H, W)] -> uint8 [T, frame_bytes(h, w)]: the rectangle cut out of every plane of every frame."""
    x0, y0, w, h = rect
    cx, cy, cw, ch = chroma_rect(fmt, rect)
    out = []
    for p in payloads:
        Y, U, V = R.split_planes(np.ascontiguousarray(p), fmt, H, W)
        out.append(R.join_planes(Y[y0:y0 + h, x0:x0 + w], U[cy:cy + ch, cx:cx + cw], V[cy:cy + ch, cx:cx + cw], fmt))
    return np.stack(out)


def paste_payloads(full: np.ndarray, cropped: np.ndarray, fmt: R.Fmt, H: int, W: int, rect) -> np.ndarray:
    """``full`` [T, frame_bytes(H, W)] with the samples of the rectangle, luma and chroma, replaced by those of ``cropped`` [T, frame_bytes(h, w)]."""
    x0, y0, w, h = rect
    cx, cy, cw, ch = chroma_rect(fmt, rect)
    out = []
    for p, c in zip(full, cropped):
        Y, U, V = (a.copy() for a in R.split_planes(np.ascontiguousarray(p), fmt, H, W))
        y, u, v = R.split_planes(np.ascontiguousarray(c), fmt, h, w)
        Y[y0:y0 + h, x0:x0 + w] = y
        U[cy:cy + ch, cx:cx + cw] = u
        V[cy:cy + ch, cx:cx + cw] = v
        out.append(R.join_planes(Y, U, V, fmt))
    return np.stack(out)


def rowcol_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int):
    """uint8 [T, frame_bytes] -> (uint32 [T, H], uint32 [T, W]): the sums of the luma codes of every row and of every column."""
    Y = np.stack([R.split_planes(np.ascontiguousarray(p), fmt, H, W)[0] for p in payloads])
    return Y.sum(axis=2).astype(np.uint32), Y.sum(axis=1).astype(np.uint32)


def black_payload(fmt: R.Fmt, H: int, W: int) -> np.ndarray:
    """One frame at the format's black: luma at the black code, chroma at the neutral code."""
    s = 1 << (fmt.bits - 8)
    ch, cw = R.chroma_shape(fmt, H, W)
    return R.join_planes(np.full((H, W), 0 if fmt.range == R.FULL else 16 * s), np.full((ch, cw), 128 * s), np.full((ch, cw), 128 * s), fmt)


# ---- the clip of the restorer's tests (tests/test_gpu_picture.py) ---------------------------------------------------------------------------
BOXED = dict(n=7, h=96, w=128, one_len=3, rect=(0, 12, 128, 72))


def boxed_payloads(fmt: R.Fmt, rgb_u8: np.ndarray) -> np.ndarray:
    """rgb_u8: [n, 72, 128, 3] picture frames -> [n, frame_bytes(96, 128)] payloads: the picture inside BOXED['rect'], bars at black."""
    c = BOXED
    x = np.ascontiguousarray(rgb_u8.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)
    inner = R.egress_emu(x, fmt, c["rect"][3], c["rect"][2])
    full = np.stack([black_payload(fmt, c["h"], c["w"])] * len(inner))
    return paste_payloads(full, inner, fmt, c["h"], c["w"], c["rect"])
