"""Host references of the scene-cut path, numpy only: the thumbnail ``sn_yuv_thumb`` must equal exactly, the cut measure restated on its own,
and the 26-frame clip with five cuts that the detector was checked on.  ``tests/yuv_ref.py`` supplies the payload layout."""
from __future__ import annotations

import numpy as np

import yuv_ref as R
from shiftnet_amd import synth

FMT420 = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)
CUTS26 = [7, 12, 18, 22, 23]                                   # scene starts of clip26: scenes of 7, 5, 6, 4, 1 and 3 frames
KINDS = ("sharp", "blurred", "noisy50")


def thumb_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int) -> np.ndarray:
    """uint8 [T, frame_bytes] -> uint16 [T, ceil(H/8), ceil(W/8)]: the sum of the luma codes of every 8 x 8 block; pixels outside H x W add nothing."""
    hb, wb = (H + 7) // 8, (W + 7) // 8
    out = np.empty((len(payloads), hb, wb), np.uint16)
    for t, p in enumerate(payloads):
        Y = R.split_planes(np.ascontiguousarray(p), fmt, H, W)[0]
        pad = np.zeros((hb * 8, wb * 8), np.int64)
        pad[:H, :W] = Y
        s = pad.reshape(hb, 8, wb, 8).sum(axis=(1, 3))
        assert s.max() <= 65535
        out[t] = s
    return out


def measure_ref(thumbs: np.ndarray, H: int, W: int, bits: int = 8):
    """m[t] = sum |S_t - S_(t-1)| / (H W 2^(bits-8)), t >= 1; m[0] = 0.0.  The numerator is a Python integer."""
    m = [0.0]
    for t in range(1, len(thumbs)):
        num = sum(abs(int(a) - int(b)) for a, b in zip(thumbs[t].reshape(-1).tolist(), thumbs[t - 1].reshape(-1).tolist()))
        m.append(num / float(H * W * (1 << (bits - 8))))
    return m


def reference_level(m, t: int) -> float:
    """ref[t]: the median of m[j], j != t, max(1, t-3) <= j <= min(last, t+3); 0.0 if there is none."""
    v = [m[j] for j in range(max(1, t - 3), min(len(m) - 1, t + 3) + 1) if j != t]
    return float(np.median(v)) if v else 0.0


def _mk(kind: str, t: int, h: int, w: int, seed: int) -> np.ndarray:
    if kind == "sharp":
        return synth.sharp_clip(t, h, w, seed)
    if kind == "blurred":
        return synth.blurred_clip(t, h, w, seed)[0]
    if kind == "noisy50":
        return np.clip(synth.sharp_clip(t, h, w, seed).astype(np.int16) + synth.noise_i16(t, h, w, 50, seed), 0, 255).astype(np.uint8)
    raise ValueError(kind)


def clip26(kind: str, h: int, w: int) -> np.ndarray:
    """[26, h, w, 3] uint8: six scenes A .. F, scene starts CUTS26.  B, C and E are inverted or compressed: scenes that differ only by the
    generator's seed are too alike for any detector (their cut measure is within 2x of the motion's own)."""
    a = _mk(kind, 7, h, w, 0)
    b = 255 - _mk(kind, 5, h, w, 3)
    c = ((_mk(kind, 6, h, w, 5) >> 1) + 40).astype(np.uint8)
    d = _mk(kind, 4, h, w, 9)
    e = 255 - _mk(kind, 1, h, w, 2)
    f = _mk(kind, 3, h, w, 7)
    return np.concatenate([a, b, c, d, e, f])


def payloads_of(rgb_u8: np.ndarray, h: int, w: int, fmt: R.Fmt = FMT420) -> np.ndarray:
    """[T, h, w, 3] uint8 RGB -> uint8 [T, frame_bytes] payloads as ``yuv_ref.egress_emu`` writes them."""
    x = np.ascontiguousarray(rgb_u8.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)
    return R.egress_emu(x, fmt, h, w)
