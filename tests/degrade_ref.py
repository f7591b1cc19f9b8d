"""Host reference of the added noise (``sn_yuv_degrade``, csrc/sn_degrade.hip), numpy only: ``yuv_ref.ingest_emu`` in float32, plus
``degrade.noise_field`` times the noise curve at every pixel's clean luma code, each product and sum rounded to float32, then ``yuv_ref.egress_emu`` --
in the order include/shiftnet_hip.h states.  The field of samples is the package's own (shiftnet_amd/degrade.py); there is no second copy of the hash."""
from __future__ import annotations

import numpy as np

import noise_ref as N
import yuv_ref as R
from shiftnet_amd import degrade

f32 = np.float32
FLAT = [10.0] * 16
FALLING = [24.0 - 1.5 * b for b in range(16)]               # 24 at black down to 1.5 at white


def knots32(knots) -> np.ndarray:
    """The curve as the kernel uses it: the float32 knots / 255 in float64, rounded once to float32."""
    k = np.asarray(knots, f32)
    assert k.shape == (16,)
    return (k.astype(np.float64) / 255.0).astype(f32)


def sigma_plane(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, knots) -> np.ndarray:
    """float32 [T, 1, H, W]: the curve at every pixel's own luma code, with the interpolation of sn_noise_map_level (tests/nlf_ref.py: map_ref)."""
    k = knots32(knots)
    lo, hi = N.clip_codes(fmt)
    sc = f32(16.0 / (float(hi) - float(lo)))
    out = []
    for p in payloads:
        Y = R.split_planes(np.ascontiguousarray(p), fmt, H, W)[0]
        u = np.minimum(np.maximum((Y.astype(f32) - f32(lo)) * sc - f32(0.5), f32(0)), f32(15))
        i = np.minimum(np.floor(u).astype(np.int64), 14)
        e = u - i.astype(f32)
        s = k[i] + e * (k[i + 1] - k[i])
        assert s.dtype == f32
        out.append(s[None])
    return np.stack(out)


def degrade_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, knots, seed: int, t0: int) -> np.ndarray:
    """uint8 [T, frame_bytes] clean payloads, frames t0 .. t0 + T - 1 of their stream -> uint8 [T, frame_bytes]."""
    payloads = np.ascontiguousarray(payloads)
    x = R.ingest_emu(payloads, fmt, H, W, H, W)
    n = sigma_plane(payloads, fmt, H, W, knots) * degrade.noise_field(seed, t0, len(payloads), H, W)
    assert x.dtype == f32 and n.dtype == f32
    return R.egress_emu(x + n, fmt, H, W)
