"""Host reference of the dithered egress (``sn_egress_yuv_dither``, csrc/sn_yuv.hip), numpy only.

``d`` restates the hash of include/shiftnet_hip.h in integer arithmetic; ``egress`` is ``yuv_ref.egress_emu`` with the dither term added before
the rounding, in float32 and in the order the header states: what the kernel must equal bit for bit.
"""
from __future__ import annotations

import numpy as np

import yuv_ref as R

f32 = np.float32
u64 = np.uint64
M32 = u64(0xFFFFFFFF)


def key(seed: int, f: int, p: int, H: int, W: int) -> np.ndarray:
    """The mixed 32-bit key of every sample of an H x W plane: uint64 arithmetic masked to 32 bits after every product (uint32 wrapping)."""
    y = (np.arange(H, dtype=u64)[:, None] * u64(0x9E3779B1)) & M32
    x = (np.arange(W, dtype=u64)[None, :] * u64(0x85EBCA77)) & M32
    k = y ^ x ^ ((u64(f) * u64(0xC2B2AE3D)) & M32) ^ ((u64(p) * u64(0x27D4EB2F)) & M32) ^ (u64(seed) & M32)
    k ^= k >> u64(16)
    k = (k * u64(0x85EBCA6B)) & M32
    k ^= k >> u64(13)
    k = (k * u64(0xC2B2AE35)) & M32
    k ^= k >> u64(16)
    return k


def d(seed: int, f: int, p: int, H: int, W: int) -> np.ndarray:
    """float32 [H, W]: the dither of frame f, plane p (0 Y, 1 Cb, 2 Cr): the sum of two 12-bit fields of the key, centred, over 4096."""
    k = key(seed, f, p, H, W)
    n = (k & u64(0xFFF)).astype(np.int64) + ((k >> u64(12)) & u64(0xFFF)).astype(np.int64) - 4095
    return n.astype(f32) / f32(4096)


def zero(seed: int, f: int, p: int, H: int, W: int) -> np.ndarray:
    return np.zeros((H, W), f32)


def egress(x: np.ndarray, fmt: R.Fmt, H: int, W: int, seed: int, t0: int, noise=d) -> np.ndarray:
    """x: float32 [T,3,Hp,Wp] (the values the kernel reads) -> uint8 [T, frame_bytes]: code = clamp(rint((off + scale * v) + d)), frame t of x
    is frame number t0 + t.  ``noise``: the dither term (``zero``: the undithered egress)."""
    assert x.dtype == f32
    c = R.constants(fmt)
    k = c["32"]
    out = []
    for t, fr in enumerate(x):
        y, u, v = R._ycc_emu(fr[:, :H, :W], k)
        if fmt.chroma != R.C444:
            u, v = R._down(u, fmt.chroma, H, W, True), R._down(v, fmt.chroma, H, W, True)

        def rnd(off, sc, a, lo, hi, p):
            raw = off + sc * a
            dd = noise(seed, t0 + t, p, *a.shape)
            assert raw.dtype == f32 and dd.dtype == f32
            return np.clip(np.rint(raw + dd).astype(np.int64), lo, hi)
        out.append(R.join_planes(rnd(k["yo"], k["ys"], y, c["ylo"], c["yhi"], 0), rnd(k["co"], k["cs"], u, c["clo"], c["chi"], 1),
                                 rnd(k["co"], k["cs"], v, c["clo"], c["chi"], 2), fmt))
    return np.stack(out)
