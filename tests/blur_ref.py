"""Host references of the motion blur (``sn_yuv_blur``, csrc/sn_blur.hip), numpy only.

``blur_ref``   the float32 restatement, in the order include/shiftnet_hip.h states: ``yuv_ref.ingest_emu``, the table arithmetic (decode, the sum in
               ascending tap order, the mean, encode), ``yuv_ref.egress_emu``; each product and sum rounded to float32.  What the kernel must equal
               bit for bit.  The tables are the package's own (``degrade.gamma_tables``); there is no second copy of them.
``blur_f64``   the definition in float64: ``yuv_ref.ingest_f64``, a real ``** g``, a float64 mean, ``** (1 / g)``, ``yuv_ref.egress_f64``.  What the
               restatement's arithmetic is judged against."""
from __future__ import annotations

import numpy as np

import yuv_ref as R
from shiftnet_amd import degrade

f32 = np.float32


def tap_indices(n: int, c0: int, T: int, lo: int, hi: int) -> np.ndarray:
    """int [T, n]: the source payload of every tap of every output, clamped to [lo, hi]."""
    r = n // 2
    return np.clip(c0 + np.arange(T)[:, None] + np.arange(-r, r + 1)[None, :], lo, hi)


def decode(x: np.ndarray, lin: np.ndarray) -> np.ndarray:
    u = x * f32(4095.0)
    i = np.minimum(u.astype(np.int64), 4094)                # u >= 0: the conversion is the floor
    e = u - i.astype(f32)
    v = lin[i] + e * (lin[i + 1] - lin[i])
    assert v.dtype == f32
    return v


def encode(m: np.ndarray, lin: np.ndarray, rinv: np.ndarray) -> np.ndarray:
    i = np.searchsorted(lin[:4095], m, side="right") - 1     # the largest index in 0 .. 4094 with lin[i] <= m
    assert i.min() >= 0
    e = np.minimum((m - lin[i]) * rinv[i], f32(1.0))
    x = (i.astype(f32) + e) * f32(1.0 / 4095.0)
    assert x.dtype == f32
    return x


def blur_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, n: int, c0: int, T: int, lo: int, hi: int, gamma: float) -> np.ndarray:
    """uint8 [S, frame_bytes] sharp payloads -> uint8 [T, frame_bytes]: outputs c0 .. c0 + T - 1.  gamma 1: no tables."""
    payloads = np.ascontiguousarray(payloads)
    assert n % 2 == 1 and 0 <= lo <= hi < len(payloads) and lo <= c0 and c0 + T - 1 <= hi
    v = R.ingest_emu(payloads, fmt, H, W, H, W)
    tables = None if gamma == 1.0 else degrade.gamma_tables(gamma)
    if tables is not None:
        v = decode(v, tables[0])
    idx = tap_indices(n, c0, T, lo, hi)
    acc = v[idx[:, 0]]
    for j in range(1, n):
        acc = acc + v[idx[:, j]]
    m = acc * f32(1.0 / n)
    assert m.dtype == f32
    return R.egress_emu(m if tables is None else encode(m, *tables), fmt, H, W)


def blur_f64(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, n: int, c0: int, T: int, lo: int, hi: int, gamma: float) -> np.ndarray:
    payloads = np.ascontiguousarray(payloads)
    v = R.ingest_f64(payloads, fmt, H, W, H, W) ** float(gamma)
    m = v[tap_indices(n, c0, T, lo, hi)].mean(axis=1)
    return R.egress_f64(m ** (1.0 / float(gamma)), fmt, H, W)


def blur_stream(payloads, fmt: R.Fmt, H: int, W: int, n: int, gamma: float, cuts=()) -> np.ndarray:
    """The whole stream blurred, every scene (``cuts``: the scene starts) on its own: what ``add_blur`` makes of it."""
    payloads = np.stack(payloads)
    starts = [0] + list(cuts) + [len(payloads)]
    return np.concatenate([blur_ref(payloads, fmt, H, W, n, a, b - a, a, b - 1, gamma) for a, b in zip(starts, starts[1:])])
