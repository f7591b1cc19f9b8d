"""Host reference of the mixed egress (``sn_egress_yuv_mix``, csrc/sn_yuv.hip), numpy only.

``egress`` is ``dither_ref.egress`` with the last line replaced by the mix of include/shiftnet_hip.h, in float32 and in the order the header
states: what the kernel must equal bit for bit.  ``egress_f64`` is the same formulas in float64 (the reference the arithmetic is judged
against); it also returns the value before the rounding.

A mix is ``(word, ay, ac)`` with word "amount" or "removed"; both references round ay and ac to float32 first, as the struct carries them.
"""
from __future__ import annotations

import numpy as np

import dither_ref as D
import yuv_ref as R

f32 = np.float32
WORDS = ("amount", "removed")


def _planes(fr, fmt: R.Fmt, H: int, W: int, emu: bool):
    """One frame [3,Hp,Wp] -> the three planes' values before ``off + scale * value`` (yuv_ref's own steps)."""
    c = R.constants(fmt)
    y, u, v = R._ycc_emu(fr[:, :H, :W], c["32"]) if emu else R._ycc_f64(fr[:, :H, :W], c)
    if fmt.chroma != R.C444:
        u, v = R._down(u, fmt.chroma, H, W, emu), R._down(v, fmt.chroma, H, W, emu)
    return y, u, v


def _mix(word: str, raw, cin, a, d, lo: int, hi: int, co):
    """raw = off + scale * value, cin the input's codes (int64), a the amount or gain, d the dither: (value before rounding, codes).  The float
    type is that of ``raw``: every operator below rounds once in it."""
    ft = raw.dtype.type
    e, a = cin.astype(raw.dtype), ft(a)
    if word == "amount":
        m = (e + a * (raw - e)) + d.astype(raw.dtype)
        q = np.clip(np.rint(m).astype(np.int64), np.minimum(lo, cin), np.maximum(hi, cin))
        return m, (cin.copy() if a == 0 else q)
    m = (ft(co) + a * (e - raw)) + d.astype(raw.dtype)
    return m, np.clip(np.rint(m).astype(np.int64), lo, hi)


def _egress(x, fmt: R.Fmt, H: int, W: int, mix, inp: np.ndarray, dither, emu: bool):
    word, ay, ac = mix
    assert word in WORDS
    ay, ac = f32(ay), f32(ac)
    c = R.constants(fmt)
    k = c["32"] if emu else c
    noise, seed, t0 = (D.zero, 0, 0) if dither is None else (D.d, *dither)
    raws, out = [], []
    for t, fr in enumerate(x):
        vals = _planes(fr, fmt, H, W, emu)
        cins = R.split_planes(inp[t], fmt, H, W)
        raw_codes = []
        for p, (val, cin) in enumerate(zip(vals, cins)):
            off, sc, lo, hi = (k["yo"], k["ys"], c["ylo"], c["yhi"]) if p == 0 else (k["co"], k["cs"], c["clo"], c["chi"])
            raw = off + sc * val
            assert raw.dtype == (f32 if emu else np.float64)
            raw_codes.append(_mix(word, raw, cin, ay if p == 0 else ac, noise(seed, t0 + t, p, *val.shape), lo, hi, k["co"]))
        raws.append(np.concatenate([m.reshape(-1) for m, _ in raw_codes]))
        out.append(R.join_planes(*(q for _, q in raw_codes), fmt))
    return np.stack(raws), np.stack(out)


def egress(x: np.ndarray, fmt: R.Fmt, H: int, W: int, mix, inp: np.ndarray, dither=None) -> np.ndarray:
    """x: float32 [T,3,Hp,Wp] (the values the kernel reads), inp: uint8 [T, frame_bytes] -> uint8 [T, frame_bytes].  ``dither``: None or
    (seed, t0), frame t of x is frame number t0 + t."""
    assert x.dtype == f32
    return _egress(x, fmt, H, W, mix, inp, dither, True)[1]


def egress_f64(x: np.ndarray, fmt: R.Fmt, H: int, W: int, mix, inp: np.ndarray, dither=None):
    """-> (the float64 values before the rounding [T, samples], in payload order; the payloads uint8 [T, frame_bytes])."""
    return _egress(np.asarray(x, np.float64), fmt, H, W, mix, inp, dither, False)


def codes(payloads: np.ndarray, fmt: R.Fmt) -> np.ndarray:
    """uint8 [T, frame_bytes] -> int64 [T, samples]: the codes in payload order."""
    return (payloads.view("<u2") if fmt.bits == 10 else payloads).astype(np.int64)


def random_payloads(fmt: R.Fmt, T: int, H: int, W: int, seed: int) -> np.ndarray:
    """Payloads drawn over the whole code range, illegal codes included."""
    rng = np.random.default_rng(seed)
    n = R.frame_bytes(fmt, H, W)
    if fmt.bits == 8:
        return rng.integers(0, 256, (T, n), dtype=np.uint8)
    return rng.integers(0, 1024, (T, n // 2)).astype("<u2").view(np.uint8).reshape(T, n)
