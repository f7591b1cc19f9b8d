"""Host references of the Y'CbCr edges (csrc/sn_yuv.hip), numpy only.

Two implementations of both directions:
  ``*_f64``  the BT.601 / BT.709 definition in float64 (the reference the arithmetic is judged against);
  ``*_emu``  float32 in exactly the order include/shiftnet_hip.h states (what the kernels must equal bit for bit).
numpy's float32 operators round every product and sum separately, which is the kernels' "no FMA" rule.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Fmt = namedtuple("Fmt", "bits chroma matrix range")     # the integer codes of sn_yuv_fmt
C444, C420_CENTER, C420_LEFT = 0, 1, 2
BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
f32 = np.float32


def constants(fmt: Fmt) -> dict:
    """The float64 expressions of make_consts() in csrc/sn_yuv.hip, term for term; '32' holds each rounded once to float32."""
    kr, kb = (0.2126, 0.0722) if fmt.matrix == BT709 else (0.299, 0.114)
    kg = 1.0 - kr - kb
    s, top = 1 << (fmt.bits - 8), (1 << fmt.bits) - 1
    full = fmt.range == FULL
    yo, ys, cs, co = (0.0 if full else 16.0 * s), (float(top) if full else 219.0 * s), (float(top) if full else 224.0 * s), 128.0 * s
    d = dict(kr=kr, kg=kg, kb=kb, yo=yo, ys=ys, cs=cs, co=co,
             ky=1.0 / ys, crv=2.0 * (1.0 - kr) / cs, cgu=-2.0 * kb * (1.0 - kb) / kg / cs, cgv=-2.0 * kr * (1.0 - kr) / kg / cs,
             cbu=2.0 * (1.0 - kb) / cs, cu=1.0 / (2.0 * (1.0 - kb)), cv=1.0 / (2.0 * (1.0 - kr)))
    d["32"] = {k: f32(v) for k, v in d.items()}
    d.update(ylo=0 if full else 16 * s, yhi=top if full else 235 * s, clo=0 if full else 16 * s, chi=top if full else 240 * s)
    return d


def chroma_shape(fmt: Fmt, H: int, W: int):
    return (H, W) if fmt.chroma == C444 else ((H + 1) // 2, (W + 1) // 2)


def frame_bytes(fmt: Fmt, H: int, W: int) -> int:
    ch, cw = chroma_shape(fmt, H, W)
    return (H * W + 2 * ch * cw) * (1 if fmt.bits == 8 else 2)


def split_planes(payload: np.ndarray, fmt: Fmt, H: int, W: int):
    """payload: uint8 [frame_bytes] -> (Y [H,W], U, V [ch,cw]) int64."""
    ch, cw = chroma_shape(fmt, H, W)
    a = payload.view("<u2") if fmt.bits == 10 else payload
    a = a.astype(np.int64)
    return a[:H * W].reshape(H, W), a[H * W:H * W + ch * cw].reshape(ch, cw), a[H * W + ch * cw:].reshape(ch, cw)


def join_planes(Y, U, V, fmt: Fmt) -> np.ndarray:
    a = np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)])
    return a.astype("<u2").view(np.uint8) if fmt.bits == 10 else a.astype(np.uint8)


# ---- per-sample conversions (arrays of equal shape) ---------------------------------------------------------------------------------
def yuv_to_rgb_f64(Y, U, V, fmt: Fmt, clamp: bool = False):
    """The definition: E'y = (Y - yo) / ys, E'cb = (U - co) / cs, E'cr likewise; R = E'y + 2 (1 - Kr) E'cr, B = E'y + 2 (1 - Kb) E'cb,
    G = (E'y - Kr R - Kb B) / Kg.  U, V may be fractional (upsampled) codes."""
    c = constants(fmt)
    y = (np.asarray(Y, np.float64) - c["yo"]) / c["ys"]
    u = (np.asarray(U, np.float64) - c["co"]) / c["cs"]
    v = (np.asarray(V, np.float64) - c["co"]) / c["cs"]
    r = y + 2.0 * (1.0 - c["kr"]) * v
    b = y + 2.0 * (1.0 - c["kb"]) * u
    g = (y - c["kr"] * r - c["kb"] * b) / c["kg"]
    out = np.stack([r, g, b])
    return np.clip(out, 0.0, 1.0) if clamp else out


def yuv_to_rgb_emu(Y, Un, Vn, den: int, fmt: Fmt, clamp: bool = True):
    """float32 in the kernel's order; Un, Vn: integer chroma numerators over den (1, 8 or 16)."""
    k = constants(fmt)["32"]
    c = constants(fmt)
    yd = (np.asarray(Y, np.int64) - int(c["yo"])).astype(f32)
    ud = (np.asarray(Un, np.int64) - den * int(c["co"])).astype(f32) * f32(1.0 / den)
    vd = (np.asarray(Vn, np.int64) - den * int(c["co"])).astype(f32) * f32(1.0 / den)
    yy = k["ky"] * yd
    r = yy + k["crv"] * vd
    g = (yy + k["cgu"] * ud) + k["cgv"] * vd
    b = yy + k["cbu"] * ud
    out = np.stack([r, g, b])
    assert out.dtype == f32
    return np.clip(out, f32(0), f32(1)) if clamp else out


def _ycc_f64(rgb, c):
    r, g, b = (np.clip(np.asarray(a, np.float64), 0.0, 1.0) for a in rgb)
    y = c["kr"] * r + c["kg"] * g + c["kb"] * b
    return y, (b - y) / (2.0 * (1.0 - c["kb"])), (r - y) / (2.0 * (1.0 - c["kr"]))


def _ycc_emu(rgb, k):
    r, g, b = (np.clip(np.asarray(a, f32), f32(0), f32(1)) for a in rgb)
    y = (k["kr"] * r + k["kg"] * g) + k["kb"] * b
    return y, (b - y) * k["cu"], (r - y) * k["cv"]


def quant_f64(y, u, v, fmt: Fmt):
    """-> (unrounded code values float64 [3,...], codes int64 [3,...])."""
    c = constants(fmt)
    raw = np.stack([c["yo"] + c["ys"] * y, c["co"] + c["cs"] * u, c["co"] + c["cs"] * v])
    q = np.rint(raw).astype(np.int64)
    q[0] = np.clip(q[0], c["ylo"], c["yhi"])
    q[1:] = np.clip(q[1:], c["clo"], c["chi"])
    return raw, q


def quant_emu(y, u, v, fmt: Fmt):
    c = constants(fmt)
    k = c["32"]
    raw = np.stack([k["yo"] + k["ys"] * y, k["co"] + k["cs"] * u, k["co"] + k["cs"] * v])
    assert raw.dtype == f32
    q = np.rint(raw).astype(np.int64)
    q[0] = np.clip(q[0], c["ylo"], c["yhi"])
    q[1:] = np.clip(q[1:], c["clo"], c["chi"])
    return raw, q


def rgb_to_yuv444_f64(rgb, fmt: Fmt):
    return quant_f64(*_ycc_f64(rgb, constants(fmt)), fmt)


def rgb_to_yuv444_emu(rgb, fmt: Fmt):
    return quant_emu(*_ycc_emu(rgb, constants(fmt)["32"]), fmt)


# ---- whole frames -------------------------------------------------------------------------------------------------------------------
def _clampi(a, n):
    return np.clip(a, 0, n - 1)


def upsample_num(C: np.ndarray, chroma: int, ye: np.ndarray, xe: np.ndarray):
    """Integer bilinear numerators of chroma plane C at luma coordinates (ye[:,None], xe[None,:]); returns (num, den)."""
    if chroma == C444:
        return C[ye[:, None], xe[None, :]], 1
    ch, cw = C.shape
    j, i = ye >> 1, xe >> 1
    jn = _clampi(j + np.where(ye & 1, 1, -1), ch)
    vr = 3 * C[j] + C[jn]                                   # [len(ye), cw]
    if chroma == C420_CENTER:
        i_n = _clampi(i + np.where(xe & 1, 1, -1), cw)
        return 3 * vr[:, i] + vr[:, i_n], 16
    i1 = _clampi(i + 1, cw)
    return np.where((xe & 1)[None, :], vr[:, i] + vr[:, i1], 2 * vr[:, i]), 8


def to_dtype_bits(x: np.ndarray, dtype: str) -> np.ndarray:
    """float32 -> the stored element: 'fp32' float32, 'fp16' float16, 'bf16' the uint16 bit pattern (all round to nearest even)."""
    if dtype == "fp32":
        return x
    if dtype == "fp16":
        return x.astype(np.float16)
    u = np.ascontiguousarray(x).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_dtype_bits(a: np.ndarray, dtype: str) -> np.ndarray:
    if dtype == "bf16":
        return (a.astype(np.uint32) << 16).view(f32)
    return a.astype(f32)


def _ingest(payloads: np.ndarray, fmt: Fmt, H, W, Hp, Wp, emu: bool):
    ye, xe = np.minimum(np.arange(Hp), H - 1), np.minimum(np.arange(Wp), W - 1)
    out = []
    for p in payloads:
        Y, U, V = split_planes(p, fmt, H, W)
        un, den = upsample_num(U, fmt.chroma, ye, xe)
        vn, _ = upsample_num(V, fmt.chroma, ye, xe)
        y = Y[ye[:, None], xe[None, :]]
        out.append(yuv_to_rgb_emu(y, un, vn, den, fmt) if emu else yuv_to_rgb_f64(y, un / den, vn / den, fmt, clamp=True))
    return np.stack(out)


def ingest_emu(payloads: np.ndarray, fmt: Fmt, H: int, W: int, Hp: int, Wp: int, dtype: str = "fp32") -> np.ndarray:
    """payloads: uint8 [T, frame_bytes] -> [T,3,Hp,Wp] in the stored form of ``dtype`` (to_dtype_bits)."""
    return to_dtype_bits(_ingest(payloads, fmt, H, W, Hp, Wp, True), dtype)


def ingest_f64(payloads: np.ndarray, fmt: Fmt, H: int, W: int, Hp: int, Wp: int) -> np.ndarray:
    return _ingest(payloads, fmt, H, W, Hp, Wp, False)


def _down(c: np.ndarray, chroma: int, H: int, W: int, emu: bool):
    """c: [H,W] chroma at luma resolution -> [ch,cw], coordinates clamped to the frame."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    y0, y1 = 2 * np.arange(ch), np.minimum(2 * np.arange(ch) + 1, H - 1)
    xc, xr = 2 * np.arange(cw), np.minimum(2 * np.arange(cw) + 1, W - 1)
    a, b = c[y0], c[y1]
    q, e, two = (f32(0.25), f32(0.125), f32(2)) if emu else (0.25, 0.125, 2.0)
    if chroma == C420_CENTER:
        return q * ((a[:, xc] + a[:, xr]) + (b[:, xc] + b[:, xr]))
    xl = np.maximum(xc - 1, 0)
    return e * (((a[:, xl] + two * a[:, xc]) + a[:, xr]) + ((b[:, xl] + two * b[:, xc]) + b[:, xr]))


def _egress(x: np.ndarray, fmt: Fmt, H: int, W: int, emu: bool) -> np.ndarray:
    c = constants(fmt)
    out = []
    for fr in x:
        rgb = fr[:, :H, :W]
        y, u, v = _ycc_emu(rgb, c["32"]) if emu else _ycc_f64(rgb, c)
        if fmt.chroma != C444:
            u, v = _down(u, fmt.chroma, H, W, emu), _down(v, fmt.chroma, H, W, emu)
        k = c["32"] if emu else c
        rnd = lambda off, sc, a, lo, hi: np.clip(np.rint(off + sc * a).astype(np.int64), lo, hi)   # noqa: E731
        out.append(join_planes(rnd(k["yo"], k["ys"], y, c["ylo"], c["yhi"]), rnd(k["co"], k["cs"], u, c["clo"], c["chi"]),
                               rnd(k["co"], k["cs"], v, c["clo"], c["chi"]), fmt))
    return np.stack(out)


def egress_emu(x: np.ndarray, fmt: Fmt, H: int, W: int) -> np.ndarray:
    """x: float32 [T,3,Hp,Wp] (the values the kernel reads, i.e. already rounded to the tensor's dtype) -> uint8 [T, frame_bytes]."""
    assert x.dtype == f32
    return _egress(x, fmt, H, W, True)


def egress_f64(x: np.ndarray, fmt: Fmt, H: int, W: int) -> np.ndarray:
    return _egress(np.asarray(x, np.float64), fmt, H, W, False)
