"""Host references of the noise-level function, numpy only: the band histograms ``sn_yuv_noise_hist_bands`` must equal exactly, the histogram ->
curve definition restated on its own (plain loops, float64), the float32 restatement ``sn_noise_map_level`` must equal bit for bit (in the order
include/shiftnet_hip.h states), and the synthetic clips with INJECTED signal-dependent noise that the curve is judged against.
``tests/yuv_ref.py`` supplies the payload layout, ``tests/noise_ref.py`` the flat statistic."""
from __future__ import annotations

import math

import numpy as np

import noise_ref as N
import yuv_ref as R

BANDS = 16
MIN_BLOCKS = 1024
f32 = np.float32


def nbv(bits: int) -> int:
    return 128 if bits == 8 else 512


def luma_of(payload: np.ndarray, fmt: R.Fmt, H: int, W: int, rect=None) -> np.ndarray:
    """The picture's luma codes, int64 [h, w]: the whole frame or rect = (x0, y0, w, h) of it."""
    Y = R.split_planes(np.ascontiguousarray(payload), fmt, H, W)[0]
    if rect is None:
        return Y
    x0, y0, w, h = rect
    return Y[y0:y0 + h, x0:x0 + w]


def hist_bands_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, lo: int, hi: int, rect=None) -> np.ndarray:
    """uint8 [T, frame_bytes] -> uint32 [T, 16, NBV]: per band of S = a + b + c + d the counts of min(|a - b - c + d|, NBV - 1) over the whole
    2 x 2 luma blocks of the picture whose codes all lie in (lo, hi)."""
    nb = nbv(fmt.bits)
    out = np.zeros((len(payloads), BANDS, nb), np.uint32)
    for t, p in enumerate(payloads):
        Y = luma_of(p, fmt, H, W, rect)
        hb, wb = Y.shape[0] // 2, Y.shape[1] // 2
        a, b = Y[0:2 * hb:2, 0:2 * wb:2], Y[0:2 * hb:2, 1:2 * wb:2]
        c, d = Y[1:2 * hb:2, 0:2 * wb:2], Y[1:2 * hb:2, 1:2 * wb:2]
        ok = np.ones(a.shape, bool)
        for q in (a, b, c, d):
            ok &= (q > lo) & (q < hi)
        v = np.minimum(np.abs(a - b - c + d), nb - 1)[ok]
        band = (((a + b + c + d) - 4 * lo) * 16)[ok] // (4 * (hi - lo)) if ok.any() else np.zeros(0, np.int64)
        assert band.size == 0 or (0 <= band.min() and band.max() <= BANDS - 1)
        out[t] = np.bincount(band * nb + v, minlength=BANDS * nb).reshape(BANDS, nb)
    return out


def knot_codes(lo: int, hi: int):
    return [lo + (b + 0.5) * (hi - lo) / BANDS for b in range(BANDS)]


def curve_ref(band_hists, fmt: R.Fmt, clamp=(0.0, 50.0)):
    """The definition, with plain loops: the window's histograms summed; per band the median bin; no estimate below MIN_BLOCKS blocks or with the
    median in the last bin; the flat definition (noise_ref.sigma_ref) otherwise; holes filled linearly in the band index, constant beyond the
    outermost estimates, all zero if there is none; clamped."""
    h = np.asarray(band_hists).astype(np.int64)
    h = h.reshape(-1, BANDS, h.shape[-1]).sum(axis=0)
    est = []
    for b in range(BANDS):
        row = [int(x) for x in h[b]]
        n = sum(row)
        if n < MIN_BLOCKS:
            est.append(None)
            continue
        cum, k = 0, 0
        for k, c in enumerate(row):
            if cum + c >= n / 2:
                break
            cum += c
        est.append(None if k == len(row) - 1 else N.sigma_ref(row, fmt))
    have = [b for b in range(BANDS) if est[b] is not None]
    out = []
    for b in range(BANDS):
        if not have:
            v = 0.0
        elif est[b] is not None:
            v = est[b]
        elif b < have[0]:
            v = est[have[0]]
        elif b > have[-1]:
            v = est[have[-1]]
        else:
            i = [x for x in have if x < b][-1]
            j = [x for x in have if x > b][0]
            v = est[i] + (est[j] - est[i]) * (b - i) / (j - i)
        out.append(min(max(v, clamp[0]), clamp[1]))
    return out


def knots32(curve) -> np.ndarray:
    """The curve as the kernel takes it: sigma / 255 in float64, rounded once to float32."""
    return (np.asarray(curve, np.float64) / 255.0).astype(f32)


def block_means(Y: np.ndarray) -> np.ndarray:
    """float32 [ceil(h/8), ceil(w/8)]: float(sum) / float(count) of every aligned 8 x 8 block, partial at the far edges."""
    h, w = Y.shape
    nby, nbx = (h + 7) // 8, (w + 7) // 8
    M = np.zeros((nby, nbx), f32)
    for j in range(nby):
        for i in range(nbx):
            blk = Y[8 * j:8 * j + 8, 8 * i:8 * i + 8]
            M[j, i] = f32(int(blk.sum())) / f32(blk.size)
    return M


def _axis(n_out: int, n: int, nb: int):
    e = np.minimum(np.arange(n_out), n - 1)
    num = 2 * e - 7                                            # (e - 3.5) / 8 in sixteenths
    i0 = num >> 4                                              # floor
    a = (num - 16 * i0).astype(f32) * f32(0.0625)
    return np.clip(i0, 0, nb - 1), np.clip(i0 + 1, 0, nb - 1), a


def map_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, Hp: int, Wp: int, knots, lo: int, hi: int, dtype: str = "fp32", rect=None) -> np.ndarray:
    """-> [T, 1, Hp, Wp] in the stored form of ``dtype`` (yuv_ref.to_dtype_bits); knots: 16 float32 (sigma / 255)."""
    k = np.asarray(knots, f32)
    assert k.shape == (BANDS,) and k.dtype == f32
    s = f32(16.0 / (float(hi) - float(lo)))
    out = []
    for p in payloads:
        Y = luma_of(p, fmt, H, W, rect)
        h, w = Y.shape
        M = block_means(Y)
        j0, j1, ay = _axis(Hp, h, M.shape[0])
        i0, i1, ax = _axis(Wp, w, M.shape[1])
        ax, ay = ax[None, :], ay[:, None]
        m00, m01 = M[j0[:, None], i0[None, :]], M[j0[:, None], i1[None, :]]
        m10, m11 = M[j1[:, None], i0[None, :]], M[j1[:, None], i1[None, :]]
        top = m00 + ax * (m01 - m00)
        bot = m10 + ax * (m11 - m10)
        m = top + ay * (bot - top)
        u = np.minimum(np.maximum((m - f32(lo)) * s - f32(0.5), f32(0)), f32(15))
        i = np.minimum(np.floor(u).astype(np.int64), BANDS - 2)
        f = u - i.astype(f32)
        val = k[i] + f * (k[i + 1] - k[i])
        assert val.dtype == f32
        out.append(val[None])
    return R.to_dtype_bits(np.stack(out), dtype)


# ---- the synthetic clip with injected signal-dependent noise ---------------------------------------------------------------------------------
FMT = R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED)
RAMP = dict(h=96, w=256, t=6, seed=7, s_black=6.0, s_white=2.0)       # sigma of the LUMA codes at the black and at the white code, affine between


def luma_to_rgb_sigma(s_luma: float, fmt: R.Fmt) -> float:
    """Sigma of the luma codes -> the sigma of i.i.d. noise on 8-bit R'G'B' with that luma noise (the unit of the curve)."""
    kr, kb = (0.2126, 0.0722) if fmt.matrix == R.BT709 else (0.299, 0.114)
    g = math.sqrt(kr ** 2 + (1.0 - kr - kb) ** 2 + kb ** 2)
    sc = ((1 << fmt.bits) - 1) / 255.0 if fmt.range == R.FULL else 219.0 * (1 << (fmt.bits - 8)) / 255.0
    return s_luma / (g * sc)


def injected_sigma(code, fmt: R.Fmt = FMT, s_black: float = RAMP["s_black"], s_white: float = RAMP["s_white"]):
    """The injected function: sigma in 8-bit R'G'B' units at luma code ``code``."""
    lo, hi = N.clip_codes(fmt)
    return luma_to_rgb_sigma(s_black + (s_white - s_black) * (np.asarray(code, np.float64) - lo) / (hi - lo), fmt)


def ramp_payloads(fmt: R.Fmt = FMT, s_black: float = RAMP["s_black"], s_white: float = RAMP["s_white"], seed: int = RAMP["seed"]) -> np.ndarray:
    """T frames of h x w: a horizontal luma ramp from the black to the white code (every band has its share of columns) plus Gaussian noise whose
    sigma is the affine function of the clean code above, rounded and clipped to the sample range; grey chroma."""
    c = RAMP
    lo, hi = N.clip_codes(fmt)
    top = (1 << fmt.bits) - 1
    rng = np.random.default_rng(seed)
    clean = np.broadcast_to(lo + (hi - lo) * (np.arange(c["w"]) + 0.5) / c["w"], (c["h"], c["w"]))
    sig = s_black + (s_white - s_black) * (clean - lo) / (hi - lo)
    ch, cw = R.chroma_shape(fmt, c["h"], c["w"])
    grey = np.full((ch, cw), 128 << (fmt.bits - 8), np.int64)
    out = []
    for _ in range(c["t"]):
        Y = np.clip(np.rint(clean + rng.normal(0.0, 1.0, clean.shape) * sig), 0, top).astype(np.int64)
        out.append(R.join_planes(Y, grey, grey, fmt))
    return np.stack(out)
