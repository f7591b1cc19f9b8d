"""Host references of the temporal noise estimate, numpy only: the two histograms of frame pairs that ``sn_yuv_noise_hist_pairs`` and
``sn_yuv_noise_hist_pairs_bands`` must equal exactly (rectangle included), the pair histogram -> sigma definition restated on its own (plain loops,
float64), a window's estimates from payloads as the restorer must report them, and the synthetic clips with INJECTED noise that the estimator is
judged against.  ``tests/yuv_ref.py`` supplies the payload layout, ``tests/noise_ref.py`` the spatial statistic and the noise
injection, ``tests/nlf_ref.py`` the spatial band histograms."""
from __future__ import annotations

import math

import numpy as np

import nlf_ref as F
import noise_ref as N
import yuv_ref as R

BANDS = 16


def nbp(bits: int) -> int:
    return 4 * ((1 << bits) - 1) + 1


def _blocks(Y: np.ndarray):
    """The four codes of every whole 2 x 2 block of a luma plane (int64), the grid anchored at its first sample."""
    hb, wb = Y.shape[0] // 2, Y.shape[1] // 2
    return (Y[0:2 * hb:2, 0:2 * wb:2], Y[0:2 * hb:2, 1:2 * wb:2], Y[1:2 * hb:2, 0:2 * wb:2], Y[1:2 * hb:2, 1:2 * wb:2])


def _pair(p0, p1, fmt: R.Fmt, H: int, W: int, lo: int, hi: int, rect):
    """(v, S) of the blocks of one pair that count: all eight codes strictly between lo and hi."""
    q0, q1 = _blocks(F.luma_of(p0, fmt, H, W, rect)), _blocks(F.luma_of(p1, fmt, H, W, rect))
    ok = np.ones(q0[0].shape, bool)
    for q in q0 + q1:
        ok &= (q > lo) & (q < hi)
    v = np.abs((q1[0] - q1[1] - q1[2] + q1[3]) - (q0[0] - q0[1] - q0[2] + q0[3]))
    S = sum(q0) + sum(q1)
    return v[ok].reshape(-1), S[ok].reshape(-1)


def hist_rect_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, lo: int, hi: int, rect=None) -> np.ndarray:
    """noise_ref.hist_ref of the picture ``rect`` (None: the whole frame), the block grid anchored at its origin: uint32 [T, NB]."""
    out = np.zeros((len(payloads), N.nbins(fmt.bits)), np.uint32)
    for t, p in enumerate(payloads):
        a, b, c, d = _blocks(F.luma_of(p, fmt, H, W, rect))
        ok = np.ones(a.shape, bool)
        for q in (a, b, c, d):
            ok &= (q > lo) & (q < hi)
        out[t] = np.bincount(np.abs(a - b - c + d)[ok].reshape(-1), minlength=out.shape[1])
    return out


def hist_pairs_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, lo: int, hi: int, rect=None) -> np.ndarray:
    """uint8 [T, frame_bytes] -> uint32 [T - 1, NBP]: per pair (p, p + 1) the counts of |HH(p + 1) - HH(p)|, HH = a - b - c + d."""
    nb = nbp(fmt.bits)
    out = np.zeros((len(payloads) - 1, nb), np.uint32)
    for p in range(len(payloads) - 1):
        v, _ = _pair(payloads[p], payloads[p + 1], fmt, H, W, lo, hi, rect)
        out[p] = np.bincount(v, minlength=nb)
    return out


def band_of(S, lo: int, hi: int):
    """band = (2 (S - 8 lo)) / (hi - lo), integer division, for the sum S of the eight codes."""
    return (2 * (np.asarray(S, np.int64) - 8 * lo)) // (hi - lo)


def hist_pairs_bands_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, lo: int, hi: int, rect=None) -> np.ndarray:
    """uint8 [T, frame_bytes] -> uint32 [T - 1, 16, NBV]: the pair statistic saturated to NBV - 1, split by the band of the eight codes' sum."""
    nb = F.nbv(fmt.bits)
    out = np.zeros((len(payloads) - 1, BANDS, nb), np.uint32)
    for p in range(len(payloads) - 1):
        v, S = _pair(payloads[p], payloads[p + 1], fmt, H, W, lo, hi, rect)
        band = band_of(S, lo, hi)
        assert band.size == 0 or (0 <= band.min() and band.max() <= BANDS - 1)
        out[p] = np.bincount(band * nb + np.minimum(v, nb - 1), minlength=BANDS * nb).reshape(BANDS, nb)
    return out


def pair_sigma_ref(hist, fmt: R.Fmt):
    """The definition, with plain loops: None for an empty histogram and for one with nothing outside bin 0; otherwise the median of v with linear
    interpolation inside the bin -> variance less 2/3, over 8 -> sigma of 8-bit R'G'B'."""
    h = [int(x) for x in np.asarray(hist).tolist()]
    n = sum(h)
    if n == 0 or n == h[0]:
        return None
    cum = 0
    for k, c in enumerate(h):
        if cum + c >= n / 2:
            left, width = (0.0, 0.5) if k == 0 else (k - 0.5, 1.0)
            med = left + width * (n / 2 - cum) / c
            break
        cum += c
    var = max((med / 0.6744897501960817) ** 2 - 2.0 / 3.0, 0.0)
    kr, kb = (0.2126, 0.0722) if fmt.matrix == R.BT709 else (0.299, 0.114)
    g = math.sqrt(kr ** 2 + (1.0 - kr - kb) ** 2 + kb ** 2)
    s = ((1 << fmt.bits) - 1) / 255.0 if fmt.range == R.FULL else 219.0 * (1 << (fmt.bits - 8)) / 255.0
    return math.sqrt(var / 8.0) / (g * s)


# ---- what the restorer must report for a stream: the restatements through the functions of shiftnet_amd/noise.py ---------------------------------
def window_estimates(pay, fmt: R.Fmt, h: int, w: int, one_len: int, estimator: str, cuts=(), clamp=(0.0, 50.0), rect=None, level: bool = False):
    """dict of lists, one entry per window: frame_sigma, pair_sigma, spatial, temporal, sigma and (level) nlf, from the frames each window is fed."""
    from shiftnet_amd import noise
    lo, hi = N.clip_codes(fmt)
    out = dict(frame_sigma=[], pair_sigma=[], spatial=[], temporal=[], sigma=[], nlf=[])
    for idx in N.window_inputs(len(pay), one_len, cuts):
        stack = np.stack([pay[i] for i in idx])
        flat = hist_rect_ref(stack, fmt, h, w, lo, hi, rect)
        per = [noise.frame_sigma(x, fmt.bits, fmt.matrix, fmt.range) for x in flat]
        ps = [noise.pair_sigma(x, fmt.bits, fmt.matrix, fmt.range) for x in hist_pairs_ref(stack, fmt, h, w, lo, hi, rect)]
        spatial, temporal = noise.frames_median(per), noise.window_sigma_temporal(ps)
        out["frame_sigma"].append(per)
        out["pair_sigma"].append(ps)
        out["spatial"].append(spatial)
        out["temporal"].append(temporal)
        out["sigma"].append(noise.combine_sigma(spatial, temporal, estimator, clamp))
        if level:
            out["nlf"].append(noise.window_curve_pairs(F.hist_bands_ref(stack, fmt, h, w, lo, hi, rect), hist_pairs_bands_ref(stack, fmt, h, w, lo, hi, rect),
                                                       fmt.bits, fmt.matrix, fmt.range, estimator, clamp))
    return out


# ---- the clips of the accuracy table: 180 x 320, five frames, BT.709 limited 8 bit ---------------------------------------------
ACC = dict(h=180, w=320, t=5, sigmas=(2, 5, 10, 20, 30))
ACC_FMT = R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED)


def flat_clip(t: int, h: int, w: int) -> np.ndarray:
    return np.full((t, 3, h, w), 0.5)


def texture_clip(t: int, h: int, w: int, speed: int = 0) -> np.ndarray:
    """[t, 3, h, w] grey frames 0.5 + 0.15 sin(0.9 x) sin(1.1 y): pixel-scale texture; ``speed`` pixels to the right per frame (0: static)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([np.repeat((0.5 + 0.15 * np.sin(0.9 * (x - speed * k)) * np.sin(1.1 * y))[None], 3, axis=0) for k in range(t)])


CLIPS = {"flat 0.5": flat_clip, "static texture": texture_clip, "texture moving 1 px per frame": lambda t, h, w: texture_clip(t, h, w, 1)}


def clip_estimates(clip: str, s: float, seed: int = 0):
    """(spatial, temporal, min) of the clip with sigma s injected on R'G'B' as noise_ref.noisy_payloads injects it: the five frames are one window's
    input, the estimates are the unclamped ones of shiftnet_amd/noise.py."""
    from shiftnet_amd import noise
    c, fmt = ACC, ACC_FMT
    pay = N.noisy_payloads(CLIPS[clip](c["t"], c["h"], c["w"]), float(s), fmt, seed=seed)
    lo, hi = N.clip_codes(fmt)
    per = [noise.frame_sigma(x, fmt.bits, fmt.matrix, fmt.range) for x in N.hist_ref(pay, fmt, c["h"], c["w"], lo, hi)]
    ps = [noise.pair_sigma(x, fmt.bits, fmt.matrix, fmt.range) for x in hist_pairs_ref(pay, fmt, c["h"], c["w"], lo, hi)]
    spatial, temporal = noise.frames_median(per), noise.window_sigma_temporal(ps)
    return spatial, temporal, noise.combine_sigma(spatial, temporal, "min", (0.0, 1e9))


if __name__ == "__main__":                                        # the table of DESIGN.md 3.20
    for name in CLIPS:
        for s in ACC["sigmas"]:
            sp, te, mn = clip_estimates(name, s)
            print(f"{name:32s} sigma {s:2d}: spatial {sp:6.2f}  temporal {te:6.2f}  min {mn:6.2f}")
