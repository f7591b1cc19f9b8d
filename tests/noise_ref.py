"""Host references of the noise-level path, numpy only: the histogram ``sn_yuv_noise_hist`` must equal exactly, the histogram -> sigma
definition restated on its own (plain loops, float64), and the synthetic clips with INJECTED noise that the estimator is judged against
(DESIGN.md 3.14).  ``tests/yuv_ref.py`` supplies the payload layout and the egress arithmetic."""
from __future__ import annotations

import math

import numpy as np

import yuv_ref as R

SIGMAS = (0, 1, 2, 5, 10, 20, 30, 40, 50)
FORMATS = {                                                    # the three formats of the accuracy table; 4:4:4 and both 4:2:0 sitings
    "8-bit 709 limited 4:2:0": R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED),
    "8-bit 601 full 4:4:4": R.Fmt(8, R.C444, R.BT601, R.FULL),
    "10-bit 709 limited 4:2:0": R.Fmt(10, R.C420_LEFT, R.BT709, R.LIMITED),
}


def nbins(bits: int) -> int:
    return 2 * ((1 << bits) - 1) + 1


def clip_codes(fmt: R.Fmt):
    s = 1 << (fmt.bits - 8)
    return (0, (1 << fmt.bits) - 1) if fmt.range == R.FULL else (16 * s, 235 * s)


def hist_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, lo: int, hi: int) -> np.ndarray:
    """uint8 [T, frame_bytes] -> uint32 [T, NB]: counts of |a - b - c + d| over the whole 2 x 2 luma blocks whose codes all lie in (lo, hi)."""
    nb, hb, wb = nbins(fmt.bits), H // 2, W // 2
    out = np.zeros((len(payloads), nb), np.uint32)
    for t, p in enumerate(payloads):
        Y = R.split_planes(np.ascontiguousarray(p), fmt, H, W)[0]
        a, b = Y[0:2 * hb:2, 0:2 * wb:2], Y[0:2 * hb:2, 1:2 * wb:2]
        c, d = Y[1:2 * hb:2, 0:2 * wb:2], Y[1:2 * hb:2, 1:2 * wb:2]
        ok = np.ones(a.shape, bool)
        for q in (a, b, c, d):
            ok &= (q > lo) & (q < hi)
        v = np.abs(a - b - c + d)[ok]
        out[t] = np.bincount(v.reshape(-1), minlength=nb)
    return out


def sigma_ref(hist, fmt: R.Fmt):
    """The definition, with plain loops: median of v with linear interpolation inside the bin -> variance less 1/3 -> sigma of 8-bit R'G'B'."""
    h = [int(x) for x in np.asarray(hist).tolist()]
    n = sum(h)
    if n == 0:
        return None
    cum = 0
    for k, c in enumerate(h):
        if cum + c >= n / 2:
            left, width = (0.0, 0.5) if k == 0 else (k - 0.5, 1.0)
            med = left + width * (n / 2 - cum) / c
            break
        cum += c
    var = max((med / 0.6744897501960817) ** 2 - 1.0 / 3.0, 0.0)
    kr, kb = (0.2126, 0.0722) if fmt.matrix == R.BT709 else (0.299, 0.114)
    g = math.sqrt(kr ** 2 + (1.0 - kr - kb) ** 2 + kb ** 2)
    s = ((1 << fmt.bits) - 1) / 255.0 if fmt.range == R.FULL else 219.0 * (1 << (fmt.bits - 8)) / 255.0
    return math.sqrt(var) / 2.0 / (g * s)


# ---- clean clips and injected noise ------------------------------------------------------------------------------------------------------
def smooth_rgb(h: int, w: int, phase: float = 0.0) -> np.ndarray:
    """[3, h, w] float64 in [0.3, 0.7]: a sinusoidal field with periods of hundreds of pixels, a different phase per channel."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([0.5 + 0.2 * np.sin(2 * np.pi * (x / 400.0 + 0.13 * c) + phase) * np.cos(2 * np.pi * (y / 300.0) + 0.7 * c) for c in range(3)])


def checker_rgb(h: int, w: int, cell: int = 31) -> np.ndarray:
    """[3, h, w] float64: flat cells of 31 x 31 pixels (an odd size, so that 2 x 2 blocks straddle the edges), levels 0.35 and 0.65."""
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((0.35 + 0.3 * (((y // cell) + (x // cell)) & 1))[None].astype(np.float64), 3, axis=0)


CLIPS = {"smooth": smooth_rgb, "checkerboard": checker_rgb, "flat 0.5": lambda h, w: np.full((3, h, w), 0.5)}


def noisy_payloads(rgb: np.ndarray, s: float, fmt: R.Fmt, seed: int = 0) -> np.ndarray:
    """rgb: [T, 3, h, w] clean frames in [0, 1] -> + N(0, s / 255) per channel, clipped to [0, 1], as payloads of ``yuv_ref.egress_emu``."""
    rng = np.random.default_rng(seed)
    x = np.clip(rgb + rng.normal(0.0, 1.0, rgb.shape) * (s / 255.0), 0.0, 1.0).astype(np.float32)
    return R.egress_emu(x, fmt, rgb.shape[2], rgb.shape[3])


def margin(s: float) -> float:
    """|estimate - injected| allowed for s <= 30: about 2.5 times what the definition alone produced on 1280 x 720."""
    return max(0.25, 0.03 * s)


# ---- the clip of the restorer's two-level test (tests/test_gpu_noise.py; its host figures are checked in tests/test_host_noise.py) ----------
TWO_LEVEL = dict(n=26, h=143, w=201, one_len=5, split=13, sigmas=(5.0, 30.0))
FMT420 = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)


def two_level_payloads() -> np.ndarray:
    """26 frames of the smooth field drifting slowly; frames 0 .. 12 carry sigma 5, frames 13 .. 25 sigma 30."""
    c = TWO_LEVEL
    rgb = np.stack([smooth_rgb(c["h"], c["w"], 0.05 * t) for t in range(c["n"])])
    a = noisy_payloads(rgb[:c["split"]], c["sigmas"][0], FMT420, seed=1)
    b = noisy_payloads(rgb[c["split"]:], c["sigmas"][1], FMT420, seed=2)
    return np.concatenate([a, b])


def window_inputs(n: int, one_len: int, cuts=()):
    """The input frame indices of every window, as shiftnet_amd.restore plans them."""
    from shiftnet_amd import restore
    plan = restore.plan_scene_windows(n, one_len, cuts) if cuts else restore.plan_windows(n, one_len)
    return [idx for _, _, idx in plan]
