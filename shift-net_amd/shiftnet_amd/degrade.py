"""The noise that ``restore_video --add_noise`` adds to a clean stream, host side (numpy only, no torch): the table ``sn_yuv_degrade``
(csrc/sn_degrade.hip) looks its Gaussian samples up in, the option's grammar, and the field of samples itself as numpy restates it.

The experiment is upstream's (``in_tensor + normal_(0, sigma)``, inference/test_denoise*.py) on footage: a clean stream, a degraded copy, its
restoration compared with the clean one.  The noise is i.i.d. per R'G'B' channel and pixel, added between the two colour edges, its sigma a curve
of 16 knots (``noise.knot_codes``) at the pixel's own clean luma code: a number is 16 equal knots.  A sample is ``gauss[h >> 16]`` of an integer
hash h of (seed, frame number in the stream, channel, row, column) -- the hash of the egress' dither on planes 3 .. 5 of the same seed space -- so
every frame carries the same noise wherever and however often it is fed, and numpy gives the kernel's bits.

Limits, stated plainly: the table has 65536 entries, so the tails end at about 4.3 sigma; the noise models what the networks were trained with,
not a sensor and a codec.

The second half of the file is the same for ``--add_blur`` and the deblurrers: the gamma tables ``sn_yuv_blur`` (csrc/sn_blur.hip) averages
consecutive frames in linear light with, the option's grammar, and the plan of the stage's launches."""
from __future__ import annotations

import functools
import math
import statistics
from typing import List

import numpy as np

from .noise import NLF_BANDS, check_sigmas

TABLE = 1 << 16


@functools.lru_cache(maxsize=1)
def _gauss_table() -> np.ndarray:
    nd = statistics.NormalDist()
    q = np.array([nd.inv_cdf((k + 0.5) / TABLE) for k in range(TABLE)], np.float64)
    t = (q / math.sqrt(float(np.mean(q * q)))).astype(np.float32)
    t.setflags(write=False)
    return t


def gauss_table() -> np.ndarray:
    """float32 [65536]: entry k is the standard normal quantile at (k + 0.5) / 65536, in float64, divided by the root mean square of the 65536
    quantiles, then rounded: mean 0, variance 1, antisymmetric, the largest about 4.3.  Made once; read-only."""
    return _gauss_table()


def parse_add_noise(text: str) -> List[float]:
    """--add_noise: SIGMA -> 16 equal knots; s0,...,s15 -> the curve, sigma of 8-bit R'G'B' codes at 16 luma levels from black to white.  All finite
    and >= 0; anything else is a ValueError."""
    words = [w.strip() for w in str(text).split(",")]
    if len(words) not in (1, NLF_BANDS):
        raise ValueError(f"a number or {NLF_BANDS} comma-separated numbers, got {text!r}")
    try:
        vals = check_sigmas([float(w) for w in words])
    except ValueError:
        raise ValueError(f"a number or {NLF_BANDS} comma-separated numbers, each finite and >= 0, got {text!r}") from None
    return vals * NLF_BANDS if len(vals) == 1 else vals


def add_noise_form(add_noise, add_noise_seed=0):
    """The restorer's ``add_noise`` / ``add_noise_seed`` -> (None, seed) or (the 16 knots, seed); ValueError for anything else."""
    seed = int(add_noise_seed)
    if isinstance(add_noise_seed, bool) or seed != add_noise_seed or not (0 <= seed < 2 ** 32):
        raise ValueError(f"add_noise_seed must be an integer in 0 .. 2^32 - 1, got {add_noise_seed!r}")
    if add_noise is None:
        return None, seed
    try:
        knots = check_sigmas(add_noise if hasattr(add_noise, "__iter__") and not isinstance(add_noise, (str, bytes)) else [add_noise])
    except (TypeError, ValueError):
        knots = []
    if len(knots) not in (1, NLF_BANDS):
        raise ValueError(f"add_noise must be a number or {NLF_BANDS} numbers, each finite and >= 0 (sigma of 8-bit R'G'B' codes), got {add_noise!r}")
    return (knots * NLF_BANDS if len(knots) == 1 else knots), seed


# ---- motion blur (``--add_blur``): the same experiment for the deblurrers -------------------------------------------------------------
# The deblur datasets (GOPRO, DVD) average consecutive frames of a sharp high-frame-rate stream -- GOPRO in linear light, through an inverse gamma of
# 2.2 -- and keep the sharp centre frame for the truth.  ``sn_yuv_blur`` (csrc/sn_blur.hip) does that between the two colour edges; here are the
# tables it walks into linear light and back with, the option's grammar, and the plan of its launches.
BLUR_MAX_TAPS = 15
GAMMA_LEVELS = 4096


@functools.lru_cache(maxsize=8)
def _gamma_tables(g: float):
    lin = ((np.arange(GAMMA_LEVELS, dtype=np.float64) / (GAMMA_LEVELS - 1)) ** g).astype(np.float32)
    rinv = (1.0 / np.diff(lin.astype(np.float64))).astype(np.float32)
    for t in (lin, rinv):
        t.setflags(write=False)
    return lin, rinv


def gamma_tables(g: float):
    """(lin float32 [4096], rinv float32 [4095]): lin[k] = (k / 4095) ** g in float64, rounded once, strictly increasing from 0 to 1;
    rinv[k] = 1 / (lin[k + 1] - lin[k]) in float64 on the rounded lin, rounded once.  g finite in [1, 3].  Made once per g; read-only."""
    g = float(g)
    if not (1.0 <= g <= 3.0):
        raise ValueError(f"a gamma in [1, 3], got {g!r}")
    return _gamma_tables(g)


def parse_add_blur(text: str) -> int:
    """--add_blur: N, the number of consecutive frames averaged: an odd integer 1 .. 15; anything else is a ValueError."""
    try:
        n = int(str(text).strip())
    except ValueError:
        n = 0
    if not (1 <= n <= BLUR_MAX_TAPS and n % 2 == 1):
        raise ValueError(f"an odd number of frames, 1 .. {BLUR_MAX_TAPS}, got {text!r}")
    return n


def add_blur_form(add_blur, add_blur_gamma=2.2):
    """The restorer's ``add_blur`` / ``add_blur_gamma`` -> (None, gamma) or (n, gamma); gamma exactly 1.0 means no tables.  ValueError for anything
    else."""
    try:
        g = float(add_blur_gamma)
    except (TypeError, ValueError):
        g = math.nan
    if isinstance(add_blur_gamma, (bool, str, bytes)) or not (1.0 <= g <= 3.0):
        raise ValueError(f"add_blur_gamma must be a finite number in [1, 3], got {add_blur_gamma!r}")
    if add_blur is None:
        return None, g
    ok = not isinstance(add_blur, (bool, str, bytes, float)) and hasattr(add_blur, "__index__")
    n = int(add_blur) if ok else 0
    if not (1 <= n <= BLUR_MAX_TAPS and n % 2 == 1):
        raise ValueError(f"add_blur must be an odd integer 1 .. {BLUR_MAX_TAPS} (frames averaged), got {add_blur!r}")
    return n, g


def plan_blur(first: int, count: int, n: int, cuts, last: int, ended: bool):
    """The launches of ``sn_yuv_blur`` for output frames first .. first + count - 1 of a stream: [(first output, count, lo, hi)] in stream indices, one
    per scene segment of the chunk, in order; [lo, hi] is what the averaging window is clamped to, the frame's scene cut down to the stream.
    ``cuts``: the listed scene starts (strictly increasing, >= 1) or None / () for one scene.  ``last``: the index of the last frame known to exist;
    ``ended``: it is the stream's last.  While the stream has not ended the caller has read r = n // 2 frames past the chunk, so no window is
    clamped at a frame that merely has not been read yet; a plan that would is a ValueError."""
    r = n // 2
    end = first + count - 1
    if count < 1 or first < 0 or last < end or (not ended and last < end + r):
        raise ValueError(f"outputs {first} .. {end} with frames known up to {last}{'' if ended else ' of a stream that goes on'}: {r} more are needed")
    starts = [0] + [c for c in (cuts or ()) if c <= last]
    out = []
    for k, lo in enumerate(starts):
        hi = starts[k + 1] - 1 if k + 1 < len(starts) else last
        a, b = max(first, lo), min(end, hi)
        if a <= b:
            out.append((a, b - a + 1, lo, hi))
    return out


def noise_field(seed: int, f0: int, T: int, H: int, W: int) -> np.ndarray:
    """float32 [T, 3, H, W]: g(f, c, y, x) of frames f0 .. f0 + T - 1 as include/shiftnet_hip.h states it under sn_yuv_degrade."""
    u = np.uint32
    f = (np.arange(T, dtype=np.uint32) + u(f0 & 0xFFFFFFFF))[:, None, None, None]
    c = np.arange(3, dtype=np.uint32)[None, :, None, None]
    y = np.arange(H, dtype=np.uint32)[None, None, :, None]
    x = np.arange(W, dtype=np.uint32)[None, None, None, :]
    with np.errstate(over="ignore"):
        k = (y * u(0x9E3779B1)) ^ (x * u(0x85EBCA77)) ^ (f * u(0xC2B2AE3D)) ^ ((c + u(3)) * u(0x27D4EB2F)) ^ u(seed & 0xFFFFFFFF)
        k ^= k >> u(16)
        k = k * u(0x85EBCA6B)
        k ^= k >> u(13)
        k = k * u(0xC2B2AE35)
        k ^= k >> u(16)
    return gauss_table()[k >> u(16)]
