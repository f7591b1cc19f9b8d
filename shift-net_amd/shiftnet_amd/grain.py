"""The grain that ``restore_video --grain`` puts back on the stream it writes, host side (numpy only, no torch): the option's grammar, the taps of the
filter that gives the grain its size, and the conversion of a level from the unit of ``--sigma`` to luma codes of the format written.  The kernel is
``sn_yuv_grain`` (csrc/sn_grain.hip; the arithmetic is stated in include/shiftnet_hip.h).

A fully denoised picture looks waxy and bands; the usual delivery chain is "denoise, encode, re-grain".  The grain is a Gaussian field: a white field
-- ``gauss[h >> 16]`` of the hash that keys the dither and ``--add_noise``, on planes 6 .. 8 of the same seed space -- under a separable 5-tap Gaussian
filter of unit energy, so ``grain_size`` changes the grain's size and not its level.  Its level is a curve of 16 knots at the written luma code, in the
unit ``--sigma`` and ``--add_noise`` use: the sigma of i.i.d. noise on 8-bit R'G'B' whose LUMA part the grain equals.  ``auto`` is a share of what the
window was restored with.

Limits, stated plainly: a Gaussian field of a size the user chooses, **not a model fitted to the removed noise** -- no AR fit, no film-grain table for an
encoder; the level is a function of the written luma code alone; the field is independent from frame to frame; under ``auto`` it steps at window
boundaries with the estimate; codes are integers, so the grain itself is rounded (variance L^2 + 1/12) and clipped at the legal range; 4:2:0 chroma
grain lives at chroma resolution and looks twice the size; the chroma share is a plain factor.  Nobody has judged it on real footage."""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

from .noise import NLF_BANDS, check_sigmas, code_scale, luma_gain

DEFAULT_SHARE = 0.5
MAX_SHARE = 4.0
MAX_SIZE = 1.2                              # beyond it a 5-tap window cuts too much of the Gaussian off


def _share(word) -> float:
    try:
        s = math.nan if isinstance(word, bool) else float(word)
    except (TypeError, ValueError):
        s = math.nan
    if not (0.0 <= s <= MAX_SHARE):
        raise ValueError(f"a share in [0, {MAX_SHARE:g}], got {word!r}")
    return s


def parse_grain(text: str):
    """--grain: SIGMA -> 16 equal knots; s0,...,s15 -> the curve (sigma of 8-bit R'G'B' codes at 16 luma levels from black to white, each finite and
    >= 0); ``auto`` / ``auto:SHARE`` -> ("auto", share), SHARE in [0, 4] times what the window was restored with (default 0.5).  Anything else is a
    ValueError."""
    word = str(text).strip()
    if word == "auto" or word.startswith("auto:"):
        try:
            return "auto", (DEFAULT_SHARE if word == "auto" else _share(word[5:]))
        except ValueError as e:
            raise ValueError(f"auto or auto:SHARE with {e}") from None
    words = [w.strip() for w in word.split(",")]
    if len(words) not in (1, NLF_BANDS):
        raise ValueError(f"a number, {NLF_BANDS} comma-separated numbers, auto or auto:SHARE, got {text!r}")
    try:
        vals = check_sigmas([float(w) for w in words])
    except ValueError:
        raise ValueError(f"a number, {NLF_BANDS} comma-separated numbers (each finite and >= 0), auto or auto:SHARE, got {text!r}") from None
    return vals * NLF_BANDS if len(vals) == 1 else vals


def _number(name: str, v, lo: float, hi: float) -> float:
    try:
        f = math.nan if isinstance(v, (bool, str, bytes)) else float(v)
    except (TypeError, ValueError):
        f = math.nan
    if not (lo <= f <= hi):
        raise ValueError(f"{name} must be a finite number in [{lo:g}, {hi:g}], got {v!r}")
    return f


def grain_form(grain, grain_size=0.0, grain_chroma=0.0, grain_seed=0):
    """The restorer's ``grain`` / ``grain_size`` / ``grain_chroma`` / ``grain_seed`` -> (mode, value, size, chroma, seed): mode None (no grain; value
    None), ``"knots"`` (value: the 16 knots, sigma of 8-bit R'G'B' codes) or ``"auto"`` (value: the share).  ``grain``: None, a number, 16 numbers,
    ``"auto"``, ``"auto:SHARE"`` or what ``parse_grain`` returns.  ValueError for anything else, and for one of the other three without ``grain``."""
    size = _number("grain_size", grain_size, 0.0, MAX_SIZE)
    try:
        chroma = _number("grain_chroma", grain_chroma, 0.0, 3.0e38)      # anything a float32 holds
    except ValueError:
        raise ValueError(f"grain_chroma must be a finite number >= 0, got {grain_chroma!r}") from None
    ok = not isinstance(grain_seed, (bool, str, bytes, float)) and hasattr(grain_seed, "__index__")
    seed = int(grain_seed) if ok else -1
    if not (0 <= seed < 2 ** 32):
        raise ValueError(f"grain_seed must be an integer in 0 .. 2^32 - 1, got {grain_seed!r}")
    if grain is None:
        if size != 0.0 or chroma != 0.0 or seed != 0:
            raise ValueError("grain_size / grain_chroma / grain_seed shape the grain: they need grain")
        return None, None, size, chroma, seed
    if isinstance(grain, str):
        try:
            grain = parse_grain(grain)
        except ValueError as e:
            raise ValueError(f"grain: {e}") from None
    if isinstance(grain, tuple) and len(grain) == 2 and grain[0] == "auto":
        try:
            return "auto", _share(grain[1]), size, chroma, seed
        except ValueError as e:
            raise ValueError(f"grain: auto with {e}") from None
    try:
        knots = check_sigmas(grain if hasattr(grain, "__iter__") and not isinstance(grain, (str, bytes)) else [grain])
    except (TypeError, ValueError):
        knots = []
    if len(knots) not in (1, NLF_BANDS):
        raise ValueError(f"grain must be a number or {NLF_BANDS} numbers, each finite and >= 0 (sigma of 8-bit R'G'B' codes), 'auto' or 'auto:SHARE', "
                         f"got {grain!r}")
    return "knots", (knots * NLF_BANDS if len(knots) == 1 else knots), size, chroma, seed


def grain_taps(size: float) -> Tuple[float, float, float]:
    """(w0, w1, w2) of the separable filter (w2, w1, w0, w1, w2): ``w_k = exp(-k^2 / (2 size^2)) / sqrt(sum_k exp(-k^2 / size^2))``, k = -2 .. 2, in
    float64, each rounded once to float32: a Gaussian of standard deviation ``size`` samples, of unit energy, so the field keeps variance 1.  ``size``
    in [0, 1.2]; 0 gives (1, 0, 0), white grain."""
    size = _number("size", size, 0.0, MAX_SIZE)
    if size == 0.0:
        return 1.0, 0.0, 0.0
    e = [math.exp(-k * k / (2.0 * size * size)) for k in range(3)]
    norm = math.sqrt(e[0] * e[0] + 2.0 * e[1] * e[1] + 2.0 * e[2] * e[2])
    w0, w1, w2 = (float(np.float32(v / norm)) for v in e)
    return w0, w1, w2


def lag1(taps: Sequence[float]) -> float:
    """rho_1 = 2 w0 w1 + 2 w1 w2: the correlation of the field with its right (or lower) neighbour.  The spatial estimator of ``--sigma auto`` reads
    about (1 - rho_1) G on a stream re-grained at level G: its 2 x 2 statistic has variance 4 G^2 (1 - rho_1)^2."""
    w0, w1, w2 = (float(t) for t in taps)
    return 2.0 * w0 * w1 + 2.0 * w1 * w2


def luma_knots(knots_rgb: Sequence[float], fmt) -> List[float]:
    """The 16 knots in luma code units of ``fmt`` (anything with ``bits``, ``matrix`` and ``range``), as ``sn_yuv_grain`` takes them:
    ``knot * noise.luma_gain(matrix) * noise.code_scale(bits, range)`` in float64, rounded once to float32 -- the standard deviation that i.i.d. noise of
    sigma ``knot`` on 8-bit R'G'B' has in the luma plane."""
    k = check_sigmas(knots_rgb)
    if len(k) != NLF_BANDS:
        raise ValueError(f"a grain curve has {NLF_BANDS} knots, got {len(k)}")
    g = luma_gain(fmt.matrix) * code_scale(fmt.bits, fmt.range)
    return [float(np.float32(v * g)) for v in k]
