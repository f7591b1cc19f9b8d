"""Brightness flicker taken out (``--deflicker R``): the option's grammar and the rule that turns the luma histograms of a clip into one tone curve
per frame.  numpy only; the histograms come from ``sn_yuv_code_hist`` and the tables go to ``sn_yuv_apply_lut`` (csrc/sn_deflicker.hip).

Old film transfers, timelapses, material shot under mains lighting and cameras whose auto-exposure hunts flicker: the brightness of whole frames steps
about from one to the next.  The rule matches every frame's histogram to the MEDIAN of its neighbours' -- exact integer and rational arithmetic, no
threshold:

    L = 2^bits; h_t[c] the luma histogram of frame t over all N samples, C_t[c] its running sum, C_t[-1] = 0.  Frame t lies in the clip [lo, hi).
    Window: r = min(R, t - lo, hi - 1 - t); the neighbours are s = t - r .. t + r.  Always symmetric, so a linear fade passes unchanged; a clip's
    first and last frame leave as they came.
    For every code c with h_t[c] > 0: a = C_t[c - 1] + C_t[c], twice the mid-rank of c.  For a neighbour s, k is the smallest code with
    2 C_s[k] >= a, and Q_s = ((2k - 1) h_s[k] + a - 2 C_s[k - 1]) / (2 h_s[k]): ONE float64 division of two exact integers, the quantile of frame s
    at that rank with code k spread uniformly over [k - 1/2, k + 1/2].  For s = t it is exactly c.
    lutY_t[c] = clamp(floor(median_s Q_s + 0.5), 0, L - 1), the median the middle of the sorted 2r + 1 values.  A code absent from frame t takes the
    value of the nearest present code below it, or of the first present code if there is none.  Non-decreasing by construction.
    Chroma ("gain"): yo the luma black code (16 * 2^(bits - 8) limited, 0 full), m and m' the frame's mean luma code before and after the table, each
    ONE float64 division of the exact sum of code * count by N; k = (m' - yo) / (m - yo) clamped to [0.5, 2], and k = 1 when m - yo < 1 or when
    lutY is the identity on every present code; lutC_t[c] = clamp(floor(co + k * (c - co) + 0.5), 0, L - 1), co = 128 * 2^(bits - 8).  "off": the
    identity.

The median, not the mean, makes the rule safe at a cut nobody listed: within R frames of a cut a frame's own side still holds r + 1 of the 2r + 1 votes.
Identical histograms in the window give identity tables: a static clip leaves byte for byte.  tests/deflicker_ref.py restates the rule with plain
loops and Python integers, and ``tables`` equals it bit for bit.

**The limits.**  One tone curve per frame: local flicker (one side of the picture, a lamp in shot) stays.  A real flash or lightning frame is pulled
towards its neighbours.  A frame within R of a cut is judged by fewer frames of its own side.  Luma decides alone; chroma gets one factor per frame,
or nothing.  The curve is computed on codes, not in linear light.  Bars are in the histogram.  Moving content that changes the histogram -- a bright
object entering the picture -- reads as flicker and is partly undone.  Nobody has judged it on real footage."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

DEFLICKER_MAX_R = 15
CHROMA_MODES = ("gain", "off")


def parse_deflicker(text: str) -> int:
    """--deflicker: R, the frames looked at on either side: an integer 1 .. 15; anything else is a ValueError."""
    try:
        r = int(str(text).strip())
    except ValueError:
        r = 0
    if not (1 <= r <= DEFLICKER_MAX_R):
        raise ValueError(f"a number of frames on either side, 1 .. {DEFLICKER_MAX_R}, got {text!r}")
    return r


def deflicker_form(deflicker, deflicker_chroma="gain", add_noise=None, add_blur=None) -> Tuple[Optional[int], str]:
    """The restorer's ``deflicker`` / ``deflicker_chroma`` -> (None, chroma) or (R, chroma).  ValueError for anything else, for a chroma word other
    than the default without ``deflicker``, and for ``deflicker`` together with ``add_noise`` or ``add_blur`` (whatever is not None)."""
    if not isinstance(deflicker_chroma, str) or deflicker_chroma not in CHROMA_MODES:
        raise ValueError(f"deflicker_chroma must be one of {', '.join(CHROMA_MODES)}, got {deflicker_chroma!r}")
    if deflicker is None:
        if deflicker_chroma != "gain":
            raise ValueError("deflicker_chroma says what deflicker does to the chroma planes: it needs deflicker")
        return None, deflicker_chroma
    ok = not isinstance(deflicker, (bool, str, bytes, float)) and hasattr(deflicker, "__index__")
    r = int(deflicker) if ok else 0
    if not (1 <= r <= DEFLICKER_MAX_R):
        raise ValueError(f"deflicker must be an integer 1 .. {DEFLICKER_MAX_R} (frames on either side), got {deflicker!r}")
    for name, other in (("add_noise", add_noise), ("add_blur", add_blur)):
        if other is not None:
            raise ValueError(f"deflicker together with {name}: {name} makes a degraded copy of a clean stream for an experiment, deflicker repairs a "
                             "stream that flickers; pick one")
    return r, deflicker_chroma


def black_code(bits: int, range_: int) -> int:
    """yo: the luma black code of a format (range_: lib.SN_YUV_LIMITED = 0, lib.SN_YUV_FULL = 1)."""
    return 0 if range_ == 1 else 16 << (bits - 8)


def _luma_table(H: np.ndarray, C: np.ndarray, t: int, r: int) -> np.ndarray:
    """lutY of frame t from the histograms H and running sums C (int64 [S][L]) of its clip, neighbours t - r .. t + r: int64 [L]."""
    L = H.shape[1]
    h = H[t]
    present = h > 0
    codes = np.nonzero(present)[0]
    a = 2 * C[t, codes] - h[codes]                                # C[c - 1] + C[c]
    Q = np.empty((2 * r + 1, codes.size), dtype=np.float64)
    for j, s in enumerate(range(t - r, t + r + 1)):
        k = np.searchsorted(2 * C[s], a, side="left")              # the smallest code with 2 C_s[k] >= a; a <= 2 N = 2 C_s[L - 1]
        hk = H[s, k]
        below = C[s, k] - hk                                      # C_s[k - 1]
        num = (2 * k - 1) * hk + a - 2 * below
        Q[j] = num.astype(np.float64) / (2 * hk).astype(np.float64)      # exact integers below 2^53: one rounding
    med = np.sort(Q, axis=0)[r]
    val = np.clip(np.floor(med + 0.5), 0, L - 1).astype(np.int64)
    at = np.maximum.accumulate(np.where(present, np.arange(L), -1))      # the nearest present code at or below
    at = np.where(at < 0, codes[0], at)
    full = np.zeros(L, dtype=np.int64)
    full[codes] = val
    return full[at]


def tables(hists, lo: int, hi: int, R: int, fmt, chroma: str = "gain", first: Optional[int] = None, count: Optional[int] = None):
    """hists: [S][2^bits] counts, the luma histograms of S consecutive frames, every one of the same total N >= 1; frames lo .. hi - 1 of them are
    the clip.  -> (uint16 [T][2][2^bits], [(r, mean_in, mean_out, chroma_gain)] * T): the tables (Y; Cb and Cr) of frames first .. first + T - 1 of
    the list (default: the whole clip, first = lo, T = hi - lo) and their four numbers, by the rule above.  fmt: anything with ``bits`` and ``range``.
    chroma: "gain" or "off"."""
    H = np.ascontiguousarray(np.asarray(hists, dtype=np.int64))
    bits = int(fmt.bits)
    L = 1 << bits
    if H.ndim != 2 or H.shape[1] != L or not (0 <= lo < hi <= H.shape[0]):
        raise ValueError(f"need [S][{L}] histograms and a clip 0 <= lo < hi <= S, got shape {H.shape}, lo {lo}, hi {hi}")
    if not (1 <= R <= DEFLICKER_MAX_R) or chroma not in CHROMA_MODES:
        raise ValueError(f"need R in 1 .. {DEFLICKER_MAX_R} and chroma one of {CHROMA_MODES}, got {R!r}, {chroma!r}")
    first = lo if first is None else int(first)
    count = hi - first if count is None else int(count)
    if not (lo <= first and count >= 1 and first + count <= hi):
        raise ValueError(f"frames {first} .. {first + count - 1} do not lie in the clip [{lo}, {hi})")
    need = slice(max(lo, first - R), min(hi, first + count + R))
    N = int(H[need.start].sum())
    if N < 1 or H[need].min() < 0 or np.any(H[need].sum(axis=1) != N):
        raise ValueError("the histograms of a clip count the same number of samples, at least one, and no bin is negative")
    C = np.cumsum(H, axis=1)
    yo, co = float(black_code(bits, int(fmt.range))), float(128 << (bits - 8))
    codes = np.arange(L, dtype=np.int64)
    ident = codes.astype(np.uint16)
    lut = np.empty((count, 2, L), dtype=np.uint16)
    info: List[Tuple[int, float, float, float]] = []
    for i, t in enumerate(range(first, first + count)):
        r = min(R, t - lo, hi - 1 - t)
        ly = _luma_table(H, C, t, r)
        h = H[t]
        m_in, m_out = int((codes * h).sum()) / N, int((ly * h).sum()) / N
        k = 1.0
        if chroma == "gain" and m_in - yo >= 1.0 and np.any(ly[h > 0] != codes[h > 0]):
            k = min(max((m_out - yo) / (m_in - yo), 0.5), 2.0)
        lut[i, 0] = ly
        lut[i, 1] = ident if k == 1.0 else np.clip(np.floor(co + k * (codes.astype(np.float64) - co) + 0.5), 0, L - 1).astype(np.uint16)
        info.append((r, m_in, m_out, k))
    return lut, info


def mean_roughness(means: Sequence[float]) -> float:
    """The rms second difference of a sequence of frame means, m[t - 1] - 2 m[t] + m[t + 1]: what flicker raises and a fade does not.  0 for fewer
    than three frames."""
    m = np.asarray(means, dtype=np.float64)
    if m.size < 3:
        return 0.0
    d = m[:-2] - 2.0 * m[1:-1] + m[2:]
    return float(np.sqrt(np.mean(d * d)))


def format_deflicker(frames: Sequence[Tuple[int, float, float, float]]) -> str:
    """--deflicker_out: one line per frame, ``r mean_in mean_out chroma_gain``, then a last line with the rms second difference of the frame means
    before and after."""
    lines = ["%d %.4f %.4f %.6f" % tuple(f) for f in frames]
    lines.append("# rms second difference of the frame means: %.4f before, %.4f after" % (mean_roughness([f[1] for f in frames]),
                                                                                         mean_roughness([f[2] for f in frames])))
    return "\n".join(lines) + "\n"
