"""Blind estimate of the noise level of footage, for the denoise variants of the video restorer (numpy only, no torch).

The histograms are what ``sn_yuv_noise_hist`` (csrc/sn_yuv_stats.hip) writes: per frame, over the luma plane, the counts of
``v = |a - b - c + d|`` of every non-overlapping 2 x 2 block whose four codes lie strictly between the format's black and white codes
(clipped pixels carry less noise than the footage has).  ``v`` is twice the Haar HH coefficient of the block: a smooth image contributes
nothing to it, and white noise of standard deviation s on the codes gives it the variance ``4 s^2 + 1/3`` (the 1/3 is the rounding of four
codes, 4 / 12).  The median of ``|v|`` is robust against the edges and texture that do reach HH:

  med   = the median of v from the cumulative histogram, linear inside the bin (bin 0 covers [0, 0.5), bin k >= 1 [k - 0.5, k + 0.5));
  var   = max((med / 0.6744897501960817)^2 - 1/3, 0);  sigma_Y = sqrt(var) / 2          (luma code units)
  sigma = sigma_Y / (g s),  g = sqrt(Kr^2 + Kg^2 + Kb^2),  s = 219 2^(bits-8) / 255 (limited) or (2^bits - 1) / 255 (full):

the standard deviation of i.i.d. noise on 8-bit R'G'B', which is what the networks were trained with (``noise_map = sigma / 255``).
A window's sigma is the median of its input frames' (as fed: reflected duplicates count), clamped.  Everything here is float64 on exact
integers, so the device's histograms and a host restatement of them give the same floats.

Noise-level function (``noise_model="level"`` of the restorer): real sensor noise is signal dependent, and after the camera's transfer curve the
shadows carry several times the noise of the highlights.  ``sn_yuv_noise_hist_bands`` splits the same statistic into ``NLF_BANDS`` = 16 bands of the
block's brightness (``band = (16 (S - 4 lo)) / (4 (hi - lo))`` for the sum S of the block's four codes; v saturated to ``nlf_bins(bits)`` - 1, the last
bin meaning "at least that").  ``window_curve`` turns a window's summed band histograms into 16 knots, sigma of 8-bit R'G'B' at luma code
``lo + (b + 0.5) (hi - lo) / 16``: the estimate above per band; a band with fewer than ``NLF_MIN_BLOCKS`` blocks or whose median falls in the saturating
bin has none and is filled linearly between the nearest bands that have (constant beyond the outermost; all 0 if none has); then every knot is
clamped.  ``sn_noise_map_level`` evaluates the curve per pixel.  ``parse_curves`` / ``format_curves`` are the file of one curve per window.

A heuristic, checked on synthetic clips only.  It assumes white Gaussian noise: compression makes noise non-white and the estimate then reads
low; pixel-scale texture adds to it in quadrature; at sigma >= 40 the clipping of R'G'B' to [0, 1] makes it read low by construction.

Temporal estimate (``sigma_estimator="temporal"`` / ``"min"`` of the restorer): texture that does not move is the same in the next frame and noise is not.
``sn_yuv_noise_hist_pairs`` counts ``v = |HH(frame p + 1) - HH(frame p)|`` with ``HH = a - b - c + d`` of the same 2 x 2 block in both frames, over the
blocks whose eight codes are unclipped.  Static content cancels exactly; HH rather than the plain frame difference also cancels smooth change (flicker,
fades, exposure drift, motion along gradients).  White noise of standard deviation s gives v the variance ``8 s^2 + 2/3`` (eight rounded codes):

  var = max((med / 0.6744897501960817)^2 - 2/3, 0);  sigma_Y = sqrt(var / 8);  sigma = sigma_Y / (g s)            (``pair_sigma``)

with ``med`` from ``hist_median`` (the same bin geometry).  A pair with no block outside bin 0 is the same frame twice -- the planner's clamped
reflection in clips of one or two frames, duplicated frames in the footage -- and has no estimate: it says nothing about noise.  A window's temporal
sigma is the median over its pairs that have one (a cut inside a window is one outlier pair).  Both estimators can only be pushed UP by picture
content -- texture raises the spatial one, moving fine detail the temporal one -- so the lower of the two is nearer the truth: ``"min"``
(``combine_sigma``), a rule without a threshold.  The curve follows suit band by band (``window_curve_pairs``): the band histograms of the pairs
(``sn_yuv_noise_hist_pairs_bands``) summed over the pairs that are not repeats, estimated per band with the rules above, combined per band with the
spatial knot, then filled and clamped.
Caveats, stated plainly: also a heuristic, checked on synthetic clips only.  Temporally correlated noise reads LOW -- inter-coded footage, where the
encoder predicts the noise, and temporally denoised footage -- and that is the one direction in which ``"min"`` can hurt.  Moving fine texture still
raises both estimates.  A noise-free static clip gives identical frames, every pair is a repeat, and the spatial estimate is what is left.

Motion compensation of the pair (``sigma_motion="blocks"`` of the restorer): a pan moves the texture, and the pair statistic then reads the motion --
the same texture moving 1 px per frame reads 9.0 at an injected 5.  ``sn_yuv_block_motion`` finds, per pair and per ``MOTION_BLOCK`` = 16 x 16 luma
block, the integer translation within +-``MOTION_RANGE`` = 7 samples with the smallest sum of absolute differences, and ``sn_yuv_noise_hist_pairs_mv`` /
``..._bands_mv`` take the next frame's 2 x 2 block where it points.  The vector with the smallest SAD among 225 also fits the noise, and the residual on
the same pixels then reads 10 % low on flat content -- the one direction in which ``"min"`` can hurt.  So the 2 x 2 blocks are split like a checkerboard:
the vector is chosen on the blocks with (i + j) even and the statistic taken only from those with (i + j) odd.  Pixel noise is independent between the
two sets, the choice cannot fit the noise it is measured on, and there is no threshold.  What is left is a small upward bias (a wrong vector on flat
content costs nothing, a wrong one on texture reads as noise) at the price of half the sample count.  ``pair_sigma`` and ``pair_band_sigma`` apply
unchanged: the variance law ``8 s^2 + 2/3`` does not depend on which blocks are counted.  ``motion_summary`` condenses a window's vectors for ``stats``.
Caveats, stated plainly: integer-pel translation per 16 x 16 block within +-7 px; sub-pixel motion, zoom, rotation, occlusion and changing motion blur
still read as noise; matching blocks that touch the black or white code take part in the SAD as they are; temporally correlated noise still reads low,
and now has one more way to do so (a vector that follows the noise pattern); the estimate reads a few per cent HIGH on flat content.  A heuristic,
checked on synthetic clips only.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

MAD_TO_SIGMA = 0.6744897501960817          # the median of |x| for x ~ N(0, 1)
CLAMP = (0.0, 50.0)                        # the range of noise levels upstream evaluates
BT601, BT709 = 0, 1                        # the codes of sn_yuv_fmt.matrix
LIMITED, FULL = 0, 1                       # ... and .range
NLF_BANDS = 16                             # SN_NLF_BANDS: knots of a noise-level function
NLF_MIN_BLOCKS = 1024                      # a band with fewer counted blocks in the window has no estimate of its own


def nbins(bits: int) -> int:
    """Bins per frame of sn_yuv_noise_hist: v = 0 .. 2 (2^bits - 1)."""
    return 2 * ((1 << bits) - 1) + 1


def clip_codes(bits: int, range_: int) -> Tuple[int, int]:
    """(lo, hi) of sn_yuv_noise_hist: the format's black and white luma codes; a block counts iff its four codes lie strictly between."""
    s = 1 << (bits - 8)
    return (0, (1 << bits) - 1) if range_ == FULL else (16 * s, 235 * s)


def luma_gain(matrix: int) -> float:
    """sqrt(Kr^2 + Kg^2 + Kb^2): the standard deviation of Y' for unit i.i.d. noise on R', G', B'."""
    kr, kb = (0.2126, 0.0722) if matrix == BT709 else (0.299, 0.114)
    kg = 1.0 - kr - kb
    return math.sqrt(kr * kr + kg * kg + kb * kb)


def code_scale(bits: int, range_: int) -> float:
    """Luma codes per 8-bit R'G'B' code."""
    return ((1 << bits) - 1) / 255.0 if range_ == FULL else 219.0 * (1 << (bits - 8)) / 255.0


def hist_median(hist) -> Optional[float]:
    """The median of v of one histogram, or None if it is empty."""
    h = np.asarray(hist).reshape(-1).astype(np.int64)
    cum = np.cumsum(h)                                       # exact integers
    n = int(cum[-1]) if len(cum) else 0
    if n == 0:
        return None
    half = n / 2.0
    k = int(np.searchsorted(cum, half, side="left"))         # the first bin whose cumulative count reaches N / 2 (hist[k] > 0 there: half > 0)
    before = int(cum[k - 1]) if k else 0
    left, width = (0.0, 0.5) if k == 0 else (k - 0.5, 1.0)
    return left + width * (half - before) / int(h[k])


def sigma_luma(hist) -> Optional[float]:
    """sigma_Y of one frame in luma code units, or None if no block counted."""
    med = hist_median(hist)
    if med is None:
        return None
    q = med / MAD_TO_SIGMA
    var = q * q - 1.0 / 3.0
    return math.sqrt(var) / 2.0 if var > 0.0 else 0.0


def frame_sigma(hist, bits: int, matrix: int, range_: int) -> Optional[float]:
    """One histogram -> the sigma of i.i.d. noise on 8-bit R'G'B' that explains it, or None if no block counted."""
    s = sigma_luma(hist)
    return None if s is None else s / (luma_gain(matrix) * code_scale(bits, range_))


def check_clamp(clamp: Sequence[float]) -> Tuple[float, float]:
    lo, hi = (float(c) for c in clamp)
    if not (0.0 <= lo <= hi):                                # refuses NaN as well
        raise ValueError(f"sigma_clamp must be (lo, hi) with 0 <= lo <= hi, got {tuple(clamp)!r}")
    return lo, hi


def window_sigma(frame_sigmas: Iterable[Optional[float]], clamp: Sequence[float] = CLAMP) -> float:
    """The median of the frames' sigmas (frames without an estimate left out; 0 if none has one), clamped."""
    lo, hi = check_clamp(clamp)
    return min(max(frames_median(frame_sigmas), lo), hi)


# ---- the temporal estimate: frame pairs ---------------------------------------------------------------------------------------------------
ESTIMATORS = ("spatial", "temporal", "min")


def pair_bins(bits: int) -> int:
    """Bins per pair of sn_yuv_noise_hist_pairs: v = 0 .. 4 (2^bits - 1)."""
    return 4 * ((1 << bits) - 1) + 1


def pair_is_repeat(hist) -> bool:
    """No block outside bin 0 (an empty histogram included): the same frame twice as far as the statistic can tell, or nothing counted."""
    h = np.asarray(hist)
    return not bool(h.reshape(-1, h.shape[-1])[:, 1:].any())


def pair_sigma_luma(hist) -> Optional[float]:
    """sigma_Y of one pair histogram in luma code units (no repeat rule here), or None if no block counted."""
    med = hist_median(hist)
    if med is None:
        return None
    q = med / MAD_TO_SIGMA
    var = q * q - 2.0 / 3.0
    return math.sqrt(var / 8.0) if var > 0.0 else 0.0


def pair_sigma(hist, bits: int, matrix: int, range_: int) -> Optional[float]:
    """One pair histogram -> the sigma of i.i.d. noise on 8-bit R'G'B' that explains it, or None: no block counted, or none fell outside bin 0."""
    if pair_is_repeat(hist):
        return None
    return pair_sigma_luma(hist) / (luma_gain(matrix) * code_scale(bits, range_))


def window_sigma_temporal(pair_sigmas: Iterable[Optional[float]]) -> Optional[float]:
    """The median over the pairs that have an estimate, or None if none has."""
    v = [s for s in pair_sigmas if s is not None]
    return float(np.median(np.asarray(v, np.float64))) if v else None


# ---- motion compensation of the pair --------------------------------------------------------------------------------------------------
MOTION_BLOCK = 16                          # luma samples per side of a vector block: 8 x 8 of the 2 x 2 blocks
MOTION_RANGE = 7                           # |dy|, |dx| <= 7: 225 candidates


def motion_grid(h: int, w: int) -> Tuple[int, int]:
    """(nby, nbx) of sn_yuv_block_motion for an h x w picture: the vector blocks that hold at least one whole 2 x 2 block; (0, 0) if there is none."""
    per = MOTION_BLOCK // 2
    hb, wb = int(h) // 2, int(w) // 2
    return ((hb + per - 1) // per, (wb + per - 1) // per) if hb > 0 and wb > 0 else (0, 0)


def motion_summary(mv) -> List[Tuple[float, float, float]]:
    """int8 [P, nby, nbx, 2] vectors (dy, dx) of a window's pairs -> per pair (the share of blocks with a nonzero vector, the median dy, the median dx);
    (0.0, 0.0, 0.0) for a pair without blocks."""
    v = np.asarray(mv)
    assert v.ndim == 4 and v.shape[3] == 2, v.shape
    out = []
    for p in v.reshape(v.shape[0], -1, 2).astype(np.int64):
        if len(p) == 0:
            out.append((0.0, 0.0, 0.0))
        else:
            out.append((float(np.count_nonzero(p.any(axis=1))) / len(p), float(np.median(p[:, 0])), float(np.median(p[:, 1]))))
    return out


def frames_median(frame_sigmas: Iterable[Optional[float]]) -> float:
    """The spatial estimate of a window before the clamp: the median of the frames' sigmas (frames without one left out; 0 if none has one)."""
    v = [s for s in frame_sigmas if s is not None]
    return float(np.median(np.asarray(v, np.float64))) if v else 0.0


def check_estimator(estimator) -> str:
    if not (isinstance(estimator, str) and estimator in ESTIMATORS):
        raise ValueError(f"sigma_estimator must be one of {', '.join(repr(e) for e in ESTIMATORS)}, got {estimator!r}")
    return estimator


def _combine(spatial: Optional[float], temporal: Optional[float], estimator: str) -> Optional[float]:
    """The rule, on estimates that may be missing: "spatial" -> the spatial one; "temporal" -> the temporal one, the spatial one where there is none;
    "min" -> the lower of the two, the one that exists where one is missing."""
    check_estimator(estimator)
    if estimator == "spatial" or temporal is None:
        return spatial
    if estimator == "temporal" or spatial is None:
        return temporal
    return min(spatial, temporal)


def combine_sigma(spatial: float, temporal: Optional[float], estimator: str = "spatial", clamp: Sequence[float] = CLAMP) -> float:
    """A window's sigma from its spatial estimate (``frames_median``, unclamped) and its temporal one (``window_sigma_temporal``, None: none):
    "spatial" -> the spatial one; "temporal" -> the temporal one, or the spatial one where it is None; "min" -> the lower of the two, or the spatial
    one where the temporal is None.  The clamp is applied last, once."""
    lo, hi = check_clamp(clamp)
    return min(max(float(_combine(float(spatial), temporal, estimator)), lo), hi)


def check_sigmas(sigmas: Iterable[float]) -> List[float]:
    """A per-window list: finite numbers >= 0."""
    out: List[float] = []
    for s in sigmas:
        if isinstance(s, (bool, str)) or not math.isfinite(float(s)) or float(s) < 0.0:
            raise ValueError(f"a sigma must be a finite number >= 0, got {s!r}")
        out.append(float(s))
    return out


def parse_sigmas(text: str) -> List[float]:
    """One sigma per line, one per window in order; '#' starts a comment, blank lines are skipped.  Anything else raises ValueError naming
    the line."""
    out: List[float] = []
    for no, line in enumerate(text.splitlines(), 1):
        word = line.split("#", 1)[0].strip()
        if not word:
            continue
        try:
            try:
                val = float(word)
            except ValueError:
                raise ValueError("not a number") from None
            out += check_sigmas([val])
        except ValueError as e:
            raise ValueError(f"line {no}: {line.strip()!r}: {e}") from None
    return out


def format_sigmas(sigmas: Iterable[float], how: str = "") -> str:
    """The text ``parse_sigmas`` reads back to the same floats (repr round-trips float64)."""
    sigmas = [float(s) for s in sigmas]
    head = f"# noise level per window (sigma of 8-bit R'G'B' codes), in the order the windows are restored; {len(sigmas)} window{'' if len(sigmas) == 1 else 's'}"
    return head + (f"; {how}" if how else "") + "\n" + "".join(f"{s!r}\n" for s in sigmas)


# ---- the noise-level function: sigma against the luma code ---------------------------------------------------------------------------------
def nlf_bins(bits: int) -> int:
    """NBV: bins per band of sn_yuv_noise_hist_bands; the last one means "at least NBV - 1"."""
    return 128 << (bits - 8)


def knot_codes(lo: int, hi: int) -> List[float]:
    """The luma codes the 16 knots sit at."""
    return [lo + (b + 0.5) * (hi - lo) / NLF_BANDS for b in range(NLF_BANDS)]


def band_sigma(hist, bits: int, matrix: int, range_: int, min_blocks: int = NLF_MIN_BLOCKS) -> Optional[float]:
    """One band's histogram (the window's sum) -> ``frame_sigma`` of it, or None: fewer than ``min_blocks`` blocks, or the median in the last bin."""
    h = np.asarray(hist).reshape(-1).astype(np.int64)
    cum = np.cumsum(h)
    n = int(cum[-1])
    if n < max(min_blocks, 1):
        return None
    if int(np.searchsorted(cum, n / 2.0, side="left")) == len(h) - 1:        # hist_median's bin: "at least NBV - 1" has no width to interpolate in
        return None
    return frame_sigma(h, bits, matrix, range_)


def fill_curve(knots: Sequence[Optional[float]]) -> List[float]:
    """None entries filled: linear in the band index between the nearest entries that have a value, a + (c - a) (b - i) / (j - i) for i < b < j;
    constant beyond the outermost; all 0.0 if there is none."""
    have = [b for b, k in enumerate(knots) if k is not None]
    if not have:
        return [0.0] * len(knots)
    out: List[float] = []
    for b, k in enumerate(knots):
        if k is not None:
            out.append(float(k))
        elif b < have[0]:
            out.append(float(knots[have[0]]))
        elif b > have[-1]:
            out.append(float(knots[have[-1]]))
        else:
            i = max(x for x in have if x < b)
            j = min(x for x in have if x > b)
            out.append(float(knots[i]) + (float(knots[j]) - float(knots[i])) * (b - i) / (j - i))
    return out


def window_curve(band_hists, bits: int, matrix: int, range_: int, clamp: Sequence[float] = CLAMP, min_blocks: int = NLF_MIN_BLOCKS) -> List[float]:
    """band_hists: [T, 16, NBV] (or [16, NBV]) counts of a window's input frames as fed -> its 16 knots: summed over the frames, estimated per band,
    holes filled, clamped."""
    lo, hi = check_clamp(clamp)
    h = np.asarray(band_hists).astype(np.int64)
    h = h.reshape(-1, NLF_BANDS, h.shape[-1]).sum(axis=0)
    knots = fill_curve([band_sigma(h[b], bits, matrix, range_, min_blocks) for b in range(NLF_BANDS)])
    return [min(max(k, lo), hi) for k in knots]


def pair_band_sigma(hist, bits: int, matrix: int, range_: int, min_blocks: int = NLF_MIN_BLOCKS) -> Optional[float]:
    """One band's pair histogram (the window's sum over its pairs) -> ``pair_sigma``'s arithmetic on it, with ``band_sigma``'s rules: None for fewer than
    ``min_blocks`` blocks or the median in the last bin."""
    h = np.asarray(hist).reshape(-1).astype(np.int64)
    cum = np.cumsum(h)
    n = int(cum[-1])
    if n < max(min_blocks, 1):
        return None
    if int(np.searchsorted(cum, n / 2.0, side="left")) == len(h) - 1:
        return None
    return pair_sigma_luma(h) / (luma_gain(matrix) * code_scale(bits, range_))


def sum_pair_bands(pair_band_hists) -> np.ndarray:
    """[P, 16, NBV] (or [16, NBV]) band histograms of a window's pairs -> their int64 sum [16, NBV] over the pairs that are not repeats
    (``pair_is_repeat``: nothing outside bin 0 in any band); the bin-0 mass of a repeat would drag every band down."""
    h = np.asarray(pair_band_hists).astype(np.int64)
    h = h.reshape(-1, NLF_BANDS, h.shape[-1])
    keep = [p for p in range(len(h)) if not pair_is_repeat(h[p])]
    return h[keep].sum(axis=0) if keep else np.zeros(h.shape[1:], np.int64)


def window_curve_pairs(band_hists, pair_band_hists, bits: int, matrix: int, range_: int, estimator: str = "min", clamp: Sequence[float] = CLAMP,
                       min_blocks: int = NLF_MIN_BLOCKS) -> List[float]:
    """``window_curve`` with the temporal estimate: band_hists [T, 16, NBV] of the window's frames and pair_band_hists [T - 1, 16, NBV] of its pairs ->
    16 knots.  Per band the spatial estimate (``band_sigma`` of the frames' sum) and the temporal one (``pair_band_sigma`` of ``sum_pair_bands``) are
    combined as ``combine_sigma`` combines (None where neither exists); then the holes are filled, then every knot is clamped."""
    lo, hi = check_clamp(clamp)
    check_estimator(estimator)
    h = np.asarray(band_hists).astype(np.int64)
    h = h.reshape(-1, NLF_BANDS, h.shape[-1]).sum(axis=0)
    ph = sum_pair_bands(pair_band_hists)
    knots = []
    for b in range(NLF_BANDS):
        spatial = band_sigma(h[b], bits, matrix, range_, min_blocks)
        temporal = pair_band_sigma(ph[b], bits, matrix, range_, min_blocks) if estimator != "spatial" else None
        knots.append(_combine(spatial, temporal, estimator))
    return [min(max(k, lo), hi) for k in fill_curve(knots)]


def check_curves(curves: Iterable[Sequence[float]]) -> List[List[float]]:
    """A per-window list of curves: each 16 finite numbers >= 0."""
    out: List[List[float]] = []
    for c in curves:
        if isinstance(c, (str, bytes)) or not hasattr(c, "__iter__"):
            raise ValueError(f"a noise curve must be a sequence of {NLF_BANDS} numbers, got {c!r}")
        c = list(c)
        if len(c) != NLF_BANDS:
            raise ValueError(f"a noise curve has {NLF_BANDS} knots, got {len(c)}")
        try:
            out.append(check_sigmas(c))
        except ValueError as e:
            raise ValueError(f"a knot of a noise curve: {e}") from None
    return out


def parse_curves(text: str) -> List[List[float]]:
    """One curve per line, 16 numbers separated by blanks, one line per window in order; '#' starts a comment, blank lines are skipped.  Anything
    else raises ValueError naming the line."""
    out: List[List[float]] = []
    for no, line in enumerate(text.splitlines(), 1):
        words = line.split("#", 1)[0].split()
        if not words:
            continue
        try:
            try:
                vals = [float(w) for w in words]
            except ValueError:
                raise ValueError("not a number") from None
            out += check_curves([vals])
        except ValueError as e:
            raise ValueError(f"line {no}: {line.strip()!r}: {e}") from None
    return out


def format_curves(curves: Iterable[Sequence[float]], how: str = "") -> str:
    """The text ``parse_curves`` reads back to the same floats (repr round-trips float64)."""
    curves = [[float(k) for k in c] for c in curves]
    head = (f"# noise-level function per window: sigma of 8-bit R'G'B' codes at {NLF_BANDS} luma levels from black to white, in the order the windows are "
            f"restored; {len(curves)} window{'' if len(curves) == 1 else 's'}")
    return head + (f"; {how}" if how else "") + "\n" + "".join(" ".join(repr(k) for k in c) + "\n" for c in curves)
