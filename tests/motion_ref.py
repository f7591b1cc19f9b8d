"""Host references of the motion-compensated temporal noise estimate, numpy only: the vectors and SADs that ``sn_yuv_block_motion``
must equal exactly, by a plain loop over the 225 candidates in the tie order; the two histograms along the vectors that
``sn_yuv_noise_hist_pairs_mv`` and ``sn_yuv_noise_hist_pairs_bands_mv`` must equal exactly, for any int8 vectors; a window's estimates as the
restorer must report them with ``sigma_motion="blocks"``; and the synthetic clips with INJECTED noise the scheme is judged against.  Nothing of the
product is shared beyond the histogram -> sigma functions of ``shiftnet_amd/noise.py`` that existed before the option.  ``split=False`` matches and
measures on every 2 x 2 block: it exists only to document the bias that the checkerboard split removes."""
from __future__ import annotations

import numpy as np

import nlf_ref as F
import noise_pairs_ref as NP
import noise_ref as N
import yuv_ref as R

RANGE = 7                                                          # |dy|, |dx| <= 7
BLOCK = 8                                                          # 2 x 2 blocks per side of a vector block: 16 x 16 samples
# the candidates in the tie order: the smallest (|dy| + |dx|, dy, dx) wins among equal SADs
CANDIDATES = sorted(((dy, dx) for dy in range(-RANGE, RANGE + 1) for dx in range(-RANGE, RANGE + 1)), key=lambda v: (abs(v[0]) + abs(v[1]), v[0], v[1]))


def grid(h: int, w: int):
    """(nby, nbx): the vector blocks that hold a whole 2 x 2 block; (0, 0) without one."""
    hb, wb = h // 2, w // 2
    return (-(-hb // BLOCK), -(-wb // BLOCK)) if hb > 0 and wb > 0 else (0, 0)


def _parity(hb: int, wb: int) -> np.ndarray:
    """(i + j) & 1 of every 2 x 2 block: 0 matches, 1 measures."""
    i, j = np.mgrid[0:hb, 0:wb]
    return (i + j) & 1


def motion_pair(Y0: np.ndarray, Y1: np.ndarray, split: bool = True):
    """Two luma planes [h, w] (int64) -> (int8 [nby, nbx, 2], uint32 [nby, nbx]): the vector and its SAD of every vector block."""
    h, w = Y0.shape
    hb, wb = h // 2, w // 2
    nby, nbx = grid(h, w)
    mv, best = np.zeros((nby, nbx, 2), np.int8), np.full((nby, nbx), -1, np.int64)
    if nby == 0:
        return mv, best.astype(np.uint32)
    take = np.repeat(np.repeat(_parity(hb, wb) == 0, 2, axis=0), 2, axis=1) if split else np.ones((2 * hb, 2 * wb), bool)      # per sample
    I, J = np.mgrid[0:nby, 0:nbx]
    ys, ye = 16 * I, 2 * np.minimum(BLOCK * I + BLOCK, hb)          # the sample extent of every vector block, clipped to the whole 2 x 2 blocks
    xs, xe = 16 * J, 2 * np.minimum(BLOCK * J + BLOCK, wb)
    for dy, dx in CANDIDATES:
        ok = (ys + dy >= 0) & (ye + dy <= h) & (xs + dx >= 0) & (xe + dx <= w)      # admissible: the displaced extent lies inside the picture
        if not ok.any():
            continue
        D = np.zeros((16 * nby, 16 * nbx), np.int64)                # |Y_p(y, x) - Y_{p+1}(y + dy, x + dx)| where both exist, on the matching samples
        y0, y1, x0, x1 = max(0, -dy), min(2 * hb, h - dy), max(0, -dx), min(2 * wb, w - dx)
        D[y0:y1, x0:x1] = np.abs(Y0[y0:y1, x0:x1] - Y1[y0 + dy:y1 + dy, x0 + dx:x1 + dx]) * take[y0:y1, x0:x1]
        sad = D.reshape(nby, 16, nbx, 16).sum(axis=(1, 3))
        better = ok & ((best < 0) | (sad < best))                   # strictly smaller: an earlier candidate in the tie order keeps a tie
        best[better] = sad[better]
        mv[better] = (dy, dx)
    assert (best >= 0).all()                                        # (0, 0) is always admissible
    return mv, best.astype(np.uint32)


def block_motion_ref(payloads: np.ndarray, fmt: R.Fmt, H: int, W: int, rect=None, split: bool = True):
    """uint8 [T, frame_bytes] -> (int8 [T - 1, nby, nbx, 2], uint32 [T - 1, nby, nbx])."""
    Y = [F.luma_of(p, fmt, H, W, rect) for p in payloads]
    out = [motion_pair(Y[p], Y[p + 1], split) for p in range(len(Y) - 1)]
    return np.stack([m for m, _ in out]), np.stack([s for _, s in out])


def _pair_mv(p0, p1, mv, fmt: R.Fmt, H: int, W: int, lo: int, hi: int, rect, split: bool = True):
    """(v, S) of the measuring blocks of one pair that count: the second payload's block taken at (2 i + dy, 2 j + dx) with (dy, dx) the vector of block
    (i / 8, j / 8), wholly inside the picture, all eight codes strictly between lo and hi.  ``mv`` may hold any int8."""
    Y0, Y1 = F.luma_of(p0, fmt, H, W, rect), F.luma_of(p1, fmt, H, W, rect)
    h, w = Y0.shape
    hb, wb = h // 2, w // 2
    if hb == 0 or wb == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    i, j = np.mgrid[0:hb, 0:wb]
    vec = np.asarray(mv).astype(np.int64)[i // BLOCK, j // BLOCK]
    y, x = 2 * i + vec[..., 0], 2 * j + vec[..., 1]
    ok = (y >= 0) & (y + 2 <= h) & (x >= 0) & (x + 2 <= w)
    if split:
        ok &= _parity(hb, wb) == 1
    i, j, y, x = i[ok], j[ok], y[ok], x[ok]
    q0 = (Y0[2 * i, 2 * j], Y0[2 * i, 2 * j + 1], Y0[2 * i + 1, 2 * j], Y0[2 * i + 1, 2 * j + 1])
    q1 = (Y1[y, x], Y1[y, x + 1], Y1[y + 1, x], Y1[y + 1, x + 1])
    keep = np.ones(i.shape, bool)
    for q in q0 + q1:
        keep &= (q > lo) & (q < hi)
    v = np.abs((q1[0] - q1[1] - q1[2] + q1[3]) - (q0[0] - q0[1] - q0[2] + q0[3]))
    return v[keep], (sum(q0) + sum(q1))[keep]


def hist_pairs_mv_ref(payloads: np.ndarray, mv: np.ndarray, fmt: R.Fmt, H: int, W: int, lo: int, hi: int, rect=None, split: bool = True) -> np.ndarray:
    """uint8 [T, frame_bytes] and int8 [T - 1, nby, nbx, 2] -> uint32 [T - 1, NBP]."""
    nb = NP.nbp(fmt.bits)
    out = np.zeros((len(payloads) - 1, nb), np.uint32)
    for p in range(len(payloads) - 1):
        v, _ = _pair_mv(payloads[p], payloads[p + 1], mv[p], fmt, H, W, lo, hi, rect, split)
        out[p] = np.bincount(np.minimum(v, nb - 1), minlength=nb)    # v <= NBP - 1 unless hi admits stored words above 2^bits - 1: saturated then
    return out


def hist_pairs_bands_mv_ref(payloads: np.ndarray, mv: np.ndarray, fmt: R.Fmt, H: int, W: int, lo: int, hi: int, rect=None, split: bool = True) -> np.ndarray:
    """uint8 [T, frame_bytes] and int8 [T - 1, nby, nbx, 2] -> uint32 [T - 1, 16, NBV]."""
    nb = F.nbv(fmt.bits)
    out = np.zeros((len(payloads) - 1, NP.BANDS, nb), np.uint32)
    for p in range(len(payloads) - 1):
        v, S = _pair_mv(payloads[p], payloads[p + 1], mv[p], fmt, H, W, lo, hi, rect, split)
        band = NP.band_of(S, lo, hi)
        assert band.size == 0 or (0 <= band.min() and band.max() <= NP.BANDS - 1)
        out[p] = np.bincount(band * nb + np.minimum(v, nb - 1), minlength=NP.BANDS * nb).reshape(NP.BANDS, nb)
    return out


def _median(values) -> float:
    s = sorted(values)
    n = len(s)
    return float(s[n // 2]) if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0


def summary_ref(mv: np.ndarray):
    """Per pair (the share of blocks with a nonzero vector, the median dy, the median dx), with plain loops; zeros for a pair without blocks."""
    out = []
    for pair in np.asarray(mv):
        vs = [(int(v[0]), int(v[1])) for row in pair for v in row]
        if not vs:
            out.append((0.0, 0.0, 0.0))
            continue
        out.append((sum(1 for v in vs if v != (0, 0)) / len(vs), _median([v[0] for v in vs]), _median([v[1] for v in vs])))
    return out


# ---- what the restorer must report for a stream with sigma_motion="blocks" ------------------------------------------------------------------------
def window_estimates(pay, fmt: R.Fmt, h: int, w: int, one_len: int, estimator: str, cuts=(), clamp=(0.0, 50.0), rect=None, level: bool = False):
    """noise_pairs_ref.window_estimates with the pairs compensated, plus ``pair_motion``: per window, per pair, the summary of the vectors."""
    from shiftnet_amd import noise
    lo, hi = N.clip_codes(fmt)
    out = dict(frame_sigma=[], pair_sigma=[], spatial=[], temporal=[], sigma=[], nlf=[], pair_motion=[])
    for idx in N.window_inputs(len(pay), one_len, cuts):
        stack = np.stack([pay[i] for i in idx])
        per = [noise.frame_sigma(x, fmt.bits, fmt.matrix, fmt.range) for x in NP.hist_rect_ref(stack, fmt, h, w, lo, hi, rect)]
        mv, _ = block_motion_ref(stack, fmt, h, w, rect)
        ps = [noise.pair_sigma(x, fmt.bits, fmt.matrix, fmt.range) for x in hist_pairs_mv_ref(stack, mv, fmt, h, w, lo, hi, rect)]
        spatial, temporal = noise.frames_median(per), noise.window_sigma_temporal(ps)
        out["frame_sigma"].append(per)
        out["pair_sigma"].append(ps)
        out["spatial"].append(spatial)
        out["temporal"].append(temporal)
        out["sigma"].append(noise.combine_sigma(spatial, temporal, estimator, clamp))
        out["pair_motion"].append(summary_ref(mv))
        if level:
            out["nlf"].append(noise.window_curve_pairs(F.hist_bands_ref(stack, fmt, h, w, lo, hi, rect),
                                                       hist_pairs_bands_mv_ref(stack, mv, fmt, h, w, lo, hi, rect), fmt.bits, fmt.matrix, fmt.range,
                                                       estimator, clamp))
    return out


# ---- the clips of the accuracy table: those of noise_pairs_ref, 180 x 320, five frames, BT.709 limited 8 bit ------------------------
def moving_clip(t: int, h: int, w: int, vy: float, vx: float) -> np.ndarray:
    """noise_pairs_ref.texture_clip moving (vy, vx) pixels per frame, down and to the right."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([np.repeat((0.5 + 0.15 * np.sin(0.9 * (x - vx * k)) * np.sin(1.1 * (y - vy * k)))[None], 3, axis=0) for k in range(t)])


# integer-pel motion inside the search range: what the matcher is built for, and what the accuracy bound is asserted on
WHOLE = {"flat 0.5": NP.flat_clip, "static texture": lambda t, h, w: NP.texture_clip(t, h, w, 0),
         "texture, 1 px per frame": lambda t, h, w: NP.texture_clip(t, h, w, 1), "texture, 3 px per frame": lambda t, h, w: NP.texture_clip(t, h, w, 3),
         "texture, 2 px per frame down": lambda t, h, w: moving_clip(t, h, w, 2, 0),
         "texture, 1 px down and 2 px right per frame": lambda t, h, w: moving_clip(t, h, w, 1, 2)}
# sub-pixel motion: a stated limit, measured and reported, not bounded
FRACTIONAL = {"texture, 1.5 px per frame": lambda t, h, w: NP.texture_clip(t, h, w, 1.5), "texture, 0.5 px per frame": lambda t, h, w: NP.texture_clip(t, h, w, 0.5)}
CLIPS = {**WHOLE, **FRACTIONAL}
SIGMAS = (2, 5, 10, 20, 30)
SEEDS = (0, 1, 2)


def clip_estimates(clip: str, s: float, seed: int = 0, split: bool = True):
    """(plain temporal, compensated temporal) of the clip with sigma s injected as noise_ref.noisy_payloads injects it: the five frames are one window's
    input, the estimates are the unclamped medians over the four pairs."""
    from shiftnet_amd import noise
    c, fmt = NP.ACC, NP.ACC_FMT
    pay = N.noisy_payloads(CLIPS[clip](c["t"], c["h"], c["w"]), float(s), fmt, seed=seed)
    lo, hi = N.clip_codes(fmt)
    plain = [noise.pair_sigma(x, fmt.bits, fmt.matrix, fmt.range) for x in NP.hist_pairs_ref(pay, fmt, c["h"], c["w"], lo, hi)]
    mv, _ = block_motion_ref(pay, fmt, c["h"], c["w"], split=split)
    comp = [noise.pair_sigma(x, fmt.bits, fmt.matrix, fmt.range) for x in hist_pairs_mv_ref(pay, mv, fmt, c["h"], c["w"], lo, hi, split=split)]
    return noise.window_sigma_temporal(plain), noise.window_sigma_temporal(comp)


if __name__ == "__main__":                                        # the table of DESIGN.md 3.23
    worst = 0.0
    for name in CLIPS:
        for s in SIGMAS:
            rows = [clip_estimates(name, s, seed) for seed in SEEDS]
            every = clip_estimates(name, s, 0, split=False)[1]
            dev = max(abs(r[1] - s) / s for r in rows)
            if name in WHOLE:
                worst = max(worst, dev)
            print(f"{name:44s} sigma {s:2d}: plain {rows[0][0]:6.2f}  every block {every:6.2f}  split " + " / ".join(f"{r[1]:6.2f}" for r in rows)
                  + f"  worst deviation {100 * dev:.2f} %")
    print(f"largest relative deviation of the split estimate on the whole-pel clips, seeds {SEEDS}: {100 * worst:.2f} %")
