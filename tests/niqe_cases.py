"""The pictures and blocks the NIQE tests run on: seeded generators, numpy only, no stored pictures.  tools/make_niqe_golden.py runs the reference
implementation on exactly these and records its answers in tests/golden/niqe_cases.npz; the tests regenerate the inputs and compare.

A frame of kind "texture" is texture (two sinusoids and a chirp), a blocky random field, a checker and seeded Gaussian noise, as luma codes of the
case's format: variances in the hundreds.  The other kinds are what a denoiser writes -- one level or a shallow ramp plus noise of about a code
("level", "ramp"), blocks that are half dark texture and half bright near-flat ("mixed"), bright texture clipped at the legal limit ("clipped") -- and
frames of one code ("flat").  There the local variance is 0.1 to 1 against squares of up to 55 000."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import yuv_ref as R

# rect: (x0, y0, w, h) or None; seeds: one per frame; sigma: the noise, in 8-bit codes for kind "texture" and in the format's own codes otherwise;
# flat: see luma_codes; kind: the generator; level: the level of "level", "mixed" (its bright half) and "flat" in the format's own codes, the two ends of
# "ramp", the centre of "clipped", and with flat the code of the flat square (None: FLAT)
Case = namedtuple("Case", "name fmt H W rect seeds sigma flat kind level", defaults=("texture", None))
# The code of the flat area.  A constant picture should filter to itself, but the 49 float64 products of the reference's window with most codes add up
# to the code give or take an ulp, and the block's coefficients are then a residue of one sign (1e-14) whose "fit" enters the reference's mean.  131 is
# one of the codes (89, 91, 131, 135, 178, 182) at which the reference's sum, at both scales, is exact, so that "cannot be fitted" means the same thing
# to the reference and here.  The kernel and its restatement need no such luck: they filter the deviations from the block's own first sample, which
# are all zero in a flat area, so every product and sum is zero at every code whatever the taps add up to (FLAT_CASES and the flat-block-196 case: 196
# is one of the codes at which a float32 filter of the values themselves left a residue of 2.8e-5 of one sign).
FLAT = 131
FLAT_SIDE = 96 + 6        # block (0, 0) and what the filters of both scales reach beyond it: 3 samples at scale 1, 3 x 2 luma samples at scale 2

_L8 = R.Fmt(8, R.C444, R.BT709, R.LIMITED)
_F8 = R.Fmt(8, R.C444, R.BT601, R.FULL)
_L10 = R.Fmt(10, R.C444, R.BT709, R.LIMITED)
_F10 = R.Fmt(10, R.C444, R.BT709, R.FULL)
TEXTURED = [
    Case("96x192", _L8, 96, 192, None, (11,), 5.0, False),                                   # the fewest blocks that give a score
    Case("192x288-sigma0", _L8, 192, 288, None, (12,), 0.0, False),
    Case("192x288-sigma10", _L8, 192, 288, None, (13,), 10.0, False),
    Case("200x300-crop", _L8, 200, 300, None, (14,), 5.0, False),                            # 8 rows and 12 columns that do not count
    Case("192x192-sigma25", _L8, 192, 192, None, (15,), 25.0, False),
    Case("192x288-flat-block", _L8, 192, 288, None, (16,), 5.0, True),                       # block (0, 0) cannot be fitted: an all-NaN row
    Case("10bit-limited", _L10, 96, 192, None, (17,), 5.0, False),
    Case("8bit-full", _F8, 96, 192, None, (18,), 5.0, False),
    Case("rect-of-240x400-420", R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED), 240, 400, (10, 8, 300, 200), (19,), 5.0, False),
    Case("T3", _L8, 96, 192, None, (20, 21, 22), 5.0, False),                                # three different frames: the payload stride
]
# near-flat, mixed and clipped frames: tests/test_host_niqe.py checks that none of their 7 x 7 windows is constant at either scale (such a window is
# the flat case, which has cases of its own) -- at a sigma of 0.3 codes some 70 windows per block are, hence no sigma below 0.6 on a single level --
# and that no map value of the restatement is zero or below 1e-9 in magnitude, so that counts can be compared for equality across precisions.  On
# integer codes this close to one level a coefficient of exactly zero is not rare (deviations of +1 and -1 under equal taps cancel exactly: 9 of
# 83 000 coefficients with seed 35 at level 230, 45 on the ramp with seed 37); the seeds 100, 102 and 104 are the first at which there is none
NEAR_FLAT = [
    Case("level20-sigma0.6", _L8, 192, 288, None, (31,), 0.6, False, "level", 20),
    Case("level20-sigma1.5", _L8, 192, 288, None, (32,), 1.5, False, "level", 20),
    Case("level128-sigma0.6", _L8, 192, 288, None, (33,), 0.6, False, "level", 128),
    Case("level128-sigma1.5", _L8, 192, 288, None, (34,), 1.5, False, "level", 128),
    Case("level230-sigma0.6", _L8, 192, 288, None, (100,), 0.6, False, "level", 230),
    Case("level230-sigma1.5", _L8, 192, 288, None, (36,), 1.5, False, "level", 230),
    Case("ramp200-212-sigma0.4", _L8, 192, 288, None, (104,), 0.4, False, "ramp", (200, 212)),
    Case("8bit-full-level250", _F8, 192, 288, None, (102,), 0.6, False, "level", 250),
    Case("10bit-limited-level900", _L10, 192, 288, None, (39,), 2.0, False, "level", 900),
    Case("10bit-full-level1000", _F10, 192, 288, None, (40,), 2.0, False, "level", 1000),
    Case("mixed-40-228", _L8, 192, 288, None, (41,), 0.6, False, "mixed", 228),              # one offset per block cannot centre both halves
    Case("clipped-225-sigma3", _L8, 192, 288, None, (42,), 3.0, False, "clipped", 225),      # a share of the samples sits on 235
]
NEW_FORMATS = [
    # x0 = 10: the rectangle's rows start 20 bytes into a 2-byte pitch, so no wide load is aligned and every group goes element by element
    Case("rect-of-240x400-420-left-10bit", R.Fmt(10, R.C420_LEFT, R.BT709, R.LIMITED), 240, 400, (10, 8, 300, 200), (43,), 5.0, False),
]
CASES = TEXTURED + NEAR_FLAT + NEW_FORMATS                     # the cases whose score the reference implementation recorded
# as 192x288-flat-block, at a code where the reference implementation's own sums leave a residue in the flat block: it has no recorded score
PARTLY_FLAT = [Case("192x288-flat-block-196", _L8, 192, 288, None, (44,), 5.0, True, "texture", 196)]
# whole pictures of one code: no block can be fitted and the score is NaN.  The reference implementation has no answer here -- it fits the residue
# its own sums leave.  215 is the code at which the separable float64 filter of the values themselves, with the model's taps, leaves 2.8e-14; 49,
# 98, 125 and 196 (10 bit: among others 98 and 125) are codes at which the float32 one left 2.8e-5; the others are the ends of the ranges
FLAT_CASES = ([Case(f"flat-{v}", _L8, 96, 192, None, (0,), 0.0, False, "flat", v) for v in (16, 49, 98, 125, 196, 215, 235)]
              + [Case(f"flat-full-{v}", _F8, 96, 192, None, (0,), 0.0, False, "flat", v) for v in (0, 255)]
              + [Case(f"flat-10bit-{v}", _L10, 96, 192, None, (0,), 0.0, False, "flat", v) for v in (64, 98, 125, 513, 940)]
              + [Case("flat-10bit-full-1023", _F10, 96, 192, None, (0,), 0.0, False, "flat", 1023)])
BY_NAME = {c.name: c for c in CASES + PARTLY_FLAT + FLAT_CASES}


def legal(fmt: R.Fmt):
    """(lowest, highest) luma code of the format."""
    s = 1 << (fmt.bits - 8)
    return (0, (1 << fmt.bits) - 1) if fmt.range == R.FULL else (16 * s, 235 * s)


def luma_codes(h: int, w: int, seed: int, sigma: float, fmt: R.Fmt, flat: bool = False) -> np.ndarray:
    """int64 [h, w] luma codes of ``fmt``; ``sigma`` is the noise in 8-bit codes.  flat: the top-left FLAT_SIDE x FLAT_SIDE samples hold FLAT."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    p1, p2 = rng.uniform(0, 2 * np.pi, 2)
    v = 0.5 + 0.16 * np.sin(2 * np.pi * (x / 37 + y / 91) + p1) + 0.10 * np.sin(2 * np.pi * (x / 11 - y / 17) + p2) + 0.06 * np.sin(x * y / 640.0)
    v += 0.08 * np.kron(rng.normal(0, 1, ((h + 7) // 8, (w + 7) // 8)), np.ones((8, 8)))[:h, :w]
    v += 0.04 * ((((x // 6) + (y // 6)).astype(np.int64) & 1) - 0.5)
    v += rng.normal(0, 1, (h, w)) * (sigma / 255.0)
    v = np.clip(v, 0.0, 1.0)
    s, top = 1 << (fmt.bits - 8), (1 << fmt.bits) - 1
    codes = np.rint(v * top) if fmt.range == R.FULL else np.rint((16 + 219 * v) * s)
    codes = codes.astype(np.int64)
    if flat:
        codes[:FLAT_SIDE, :FLAT_SIDE] = FLAT
    return codes


def smooth_codes(case: Case, seed: int) -> np.ndarray:
    """int64 [H, W] luma codes of the kinds other than "texture": a level of the format's own codes plus Gaussian noise of ``sigma`` such codes,
    rounded and kept inside the format's legal range."""
    h, w, fmt = case.H, case.W, case.fmt
    lo, hi = legal(fmt)
    if case.kind == "flat":
        assert lo <= case.level <= hi
        return np.full((h, w), case.level, np.int64)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    noise = rng.normal(0, 1, (h, w)) * case.sigma
    if case.kind == "level":
        v = case.level + noise
    elif case.kind == "ramp":
        v = case.level[0] + (case.level[1] - case.level[0]) * x / (w - 1) + noise
    elif case.kind == "mixed":                                  # the left half of every 96-wide block: texture around 40; the right half: the level
        p1, p2 = rng.uniform(0, 2 * np.pi, 2)
        dark = 40 + 10 * np.sin(2 * np.pi * (x / 37 + y / 91) + p1) + 6 * np.sin(2 * np.pi * (x / 11 - y / 17) + p2) + 4 * rng.normal(0, 1, (h, w))
        v = np.where(x % 96 < 48, dark, case.level + noise)
    elif case.kind == "clipped":
        p1, p2 = rng.uniform(0, 2 * np.pi, 2)
        v = case.level + 4 * np.sin(2 * np.pi * (x / 37 + y / 91) + p1) + 3 * np.sin(2 * np.pi * (x / 11 - y / 17) + p2) + noise
    else:
        raise ValueError(case.kind)
    return np.clip(np.rint(v), lo, hi).astype(np.int64)


def frames(case: Case) -> list:
    """The case's frames, int64 [H, W] luma codes each."""
    if case.kind != "texture":
        return [smooth_codes(case, s) for s in case.seeds]
    out = [luma_codes(case.H, case.W, s, case.sigma, case.fmt, case.flat) for s in case.seeds]
    if case.flat and case.level is not None:
        for Y in out:
            Y[:FLAT_SIDE, :FLAT_SIDE] = case.level
    return out


def payloads(case: Case) -> np.ndarray:
    """uint8 [T, frame_bytes]: the frames with neutral chroma."""
    ch, cw = R.chroma_shape(case.fmt, case.H, case.W)
    c = np.full((ch, cw), 128 << (case.fmt.bits - 8), np.int64)
    return np.stack([R.join_planes(Y, c, c, case.fmt) for Y in frames(case)])


def picture(case: Case, Y: np.ndarray) -> np.ndarray:
    """The luma of the picture the score is of: the rectangle, or the frame."""
    if case.rect is None:
        return Y
    x0, y0, w, h = case.rect
    return Y[y0:y0 + h, x0:x0 + w]


def values(Y: np.ndarray, fmt: R.Fmt) -> np.ndarray:
    """Luma codes -> float64 on the 16 .. 235 scale of an 8-bit limited-range Y' (include/shiftnet_hip.h, sn_yuv_niqe_sums)."""
    Y = np.asarray(Y, np.float64)
    if fmt.range == R.FULL:
        return 16.0 + Y * (219.0 / ((1 << fmt.bits) - 1))
    return Y / (1 << (fmt.bits - 8))


def feature_blocks() -> list:
    """(name, float32 [B, B]) blocks of coefficients for the feature fit, B = 96 and 48: symmetric, heavy-tailed, skewed to either side, correlated,
    and one that is positive everywhere -- none of its products is negative, so the fit has an empty side."""
    rng = np.random.default_rng(4242)
    out = []
    for B in (96, 48):
        g = rng.normal(0, 1, (B, B))
        smooth = (g + np.roll(g, 1, 0) + np.roll(g, 1, 1) + np.roll(g, (1, 1), (0, 1))) / 2
        out += [(f"gauss{B}", 0.4 * g),
                (f"laplace{B}", rng.laplace(0, 0.3, (B, B))),
                (f"skew-right{B}", 0.3 * (rng.gamma(2.0, 1.0, (B, B)) - 1.6)),
                (f"skew-left{B}", -0.3 * (rng.gamma(1.5, 1.0, (B, B)) - 1.1)),
                (f"correlated{B}", 0.35 * smooth),
                (f"positive{B}", 0.2 * np.abs(rng.normal(0, 1, (B, B))) + 0.01)]
    return [(n, b.astype(np.float32)) for n, b in out]
