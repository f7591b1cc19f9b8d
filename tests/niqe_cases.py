"""The pictures and blocks the NIQE tests run on: seeded generators, numpy only, no stored pictures.  tools/make_niqe_golden.py runs the reference
implementation on exactly these and records its answers in tests/golden/niqe_cases.npz; the tests regenerate the inputs and compare.

A frame is texture (two sinusoids and a chirp), a blocky random field, a checker and seeded Gaussian noise, as luma codes of the case's format."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import yuv_ref as R

Case = namedtuple("Case", "name fmt H W rect seeds sigma flat")      # rect: (x0, y0, w, h) or None; seeds: one per frame; flat: see luma_codes
# The code of the flat area.  A constant picture should filter to itself, but the 49 float64 products of the reference's window with most codes add up
# to the code give or take an ulp, and the block's coefficients are then a residue of one sign (1e-14) whose "fit" enters the reference's mean.  131 is
# one of the codes (89, 91, 131, 135, 178, 182) at which the reference's sum, at both scales, the float64 restatement's and the kernel's float32 sum
# are all exact: the block's coefficients are exactly zero everywhere, and "cannot be fitted" means the same thing in all three.
FLAT = 131
FLAT_SIDE = 96 + 6        # block (0, 0) and what the filters of both scales reach beyond it: 3 samples at scale 1, 3 x 2 luma samples at scale 2

_L8 = R.Fmt(8, R.C444, R.BT709, R.LIMITED)
CASES = [
    Case("96x192", _L8, 96, 192, None, (11,), 5.0, False),                                   # the fewest blocks that give a score
    Case("192x288-sigma0", _L8, 192, 288, None, (12,), 0.0, False),
    Case("192x288-sigma10", _L8, 192, 288, None, (13,), 10.0, False),
    Case("200x300-crop", _L8, 200, 300, None, (14,), 5.0, False),                            # 8 rows and 12 columns that do not count
    Case("192x192-sigma25", _L8, 192, 192, None, (15,), 25.0, False),
    Case("192x288-flat-block", _L8, 192, 288, None, (16,), 5.0, True),                       # block (0, 0) cannot be fitted: an all-NaN row
    Case("10bit-limited", R.Fmt(10, R.C444, R.BT709, R.LIMITED), 96, 192, None, (17,), 5.0, False),
    Case("8bit-full", R.Fmt(8, R.C444, R.BT601, R.FULL), 96, 192, None, (18,), 5.0, False),
    Case("rect-of-240x400-420", R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED), 240, 400, (10, 8, 300, 200), (19,), 5.0, False),
    Case("T3", _L8, 96, 192, None, (20, 21, 22), 5.0, False),                                # three different frames: the payload stride
]
BY_NAME = {c.name: c for c in CASES}


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


def frames(case: Case) -> list:
    """The case's frames, int64 [H, W] luma codes each."""
    return [luma_codes(case.H, case.W, s, case.sigma, case.fmt, case.flat) for s in case.seeds]


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
