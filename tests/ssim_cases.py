"""The pairs of pictures the full-reference tests run on: seeded generators, numpy only, no stored pictures.  tools/make_ssim_golden.py runs the
reference implementation on exactly these and records its answers in tests/golden/ssim_cases.npz; the tests regenerate the inputs and compare.

A pair is a truth ``a`` -- texture (two sinusoids and a chirp), a blocky random field and a checker, in all three planes -- and a degraded copy ``b``: the
truth with a little less contrast and lifted blacks (so that "noise 0" is not "the same picture") plus seeded Gaussian noise, as codes of the case's
format.  The shapes are the smallest at which the kernel can still go wrong: both borders inside one window, one tile exactly, one position beyond a
tile both ways, partial tiles, rectangles at odd and even offsets, three different frames in one launch.

A case with ``level`` set is a near-flat pair instead, far from mid-grey or at it: all three planes of the truth are that one code, and the degraded copy is the
code plus seeded Gaussian noise of ``sigma`` codes OF THE CASE'S FORMAT, rounded and clipped to the format's range (0 .. 2^bits - 1).  There the variances are
tiny against the squares they are the difference of, and they are divided by something close to C2: sky, walls, night, bars -- what a denoiser outputs.  A
tuple of levels gives every frame its own."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import picture_ref as P
import yuv_ref as R

# rect: (x0, y0, w, h) or None; seeds: one per frame; sigma: noise in 8-bit codes (in the format's codes with ``level``); same: b is a;
# level: None, or the one code of a near-flat truth (a tuple: one per frame)
Case = namedtuple("Case", "name fmt H W rect seeds sigma same level", defaults=(None,))
_L8 = R.Fmt(8, R.C444, R.BT709, R.LIMITED)
_L8_420 = R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED)
_F8 = R.Fmt(8, R.C444, R.BT601, R.FULL)
_L10 = R.Fmt(10, R.C420_LEFT, R.BT709, R.LIMITED)
CASES = [
    Case("3x7", _L8, 3, 7, None, (31,), 5.0, False),                                         # both borders replicate inside one window
    Case("7x3", _L8, 7, 3, None, (32,), 5.0, False),
    Case("11x11", _L8, 11, 11, None, (33,), 5.0, False),                                     # the window itself
    Case("32x32", _L8, 32, 32, None, (34,), 5.0, False),                                     # exactly one tile
    Case("33x65", _L8, 33, 65, None, (35,), 5.0, False),                                     # one position beyond a tile both ways
    Case("70x100-sigma0", _L8, 70, 100, None, (36,), 0.0, False),
    Case("70x100-sigma2", _L8, 70, 100, None, (37,), 2.0, False),
    Case("70x100-sigma25", _L8, 70, 100, None, (38,), 25.0, False),
    Case("10bit-limited", R.Fmt(10, R.C420_LEFT, R.BT709, R.LIMITED), 40, 72, None, (39,), 5.0, False),
    Case("8bit-full", R.Fmt(8, R.C444, R.BT601, R.FULL), 40, 72, None, (40,), 5.0, False),
    Case("rect-odd-of-50x70-444", _L8, 50, 70, (3, 5, 41, 37), (41,), 5.0, False),           # odd origin, odd sides: no load of the picture is aligned
    Case("rect-of-96x128-420", _L8_420, 96, 128, (10, 8, 100, 70), (42,), 5.0, False),
    Case("T3", _L8_420, 40, 72, None, (43, 44, 45), 5.0, False),                             # three different pairs: the payload stride
    Case("same", _L8, 33, 65, None, (46,), 5.0, True),                                       # a == b: SSIM 1, PSNR inf
    # near-flat pairs (appended: the rows above keep their seeds and their recorded answers)
    Case("flat235-s1", _L8, 70, 100, None, (47,), 1.0, False, 235),                          # limited-range white
    Case("flat235-s2", _L8, 70, 100, None, (48,), 2.0, False, 235),
    Case("flat16-s1", _L8, 70, 100, None, (49,), 1.0, False, 16),                            # limited-range black
    Case("flat250-s1-full", _F8, 70, 100, None, (50,), 1.0, False, 250),
    Case("flat2-s1-full", _F8, 70, 100, None, (51,), 1.0, False, 2),                         # the noise clips at code 0
    Case("flat940-s4-10bit", _L10, 70, 100, None, (52,), 4.0, False, 940),
    Case("flat-T3", _L8, 33, 65, None, (53, 54, 55), 1.0, False, (235, 128, 16)),            # bright, mid-grey and dark in one launch: the payload stride
]
FLAT = tuple(c.name for c in CASES if c.level is not None)
BY_NAME = {c.name: c for c in CASES}


def _plane(h: int, w: int, rng, fx: float, fy: float) -> np.ndarray:
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    p1, p2 = rng.uniform(0, 2 * np.pi, 2)
    v = 0.5 + 0.16 * np.sin(2 * np.pi * (x / fx + y / 91) + p1) + 0.10 * np.sin(2 * np.pi * (x / 11 - y / fy) + p2) + 0.06 * np.sin(x * y / 640.0)
    v += 0.08 * np.kron(rng.normal(0, 1, ((h + 7) // 8, (w + 7) // 8)), np.ones((8, 8)))[:h, :w]
    v += 0.04 * ((((x // 6) + (y // 6)).astype(np.int64) & 1) - 0.5)
    return np.clip(v, 0.0, 1.0)


def _codes(v: np.ndarray, fmt: R.Fmt, chroma: bool) -> np.ndarray:
    s, top = 1 << (fmt.bits - 8), (1 << fmt.bits) - 1
    v = np.clip(v, 0.0, 1.0)
    if fmt.range == R.FULL:
        return np.rint(v * top).astype(np.int64)
    return np.rint((16 + (224 if chroma else 219) * v) * s).astype(np.int64)


def frame_pair(case: Case, seed: int):
    """((Ya, Ua, Va), (Yb, Ub, Vb)): int64 planes of the truth and of the degraded copy of one frame."""
    rng = np.random.default_rng(seed)
    ch, cw = R.chroma_shape(case.fmt, case.H, case.W)
    a, b = [], []
    if case.level is not None:
        level = case.level[case.seeds.index(seed)] if isinstance(case.level, tuple) else case.level
        for h, w in ((case.H, case.W), (ch, cw), (ch, cw)):
            a.append(np.full((h, w), level, np.int64))
            b.append(np.clip(np.rint(level + rng.normal(0, 1, (h, w)) * case.sigma), 0, (1 << case.fmt.bits) - 1).astype(np.int64))
        return tuple(a), tuple(b)
    for i, (h, w) in enumerate(((case.H, case.W), (ch, cw), (ch, cw))):
        v = _plane(h, w, rng, (37, 23, 29)[i], (17, 13, 19)[i])
        noise = rng.normal(0, 1, (h, w)) * (case.sigma / 255.0)
        a.append(_codes(v, case.fmt, i > 0))
        b.append(a[-1] if case.same else _codes(0.02 + 0.95 * v + noise, case.fmt, i > 0))
    return tuple(a), tuple(b)


def payloads(case: Case):
    """(a, b): uint8 [T, frame_bytes] each, the truth and the degraded copy."""
    pairs = [frame_pair(case, s) for s in case.seeds]
    return (np.stack([R.join_planes(*p[0], case.fmt) for p in pairs]), np.stack([R.join_planes(*p[1], case.fmt) for p in pairs]))


def pictures(case: Case):
    """Per frame ((Ya, Ua, Va), (Yb, Ub, Vb)) of the picture the numbers are of: the planes of the rectangle, or of the frame (int64)."""
    a, b = payloads(case)
    H, W = case.H, case.W
    if case.rect is not None:
        a, b = P.crop_payloads(a, case.fmt, H, W, case.rect), P.crop_payloads(b, case.fmt, H, W, case.rect)
        H, W = case.rect[3], case.rect[2]
    return [(R.split_planes(x, case.fmt, H, W), R.split_planes(y, case.fmt, H, W)) for x, y in zip(a, b)]


def upstream_scale(codes: np.ndarray, fmt: R.Fmt) -> np.ndarray:
    """Codes -> float64 on the reference's 0 .. 255 scale: the codes themselves at 8 bit, codes * 255 / 1023 at 10 bit."""
    return np.asarray(codes, np.float64) * (255.0 / ((1 << fmt.bits) - 1)) if fmt.bits != 8 else np.asarray(codes, np.float64)
