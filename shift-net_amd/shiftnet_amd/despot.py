"""Dirt, dust, blotches and dropouts taken out (``--despot T``): the option's grammar, the guard and the text of ``--despot_out``.  No numpy rule
lives here: the rule runs on the device (``sn_yuv_despot``, csrc/sn_despot.hip, along the vectors of ``sn_yuv_block_motion``), include/shiftnet_hip.h
states it and tests/despot_ref.py restates it.

Dirt is a small region that is wrong in exactly ONE frame.  The detector is the spike detection index of the film-restoration literature (Kokaram)
run along integer block vectors, in integers:

    A frame f of a clip (the stream, or its scene under a LISTED ``scene_cuts``) is repaired from the ORIGINAL frames f - 1, f, f + 1 only, so the
    result depends on neither chunks, windows nor order; a clip's first and last frame leave as they came.
    c = Y_f(y, x); p = Y_{f-1} and n = Y_{f+1} at the places the vectors of the sample's 16 x 16 block point to (clamped to the plane);
    a = c - p, b = c - n; d = min(|a|, |b|) if a and b are both positive or both negative, else 0.
    SEED iff d > T + |p - n|: ONE threshold, in 8-bit codes (times 2^(bits - 8)), raised by how much the two neighbours disagree with each other --
    what occlusion and a failed vector look like.
    CORE iff a seed with at least K seeds among its eight neighbours: dirt comes in blobs, noise in single samples.
    M = the core seeds dilated by the (2G + 1) x (2G + 1) square: a blotch has a soft edge that stays under T.
    A luma sample in M becomes (p + n + 1) >> 1; chroma ("follow") is repaired where its luma is, or ("off") left alone.
    Guard: a frame whose replaced share |M| / (h w) exceeds ``max_share`` is handed on as the ORIGINAL and marked kept -- a flash, a frame under
    uncorrected flicker, a cut the motion search could not follow.

**The limits.**  One threshold in codes, not scaled to the footage's noise.  Integer-pel vectors within +-7 px per 16 x 16 block, chosen on a block
that contains the dirt: a blotch larger than a good part of a block misleads its own vector.  Dirt at the same place in two consecutive frames,
vertical line scratches and anything else that persists are not found.  Small fast objects that are in one place for one frame (a ball, rain,
sparks) ARE taken for dirt.  The repair is the mean of two neighbours, which is soft.  Luma alone decides.  A clip's two end frames are never
repaired.  Nobody has judged it on real footage."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

DESPOT_MAX_T = 255
DESPOT_MAX_GROW = 2
CHROMA_MODES = ("follow", "off")
DEFAULT_SUPPORT, DEFAULT_GROW, DEFAULT_CHROMA, DEFAULT_MAX_SHARE = 2, 1, "follow", 0.05


def parse_despot(text: str) -> int:
    """--despot: T, the threshold in 8-bit codes: an integer 1 .. 255; anything else is a ValueError."""
    try:
        t = int(str(text).strip())
    except ValueError:
        t = 0
    if not (1 <= t <= DESPOT_MAX_T):
        raise ValueError(f"a threshold in 8-bit codes, 1 .. {DESPOT_MAX_T}, got {text!r}")
    return t


def _index(value, lo: int, hi: int) -> Optional[int]:
    ok = not isinstance(value, (bool, str, bytes, float)) and hasattr(value, "__index__")
    v = int(value) if ok else None
    return v if v is not None and lo <= v <= hi else None


def despot_form(despot, support=DEFAULT_SUPPORT, grow=DEFAULT_GROW, chroma=DEFAULT_CHROMA, max_share=DEFAULT_MAX_SHARE, add_noise=None,
                add_blur=None) -> Tuple[Optional[int], int, int, str, float]:
    """The restorer's ``despot`` / ``despot_support`` / ``despot_grow`` / ``despot_chroma`` / ``despot_max_share`` -> (None or T, K, G, chroma,
    max_share).  ValueError for anything else, for one of the four other than its default without ``despot``, and for ``despot`` together with
    ``add_noise`` or ``add_blur`` (whatever is not None)."""
    k, g = _index(support, 0, 8), _index(grow, 0, DESPOT_MAX_GROW)
    if k is None:
        raise ValueError(f"despot_support must be an integer 0 .. 8 (seeds among the eight neighbours), got {support!r}")
    if g is None:
        raise ValueError(f"despot_grow must be an integer 0 .. {DESPOT_MAX_GROW} (samples the mask grows by), got {grow!r}")
    if not isinstance(chroma, str) or chroma not in CHROMA_MODES:
        raise ValueError(f"despot_chroma must be one of {', '.join(CHROMA_MODES)}, got {chroma!r}")
    try:
        share = math.nan if isinstance(max_share, (bool, str, bytes)) else float(max_share)
    except (TypeError, ValueError):
        share = math.nan
    if not (0.0 < share <= 1.0):
        raise ValueError(f"despot_max_share must be a number in (0, 1] (the share of a frame that may be replaced), got {max_share!r}")
    if despot is None:
        for name, value, default in (("despot_support", k, DEFAULT_SUPPORT), ("despot_grow", g, DEFAULT_GROW), ("despot_chroma", chroma, DEFAULT_CHROMA),
                                     ("despot_max_share", share, DEFAULT_MAX_SHARE)):
            if value != default:
                raise ValueError(f"{name} says how despot finds and repairs dirt: it needs despot")
        return None, k, g, chroma, share
    t = _index(despot, 1, DESPOT_MAX_T)
    if t is None:
        raise ValueError(f"despot must be an integer 1 .. {DESPOT_MAX_T} (the threshold in 8-bit codes), got {despot!r}")
    for name, other in (("add_noise", add_noise), ("add_blur", add_blur)):
        if other is not None:
            raise ValueError(f"despot together with {name}: {name} makes a degraded copy of a clean stream for an experiment, despot repairs a "
                             "stream that carries dirt; pick one")
    return t, k, g, chroma, share


def frame_record(seeds: int, replaced: int, samples: int, max_share: float) -> Tuple[int, int, float, bool]:
    """The two counts of a frame of ``samples`` luma samples -> (seeds, replaced, share, kept): share = replaced / samples, one float64 division; kept
    (the guard: hand on the original) iff share > max_share."""
    share = int(replaced) / int(samples)
    return int(seeds), int(replaced), share, share > max_share


END_RECORD = (0, 0, 0.0, False)                                   # a clip's first or last frame: one neighbour only, it leaves as it came


def median_share(frames: Sequence[Tuple[int, int, float, bool]]) -> float:
    """The median of the frames' replaced shares (the mean of the middle two of an even number); 0 without frames."""
    s = sorted(f[2] for f in frames)
    n = len(s)
    return 0.0 if not n else (s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0)


def frames_kept(frames: Sequence[Tuple[int, int, float, bool]]) -> int:
    return sum(1 for f in frames if f[3])


def format_despot(frames: Sequence[Tuple[int, int, float, bool]]) -> str:
    """--despot_out: one line per frame, ``seeds replaced share kept`` (share as %.6f, kept as 0 / 1), then a last line with the median share and the
    number of frames kept."""
    lines = ["%d %d %.6f %d" % (f[0], f[1], f[2], 1 if f[3] else 0) for f in frames]
    lines.append("# median share replaced: %.6f; frames kept as they came (the guard): %d" % (median_share(frames), frames_kept(frames)))
    return "\n".join(lines) + "\n"
