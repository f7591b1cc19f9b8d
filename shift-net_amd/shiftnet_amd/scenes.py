"""Scene cuts of a video from luma thumbnails: the rule the video restorer uses to treat every scene as a clip of its own.

The thumbnails ``S_t`` are what ``sn_yuv_thumb`` (csrc/sn_yuv_stats.hip) writes: the integer sum of the luma codes of every 8 x 8 block of frame t,
``uint16 [ceil(H/8), ceil(W/8)]``.  From them, on the host and in exact integers:

  ``m[t]   = sum |S_t - S_(t-1)| / (H W 2^(bits-8))`` for t >= 1: the mean absolute difference of the 8 x 8 block means of two consecutive frames
             in 8-bit code units (float64 from an exact integer numerator); ``m[0]`` is 0.0 and is never looked at;
  ``ref[t] = median of the m[j], j != t, max(1, t-3) <= j <= min(last, t+3)`` that exist (0.0 if there is none);
  frame t starts a new scene iff ``m[t] >= threshold`` and ``m[t] >= ratio * ref[t]``.

Block means make the measure blind to noise and to one-pixel motion of fine texture; the median over the neighbours lets a cut stand out against
the shot's own motion level, whatever it is, and still finds a scene of a single frame (two cuts in a row: each is outvoted by the four ordinary
neighbours of the other).  The defaults, threshold 4.0 and ratio 2.5, are a HEURISTIC: they were checked on synthetic clips only and
nothing here is a measurement on real footage.  Fades and dissolves are not cuts and are not looked for.

No torch here: the module is used by the CPU tests and by the command line before a device exists.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

RADIUS = 3                       # neighbours on each side that vote in ref[t]: the decision for frame t needs frame t + RADIUS
THRESHOLD, RATIO = 4.0, 2.5      # heuristic defaults, see the module text


def block_diff(a: np.ndarray, b: np.ndarray) -> int:
    """sum |a - b| of two thumbnails as an exact integer."""
    return int(np.abs(a.astype(np.int64) - b.astype(np.int64)).sum())


def cut_measure(thumbs: np.ndarray, H: int, W: int, bits: int = 8) -> List[float]:
    """thumbs: [T, ceil(H/8), ceil(W/8)] integer block sums -> m, one value per frame (m[0] = 0.0)."""
    den = float(H * W * (1 << (bits - 8)))
    return [0.0] + [block_diff(thumbs[t], thumbs[t - 1]) / den for t in range(1, len(thumbs))]


def _median(v: Sequence[float]) -> float:
    if not v:
        return 0.0
    s = sorted(v)
    h = len(s) // 2
    return s[h] if len(s) % 2 else 0.5 * (s[h - 1] + s[h])


def cut_reference(m: Sequence[float], t: int) -> float:
    """ref[t] of the module text; m is indexed by frame and reaches at least to frame min(last frame of the stream, t + 3)."""
    last = len(m) - 1
    return _median([m[j] for j in range(max(1, t - RADIUS), min(last, t + RADIUS) + 1) if j != t])


def is_cut(m: Sequence[float], t: int, threshold: float = THRESHOLD, ratio: float = RATIO) -> bool:
    return t >= 1 and m[t] >= threshold and m[t] >= ratio * cut_reference(m, t)


def detect_cuts(m: Sequence[float], threshold: float = THRESHOLD, ratio: float = RATIO) -> List[int]:
    """The frames that start a new scene, from the measure of a whole sequence (m[t] for every frame t, m[0] ignored)."""
    return [t for t in range(1, len(m)) if is_cut(m, t, threshold, ratio)]


class CutDetector:
    """The same rule, incrementally: ``feed`` thumbnails in chunks of any size, every frame exactly once and in order; the decision for frame t
    is released once frame t + 3 has been fed or ``finish`` has said that the stream has ended.  ``feed`` / ``finish`` return the decisions
    they release as (frame, starts a scene) pairs; ``decided`` counts them, ``cuts`` lists the scene starts among them, ``m`` is the measure."""
    lookahead = RADIUS

    def __init__(self, H: int, W: int, bits: int = 8, threshold: float = THRESHOLD, ratio: float = RATIO) -> None:
        self.den = float(H * W * (1 << (bits - 8)))
        self.shape = ((H + 7) // 8, (W + 7) // 8)
        self.threshold, self.ratio = float(threshold), float(ratio)
        self.m: List[float] = []
        self.cuts: List[int] = []
        self.decided = 0
        self.ended = False
        self._prev: Optional[np.ndarray] = None
        self._cutset = set()

    def _release(self, upto: int) -> List[Tuple[int, bool]]:
        """Decide every frame below ``upto``.  Frame t < upto <= len(m) - RADIUS has its whole neighbourhood in m; at the end m is complete."""
        out = []
        while self.decided < upto:
            t = self.decided
            cut = is_cut(self.m, t, self.threshold, self.ratio)      # m reaches frame t + RADIUS, or the end of the stream
            if cut:
                self.cuts.append(t)
                self._cutset.add(t)
            out.append((t, cut))
            self.decided += 1
        return out

    def feed(self, thumbs: Iterable[np.ndarray]) -> List[Tuple[int, bool]]:
        if self.ended:
            raise ValueError("CutDetector.feed after finish")
        for s in thumbs:
            s = np.asarray(s)
            if s.shape != self.shape:
                raise ValueError(f"thumbnail of shape {s.shape}, the frame size says {self.shape}")
            s = s.astype(np.int64)
            self.m.append(0.0 if self._prev is None else int(np.abs(s - self._prev).sum()) / self.den)
            self._prev = s
        return self._release(len(self.m) - RADIUS)

    def finish(self) -> List[Tuple[int, bool]]:
        self.ended = True
        return self._release(len(self.m))

    def is_cut(self, t: int) -> bool:
        """The released decision for frame t."""
        if t >= self.decided:
            raise ValueError(f"the decision for frame {t} has not been released ({self.decided} have)")
        return t in self._cutset


class ListedCuts:
    """Scene starts given by the caller, in the form the frame source of the restorer asks a detector: every decision is known at once."""
    lookahead = 0
    decided = float("inf")

    def __init__(self, cuts: Iterable[int]) -> None:
        self.all = check_cuts(cuts)
        self._set = set(self.all)

    def feed(self, frames) -> None:
        pass

    def finish(self) -> None:
        pass

    def is_cut(self, t: int) -> bool:
        return t in self._set


def check_cuts(cuts: Iterable[int]) -> List[int]:
    """A list of scene starts: integers, each >= 1, strictly increasing."""
    out: List[int] = []
    for c in cuts:
        if isinstance(c, bool) or int(c) != c:
            raise ValueError(f"scene cuts must be integers, got {c!r}")
        c = int(c)
        if c < 1:
            raise ValueError(f"a scene cut must be a frame index >= 1 (frame 0 starts the first scene), got {c}")
        if out and c <= out[-1]:
            raise ValueError(f"scene cuts must be strictly increasing, got {c} after {out[-1]}")
        out.append(c)
    return out


def parse_cuts(text: str) -> List[int]:
    """One frame index per line; '#' starts a comment, blank lines are skipped.  Strictly increasing, each >= 1; anything else raises
    ValueError naming the line."""
    out: List[int] = []
    for no, line in enumerate(text.splitlines(), 1):
        word = line.split("#", 1)[0].strip()
        if not word:
            continue
        try:
            if not word.isdigit():                   # no signs, no spaces inside, no floats
                raise ValueError("not a frame index")
            out += check_cuts(out[-1:] + [int(word)])[-1:]
        except ValueError as e:
            raise ValueError(f"line {no}: {line.strip()!r}: {e}") from None
    return out


def format_cuts(cuts: Iterable[int]) -> str:
    """The text ``parse_cuts`` reads back to the same list."""
    cuts = list(cuts)
    return f"# scene starts (frame index, the first frame is 0); {len(cuts) + 1} scene{'s' if cuts else ''}\n" + "".join(f"{c}\n" for c in cuts)
