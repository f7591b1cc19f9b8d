"""The active picture of a letterboxed or pillarboxed stream, for the video restorer (numpy only, no torch).

A picture rectangle is ``(x0, y0, w, h)`` in luma samples of the ``H x W`` stream.  The restorer then restores the rectangle as if it were the
whole video -- inside it the bytes are those of restoring the cropped stream -- and leaves every sample outside as it came in.  For 4:2:0
``x0`` and ``y0`` are even, ``w`` is even unless the rectangle reaches the frame's right edge and ``h`` unless it reaches the bottom edge, so that
no chroma sample is shared between the inside and the outside.

``decide_picture`` is the rule of ``picture="auto"``.  It looks at the sums ``sn_yuv_rowcol_sums`` (csrc/sn_yuv_stats.hip) writes: per frame the exact
integer sum of the luma codes of every row and of every column.  With ``black`` the format's black luma code (16 s limited, 0 full) and
``s = 2^(bits - 8)``:

  row y is a bar row iff ``rows[t][y] <= (black + level * s) * W`` for every frame t of the window (its mean is at most ``level`` 8-bit codes
  above black); column x likewise with ``cols[t][x]`` and ``H``;
  the bars are the maximal runs of bar rows from the top and from the bottom and of bar columns from the left and from the right;
  at 4:2:0 the near edges move up to even and the far edges down to even unless they are the frame's;
  no bars, everything bar (a black window) or a rectangle below the smallest legal size -> None: the full frame is restored.

The comparison is made on integers and one float64 product, the same on every host.

Where the restorer writes another format than it reads (``out_format``) the rectangle must be legal in both: ``out_fmt`` below.  If either is 4:2:0
the even-alignment rule applies, to a listed rectangle and to the one ``decide_picture`` finds.

A heuristic, checked on synthetic clips only.  Noisy analogue bars need a higher level; a part of the picture that stays at black for a whole
window is taken for bar and left as it is; a logo or a subtitle inside a bar ends the bar where it is.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

Rect = Tuple[int, int, int, int]
C444 = 0                                   # sn_yuv_fmt.chroma: SN_YUV_444; the other codes are 4:2:0
FULL = 1                                   # sn_yuv_fmt.range: SN_YUV_FULL
LEVEL = 1.0                                # the default bar level, in 8-bit code values above black
# The smallest picture: what the restorer takes as a whole frame.  It pads every frame to the network's multiple by repeating the edge (4 for
# the "small" topology, whose coarsest level is 1/4; 8 for "plus", coarsest 1/8), and the channel attention of every CAB wants a map of at least
# 2 x 2 (sn_cab_ca and its kin refuse less): the padded frame is at least 8 x 8 / 16 x 16, so the frame is at least 5 x 5 / 9 x 9.
SMALLEST = {"small": 5, "plus": 9}
MIN_SIDE = min(SMALLEST.values())          # where the network is not known (the command line's parser, a file): the laxest of the two


def smallest_picture(topo: str) -> int:
    """The smallest width and height of a frame, and therefore of a picture, that a network of topology ``topo`` restores."""
    return SMALLEST[topo]


def black_code(bits: int, range_: int) -> int:
    return 0 if range_ == FULL else 16 << (bits - 8)


def subsampled(fmt, out_fmt=None) -> bool:
    """Does the even-alignment rule of 4:2:0 apply: to ``fmt``, or to the format written where that is another (``out_fmt``)."""
    return fmt.chroma != C444 or (out_fmt is not None and out_fmt.chroma != C444)


def check_rect(rect, fmt, h: int, w: int, smallest: int = MIN_SIDE, out_fmt=None) -> Rect:
    """``rect`` as a tuple of four ints if it is a legal picture of an ``h x w`` stream of ``fmt`` (anything with ``.chroma``), else ValueError.
    ``smallest``: the least width and height (``smallest_picture(topo)`` where the network is known; 1 for the kernels alone).  ``out_fmt``: the
    format the stream is written in where it is not ``fmt``; the rectangle is then legal in both."""
    try:
        vals = tuple(rect)
        if len(vals) != 4 or any(isinstance(v, (bool, float, str)) or int(v) != v for v in vals):
            raise TypeError
        x0, y0, rw, rh = (int(v) for v in vals)
    except (TypeError, ValueError):
        raise ValueError(f"a picture rectangle is (x0, y0, w, h) in integers, got {rect!r}") from None
    if rw < smallest or rh < smallest:
        raise ValueError(f"picture {(x0, y0, rw, rh)}: the smallest picture the restorer takes is {smallest} x {smallest}, as the smallest frame")
    if x0 < 0 or y0 < 0 or x0 + rw > w or y0 + rh > h:
        raise ValueError(f"picture {(x0, y0, rw, rh)} does not lie inside the {w} x {h} frame")
    if subsampled(fmt, out_fmt):
        if x0 % 2 or y0 % 2:
            raise ValueError(f"picture {(x0, y0, rw, rh)}: x0 and y0 must be even at 4:2:0 (a chroma sample covers 2 x 2 luma samples)")
        if rw % 2 and x0 + rw != w:
            raise ValueError(f"picture {(x0, y0, rw, rh)}: an odd w is legal at 4:2:0 only where the picture reaches the frame's right edge ({w})")
        if rh % 2 and y0 + rh != h:
            raise ValueError(f"picture {(x0, y0, rw, rh)}: an odd h is legal at 4:2:0 only where the picture reaches the frame's bottom edge ({h})")
    return x0, y0, rw, rh


def _runs(bar: np.ndarray) -> Tuple[int, int]:
    """(length of the run of True from the start, from the end) of a boolean vector."""
    n = len(bar)
    nz = np.flatnonzero(~bar)
    return (n, n) if len(nz) == 0 else (int(nz[0]), n - 1 - int(nz[-1]))


def decide_picture(rows, cols, fmt, h: int, w: int, level: float = LEVEL, smallest: int = MIN_SIDE, out_fmt=None) -> Optional[Rect]:
    """rows: integers [T, h], cols: [T, w] -- the sums of the luma codes of every row and column of the T input frames of a window -> the picture
    of the window, or None for the full frame (the rule of the module text).  ``out_fmt``: as for check_rect; bits and range are ``fmt``'s, the sums'."""
    rows = np.asarray(rows).astype(np.int64).reshape(-1, h)
    cols = np.asarray(cols).astype(np.int64).reshape(-1, w)
    if len(rows) < 1 or len(rows) != len(cols):
        raise ValueError(f"decide_picture: need the sums of the same T >= 1 frames, got {len(rows)} and {len(cols)}")
    s = 1 << (fmt.bits - 8)
    code = black_code(fmt.bits, fmt.range) + float(level) * s
    top, bottom = _runs((rows <= code * w).all(axis=0))
    left, right = _runs((cols <= code * h).all(axis=0))
    if top == h or left == w:                              # everything is bar
        return None
    x0, y0, x1, y1 = left, top, w - right, h - bottom
    if subsampled(fmt, out_fmt):
        x0, y0 = x0 + (x0 & 1), y0 + (y0 & 1)
        x1 -= (x1 & 1) if x1 != w else 0
        y1 -= (y1 & 1) if y1 != h else 0
    if (x0, y0, x1, y1) == (0, 0, w, h):                    # no bars
        return None
    if x1 - x0 < smallest or y1 - y0 < smallest:
        return None
    return x0, y0, x1 - x0, y1 - y0


def check_pictures(rects: Iterable, fmt, h: int, w: int, smallest: int = MIN_SIDE, out_fmt=None) -> List[Optional[Rect]]:
    """A per-window list: every entry a legal rectangle, or None for the full frame."""
    return [None if r is None else check_rect(r, fmt, h, w, smallest, out_fmt) for r in rects]


def parse_pictures(text: str) -> List[Optional[Rect]]:
    """One window per line, in the order the windows are restored: ``x0 y0 w h``, or ``full`` for the full frame; '#' starts a comment, blank
    lines are skipped.  Anything else raises ValueError naming the line.  (Whether a rectangle fits the stream is checked where the stream is
    known.)"""
    out: List[Optional[Rect]] = []
    for no, line in enumerate(text.splitlines(), 1):
        words = line.split("#", 1)[0].split()
        if not words:
            continue
        if words == ["full"]:
            out.append(None)
            continue
        try:
            if len(words) != 4:
                raise ValueError("expected 'x0 y0 w h' or 'full'")
            try:
                x0, y0, rw, rh = (int(t) for t in words)
            except ValueError:
                raise ValueError("not four integers") from None
            if x0 < 0 or y0 < 0 or rw < 1 or rh < 1:
                raise ValueError("x0, y0 >= 0 and w, h >= 1")
            out.append((x0, y0, rw, rh))
        except ValueError as e:
            raise ValueError(f"line {no}: {line.strip()!r}: {e}") from None
    return out


def format_pictures(rects: Sequence[Optional[Sequence[int]]], how: str = "") -> str:
    rects = list(rects)
    head = (f"# picture per window (x0 y0 w h in luma samples, 'full' for the whole frame), in the order the windows are restored; "
            f"{len(rects)} window{'' if len(rects) == 1 else 's'}")
    return head + (f"; {how}" if how else "") + "\n" + "".join("full\n" if r is None else "%d %d %d %d\n" % tuple(r) for r in rects)


def read_pictures(path) -> List[Optional[Rect]]:
    with open(path, "r") as fh:
        return parse_pictures(fh.read())


def write_pictures(path, rects: Sequence[Optional[Sequence[int]]], how: str = "") -> None:
    with open(path, "w") as fh:
        fh.write(format_pictures(rects, how))
