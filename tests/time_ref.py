"""A restatement of the restorer's windows that overlap in time (``VideoRestorer(window_overlap=V)``), not a test: the plan written position by
position, the cross-fade's weights, the cross-fade of ``sn_time_crossfade`` in float32 with every operation rounded on its own, its statistic as exact
Python integers, and ``seam_rms``.  Nothing here imports the product code."""
import math
from fractions import Fraction

import numpy as np

PAST, FUTURE = 2, 2


def reflect(i, n):
    """Frame i of a clip of n frames: mirrored about the first and the last frame without repeating it; clamped where n <= 2."""
    if n <= 2:
        return min(max(i, 0), n - 1)
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    return min(max(i, 0), n - 1)


def plan(n, one_len, V):
    """The windows of a clip of n frames, found frame by frame: a window is opened at its first frame and takes frames until it holds ``one_len`` of them
    or the clip ends; a window that did not reach the clip's end hands its last V frames to a successor that starts with them.  Per window
    (lo, cnt, indices, head, written)."""
    assert n >= 1 and one_len >= 1 and 0 <= V and 2 * V <= one_len
    out = []
    start, shared = 0, 0                       # the window being filled: its first frame, and how many of its first frames the one before holds too
    while True:
        frames = []
        f = start
        while f < n and len(frames) < one_len:
            frames.append(f)
            f += 1
        reaches_end = frames[-1] == n - 1
        keep_back = 0 if reaches_end else V
        idx = [reflect(i, n) for i in range(frames[0] - PAST, frames[-1] + 1 + FUTURE)]
        out.append((frames[0], len(frames), idx, shared, len(frames) - keep_back))
        if reaches_end:
            return out
        start, shared = frames[-1] + 1 - V, V


def scene_plan(n, one_len, cuts, V):
    """``plan`` of every scene on its own; a cut at or beyond n is ignored."""
    starts = [0] + [c for c in cuts if c < n]
    out = []
    for a, b in zip(starts, starts[1:] + [n]):
        out += [(a + lo, cnt, [a + i for i in idx], head, written) for lo, cnt, idx, head, written in plan(b - a, one_len, V)]
    return out


def weights(V):
    """(the older window's, the newer window's) float32 weights on shared frame j = 0 .. V - 1: (V - j) / (V + 1) and (j + 1) / (V + 1), each the exact
    fraction rounded once."""
    old = np.array([float(Fraction(V - j, V + 1)) for j in range(V)], dtype=np.float64).astype(np.float32)      # float(Fraction) is correctly rounded
    new = np.array([float(Fraction(j + 1, V + 1)) for j in range(V)], dtype=np.float64).astype(np.float32)
    return old, new


def crossfade(prev, cur, w_prev, w_cur):
    """prev, cur: float32 [V, C, Hp, Wp]; -> (w_prev[j] * prev) + (w_cur[j] * cur), two float32 products and one float32 sum, each rounded."""
    prev, cur = np.asarray(prev, np.float32), np.asarray(cur, np.float32)
    a = (np.asarray(w_prev, np.float32)[:, None, None, None] * prev).astype(np.float32)
    b = (np.asarray(w_cur, np.float32)[:, None, None, None] * cur).astype(np.float32)
    return (a + b).astype(np.float32)


def seam_sq(prev, cur, h, w):
    """-> [V][C] Python integers: over the h x w picture of every plane the sum of q * q, q = rint(min(max(prev - cur, -8), 8) * 65536) with the
    difference in float32 and ties to even."""
    prev, cur = np.asarray(prev, np.float32), np.asarray(cur, np.float32)
    d = (prev[:, :, :h, :w] - cur[:, :, :h, :w]).astype(np.float32)
    d = np.fmin(np.fmax(d, np.float32(-8)), np.float32(8))
    q = np.rint((d * np.float32(65536)).astype(np.float32))          # np.rint rounds half to even
    V, C = q.shape[:2]
    return [[sum(int(v) * int(v) for v in q[j, c].ravel()) for c in range(C)] for j in range(V)]


def seam_rms(sq_row, h, w):
    """The C sums of one shared frame -> the rms difference of the two answers in 8-bit code units."""
    return 255.0 * math.sqrt(sum(sq_row) / (2.0 ** 32 * len(sq_row) * h * w))
