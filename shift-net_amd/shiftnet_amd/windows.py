"""The pure part of the video restorer (shiftnet_amd/restore.py): which frames a window reads, the format a stream is written in, the
per-window options, and the frame source that turns an iterator of unknown length into windows.

No torch here: the module is used by the CPU tests and by the command line before a device exists.
"""
from __future__ import annotations

import queue
import threading
from typing import Iterable, Iterator, List, Optional, Tuple

import numpy as np

from .scenes import ListedCuts, check_cuts

PAST, FUTURE = 2, 2


# ---- the window planner -----------------------------------------------------------------------------------------------------------
def reflect_index(i: int, n: int) -> int:
    """Frame index i of a clip of n frames: reflection about the first / last frame without repeating it; clamped where n <= 2."""
    if n <= 2:
        return min(max(i, 0), n - 1)
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    return min(max(i, 0), n - 1)


def window_indices(k: int, one_len: int, n: int, past: int = PAST, future: int = FUTURE) -> Tuple[int, int, List[int]]:
    """(first restored frame, number restored, the past + number + future input frame indices) of window k of a clip of n frames."""
    lo = k * one_len
    hi = min(lo + one_len, n)
    return lo, hi - lo, [reflect_index(i, n) for i in range(lo - past, hi + future)]


def plan_windows(n: int, one_len: int, past: int = PAST, future: int = FUTURE) -> List[Tuple[int, int, List[int]]]:
    if n < 1 or one_len < 1:
        raise ValueError(f"plan_windows: need n >= 1 and one_len >= 1, got {n}, {one_len}")
    return [window_indices(k, one_len, n, past, future) for k in range((n + one_len - 1) // one_len)]


def plan_scene_windows(n: int, one_len: int, cuts: Iterable[int], past: int = PAST, future: int = FUTURE) -> List[Tuple[int, int, List[int]]]:
    """plan_windows of every scene [0, c_1), [c_1, c_2), ..., [c_k, n) on its own, indices shifted to the stream's.  Cuts at or beyond n are
    ignored."""
    if n < 1 or one_len < 1:
        raise ValueError(f"plan_scene_windows: need n >= 1 and one_len >= 1, got {n}, {one_len}")
    starts = [0] + [c for c in check_cuts(cuts) if c < n]
    plan = []
    for a, b in zip(starts, starts[1:] + [n]):
        plan += [(a + lo, cnt, [a + i for i in idx]) for lo, cnt, idx in plan_windows(b - a, one_len, past, future)]
    return plan


# ---- windows that overlap in time: consecutive windows of a scene share V frames, which are cross-faded --------------------------------------
def window_overlap_form(window_overlap, one_len: int) -> int:
    """-> V, the frames consecutive windows of a scene share: an integer with ``0 <= V`` and ``2 * V <= one_len``, so that a frame is covered by at most
    two windows.  0 is no overlap: the code path without any of it.  ValueError for anything else."""
    v = window_overlap
    if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)) or v < 0:
        raise ValueError(f"window_overlap must be an integer >= 0, got {window_overlap!r}")
    if 2 * int(v) > int(one_len):
        raise ValueError(f"window_overlap must be at most half of one_len ({int(one_len) // 2}), got {window_overlap!r}")
    return int(v)


def overlap_weights(overlap: int) -> Tuple[np.ndarray, np.ndarray]:
    """(the older window's weights, the newer window's) on the V shared frames, in time order, float32 [V] each: ``(V - j) / (V + 1)`` and
    ``(j + 1) / (V + 1)`` for j = 0 .. V - 1, computed in float64 and rounded once.  This is the ramp of ``tile_axis``: two tiles of side L that overlap
    by V, ``tile_axis(2 * L - V, L, V)``, have exactly these weights on the overlap."""
    j = np.arange(int(overlap), dtype=np.float64)
    return ((overlap - j) / (overlap + 1.0)).astype(np.float32), ((j + 1.0) / (overlap + 1.0)).astype(np.float32)


def plan_overlap_windows(n: int, one_len: int, overlap: int = 0, past: int = PAST, future: int = FUTURE) -> List[Tuple[int, int, List[int], int, int]]:
    """The windows of a clip of n frames when consecutive windows share ``overlap`` = V frames: per window (first restored frame ``lo``, number restored
    ``cnt``, the input frame indices, ``head``, ``written``).  Window 0 restores [0, min(one_len, n)); a window that restores [lo, hi) with hi < n is
    followed by one that starts at hi - V; a window with hi == n is the last.  The indices are ``reflect_index`` over lo - past .. hi + future - 1, as
    ``plan_windows``'s.  ``head``: how many of the window's first frames the predecessor has restored as well and are cross-faded with its answer
    (``overlap_weights``): 0 for window 0, V after it.  ``written``: the window writes its first ``written`` frames, [lo, lo + written): all ``cnt`` if it
    is the last, else ``cnt - V`` -- its last V frames wait for the successor.  So every frame is written exactly once and in order, at most two windows
    cover a frame, and a window after the first has at least V + 1 frames.  With V = 0 the first three fields are ``plan_windows``'s."""
    if n < 1 or one_len < 1:
        raise ValueError(f"plan_overlap_windows: need n >= 1 and one_len >= 1, got {n}, {one_len}")
    overlap = window_overlap_form(overlap, one_len)
    plan, lo = [], 0
    while True:
        hi = min(lo + one_len, n)
        last = hi == n
        plan.append((lo, hi - lo, [reflect_index(i, n) for i in range(lo - past, hi + future)], overlap if plan else 0, hi - lo - (0 if last else overlap)))
        if last:
            return plan
        lo = hi - overlap


def plan_scene_overlap_windows(n: int, one_len: int, cuts: Iterable[int], overlap: int = 0, past: int = PAST,
                               future: int = FUTURE) -> List[Tuple[int, int, List[int], int, int]]:
    """plan_overlap_windows of every scene on its own, indices shifted to the stream's, as ``plan_scene_windows`` does for ``plan_windows``: the overlap
    never crosses a scene start, every scene begins with a window that has no predecessor."""
    if n < 1 or one_len < 1:
        raise ValueError(f"plan_scene_overlap_windows: need n >= 1 and one_len >= 1, got {n}, {one_len}")
    starts = [0] + [c for c in check_cuts(cuts) if c < n]
    plan = []
    for a, b in zip(starts, starts[1:] + [n]):
        plan += [(a + lo, cnt, [a + i for i in idx], head, written) for lo, cnt, idx, head, written in plan_overlap_windows(b - a, one_len, overlap, past, future)]
    return plan


def format_seams(seams) -> str:
    """``stats["seam_rms"]`` as text, one line per window: ``-`` (no seam) or the V numbers, written so that ``parse_seams`` gives them back exactly."""
    return "# rms difference of the two answers on every shared frame, 8-bit code units, oldest first; one line per window, - : no seam\n" + \
        "".join(("-" if s is None else " ".join(repr(float(v)) for v in s)) + "\n" for s in seams)


def parse_seams(text: str):
    """The inverse of ``format_seams``: per window None or the list of floats ('#' comments)."""
    out = []
    for line in text.splitlines():
        line = line.split("#", 1)[0].strip()
        if line:
            out.append(None if line == "-" else [float(v) for v in line.split()])
    return out


DITHERS = ("tpdf",)


def plan_output(fmt, out_format=None, dither=None, dither_seed=0):
    """(the format written, the dither word or None, the seed) for a stream read as ``fmt`` (anything with bits, chroma, matrix, range that is built
    from the four): ``out_format`` is a C tag of y4m.MODES and changes bit depth and chroma layout only, matrix and range stay the input's; None,
    or a tag that says what ``fmt`` says, returns ``fmt`` itself.  ValueError for an unknown tag, a dither word other than None / "tpdf", and a seed
    outside 0 .. 2^32 - 1."""
    from .y4m import MODES
    out = fmt
    if out_format is not None:
        if not isinstance(out_format, str) or out_format not in MODES:
            raise ValueError(f"out_format must be None or one of {', '.join(MODES)}, got {out_format!r}")
        bits, chroma = MODES[out_format]
        if (bits, chroma) != (fmt.bits, fmt.chroma):
            out = type(fmt)(bits, chroma, fmt.matrix, fmt.range)
    if dither is not None and not (isinstance(dither, str) and dither in DITHERS):
        raise ValueError(f"dither must be None or 'tpdf', got {dither!r}")
    if isinstance(dither_seed, (bool, float, str)) or int(dither_seed) != dither_seed or not (0 <= int(dither_seed) < 2 ** 32):
        raise ValueError(f"dither_seed must be an integer in 0 .. 2^32 - 1, got {dither_seed!r}")
    return out, dither, int(dither_seed)


def pad_multiple(topo: str) -> int:
    return 8 if topo == "plus" else 4


def padded_size(h: int, w: int, topo: str) -> Tuple[int, int]:
    m = pad_multiple(topo)
    return (h + m - 1) // m * m, (w + m - 1) // m * m


# ---- tiles: a window's frames cut into overlapping rectangles of one size, and the weights that blend their results ------------------
DEFAULT_TILE_OVERLAP = 32      # upstream's four quadrants crop 17 to 32 samples per side (cli.quadrant_forward); nobody has tuned it


def tile_axis(length: int, side: int, overlap: int) -> Tuple[List[int], np.ndarray]:
    """One axis of plan_tiles: (the origins of the tiles, their weights as float64 [n][min(side, length)]).

    ``side >= length``: one tile [0, length) of weight 1.  Otherwise ``step = side - overlap``, ``n = ceil((length - side) / step) + 1`` tiles at
    ``o_k = min(k * step, length - side)``: all of one size, the last at the far edge, consecutive ones overlapping by at least ``overlap``.
    The weight of tile k at position p is ``t_k(p) / sum_j t_j(p)`` over the tiles j that cover p, with
    ``t_k(p) = min(p - o_k + 1 if k > 0, o_k + side - p if k < n - 1)``: a ramp towards every edge the tile shares with a neighbour and none at the
    picture's own edges; a lone tile has weight 1.  Where one tile covers p the weight is exactly 1.0, where two tiles face each other with their
    ramps the cross-fade is linear, and where the shifted last tile overlaps its neighbour by more than half a side the weights are still positive
    and still sum to 1."""
    if length < 1 or side < 1 or not (0 <= overlap < side):
        raise ValueError(f"tile_axis: need length >= 1, side >= 1 and 0 <= overlap < side, got {length}, {side}, {overlap}")
    if side >= length:
        return [0], np.ones((1, length), dtype=np.float64)
    step = side - overlap
    n = -(-(length - side) // step) + 1
    origins = [min(k * step, length - side) for k in range(n)]
    t = np.zeros((n, length), dtype=np.float64)
    for k, o in enumerate(origins):
        p = np.arange(o, o + side, dtype=np.float64)
        ramp = np.full(side, np.inf)
        if k > 0:
            ramp = np.minimum(ramp, p - o + 1)
        if k < n - 1:
            ramp = np.minimum(ramp, o + side - p)
        t[k, o:o + side] = ramp                                   # n >= 2 here: every tile has a neighbour, so no inf stays
    total = t.sum(axis=0)
    return origins, np.stack([t[k, o:o + side] / total[o:o + side] for k, o in enumerate(origins)])


class TilePlan:
    """plan_tiles' result: the tile's size (th, tw) as run -- clipped to the picture --, the origins ``ys`` and ``xs`` per axis, the float32 weight
    tables ``wy`` [len(ys)][th] and ``wx`` [len(xs)][tw] (computed in float64, rounded once), and ``tiles``: (y0, x0, th, tw) in row-major order,
    the order they are run and accumulated in.  The weight of tile (i, j) at (y, x) is ``wy[i][y] * wx[j][x]``."""

    def __init__(self, hp: int, wp: int, th: int, tw: int, overlap: int) -> None:
        self.ys, wy = tile_axis(hp, th, overlap)
        self.xs, wx = tile_axis(wp, tw, overlap)
        self.wy, self.wx = wy.astype(np.float32), wx.astype(np.float32)
        self.th, self.tw = self.wy.shape[1], self.wx.shape[1]
        self.tiles = [(y0, x0, self.th, self.tw) for y0 in self.ys for x0 in self.xs]

    @property
    def single(self) -> bool:
        """One tile that is the whole picture: nothing to blend."""
        return len(self.tiles) == 1


def plan_tiles(hp: int, wp: int, th: int, tw: int, overlap: int) -> TilePlan:
    """The tiles of an hp x wp picture (the padded size the network is fed) for tiles of th x tw that overlap by at least ``overlap`` samples: per
    axis ``tile_axis``.  Pure: the same plan for every window of one size."""
    return TilePlan(int(hp), int(wp), int(th), int(tw), int(overlap))


def tile_form(tile, tile_overlap=DEFAULT_TILE_OVERLAP, topo: str = "small"):
    """-> None (no tiles: the code path without any of it) or (th, tw, overlap).  ``tile``: None, an int n (n x n) or (th, tw); both sides multiples
    of ``pad_multiple(topo)`` and at least twice it (the network takes no map one pixel high at its coarsest level); ``tile_overlap``: an int with
    ``0 <= overlap <= min(th, tw) // 2``, judged even where ``tile`` is None.  ValueError for anything else."""
    def integer(v) -> bool:
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if not integer(tile_overlap) or tile_overlap < 0:
        raise ValueError(f"tile_overlap must be an integer >= 0, got {tile_overlap!r}")
    if tile is None:
        return None
    m = pad_multiple(topo)
    if integer(tile):
        pair = (int(tile), int(tile))
    else:
        try:
            pair = () if isinstance(tile, (str, bytes)) else tuple(tile)
        except TypeError:
            pair = ()
        if len(pair) != 2 or not all(integer(v) for v in pair):
            raise ValueError(f"tile must be None, an integer n (n x n) or (th, tw), got {tile!r}")
        pair = (int(pair[0]), int(pair[1]))
    if not all(v >= 2 * m and v % m == 0 for v in pair):
        raise ValueError(f"tile: both sides must be multiples of {m} and at least {2 * m} for this network, got {tile!r}")
    if tile_overlap > min(pair) // 2:
        raise ValueError(f"tile_overlap must be at most half the tile's shorter side ({min(pair) // 2}), got {tile_overlap!r}")
    return pair[0], pair[1], int(tile_overlap)


# ---- per-window options: one value for the stream, or a list with one entry per window ---------------------------------------------
class PerWindow:
    """An option of the restorer that is one value for the stream (``listed=False``) or a list with one entry per window in the order the
    windows are restored.  How many windows a stream has is known only at its end, so a list that is too short is found at the window
    without an entry."""

    def __init__(self, name: str, value, listed: bool) -> None:
        self.name, self.value, self.listed = name, value, listed

    def at(self, k: int):
        if not self.listed:
            return self.value
        n = len(self.value)
        if k >= n:
            raise ValueError(f"{self.name} lists {n} window{'' if n == 1 else 's'}, window {k} has no entry")
        return self.value[k]


# The accepted forms of the options, each -> (mode, value).  What depends on the network (deblur or denoise) is judged by the caller.
def scene_cuts_form(scene_cuts):
    """None -> ("off", None); "auto" -> ("auto", "auto"); an iterable of frame indices -> ("list", the checked list)."""
    if scene_cuts is None:
        return "off", None
    if isinstance(scene_cuts, str):
        if scene_cuts != "auto":
            raise ValueError(f"scene_cuts must be None, 'auto' or an iterable of frame indices, got {scene_cuts!r}")
        return "auto", "auto"
    return "list", check_cuts(scene_cuts)


def sigma_form(sigma):
    """None or a number -> ("fixed", PerWindow of None or the float); "auto" -> ("auto", None); a sequence -> ("list", PerWindow of the checked list)."""
    if isinstance(sigma, str):
        if sigma != "auto":
            raise ValueError(f"sigma must be a number, 'auto' or a sequence of numbers, got {sigma!r}")
        return "auto", None
    if sigma is not None and hasattr(sigma, "__iter__"):
        from .noise import check_sigmas
        return "list", PerWindow("sigma", check_sigmas(sigma), True)
    return "fixed", PerWindow("sigma", None if sigma is None else float(sigma), False)


def noise_model_form(noise_model):
    """None -> (None, None); "level" -> ("level", None); a list of curves -> ("list", PerWindow of the checked list)."""
    if noise_model is None:
        return None, None
    if isinstance(noise_model, str) and noise_model == "level":
        return "level", None
    if isinstance(noise_model, str) or not hasattr(noise_model, "__iter__"):
        raise ValueError(f"noise_model must be None, 'level' or a list of curves, got {noise_model!r}")
    from .noise import check_curves
    return "list", PerWindow("noise_model", check_curves(noise_model), True)


def sigma_estimator_form(sigma_estimator, sigma_mode: str = "auto") -> str:
    """"spatial" | "temporal" | "min" -> the word; ValueError for any other, and for one that is not "spatial" unless the sigma is estimated
    (``sigma_mode`` of ``sigma_form``): only sigma="auto" has an estimate to choose."""
    from .noise import check_estimator
    word = check_estimator(sigma_estimator)
    if word != "spatial" and sigma_mode != "auto":
        raise ValueError(f"sigma_estimator={word!r} chooses how sigma='auto' estimates the noise level: it needs sigma='auto'")
    return word


MOTIONS = ("blocks",)


def sigma_motion_form(sigma_motion, sigma_estimator: str = "min"):
    """None | "blocks" -> the same; ValueError for anything else, and for "blocks" with sigma_estimator="spatial": the vectors compensate the frame
    pairs of the temporal estimate, and the spatial one has no pairs."""
    if sigma_motion is None:
        return None
    if not (isinstance(sigma_motion, str) and sigma_motion in MOTIONS):
        raise ValueError(f"sigma_motion must be None or 'blocks', got {sigma_motion!r}")
    if sigma_estimator == "spatial":
        raise ValueError(f"sigma_motion={sigma_motion!r} compensates the frame pairs of the temporal estimate: it needs sigma_estimator='temporal' or 'min', "
                         "not 'spatial'")
    return sigma_motion


VIEWS = ("removed",)


def amount_form(amount, view=None, removed_gain=1.0):
    """-> (the mix ``egress_yuv`` takes or None, the amounts (ay, ac) or None, the view or None).  ``amount``: None, a number (both planes) or
    (luma, chroma), each in [0, 1]; ``view``: None or "removed", which shows input minus result around mid-grey times ``removed_gain`` (finite,
    >= 0) and goes with no amount other than None or 1.  None, 1 or (1, 1) without a view is no mix: the code path without any of this."""
    import math
    if amount is None:
        pair = None
    else:
        try:
            pair = () if isinstance(amount, str) else (tuple(float(v) for v in amount) if hasattr(amount, "__iter__") else (float(amount),) * 2)
        except (TypeError, ValueError):
            pair = ()
        if len(pair) != 2 or not all(0.0 <= v <= 1.0 for v in pair):                # refuses NaN as well
            raise ValueError(f"amount must be None, a number in [0, 1] or (luma, chroma) with both in [0, 1], got {amount!r}")
    if view is not None and not (isinstance(view, str) and view in VIEWS):
        raise ValueError(f"view must be None or 'removed', got {view!r}")
    full = pair is None or pair == (1.0, 1.0)
    if view is None:
        return (None if full else ("amount",) + pair), pair, None
    if not full:
        raise ValueError(f"view='removed' shows what the full restoration took out: it goes with amount None or 1, got {amount!r}")
    try:
        gain = math.nan if isinstance(removed_gain, (bool, str)) else float(removed_gain)
    except (TypeError, ValueError):
        gain = math.nan
    if not (math.isfinite(gain) and gain >= 0.0):
        raise ValueError(f"removed_gain must be a finite number >= 0, got {removed_gain!r}")
    return ("removed", gain, gain), pair, view


def report_form(report=False, report_edge=16.0, view=None):
    """-> (whether the method-noise report is made, its edge threshold in 8-bit code units).  ``report``: False or True; ``report_edge``: finite and
    >= 0; ``view="removed"`` with the report is refused: the report describes the stream that was written, and that view writes the difference itself."""
    import math
    if not isinstance(report, (bool, np.bool_)):
        raise ValueError(f"report must be False or True, got {report!r}")
    try:
        edge = math.nan if isinstance(report_edge, (bool, str)) else float(report_edge)
    except (TypeError, ValueError):
        edge = math.nan
    if not (math.isfinite(edge) and edge >= 0.0):
        raise ValueError(f"report_edge must be a finite number >= 0 (8-bit code units), got {report_edge!r}")
    if report and view is not None:
        raise ValueError(f"report=True measures input minus the stream written, and view={view!r} writes that difference instead of the restored "
                         "frames: use one or the other")
    return bool(report), edge


REPORT_MOTIONS = ("blocks",)


def report_motion_form(report_motion=None, report=False):
    """None | "blocks" -> the same; ValueError for anything else, and for "blocks" without ``report=True``: the vectors compensate the report's temporal
    correlation, and without the report there is nothing to compensate."""
    if report_motion is None:
        return None
    if not (isinstance(report_motion, str) and report_motion in REPORT_MOTIONS):
        raise ValueError(f"report_motion must be None or 'blocks', got {report_motion!r}")
    if not (isinstance(report, (bool, np.bool_)) and report):
        raise ValueError(f"report_motion={report_motion!r} follows the picture in the report's temporal correlation: it needs report=True")
    return report_motion


REPORT_QUALITIES = ("niqe",)


def quality_form(report_quality=None, niqe_params=None, report=False):
    """-> None (no quality score: the code path without any of it) or (mu[36], cov[36, 36], win7[7]), the pristine model of niqe.load_params read from
    ``niqe_params`` (None: tests/golden/niqe_pris_params.npz of the checkout).  ``report_quality``: None | "niqe".  ValueError for anything else, for
    "niqe" without ``report=True`` (the score is two more columns of the report), for ``niqe_params`` without "niqe", and for a model file that is
    missing or is not one -- that message names the option."""
    if report_quality is None:
        if niqe_params is not None:
            raise ValueError(f"niqe_params={niqe_params!r} is the model of report_quality='niqe': it needs that option")
        return None
    if not (isinstance(report_quality, str) and report_quality in REPORT_QUALITIES):
        raise ValueError(f"report_quality must be None or 'niqe', got {report_quality!r}")
    if not (isinstance(report, (bool, np.bool_)) and report):
        raise ValueError(f"report_quality={report_quality!r} adds the score of the input and of the written frame to the report: it needs report=True")
    import zipfile
    from . import niqe
    path = niqe.default_params_path() if niqe_params is None else niqe_params
    try:
        return niqe.load_params(path)
    except (OSError, KeyError, ValueError, zipfile.BadZipFile) as e:
        raise ValueError(f"niqe_params: the pristine model of report_quality='niqe' could not be read from {path!r} ({e}); "
                         "name the file with niqe_params= / --niqe_params") from None


def ensemble_form(ensemble=None, ensemble_time=False, tile=None):
    """-> None (no ensemble: the code path without any of it) or (ensemble, time, the members' ops in the order they run).  ``ensemble``: None, 1, 2, 4
    or 8 (ensemble.members); ``ensemble_time``: a bool.  One member -- None or 1 without time -- is no ensemble.  ``tile``: the restorer's parsed tile;
    an ensemble together with tiles is a ValueError (a tile of a transposed member needs a rule for its own sides: a follow-up).  ValueError for
    anything else."""
    from .ensemble import members
    if not isinstance(ensemble_time, (bool, np.bool_)):
        raise ValueError(f"ensemble_time must be a bool, got {ensemble_time!r}")
    if isinstance(ensemble, np.integer):
        ensemble = int(ensemble)
    ops = members(ensemble, bool(ensemble_time))
    if len(ops) == 1:
        return None
    if tile is not None:
        raise ValueError("ensemble / ensemble_time cannot be combined with tile: the tiles of a transposed member need a rule of their own")
    return (1 if ensemble is None else ensemble), bool(ensemble_time), ops


def picture_form(picture):
    """None -> ("full", None); "auto" -> ("auto", None); four numbers -> ("fixed", the tuple); anything whose elements are sequences or None ->
    ("list", the list).  The rectangles are judged where the stream is known (picture.check_pictures)."""
    if picture is None:
        return "full", None
    if isinstance(picture, str):
        if picture != "auto":
            raise ValueError(f"picture must be None, 'auto', (x0, y0, w, h) or a list of rectangles, got {picture!r}")
        return "auto", None
    picture = list(picture)
    if len(picture) == 4 and not any(r is None or hasattr(r, "__iter__") for r in picture):
        return "fixed", tuple(picture)
    return "list", picture


# ---- frame source: look-ahead over an iterator whose length is unknown until it ends ----------------------------------------------
class _SceneFrames:
    """The windows of plan_scene_windows from an iterator of unknown length, with the cut decisions arriving late.  ``decider``
    (scenes.ListedCuts, scenes.CutDetector behind the restorer's _DeviceThumbs, or anything shaped like them) is fed every frame exactly once
    and in order, in chunks, and answers ``is_cut(t)`` for t < ``decided``; it needs ``lookahead`` frames beyond t to decide t.

    The window that restores [lo, lo + L) of a scene that started at a reads frames lo - 2 .. lo + L + 1 unless the scene ends before: it
    depends on the decisions for lo + 1 .. lo + L + 1, so it is handed out once frame lo + L + 1 + lookahead has been read or the stream has
    ended.  Frames before max(a, lo - 2) of the next window are dropped: at most L + 4 + lookahead + 1 are held.

    ``overlap`` = V > 0 hands out plan_scene_overlap_windows' instead: the window after [lo, hi) starts at hi - V unless the scene ended at hi.  While
    the scene's end is not known it lies beyond the window's last input frame, so that window is not the scene's last.  ``head`` and ``written`` are
    those of the window handed out last; the next window reaches back to hi - V - 2, so V more frames are held."""

    def __init__(self, it: Iterable[np.ndarray], decider) -> None:
        self.it = iter(it)
        self.decider = decider
        self.base = 0                     # index of buf[0]
        self.buf: List[np.ndarray] = []
        self.n: Optional[int] = None      # known once the iterator ends
        self.fed = 0                      # frames handed to the decider
        self.finished = False             # the decider has been told that the stream has ended
        self.a = 0                        # first frame of the current scene
        self.lo = 0                       # next frame to restore
        self.k = 0
        self.cuts: List[int] = []         # the scene starts used
        self.clip_lo = 0                  # the first restored frame of the window handed out last, counted from the first frame of its clip: the scene
        self.head = 0                     # ... how many of its first frames are shared with its predecessor (0, or the overlap)
        self.written = 0                  # ... and how many of its frames, from the first on, it writes

    def _fill(self, upto: int) -> None:
        while self.n is None and self.base + len(self.buf) <= upto:
            try:
                self.buf.append(next(self.it))
            except StopIteration:
                self.n = self.base + len(self.buf)
        have = self.base + len(self.buf)
        if have > self.fed:
            self.decider.feed(self.buf[self.fed - self.base:])
            self.fed = have
        if self.n is not None and not self.finished:
            self.decider.finish()
            self.finished = True

    def window(self, k: int, one_len: int, overlap: int = 0) -> Optional[Tuple[int, int, List[np.ndarray]]]:
        """The frames of the k-th window of the stream (k counts up from 0 across the scenes), or None past the end."""
        assert k == self.k, "windows are handed out in order"
        lo, a = self.lo, self.a
        last = lo + one_len + FUTURE - 1                                      # the last frame this window can read
        self._fill(last + self.decider.lookahead)
        n = self.n if self.n is not None else self.base + len(self.buf)      # not at the end: n > last
        if lo >= n:
            return None
        cut = next((t for t in range(lo + 1, min(last, n - 1) + 1) if self.decider.is_cut(t)), None)
        # the scene's end.  Without a cut in reach and before the end of the stream it is not known, only that it lies beyond `last`: then no
        # index of this window reflects about it, and n (> last) stands in for it with the same result
        b = cut if cut is not None else n
        hi = min(lo + one_len, b)
        frames = [self.buf[a + reflect_index(i - a, b - a) - self.base] for i in range(lo - PAST, hi + FUTURE)]
        self.k += 1
        ended = hi == b                                                       # the scene ends with this window (a stand-in b lies beyond hi)
        self.head = overlap if lo > a else 0
        self.written = hi - lo - (0 if ended else overlap)
        self.lo = hi if ended else hi - overlap
        self.clip_lo = lo - a
        if cut is not None and hi == cut:
            self.a = cut
            self.cuts.append(cut)
        drop = max(self.a, self.lo - PAST) - self.base                        # the next window reaches back to here
        if drop > 0:
            del self.buf[:drop]
            self.base += drop
        return lo, hi - lo, frames

    def windows(self, one_len: int, overlap: int = 0) -> Iterator[Tuple[int, List[np.ndarray], int]]:
        """(k, the frames of window k, its clip_lo) of every window of the stream, in order."""
        k = 0
        while True:
            win = self.window(k, one_len, overlap)
            if win is None:
                return
            yield k, win[2], self.clip_lo
            k += 1


class _Frames(_SceneFrames):
    """The source of a stream that is one clip: no frame starts a scene, so the windows are plan_windows'."""

    def __init__(self, it: Iterable[np.ndarray]) -> None:
        super().__init__(it, ListedCuts(()))


class _Thread(threading.Thread):
    """A producer thread: runs fn(put) and forwards its exception to the consumer of the queue."""
    END = object()

    def __init__(self, fn, depth: int) -> None:
        super().__init__(daemon=True)
        self.q: "queue.Queue" = queue.Queue(maxsize=depth)
        self.fn, self.stop = fn, threading.Event()

    def put(self, item) -> bool:
        while not self.stop.is_set():
            try:
                self.q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def run(self) -> None:
        try:
            self.fn(self.put)
            self.put(self.END)
        except BaseException as e:      # noqa: BLE001 -- handed to the consumer, which raises it
            self.put(e)

    def __iter__(self):
        while True:
            item = self.q.get()
            if item is self.END:
                return
            if isinstance(item, BaseException):
                raise item
            yield item

    def close(self) -> None:
        self.stop.set()
        while self.is_alive():
            try:
                self.q.get_nowait()
            except queue.Empty:
                pass
            self.join(timeout=0.05)
