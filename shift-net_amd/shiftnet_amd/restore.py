"""Restore a whole video: N frames in, N restored frames of the same size out, in the same pixel format unless another is asked for (single GPU).

Not part of the upstream API.  The programs under ``inference/test_*.py`` are upstream's evaluation harnesses (ground truth, dropped border
frames, crops); this is the path for footage.  Frames are planar Y'CbCr payloads as a Y4M stream carries them (shiftnet_amd/y4m.py); the
colour conversion, the padding to a legal size and the crop run on the device (csrc/sn_yuv.hip), so 1.5 bytes per pixel cross PCIe for
8-bit 4:2:0 and no float frame touches the host.

Windows: window k restores frames [k L, min((k + 1) L, N)) and feeds the network those plus 2 frames before and 2 after; frames before
0 and after N - 1 are reflected without repeating the edge (-1 -> 1, -2 -> 2, N -> N - 2), or clamped where N <= 2.

Scenes (``scene_cuts``, off by default): every GSTS unit of the network borrows channels from the neighbouring frames, so across a cut the
last frames of one shot would be restored with features of the next.  With scene cuts c_1 < c_2 < ... the scenes [0, c_1), [c_1, c_2), ...
are clips of their own: windows restart at every scene start and reflect about the scene's first and last frame, and the bytes written are
those of restoring every scene as a separate video.  The cuts are listed by the caller or found from luma thumbnails made on the device
(``sn_yuv_thumb``, shiftnet_amd/scenes.py).

Noise level (``sigma``, denoise variants): a number, a list with one number per window, or ``"auto"``: a blind estimate per window from
histograms of the luma's 2 x 2 Haar HH coefficient, made on the device from the payloads the window has uploaded anyway
(``sn_yuv_noise_hist``, shiftnet_amd/noise.py).

Noise model (``noise_model``, denoise variants, off by default): sensor noise is signal dependent, the shadows of R'G'B' carry more of it than the
highlights.  ``"level"`` estimates per window a noise-level function -- sigma against the luma code, 16 knots -- from the same histograms split by
brightness (``sn_yuv_noise_hist_bands``) and writes the network's noise plane per pixel from it (``sn_noise_map_level``), in place of one level everywhere.

Active picture (``picture``, off by default): a letterboxed or pillarboxed stream is restored inside its picture rectangle only -- there the bytes
are those of restoring the cropped stream, and the bars leave as they came in.  The rectangle is given by the caller, for the stream or per window,
or found per window from the sums of the luma's rows and columns, made on the device from the payloads the window has uploaded anyway
(``sn_yuv_rowcol_sums``, shiftnet_amd/picture.py).

Output format (``out_format``, ``dither``; both off by default): the network's result is float32, and rounding it to the 8-bit codes it came from
puts back the steps that the noise just removed was hiding.  ``out_format`` writes another bit depth and chroma layout than was read (10 bit
from 8 bit footage keeps the precision); ``dither="tpdf"`` adds triangular noise of +-1 code before the rounding, which makes the mean of the codes
follow the value at the price of about 0.5 code rms of noise (``sn_egress_yuv_dither``, csrc/sn_yuv.hip).  The noise is a hash of the seed, the
sample's position and the number of the frame in its clip -- the stream, or the scene -- so the bytes do not depend on how the windows are run.
"""
from __future__ import annotations

import argparse
import queue
import sys
import threading
import time
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

PAST, FUTURE = 2, 2
VARIANTS = {"deblur": "gshift_deblur1", "deblur_small": "gshift_deblur2", "denoise": "gshift_denoise1", "denoise_small": "gshift_denoise2"}


# ---- the window planner (pure) ----------------------------------------------------------------------------------------------------
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
    from .scenes import check_cuts
    if n < 1 or one_len < 1:
        raise ValueError(f"plan_scene_windows: need n >= 1 and one_len >= 1, got {n}, {one_len}")
    starts = [0] + [c for c in check_cuts(cuts) if c < n]
    plan = []
    for a, b in zip(starts, starts[1:] + [n]):
        plan += [(a + lo, cnt, [a + i for i in idx]) for lo, cnt, idx in plan_windows(b - a, one_len, past, future)]
    return plan


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


# ---- frame source: look-ahead over an iterator whose length is unknown until it ends ----------------------------------------------
class _Frames:
    def __init__(self, it: Iterable[np.ndarray]) -> None:
        self.it = iter(it)
        self.base = 0                     # index of buf[0]
        self.buf: List[np.ndarray] = []
        self.n: Optional[int] = None      # known once the iterator ends
        self.clip_lo = 0                  # the first restored frame of the window handed out last, counted from the first frame of its clip

    def _fill(self, upto: int) -> None:
        while self.n is None and self.base + len(self.buf) <= upto:
            try:
                self.buf.append(next(self.it))
            except StopIteration:
                self.n = self.base + len(self.buf)

    def window(self, k: int, one_len: int) -> Optional[Tuple[int, int, List[np.ndarray]]]:
        """The frames of window k, or None past the end.  Reads ahead as far as the window reaches."""
        self._fill((k + 1) * one_len + FUTURE - 1)
        n = self.n if self.n is not None else self.base + len(self.buf)      # not at the end: every index of the window is < frames read
        if n == 0 and k == 0:
            return None
        if k * one_len >= n:
            return None
        lo, cnt, idx = window_indices(k, one_len, n)
        self.clip_lo = lo
        frames = [self.buf[i - self.base] for i in idx]
        drop = max(0, (k + 1) * one_len - PAST - self.base)                  # the next window reaches back to (k + 1) L - PAST
        if drop > 0:
            del self.buf[:drop]
            self.base += drop
        return lo, cnt, frames


class _SceneFrames:
    """_Frames for a stream with scene cuts: the windows of plan_scene_windows from an iterator of unknown length, with the cut decisions
    arriving late.  ``decider`` (scenes.ListedCuts, scenes.CutDetector behind _DeviceThumbs, or anything shaped like them) is fed every frame
    exactly once and in order, in chunks, and answers ``is_cut(t)`` for t < ``decided``; it needs ``lookahead`` frames beyond t to decide t.

    The window that restores [lo, lo + L) of a scene that started at a reads frames lo - 2 .. lo + L + 1 unless the scene ends before: it
    depends on the decisions for lo + 1 .. lo + L + 1, so it is handed out once frame lo + L + 1 + lookahead has been read or the stream has
    ended.  Frames before max(a, lo - 2) of the next window are dropped: at most L + 4 + lookahead + 1 are held."""

    def __init__(self, it: Iterable[np.ndarray], decider) -> None:
        self.it = iter(it)
        self.decider = decider
        self.base = 0
        self.buf: List[np.ndarray] = []
        self.n: Optional[int] = None
        self.fed = 0                      # frames handed to the decider
        self.finished = False             # the decider has been told that the stream has ended
        self.a = 0                        # first frame of the current scene
        self.lo = 0                       # next frame to restore
        self.k = 0
        self.cuts: List[int] = []         # the scene starts used
        self.clip_lo = 0                  # as _Frames.clip_lo: the clip is the scene

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

    def window(self, k: int, one_len: int) -> Optional[Tuple[int, int, List[np.ndarray]]]:
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
        self.lo = hi
        self.clip_lo = lo - a
        if cut is not None and hi == cut:
            self.a = cut
            self.cuts.append(cut)
        drop = max(self.a, self.lo - PAST) - self.base                        # the next window reaches back to here
        if drop > 0:
            del self.buf[:drop]
            self.base += drop
        return lo, hi - lo, frames


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


# ---- cut detection on the device ----------------------------------------------------------------------------------------------------
class _DeviceThumbs:
    """The decider of _SceneFrames for ``scene_cuts="auto"``: host payloads -> luma thumbnails on the device (sn_yuv_thumb) -> scenes.CutDetector.

    The detector has an upload of its own, luma bytes only: which frames a window holds depends on the decisions, so the thumbnails must exist
    before the window is assembled and uploaded, and the window's upload repeats reflected frames while the detector takes every frame once.
    One chunk = the new frames of one window: their luma planes go through a pinned buffer into payload-shaped device slots (the chroma part
    of a slot is never written and never read), one launch makes the thumbnails, one copy brings the uint16 sums back into pinned memory, and the
    calling thread waits for the event recorded behind that copy on the detector's own stream -- never for the device, and never for the stream
    the forward runs on."""

    def __init__(self, torch, dev, fmt, h: int, w: int, chunk: int, threshold: float, ratio: float) -> None:
        from .scenes import CutDetector
        self.torch, self.dev, self.fmt, self.h, self.w, self.chunk = torch, dev, fmt, h, w, chunk
        self.lb = h * w * (1 if fmt.bits == 8 else 2)                    # the luma plane leads the payload
        hb, wb = (h + 7) // 8, (w + 7) // 8
        self.pin_y = torch.empty((chunk, self.lb), dtype=torch.uint8).pin_memory()
        self.dev_y = torch.empty((chunk, fmt.frame_bytes(h, w)), dtype=torch.uint8, device=dev)
        self.dev_s = torch.empty((chunk, hb, wb), dtype=torch.uint16, device=dev)
        self.pin_s = torch.empty((chunk, hb, wb), dtype=torch.uint16).pin_memory()
        self.stream, self.event = torch.cuda.Stream(dev), torch.cuda.Event()
        self.detector = CutDetector(h, w, fmt.bits, threshold, ratio)
        self.lookahead = self.detector.lookahead
        self.frames = self.launches = 0

    def feed(self, frames: Sequence[np.ndarray]) -> None:
        from .io_edges import thumb_yuv
        torch = self.torch
        for o in range(0, len(frames), self.chunk):
            part = frames[o:o + self.chunk]
            t = len(part)
            pin = self.pin_y.numpy()
            for i, f in enumerate(part):
                pin[i] = f[:self.lb]
            with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
                for i in range(t):
                    self.dev_y[i, :self.lb].copy_(self.pin_y[i], non_blocking=True)
                thumb_yuv(self.dev_y[:t], self.fmt, self.h, self.w, out=self.dev_s[:t])
                self.pin_s[:t].copy_(self.dev_s[:t], non_blocking=True)
                self.event.record(self.stream)
            self.event.synchronize()
            self.detector.feed(self.pin_s[:t].numpy())
            self.frames += t
            self.launches += 1

    def finish(self) -> None:
        self.detector.finish()

    @property
    def decided(self) -> int:
        return self.detector.decided

    def is_cut(self, t: int) -> bool:
        return self.detector.is_cut(t)


# ---- the restorer -----------------------------------------------------------------------------------------------------------------
class VideoRestorer:
    """``VideoRestorer(net, one_len, sigma=None).restore(frames, fmt, height, width)`` -> iterator of restored payloads, one per input frame.

    net: a GShiftNet of shiftnet_amd.arch on a HIP device (eval mode, any dtype).  sigma: the noise level in 8-bit code values for the
    denoise variants (noise_map = sigma / 255 everywhere; no noise is added and the frame is not cut into quadrants): a number; a sequence of
    numbers, one per window in the order the windows are restored (running out is a ValueError that names the window); or ``"auto"`` -- per window
    the median over its input frames of a blind estimate from the luma plane (noise.py; a heuristic that assumes white Gaussian noise), clamped to
    ``sigma_clamp``.  The deblur variants ignore a number and refuse the other two.  Once ``restore()`` has been exhausted
    ``stats["window_sigma"]`` lists the sigma of every window (denoise variants), ``stats["window_frame_sigma"]`` the estimates of every window's
    input frames (auto only; None where no block of a frame counted) and ``stats["noise_launches"]`` the ``sn_yuv_noise_hist`` launches.
    pipeline: read / copy / ingest window k + 1 on a side stream and copy back / hand out window k - 1 while window k runs; False runs
    the same steps one after the other.  Both give identical bytes.
    scene_cuts: None -- the stream is one clip; ``"auto"`` -- find the cuts from luma thumbnails made on the device (scenes.py: frame t starts a
    scene iff its measure m[t] >= cut_threshold and >= cut_ratio times the median of its six neighbours'; heuristic defaults); an iterable of
    frame indices (each >= 1, strictly increasing) -- use these, run no detector.  Every scene is then restored as a clip of its own: the bytes
    are those of restoring each scene as a separate video.  Once ``restore()`` has been exhausted ``stats["cuts"]`` lists the scene starts used,
    ``stats["cut_measure"]`` the m[t] of every frame (auto only; m[0] = 0.0) and ``stats["cuts_ignored"]`` the listed cuts at or beyond the end.
    noise_model: None -- ``noise_map = sigma / 255`` at every pixel, today's code path and bytes; ``"level"`` (needs ``sigma="auto"``) -- per window a
    noise-level function is estimated from band histograms of the payloads the window has uploaded anyway (``sn_yuv_noise_hist_bands``; noise.window_curve
    on the host: sigma of 8-bit R'G'B' at 16 luma levels, holes filled, clamped to ``sigma_clamp``) and ``sn_noise_map_level`` writes the window's noise
    plane from it: the curve at the low-passed luma of every pixel, which replaces the broadcast number.  The flat estimate still runs and is still
    reported.  A list of curves (16 numbers each), one per window in the order the windows are restored, is used as given: no estimate of the curve
    runs, and running out is a ValueError that names the window.  Any ``noise_model`` with a deblur variant is a ValueError.  **A heuristic, checked on
    synthetic clips only**: the networks were trained with uniform maps and nobody has judged their output for a varying one; the curve is a function
    of the luma alone; texture adds to a band's estimate as it does to the flat one.  With ``picture`` both kernels see the rectangle as the whole
    frame.  ``stats["window_nlf"]`` lists the 16 knots of every window, ``stats["nlf_launches"]`` counts the ``sn_yuv_noise_hist_bands`` launches and
    ``stats["nlf_map_launches"]`` the ``sn_noise_map_level`` launches.
    picture: None -- the whole frame, today's code path and bytes; ``(x0, y0, w, h)`` in luma samples -- restore that rectangle of every frame; a
    list with one rectangle (or None) per window in the order the windows are restored (running out is a ValueError that names the window).  The
    two are told apart by their elements: four numbers are one rectangle, anything whose elements are sequences or None is a list, of four windows
    too.  Every entry is judged against the stream's size and format when restore() starts (a ValueError before the first window); how many
    windows a stream has is known only at its end, so a list that is too short is found when the stager reaches the window without an entry;
    ``"auto"`` -- per window the rectangle left by the black bars of its input frames as fed (picture.py: rows and columns whose mean luma stays
    within ``bar_level`` 8-bit codes of black in every frame of the window; a heuristic; None where it finds no bars, or nothing but bars).  At
    4:2:0 x0 and y0 are even, and w and h unless the rectangle reaches the frame's far edge; a rectangle is at least as large as the smallest
    frame the network takes, 5 x 5 ("small" topology) or 9 x 9 ("plus") (picture.check_rect, picture.smallest_picture).  Inside the rectangle, luma and
    chroma, the output equals that of this restorer with the same other arguments on the cropped stream -- the network, the chroma filters of both
    edges and the ``sigma="auto"`` estimate see the rectangle as the whole frame -- and every sample outside equals the input's.
    ``scene_cuts="auto"`` keeps looking at the whole frame: the bars add nothing to the difference measure but dilute its mean, so the cuts found
    may differ from those of the cropped stream.  A window whose rectangle differs from the previous window's has a new input signature for the
    engine: a new plan, and a new captured graph where graphs are on.  Once ``restore()`` has been exhausted ``stats["window_picture"]`` lists the
    rectangle of every window (None: the full frame), ``stats["picture_launches"]`` counts the ``sn_yuv_rowcol_sums`` launches and
    ``stats["picture_wait_ms"]`` (auto only) lists how long the stager waited for every window's sums (upload, kernel and copy back included).
    out_format: None -- the payloads yielded have the format of those read, today's code path and bytes; a C tag of y4m.MODES -- they have that bit
    depth and chroma layout (``plan_output(fmt, tag)[0].frame_bytes(h, w)`` bytes each), matrix and range stay the input's.  A tag that says what the
    input's says is None.  With ``picture`` a rectangle must then be legal in both formats (the even-alignment rule applies if either is 4:2:0, to
    ``"auto"`` as well), and the samples outside it cannot be copied: they are the whole input frame converted, ``egress(out format,
    ingest_float32(in format, frame))``, undithered -- a bar at 8-bit code 16 leaves at 10-bit code 64.
    dither: None -- codes are rounded to nearest, today's bytes; ``"tpdf"`` -- triangular noise of +-1 code is added before the rounding
    (``sn_egress_yuv_dither``): the mean of the codes of a flat area follows its value instead of sitting on a step, at the price of noise of about
    0.5 code rms.  ``dither_seed`` (0 .. 2^32 - 1) picks the noise.  The noise of a sample is a hash of the seed, its plane, row and column -- counted
    from the picture's origin under ``picture`` -- and the number of its frame counted from the first frame of its clip: the stream, or the scene under
    ``scene_cuts``.  So the bytes are the same with ``pipeline`` on and off, those of restoring every scene as a separate video, and inside a picture
    those of restoring the cropped stream.  ``stats["out_format"]`` and ``stats["dither"]`` record the two arguments as used (None: the input's
    format / no dither), ``stats["dither_seed"]`` the seed."""

    def __init__(self, net, one_len: int, sigma=None, pipeline: bool = True, scene_cuts=None,
                 cut_threshold: float = 4.0, cut_ratio: float = 2.5, sigma_clamp: Sequence[float] = (0.0, 50.0),
                 picture=None, bar_level: float = 1.0, out_format=None, dither=None, dither_seed: int = 0, noise_model=None) -> None:
        import torch
        from .lib import YuvFmt
        self.torch = torch
        _, self.dither, self.dither_seed = plan_output(YuvFmt(8, 0, 0, 0), out_format, dither, dither_seed)      # the argument errors, before anything else
        self.out_format = out_format
        self.net, self.one_len, self.pipeline = net, int(one_len), bool(pipeline)
        if self.one_len < 1:
            raise ValueError("one_len must be >= 1")
        if scene_cuts is None or (isinstance(scene_cuts, str) and scene_cuts == "auto"):
            self.scene_cuts = scene_cuts
        elif isinstance(scene_cuts, str):
            raise ValueError(f"scene_cuts must be None, 'auto' or an iterable of frame indices, got {scene_cuts!r}")
        else:
            from .scenes import check_cuts
            self.scene_cuts = check_cuts(scene_cuts)
        self.cut_threshold, self.cut_ratio = float(cut_threshold), float(cut_ratio)
        self.V = net.V
        if self.V.denoise and sigma is None:
            raise ValueError("sigma is required by the denoise variants (the noise level of the footage, in 8-bit code values)")
        from .noise import check_clamp, check_sigmas
        self.sigma_clamp = check_clamp(sigma_clamp)
        # sigma_mode: "fixed" (a number: the code path without any of the rest), "auto", "list"
        self.sigma, self.sigma_list, self.sigma_mode = None, None, "fixed"
        if isinstance(sigma, str):
            if sigma != "auto":
                raise ValueError(f"sigma must be a number, 'auto' or a sequence of numbers, got {sigma!r}")
            self.sigma_mode = "auto"
        elif sigma is not None and hasattr(sigma, "__iter__"):
            self.sigma_list, self.sigma_mode = check_sigmas(sigma), "list"
        elif sigma is not None:
            self.sigma = float(sigma)
        if self.sigma_mode != "fixed" and not self.V.denoise:
            raise ValueError(f"sigma={'auto' if self.sigma_mode == 'auto' else 'a per-window list'!r} is for the denoise variants; {type(net).__name__} "
                             "of a deblur variant takes no noise level")
        # nlf_mode: None (the code path without any of the rest), "level", "list"
        self.nlf_mode, self.nlf_list = None, None
        if noise_model is not None:
            if not self.V.denoise:
                raise ValueError(f"noise_model is for the denoise variants; {type(net).__name__} of a deblur variant takes no noise level")
            if isinstance(noise_model, str):
                if noise_model != "level":
                    raise ValueError(f"noise_model must be None, 'level' or a list of curves, got {noise_model!r}")
                if self.sigma_mode != "auto":
                    raise ValueError("noise_model='level' estimates the curve beside the flat estimate: it needs sigma='auto'")
                self.nlf_mode = "level"
            elif hasattr(noise_model, "__iter__"):
                from .noise import check_curves
                self.nlf_list, self.nlf_mode = check_curves(noise_model), "list"
            else:
                raise ValueError(f"noise_model must be None, 'level' or a list of curves, got {noise_model!r}")
        # picture_mode: "full" (None: the code path without any of the rest), "auto", "fixed" (one rectangle), "list"
        self.picture, self.picture_mode, self.bar_level = None, "full", float(bar_level)
        if isinstance(picture, str):
            if picture != "auto":
                raise ValueError(f"picture must be None, 'auto', (x0, y0, w, h) or a list of rectangles, got {picture!r}")
            self.picture_mode = "auto"
        elif picture is not None:
            picture = list(picture)
            if len(picture) == 4 and not any(r is None or hasattr(r, "__iter__") for r in picture):
                self.picture, self.picture_mode = tuple(picture), "fixed"
            else:
                self.picture, self.picture_mode = picture, "list"
        if not (self.bar_level >= 0.0):                            # refuses NaN as well
            raise ValueError(f"bar_level must be >= 0, got {bar_level!r}")
        p = next(net.parameters())
        self.dev, self.dtype = p.device, p.dtype
        if self.dev.type != "cuda":
            raise ValueError("VideoRestorer needs the module on a HIP device")
        self.stats = {"frames": 0, "windows": 0, "forward_s": 0.0, "window_forward_ms": []}
        self._shape = None
        self._wsig, self._wfsig, self._noise_launches = [], [], 0
        self._wpic, self._picture_launches, self._staged, self._picture_wait = [], 0, 0, []
        self._wnlf, self._nlf_launches, self._nlf_map_launches = [], 0, 0

    # -- per-shape state: two slots of staging and device buffers, sized for the largest window -------------------------------------
    def _prepare(self, fmt, h: int, w: int) -> None:
        torch = self.torch
        key = (fmt.bits, fmt.chroma, fmt.matrix, fmt.range, h, w)
        ofmt = plan_output(fmt, self.out_format)[0]               # fmt itself unless another bit depth or chroma layout is written
        if self.picture_mode in ("fixed", "list"):                # the rectangles are judged against this stream, as read and as written
            from .picture import check_pictures, smallest_picture
            self._pics = check_pictures([self.picture] if self.picture_mode == "fixed" else self.picture, fmt, h, w, smallest_picture(self.V.topo),
                                        out_fmt=ofmt)
        if self._shape == key:
            return
        self._shape = key
        self.fmt, self.h, self.w = fmt, h, w
        self.ofmt, self.convert = ofmt, ofmt is not fmt
        self.hp, self.wp = padded_size(h, w, self.V.topo)
        self.fb, self.ofb = fmt.frame_bytes(h, w), ofmt.frame_bytes(h, w)
        tin, tout = self.one_len + PAST + FUTURE, self.one_len
        dev = self.dev
        self.pin_in = [torch.empty((tin, self.fb), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.pin_out = [torch.empty((tout, self.ofb), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev_in = [torch.empty((tin, self.fb), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.dev_out = [torch.empty((tout, self.ofb), dtype=torch.uint8, device=dev) for _ in range(2)]
        # a picture in another format than was read: the window's whole frames as float32 on their way from one format to the other (main stream only)
        self.conv32 = torch.empty(tout * 3 * h * w, dtype=torch.float32, device=dev) if self.convert and self.picture_mode != "full" else None
        self.t0 = [0, 0]                                          # the frame number, in its clip, of the first frame the window of a slot restores
        # flat, sized for the full frame: a window's tensors are views of the leading elements at the padded size of its picture
        self.x = [torch.empty(tin * 3 * self.hp * self.wp, dtype=self.dtype, device=dev) for _ in range(2)]
        half = self.dtype != torch.float32
        self.x32 = [torch.empty(tin * 3 * self.hp * self.wp, dtype=torch.float32, device=dev) if half else None for _ in range(2)]
        self.rect = [None, None]                                  # the picture of the window a slot holds (None: the full frame)
        self.s_in, self.s_out = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        ev = lambda: [torch.cuda.Event() for _ in range(2)]      # noqa: E731
        self.ev_h2d, self.ev_ready, self.ev_done, self.ev_d2h = ev(), ev(), ev(), ev()
        self.used = [False, False]
        if self.sigma_mode == "auto":                             # per slot: the window's histograms on the device and in pinned memory
            from .noise import clip_codes, nbins
            self.nb = nbins(fmt.bits)
            self.noise_lo, self.noise_hi = clip_codes(fmt.bits, fmt.range)
            self.dev_hist = [torch.empty((tin, self.nb), dtype=torch.uint32, device=dev) for _ in range(2)]
            self.pin_hist = [torch.empty((tin, self.nb), dtype=torch.uint32).pin_memory() for _ in range(2)]
            self.ev_noise = ev()
        if self.nlf_mode is not None:
            from .noise import clip_codes
            self.noise_lo, self.noise_hi = clip_codes(fmt.bits, fmt.range)
        if self.nlf_mode == "level":                              # per slot: the window's band histograms on the device and in pinned memory
            from .noise import NLF_BANDS, nlf_bins
            nbv = nlf_bins(fmt.bits)
            self.dev_bands = [torch.empty((tin, NLF_BANDS, nbv), dtype=torch.uint32, device=dev) for _ in range(2)]
            self.pin_bands = [torch.empty((tin, NLF_BANDS, nbv), dtype=torch.uint32).pin_memory() for _ in range(2)]
            self.ev_bands = ev()
        if self.picture_mode == "auto":                           # per slot: the window's row and column sums on the device and in pinned memory
            self.dev_rows = [torch.empty((tin, h), dtype=torch.uint32, device=dev) for _ in range(2)]
            self.dev_cols = [torch.empty((tin, w), dtype=torch.uint32, device=dev) for _ in range(2)]
            self.pin_rows = [torch.empty((tin, h), dtype=torch.uint32).pin_memory() for _ in range(2)]
            self.pin_cols = [torch.empty((tin, w), dtype=torch.uint32).pin_memory() for _ in range(2)]
            self.ev_sums = ev()

    def _size(self, rect) -> Tuple[int, int, int, int]:
        """(h, w, padded h, padded w) of what a window with picture ``rect`` feeds the network."""
        h, w = (self.h, self.w) if rect is None else (rect[3], rect[2])
        return (h, w) + padded_size(h, w, self.V.topo)

    def _views(self, slot: int, t: int, rect):
        """The window's input tensors [1, t, 3, hp, wp]: views of the slot's flat buffers."""
        _, _, hp, wp = self._size(rect)
        n = t * 3 * hp * wp
        x32 = self.x32[slot]
        return self.x[slot][:n].view(1, t, 3, hp, wp), (x32[:n].view(1, t, 3, hp, wp) if x32 is not None else None)

    def _listed_picture(self, k: int):
        if self.picture_mode == "fixed":
            return self._pics[0]
        if k >= len(self._pics):
            raise ValueError(f"picture lists {len(self._pics)} window{'' if len(self._pics) == 1 else 's'}, window {k} has no entry")
        return self._pics[k]

    # -- the steps of one window; slot = k % 2 -------------------------------------------------------------------------------------
    def _stage(self, slot: int, frames: Sequence[np.ndarray], t0: int = 0) -> int:
        """Host frames -> pinned slot -> device -> RGB tensors, on the side stream.  Windows are staged in the order they are restored.
        t0: the number of the window's first restored frame in its clip (the dither's frame number)."""
        from .io_edges import ingest_yuv, noise_hist_bands_yuv, noise_hist_yuv, rowcol_sums_yuv
        torch = self.torch
        t = len(frames)
        rect = None
        if self.picture_mode in ("fixed", "list"):
            rect = self._listed_picture(self._staged)
        self._staged += 1
        self.t0[slot] = t0
        if self.used[slot]:
            self.ev_h2d[slot].synchronize()                      # the copy that last read this pinned slot has finished
        pin = self.pin_in[slot].numpy()
        for i, f in enumerate(frames):
            pin[i] = f
        with torch.cuda.stream(self.s_in):
            if self.used[slot]:
                self.s_in.wait_event(self.ev_done[slot])         # the forward that last read this slot's tensors has finished
            self.dev_in[slot][:t].copy_(self.pin_in[slot][:t], non_blocking=True)
            self.ev_h2d[slot].record(self.s_in)
            if self.picture_mode == "auto":
                # the sums of the payloads just uploaded; this thread waits for the event behind their copy to the host -- the side stream's own
                # work, never the device and never the stream the forward runs on -- because the rectangle shapes everything staged from here on
                from .picture import decide_picture, smallest_picture
                rowcol_sums_yuv(self.dev_in[slot][:t], self.fmt, self.h, self.w, out_rows=self.dev_rows[slot][:t], out_cols=self.dev_cols[slot][:t])
                self.pin_rows[slot][:t].copy_(self.dev_rows[slot][:t], non_blocking=True)
                self.pin_cols[slot][:t].copy_(self.dev_cols[slot][:t], non_blocking=True)
                self.ev_sums[slot].record(self.s_in)
                self._picture_launches += 1
                t0 = time.perf_counter()
                self.ev_sums[slot].synchronize()
                self._picture_wait.append((time.perf_counter() - t0) * 1e3)
                rect = decide_picture(self.pin_rows[slot][:t].numpy(), self.pin_cols[slot][:t].numpy(), self.fmt, self.h, self.w, self.bar_level,
                                      smallest_picture(self.V.topo), out_fmt=self.ofmt)
            self.rect[slot] = rect
            x, x32 = self._views(slot, t, rect)
            hp, wp = x.shape[3], x.shape[4]
            if self.sigma_mode == "auto":
                # the histograms of the payloads just uploaded, ahead of the ingest so that they are on the host long before _run asks.  The
                # pinned slot is free: _run read it on the host before this slot was handed back to the stager
                noise_hist_yuv(self.dev_in[slot][:t], self.fmt, self.h, self.w, self.noise_lo, self.noise_hi, out=self.dev_hist[slot][:t], rect=rect)
                self.pin_hist[slot][:t].copy_(self.dev_hist[slot][:t], non_blocking=True)
                self.ev_noise[slot].record(self.s_in)
                self._noise_launches += 1
            if self.nlf_mode == "level":                         # the same statistic by brightness band, from the same payloads, behind it
                noise_hist_bands_yuv(self.dev_in[slot][:t], self.fmt, self.h, self.w, self.noise_lo, self.noise_hi, out=self.dev_bands[slot][:t], rect=rect)
                self.pin_bands[slot][:t].copy_(self.dev_bands[slot][:t], non_blocking=True)
                self.ev_bands[slot].record(self.s_in)
                self._nlf_launches += 1
            ingest_yuv(self.dev_in[slot][:t], self.fmt, self.h, self.w, hp, wp, self.dtype, out=x, rect=rect)
            if x32 is not None:
                ingest_yuv(self.dev_in[slot][:t], self.fmt, self.h, self.w, hp, wp, torch.float32, out=x32, rect=rect)
            self.ev_ready[slot].record(self.s_in)
        return t

    def _window_sigma(self, slot: int, t: int) -> float:
        """The noise level of the window about to run (denoise variants); windows run in the order they are handed out."""
        k = len(self._wsig)
        if self.sigma_mode == "auto":
            from .noise import frame_sigma, window_sigma
            self.ev_noise[slot].synchronize()                    # the copy of this slot's histograms, on the side stream: not the device, not main
            hist = self.pin_hist[slot][:t].numpy()
            per = [frame_sigma(hist[i], self.fmt.bits, self.fmt.matrix, self.fmt.range) for i in range(t)]
            self._wfsig.append(per)
            sigma = window_sigma(per, self.sigma_clamp)
        elif self.sigma_mode == "list":
            if k >= len(self.sigma_list):
                raise ValueError(f"sigma lists {len(self.sigma_list)} window{'' if len(self.sigma_list) == 1 else 's'}, window {k} has no entry")
            sigma = self.sigma_list[k]
        else:
            sigma = self.sigma
        self._wsig.append(sigma)
        return sigma

    def _window_curve(self, slot: int, t: int) -> List[float]:
        """The noise-level function of the window about to run (noise_model): 16 knots, sigma of 8-bit R'G'B'."""
        k = len(self._wnlf)
        if self.nlf_mode == "level":
            from .noise import window_curve
            self.ev_bands[slot].synchronize()                    # the copy of this slot's band histograms, on the side stream: not the device, not main
            curve = window_curve(self.pin_bands[slot][:t].numpy(), self.fmt.bits, self.fmt.matrix, self.fmt.range, self.sigma_clamp)
        else:
            if k >= len(self.nlf_list):
                raise ValueError(f"noise_model lists {len(self.nlf_list)} window{'' if len(self.nlf_list) == 1 else 's'}, window {k} has no entry")
            curve = list(self.nlf_list[k])
        self._wnlf.append(curve)
        return curve

    def _run(self, slot: int, t: int, main) -> int:
        """Forward + egress on the main stream, copy back on the output stream."""
        from .io_edges import egress_yuv, ingest_yuv, noise_map_level
        torch = self.torch
        n = t - PAST - FUTURE
        sigma = self._window_sigma(slot, t) if self.V.denoise else None
        curve = self._window_curve(slot, t) if self.nlf_mode is not None else None
        rect = self.rect[slot]
        self._wpic.append(rect)
        with torch.cuda.stream(main), torch.no_grad():
            main.wait_event(self.ev_ready[slot])
            if self.used[slot]:
                main.wait_event(self.ev_d2h[slot])               # the copy that last read this slot's device payloads has finished
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(main)
            x, x32 = self._views(slot, t, rect)
            kw = {}
            if x32 is not None:
                kw["shortcut"] = x32
            if curve is not None:
                # the plane from the payloads the ingest read (ev_ready lies behind their upload; they stay until ev_done); the knots are a kernel argument
                nm = noise_map_level(self.dev_in[slot][:t], self.fmt, self.h, self.w, x.shape[3], x.shape[4], [c / 255.0 for c in curve], self.dtype,
                                     self.noise_lo, self.noise_hi, rect=rect)
                self._nlf_map_launches += 1
                out = self.net.forward_fp32_out(x, nm, **kw)
            elif self.V.denoise:
                nm = torch.full((1, 1, 1, 1, 1), sigma / 255.0, dtype=self.dtype, device=self.dev).expand(1, t, 1, x.shape[3], x.shape[4])
                out = self.net.forward_fp32_out(x, nm, **kw)
            else:
                out = self.net.forward_fp32_out(x, **kw)
            e1.record(main)
            self._timers.append((e0, e1))
            if rect is not None and not self.convert:
                # everything outside the picture leaves as it came in: the window's own n frames (not the reflected ones around them) first
                self.dev_out[slot][:n].copy_(self.dev_in[slot][PAST:PAST + n], non_blocking=True)
            elif rect is not None:
                # ... in the format written: the whole frames converted by the two edges, float32 between them, rounded to nearest
                full = self.conv32[:n * 3 * self.h * self.w].view(1, n, 3, self.h, self.w)
                ingest_yuv(self.dev_in[slot][PAST:PAST + n], self.fmt, self.h, self.w, self.h, self.w, torch.float32, out=full)
                egress_yuv(full[0], self.ofmt, self.h, self.w, dst=self.dev_out[slot][:n])
            dither = None if self.dither is None else (self.dither_seed, self.t0[slot])
            egress_yuv(out, self.ofmt, self.h, self.w, dst=self.dev_out[slot][:n], rect=rect, dither=dither)
            self.ev_done[slot].record(main)
        with torch.cuda.stream(self.s_out):
            self.s_out.wait_event(self.ev_done[slot])
            self.pin_out[slot][:n].copy_(self.dev_out[slot][:n], non_blocking=True)
            self.ev_d2h[slot].record(self.s_out)
        self.used[slot] = True
        return n

    def _collect(self, slot: int, n: int) -> List[np.ndarray]:
        self.ev_d2h[slot].synchronize()
        return list(self.pin_out[slot][:n].numpy().copy())

    def _finish_stats(self) -> None:
        ms = [a.elapsed_time(b) for a, b in self._timers]        # every event has completed: the last copy back has been waited for
        self.stats["window_forward_ms"] = ms
        self.stats["forward_s"] = sum(ms) / 1e3
        self.stats["windows"] = len(ms)
        self.stats["noise_launches"] = self._noise_launches
        if self.nlf_mode is not None:
            self.stats["window_nlf"] = [list(c) for c in self._wnlf]
            self.stats["nlf_launches"], self.stats["nlf_map_launches"] = self._nlf_launches, self._nlf_map_launches
        self.stats["window_picture"] = list(self._wpic)
        self.stats["picture_launches"] = self._picture_launches
        if self.picture_mode == "auto":
            self.stats["picture_wait_ms"] = list(self._picture_wait)
        if self.V.denoise:
            self.stats["window_sigma"] = list(self._wsig)
            if self.sigma_mode == "auto":
                self.stats["window_frame_sigma"] = [list(p) for p in self._wfsig]
        src = self._src
        if isinstance(src, _SceneFrames):                        # its thread has ended: the stream has been read to its end
            self.stats["cuts"] = list(src.cuts)
            if isinstance(src.decider, _DeviceThumbs):
                self.stats["cut_measure"] = list(src.decider.detector.m)
                self.stats["thumb_frames"], self.stats["thumb_launches"] = src.decider.frames, src.decider.launches
            else:
                self.stats["cuts_ignored"] = [c for c in src.decider.all if c >= (src.n or 0)]

    def _source(self, frames: Iterable[np.ndarray]):
        """The frame source of one restore(): today's for scene_cuts=None, the scene-aware one otherwise."""
        if self.scene_cuts is None:
            self._src = _Frames(frames)
        elif self.scene_cuts == "auto":
            self._src = _SceneFrames(frames, _DeviceThumbs(self.torch, self.dev, self.fmt, self.h, self.w, self.one_len + PAST + FUTURE + 4,
                                                           self.cut_threshold, self.cut_ratio))
        else:
            from .scenes import ListedCuts
            self._src = _SceneFrames(frames, ListedCuts(self.scene_cuts))
        return self._src

    # -- drivers -------------------------------------------------------------------------------------------------------------------
    def restore(self, frames: Iterable[np.ndarray], fmt, height: int, width: int) -> Iterator[np.ndarray]:
        """frames: iterable of uint8 payloads (``fmt.frame_bytes(height, width)`` each) -> the restored payloads, in order."""
        torch = self.torch
        self._prepare(fmt, height, width)
        self._timers: List = []
        self.used = [False, False]
        self.stats = {"frames": 0, "windows": 0, "forward_s": 0.0, "window_forward_ms": []}
        self.stats["out_format"], self.stats["dither"], self.stats["dither_seed"] = (self.out_format if self.convert else None), self.dither, self.dither_seed
        self._src = None
        self._wsig, self._wfsig, self._noise_launches = [], [], 0
        self._wpic, self._picture_launches, self._staged, self._picture_wait = [], 0, 0, []
        self._wnlf, self._nlf_launches, self._nlf_map_launches = [], 0, 0
        main = torch.cuda.current_stream(self.dev)

        def checked(it):
            for f in it:
                f = np.asarray(f, dtype=np.uint8).reshape(-1)
                if f.size != self.fb:
                    raise ValueError(f"frame payload of {f.size} bytes, the format and size say {self.fb}")
                yield f

        if not self.pipeline:
            src = self._source(checked(frames))
            k = 0
            with torch.cuda.device(self.dev):
                while True:
                    win = src.window(k, self.one_len)
                    if win is None:
                        break
                    t = self._stage(k % 2, win[2], src.clip_lo)
                    n = self._run(k % 2, t, main)
                    for p in self._collect(k % 2, n):
                        self.stats["frames"] += 1
                        yield p
                    k += 1
                self._finish_stats()
            return

        # Three threads besides the kernels: the stager reads frames and brings window k + 1 onto the device (side stream), the forward
        # thread runs window k (its range-guard check waits for the device, so nothing else may depend on this thread), and the caller's
        # thread takes window k - 1 out of the pinned buffer.  Streams order the device work with events; the semaphores only say that
        # the event a stream is about to wait for HAS been recorded (in slots) and that a pinned output slot has been emptied (out slots).
        in_free = [threading.Semaphore(1), threading.Semaphore(1)]
        out_free = [threading.Semaphore(1), threading.Semaphore(1)]
        halt = threading.Event()

        def acquire(sem) -> bool:
            while not halt.is_set():
                if sem.acquire(timeout=0.1):
                    return True
            return False

        def stage_loop(put):
            src = self._source(checked(frames))
            k = 0
            with torch.cuda.device(self.dev):
                while True:
                    win = src.window(k, self.one_len)
                    if win is None or not acquire(in_free[k % 2]):
                        return
                    if not put((k % 2, self._stage(k % 2, win[2], src.clip_lo))):
                        return
                    k += 1

        stager = _Thread(stage_loop, depth=1)

        def forward_loop(put):
            with torch.cuda.device(self.dev):
                for slot, t in stager:
                    if not acquire(out_free[slot]):
                        return
                    n = self._run(slot, t, main)
                    in_free[slot].release()
                    if not put((slot, n)):
                        return

        worker = _Thread(forward_loop, depth=1)
        stager.start()
        worker.start()
        try:
            for slot, n in worker:
                payloads = self._collect(slot, n)
                out_free[slot].release()
                for p in payloads:
                    self.stats["frames"] += 1
                    yield p
            self._finish_stats()
        finally:
            halt.set()
            worker.close()
            stager.close()


# ---- command line -------------------------------------------------------------------------------------------------------------------
def sigma_arg(word: str):
    """--sigma: a number stays the float it always was; 'auto'; anything else names a file with one sigma per window."""
    try:
        return float(word)
    except ValueError:
        return word


def picture_arg(word: str):
    """--picture: 'full' -> None; 'auto'; X:Y:W:H -> the rectangle; anything else names a file with one rectangle per window."""
    if word == "full":
        return None
    parts = word.split(":")
    if len(parts) == 4 and all(p.isdigit() for p in parts):
        return tuple(int(p) for p in parts)
    return word


def _modes():
    from .y4m import MODES
    return MODES


def make_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Restore a Y4M video with Shift-Net on the MI355X: same frames and size out, same pixel format unless "
                                             "--out_format names another")
    ap.add_argument("--variant", choices=list(VARIANTS), required=True)
    ap.add_argument("--checkpoint", required=True, help="checkpoint path, or 'synthetic' for the deterministic synthetic weights")
    ap.add_argument("--dtype", choices=["fp32", "fp16", "bf16"], default="bf16")
    ap.add_argument("--one_len", type=int, default=16, help="frames restored per window")
    ap.add_argument("--sigma", type=sigma_arg, default=None, metavar="{NUMBER,auto,FILE}",
                    help="noise level (8-bit code values), required by the denoise variants: a number; 'auto' estimates it per window on the device "
                         "(a heuristic that assumes white Gaussian noise); FILE lists one sigma per window, one per line ('#' comments)")
    ap.add_argument("--sigma_clamp", type=float, nargs=2, default=(0.0, 50.0), metavar=("LO", "HI"), help="auto: the estimate is clamped to this range")
    ap.add_argument("--sigma_out", default=None, metavar="FILE", help="write the sigma that every window was restored with, in the format --sigma FILE reads")
    ap.add_argument("--noise_model", default="flat", metavar="{flat,level,FILE}",
                    help="denoise variants: 'level' (needs --sigma auto) estimates per window the noise level as a function of brightness on the device and "
                         "gives the network a noise plane that follows it (a heuristic, checked on synthetic clips only); FILE lists one curve per window, "
                         "16 sigmas per line from black to white ('#' comments); default flat: one level per window")
    ap.add_argument("--noise_model_out", default=None, metavar="FILE",
                    help="write the curve every window was restored with, in the format --noise_model FILE reads")
    ap.add_argument("--matrix", choices=["bt601", "bt709"], default=None, help="default: bt709 when H >= 720, else bt601")
    ap.add_argument("--range", choices=["limited", "full"], default=None, help="default: the stream's XCOLORRANGE, else limited")
    ap.add_argument("--no_pipeline", action="store_true", help="run read / copy / forward / write one after the other")
    ap.add_argument("--scene_cuts", default="off", metavar="{off,auto,FILE}",
                    help="restore every scene as a clip of its own: 'auto' finds the cuts on the device (a heuristic, see --cut_threshold / --cut_ratio), "
                         "FILE lists the first frame of every scene but the first, one index per line ('#' comments); default off: the stream is one clip")
    ap.add_argument("--cut_threshold", type=float, default=4.0, help="auto: smallest mean absolute difference of 8x8 block means (8-bit code units) of a cut")
    ap.add_argument("--cut_ratio", type=float, default=2.5, help="auto: ... and at least this many times the median of the six neighbouring frames' differences")
    ap.add_argument("--picture", default="full", metavar="{full,auto,X:Y:W:H,FILE}",
                    help="restore the active picture of a letterboxed / pillarboxed stream only and leave the bars as they are: X:Y:W:H in luma samples; "
                         "'auto' finds the bars per window on the device (a heuristic, see --bar_level); FILE lists 'x0 y0 w h' (or 'full') per window, one "
                         "per line ('#' comments); default full: the whole frame")
    ap.add_argument("--bar_level", type=float, default=1.0, help="auto: a row or column is bar if its mean luma stays within this many 8-bit codes of black")
    ap.add_argument("--picture_out", default=None, metavar="FILE", help="write the picture every window was restored with, in the format --picture FILE reads")
    ap.add_argument("--out_format", choices=list(_modes()), default=None, metavar="TAG",
                    help="write this Y4M C tag instead of the input's (%(choices)s): another bit depth and chroma layout, e.g. 444p10 or 420p10 to keep the "
                         "precision of the result when 8 bit came in; matrix and range stay the input's; default: the input's format")
    ap.add_argument("--dither", choices=["none", "tpdf"], default="none",
                    help="tpdf: add triangular noise of +-1 code before rounding to the output's codes: no banding, about 0.5 code rms of noise instead; "
                         "default none: round to nearest")
    ap.add_argument("--dither_seed", type=int, default=0, metavar="N", help="tpdf: which noise (0 .. 2^32 - 1); the same seed gives the same bytes")
    ap.add_argument("--cuts_out", default=None, metavar="FILE", help="write the scene starts that were used, in the format --scene_cuts FILE reads")
    ap.add_argument("input", metavar="IN", help="Y4M file, or - for stdin")
    ap.add_argument("output", metavar="OUT", help="Y4M file, or - for stdout")
    return ap


def load_net(variant: str, checkpoint: str, dtype: str, device="cuda"):
    import torch
    from .arch import CLASSES
    from .weights import synth_state_dict
    name = VARIANTS[variant]
    net = CLASSES[name](future_frames=FUTURE, past_frames=PAST)
    if checkpoint == "synthetic":
        net.load_state_dict(synth_state_dict(name), strict=True)
    else:
        net.load_state_dict(torch.load(checkpoint, map_location="cpu")["params"])
    dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    return net.to(dt).to(device).eval()


def main(argv: Optional[Sequence[str]] = None) -> int:
    from . import lib as L
    from .io_edges import yuv_fmt
    from .y4m import Y4MReader, Y4MWriter, output_header
    ap = make_parser()
    a = ap.parse_args(argv)
    if not (0 <= a.dither_seed < 2 ** 32):
        ap.error("--dither_seed: an integer in 0 .. 2^32 - 1")
    if "denoise" in a.variant and a.sigma is None:
        ap.error("--sigma is required by the denoise variants")
    log = lambda s: (sys.stderr.write(s + "\n"), sys.stderr.flush())      # noqa: E731
    sigma, sigma_how = a.sigma, "fixed"
    if isinstance(sigma, str):
        if "denoise" not in a.variant:
            ap.error(f"--sigma {sigma} is for the denoise variants")
        if sigma == "auto":
            sigma_how = "auto"
        else:
            from .noise import parse_sigmas
            try:
                with open(sigma, "r") as fh:
                    sigma, sigma_how = parse_sigmas(fh.read()), "listed"
            except (OSError, ValueError) as e:
                ap.error(f"--sigma {a.sigma}: {e}")
    noise_model, nlf_how = None, "flat"
    if a.noise_model != "flat":
        if "denoise" not in a.variant:
            ap.error(f"--noise_model {a.noise_model} is for the denoise variants")
        if a.noise_model == "level":
            if sigma_how != "auto":
                ap.error("--noise_model level needs --sigma auto")
            noise_model, nlf_how = "level", "level"
        else:
            from .noise import parse_curves
            try:
                with open(a.noise_model, "r") as fh:
                    noise_model, nlf_how = parse_curves(fh.read()), "listed"
            except (OSError, ValueError) as e:
                ap.error(f"--noise_model {a.noise_model}: {e}")
    try:
        from .noise import check_clamp
        check_clamp(a.sigma_clamp)
    except ValueError as e:
        ap.error(f"--sigma_clamp: {e}")
    if a.scene_cuts == "off":
        cuts = None
    elif a.scene_cuts == "auto":
        cuts = "auto"
    else:
        from .scenes import parse_cuts
        try:
            with open(a.scene_cuts, "r") as fh:
                cuts = parse_cuts(fh.read())
        except (OSError, ValueError) as e:
            ap.error(f"--scene_cuts {a.scene_cuts}: {e}")
    picture, picture_how = picture_arg(a.picture), "fixed"
    if picture == "auto":
        picture_how = "auto"
    elif isinstance(picture, str):
        from .picture import read_pictures
        try:
            picture, picture_how = read_pictures(picture), "listed"
        except (OSError, ValueError) as e:
            ap.error(f"--picture {a.picture}: {e}")
    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    fout = sys.stdout.buffer if a.output == "-" else open(a.output, "wb")
    try:
        rd = Y4MReader(fin)
        hd = rd.header
        matrix = a.matrix or ("bt709" if hd.height >= 720 else "bt601")
        rng = a.range or (hd.color_range if hd.color_range in ("full", "limited") else "limited")
        log(f"input: {hd.width}x{hd.height} C{hd.chroma} F{hd.fps}; matrix {matrix}{'' if a.matrix else ' (default)'}, range {rng}"
            f"{'' if a.range else (' (stream)' if hd.color_range else ' (default)')}")
        fmt = yuv_fmt(hd.bits, hd.chroma_code, L.SN_YUV_BT709 if matrix == "bt709" else L.SN_YUV_BT601,
                      L.SN_YUV_FULL if rng == "full" else L.SN_YUV_LIMITED)
        net = load_net(a.variant, a.checkpoint, a.dtype)
        vr = VideoRestorer(net, a.one_len, sigma=sigma, pipeline=not a.no_pipeline, scene_cuts=cuts, cut_threshold=a.cut_threshold,
                           cut_ratio=a.cut_ratio, sigma_clamp=a.sigma_clamp, picture=picture, bar_level=a.bar_level, out_format=a.out_format,
                           dither=None if a.dither == "none" else a.dither, dither_seed=a.dither_seed, noise_model=noise_model)
        if a.out_format is not None or a.dither != "none":
            log(f"output: C{a.out_format or hd.chroma}{'' if a.out_format else ' (as the input)'}, dither {a.dither}"
                f"{' seed %d' % a.dither_seed if a.dither != 'none' else ''}")
        wr = Y4MWriter(fout, output_header(hd, a.out_format))
        t0 = time.perf_counter()
        n = 0
        for p in vr.restore(rd, fmt, hd.height, hd.width):
            wr.write(p)
            n += 1
            if n % max(a.one_len, 1) == 0:
                log(f"  {n} frames, {time.perf_counter() - t0:.1f} s")
        fout.flush()
        dt = time.perf_counter() - t0
        fwd = vr.stats["forward_s"]
        used = vr.stats.get("cuts", [])
        if vr.stats.get("cuts_ignored"):
            log(f"scene cuts at or beyond the end of the stream ({n} frames) ignored: {vr.stats['cuts_ignored']}")
        if a.cuts_out is not None:
            from .scenes import format_cuts
            with open(a.cuts_out, "w") as fh:
                fh.write(format_cuts(used))
        log(f"done: {n} frames in {dt:.2f} s, {n / dt if dt > 0 else 0.0:.2f} frames/s end to end, "
            f"{n / fwd if fwd > 0 else 0.0:.2f} frames/s forward only, {len(used) + 1} scene{'s' if used else ''}"
            f"{'' if cuts is None else (' (cuts found)' if cuts == 'auto' else ' (cuts listed)')}")
        wp = vr.stats.get("window_picture", [])
        if a.picture_out is not None:
            from .picture import write_pictures
            write_pictures(a.picture_out, wp, picture_how)
        if picture is not None:
            kinds = sorted({r for r in wp if r is not None})
            log(f"picture ({picture_how}): {sum(r is not None for r in wp)} of {len(wp)} window{'' if len(wp) == 1 else 's'} restored inside a rectangle"
                f"{': ' + ', '.join('%d:%d:%d:%d' % r for r in kinds[:4]) + (' ...' if len(kinds) > 4 else '') if kinds else ''}")
        ws = vr.stats.get("window_sigma")
        if a.sigma_out is not None:
            from .noise import format_sigmas
            with open(a.sigma_out, "w") as fh:
                fh.write(format_sigmas(ws or [], sigma_how))
        wn = vr.stats.get("window_nlf")
        if a.noise_model_out is not None:
            from .noise import format_curves
            with open(a.noise_model_out, "w") as fh:
                fh.write(format_curves(wn or [], nlf_how))
        if wn:
            log(f"noise model ({nlf_how}): knots min {min(min(c) for c in wn):.2f} / max {max(max(c) for c in wn):.2f} over {len(wn)} "
                f"window{'' if len(wn) == 1 else 's'}")
        if ws:
            log(f"sigma ({sigma_how}{', clamped to [%g, %g]' % tuple(a.sigma_clamp) if sigma_how == 'auto' else ''}): "
                f"min {min(ws):.2f} / median {float(np.median(ws)):.2f} / max {max(ws):.2f} over {len(ws)} window{'' if len(ws) == 1 else 's'}")
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
        if fout is not sys.stdout.buffer:
            fout.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
