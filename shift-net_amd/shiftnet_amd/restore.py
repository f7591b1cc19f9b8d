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

Active picture (``picture``, off by default): a letterboxed or pillarboxed stream is restored inside its picture rectangle only -- there the bytes
are those of restoring the cropped stream, and the bars leave as they came in.  The rectangle is given by the caller, for the stream or per window,
or found per window from the sums of the luma's rows and columns, made on the device from the payloads the window has uploaded anyway
(``sn_yuv_rowcol_sums``, shiftnet_amd/picture.py).

Output format (``out_format``, ``dither``; both off by default): the network's result is float32, and rounding it to the 8-bit codes it came from
puts back the steps that the noise just removed was hiding.  ``out_format`` writes another bit depth and chroma layout than was read (10 bit
from 8 bit footage keeps the precision); ``dither="tpdf"`` adds triangular noise of +-1 code before the rounding, which makes the mean of the codes
follow the value at the price of about 0.5 code rms of noise (``sn_egress_yuv_dither``, csrc/sn_yuv.hip).  The noise is a hash of the seed, the
sample's position and the number of the frame in its clip -- the stream, or the scene -- so the bytes do not depend on how the windows are run.

Amount and the removed view (``amount``, ``view``; both off by default): ``amount`` writes the input's codes moved by that share of the way to the
result's, separately for luma and chroma -- the fallback when the restoration is too strong; ``view="removed"`` writes input minus result around
mid-grey, to see whether detail leaves with the noise.  Both happen in the egress, in the code domain, from the payloads the window has uploaded
anyway (``sn_egress_yuv_mix``): amount 0 is the input byte for byte.  The blend is linear in the codes, not perceptual.

Noise level (``sigma``, ``noise_model``; denoise variants), method-noise report (``report``), tiles (``tile``), the self-ensemble (``ensemble``) and
windows that overlap in time (``window_overlap``): each is a part of its own, described at its class in shiftnet_amd/restore_parts.py (``NoiseLevel``,
``Report``, ``Tiles``, ``Ensemble``, ``Overlap``); the restorer holds each or None and calls it by name.

Ground truth (``restore(..., gt=...)``, off by default; needs ``report``): a second stream, the clean frames of which the input is a degraded copy, goes
through the pipeline beside the input, and the report gains PSNR and SSIM of the input and of every frame written against it (shiftnet_amd/fullref.py).

Added noise (``add_noise``, off by default): the other half of that experiment.  The frames given are the clean stream; a stage in front of everything
else degrades them on the device (``sn_yuv_degrade``, shiftnet_amd/degrade.py), the degraded payloads are the input of all the rest, and under
``report`` the clean ones are the truth.  Added blur (``add_blur``, off by default) is the same stage for the deblurrers: every frame becomes the mean
of the frames around it (``sn_yuv_blur``), as the deblur datasets are made.

Grain put back (``grain``, off by default): behind every window's egress, and ahead of the report, a spatially correlated Gaussian field is added to
the written payloads in place (``sn_yuv_grain``, shiftnet_amd/grain.py; the part ``Grain`` in restore_parts.py), at a level, a curve, or a share of
what the window was restored with.
Flicker taken out (``deflicker``, off by default): one more stage in front of everything else, in the place of ``add_noise`` and ``add_blur``.  Every
frame gets one tone curve that matches its luma histogram to the median of its neighbours' (``sn_yuv_code_hist``, the rule of
shiftnet_amd/deflicker.py on the host, ``sn_yuv_apply_lut``); the deflickered payloads are the input of all the rest.
Dirt taken out (``despot``, off by default): a stage in the same place, behind ``deflicker`` when both are on.  Every frame is repaired from its two
ORIGINAL neighbours along block vectors (``sn_yuv_block_motion`` both ways in time, ``sn_yuv_despot``; shiftnet_amd/despot.py states the rule); the
despotted payloads are the input of all the rest.
"""
from __future__ import annotations

import sys
import threading
import time
from typing import Iterable, Iterator, List, Sequence, Tuple

import numpy as np

from .restore_cli import amount_arg, main, make_parser, picture_arg, sigma_arg, tile_arg  # noqa: F401 -- the command line (restore_cli.py), reached through this module
from .restore_parts import Ensemble, Grain, NoiseLevel, Overlap, Report, Tiles, _Stat
from .windows import (DEFAULT_TILE_OVERLAP, DITHERS, FUTURE, PAST, PerWindow, _Frames, _SceneFrames, _Thread, amount_form, noise_model_form, pad_multiple,  # noqa: F401
                      padded_size, picture_form, plan_output, plan_scene_windows, plan_windows, quality_form, reflect_index, report_form, report_motion_form, scene_cuts_form,
                      sigma_estimator_form, sigma_form, sigma_motion_form, tile_form, plan_tiles, window_indices, ensemble_form, overlap_weights,
                      plan_overlap_windows, plan_scene_overlap_windows, window_overlap_form)

VARIANTS = {"deblur": "gshift_deblur1", "deblur_small": "gshift_deblur2", "denoise": "gshift_denoise1", "denoise_small": "gshift_denoise2"}


# ---- the pieces of the restorer: a slot, the state of one run (a per-window statistic, _Stat, lives in restore_parts.py) -----------------
class _Slot:
    """Everything one of the two double-buffer slots owns: staging and device buffers sized for the largest window, the events that order the
    streams about them, what the stager notes for the window the slot holds, and one state object per part that keeps any (None where it keeps none)."""

    def __init__(self, torch, dev, dtype, tin: int, tout: int, fb: int, ofb: int, pixels: int) -> None:
        self.pin_in = torch.empty((tin, fb), dtype=torch.uint8).pin_memory()
        self.pin_out = torch.empty((tout, ofb), dtype=torch.uint8).pin_memory()
        self.dev_in = torch.empty((tin, fb), dtype=torch.uint8, device=dev)
        self.dev_out = torch.empty((tout, ofb), dtype=torch.uint8, device=dev)
        # flat, sized for the full frame: a window's tensors are views of the leading elements at the padded size of its picture
        self.x = torch.empty(tin * 3 * pixels, dtype=dtype, device=dev)
        self.x32 = torch.empty(tin * 3 * pixels, dtype=torch.float32, device=dev) if dtype != torch.float32 else None
        self.ev_h2d, self.ev_ready, self.ev_done, self.ev_d2h = (torch.cuda.Event() for _ in range(4))
        self.rect = None                                          # the picture of the window the slot holds (None: the full frame)
        self.t0 = 0                                               # the frame number, in its clip, of the first frame that window restores
        self.head, self.written = 0, None                         # window_overlap: frames shared with the predecessor, frames written (None: all)
        self.seam = self.seam_size = None                         # what the part Overlap keeps per slot (restore_parts.py)
        self.used = False                                         # in this restore(): a window has gone through the slot
        self.sums = None                                          # picture="auto": _Stat of the window's row and column sums
        self.noise = self.report = None                           # what the parts NoiseLevel and Report keep per slot (restore_parts.py)
        self.dev_ref = None                                       # a mix or a report with another format out: the window's input payloads in the format written
        self.pin_gt = self.dev_gt = None                          # restore(gt=...): the truth for the frames the window writes, payloads of the format written


class _Run:
    """The records of one restore(): what every window used, the launches counted, the forward timers.  _finish_stats makes ``stats`` of it."""

    def __init__(self) -> None:
        self.timers: List = []
        self.staged = 0                                           # windows the stager has taken on
        self.window_sigma: List = []
        self.window_frame_sigma: List = []
        self.window_nlf: List = []
        self.window_picture: List = []
        self.picture_wait_ms: List[float] = []
        self.window_sigma_spatial: List = []                      # sigma_estimator other than "spatial": the two estimates before the rule and the clamp
        self.window_sigma_temporal: List = []
        self.window_pair_sigma: List = []
        self.window_pair_motion: List = []                        # sigma_motion: per window, per pair, noise.motion_summary's triple
        self.launches = {"noise": 0, "nlf": 0, "nlf_map": 0, "picture": 0, "thumb": 0, "noise_pairs": 0, "nlf_pairs": 0, "report": 0, "motion": 0,
                         "report_motion": 0, "report_mv": 0,      # report_motion: the block matcher on the written frames, the sums along its vectors
                         "report_quality": 0,                     # report_quality: the NIQE sums of the input and of the written frames
                         "fullref": 0,                            # gt: the difference sums and the SSIM sums of input and written frames against the truth
                         "tile": 0,                               # tile: the tiles added into the canvas
                         "geo_transform": 0, "geo_accumulate": 0, # ensemble: the members' inputs made, their results added into the canvas
                         "overlap": 0,                            # window_overlap: the cross-fades of shared frames
                         "degrade": 0,                            # add_noise: the chunks of the clean stream degraded
                         "blur": 0,                               # add_blur: the scene segments of the chunks of the sharp stream blurred
                         "grain": 0,                              # grain: the windows whose written payloads got grain
                         "deflicker": 0,                          # deflicker: the histogram and the table launches of the chunks of the stream
                         "despot": 0}                             # despot: the motion launches of the chunks (two each) and the repair launches
        self.frame_despot: List = []                              # despot: (seeds, replaced, share, kept) of every frame, in stream order
        self.frame_deflicker: List = []                           # deflicker: (r, mean_in, mean_out, chroma_gain) of every frame, in stream order
        self.window_grain: List = []                              # grain: the 16 knots (sigma of 8-bit R'G'B') of every window's grain
        self.window_written: List[int] = []                       # window_overlap: the frames every window wrote
        self.seam_rms: List = []                                  # ... and per window None or the rms difference of the two answers on every shared frame
        self.window_tiles: List = []                              # tile: per window, the (y0, x0, th, tw) of its tiles in the order they ran
        self.frame_sums: List = []                                # report: the 16 sums of every frame handed out, the window it came from, that window's sigma
        self.frame_window: List[int] = []
        self.frame_sigma: List = []
        self.pair_sums_mv: List = []                              # report_motion: the 8 sums of the pair (frame, frame + 1) of every frame handed out, or None
        self.frame_size: List = []                                # ... and the (h, w) of the picture its window was restored in
        self.frame_niqe: List = []                                # report_quality: (niqe_in, niqe_out) of every frame handed out
        self.gt = None                                            # gt: the iterator over the truth's payloads, and how many the stager has taken
        self.gt_taken = 0
        self.frame_fullref: List = []                             # gt: the fullref.FullRef of every frame handed out
        self.collected = 0                                        # windows handed out
        self.src = None                                           # the frame source


# ---- cut detection on the device ----------------------------------------------------------------------------------------------------
class _DeviceThumbs:
    """The decider of _SceneFrames for ``scene_cuts="auto"``: host payloads -> luma thumbnails on the device (sn_yuv_thumb) -> scenes.CutDetector.

    The detector has an upload of its own, luma bytes only: which frames a window holds depends on the decisions, so the thumbnails must exist
    before the window is assembled and uploaded, and the window's upload repeats reflected frames while the detector takes every frame once.
    One chunk = the new frames of one window: their luma planes go through a pinned buffer into payload-shaped device slots (the chroma part
    of a slot is never written and never read), one launch makes the thumbnails, one copy brings the uint16 sums back into pinned memory, and the
    calling thread waits for the event recorded behind that copy on the detector's own stream -- never for the device, and never for the stream
    the forward runs on."""

    def __init__(self, torch, dev, fmt, h: int, w: int, chunk: int, threshold: float, ratio: float, run: "_Run") -> None:
        from .scenes import CutDetector
        self.torch, self.dev, self.fmt, self.h, self.w, self.chunk, self.run = torch, dev, fmt, h, w, chunk, run
        self.lb = h * w * (1 if fmt.bits == 8 else 2)                    # the luma plane leads the payload
        self.pin_y = torch.empty((chunk, self.lb), dtype=torch.uint8).pin_memory()
        self.dev_y = torch.empty((chunk, fmt.frame_bytes(h, w)), dtype=torch.uint8, device=dev)
        self.thumbs = _Stat(torch, dev, "thumb", chunk, [((h + 7) // 8, (w + 7) // 8)], torch.uint16)
        self.stream = torch.cuda.Stream(dev)
        self.detector = CutDetector(h, w, fmt.bits, threshold, ratio)
        self.lookahead = self.detector.lookahead
        self.frames = 0

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
                self.thumbs.launch(t, self.run, lambda out: thumb_yuv(self.dev_y[:t], self.fmt, self.h, self.w, out=out))
            self.detector.feed(self.thumbs.wait(t)[0])
            self.frames += t

    def finish(self) -> None:
        self.detector.finish()

    @property
    def decided(self) -> int:
        return self.detector.decided

    def is_cut(self, t: int) -> bool:
        return self.detector.is_cut(t)


# ---- a degraded copy of a clean stream, made in front of everything else ----------------------------------------------------------------
class _DeviceStage:
    """What the stages in front of the frame source share (``add_noise``: _DeviceDegrade, ``add_blur``: _DeviceBlur), in the style of _DeviceThumbs:
    host payloads go through a pinned buffer to the device on a stream of the stage's own, the stage's launches make up to ``chunk`` payloads of them,
    one copy brings those back into pinned memory, and the calling thread waits for the event recorded behind that copy -- never for the device, and
    never for the stream the forward runs on.  ``held``: the source payloads the device buffer has room for.  ``keep_clean``: the clean payloads queue
    up as the run's truth (``truth()``), in the order the frames are read, which is the order they are written in."""

    def __init__(self, torch, dev, fmt, h: int, w: int, chunk: int, held: int, keep_clean: bool, run: "_Run") -> None:
        from collections import deque
        self.torch, self.dev, self.fmt, self.h, self.w, self.chunk, self.run = torch, dev, fmt, h, w, chunk, run
        fb = fmt.frame_bytes(h, w)
        self.pin_in, self.pin_out = (torch.empty((k, fb), dtype=torch.uint8).pin_memory() for k in (held, chunk))
        self.dev_in, self.dev_out = (torch.empty((k, fb), dtype=torch.uint8, device=dev) for k in (held, chunk))
        self.stream, self.event = torch.cuda.Stream(dev), torch.cuda.Event()
        self.clean = deque() if keep_clean else None

    def _chunk(self, part: Sequence[np.ndarray], at: int, launch, tap) -> Iterator[np.ndarray]:
        """``part``: the host payloads read for this chunk -> dev_in[at : at + len(part)]; ``launch()``, on the stage's stream, leaves t payloads in
        dev_out and returns t; -> their host copies, in order, ``tap`` called with each before it is handed on."""
        torch = self.torch
        k = len(part)
        pin = self.pin_in.numpy()
        for i, f in enumerate(part):
            pin[i] = f
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            if k:
                self.dev_in[at:at + k].copy_(self.pin_in[:k], non_blocking=True)
            t = launch()
            self.pin_out[:t].copy_(self.dev_out[:t], non_blocking=True)
            self.event.record()
        self.event.synchronize()
        if self.clean is not None:
            self.clean.extend(pin[:k].copy())
        for d in self.pin_out[:t].numpy().copy():
            if tap is not None:
                tap(d)
            yield d

    def truth(self) -> Iterator[np.ndarray]:
        """The clean payloads, oldest first: a window's own frames have been read, and so degraded, before the stager asks for their truth."""
        while True:
            yield self.clean.popleft()


class _DeviceDegrade(_DeviceStage):
    """``add_noise``: the clean stream's payloads -> the degraded stream's, which the rest of restore() takes for its input (sn_yuv_degrade).

    Chunks of up to ``chunk`` payloads, one launch each.  The noise of a frame is keyed by its index in the STREAM, which only this stage knows:
    whatever the windows, the scenes and the reflections make of a frame later, it carries the same noise."""

    def __init__(self, torch, dev, fmt, h: int, w: int, chunk: int, knots: Sequence[float], seed: int, keep_clean: bool, run: "_Run") -> None:
        from .degrade import gauss_table
        super().__init__(torch, dev, fmt, h, w, chunk, chunk, keep_clean, run)
        self.knots, self.seed = knots, seed
        self.gauss = torch.from_numpy(gauss_table().copy()).to(dev)

    def frames(self, it: Iterable[np.ndarray], tap=None) -> Iterator[np.ndarray]:
        """The degraded payloads of ``it``'s clean ones, in order; ``tap`` is called with each before it is handed on."""
        from itertools import islice
        from .io_edges import degrade_yuv
        it, f0 = iter(it), 0
        while True:
            part = list(islice(it, self.chunk))
            t = len(part)
            if not t:
                return

            def launch() -> int:
                degrade_yuv(self.dev_in[:t], self.fmt, self.h, self.w, self.knots, self.seed, f0, self.gauss, out=self.dev_out[:t])
                self.run.launches["degrade"] += 1
                return t

            yield from self._chunk(part, 0, launch, tap)
            f0 += t


class _DeviceBlur(_DeviceStage):
    """``add_blur``: the sharp stream's payloads -> the blurred stream's, which the rest of restore() takes for its input (sn_yuv_blur).

    Output f is the mean of the n frames around frame f of the stream, so the stage reads r = n // 2 frames ahead of the chunk it makes, and launches
    once per scene segment of the chunk (degrade.plan_blur): under a LISTED ``scene_cuts`` the averaging window is clamped to the frame's scene, as it
    is to the stream's two ends.  **The 2r halo frames are carried on the device**: the device buffer holds chunk + 2r source payloads, and after a
    chunk's launches the payloads the next chunk's windows reach back to are moved to its front (two device copies of at most 2r payloads); only new
    frames are uploaded, each once."""

    def __init__(self, torch, dev, fmt, h: int, w: int, chunk: int, n: int, gamma: float, cuts, keep_clean: bool, run: "_Run") -> None:
        from .degrade import gamma_tables
        r = n // 2
        super().__init__(torch, dev, fmt, h, w, chunk, chunk + 2 * r, keep_clean, run)
        self.n, self.cuts = n, cuts
        self.tables = None if gamma == 1.0 else tuple(torch.from_numpy(t.copy()).to(dev) for t in gamma_tables(gamma))
        self.halo = torch.empty((2 * r, fmt.frame_bytes(h, w)), dtype=torch.uint8, device=dev) if r else None

    def frames(self, it: Iterable[np.ndarray], tap=None) -> Iterator[np.ndarray]:
        """The blurred payloads of ``it``'s sharp ones, in order; ``tap`` is called with each before it is handed on."""
        from itertools import islice
        from .degrade import plan_blur
        from .io_edges import blur_yuv
        it, r = iter(it), self.n // 2
        f0, base, held, ended = 0, 0, 0, False                   # the next output; dev_in[:held] are frames base .. base + held - 1 of the stream
        while True:
            want = f0 + self.chunk + r - (base + held)           # up to r frames past the chunk
            part = [] if ended else list(islice(it, want))
            ended = ended or len(part) < want
            S = held + len(part)
            last = base + S - 1
            t = min(self.chunk, last - f0 + 1)
            if t < 1:
                return
            keep_from = max(base, f0 + t - r)                    # what the next chunk's windows reach back to

            def launch() -> int:
                for a, cnt, lo, hi in plan_blur(f0, t, self.n, self.cuts, last, ended):
                    blur_yuv(self.dev_in[:S], self.fmt, self.h, self.w, self.n, a - base, max(lo, base) - base, min(hi, last) - base, self.tables,
                             out=self.dev_out[a - f0:a - f0 + cnt])
                    self.run.launches["blur"] += 1
                k = last + 1 - keep_from
                if k > 0 and keep_from > base:                   # through a buffer of its own: the two ranges may overlap
                    self.halo[:k].copy_(self.dev_in[keep_from - base:S])
                    self.dev_in[:k].copy_(self.halo[:k])
                return t

            yield from self._chunk(part, held, launch, tap)
            f0, base, held = f0 + t, keep_from, max(last + 1 - keep_from, 0)


class _DeviceDeflicker(_DeviceStage):
    """``deflicker``: the stream's payloads -> the same payloads under one tone curve per frame, which the rest of restore() takes for its input
    (sn_yuv_code_hist, the rule of shiftnet_amd/deflicker.py on the host, sn_yuv_apply_lut).  Payloads in, payloads out, the whole frame always.

    Frame f's curve needs the histograms of frames f - R .. f + R, so the stage reads R frames ahead of the chunk it makes, as _DeviceBlur does.  Every
    frame is uploaded once; the device buffer holds chunk + R payloads and the payloads the next chunk still needs move to its front.  The histograms
    of the last R frames behind the chunk stay on the host (at most 4 KB per frame come back).  Per chunk: one histogram launch on the new frames,
    their copy to pinned memory and a wait ON THE STAGE'S OWN STREAM ONLY, the tables of the chunk's frames on the host and their upload, one apply
    launch.  A closing chunk that reads no new frame has no histogram launch.  Under a LISTED ``scene_cuts`` the window is clamped to the frame's
    scene (degrade.plan_blur), as it is to the stream's two ends."""

    def __init__(self, torch, dev, fmt, h: int, w: int, chunk: int, R: int, chroma: str, cuts, run: "_Run") -> None:
        from collections import deque
        super().__init__(torch, dev, fmt, h, w, chunk, chunk + R, False, run)
        self.R, self.chroma, self.cuts = R, chroma, cuts
        codes = 1 << fmt.bits
        self.pin_hist = torch.empty((chunk + R, codes), dtype=torch.int32).pin_memory()
        self.dev_hist = torch.empty((chunk + R, codes), dtype=torch.int32, device=dev)
        self.pin_lut = torch.empty((chunk, 2, codes), dtype=torch.int16).pin_memory()
        self.dev_lut = torch.empty((chunk, 2, codes), dtype=torch.int16, device=dev)
        self.halo = torch.empty((R, fmt.frame_bytes(h, w)), dtype=torch.uint8, device=dev)
        self.hists = deque()                                      # host: the histograms of frames hist0 .. of the stream
        self.hist0 = 0

    def frames(self, it: Iterable[np.ndarray], tap=None) -> Iterator[np.ndarray]:
        """The deflickered payloads of ``it``'s, in order; ``tap`` is called with each before it is handed on."""
        from itertools import islice
        from .deflicker import tables
        from .degrade import plan_blur
        from .io_edges import apply_lut_yuv, code_hist_yuv
        it, R = iter(it), self.R
        f0, held, ended = 0, 0, False                             # the next output; dev_in[:held] are frames f0 .. f0 + held - 1 of the stream
        while True:
            want = self.chunk + R - held                          # up to R frames past the chunk
            part = [] if ended else list(islice(it, want))
            ended = ended or len(part) < want
            k, S = len(part), held + len(part)
            last = f0 + S - 1
            t = min(self.chunk, S)
            if t < 1:
                return

            def launch() -> int:
                if k:
                    code_hist_yuv(self.dev_in[held:S], self.fmt, self.h, self.w, out=self.dev_hist[:k])
                    self.pin_hist[:k].copy_(self.dev_hist[:k], non_blocking=True)
                    self.event.record()
                    self.event.synchronize()                      # the stage's own stream: never the device, never the stream of the forward
                    self.hists.extend(self.pin_hist[:k].numpy().view(np.uint32).astype(np.int64))
                    self.run.launches["deflicker"] += 1
                H = np.stack(self.hists)                          # frames hist0 .. last
                lut = self.pin_lut.numpy().view(np.uint16)
                for a, cnt, lo, hi in plan_blur(f0, t, 2 * R + 1, self.cuts, last, ended):
                    lo = max(lo, self.hist0)                      # a clip that began further back: R frames behind the chunk are here, no window reaches past them
                    lut[a - f0:a - f0 + cnt], info = tables(H, lo - self.hist0, hi + 1 - self.hist0, R, self.fmt, self.chroma, a - self.hist0, cnt)
                    self.run.frame_deflicker.extend(info)
                self.dev_lut[:t].copy_(self.pin_lut[:t], non_blocking=True)
                apply_lut_yuv(self.dev_in[:t], self.fmt, self.h, self.w, self.dev_lut[:t], out=self.dev_out[:t])
                self.run.launches["deflicker"] += 1
                if S > t:                                         # through a buffer of its own: the two ranges may overlap
                    self.halo[:S - t].copy_(self.dev_in[t:S])
                    self.dev_in[:S - t].copy_(self.halo[:S - t])
                return t

            yield from self._chunk(part, held, launch, tap)
            f0, held = f0 + t, S - t
            while self.hist0 < f0 - R:                            # what no later window reaches back to
                self.hists.popleft()
                self.hist0 += 1


class _DeviceDespot(_DeviceStage):
    """``despot``: the stream's payloads -> the same payloads with dirt and blotches taken out, which the rest of restore() takes for its input
    (sn_yuv_block_motion both ways in time, sn_yuv_despot; shiftnet_amd/despot.py states the rule).  Payloads in, payloads out, the whole frame always.

    Frame f is repaired from the ORIGINAL frames f - 1, f and f + 1, so the stage reads one frame ahead of the chunk it makes, as _DeviceBlur does at
    three taps: every frame is uploaded once, the device buffer holds chunk + 2 payloads and the payloads the next chunk reaches back to move to its
    front.  Per chunk, on the stage's own stream: the two motion launches on the payloads held (``despot_vectors``), then one ``sn_yuv_despot`` launch
    per scene segment of the chunk (degrade.plan_blur): under a LISTED ``scene_cuts`` the frame's neighbours are those of its scene, as they are the
    stream's.  A clip's first and last frame have one neighbour only: a plain device copy and the record (0, 0, 0.0, False); a segment with nothing
    but such frames launches nothing, and a chunk with nothing but such segments has no motion launches either.  The counts come back with the
    payloads, behind the stage's own event; the guard -- a frame whose replaced share exceeds ``max_share`` is handed on as the ORIGINAL -- is a
    substitution of host bytes the stage still holds, not a second launch."""

    def __init__(self, torch, dev, fmt, h: int, w: int, chunk: int, T: int, K: int, G: int, chroma: str, max_share: float, cuts, run: "_Run") -> None:
        from collections import deque
        super().__init__(torch, dev, fmt, h, w, chunk, chunk + 2, False, run)
        self.T, self.K, self.G, self.chroma, self.max_share, self.cuts = T, K, G, chroma, max_share, cuts
        self.halo = torch.empty((2, fmt.frame_bytes(h, w)), dtype=torch.uint8, device=dev)
        self.pin_counts = torch.empty((chunk, 2), dtype=torch.int32).pin_memory()
        self.dev_counts = torch.empty((chunk, 2), dtype=torch.int32, device=dev)
        self.host = deque()                                       # host: the source payloads of frames host0 .. of the stream, for the guard
        self.host0 = 0

    def frames(self, it: Iterable[np.ndarray], tap=None) -> Iterator[np.ndarray]:
        """The payloads of ``it`` with dirt taken out, in order; ``tap`` is called with each before it is handed on."""
        from itertools import islice
        from .degrade import plan_blur
        from .despot import END_RECORD, frame_record
        from .io_edges import despot_vectors, despot_yuv
        from .noise import motion_grid
        it = iter(it)
        motion = 2 if all(motion_grid(self.h, self.w)) else 0     # a picture without a vector block: despot_vectors launches nothing
        f0, base, held, ended = 0, 0, 0, False                    # the next output; dev_in[:held] are frames base .. base + held - 1 of the stream
        while True:
            want = f0 + self.chunk + 1 - (base + held)            # one frame past the chunk
            part = [] if ended else list(islice(it, want))
            ended = ended or len(part) < want
            S = held + len(part)
            last = base + S - 1
            t = min(self.chunk, last - f0 + 1)
            if t < 1:
                return
            self.host.extend(np.array(f, copy=True) for f in part)
            keep_from = max(base, f0 + t - 1)                     # what the next chunk's first frame reaches back to
            inner = [False] * t                                   # the chunk's frames with two neighbours in their clip

            def launch() -> int:
                vectors = None
                for a, cnt, lo, hi in plan_blur(f0, t, 3, self.cuts, last, ended):
                    ia, ib = max(a, lo + 1), min(a + cnt - 1, hi - 1)      # hi is the clip's last frame, or a frame past the chunk
                    for f in range(a, a + cnt):
                        if not ia <= f <= ib:
                            self.dev_out[f - f0].copy_(self.dev_in[f - base])
                    if ia > ib:
                        continue
                    if vectors is None:
                        vectors = despot_vectors(self.dev_in[:S], self.fmt, self.h, self.w)
                        self.run.launches["despot"] += motion
                    despot_yuv(self.dev_in[:S], self.fmt, self.h, self.w, vectors[0], vectors[1], ia - base, ib - ia + 1, self.T, self.K, self.G,
                               self.chroma, out=self.dev_out[ia - f0:ib + 1 - f0], out_counts=self.dev_counts[ia - f0:ib + 1 - f0])
                    self.run.launches["despot"] += 1
                    inner[ia - f0:ib + 1 - f0] = [True] * (ib - ia + 1)
                self.pin_counts[:t].copy_(self.dev_counts[:t], non_blocking=True)
                k = last + 1 - keep_from
                if k > 0 and keep_from > base:                    # through a buffer of its own: the two ranges may overlap
                    self.halo[:k].copy_(self.dev_in[keep_from - base:S])
                    self.dev_in[:k].copy_(self.halo[:k])
                return t

            counts = None
            for i, d in enumerate(self._chunk(part, held, launch, None)):
                if counts is None:                                # behind the stage's event: the counts have come back with the payloads
                    counts = self.pin_counts[:t].numpy().view(np.uint32).copy()
                rec = frame_record(counts[i, 0], counts[i, 1], self.h * self.w, self.max_share) if inner[i] else END_RECORD
                if rec[3]:                                        # the guard: the original, from the host
                    d = self.host[f0 + i - self.host0].copy()
                self.run.frame_despot.append(rec)
                if tap is not None:
                    tap(d)
                yield d
            f0, base, held = f0 + t, keep_from, max(last + 1 - keep_from, 0)
            while self.host0 < f0:                                # the guard never reaches back
                self.host.popleft()
                self.host0 += 1


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
    format / no dither), ``stats["dither_seed"]`` the seed.
    amount: None -- the network's result is written, today's code path and bytes, and so are 1.0 and (1.0, 1.0); a number in [0, 1] -- every code
    written is ``code_in + amount * (code_out - code_in)`` rounded (dithered where ``dither`` says so): that share of the correction; ``(luma, chroma)``
    -- the two kinds of plane separately ("denoise chroma fully, luma at half" is ``(0.5, 1.0)``, "leave chroma alone" ``(1.0, 0.0)``).  The blend is
    made by the egress in the code domain (``sn_egress_yuv_mix``) against the payloads the window has uploaded anyway: amount 0 returns every input
    frame byte for byte, illegal codes included, and no float frame is made.  **Linear in the code domain, not perceptual**, and at 4:2:0 not the blend
    of the two R'G'B' pictures; nobody has judged it on real footage.  With ``out_format`` the input side of the blend is the input converted as the
    frames outside a picture are (``egress(out format, ingest_float32(in format, frame))``, undithered), kept in one more device buffer per slot.
    view: None -- the restored frames; ``"removed"`` (with ``amount`` None or 1) -- what the restoration took out: ``mid-grey + removed_gain * (code_in
    - code_out)`` per sample, clamped to the legal codes, 128 (512 at 10 bit) in all three planes where nothing changed.  ``removed_gain`` (finite, >= 0)
    makes small differences visible.  With ``picture`` the samples outside the rectangle stay what they are without a view.
    ``stats["amount"]`` is the pair of amounts used (None: none given) and ``stats["view"]`` the view.
    sigma_estimator: ``"spatial"`` -- the estimate of ``sigma="auto"`` as described above, today's launches, bytes and stats keys; ``"temporal"`` or ``"min"``
    (both need ``sigma="auto"``) -- the window's input frames as fed are also taken in consecutive pairs, and the same 2 x 2 statistic of the DIFFERENCE
    of the two frames is counted (``sn_yuv_noise_hist_pairs``, one more launch on the side stream): content that does not move cancels in it, so
    pixel-scale texture, which the spatial estimate reads as noise, does not reach it.  A pair of identical frames (a reflected duplicate in a clip of
    one or two frames, a repeated frame) has no estimate; the window's temporal sigma is the median over the pairs that have one.  ``"temporal"`` uses
    it, or the spatial estimate where no pair has one; ``"min"`` uses the lower of the two -- picture content can only push either one up.  The clamp
    comes last.  With ``noise_model="level"`` the curve is combined band by band in the same way (``sn_yuv_noise_hist_pairs_bands``,
    noise.window_curve_pairs).  **A heuristic, checked on synthetic clips only**: temporally correlated noise (inter-coded or temporally denoised footage)
    reads LOW, the one direction in which ``"min"`` can hurt; moving fine texture still raises both estimates.  With ``picture`` the pair statistic sees
    the window's rectangle, as the spatial one does; windows never cross a cut under ``scene_cuts``, and without it a cut inside a window is one outlier
    pair, which the median over the pairs takes.  ``stats`` then also has ``sigma_estimator``, ``window_sigma_spatial`` and ``window_sigma_temporal`` (the
    two estimates of every window before the rule and the clamp; None where no pair has one), ``window_pair_sigma`` (per window, one entry per pair, None
    allowed), ``noise_pairs_launches`` and, with ``"level"``, ``nlf_pairs_launches``; ``window_sigma``, ``window_frame_sigma`` and ``window_nlf`` keep their
    meaning: what the window was restored with, the per-frame spatial values, the curve used.
    sigma_motion: None -- the pairs compare every 2 x 2 block with the block at the same place in the next frame, today's launches, bytes and stats keys;
    ``"blocks"`` (needs ``sigma_estimator="temporal"`` or ``"min"``) -- once per window ``sn_yuv_block_motion`` (side stream) finds for every pair and
    every 16 x 16 luma block the integer translation within +-7 samples with the smallest sum of absolute differences, and
    ``sn_yuv_noise_hist_pairs_mv`` runs IN PLACE OF the plain pair histogram (with ``noise_model="level"`` ``..._bands_mv`` in place of the plain band
    one): the next frame's block is taken where the vector points.  The vector is chosen on one half of the 2 x 2 blocks (checkerboard parity even) and
    the statistic taken from the other half, so that the choice cannot fit the noise it is measured on (noise.py).  The vectors and their SADs live in
    per-slot device buffers; the vectors come back to the host in pinned memory (137 KB for a 720p window of 20 frames).  **A heuristic, checked on
    synthetic clips only**: integer-pel translation per block; sub-pixel motion, zoom, rotation, occlusion and changing motion blur still read as noise;
    temporally correlated noise still reads LOW; on flat content the estimate reads a few per cent HIGH.  With ``picture`` the vectors are those of the
    window's rectangle; a cut inside a window stays one outlier pair.  ``stats`` then also has ``sigma_motion`` and ``window_pair_motion`` (per window,
    per pair: the share of blocks with a nonzero vector, the median dy, the median dx), ``noise_launches`` counts the ``sn_yuv_block_motion`` launches
    beside the spatial histogram's, and ``noise_pairs_launches`` / ``nlf_pairs_launches`` count the ``_mv`` launches.
    report: False -- today's launches, bytes and stats keys; True -- behind every window's egress one more launch (``sn_yuv_diff_stats``, main stream)
    sums d = written - input over the window's own frames: the payloads written against the input frames in the format written -- the payloads read, or
    with ``out_format`` the input converted as ``amount`` defines it (``egress(out format, ingest_float32(in format, frame))``, undithered) -- inside the
    window's rectangle under ``picture``.  The sums are exact integers, the same with ``pipeline`` on and off, and no byte written changes.
    ``stats["frame_sums"]`` is one list of 16 ints per written frame (report.SUMS), ``stats["frame_report"]`` one report.FrameReport per frame: the
    luma difference's mean, rms and ``removed_sigma`` (its standard deviation as the sigma of i.i.d. noise on 8-bit R'G'B', the unit of ``sigma``), its
    correlation with the right and the lower neighbour (``rho_x``, ``rho_y``) and with the next frame's difference (``rho_t``; nan where the next frame
    lies in another window), the share of edge pixels and the mean of d^2 on them over that elsewhere (``edge_ratio``), the chroma planes' mean and rms;
    ``stats["report_summary"]`` their medians, ``stats["report_launches"]`` the launches.  A pixel is an edge where the written luma's gradient,
    |right - here| + |below - here|, is at least ``report_edge`` 8-bit codes (finite, >= 0; **the default of 16 is a guess nobody has tuned**).  The
    report describes the stream that was written: with ``amount`` the blended one, with ``dither`` the dither is part of d; ``view="removed"`` with
    ``report=True`` is a ValueError.  A noise-only removal reads rho_x ~ rho_y ~ rho_t ~ 0, edge_ratio ~ 1, removed_sigma ~ sigma.  **Unvalidated on real
    footage**: the deblur variants change edges by design, and at 4:2:0 the luma noise of real footage need not be white to begin with.
    report_motion: None -- today's launches, bytes, stats keys and report; ``"blocks"`` (needs ``report=True``) -- ``rho_t`` compares a frame's d with the
    next frame's at the same place, so removed detail that moves with the picture reads as uncorrelated, exactly as noise does.  Behind the report's
    launch, for every window that writes at least two frames, ``sn_yuv_block_motion`` finds the vectors of the WRITTEN frames' pairs (the clean picture,
    as for the edge rule) and ``sn_yuv_diff_stats_mv`` sums d of both frames of a pair along them, on the half of the 2 x 2 blocks the vectors were not
    chosen on (two more launches on the main stream; the vectors stay on the device).  ``stats`` then also has ``report_motion``, ``pair_sums_mv`` (per
    written frame the 8 ints of report.SUMS_MV for the pair with the next frame, None where that one lies in another window),
    ``frame_report_motion`` (one report.MotionReport per frame: ``rho_t_mv``, the rms of the written picture's difference along the vectors, the share
    of counted samples that moved, the share of the picture counted), ``report_motion_summary`` (their medians) and ``report_motion_launches``.
    ``frame_report``, ``frame_sums`` and every byte written stay what they are without it.  It is independent of ``sigma_motion``, whose vectors are
    those of the input frames as fed.  **Limits**: integer-pel vectors within +-7 samples per 16 x 16 block; half of the samples; blocks at the border
    whose true vector leaves the picture read low (the synthetic pans of the tests read 0.6 to 0.9 where everything removed was detail); pairs across windows have no value;
    zoom, rotation and occlusion still read as uncorrelated; no threshold and no verdict; unvalidated on real footage.
    report_quality: None -- today's launches, bytes, stats keys and report; ``"niqe"`` (needs ``report=True``) -- the report says what changed, not how the
    pictures look.  NIQE is a no-reference score: the distance of the statistics of a picture's 96 x 96 luma blocks, at two scales, from those of pristine
    natural images (shiftnet_amd/niqe.py; lower is nearer).  Behind the report's launch two more (``sn_yuv_niqe_sums``, main stream) make the per-pixel
    sums of the window's input frames and of the frames written for them, in the format written and on the same rectangle; the fit and the distance
    are float64 on the thread that hands the frames out.  ``stats["frame_niqe"]`` is one ``(niqe_in, niqe_out)`` per written frame (nan for a picture
    with fewer than two whole blocks), ``stats["report_quality_summary"]`` their medians ignoring nan, ``stats["report_quality_launches"]`` the
    launches.  ``niqe_params``: the pristine model's .npz (None: tests/golden/niqe_pris_params.npz of the checkout; a missing file is a ValueError
    that names the option).  The model was fitted on natural stills, on the Y of BT.601 R'G'B'; the stream's own luma is fed, whatever its matrix.
    Denoising can move the score either way -- over-smoothing is not natural either.  No threshold, no verdict, nothing fed back; **unvalidated on
    real footage**, and on synthetic weights it says nothing about the network.  No byte written changes.
    gt (an argument of ``restore()``, not of the constructor; needs ``report=True``, a ValueError naming it otherwise): None -- today's launches, bytes,
    stats keys and report; an iterable of payloads -- a ground-truth stream, frame i the truth of written frame i, **in the format written**
    (``out_format`` if given, else the input's) and of the stream's size: the standard experiment of a clean clip, a degraded copy and its restoration
    compared with the clip, on every frame and under every other option.  The stager takes from ``gt`` exactly the frames its window will write (all
    it restores, or fewer under ``window_overlap``) and uploads them on the side stream beside the window's input.  Behind the report's launches four
    more (main stream): ``sn_yuv_diff_stats`` of (truth, input as written) and of (truth, written), edge 0 -- exact sums, PSNR of Y, U and V with
    p = 2^bits - 1 -- and ``sn_yuv_ssim_sums`` of the same two pairs -- the Y-channel SSIM of the evaluation harnesses on the luma codes, constants
    following 2^bits - 1 (shiftnet_amd/fullref.py) -- on the same rectangle as the rest of the report under ``picture``.  ``stats["frame_fullref"]`` is
    one fullref.FullRef per written frame (``psnr_y_in``, ``psnr_y_out``, ... ``ssim_in``, ``ssim_out``: ``_in`` the input against the truth, ``_out``
    the frame written; ``inf`` where a plane equals the truth's), ``stats["fullref_summary"]`` their means (``inf`` frames left out and counted) and
    medians, ``stats["fullref_launches"]`` the launches, 4 per window.  A ``gt`` that ends before the frames written do is a ValueError naming ``gt`` and
    the frame; a payload of another size likewise; payloads beyond the input's last frame are not looked for, so a longer ``gt`` goes unnoticed.
    **Luma SSIM only; no MS-SSIM, no VMAF; the truth must be frame-aligned by the caller -- no offset is searched; no threshold, no verdict, nothing fed
    back into ``amount`` or ``sigma``.**  No byte written changes.
    tile: None -- the network is given whole frames, today's launches, bytes and stats keys; ``(th, tw)`` or an int ``n`` (``(n, n)``) -- the forward of
    every window runs on overlapping th x tw rectangles of the window's padded frames instead, one after the other in row-major order, each on the
    contiguous crop of the input tensors (and of the noise plane under ``noise_model``; a flat sigma is broadcast to the tile's shape), and
    ``sn_tile_accumulate`` adds each float32 result into one float32 canvas of the whole picture with feather weights; the egress, the mix and the
    report read the canvas as they read the network's result without tiles.  Ingest, the statistics, the noise plane and the egress still see the whole
    picture -- the frame, or the window's rectangle under ``picture`` -- so chroma is upsampled from its true neighbours and ``sigma="auto"`` still
    estimates on the whole frame.  Both sides are multiples of the network's padding multiple (4, or 8 for the "+" variants) and at least twice it.
    ``tile_overlap`` (an int, ``0 <= tile_overlap <= min(th, tw) // 2``): consecutive tiles overlap by at least that many samples.  The plan is
    windows.plan_tiles: per axis of length L, tiles of side S at ``min(k (S - overlap), L - S)`` -- all of one size, the last at the far edge -- and a
    side that is not shorter than the picture gives one tile; where two tiles overlap their results cross-fade linearly, a sample that one tile covers has
    weight exactly 1, and there is no ramp at the picture's own edges.  A window whose plan is one tile takes the path, the launches and the bytes of
    ``tile=None``.  With ``picture`` and ``out_format`` together, the input side of ``amount``'s blend and of the report is, inside the rectangle of a
    window that ran tiled, the rectangle converted as the cropped stream's frames are (two more launches, ``sn_ingest_yuv_rect`` and
    ``sn_egress_yuv_rect``), so that a tiled window equals the tiled cropped stream inside its rectangle byte for byte and sum for sum; without tiles it
    stays the whole frame converted, as ``amount`` describes it, which differs within 2 samples of the rectangle's edges where 4:2:0 chroma is
    upsampled from the bars.  The tiles of a window share one range-guard check and are run once more if it tripped.  **A tiled result is not the full-frame
    result**: every CALayer pools over the map it is given, so it sees the tile, and the receptive field is cut at tile edges; the feather turns a
    mismatch into a gradient instead of an edge, it does not remove it.  **The default overlap of 32 is taken from upstream's quadrants, which crop 17 to
    32 samples per side; nobody has tuned it, and no trained checkpoint ships, so nobody has looked at a seam on real footage.**  Tiles of one window run
    one at a time (not as one ``forward_clips`` batch), have one size, and do not cut the window in time.  ``stats`` then also has ``tile`` (th, tw),
    ``tile_overlap``, ``window_tiles`` (per window the list of (y0, x0, th, tw) in the order run) and ``tile_launches`` (the ``sn_tile_accumulate``
    launches).
    ensemble: None or 1 -- one forward per window, today's launches, bytes, buffers and stats keys; 2, 4 or 8 -- a test-time self-ensemble
    (shiftnet_amd/ensemble.py): the forward of every window runs on that many copies of the window's tensors -- the window itself, its columns
    mirrored, its rows mirrored and both, and at 8 the transposes of those four -- every float32 result is mapped back, and their mean is what the egress,
    the mix and the report read.  ``ensemble_time=True`` doubles the members: the same copies of the window reversed in time (a legal window, because
    it has as many past as future frames).  The network is not equivariant under any of these -- its grouped spatial shifts point in fixed directions
    and its temporal shift tells past from future -- so every member gives another answer.  **A window costs M forwards**, M the number of members (2
    to 16).  The copies are made by ``sn_geo_transform`` into buffers that are reused (the frames, their float32 twin and, under
    ``noise_model``, the noise plane, which is transformed with the frames; a flat sigma is the same for every member and copies nothing);
    ``sn_geo_accumulate`` adds each result into one float32 canvas and the last launch multiplies by 1 / M, which is exact: the result is the sequential
    float32 sum in the order of ``stats["ensemble_members"]``, divided by M -- ``net.forward_ensemble_fp32_out`` on the window, bit for bit.  The
    transposed members have another input signature, hp and wp swapped, so the engine keeps a plan of its own for them, and the first window pays
    for building it.  The members of a window share one range-guard check and are run once more if it tripped.  ``ensemble`` or ``ensemble_time`` together
    with ``tile`` is a ValueError: the tiles of a transposed member need a rule for their own sides.  **Nobody has measured what the ensemble gains on this
    network**: the +0.05 to +0.2 dB quoted for image super-resolution is a figure from the literature for other networks, not a property of Shift-Net,
    and no trained checkpoint ships here.  The ``inference/test_*.py`` harnesses, where a PSNR against ground truth could be measured once somebody
    has a checkpoint, do not take the option yet; ``GShiftNet.forward_ensemble_fp32_out`` is there for it.  ``stats`` then also has ``ensemble``,
    ``ensemble_time``, ``ensemble_members`` (the ops in the order run: bit 1 mirrors the columns, 2 the rows, 4 transposes, 8 reverses time) and
    ``ensemble_launches`` (``{"transform": the sn_geo_transform launches, "accumulate": the sn_geo_accumulate launches}``).
    window_overlap: 0 -- window k + 1 starts where window k ends, today's launches, bytes and stats keys; V, an integer with ``2 * V <= one_len`` --
    consecutive windows of a scene share V frames (windows.plan_scene_overlap_windows): the window after [lo, hi) starts at hi - V unless the scene ends
    at hi, and never reaches across a scene start.  Every window still runs on its own, with 2 input frames of context on each side; a window with a
    successor writes all but its last V frames and keeps those, float32, in one carry buffer on the device; the successor's first V frames are
    cross-faded with them in place before its egress (``sn_time_crossfade``, csrc/sn_time.hip; one launch per seam on the main stream): on shared frame
    j = 0 .. V - 1 the newer window weighs ``(j + 1) / (V + 1)`` and the older ``(V - j) / (V + 1)`` (windows.overlap_weights, the ramp of two tiles
    that overlap by V).  Every frame is still written once and in order, and the bytes are the same with ``pipeline`` on and off.  The per-window
    options and statistics stay per window -- ``sigma`` / ``noise_model`` / ``picture`` lists, ``stats["window_*"]`` -- there are simply more windows, and
    a list written with one overlap reproduces the bytes when read back with the same overlap; the dither's frame number is that of the window's first
    written frame, so dithered bytes do not depend on the windowing of frames one window covers; the report's ``rho_t`` stays nan across windows.  Two
    windows whose ``picture`` rectangles differ have results of different shapes: their shared frames are the later window's alone.  The same launch
    sums the squared difference of the two answers before the blend, exactly (integers; clamped to +-8 per sample): ``stats["seam_rms"]`` has per window
    None (no predecessor in its scene, or another rectangle) or V numbers, the rms difference in 8-bit R'G'B' code units on each shared frame, oldest
    first -- how far a window's edge is from the next window's interior, on any footage with any weights.  ``stats["window_overlap"]`` is V,
    ``stats["window_written"]`` the frames every window wrote, ``stats["overlap_launches"]`` the launches.  **A window still costs one forward, and
    there are one_len / (one_len - V) times as many.  The cross-fade blends two different answers -- restored with different sigmas, possibly -- so a
    mismatch becomes a ramp over V frames and is not removed.  Nobody has looked at a seam of a trained network: no checkpoint ships, and ``seam_rms`` on
    synthetic weights says nothing about one; it is there so that somebody with a checkpoint can find out.**
    add_noise: None -- the frames given are the input, today's launches, bytes and stats keys; a number, or 16 numbers (each finite and >= 0) -- the
    frames given are a CLEAN stream, and a stage in front of everything else makes the input from them on the device (``sn_yuv_degrade``,
    csrc/sn_degrade.hip; shiftnet_amd/degrade.py): ``egress(ingest_float32(frame) + s * g)``, Gaussian noise g, i.i.d. per R'G'B' channel and pixel, with
    sigma s in 8-bit code units -- the number, or the curve of 16 knots (noise.knot_codes, what ``noise_model`` reads) at the pixel's own clean luma
    code.  Chunks of up to ``one_len`` payloads go to the device on a stream of the stage's own, one launch each, and come back as payloads; the rest
    of restore() -- the cut detector, the stager, every statistic, ``amount``, ``view`` -- takes the degraded payloads for THE input and is untouched.
    The noise of a frame is a hash of ``add_noise_seed`` (0 .. 2^32 - 1), the frame's index in the stream, the channel, the row and the column: a frame
    carries the same noise as a window's own frame, as a neighbour's halo, reflected at a clip's end, and under ``scene_cuts`` and ``window_overlap``.
    With ``report=True`` the clean payloads are the run's truth by the mechanism of ``gt``: ``stats["frame_fullref"]`` and the report's eight columns
    appear without a second stream.  ``restore(..., degraded=callable)`` is called with every degraded payload, in order.  ``add_noise`` with ``gt`` is
    a ValueError, and so is ``add_noise`` with ``report`` and an ``out_format`` that differs from the input's (the truth would have to be converted).
    ``stats`` then also has ``add_noise`` (the 16 knots), ``add_noise_seed`` and ``degrade_launches``.  **The conversion round trip runs even at sigma
    0**: at 4:2:0 the degraded stream's chroma has been up- and down-sampled once, ``psnr_u_in`` / ``psnr_v_in`` include that, and sigma 0 is not the
    input byte for byte.  **The noise is clipped** to [0, 1] and to the legal codes on the way out; **its tails end at about 4.3 sigma** (a table of
    65536 quantiles); it is added before the chroma subsampling and depends on the clean luma only: what the networks were trained with, not a sensor
    and a codec.  **Bars are noised too**: ``picture="auto"`` then needs a higher ``bar_level``.  It covers the noise experiment only -- no blur is
    synthesised by it (``add_blur`` does that) -- and says nothing about the network without a trained checkpoint.
    add_blur: None -- as above; an odd integer N in 1 .. 15 -- the frames given are a SHARP stream, and the same stage in front of everything else
    makes the input from them on the device (``sn_yuv_blur``, csrc/sn_blur.hip; shiftnet_amd/degrade.py): frame f of the input is the mean of frames
    f - N // 2 .. f + N // 2 of the stream, taken on R'G'B' between the two colour edges, in linear light through ``add_blur_gamma`` (finite, in
    [1, 3], default 2.2, GOPRO's; exactly 1 averages the R'G'B' values as they are, DVD's) -- how the deblur datasets are made, with the sharp centre
    frame for the truth.  The window is clamped at the stream's two ends, so the first and last frames are replicated.  With a LISTED ``scene_cuts``
    it is clamped to the frame's scene as well.  **With ``scene_cuts="auto"`` it is not: the cuts are found afterwards, on the blurred stream, and the
    blur crosses them** -- N // 2 frames on either side of a cut are a mix of two scenes, and the detector sees a cross-fade where the cut was.  The
    stage reads N // 2 frames ahead, launches once per scene segment of a chunk of ``one_len`` frames, and carries the frames two chunks share on the
    device.  ``report``, ``degraded`` and the refusals are ``add_noise``'s (not with ``gt``; not with ``report`` and another ``out_format``); and
    ``add_blur`` with ``add_noise`` is a ValueError: no network here was trained on both.  ``stats`` then also has ``add_blur``, ``add_blur_gamma``
    and ``blur_launches``.  **The blur is a box over N frames of the stream as it is**: its length in time is N / fps of the input, no frame is
    dropped, and a stream that was not shot at a high frame rate gets ghosting and not motion blur.  **A pure power law, not the sRGB curve; not a
    lens and not a rolling shutter.**  **N = 1 still runs the conversion round trip** (see ``add_noise``), and **bars are averaged too**.
    grain: None -- nothing is added to what the egress wrote, today's launches, bytes and stats keys; a number G, or 16 numbers (each finite and >= 0)
    -- behind every window's egress, and ahead of the report, one launch (``sn_yuv_grain``, csrc/sn_grain.hip; main stream) puts grain back on the
    window's written payloads in place, inside its rectangle under ``picture`` (restore_parts.Grain; shiftnet_amd/grain.py): a Gaussian field times a
    level, added to the codes and rounded.  The level is in the unit of ``sigma``: the sigma of i.i.d. noise on 8-bit R'G'B' whose LUMA part the grain
    equals; 16 numbers are a curve (noise.knot_codes) taken at the written luma code.  ``"auto"`` / ``"auto:SHARE"`` (denoise variants; SHARE in
    [0, 4], default 0.5): SHARE times what the window was restored with -- its sigma as 16 equal knots, or its curve under ``noise_model`` -- whether
    that was given, listed or estimated.  ``grain_size`` (0 .. 1.2): the standard deviation, in samples, of the 5-tap Gaussian of unit energy the white
    field is filtered with each way; 0 is white grain.  ``grain_chroma`` (>= 0): the chroma planes get fields of their own at that share of the
    level (0: chroma stays); ``grain_seed`` (0 .. 2^32 - 1) picks the grain.  The field is a hash of the seed, the plane, the sample's row and column
    counted from the picture's origin and the dither's frame number, so the bytes are the same with ``pipeline`` on and off, those of restoring every
    scene as a separate video, and inside a picture those of the cropped stream.  ``report``, ``gt`` and NIQE describe the stream that is written,
    grain included.  ``grain`` with ``view="removed"`` is a ValueError, and so are ``"auto"`` with a deblur variant and any of the other three without
    ``grain``.  ``stats`` then also has ``grain`` (the 16 knots, or ``"auto:SHARE"``), ``grain_size``, ``grain_chroma``, ``grain_seed``,
    ``window_grain`` (the 16 knots of every window, in the unit above) and ``grain_launches``.  **A Gaussian field of a size the user chooses, not a
    model fitted to the removed noise: no AR fit, no film-grain table for an encoder.**  Its level is a function of the written luma code alone; it is
    independent from frame to frame; under ``"auto"`` it steps at window boundaries with the estimate; codes are integers, so the grain itself is
    rounded (variance L^2 + 1/12) and clipped at the legal range; 4:2:0 chroma grain lives at chroma resolution and looks twice the size; the chroma
    share is a plain factor; ``sigma="auto"`` run on a re-grained stream reads about (1 - rho_1) G for sized grain (grain.lag1; 0.33 G at size 0.8).
    **Nobody has judged it on real footage.**
    deflicker: None -- the frames given are the input, today's launches, bytes and stats keys; an integer R in 1 .. 15 -- a stage in front of
    everything else (_DeviceDeflicker; ``sn_yuv_code_hist`` and ``sn_yuv_apply_lut``, csrc/sn_deflicker.hip; a stream of its own) takes brightness
    flicker out of the payloads, whole frames, no float frame and no colour conversion: every frame gets ONE tone curve that matches its luma
    histogram to the median of the quantiles of the r = min(R, frames to the clip's start, frames to its end) frames on either side
    (shiftnet_amd/deflicker.py states the rule and its limits).  The clip is the stream, or the frame's scene under a LISTED ``scene_cuts``; with
    ``"auto"`` the cuts are found afterwards, on the deflickered stream.  ``deflicker_chroma``: ``"gain"`` scales Cb and Cr about mid-grey by the
    factor the frame's mean luma above black changed by, clamped to [0.5, 2]; ``"off"`` leaves chroma as it came.  The rest of restore() -- the cut
    detector, the stager, every statistic, ``amount`` (0 returns the deflickered stream), ``view``, ``report``, ``gt`` -- takes the deflickered
    payloads for THE input.  ``restore(..., deflickered=callable)`` is called with every one of them, in order.  A static clip leaves byte for byte.
    ``deflicker`` with ``add_noise`` or ``add_blur`` is a ValueError.  ``stats`` then also has ``deflicker``, ``deflicker_chroma``,
    ``frame_deflicker`` ((r, mean_in, mean_out, chroma_gain) of every frame) and ``deflicker_launches`` (two per chunk of ``one_len`` frames; one
    for a closing chunk that reads no new frame).  **One curve per frame: local flicker stays; a real flash is pulled towards its neighbours; luma
    decides alone; computed on codes, not in linear light; bars are in the histogram; moving content that changes the histogram reads as flicker.
    Nobody has judged it on real footage.**
    despot: None -- the frames given are the input, today's launches, bytes and stats keys; an integer T in 1 .. 255, the threshold in 8-bit codes --
    a stage in front of everything else (_DeviceDespot; ``sn_yuv_block_motion`` on the stack and on the time-reversed stack, ``sn_yuv_despot``,
    csrc/sn_despot.hip; a stream of its own) takes dirt, dust, blotches and dropouts out of the payloads -- small regions that are wrong in exactly
    ONE frame -- whole frames, no float frame and no colour conversion.  Frame f is repaired from the ORIGINAL frames f - 1, f, f + 1 only, never from
    a repaired neighbour, so the result depends on neither ``one_len``, the windows nor ``pipeline``: a luma sample is a seed iff it differs from both
    motion-compensated neighbours in the same direction by more than T + |p - n|; a seed with at least ``despot_support`` (K, 0 .. 8, default 2)
    seeds among its eight neighbours is a core seed; the core seeds grown by ``despot_grow`` (G, 0 .. 2, default 1) samples are replaced by
    (p + n + 1) >> 1; ``despot_chroma``: ``"follow"`` repairs chroma where its luma is repaired, ``"off"`` leaves it (shiftnet_amd/despot.py states
    the rule and its limits).  The clip is the stream, or the frame's scene under a LISTED ``scene_cuts``; a clip's first and last frame leave as they
    came; with ``"auto"`` the cuts are found afterwards, on the despotted stream.  A frame of which more than ``despot_max_share`` (default 0.05)
    would be replaced -- a flash, a frame under uncorrected flicker, a cut the motion search could not follow -- is handed on as it came and marked
    kept.  **With ``deflicker`` the stage runs BEHIND it**, each on a stream of its own: uncorrected flicker makes whole frames read as spikes, so
    flicker goes first.  The rest of restore() -- the cut detector, the stager, every statistic, ``amount``, ``view``, ``report``, ``gt`` -- takes
    the despotted payloads for THE input.  ``restore(..., despotted=callable)`` is called with every one of them, in order.  A static clip leaves
    byte for byte.  ``despot`` with ``add_noise`` or ``add_blur`` is a ValueError.  ``stats`` then also has ``despot``, ``despot_support``,
    ``despot_grow``, ``despot_chroma``, ``despot_max_share``, ``frame_despot`` ((seeds, replaced, share, kept) of every frame) and
    ``despot_launches`` (per chunk of ``one_len`` frames the two motion launches and one repair launch per scene segment that has a frame with two
    neighbours).  **One threshold in codes, not scaled to the footage's noise; integer-pel vectors within +-7 px per 16 x 16 block, chosen on a block
    that contains the dirt; dirt that persists for two frames, line scratches and anything else that stays are not found; small fast objects that
    are in one place for one frame ARE taken for dirt; the repair is the mean of two neighbours, which is soft; luma alone decides.  Nobody has
    judged it on real footage.**"""

    def __init__(self, net, one_len: int, sigma=None, pipeline: bool = True, scene_cuts=None,
                 cut_threshold: float = 4.0, cut_ratio: float = 2.5, sigma_clamp: Sequence[float] = (0.0, 50.0),
                 picture=None, bar_level: float = 1.0, out_format=None, dither=None, dither_seed: int = 0, noise_model=None,
                 amount=None, view=None, removed_gain: float = 1.0, sigma_estimator: str = "spatial", report: bool = False,
                 report_edge: float = 16.0, sigma_motion=None, report_motion=None, tile=None,
                 tile_overlap: int = DEFAULT_TILE_OVERLAP, ensemble=None, ensemble_time: bool = False, window_overlap: int = 0,
                 report_quality=None, niqe_params=None, add_noise=None, add_noise_seed: int = 0, add_blur=None,
                 add_blur_gamma: float = 2.2, grain=None, grain_size: float = 0.0, grain_chroma: float = 0.0, grain_seed: int = 0, deflicker=None,
                 deflicker_chroma: str = "gain", despot=None, despot_support: int = 2, despot_grow: int = 1, despot_chroma: str = "follow",
                 despot_max_share: float = 0.05) -> None:
        import torch
        from .deflicker import deflicker_form
        from .despot import despot_form
        from .degrade import add_blur_form, add_noise_form
        from .grain import grain_form
        from .lib import YuvFmt
        from .noise import check_clamp
        self.torch = torch
        _, self.dither, self.dither_seed = plan_output(YuvFmt(8, 0, 0, 0), out_format, dither, dither_seed)      # the argument errors, before anything else
        self.out_format = out_format
        # the mix of the last egress (None: the code path without any of it), the amounts and the view as stats reports them
        self.mix, self.amount, self.view = amount_form(amount, view, removed_gain)
        self.report, self.report_edge = report_form(report, report_edge, self.view)      # False: the code path without any of it
        self.report_motion = report_motion_form(report_motion, self.report)      # None: the code path without any of it
        self.report_quality = quality_form(report_quality, niqe_params, self.report)      # None: the code path without any of it; or the pristine model
        self.net, self.one_len, self.pipeline = net, int(one_len), bool(pipeline)
        if self.one_len < 1:
            raise ValueError("one_len must be >= 1")
        self.window_overlap = window_overlap_form(window_overlap, self.one_len)      # 0: the code path without any of it
        self.cuts_mode, self.scene_cuts = scene_cuts_form(scene_cuts)          # "off", "auto", "list"
        self.cut_threshold, self.cut_ratio = float(cut_threshold), float(cut_ratio)
        self.V = net.V
        self.tile = tile_form(tile, tile_overlap, self.V.topo)    # None (the code path without any of it) or (th, tw, overlap)
        self.ensemble = ensemble_form(ensemble, ensemble_time, self.tile)      # None (the code path without any of it) or (ensemble, time, the ops)
        if self.V.denoise and sigma is None:
            raise ValueError("sigma is required by the denoise variants (the noise level of the footage, in 8-bit code values)")
        self.sigma_clamp = check_clamp(sigma_clamp)
        # "fixed" (a number: the code path without any of the rest), "auto", "list"; a PerWindow unless "auto"
        self.sigma_mode, self.sigma = sigma_form(sigma)
        if self.sigma_mode != "fixed" and not self.V.denoise:
            raise ValueError(f"sigma={'auto' if self.sigma_mode == 'auto' else 'a per-window list'!r} is for the denoise variants; {type(net).__name__} "
                             "of a deblur variant takes no noise level")
        self.sigma_estimator = sigma_estimator_form(sigma_estimator, self.sigma_mode)      # "spatial": the code path without any of the rest
        self.sigma_motion = sigma_motion_form(sigma_motion, self.sigma_estimator)      # None: the code path without any of the rest
        if noise_model is not None and not self.V.denoise:
            raise ValueError(f"noise_model is for the denoise variants; {type(net).__name__} of a deblur variant takes no noise level")
        # None (the code path without any of the rest), "level", "list" (a PerWindow)
        self.nlf_mode, self.nlf = noise_model_form(noise_model)
        if self.nlf_mode == "level" and self.sigma_mode != "auto":
            raise ValueError("noise_model='level' estimates the curve beside the flat estimate: it needs sigma='auto'")
        # "full" (None: the code path without any of the rest), "auto", "fixed" (one rectangle), "list"; judged against the stream in _prepare
        self.picture_mode, self.picture = picture_form(picture)
        self.bar_level = float(bar_level)
        if not (self.bar_level >= 0.0):                            # refuses NaN as well
            raise ValueError(f"bar_level must be >= 0, got {bar_level!r}")
        p = next(net.parameters())
        self.dev, self.dtype = p.device, p.dtype
        if self.dev.type != "cuda":
            raise ValueError("VideoRestorer needs the module on a HIP device")
        # the parts (restore_parts.py), each None where its feature is off: they are given what was parsed above
        self.noise = NoiseLevel(self.sigma_mode, self.sigma, self.sigma_estimator, self.sigma_motion, self.nlf_mode, self.nlf,
                                self.sigma_clamp) if self.V.denoise else None
        self.report_part = Report(self.report_edge, self.report_motion, self.V.denoise, self.report_quality) if self.report else None
        self.tiles = Tiles(torch, net, self.dev, self.tile) if self.tile is not None else None
        self.ensemble_part = Ensemble(torch, net, self.dev, self.dtype, self.ensemble,
                                      plane=self.noise is not None and not self.noise.flat) if self.ensemble is not None else None
        self.overlap = Overlap(torch, self.dev, self.window_overlap) if self.window_overlap else None
        self.add_noise, self.add_noise_seed = add_noise_form(add_noise, add_noise_seed)      # None: the code path without any of it; or the 16 knots
        self.add_blur, self.add_blur_gamma = add_blur_form(add_blur, add_blur_gamma)          # None: the code path without any of it; or the taps
        if self.add_blur is not None and self.add_noise is not None:
            raise ValueError("add_blur together with add_noise: no network here was trained on both, pick one")
        # None: the code path without any of it; or R
        self.deflicker, self.deflicker_chroma = deflicker_form(deflicker, deflicker_chroma, self.add_noise, self.add_blur)
        # None: the code path without any of it; or T
        self.despot, self.despot_support, self.despot_grow, self.despot_chroma, self.despot_max_share = despot_form(
            despot, despot_support, despot_grow, despot_chroma, despot_max_share, self.add_noise, self.add_blur)
        grain_mode, grain_value, *grain_rest = grain_form(grain, grain_size, grain_chroma, grain_seed)      # None: the code path without any of it
        if grain_mode is not None and self.view is not None:
            raise ValueError(f"grain together with view={self.view!r}: the view is not the restored stream, there is nothing to put grain back on")
        if grain_mode == "auto" and not self.V.denoise:
            raise ValueError(f"grain='auto' is a share of the noise level a window was restored with; {type(net).__name__} of a deblur variant takes none: "
                             "give grain a number or 16 knots")
        self.grain_part = Grain(grain_mode, grain_value, *grain_rest) if grain_mode is not None else None
        self._shape = None
        self._reset()

    def _reset(self) -> None:
        """The per-run state: everything one restore() records, and the ``stats`` it fills while it runs."""
        self.run = _Run()
        self.stats = {"frames": 0, "windows": 0, "forward_s": 0.0, "window_forward_ms": []}

    # -- per-shape state: two slots of staging and device buffers, sized for the largest window -------------------------------------
    def _prepare(self, fmt, h: int, w: int) -> None:
        torch = self.torch
        key = (fmt.bits, fmt.chroma, fmt.matrix, fmt.range, h, w)
        ofmt = plan_output(fmt, self.out_format)[0]               # fmt itself unless another bit depth or chroma layout is written
        if self.picture_mode in ("fixed", "list"):                # the rectangles are judged against this stream, as read and as written
            from .picture import check_pictures, smallest_picture
            listed = self.picture_mode == "list"
            pics = check_pictures(self.picture if listed else [self.picture], fmt, h, w, smallest_picture(self.V.topo), out_fmt=ofmt)
            self._pics = PerWindow("picture", pics if listed else pics[0], listed)
        if self._shape == key:
            return
        self._shape = key
        self.fmt, self.h, self.w = fmt, h, w
        self.ofmt, self.convert = ofmt, ofmt is not fmt
        self.hp, self.wp = padded_size(h, w, self.V.topo)
        self.fb, self.ofb = fmt.frame_bytes(h, w), ofmt.frame_bytes(h, w)
        tin, tout = self.one_len + PAST + FUTURE, self.one_len
        dev = self.dev
        self.slots = [_Slot(torch, dev, self.dtype, tin, tout, self.fb, self.ofb, self.hp * self.wp) for _ in range(2)]
        # a picture in another format than was read: the window's whole frames as float32 on their way from one format to the other (main stream only)
        # ... and a mix in another format than was read: the same conversion gives the input side of the mix, one buffer of payloads per slot
        # ... and so does a report: the input side of its difference
        ref = self.convert and (self.mix is not None or self.report)
        self.conv32 = torch.empty(tout * 3 * h * w, dtype=torch.float32, device=dev) if self.convert and (self.picture_mode != "full" or ref) else None
        for s in self.slots:
            s.dev_ref = torch.empty((tout, self.ofb), dtype=torch.uint8, device=dev) if ref else None
        self.s_in, self.s_out = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        if self.picture_mode == "auto":
            for s in self.slots:
                s.sums = _Stat(torch, dev, "picture", tin, [(h,), (w,)])
        if self.noise is not None:
            self.noise.prepare(torch, dev, self.dtype, fmt, h, w, tin, self.slots)
        if self.report_part is not None:
            self.report_part.prepare(torch, dev, ofmt, h, w, tout, self.slots)
        if self.tiles is not None:
            self.tiles.prepare(tout, self.hp, self.wp)
        if self.ensemble_part is not None:
            self.ensemble_part.prepare(tin, tout, self.hp, self.wp)
        if self.overlap is not None:
            self.overlap.prepare(self.hp, self.wp, self.slots)
        if self.grain_part is not None:
            self.grain_part.prepare(torch, dev, ofmt, h, w)

    def _size(self, rect) -> Tuple[int, int, int, int]:
        """(h, w, padded h, padded w) of what a window with picture ``rect`` feeds the network."""
        h, w = (self.h, self.w) if rect is None else (rect[3], rect[2])
        return (h, w) + padded_size(h, w, self.V.topo)

    def _views(self, slot: _Slot, t: int, rect):
        """The window's input tensors [1, t, 3, hp, wp]: views of the slot's flat buffers."""
        _, _, hp, wp = self._size(rect)
        n = t * 3 * hp * wp
        return slot.x[:n].view(1, t, 3, hp, wp), (slot.x32[:n].view(1, t, 3, hp, wp) if slot.x32 is not None else None)

    def _window_picture(self):
        """The picture the caller gave for the window about to be staged (None: the full frame, which is also where "auto" starts from)."""
        run = self.run
        rect = self._pics.at(run.staged) if self.picture_mode in ("fixed", "list") else None
        run.staged += 1
        return rect

    # -- the steps of one window; the slot is slots[k % 2] -------------------------------------------------------------------------
    def _stage(self, slot: _Slot, frames: Sequence[np.ndarray], t0: int = 0, head: int = 0, written=None) -> int:
        """Host frames -> pinned slot -> device -> RGB tensors, on the side stream.  Windows are staged in the order they are restored.
        t0: the number of the window's first restored frame in its clip (the dither's frame number).  head, written: under ``window_overlap`` the frames
        the window shares with its predecessor and the frames it writes (None: all it restores)."""
        from .io_edges import ingest_yuv, rowcol_sums_yuv
        torch, run = self.torch, self.run
        t = len(frames)
        rect = self._window_picture()
        slot.t0, slot.head, slot.written = t0, head, written
        if slot.used:
            slot.ev_h2d.synchronize()                            # the copy that last read this pinned slot has finished
        pin = slot.pin_in.numpy()
        for i, f in enumerate(frames):
            pin[i] = f
        n_gt = self._take_gt(slot, (t - PAST - FUTURE) if written is None else written)
        with torch.cuda.stream(self.s_in):
            if slot.used:
                self.s_in.wait_event(slot.ev_done)               # the forward that last read this slot's tensors has finished
            payloads = slot.dev_in[:t]
            payloads.copy_(slot.pin_in[:t], non_blocking=True)
            if n_gt:                                             # behind the same events as dev_in: ev_h2d frees the pinned twin, ev_ready orders the report's reads
                slot.dev_gt[:n_gt].copy_(slot.pin_gt[:n_gt], non_blocking=True)
            slot.ev_h2d.record(self.s_in)
            if self.picture_mode == "auto":
                # the sums of the payloads just uploaded; this thread waits for the event behind their copy to the host -- the side stream's own
                # work, never the device and never the stream the forward runs on -- because the rectangle shapes everything staged from here on
                from .picture import decide_picture, smallest_picture
                slot.sums.launch(t, run, lambda rows, cols: rowcol_sums_yuv(payloads, self.fmt, self.h, self.w, out_rows=rows, out_cols=cols))
                began = time.perf_counter()
                rows, cols = slot.sums.wait(t)
                run.picture_wait_ms.append((time.perf_counter() - began) * 1e3)
                rect = decide_picture(rows, cols, self.fmt, self.h, self.w, self.bar_level, smallest_picture(self.V.topo), out_fmt=self.ofmt)
            slot.rect = rect
            x, x32 = self._views(slot, t, rect)
            hp, wp = x.shape[3], x.shape[4]
            if self.noise is not None:
                self.noise.stage(slot.noise, payloads, rect, run)
            ingest_yuv(payloads, self.fmt, self.h, self.w, hp, wp, self.dtype, out=x, rect=rect)
            if x32 is not None:
                ingest_yuv(payloads, self.fmt, self.h, self.w, hp, wp, torch.float32, out=x32, rect=rect)
            slot.ev_ready.record(self.s_in)
        return t

    def _take_gt(self, slot: _Slot, n: int) -> int:
        """The truth for the n frames the window being staged will write, from the run's ``gt`` into the slot's pinned buffer -> n (0 without ``gt``).
        Every frame is written once and in order, so the next n payloads of ``gt`` are theirs; the pinned buffer is free (``_stage`` has waited for ev_h2d)."""
        run = self.run
        if run.gt is None:
            return 0
        pin = slot.pin_gt.numpy()
        for i in range(n):
            try:
                f = next(run.gt)
            except StopIteration:
                raise ValueError(f"gt ended early: it has no payload for frame {run.gt_taken} of the stream written") from None
            f = np.asarray(f, dtype=np.uint8).reshape(-1)
            if f.size != self.ofb:
                raise ValueError(f"gt: frame {run.gt_taken} is a payload of {f.size} bytes, the format written and the size say {self.ofb}")
            pin[i] = f
            run.gt_taken += 1
        return n

    def _forward(self, x, x32, nm, crop=None):
        """The one call of the network: x [1, t, 3, hp, wp], x32 its float32 twin or None, nm the noise plane [1, t, 1, hp, wp] or None (the deblur
        variants take none) -> float32 [t - 4, 3, hp, wp].  crop: a tile's index into those tensors; the network is given contiguous crops, and of a flat
        noise level its stride-0 expansion cut to the tile's shape, which copies nothing."""
        if crop is not None:
            x, x32 = x[crop].contiguous(), (x32[crop].contiguous() if x32 is not None else None)
            if nm is not None:
                nm = nm[crop] if self.noise.flat else nm[crop].contiguous()
        args = (x,) if nm is None else (x, nm)
        return self.net.forward_fp32_out(*args, **({"shortcut": x32} if x32 is not None else {}))

    def _input_as_written(self, slot: _Slot, n: int, rect, tiled: bool):
        """The window's own n input frames (not the reflected ones around them) in the format written, on the device: the payloads read, or with another
        format out the whole frames converted by the two edges, float32 between them, rounded to nearest -- into the slot's reference buffer where a mix or
        a report reads them again after dev_out has been written, straight into dev_out where only the samples outside a picture are wanted (main stream)."""
        from .io_edges import egress_yuv, ingest_yuv
        read = slot.dev_in[PAST:PAST + n]
        if not self.convert or (slot.dev_ref is None and rect is None):      # as read; or nothing asks
            return read
        full = self.conv32[:n * 3 * self.h * self.w].view(1, n, 3, self.h, self.w)
        ingest_yuv(read, self.fmt, self.h, self.w, self.h, self.w, self.torch.float32, out=full)
        own = egress_yuv(full[0], self.ofmt, self.h, self.w, dst=(slot.dev_out if slot.dev_ref is None else slot.dev_ref)[:n])
        if tiled and slot.dev_ref is not None and rect is not None:
            # a tiled window's mix and report take the rectangle as the whole picture, as everything else of it does: inside the rectangle their
            # input side is the rectangle converted as the cropped stream's frames are -- chroma from the rectangle's own clamped neighbours, not from
            # the bars'.  The float32 buffer is free again: the egress that read it lies ahead on this stream
            part = self.conv32[:n * 3 * rect[3] * rect[2]].view(1, n, 3, rect[3], rect[2])
            ingest_yuv(read, self.fmt, self.h, self.w, rect[3], rect[2], self.torch.float32, out=part, rect=rect)
            egress_yuv(part[0], self.ofmt, self.h, self.w, dst=own, rect=rect)
        return own

    def _run(self, slot: _Slot, t: int, main) -> int:
        """Forward + egress on the main stream, copy back on the output stream -> the frames the window wrote."""
        from .io_edges import egress_yuv
        torch, run = self.torch, self.run
        n = t - PAST - FUTURE
        level = self.noise.level(slot.noise, t, run) if self.noise is not None else None
        rect = slot.rect
        run.window_picture.append(rect)
        with torch.cuda.stream(main), torch.no_grad():
            main.wait_event(slot.ev_ready)
            if slot.used:
                main.wait_event(slot.ev_d2h)                     # the copy that last read this slot's device payloads has finished
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(main)
            x, x32 = self._views(slot, t, rect)
            hp, wp = x.shape[3], x.shape[4]
            # the plane from the payloads the ingest read (ev_ready lies behind their upload; they stay until ev_done)
            nm = self.noise.plane(slot.dev_in[:t], rect, hp, wp, level, run) if self.noise is not None else None
            out = self.tiles.forward(lambda crop: self._forward(x, x32, nm, crop), n, hp, wp, run) if self.tiles is not None else None
            tiled = out is not None                              # a window whose plan is one tile takes the path of tile=None
            if self.ensemble_part is not None:                   # never with tiles: the members' mean in place of the one forward
                out = self.ensemble_part.forward(x, x32, nm, n, hp, wp, run)
            elif not tiled:
                out = self._forward(x, x32, nm)
            e1.record(main)
            run.timers.append((e0, e1))
            if self.overlap is not None:
                # the shared frames cross-faded with the predecessor's, the window's own tail kept for the successor; from here on the window is the
                # frames it writes
                self.overlap.step(slot, out, slot.head, slot.written, rect, self._size(rect), run)
                n = slot.written
                out = out[:n]
            own = self._input_as_written(slot, n, rect, tiled)
            written = slot.dev_out[:n]
            if rect is not None and (slot.dev_ref is not None or not self.convert):
                # everything outside the picture leaves as it came in (as converted, in another format; converted frames that nothing reads again are
                # in dev_out already): the egress below writes the inside only
                written.copy_(own, non_blocking=True)
            dither = None if self.dither is None else (self.dither_seed, slot.t0)
            egress_yuv(out, self.ofmt, self.h, self.w, dst=written, rect=rect, dither=dither, mix=self.mix, ref=own if self.mix is not None else None)
            if self.grain_part is not None:                      # in place, ahead of everything that describes the stream written
                self.grain_part.launch(written, rect, slot.t0, level, run)
            if self.report_part is not None:
                self.report_part.launch(slot.report, own, written, rect, run, gt=slot.dev_gt[:n] if run.gt is not None else None)
            slot.ev_done.record(main)
        with torch.cuda.stream(self.s_out):
            self.s_out.wait_event(slot.ev_done)
            slot.pin_out[:n].copy_(slot.dev_out[:n], non_blocking=True)
            slot.ev_d2h.record(self.s_out)
        slot.used = True
        return n

    def _collect(self, slot: _Slot, n: int) -> List[np.ndarray]:
        slot.ev_d2h.synchronize()
        run = self.run
        if self.report_part is not None:
            self.report_part.collect(slot.report, n, run)
        if self.overlap is not None:
            self.overlap.collect(slot, run)
        run.collected += 1
        return list(slot.pin_out[:n].numpy().copy())

    def _finish_stats(self) -> None:
        run, stats = self.run, self.stats
        ms = [a.elapsed_time(b) for a, b in run.timers]          # every event has completed: the last copy back has been waited for
        stats["window_forward_ms"] = ms
        stats["forward_s"] = sum(ms) / 1e3
        stats["windows"] = len(ms)
        stats["noise_launches"] = 0                              # the deblur variants estimate nothing; NoiseLevel.finish counts its own
        stats["window_picture"] = list(run.window_picture)
        stats["picture_launches"] = run.launches["picture"]
        if self.picture_mode == "auto":
            stats["picture_wait_ms"] = list(run.picture_wait_ms)
        for part in (self.noise, self.report_part, self.tiles, self.ensemble_part, self.overlap, self.grain_part):
            if part is not None:
                part.finish(run, stats)
        if self.add_noise is not None:
            stats["add_noise"], stats["add_noise_seed"], stats["degrade_launches"] = list(self.add_noise), self.add_noise_seed, run.launches["degrade"]
        if self.add_blur is not None:
            stats["add_blur"], stats["add_blur_gamma"], stats["blur_launches"] = self.add_blur, self.add_blur_gamma, run.launches["blur"]
        if self.deflicker is not None:
            stats["deflicker"], stats["deflicker_chroma"], stats["deflicker_launches"] = self.deflicker, self.deflicker_chroma, run.launches["deflicker"]
            stats["frame_deflicker"] = [tuple(f) for f in run.frame_deflicker]
        if self.despot is not None:
            stats["despot"], stats["despot_support"], stats["despot_grow"] = self.despot, self.despot_support, self.despot_grow
            stats["despot_chroma"], stats["despot_max_share"], stats["despot_launches"] = self.despot_chroma, self.despot_max_share, run.launches["despot"]
            stats["frame_despot"] = [tuple(f) for f in run.frame_despot]
        src = run.src
        if self.scene_cuts is not None:                          # its thread has ended: the stream has been read to its end
            stats["cuts"] = list(src.cuts)
            if self.cuts_mode == "auto":
                stats["cut_measure"] = list(src.decider.detector.m)
                stats["thumb_frames"], stats["thumb_launches"] = src.decider.frames, run.launches["thumb"]
            else:
                stats["cuts_ignored"] = [c for c in src.decider.all if c >= (src.n or 0)]

    def _source(self, frames: Iterable[np.ndarray]) -> _SceneFrames:
        """The frame source of one restore(): what says where the scenes start is all that differs."""
        from .scenes import ListedCuts
        if self.cuts_mode == "auto":
            decider = _DeviceThumbs(self.torch, self.dev, self.fmt, self.h, self.w, self.one_len + PAST + FUTURE + 4, self.cut_threshold, self.cut_ratio,
                                    self.run)
        else:
            decider = ListedCuts(self.scene_cuts or ())
        self.run.src = _SceneFrames(frames, decider)
        return self.run.src

    # -- drivers -------------------------------------------------------------------------------------------------------------------
    def restore(self, frames: Iterable[np.ndarray], fmt, height: int, width: int, gt=None, degraded=None, deflickered=None,
                despotted=None) -> Iterator[np.ndarray]:
        """frames: iterable of uint8 payloads (``fmt.frame_bytes(height, width)`` each) -> the restored payloads, in order.  gt: None, or an iterable of
        ground-truth payloads in the format WRITTEN and of the stream's size, frame i the truth of written frame i (needs ``report=True``; see the class).
        degraded: None, or a callable that is given every payload ``add_noise`` or ``add_blur`` makes of ``frames``, in order, on the thread that reads
        ``frames`` (needs one of the two).  deflickered: the same for the payloads ``deflicker`` makes of ``frames`` (needs it).  despotted: the same for
        the payloads ``despot`` hands on (needs it): with ``deflicker`` they are made of the deflickered ones."""
        torch = self.torch
        if gt is not None and self.report_part is None:
            raise ValueError("gt adds PSNR and SSIM against the truth to the report: it needs report=True")
        option = "add_noise" if self.add_noise is not None else ("add_blur" if self.add_blur is not None else None)
        if gt is not None and option is not None:
            raise ValueError(f"{option} makes the clean frames the truth of the report: not together with gt")
        if degraded is not None and option is None:
            raise ValueError("degraded is given the payloads add_noise or add_blur makes: it needs one of them")
        if deflickered is not None and self.deflicker is None:
            raise ValueError("deflickered is given the payloads deflicker makes: it needs deflicker")
        if despotted is not None and self.despot is None:
            raise ValueError("despotted is given the payloads despot hands on: it needs despot")
        self._prepare(fmt, height, width)
        if option is not None and self.report_part is not None and self.convert:
            raise ValueError(f"{option} with report and out_format={self.out_format!r}, another format than the input's: the clean frames, the truth of "
                             "the report, would have to be converted")
        self._reset()
        stage = None
        if self.add_noise is not None:
            stage = _DeviceDegrade(torch, self.dev, fmt, height, width, self.one_len, self.add_noise, self.add_noise_seed, self.report_part is not None,
                                   self.run)
        elif self.add_blur is not None:
            stage = _DeviceBlur(torch, self.dev, fmt, height, width, self.one_len, self.add_blur, self.add_blur_gamma,
                                self.scene_cuts if self.cuts_mode == "list" else None, self.report_part is not None, self.run)
        if stage is not None and self.report_part is not None:
            gt = stage.truth()
        if self.deflicker is not None:                           # not a degraded copy: no truth comes of it, and gt stays what the caller gave
            stage = _DeviceDeflicker(torch, self.dev, fmt, height, width, self.one_len, self.deflicker, self.deflicker_chroma,
                                     self.scene_cuts if self.cuts_mode == "list" else None, self.run)
            degraded = deflickered
        despot_stage = None
        if self.despot is not None:                              # behind deflicker, each on a stream of its own: flicker reads as spikes, so it goes first
            despot_stage = _DeviceDespot(torch, self.dev, fmt, height, width, self.one_len, self.despot, self.despot_support, self.despot_grow,
                                         self.despot_chroma, self.despot_max_share, self.scene_cuts if self.cuts_mode == "list" else None, self.run)
        if gt is not None:
            self.run.gt = iter(gt)
            for s in self.slots:                                 # once per stream shape, and only for a run that asks
                if s.pin_gt is None:
                    s.pin_gt = torch.empty((self.one_len, self.ofb), dtype=torch.uint8).pin_memory()
                    s.dev_gt = torch.empty((self.one_len, self.ofb), dtype=torch.uint8, device=self.dev)
            self.report_part.prepare_gt(torch, self.dev, self.one_len, self.slots)
        for slot in self.slots:
            slot.used = False
        if self.overlap is not None:
            self.overlap.reset()
        self.stats["out_format"], self.stats["dither"], self.stats["dither_seed"] = (self.out_format if self.convert else None), self.dither, self.dither_seed
        self.stats["amount"], self.stats["view"] = self.amount, self.view
        main = torch.cuda.current_stream(self.dev)

        def checked(it):
            for f in it:
                f = np.asarray(f, dtype=np.uint8).reshape(-1)
                if f.size != self.fb:
                    raise ValueError(f"frame payload of {f.size} bytes, the format and size say {self.fb}")
                yield f

        def windows():
            """(the slot, the frames, their first restored frame's number in its clip, the frames shared with the predecessor, the frames written) of
            every window, in the order they are restored."""
            feed = checked(frames) if stage is None else stage.frames(checked(frames), degraded)
            src = self._source(feed if despot_stage is None else despot_stage.frames(feed, despotted))
            for k, win, clip_lo in src.windows(self.one_len, self.window_overlap):
                yield self.slots[k % 2], win, clip_lo, src.head, src.written

        if not self.pipeline:
            with torch.cuda.device(self.dev):
                for slot, win, *marks in windows():
                    n = self._run(slot, self._stage(slot, win, *marks), main)
                    for p in self._collect(slot, n):
                        self.stats["frames"] += 1
                        yield p
                self._finish_stats()
            return

        # Three threads besides the kernels: the stager reads frames and brings window k + 1 onto the device (side stream), the forward
        # thread runs window k (its range-guard check waits for the device, so nothing else may depend on this thread), and the caller's
        # thread takes window k - 1 out of the pinned buffer.  Streams order the device work with events; the semaphores only say that
        # the event a stream is about to wait for HAS been recorded (in slots) and that a pinned output slot has been emptied (out slots).
        in_free = {slot: threading.Semaphore(1) for slot in self.slots}
        out_free = {slot: threading.Semaphore(1) for slot in self.slots}
        halt = threading.Event()

        def acquire(sem) -> bool:
            while not halt.is_set():
                if sem.acquire(timeout=0.1):
                    return True
            return False

        def stage_loop(put):
            with torch.cuda.device(self.dev):
                for slot, win, *marks in windows():
                    if not acquire(in_free[slot]) or not put((slot, self._stage(slot, win, *marks))):
                        return

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


if __name__ == "__main__":
    sys.exit(main())
