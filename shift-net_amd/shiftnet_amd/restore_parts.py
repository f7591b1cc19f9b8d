"""The optional features of the video restorer (shiftnet_amd/restore.py), one class each: ``NoiseLevel`` (what a window's noise level is and how it is
obtained), ``Report`` (the method-noise report), ``Tiles`` (the forward in overlapping tiles), ``Ensemble`` (the forward on mirrored, transposed
and time-reversed copies), ``Overlap`` (windows that overlap in time, their shared frames cross-faded) and ``Grain`` (grain put back on the payloads
written).  A part owns everything of its feature -- its state per
slot on the device and in pinned memory, its launches, its host arithmetic and its keys of ``stats`` -- and writes into the one record of a
``restore()`` (``restore._Run``) that ``VideoRestorer`` hands it; ``VideoRestorer`` holds each part or None and calls it by name.  The parts are given
parsed values (windows.py's ``*_form`` functions) and validate nothing.  ``_Stat`` and ``_Vectors`` are what they share."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .noise import (NLF_BANDS, clip_codes, combine_sigma, frame_sigma, frames_median, motion_grid, motion_summary, nbins, nlf_bins, pair_bins, pair_sigma,
                    window_curve, window_curve_pairs, window_sigma, window_sigma_temporal)
from .report import frames_report, frames_report_motion, summarize, summarize_motion, summarize_quality
from .windows import overlap_weights, plan_tiles


class _Stat:
    """A statistic of the payloads a window has uploaded, made on the device and read on the host: the device tensor or tensors (``rows`` leading
    rows each, for the largest window), their pinned twins and the event behind the copies.  ``launch`` and ``wait`` may be on different threads;
    the waiting one waits for that event -- the launching stream's own work, never the device and never the stream the forward runs on."""

    def __init__(self, torch, dev, name: str, rows: int, shapes, dtype=None) -> None:
        dtype = torch.uint32 if dtype is None else dtype
        self.name = name                                         # of its launch counter in _Run.launches
        self.dev = [torch.empty((rows,) + tuple(s), dtype=dtype, device=dev) for s in shapes]
        self.pin = [torch.empty((rows,) + tuple(s), dtype=dtype).pin_memory() for s in shapes]
        self.event = torch.cuda.Event()

    def launch(self, t: int, run: "_Run", kernel) -> None:
        """``kernel(the first t rows of every device tensor)`` on the current stream, their copies to the host behind it, the event behind those."""
        kernel(*(d[:t] for d in self.dev))
        for p, d in zip(self.pin, self.dev):
            p[:t].copy_(d[:t], non_blocking=True)
        self.event.record()
        run.launches[self.name] += 1

    def wait(self, t: int) -> List[np.ndarray]:
        self.event.synchronize()
        return [p[:t].numpy() for p in self.pin]


def _picture_size(rect, h: int, w: int) -> Tuple[int, int]:
    """(h, w) of a window's picture: the rectangle's, or the frame's."""
    return (h, w) if rect is None else (rect[3], rect[2])


class _Vectors:
    """The block vectors (``sn_yuv_block_motion``) of the largest window's ``pairs`` pairs at the full frame's grid, flat: int8 vectors and uint32 SADs
    on the device.  A window's are views of the leading elements at the grid of its picture.  ``stat``: the name of a ``_Stat`` that brings the
    vectors to the host as well (None: they stay on the device)."""

    def __init__(self, torch, dev, pairs: int, h: int, w: int, stat=None) -> None:
        blocks = max(pairs * int(np.prod(motion_grid(h, w))), 1)
        self.stat = _Stat(torch, dev, stat, 2 * blocks, [()], torch.int8) if stat is not None else None
        self.mv = self.stat.dev[0] if stat is not None else torch.empty(2 * blocks, dtype=torch.int8, device=dev)
        self.sad = torch.empty(blocks, dtype=torch.uint32, device=dev)

    def views(self, p: int, h: int, w: int):
        """(int8 [p, gy, gx, 2], uint32 [p, gy, gx]) for a window of p pairs and a picture of h x w."""
        gy, gx = motion_grid(h, w)
        return self.mv[:2 * p * gy * gx].view(p, gy, gx, 2), self.sad[:p * gy * gx].view(p, gy, gx)


# ---- the noise level ------------------------------------------------------------------------------------------------------------------
class _NoiseState:
    """What a slot holds for ``sigma="auto"``: the ``_Stat``s of the window's histograms (None where the mode needs none) and its vectors."""

    def __init__(self, torch, dev, part: "NoiseLevel", bits: int, h: int, w: int, tin: int) -> None:
        temporal, level = part.estimator != "spatial", part.nlf_mode == "level"
        self.hist = _Stat(torch, dev, "noise", tin, [(nbins(bits),)])
        self.bands = _Stat(torch, dev, "nlf", tin, [(NLF_BANDS, nlf_bins(bits))]) if level else None
        self.pairs = _Stat(torch, dev, "noise_pairs", tin - 1, [(pair_bins(bits),)]) if temporal else None      # tin frames are tin - 1 pairs
        self.pair_bands = _Stat(torch, dev, "nlf_pairs", tin - 1, [(NLF_BANDS, nlf_bins(bits))]) if temporal and level else None
        self.vectors = _Vectors(torch, dev, tin - 1, h, w, stat="motion") if part.motion is not None else None
        self.grid = (0, 0)                                       # the vector blocks of the window the slot holds


class NoiseLevel:
    """What a window's noise level is and how it is obtained (the denoise variants; every ``sigma`` mode).

    Noise level (``sigma``): a number, a list with one number per window, or ``"auto"``: a blind estimate per window from
    histograms of the luma's 2 x 2 Haar HH coefficient, made on the device from the payloads the window has uploaded anyway
    (``sn_yuv_noise_hist``, shiftnet_amd/noise.py).  ``sigma_estimator="temporal"`` / ``"min"`` adds the same statistic of the difference of consecutive
    input frames (``sn_yuv_noise_hist_pairs``), in which texture that does not move cancels, and uses it alone or the lower of the two.
    ``sigma_motion="blocks"`` lets that difference follow the picture: one integer vector per 16 x 16 luma block and pair, found on the device
    (``sn_yuv_block_motion``), so that a pan no longer reads as noise.

    Noise model (``noise_model``, off by default): sensor noise is signal dependent, the shadows of R'G'B' carry more of it than the
    highlights.  ``"level"`` estimates per window a noise-level function -- sigma against the luma code, 16 knots -- from the same histograms split by
    brightness (``sn_yuv_noise_hist_bands``) and writes the network's noise plane per pixel from it (``sn_noise_map_level``), in place of one level everywhere.

    ``stage`` runs on the side stream, ``level`` on the thread that runs the forward (it waits for the events of ``stage``'s copies), ``plane`` on
    the main stream.  ``flat``: the plane is one number everywhere, a stride-0 expansion of one element."""

    def __init__(self, sigma_mode: str, sigma, estimator: str = "spatial", motion=None, nlf_mode=None, nlf=None, clamp=(0.0, 50.0)) -> None:
        self.sigma_mode, self.sigma, self.estimator, self.motion, self.nlf_mode, self.nlf, self.clamp = sigma_mode, sigma, estimator, motion, nlf_mode, nlf, clamp
        self.flat = nlf_mode is None
        if estimator != "spatial":                               # the statistic of the pairs: at the same place, or along the window's vectors
            from . import io_edges as E
            self.pair_hist = E.noise_hist_pairs_yuv if motion is None else E.noise_hist_pairs_mv_yuv
            self.pair_band_hist = E.noise_hist_pairs_bands_yuv if motion is None else E.noise_hist_pairs_bands_mv_yuv

    def prepare(self, torch, dev, dtype, fmt, h: int, w: int, tin: int, slots) -> None:
        """Per stream shape: the clip codes, and per slot the statistics of the largest window (``slot.noise``; None unless ``sigma="auto"``)."""
        self.torch, self.dev, self.dtype, self.fmt, self.h, self.w = torch, dev, dtype, fmt, h, w
        self.lo, self.hi = clip_codes(fmt.bits, fmt.range)
        self.codes = (fmt.bits, fmt.matrix, fmt.range)           # what the host arithmetic of noise.py asks of the format
        for s in slots:
            s.noise = _NoiseState(torch, dev, self, fmt.bits, h, w, tin) if self.sigma_mode == "auto" else None

    def stage(self, st, payloads, rect, run) -> None:
        """The histograms of the payloads just uploaded (current stream: the side stream), ahead of the ingest so that they are on the host long before
        ``level`` asks.  The pinned twins are free: ``level`` read them on the host before the slot was handed back to the stager."""
        if st is None:
            return
        from .io_edges import block_motion_yuv, noise_hist_bands_yuv, noise_hist_yuv
        t = payloads.shape[0]
        head, kw = (payloads, self.fmt, self.h, self.w), dict(lo=self.lo, hi=self.hi, rect=rect)
        st.hist.launch(t, run, lambda out: noise_hist_yuv(*head, out=out, **kw))
        along = head
        if st.vectors is not None:
            # the vectors of the t - 1 pairs, once per window and ahead of the histograms that follow them; their copy to the host is for stats alone
            size = _picture_size(rect, self.h, self.w)
            st.grid = motion_grid(*size)
            mv, sad = st.vectors.views(t - 1, *size)
            st.vectors.stat.launch(mv.numel(), run, lambda out: block_motion_yuv(*head, rect=rect, out_mv=mv, out_sad=sad))
            along = head + (mv,)
        if st.pairs is not None:                                 # the statistic of the t - 1 pairs of consecutive payloads (t >= 5: a window has 4 neighbours)
            st.pairs.launch(t - 1, run, lambda out: self.pair_hist(*along, out=out, **kw))
        if st.bands is not None:                                 # the same statistic by brightness band, from the same payloads, behind it
            st.bands.launch(t, run, lambda out: noise_hist_bands_yuv(*head, out=out, **kw))
        if st.pair_bands is not None:
            st.pair_bands.launch(t - 1, run, lambda out: self.pair_band_hist(*along, out=out, **kw))

    def level(self, st, t: int, run):
        """(sigma, curve) of the window about to run: the noise level in 8-bit codes, and the noise-level function (16 knots, sigma of 8-bit R'G'B';
        None without ``noise_model``).  Windows run in the order they are handed out.  What the window used is recorded only after it was obtained."""
        if self.sigma_mode == "auto":
            hist, = st.hist.wait(t)
            per = [frame_sigma(hist[i], *self.codes) for i in range(t)]
            run.window_frame_sigma.append(per)
            if self.estimator == "spatial":
                sigma = window_sigma(per, self.clamp)
            else:
                pairs, = st.pairs.wait(t - 1)
                ps = [pair_sigma(pairs[i], *self.codes) for i in range(t - 1)]
                spatial, temporal = frames_median(per), window_sigma_temporal(ps)
                run.window_pair_sigma.append(ps)
                run.window_sigma_spatial.append(spatial)
                run.window_sigma_temporal.append(temporal)
                if st.vectors is not None:
                    gy, gx = st.grid
                    flat, = st.vectors.stat.wait(2 * (t - 1) * gy * gx)
                    run.window_pair_motion.append(motion_summary(flat.reshape(t - 1, gy, gx, 2)))
                sigma = combine_sigma(spatial, temporal, self.estimator, self.clamp)
        else:
            sigma = self.sigma.at(len(run.window_sigma))
        run.window_sigma.append(sigma)
        if self.nlf_mode is None:
            return sigma, None
        if self.nlf_mode == "level":
            bands, = st.bands.wait(t)
            if self.estimator == "spatial":
                curve = window_curve(bands, *self.codes, self.clamp)
            else:
                pair_bands, = st.pair_bands.wait(t - 1)
                curve = window_curve_pairs(bands, pair_bands, *self.codes, self.estimator, self.clamp)
        else:
            curve = list(self.nlf.at(len(run.window_nlf)))
        run.window_nlf.append(curve)
        return sigma, curve

    def plane(self, payloads, rect, hp: int, wp: int, level, run):
        """What the network is given as its second argument (current stream: the main stream), [1, t, 1, hp, wp]: the plane of the window's curve from
        the payloads the ingest read -- the knots are a kernel argument -- or ``sigma / 255`` everywhere."""
        sigma, curve = level
        t = payloads.shape[0]
        if curve is None:
            return self.torch.full((1, 1, 1, 1, 1), sigma / 255.0, dtype=self.dtype, device=self.dev).expand(1, t, 1, hp, wp)
        from .io_edges import noise_map_level
        nm = noise_map_level(payloads, self.fmt, self.h, self.w, hp, wp, [c / 255.0 for c in curve], self.dtype, self.lo, self.hi, rect=rect)
        run.launches["nlf_map"] += 1
        return nm

    def finish(self, run, stats) -> None:
        stats["noise_launches"] = run.launches["noise"] + run.launches["motion"]      # "motion" stays 0 without sigma_motion
        if self.nlf_mode is not None:
            stats["window_nlf"] = [list(c) for c in run.window_nlf]
            stats["nlf_launches"], stats["nlf_map_launches"] = run.launches["nlf"], run.launches["nlf_map"]
        stats["window_sigma"] = list(run.window_sigma)
        if self.sigma_mode == "auto":
            stats["window_frame_sigma"] = [list(p) for p in run.window_frame_sigma]
        if self.estimator != "spatial":
            stats["sigma_estimator"] = self.estimator
            stats["window_sigma_spatial"], stats["window_sigma_temporal"] = list(run.window_sigma_spatial), list(run.window_sigma_temporal)
            stats["window_pair_sigma"] = [list(p) for p in run.window_pair_sigma]
            stats["noise_pairs_launches"] = run.launches["noise_pairs"]
            if self.nlf_mode == "level":
                stats["nlf_pairs_launches"] = run.launches["nlf_pairs"]
            if self.motion is not None:
                stats["sigma_motion"] = self.motion
                stats["window_pair_motion"] = [list(p) for p in run.window_pair_motion]


# ---- the method-noise report ------------------------------------------------------------------------------------------------------------
def _niqe_shape(h: int, w: int) -> Tuple[int, ...]:
    """What ``sn_yuv_niqe_sums`` writes per frame of a picture of h x w luma samples: (2 scales, nbh, nbw whole 96 x 96 blocks, 5 maps, 5 sums)."""
    from .lib import SN_NIQE_BLOCK, SN_NIQE_MAPS, SN_NIQE_SUMS
    return (2, h // SN_NIQE_BLOCK, w // SN_NIQE_BLOCK, SN_NIQE_MAPS, SN_NIQE_SUMS)


class _ReportState:
    """What a slot holds for the report: the ``_Stat`` of the sums of written minus input of the window's own frames (one row per frame the window
    writes), under ``report_motion`` that of the sums of the written pairs along their vectors (one row per pair) and those vectors, and under
    ``report_quality`` those of the NIQE sums of the input and of the written frames."""

    def __init__(self, torch, dev, motion, quality, h: int, w: int, tout: int) -> None:
        from .lib import SN_DIFF_STATS, SN_DIFF_STATS_MV
        self.sums = _Stat(torch, dev, "report", tout, [(SN_DIFF_STATS,)], torch.int64)
        self.pair_sums = _Stat(torch, dev, "report_mv", max(tout - 1, 1), [(SN_DIFF_STATS_MV,)], torch.int64) if motion is not None else None
        self.vectors = _Vectors(torch, dev, tout - 1, h, w) if motion is not None else None
        # report_quality: the NIQE sums of the window's input and written frames, flat and sized for the full frame's blocks; a window's are views of
        # the leading elements at the grid of its picture (one _Stat each: each is one launch)
        words = max(tout * int(np.prod(_niqe_shape(h, w))), 1)
        self.niqe_in = _Stat(torch, dev, "report_quality", words, [()], torch.float64) if quality is not None else None
        self.niqe_out = _Stat(torch, dev, "report_quality", words, [()], torch.float64) if quality is not None else None
        self.truth = None                                        # restore(gt=...): a _TruthState, made by Report.prepare_gt for a run that asks


class _TruthState:
    """What a slot holds for a report against a ground-truth stream: the ``_Stat``s of the difference sums (one row per written frame) and of the SSIM
    tile sums (flat and sized for the full frame's tiles; a window's are views of the leading elements at the grid of its picture) of the pairs
    (truth, input as written) and (truth, written).  One _Stat each: each is one launch."""

    def __init__(self, torch, dev, h: int, w: int, tout: int) -> None:
        from .io_edges import ssim_tiles
        from .lib import SN_DIFF_STATS
        words = tout * int(np.prod(ssim_tiles(h, w)))
        self.sums = [_Stat(torch, dev, "fullref", tout, [(SN_DIFF_STATS,)], torch.int64) for _ in range(2)]
        self.ssim = [_Stat(torch, dev, "fullref", words, [()], torch.float64) for _ in range(2)]


class Report:
    """Method-noise report (``report``, off by default): numbers about what the run changed, per written frame -- whether input minus output is white in
    space, independent from frame to frame, no stronger on edges than elsewhere, and as strong as the sigma the window was restored with.  Exact integer
    sums of the two sets of payloads the window holds on the device anyway once the egress has run (``sn_yuv_diff_stats``), float64 on the host
    (shiftnet_amd/report.py).  It changes no byte written.  What the numbers mean on real footage nobody has validated.  ``report_motion="blocks"`` adds the
    temporal correlation of that difference along the motion of the written picture (``sn_yuv_block_motion`` on the frames written, then
    ``sn_yuv_diff_stats_mv``): removed detail that moves with a pan reads as uncorrelated at the same place, and as correlated along its vector.

    ``report_quality="niqe"`` adds a number about the pictures themselves, which the difference cannot give: NIQE (shiftnet_amd/niqe.py) of the luma of every
    input frame and of the frame written for it, in the format written.  Two more launches behind the report's own (``sn_yuv_niqe_sums`` on ``own`` and
    on ``written``, the same rectangle); the fit of the blocks and the distance are float64 on the host, in ``collect``.  A picture with fewer than two
    whole 96 x 96 blocks has no score: nan.  No threshold and no verdict; unvalidated on real footage.

    ``restore(gt=...)`` compares with a ground-truth stream, which neither of the above can: PSNR of Y, U and V and the luma's SSIM of every input frame
    and of the frame written for it against the truth's frame, all in the format written (shiftnet_amd/fullref.py).  Four more launches behind the others:
    ``sn_yuv_diff_stats`` of (truth, ``own``) and (truth, ``written``) with edge 0, whose exact sums give PSNR, and ``sn_yuv_ssim_sums`` of the same two
    pairs, on the same rectangle.  **Luma SSIM only; the truth must be in the format written and frame-aligned by the caller; no verdict.**

    ``launch`` runs on the main stream behind the egress, ``collect`` on the thread that hands the window's frames out."""

    def __init__(self, edge: float, motion, denoise: bool, quality=None) -> None:
        self.edge, self.motion, self.denoise, self.quality = edge, motion, denoise, quality      # quality: None or niqe.load_params' (mu, cov, win7)

    def prepare(self, torch, dev, ofmt, h: int, w: int, tout: int, slots) -> None:
        """Per stream shape: the format written, the edge rule in its codes, and per slot the sums of the largest window (``slot.report``)."""
        self.ofmt, self.h, self.w = ofmt, h, w
        self.code_edge = int(round(self.edge * (1 << (ofmt.bits - 8))))
        if self.quality is not None:                             # the window's taps, float32 on the device
            self.win7 = torch.from_numpy(np.ascontiguousarray(self.quality[2], dtype=np.float32)).to(dev)
        for s in slots:
            s.report = _ReportState(torch, dev, self.motion, self.quality, h, w, tout)

    def prepare_gt(self, torch, dev, tout: int, slots) -> None:
        """For a run with ``gt``: per slot the sums against the truth of the largest window (``slot.report.truth``), made once per stream shape."""
        for s in slots:
            if s.report.truth is None:
                s.report.truth = _TruthState(torch, dev, self.h, self.w, tout)

    def launch(self, st, own, written, rect, run, gt=None) -> None:
        """Written minus input, the window's own n frames of both still on the device (current stream: the main stream); ``collect`` reads the sums.
        gt: None, or the truth's n payloads for the frames written, on the device in the format written."""
        from .io_edges import block_motion_yuv, diff_stats_mv_yuv, diff_stats_yuv
        n = written.shape[0]
        head = (own, written, self.ofmt, self.h, self.w)
        st.sums.launch(n, run, lambda sums: diff_stats_yuv(*head, rect=rect, edge=self.code_edge, out_sums=sums))
        if st.pair_sums is not None and n >= 2:
            # the vectors of the n - 1 pairs of the frames written (the clean picture), then d of both frames of every pair along them
            mv, sad = st.vectors.views(n - 1, *_picture_size(rect, self.h, self.w))
            block_motion_yuv(written, self.ofmt, self.h, self.w, rect=rect, out_mv=mv, out_sad=sad)
            run.launches["report_motion"] += 1
            st.pair_sums.launch(n - 1, run, lambda sums: diff_stats_mv_yuv(*head, mv, rect=rect, out_sums=sums))
        if self.quality is not None:
            from .io_edges import niqe_sums_yuv
            shape = (n,) + _niqe_shape(*_picture_size(rect, self.h, self.w))
            if shape[2] * shape[3]:                              # a picture without a whole block: nothing to launch, and no score
                for stat, payloads in ((st.niqe_in, own), (st.niqe_out, written)):
                    stat.launch(int(np.prod(shape)), run,
                                lambda flat, p=payloads: niqe_sums_yuv(p, self.ofmt, self.h, self.w, self.win7, rect=rect, out=flat.view(shape)))
        if gt is not None:
            # the truth against the input as written and against the frames written: the exact sums PSNR is made of, then the SSIM tile sums
            from .io_edges import ssim_sums_yuv, ssim_tiles
            shape = (n,) + ssim_tiles(*_picture_size(rect, self.h, self.w))
            for k, payloads in enumerate((own, written)):
                st.truth.sums[k].launch(n, run, lambda sums, p=payloads: diff_stats_yuv(gt, p, self.ofmt, self.h, self.w, rect=rect, edge=0, out_sums=sums))
            for k, payloads in enumerate((own, written)):
                st.truth.ssim[k].launch(int(np.prod(shape)), run,
                                        lambda flat, p=payloads: ssim_sums_yuv(gt, p, self.ofmt, self.h, self.w, rect=rect, out_sums=flat.view(shape)))

    def collect(self, st, n: int, run) -> None:
        """The sums of the window being handed out.  Windows are handed out in the order they ran: ``run.window_sigma`` and ``run.window_picture`` have
        this one's entry at ``run.collected``."""
        sums, = st.sums.wait(n)
        run.frame_sums += [[int(v) for v in row] for row in sums]
        run.frame_window += [run.collected] * n
        run.frame_sigma += [run.window_sigma[run.collected] if self.denoise else None] * n
        if st.pair_sums is not None:                             # frame i carries the pair (i, i + 1); a window's last frame has none
            pairs = [[int(v) for v in row] for row in st.pair_sums.wait(n - 1)[0]] if n >= 2 else []
            run.pair_sums_mv += pairs + [None]
            run.frame_size += [_picture_size(run.window_picture[run.collected], self.h, self.w)] * n
        if self.quality is not None:
            from .niqe import frame_score
            shape = (n,) + _niqe_shape(*_picture_size(run.window_picture[run.collected], self.h, self.w))
            if shape[2] * shape[3]:
                a, b = (stat.wait(int(np.prod(shape)))[0].reshape(shape) for stat in (st.niqe_in, st.niqe_out))
                run.frame_niqe += [(frame_score(a[i], *self.quality[:2]), frame_score(b[i], *self.quality[:2])) for i in range(n)]
            else:
                run.frame_niqe += [(float("nan"), float("nan"))] * n
        if run.gt is not None:
            from .fullref import frame_fullref
            from .io_edges import ssim_tiles
            h, w = _picture_size(run.window_picture[run.collected], self.h, self.w)
            shape = (n,) + ssim_tiles(h, w)
            (si,), (so,) = (stat.wait(n) for stat in st.truth.sums)
            ti, to = (stat.wait(int(np.prod(shape)))[0].reshape(shape) for stat in st.truth.ssim)
            run.frame_fullref += [frame_fullref(si[i], so[i], ti[i], to[i], self.ofmt.bits, h, w) for i in range(n)]

    def finish(self, run, stats) -> None:
        bits = self.ofmt.bits
        stats["frame_sums"] = [list(r) for r in run.frame_sums]
        stats["frame_report"] = frames_report(run.frame_sums, run.frame_window, run.frame_sigma, bits, self.ofmt.matrix, self.ofmt.range)
        stats["report_summary"] = summarize(stats["frame_report"])
        stats["report_launches"] = run.launches["report"]
        if self.motion is not None:
            stats["report_motion"] = self.motion
            stats["pair_sums_mv"] = [None if r is None else list(r) for r in run.pair_sums_mv]
            stats["frame_report_motion"] = frames_report_motion(run.pair_sums_mv, bits, run.frame_size)
            stats["report_motion_summary"] = summarize_motion(stats["frame_report_motion"])
            stats["report_motion_launches"] = run.launches["report_motion"] + run.launches["report_mv"]
        if self.quality is not None:
            stats["report_quality"] = "niqe"
            stats["frame_niqe"] = list(run.frame_niqe)
            stats["report_quality_summary"] = summarize_quality(run.frame_niqe)
            stats["report_quality_launches"] = run.launches["report_quality"]
        if run.gt is not None:
            from .fullref import summarize_fullref
            stats["frame_fullref"] = list(run.frame_fullref)
            stats["fullref_summary"] = summarize_fullref(run.frame_fullref)
            stats["fullref_launches"] = run.launches["fullref"]


# ---- tiles ----------------------------------------------------------------------------------------------------------------------------
class Tiles:
    """Tiles (``tile``, ``tile_overlap``; off by default): the network's activations grow with the pixels of the frames it is given, and a large frame does
    not fit the device at any useful window length.  With a tile size the forward -- and only the forward -- runs on overlapping rectangles of the
    window's frames, one after the other, and their float32 results are added into one float32 canvas with feather weights (``sn_tile_accumulate``,
    csrc/sn_tile.hip; the plan is windows.plan_tiles); everything before and after still works on the whole picture.  **A tiled result is not the
    full-frame result**: every channel-attention layer pools over the map it is given, so it sees the tile, and the receptive field is cut at tile edges.
    The feather turns a mismatch into a gradient instead of an edge; it does not remove it."""

    def __init__(self, torch, net, dev, tile) -> None:
        self.torch, self.net, self.dev, self.tile = torch, net, dev, tile      # tile: (th, tw, overlap)
        self.plans = {}                                          # (hp, wp) -> (the plan, its weight tables on the device)
        self.canvas = None

    def prepare(self, tout: int, hp: int, wp: int) -> None:
        """Per stream shape: the float32 canvas the tiles' results are added into, flat and sized for the full frame as the slots' tensors are.  One for
        the restorer (main stream only): the egress of a window has consumed it before the next window's forward runs."""
        self.canvas = self.torch.empty(tout * 3 * hp * wp, dtype=self.torch.float32, device=self.dev)

    def plan(self, hp: int, wp: int):
        """(windows.plan_tiles for a padded picture of hp x wp, its weight tables [n_y][th] and [n_x][tw] on the device), made once per size."""
        key = (int(hp), int(wp))
        if key not in self.plans:
            plan = plan_tiles(key[0], key[1], *self.tile)
            to_dev = lambda a: self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)      # noqa: E731
            self.plans[key] = (plan, to_dev(plan.wy), to_dev(plan.wx))
        return self.plans[key]

    def forward(self, forward, n: int, hp: int, wp: int, run):
        """The forward of one window tile by tile (current stream): ``forward(crop)`` is the network's float32 result [n, 3, th, tw] on the crop
        (a 5-d index) of the window's tensors -> the float32 canvas [n, 3, hp, wp]; None where the window's plan is one tile, which takes the path of
        ``tile=None``."""
        from .io_edges import tile_accumulate
        plan, wy, wx = self.plan(hp, wp)
        run.window_tiles.append(list(plan.tiles))
        if plan.single:
            return None
        canvas = self.canvas[:n * 3 * hp * wp].view(n, 3, hp, wp)
        for _ in range(2):      # one range-guard check for the window's tiles (no device sync between them); a tripped guard moved the module to the
            canvas.zero_()      # two-kernel chain: run them once more, into a canvas that starts at zero again
            with self.net.guard_scope() as gs:
                for i, y0 in enumerate(plan.ys):
                    for j, x0 in enumerate(plan.xs):
                        crop = (slice(None), slice(None), slice(None), slice(y0, y0 + plan.th), slice(x0, x0 + plan.tw))
                        tile_accumulate(forward(crop), canvas, wy[i], wx[j], y0, x0)
                        run.launches["tile"] += 1
            if not gs.tripped:
                break
        return canvas

    def finish(self, run, stats) -> None:
        stats["tile"], stats["tile_overlap"] = self.tile[:2], self.tile[2]
        stats["window_tiles"] = [list(w) for w in run.window_tiles]
        stats["tile_launches"] = run.launches["tile"]


# ---- the self-ensemble ----------------------------------------------------------------------------------------------------------------
class Ensemble:
    """Self-ensemble (``ensemble``, ``ensemble_time``; off by default): the forward -- and only the forward -- of every window runs on M copies of the
    window's tensors, mirrored, transposed and reversed in time (shiftnet_amd/ensemble.py); every float32 result is mapped back and added into one
    float32 canvas, which the last launch divides by M (``sn_geo_transform``, ``sn_geo_accumulate``; csrc/sn_geo.hip).  Everything before and after
    works as without it.  **A window costs M forwards.  Nobody has measured what the ensemble gains on this network.**"""

    def __init__(self, torch, net, dev, dtype, form, plane: bool) -> None:
        from .ensemble import Buffers
        self.torch, self.net, self.dev, self.dtype = torch, net, dev, dtype
        self.ensemble, self.time, self.members = form            # windows.ensemble_form's
        self.plane = plane                                       # the noise level is a plane (noise_model): it is transformed with the frames
        self.buffers = Buffers()
        self.canvas = None

    def prepare(self, tin: int, tout: int, hp: int, wp: int) -> None:
        """Per stream shape: the members' input buffers and the float32 canvas, flat and sized for the full frame as the slots' tensors are (a
        ``picture`` only makes the views smaller, at the same addresses).  One set for the restorer (main stream only)."""
        torch, px = self.torch, hp * wp
        self.buffers.reserve(torch, "x", tin * 3 * px, self.dtype, self.dev)
        if self.dtype != torch.float32:
            self.buffers.reserve(torch, "shortcut", tin * 3 * px, torch.float32, self.dev)
        if self.plane:
            self.buffers.reserve(torch, "plane", tin * px, self.dtype, self.dev)
        self.canvas = torch.empty(tout * 3 * px, dtype=torch.float32, device=self.dev)

    def forward(self, x, x32, nm, n: int, hp: int, wp: int, run):
        """The forward of one window member by member (current stream): x [1, t, 3, hp, wp], x32 its float32 twin or None, nm the noise plane or
        level or None -> the float32 canvas [n, 3, hp, wp]."""
        from .ensemble import forward_ensemble
        canvas = self.canvas[:n * 3 * hp * wp].view(n, 3, hp, wp)
        return forward_ensemble(self.net, x, nm, x32, self.members, out=canvas, buffers=self.buffers, counts=run.launches)

    def finish(self, run, stats) -> None:
        stats["ensemble"], stats["ensemble_time"], stats["ensemble_members"] = self.ensemble, self.time, list(self.members)
        stats["ensemble_launches"] = {"transform": run.launches["geo_transform"], "accumulate": run.launches["geo_accumulate"]}


# ---- windows that overlap in time -------------------------------------------------------------------------------------------------------
class Overlap:
    """Windows that overlap in time (``window_overlap`` = V; off by default): every window runs through the network on its own, and the network restores
    a window's last frames with less temporal context than the first frames of the next window, and each window with its own sigma, noise curve and
    channel-attention pools -- the result can step at every window boundary.  With V > 0 consecutive windows of a scene share V frames (the plan is
    windows.plan_scene_overlap_windows); the older window's float32 answer for them is kept in one carry buffer and the newer window's is cross-faded
    with it, a linear ramp in time (``sn_time_crossfade``, csrc/sn_time.hip; windows.overlap_weights).  The same launch sums, exactly, the squared
    difference of the two answers before the blend: ``seam_rms``, how far a window's edge is from the next window's interior.  **A window still costs one
    forward, and there are one_len / (one_len - V) times as many.  The cross-fade blends two different answers: a mismatch becomes a ramp over V
    frames, it is not removed.**

    ``step`` runs on the main stream behind the forward, ``collect`` on the thread that hands the window's frames out.  One carry for the restorer: the
    forward, the cross-fade and the egress of all windows run on the main stream, in window order."""

    NONE = object()                                              # the carry holds no window's tail

    def __init__(self, torch, dev, overlap: int) -> None:
        self.torch, self.dev, self.V = torch, dev, overlap
        w_prev, w_cur = overlap_weights(overlap)
        self.w_prev, self.w_cur = torch.from_numpy(w_prev).to(dev), torch.from_numpy(w_cur).to(dev)
        self.carry = None
        self.held = self.NONE                                    # the picture rectangle (None: the full frame) of the window whose tail the carry holds

    def prepare(self, hp: int, wp: int, slots) -> None:
        """Per stream shape: the carry, flat and sized for the full frame as the slots' tensors are, and per slot the sums of a seam (``slot.seam``)."""
        self.carry = self.torch.empty(self.V * 3 * hp * wp, dtype=self.torch.float32, device=self.dev)
        for s in slots:
            s.seam = _Stat(self.torch, self.dev, "overlap", self.V, [(3,)], self.torch.int64)
            s.seam_size = None

    def reset(self) -> None:
        self.held = self.NONE

    def step(self, slot, out, head: int, written: int, rect, size, run) -> None:
        """The window's float32 result ``out`` [n, 3, hp, wp] (current stream: the main stream): its first ``head`` frames cross-faded in place with the
        predecessor's last, where the carry holds them at the same picture rectangle -- with another rectangle the shapes differ, the shared frames stay
        this window's alone and the seam has no statistic --, then its own last V frames into the carry if it writes only ``written`` < n of them."""
        from .io_edges import time_crossfade
        V, n = self.V, out.shape[0]
        h, w, hp, wp = size
        carry = self.carry[:V * 3 * hp * wp].view(V, 3, hp, wp)
        slot.seam_size = None
        if head and self.held is not self.NONE and self.held == rect:
            slot.seam.launch(V, run, lambda sq: time_crossfade(carry, out[:V], self.w_prev, self.w_cur, h, w, sq=sq.zero_()))
            slot.seam_size = (h, w)
        if written < n:
            carry.copy_(out[n - V:])
            self.held = rect
        else:
            self.held = self.NONE
        run.window_written.append(written)

    def collect(self, slot, run) -> None:
        """The seam of the window being handed out: None, or per shared frame, oldest first, the rms difference of the two answers in 8-bit R'G'B' code
        units, ``255 * sqrt(sum over the planes of sq / (2^32 * 3 * h * w))``."""
        if slot.seam_size is None:
            run.seam_rms.append(None)
            return
        h, w = slot.seam_size
        sq, = slot.seam.wait(self.V)
        run.seam_rms.append([seam_rms([int(v) for v in row], h, w) for row in sq])

    def finish(self, run, stats) -> None:
        stats["window_overlap"] = self.V
        stats["window_written"] = list(run.window_written)
        stats["seam_rms"] = [None if s is None else list(s) for s in run.seam_rms]
        stats["overlap_launches"] = run.launches["overlap"]


# ---- grain put back on the stream written ------------------------------------------------------------------------------------------------
class Grain:
    """Grain put back (``grain``; off by default): a fully denoised picture looks waxy and bands, and the usual delivery chain is "denoise, encode,
    re-grain".  Behind every window's egress one launch (``sn_yuv_grain``, csrc/sn_grain.hip; main stream) adds a spatially correlated Gaussian field
    to the window's written payloads IN PLACE, inside the window's rectangle under ``picture``: luma, and chroma at ``grain_chroma`` times the level.
    The level is a curve of 16 knots at the written luma code, in the unit of ``sigma`` (the sigma of i.i.d. noise on 8-bit R'G'B' whose luma part
    the grain equals): the knots given, or under ``"auto"`` the share times what THIS window was restored with -- ``NoiseLevel.level``'s sigma as 16
    equal knots, or its curve under ``noise_model``.  The field is keyed by the dither's frame number, so the bytes do not depend on how the windows
    are run.  Everything behind it -- the report, ``gt``, NIQE -- describes the stream with the grain.  **A Gaussian field of a size the user chooses,
    not a model fitted to the removed noise** (shiftnet_amd/grain.py states the limits).

    ``launch`` runs on the main stream between the egress and the report."""

    def __init__(self, mode: str, value, size: float, chroma: float, seed: int) -> None:
        from .grain import grain_taps
        self.mode, self.value, self.size, self.chroma, self.seed = mode, value, size, chroma, seed
        self.taps = grain_taps(size)
        if mode == "auto":
            self.how = "auto:%g" % value
        else:
            self.how = "level %g" % value[0] if min(value) == max(value) else "a curve, %g at black .. %g at white" % (value[0], value[-1])
        self.gauss = None

    def prepare(self, torch, dev, ofmt, h: int, w: int) -> None:
        """Per stream shape: the format written and, once, the table on the device."""
        self.ofmt, self.h, self.w = ofmt, h, w
        if self.gauss is None:
            from .degrade import gauss_table
            self.gauss = torch.from_numpy(gauss_table().copy()).to(dev)

    def knots(self, level) -> List[float]:
        """The 16 knots of the window whose ``NoiseLevel.level`` is ``level``, in 8-bit R'G'B' code units."""
        if self.mode != "auto":
            return list(self.value)
        sigma, curve = level
        return [self.value * k for k in (curve if curve is not None else [sigma] * NLF_BANDS)]

    def launch(self, written, rect, t0: int, level, run) -> None:
        """``written``: the window's payloads as the egress left them (current stream: the main stream), grained in place; t0: the dither's frame number."""
        from .io_edges import grain_yuv
        knots = self.knots(level)
        run.window_grain.append(knots)
        grain_yuv(written, self.ofmt, self.h, self.w, knots, self.taps, self.chroma, self.seed, t0, self.gauss, rect=rect, out=written)
        run.launches["grain"] += 1

    def finish(self, run, stats) -> None:
        stats["grain"] = self.how if self.mode == "auto" else list(self.value)
        stats["grain_size"], stats["grain_chroma"], stats["grain_seed"] = self.size, self.chroma, self.seed
        stats["window_grain"] = [list(k) for k in run.window_grain]
        stats["grain_launches"] = run.launches["grain"]


def seam_rms(sq, h: int, w: int) -> float:
    """The sums of ``sn_time_crossfade`` of one shared frame's planes -> the rms difference in 8-bit code units (the sums are of (d * 65536)^2)."""
    import math
    return 255.0 * math.sqrt(sum(sq) / (2.0 ** 32 * len(sq) * h * w))
