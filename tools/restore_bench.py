#!/usr/bin/env python3
"""Measurements behind DESIGN.md 3.11, 3.13, 3.14, 3.15, 3.16, 3.17, 3.19, 3.20, 3.21, 3.23, 3.25, 3.29, 3.33 and 3.38 (run on the MI355X from the repository root).

  kernels : time per pixel of sn_ingest_yuv / sn_egress_yuv / sn_yuv_thumb / sn_yuv_noise_hist (4:2:0 8 bit, 720p x 20 frames; the noise
            histogram on the same frames with noise of sigma 10 as well) beside sn_ingest_u8 / sn_egress_u8 on the same
            frames, interleaved in one process: REPS repetitions, each timing INNER back-to-back launches of every kernel with device events;
            median and min..max over the repetitions.  Since 3.16 also the dithered egress (sn_egress_yuv_dither) from float32 at 8 bit 4:2:0,
            10 bit 4:2:0 and 10 bit 4:4:4 beside the undithered egress of the same formats, and with --parent_lib SO the undithered sn_egress_yuv
            of another build on the same tensors.  Since 3.19 also the mixed egress (sn_egress_yuv_mix, amount (0.5, 0.5)) from float32 at 8 bit
            4:2:0 and 10 bit 4:4:4, dithered and not, and the removed view at 8 bit 4:2:0, beside the plain egress of the same formats.  Since 3.20
            also sn_yuv_noise_hist_pairs on the payloads of the noise histogram (20 frames are 19 pairs).
  pipeline: steady-state wall time per 720p window of the pipelined restorer (Shift-Net-s, one_len 16, bf16, Y4M held in memory) beside the
            forward-only time of the same windows (device events in the same runs) and beside pipeline=False, the two alternating.
            --scene_cuts auto: the same stream with the cut detector running (sn_yuv_thumb; 3.13).  --cut_every N: every second scene of N frames
            is inverted, so that the stream has a cut every N frames; with --scene_cuts off / auto / listed.
  sigma   : steady-state wall time per 720p window of the pipelined denoiser (Shift-Net-s denoise, one_len 16, bf16) with sigma=10.0 and with
            sigma="auto" (sn_yuv_noise_hist per window; 3.14), and since 3.20 with sigma="auto", sigma_estimator="min" (sn_yuv_noise_hist_pairs on
            top), runs of the three alternating in one process, the first two windows left out.
  picture : the active picture (3.15) on a 1920 x 1080 stream whose picture is (0, 138, 1920, 804), bars at black.  --mode forward: steady-state
            forward time per window of the pipelined restorer (Shift-Net-s, one_len 16, bf16, Y4M held in memory) with picture=None and with
            picture="auto" (or --picture fixed), runs of the two alternating in one process, the first two windows left out, beside the wall time
            per window and the time the stager waits for the sums.  --mode kernels: time per pixel of sn_ingest_yuv / sn_egress_yuv on a 1080p and
            on an 804-row stream beside the _rect entry points with the whole-frame rectangle and with the picture's, and sn_yuv_rowcol_sums beside
            sn_yuv_thumb on the same payloads, interleaved as in the kernels part; --parent_lib SO adds the two entry points of another build.
  nlf     : the noise-level function (3.17).  --mode kernels: time per launch of sn_yuv_noise_hist_bands and sn_noise_map_level (-> bf16) beside
            sn_yuv_noise_hist and sn_ingest_yuv on the same payloads (4:2:0 8 bit, 720p x 20 frames, a blurred clip and the same with noise of sigma 10),
            interleaved as in the kernels part; since 3.20 also sn_yuv_noise_hist_pairs and sn_yuv_noise_hist_pairs_bands.  --mode forward: steady-state wall time per 720p window of the pipelined denoiser (as the sigma part)
            with sigma="auto" alone and with noise_model="level" on top, runs of the two alternating in one process, the first two windows left out.
  report  : the method-noise report (3.21).  --mode kernels: time per launch of sn_yuv_diff_stats (4:2:0 8 bit, 720p x 16 frames: a noisy clip against its
            clean twin, edge 16) beside sn_egress_yuv from float32 and sn_yuv_noise_hist_pairs on the same frames, interleaved as in the kernels part;
            since 3.26 also sn_yuv_diff_stats_mv with the matcher's vectors and with all-zero vectors, and sn_yuv_block_motion on the written payloads.
            --mode forward: steady-state wall time per 720p window of the pipelined denoiser (as the sigma part, sigma=10.0) with report=False, with
            report=True and with report_motion="blocks" on top, runs of the three alternating in one process, the first two windows left out.
  motion  : the motion-compensated temporal estimate (3.23).  --mode kernels: time per launch of sn_yuv_block_motion, sn_yuv_noise_hist_pairs_mv and
            sn_yuv_noise_hist_pairs_bands_mv beside the two plain pair histograms (4:2:0 8 bit, 720p x 20 frames with noise of sigma 10), interleaved as
            in the kernels part.  --mode forward: steady-state wall time per 720p window of the pipelined denoiser (as the sigma part) with
            sigma_estimator="min" alone and with sigma_motion="blocks" on top, runs of the two alternating in one process, the first two windows left out.
            Since 3.25, --mode kernels of the nlf and motion parts with --parent_lib SO: the seven noise-histogram entry points of this build and, twice, of
            another build through one ctypes argument list, at 8 bit and 10 bit 4:2:0, with this build's median against the other's third quartile.
  tiles   : the tiled restorer (3.29).  --mode forward: steady-state forward time per window and frames/s of the restorer (Shift-Net-s, one_len 16, bf16,
            --size HxW, default 720x1280) for every --tile form given (``full``, ``N`` or ``HxW``; repeat the option) at --tile_overlap, runs of the forms
            alternating in one process, the first window of every run left out, and beside the times ``torch.cuda.max_memory_allocated()`` of every run
            (the allocator's cache emptied and the peak reset before it; the engine keeps the buffers of the sizes it has seen, so the peak of a form is
            clean only in a process that runs that form alone: give one --tile).  --mode quality: max and rms of |tiled - full| of the written samples
            (10 bit 4:4:4 out, in 8-bit code units) at --size (default 256x384) with 2 x 2 tiles for overlaps 0, 16, 32 and 64.
  overlap : windows that overlap in time (3.31).  --mode forward: steady-state forward time per window and frames/s end to end of the restorer (Shift-Net-s,
            one_len 16, bf16, 720p, --windows times 16 frames) for every --overlap V given (repeat the option), runs of the forms alternating in one
            process, the first window of every run left out.  --mode kernels: ``sn_time_crossfade`` on V = 4 frames of 720p, with and without the
            statistic, beside a plain device copy of one such tensor, interleaved; bytes per second at 12 bytes per sample (8 for the copy); each also
            ``_cold``: on six sets of tensors taken in turn, more than the Infinity Cache holds.
  quality : the no-reference score of the report (3.33).  --mode kernels: time per launch of ``sn_yuv_niqe_sums`` (4:2:0 8 bit, 720p x 16 frames with noise
            of sigma 10) beside a plain device copy of the same frames' luma planes -- the kernel reads every luma plane once per scale -- and beside
            sn_yuv_diff_stats on the same frames, interleaved as in the kernels part; and the host's milliseconds per frame for the fit and the
            distance (niqe.frame_score on those sums).  --mode forward: steady-state wall time per 720p window of the pipelined denoiser (as the report
            part) with report=True alone and with report_quality="niqe" on top, runs of the two alternating in one process, the first two windows left out.
  fullref : the report's comparison with a ground-truth stream (3.34).  --mode kernels: time per launch of ``sn_yuv_ssim_sums`` (4:2:0 8 bit, 720p x 16
            frames: a clean clip against its copy with noise of sigma 10) beside a plain device copy of the luma planes of both sets -- the bytes the
            kernel reads, once -- and beside sn_yuv_diff_stats on the same frames, interleaved as in the kernels part.  --mode forward: steady-state wall
            time per 720p window of the pipelined denoiser (as the report part) with report=True alone and with gt= on top, runs of the two alternating in
            one process, the first two windows left out.
  degrade : --mode kernels: sn_yuv_degrade on 16 frames of 1280 x 720 at 8-bit 4:2:0 (both sitings) and at 10-bit 4:4:4 beside sn_egress_yuv from float32
            and a plain device copy of the same payloads, and sn_yuv_blur at n = 1, 7, 15 with and without gamma tables (16 - 2r outputs from the 16
            sources), interleaved; microseconds per launch and TB/s of each case's own bytes.  --mode forward: the
            stream restored with add_noise=10 and report=True against the same stream degraded beforehand and restored with the clean one as gt.
  grain   : --mode kernels: sn_yuv_grain on 16 frames of 1280 x 720 at 8-bit 4:2:0, size 0 and 0.8, chroma share 0 and 0.5, out of place and in place,
            beside a plain device copy of the same payloads and sn_yuv_degrade, interleaved; microseconds per launch and TB/s of each case's own bytes
            (3.38).  --mode forward: steady-state wall time per 720p window of the pipelined denoiser (as the sigma part, sigma=10.0) without grain and
            with grain="auto:0.5" at size 0.8 and chroma share 0.5, runs of the two alternating in one process, the first two windows left out.
  deflicker : --mode kernels: sn_yuv_code_hist and sn_yuv_apply_lut on 16 frames of 1280 x 720 at 8-bit and 10-bit 4:2:0, each on a NOISY clip and on a
            FLAT one (every luma sample one code: the histogram's worst case), beside a plain device copy of the same payloads and sn_yuv_degrade,
            interleaved; microseconds per launch, TB/s of each case's own bytes and the histogram's flat-to-noisy ratio (3.39).  --mode forward:
            steady-state wall time per 720p window of the pipelined deblurrer without and with deflicker=3 on a stream whose luma flickers by +-8 %,
            runs of the two alternating in one process, the first two windows left out.
  despot  : --mode kernels: sn_yuv_despot (chroma follow and off) on the 14 frames of 16 payloads of 1280 x 720 that have two neighbours, and the two
            sn_yuv_block_motion launches that make its vectors, at 8-bit and 10-bit 4:2:0, beside a plain device copy of the 16 payloads,
            interleaved; microseconds per call and TB/s of each case's own bytes (3.40).  --mode forward: steady-state wall time per 720p window
            of the pipelined deblurrer without and with despot=24, runs of the two alternating in one process, the first two windows left out.
Prints one JSON object per part.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from shiftnet_amd import lib as L  # noqa: E402
from shiftnet_amd import restore, synth, y4m  # noqa: E402
from shiftnet_amd.io_edges import (block_motion_yuv, noise_hist_pairs_bands_mv_yuv, noise_hist_pairs_mv_yuv, diff_stats_mv_yuv, diff_stats_yuv, egress_u8, egress_yuv, ingest_u8, ingest_yuv, noise_hist_bands_yuv, noise_hist_pairs_bands_yuv, noise_hist_pairs_yuv,  # noqa: E402
                                   noise_hist_yuv, noise_map_level, rowcol_sums_yuv, thumb_yuv, yuv_fmt)


def summary(v):
    v = sorted(v)
    return {"median": statistics.median(v), "min": v[0], "max": v[-1], "n": len(v)}


def kernels(a):
    T, H, W = 20, 720, 1280
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    u8 = torch.from_numpy(np.concatenate([blur] * 5)).cuda()                       # [20,720,1280,3]
    rgb = ingest_u8(u8, torch.float32)[0]
    pay = egress_yuv(rgb, fmt, H, W)
    out_bf, out_32 = rgb.to(torch.bfloat16), rgb
    x_bf = torch.empty((1, T, 3, H, W), dtype=torch.bfloat16, device="cuda")
    dst = torch.empty_like(pay)
    thumbs = torch.empty((T, (H + 7) // 8, (W + 7) // 8), dtype=torch.uint16, device="cuda")
    hists = torch.empty((T, 511), dtype=torch.uint32, device="cuda")
    pairs = torch.empty((T - 1, 1021), dtype=torch.uint32, device="cuda")
    pay_noisy = egress_yuv((rgb + torch.randn(rgb.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * (10.0 / 255)).clamp(0, 1), fmt, H, W)
    fmt10, fmt444 = yuv_fmt(10, L.SN_YUV_420_LEFT, L.SN_YUV_BT709, L.SN_YUV_LIMITED), yuv_fmt(10, L.SN_YUV_444, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    dst10 = torch.empty((T, fmt10.frame_bytes(H, W)), dtype=torch.uint8, device="cuda")
    dst444 = torch.empty((T, fmt444.frame_bytes(H, W)), dtype=torch.uint8, device="cuda")
    pay444 = egress_yuv(rgb, fmt444, H, W)                                           # the input side of the mix at 10 bit 4:4:4
    half, removed = ("amount", 0.5, 0.5), ("removed", 1.0, 1.0)
    parent = {}
    if a.parent_lib:                                                                 # another build's undithered egress, interleaved with this one's
        import ctypes as C
        plib = C.CDLL(os.path.abspath(a.parent_lib))
        plib.sn_egress_yuv.argtypes = [C.c_void_p, C.c_int, C.POINTER(L.YuvFmt), C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]

        def pegr(o, code, f, d):
            return lambda: L.check(plib.sn_egress_yuv(o.data_ptr(), code, f, d.data_ptr(), T, H, W, H, W, torch.cuda.current_stream().cuda_stream), "parent sn_egress_yuv")
        parent = {"parent_egress_yuv_bf16": pegr(out_bf, L.SN_BF16, fmt, dst), "parent_egress_yuv_fp32": pegr(out_32, L.SN_F32, fmt, dst),
                  "parent_egress_yuv_420p10_fp32": pegr(out_32, L.SN_F32, fmt10, dst10), "parent_egress_yuv_444p10_fp32": pegr(out_32, L.SN_F32, fmt444, dst444)}
    cases = {
        "ingest_yuv_bf16": lambda: ingest_yuv(pay, fmt, H, W, H, W, torch.bfloat16, out=x_bf),
        "thumb_yuv": lambda: thumb_yuv(pay, fmt, H, W, out=thumbs),
        "noise_hist_yuv": lambda: noise_hist_yuv(pay, fmt, H, W, out=hists),                 # a blurred clip: the mass sits in bins 0 .. 2
        "noise_hist_yuv_sigma10": lambda: noise_hist_yuv(pay_noisy, fmt, H, W, out=hists),   # spread over the first few dozen bins
        "noise_hist_pairs_yuv": lambda: noise_hist_pairs_yuv(pay, fmt, H, W, out=pairs),     # the same payloads: 20 frames, 19 pairs
        "noise_hist_pairs_yuv_sigma10": lambda: noise_hist_pairs_yuv(pay_noisy, fmt, H, W, out=pairs),
        "ingest_u8_bf16": lambda: ingest_u8(u8, torch.bfloat16),
        "egress_yuv_bf16": lambda: egress_yuv(out_bf, fmt, H, W, dst=dst),
        "egress_u8_bf16": lambda: egress_u8(out_bf),
        "egress_yuv_fp32": lambda: egress_yuv(out_32, fmt, H, W, dst=dst),
        "egress_u8_fp32": lambda: egress_u8(out_32),
        "egress_yuv_fp32_tpdf": lambda: egress_yuv(out_32, fmt, H, W, dst=dst, dither=(1, 0)),
        "egress_yuv_420p10_fp32": lambda: egress_yuv(out_32, fmt10, H, W, dst=dst10),
        "egress_yuv_420p10_fp32_tpdf": lambda: egress_yuv(out_32, fmt10, H, W, dst=dst10, dither=(1, 0)),
        "egress_yuv_444p10_fp32": lambda: egress_yuv(out_32, fmt444, H, W, dst=dst444),
        "egress_yuv_444p10_fp32_tpdf": lambda: egress_yuv(out_32, fmt444, H, W, dst=dst444, dither=(1, 0)),
        "egress_yuv_mix_fp32": lambda: egress_yuv(out_32, fmt, H, W, dst=dst, mix=half, ref=pay),
        "egress_yuv_mix_fp32_tpdf": lambda: egress_yuv(out_32, fmt, H, W, dst=dst, dither=(1, 0), mix=half, ref=pay),
        "egress_yuv_removed_fp32": lambda: egress_yuv(out_32, fmt, H, W, dst=dst, mix=removed, ref=pay),
        "egress_yuv_mix_444p10_fp32": lambda: egress_yuv(out_32, fmt444, H, W, dst=dst444, mix=half, ref=pay444),
        "egress_yuv_mix_444p10_fp32_tpdf": lambda: egress_yuv(out_32, fmt444, H, W, dst=dst444, dither=(1, 0), mix=half, ref=pay444),
        **parent,
    }
    if a.only_cases:
        cases = {k: f for k, f in cases.items() if any(w in k for w in a.only_cases.split(","))}
    for f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():                                                   # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    px = T * H * W
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "ps_per_pixel": summary([m * 1e9 / px for m in v])} for k, v in ms.items()}
    print(json.dumps({"part": "kernels", "frames": T, "size": [H, W], "reps": a.reps, "inner": a.inner, "note": "egress_u8/ingest_u8 allocate their output per call", **res}))


def pipeline(a):
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(8, H, W, seed=2)
    pay8 = egress_yuv(ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0], fmt, H, W).cpu().numpy()
    hd = y4m.Y4MHeader(width=W, height=H, chroma="420jpeg")
    buf = io.BytesIO()
    wr = y4m.Y4MWriter(buf, hd)
    for i in range(n):
        j = i % 14                                                                   # 0 .. 7, 6 .. 1: consecutive frames are always neighbours of
        p = pay8[j if j < 8 else 14 - j]                                             # the clip (a jump back from 7 to 0 would look like a cut)
        if a.cut_every and (i // a.cut_every) % 2:                                   # every second scene inverted (the luma plane: 235 + 16 - Y)
            p = p.copy()
            p[:H * W] = 251 - p[:H * W]
        wr.write(p)
    data = buf.getvalue()
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    cuts = {"off": None, "auto": "auto", "listed": list(range(a.cut_every, n, a.cut_every)) if a.cut_every else []}[a.scene_cuts]
    found = []

    def run(pipe):
        vr = restore.VideoRestorer(net, one_len, pipeline=pipe, scene_cuts=cuts)
        sink = y4m.Y4MWriter(io.BytesIO(), hd)
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(y4m.Y4MReader(io.BytesIO(data)), fmt, H, W)):
            sink.write(p)
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        found.append(vr.stats.get("cuts"))
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(a.only != "serial")                                                          # warm-up: code objects, engine buffers
    runs = {"pipelined": [], "serial": []}
    for _ in range(a.runs):
        if a.only in ("both", "pipelined"):
            runs["pipelined"].append(run(True))
        if a.only in ("both", "serial"):
            runs["serial"].append(run(False))
    res = {}
    for k, rs in runs.items():
        if not rs:
            continue
        wall = [g for r in rs for g in r["window_wall_ms"]]
        fwd = [g for r in rs for g in r["window_forward_ms"]]
        res[k] = {"window_wall_ms": summary(wall), "window_forward_ms": summary(fwd), "total_s": [round(r["total_s"], 3) for r in rs],
                  "frames_per_s_end_to_end": [round(n / r["total_s"], 2) for r in rs]}
    print(json.dumps({"part": "pipeline", "variant": "deblur_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W], "runs": a.runs,
                      "scene_cuts": a.scene_cuts, "cut_every": a.cut_every, "cuts_found": found[-1], **res}))


def sigma(a):
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(8, H, W, seed=2)
    rgb = ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0]
    g = torch.Generator("cuda").manual_seed(1)
    frames = []
    for i in range(n):                                                               # fresh noise of sigma 10 on every frame
        j = i % 14
        x = rgb[j if j < 8 else 14 - j][None]
        frames.append(egress_yuv((x + torch.randn(x.shape, device="cuda", generator=g) * (10.0 / 255)).clamp(0, 1), fmt, H, W)[0].cpu().numpy())
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    seen = {}

    def run(sig, estimator="spatial"):
        vr = restore.VideoRestorer(net, one_len, sigma=sig, pipeline=True, sigma_estimator=estimator)
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[str(sig) if estimator == "spatial" else estimator] = vr.stats["window_sigma"]
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(10.0)                                                                        # warm-up: code objects, engine buffers
    run("auto")
    run("auto", "min")
    runs = {"fixed": [], "auto": [], "auto_min": []}
    for _ in range(a.runs):
        runs["fixed"].append(run(10.0))
        runs["auto"].append(run("auto"))
        runs["auto_min"].append(run("auto", "min"))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "sigma", "variant": "denoise_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W], "runs": a.runs,
                      "window_sigma_auto": [round(s, 3) for s in seen["auto"]], "window_sigma_auto_min": [round(s, 3) for s in seen["min"]], **res}))


def hist_ab_cases(parent_lib, symbols, tag, pay, fmt, H, W, mv=None):
    """The noise-histogram entry points ``symbols`` of this build and of ANOTHER build (--parent_lib: the parent commit's whole csrc compiled into a shared
    library of its own), called through ctypes with one argument list on the same tensors, so that the builds are timed interleaved in one process
    (3.25).  The other build appears twice, as parentA_ and parentB_, with this build between them: the spread between two copies of identical code
    is the run's own noise, and what a case owes to its place after another kernel falls on one copy of either side."""
    if not parent_lib:
        return {}
    import ctypes as C
    from shiftnet_amd.noise import clip_codes
    plib, T = C.CDLL(os.path.abspath(parent_lib)), pay.shape[0]
    lo, hi = clip_codes(fmt.bits, fmt.range)
    dst = torch.empty(T * 16 * 512, dtype=torch.uint32, device="cuda")              # room for the largest of the histograms
    cases = {}
    for sym in symbols:
        rect = [] if sym == "sn_yuv_noise_hist" else [L.YuvRect(0, 0, W, H) if sym.endswith("_rect") else None]
        args = [pay.data_ptr(), fmt] + rect + ([mv.data_ptr()] if sym.endswith("_mv") else []) + [dst.data_ptr(), lo, hi, T, H, W]
        for who, lib in (("parentA", plib), ("new", L.load()), ("parentB", plib)):
            fn = getattr(lib, sym)
            fn.argtypes = getattr(L.load(), sym).argtypes
            cases[f"{who}_{sym[len('sn_yuv_'):]}{tag}"] = lambda fn=fn, args=args, sym=sym, keep=(pay, mv, dst): L.check(
                fn(*args, torch.cuda.current_stream().cuda_stream), sym)
    return cases


def hist_ab_verdict(ms):
    """Per case of ``hist_ab_cases``: this build's median against the larger third quartile of the two copies of the other build, same run."""
    out = {}
    for k, v in ms.items():
        if k.startswith("new_"):
            q3 = max(statistics.quantiles(ms[w + k[4:]], n=4, method="inclusive")[2] for w in ("parentA_", "parentB_"))
            out[k[4:]] = {"new_median_us": statistics.median(v) * 1e3, "parent_q3_us": q3 * 1e3, "ok": statistics.median(v) <= q3}
    return out


def nlf_kernels(a):
    T, H, W = 20, 720, 1280
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    rgb = ingest_u8(torch.from_numpy(np.concatenate([blur] * 5)).cuda(), torch.float32)[0]
    pay = egress_yuv(rgb, fmt, H, W)
    noisy = (rgb + torch.randn(rgb.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * (10.0 / 255)).clamp(0, 1)
    pay_noisy = egress_yuv(noisy, fmt, H, W)
    x_bf = torch.empty((1, T, 3, H, W), dtype=torch.bfloat16, device="cuda")
    nm = torch.empty((1, T, 1, H, W), dtype=torch.bfloat16, device="cuda")
    hists = torch.empty((T, 511), dtype=torch.uint32, device="cuda")
    bands = torch.empty((T, 16, 128), dtype=torch.uint32, device="cuda")
    pairs = torch.empty((T - 1, 1021), dtype=torch.uint32, device="cuda")
    pair_bands = torch.empty((T - 1, 16, 128), dtype=torch.uint32, device="cuda")
    knots = [(9.0 - 0.4 * b) / 255.0 for b in range(16)]
    cases = {
        "ingest_yuv_bf16": lambda: ingest_yuv(pay, fmt, H, W, H, W, torch.bfloat16, out=x_bf),
        "noise_hist_yuv": lambda: noise_hist_yuv(pay, fmt, H, W, out=hists),
        "noise_hist_yuv_sigma10": lambda: noise_hist_yuv(pay_noisy, fmt, H, W, out=hists),
        "noise_hist_bands_yuv": lambda: noise_hist_bands_yuv(pay, fmt, H, W, out=bands),
        "noise_hist_bands_yuv_sigma10": lambda: noise_hist_bands_yuv(pay_noisy, fmt, H, W, out=bands),
        "noise_hist_pairs_yuv": lambda: noise_hist_pairs_yuv(pay, fmt, H, W, out=pairs),     # the same payloads: 20 frames, 19 pairs
        "noise_hist_pairs_yuv_sigma10": lambda: noise_hist_pairs_yuv(pay_noisy, fmt, H, W, out=pairs),
        "noise_hist_pairs_bands_yuv": lambda: noise_hist_pairs_bands_yuv(pay, fmt, H, W, out=pair_bands),
        "noise_hist_pairs_bands_yuv_sigma10": lambda: noise_hist_pairs_bands_yuv(pay_noisy, fmt, H, W, out=pair_bands),
        "noise_map_level_bf16": lambda: noise_map_level(pay, fmt, H, W, H, W, knots, torch.bfloat16, out=nm),
        "noise_map_level_bf16_sigma10": lambda: noise_map_level(pay_noisy, fmt, H, W, H, W, knots, torch.bfloat16, out=nm),
    }
    fmt10 = yuv_fmt(10, L.SN_YUV_420_LEFT, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    syms = ["sn_yuv_noise_hist", "sn_yuv_noise_hist_rect", "sn_yuv_noise_hist_bands", "sn_yuv_noise_hist_pairs", "sn_yuv_noise_hist_pairs_bands"]
    for tag, p, f in (("", pay, fmt), ("_sigma10", pay_noisy, fmt), ("_420p10", egress_yuv(rgb, fmt10, H, W), fmt10),
                      ("_420p10_sigma10", egress_yuv(noisy, fmt10, H, W), fmt10)):
        cases.update(hist_ab_cases(a.parent_lib, syms, tag, p, f, H, W))
    for f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():                                                   # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    px = T * H * W
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "ps_per_pixel": summary([m * 1e9 / px for m in v])} for k, v in ms.items()}
    print(json.dumps({"part": "nlf", "mode": "kernels", "frames": T, "size": [H, W], "reps": a.reps, "inner": a.inner, "new_vs_parent": hist_ab_verdict(ms), **res}))


def nlf_forward(a):
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(8, H, W, seed=2)
    rgb = ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0]
    g = torch.Generator("cuda").manual_seed(1)
    frames = []
    for i in range(n):                                                               # fresh noise of sigma 10 on every frame, as the sigma part
        j = i % 14
        x = rgb[j if j < 8 else 14 - j][None]
        frames.append(egress_yuv((x + torch.randn(x.shape, device="cuda", generator=g) * (10.0 / 255)).clamp(0, 1), fmt, H, W)[0].cpu().numpy())
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    seen = {}

    def run(model):
        vr = restore.VideoRestorer(net, one_len, sigma="auto", pipeline=True, noise_model=model)
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[str(model)] = vr.stats.get("window_nlf")
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(None)                                                                        # warm-up: code objects, engine buffers
    run("level")
    runs = {"auto": [], "level": []}
    for _ in range(a.runs):
        runs["auto"].append(run(None))
        runs["level"].append(run("level"))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs],
                  "frames_per_s_end_to_end": [round(n / r["total_s"], 2) for r in rs]}
    print(json.dumps({"part": "nlf", "mode": "forward", "variant": "denoise_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "runs": a.runs, "window_nlf_first": [round(k, 3) for k in seen["level"][0]], **res}))


def motion_kernels(a):
    """3.23: the matcher and the two histograms along its vectors beside the two plain pair histograms, 720p x 20 frames, 8 bit 4:2:0, interleaved."""
    T, H, W = 20, 720, 1280
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    rgb = ingest_u8(torch.from_numpy(np.concatenate([blur] * 5)).cuda(), torch.float32)[0]
    noisy = (rgb + torch.randn(rgb.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * (10.0 / 255)).clamp(0, 1)
    pay = egress_yuv(noisy, fmt, H, W)
    pairs = torch.empty((T - 1, 1021), dtype=torch.uint32, device="cuda")
    pair_bands = torch.empty((T - 1, 16, 128), dtype=torch.uint32, device="cuda")
    mv, sad = block_motion_yuv(pay, fmt, H, W)
    cases = {
        "noise_hist_pairs_yuv": lambda: noise_hist_pairs_yuv(pay, fmt, H, W, out=pairs),
        "noise_hist_pairs_bands_yuv": lambda: noise_hist_pairs_bands_yuv(pay, fmt, H, W, out=pair_bands),
        "block_motion_yuv": lambda: block_motion_yuv(pay, fmt, H, W, out_mv=mv, out_sad=sad),
        "noise_hist_pairs_mv_yuv": lambda: noise_hist_pairs_mv_yuv(pay, fmt, H, W, mv, out=pairs),
        "noise_hist_pairs_bands_mv_yuv": lambda: noise_hist_pairs_bands_mv_yuv(pay, fmt, H, W, mv, out=pair_bands),
    }
    fmt10 = yuv_fmt(10, L.SN_YUV_420_LEFT, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    pay10 = egress_yuv(noisy, fmt10, H, W)
    syms = ["sn_yuv_noise_hist_pairs", "sn_yuv_noise_hist_pairs_bands", "sn_yuv_noise_hist_pairs_mv", "sn_yuv_noise_hist_pairs_bands_mv"]
    for tag, p, f in (("", pay, fmt), ("_420p10", pay10, fmt10)):
        cases.update(hist_ab_cases(a.parent_lib, syms, tag, p, f, H, W, mv=mv if f is fmt else block_motion_yuv(p, f, H, W)[0]))
    for f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():                                                   # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    px = (T - 1) * H * W                                                             # per pixel of a pair
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "ps_per_pixel": summary([m * 1e9 / px for m in v])} for k, v in ms.items()}
    nz = float((mv != 0).any(dim=3).float().mean())
    print(json.dumps({"part": "motion", "mode": "kernels", "frames": T, "size": [H, W], "reps": a.reps, "inner": a.inner, "nonzero_vectors": round(nz, 4), "new_vs_parent": hist_ab_verdict(ms), **res}))


def motion_forward(a):
    """3.23: steady-state wall time per 720p window of the pipelined denoiser with sigma_estimator="min", without and with sigma_motion="blocks",
    alternating (the stream and the pattern of the sigma part)."""
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(8, H, W, seed=2)
    rgb = ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0]
    g = torch.Generator("cuda").manual_seed(1)
    frames = []
    for i in range(n):                                                               # fresh noise of sigma 10 on every frame, as the sigma part
        j = i % 14
        x = rgb[j if j < 8 else 14 - j][None]
        frames.append(egress_yuv((x + torch.randn(x.shape, device="cuda", generator=g) * (10.0 / 255)).clamp(0, 1), fmt, H, W)[0].cpu().numpy())
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    seen = {}

    def run(motion):
        vr = restore.VideoRestorer(net, one_len, sigma="auto", pipeline=True, sigma_estimator="min", sigma_motion=motion)
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[str(motion)] = (vr.stats["window_sigma"], vr.stats["window_sigma_temporal"])
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(None)                                                                        # warm-up: code objects, engine buffers
    run("blocks")
    runs = {"min": [], "min_blocks": []}
    for _ in range(a.runs):
        runs["min"].append(run(None))
        runs["min_blocks"].append(run("blocks"))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "motion", "mode": "forward", "variant": "denoise_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "runs": a.runs, "window_sigma_min": [round(s, 3) for s in seen["None"][0]], "window_sigma_min_blocks": [round(s, 3) for s in seen["blocks"][0]],
                      "window_temporal_min": [round(s, 3) for s in seen["None"][1]], "window_temporal_min_blocks": [round(s, 3) for s in seen["blocks"][1]], **res}))


def report_kernels(a):
    T, H, W = 16, 720, 1280
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    rgb = ingest_u8(torch.from_numpy(np.concatenate([blur] * 4)).cuda(), torch.float32)[0]
    clean = egress_yuv(rgb, fmt, H, W)                                               # what was written
    noisy = egress_yuv((rgb + torch.randn(rgb.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * (10.0 / 255)).clamp(0, 1), fmt, H, W)
    dst = torch.empty_like(clean)
    sums = torch.empty((T, L.SN_DIFF_STATS), dtype=torch.int64, device="cuda")
    pairs = torch.empty((T - 1, 1021), dtype=torch.uint32, device="cuda")
    sums_mv = torch.empty((T - 1, L.SN_DIFF_STATS_MV), dtype=torch.int64, device="cuda")
    mv, sad = block_motion_yuv(clean, fmt, H, W)                                     # the vectors of the written payloads, as the restorer takes them
    mv0 = torch.zeros_like(mv)
    cases = {
        "egress_yuv_fp32": lambda: egress_yuv(rgb, fmt, H, W, dst=dst),              # the launch the statistic follows: three times the bytes
        "diff_stats_yuv": lambda: diff_stats_yuv(noisy, clean, fmt, H, W, edge=16, out_sums=sums),
        "diff_stats_yuv_same": lambda: diff_stats_yuv(clean, clean, fmt, H, W, edge=16, out_sums=sums),      # d = 0 everywhere: the same loads
        "noise_hist_pairs_yuv": lambda: noise_hist_pairs_yuv(noisy, fmt, H, W, out=pairs),                   # a statistic that reads every luma plane twice
        "diff_stats_mv_yuv": lambda: diff_stats_mv_yuv(noisy, clean, fmt, H, W, mv, out_sums=sums_mv),      # report_motion: along the matcher's vectors
        "diff_stats_mv_yuv_zero": lambda: diff_stats_mv_yuv(noisy, clean, fmt, H, W, mv0, out_sums=sums_mv),      # all-zero vectors: the displaced rows are aligned
        "block_motion_yuv": lambda: block_motion_yuv(clean, fmt, H, W, out_mv=mv, out_sad=sad),              # ... and the matcher that precedes it
    }
    for f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():                                                   # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    px = T * H * W
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "ps_per_pixel": summary([m * 1e9 / px for m in v])} for k, v in ms.items()}
    print(json.dumps({"part": "report", "mode": "kernels", "frames": T, "size": [H, W], "reps": a.reps, "inner": a.inner,
                      "note": "diff_stats, diff_stats_mv and the pair histogram include the memset of dst",
                      "mv_nonzero_share": round(float((mv != 0).any(dim=-1).float().mean()), 4), **res}))


def report_forward(a):
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(8, H, W, seed=2)
    rgb = ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0]
    g = torch.Generator("cuda").manual_seed(1)
    frames = []
    for i in range(n):                                                               # fresh noise of sigma 10 on every frame, as the sigma part
        j = i % 14
        x = rgb[j if j < 8 else 14 - j][None]
        frames.append(egress_yuv((x + torch.randn(x.shape, device="cuda", generator=g) * (10.0 / 255)).clamp(0, 1), fmt, H, W)[0].cpu().numpy())
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    seen = {}

    def run(rep):
        vr = restore.VideoRestorer(net, one_len, sigma=10.0, pipeline=True, report=bool(rep), report_motion="blocks" if rep == "motion" else None)
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[rep] = vr.stats.get("report_summary")
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(False)                                                                       # warm-up: code objects, engine buffers
    run(True)
    run("motion")
    runs = {"off": [], "report": [], "report_motion": []}
    for _ in range(a.runs):
        runs["off"].append(run(False))
        runs["report"].append(run(True))
        runs["report_motion"].append(run("motion"))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "report", "mode": "forward", "variant": "denoise_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "runs": a.runs, "report_summary": {k: round(v, 4) for k, v in seen[True].items()}, **res}))


def quality_kernels(a):
    from shiftnet_amd import niqe
    from shiftnet_amd.io_edges import niqe_sums_yuv
    T, H, W = 16, 720, 1280
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    rgb = ingest_u8(torch.from_numpy(np.concatenate([blur] * 4)).cuda(), torch.float32)[0]
    clean = egress_yuv(rgb, fmt, H, W)
    noisy = egress_yuv((rgb + torch.randn(rgb.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * (10.0 / 255)).clamp(0, 1), fmt, H, W)
    mu, cov, win7 = niqe.load_params(niqe.default_params_path())
    taps = torch.from_numpy(win7.astype(np.float32)).cuda()
    sums = niqe_sums_yuv(noisy, fmt, H, W, taps)
    dsums = torch.empty((T, L.SN_DIFF_STATS), dtype=torch.int64, device="cuda")
    luma = torch.empty((T, H * W), dtype=torch.uint8, device="cuda")
    cases = {
        "niqe_sums_yuv": lambda: niqe_sums_yuv(noisy, fmt, H, W, taps, out=sums),
        "copy_luma": lambda: luma.copy_(noisy[:, :H * W]),                            # the bytes the kernel reads, once, and as many written
        "diff_stats_yuv": lambda: diff_stats_yuv(noisy, clean, fmt, H, W, edge=16, out_sums=dsums),      # the report's own launch
    }
    for f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():                                                   # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    host = sums.cpu().numpy()
    host_ms, scores = [], []
    for _ in range(3):
        for t in range(T):
            t0 = time.perf_counter()
            scores.append(niqe.frame_score(host[t], mu, cov))
            host_ms.append((time.perf_counter() - t0) * 1e3)
    px = T * H * W
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "us_per_frame": summary([m * 1e3 / T for m in v]),
               "ps_per_pixel": summary([m * 1e9 / px for m in v])} for k, v in ms.items()}
    print(json.dumps({"part": "quality", "mode": "kernels", "frames": T, "size": [H, W], "blocks": list(sums.shape[2:4]), "reps": a.reps, "inner": a.inner,
                      "host_ms_per_frame": summary(host_ms[T:]), "niqe_of_the_noisy_frames": summary(scores[:T]), **res}))


def quality_forward(a):
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(8, H, W, seed=2)
    rgb = ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0]
    g = torch.Generator("cuda").manual_seed(1)
    frames = []
    for i in range(n):                                                               # fresh noise of sigma 10 on every frame, as the report part
        j = i % 14
        x = rgb[j if j < 8 else 14 - j][None]
        frames.append(egress_yuv((x + torch.randn(x.shape, device="cuda", generator=g) * (10.0 / 255)).clamp(0, 1), fmt, H, W)[0].cpu().numpy())
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    seen = {}

    def run(quality):
        vr = restore.VideoRestorer(net, one_len, sigma=10.0, pipeline=True, report=True, report_quality=quality)
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[quality] = vr.stats.get("report_quality_summary")
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(None)                                                                        # warm-up: code objects, engine buffers
    run("niqe")
    runs = {"report": [], "report_quality": []}
    for _ in range(a.runs):
        runs["report"].append(run(None))
        runs["report_quality"].append(run("niqe"))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "quality", "mode": "forward", "variant": "denoise_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "runs": a.runs, "report_quality_summary": {k: round(v, 4) for k, v in seen["niqe"].items()}, **res}))


def fullref_kernels(a):
    from shiftnet_amd import fullref
    from shiftnet_amd.io_edges import ssim_sums_yuv
    T, H, W = 16, 720, 1280
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    rgb = ingest_u8(torch.from_numpy(np.concatenate([blur] * 4)).cuda(), torch.float32)[0]
    clean = egress_yuv(rgb, fmt, H, W)
    noisy = egress_yuv((rgb + torch.randn(rgb.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * (10.0 / 255)).clamp(0, 1), fmt, H, W)
    tiles = ssim_sums_yuv(clean, noisy, fmt, H, W)
    dsums = torch.empty((T, L.SN_DIFF_STATS), dtype=torch.int64, device="cuda")
    luma = torch.empty((2, T, H * W), dtype=torch.uint8, device="cuda")
    cases = {
        "ssim_sums_yuv": lambda: ssim_sums_yuv(clean, noisy, fmt, H, W, out_sums=tiles),
        "copy_luma_x2": lambda: (luma[0].copy_(clean[:, :H * W]), luma[1].copy_(noisy[:, :H * W])),      # the bytes the kernel reads, once, and as many written
        "diff_stats_yuv": lambda: diff_stats_yuv(clean, noisy, fmt, H, W, edge=0, out_sums=dsums),       # the other launch of the comparison
    }
    for f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():                                                   # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    host, rows = tiles.cpu().numpy(), dsums.cpu().numpy()
    px = T * H * W
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "us_per_frame": summary([m * 1e3 / T for m in v]),
               "ps_per_pixel": summary([m * 1e9 / px for m in v])} for k, v in ms.items()}
    print(json.dumps({"part": "fullref", "mode": "kernels", "frames": T, "size": [H, W], "tiles": list(tiles.shape[1:]), "reps": a.reps, "inner": a.inner,
                      "ssim_of_the_noisy_frames": summary([fullref.ssim_from_tiles(host[t], H, W) for t in range(T)]),
                      "psnr_y_of_the_noisy_frames": summary([fullref.psnr_from_sums(rows[t], 8)[0] for t in range(T)]), **res}))


def fullref_forward(a):
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(8, H, W, seed=2)
    rgb = ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0]
    g = torch.Generator("cuda").manual_seed(1)
    frames, truth = [], []
    for i in range(n):                                                               # fresh noise of sigma 10 on every frame, as the report part
        j = i % 14
        x = rgb[j if j < 8 else 14 - j][None]
        truth.append(egress_yuv(x, fmt, H, W)[0].cpu().numpy())
        frames.append(egress_yuv((x + torch.randn(x.shape, device="cuda", generator=g) * (10.0 / 255)).clamp(0, 1), fmt, H, W)[0].cpu().numpy())
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    seen = {}

    def run(gt):
        vr = restore.VideoRestorer(net, one_len, sigma=10.0, pipeline=True, report=True)
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W, gt=iter(truth) if gt else None)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[gt] = vr.stats.get("fullref_summary")
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(False)                                                                       # warm-up: code objects, engine buffers
    run(True)
    runs = {"report": [], "report_gt": []}
    for _ in range(a.runs):
        runs["report"].append(run(False))
        runs["report_gt"].append(run(True))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "fullref", "mode": "forward", "variant": "denoise_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "runs": a.runs, "fullref_means": {k: round(v, 4) for k, v in seen[True]["mean"].items()}, **res}))


def degrade_kernels(a):
    from shiftnet_amd import degrade
    from shiftnet_amd.io_edges import blur_yuv, degrade_yuv
    T, H, W = 16, 720, 1280
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    rgb = ingest_u8(torch.from_numpy(np.concatenate([blur] * 4)).cuda(), torch.float32)[0]
    gauss = torch.from_numpy(degrade.gauss_table().copy()).cuda()
    knots = [10.0] * 16
    tables = tuple(torch.from_numpy(t.copy()).cuda() for t in degrade.gamma_tables(2.2))
    cases, nbytes = {}, {}
    for tag, f in (("420p8", yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)), ("420p8_left", yuv_fmt(8, L.SN_YUV_420_LEFT, L.SN_YUV_BT709, L.SN_YUV_LIMITED)),
                   ("444p10", yuv_fmt(10, L.SN_YUV_444, L.SN_YUV_BT709, L.SN_YUV_LIMITED))):
        clean = egress_yuv(rgb, f, H, W)
        dst = torch.empty_like(clean)
        fb = f.frame_bytes(H, W)
        cases["degrade_yuv_" + tag] = (lambda c=clean, d=dst, f=f: degrade_yuv(c, f, H, W, knots, 1, 0, gauss, out=d))
        cases["egress_yuv_fp32_" + tag] = (lambda d=dst, f=f: egress_yuv(rgb, f, H, W, dst=d))
        cases["copy_payloads_" + tag] = (lambda c=clean, d=dst: d.copy_(c, non_blocking=True))
        nbytes["degrade_yuv_" + tag] = nbytes["copy_payloads_" + tag] = 2 * T * fb                    # the kernel's own bytes: every payload read once, written once
        nbytes["egress_yuv_fp32_" + tag] = T * (12 * H * W + fb)
        for n in (1, 7, 15):                                                             # the 16 payloads are the sources: T - 2r outputs whose windows clamp nowhere
            r, to = n // 2, T - 2 * (n // 2)
            for how, tab in (("gamma", tables), ("plain", None)):
                k = f"blur_yuv_n{n}_{how}_{tag}"
                cases[k] = (lambda c=clean, d=dst, f=f, n=n, r=r, to=to, tab=tab: blur_yuv(c, f, H, W, n, r, 0, T - 1, tab, out=d[:to]))
                nbytes[k] = (T + to) * fb                                                # the unique bytes: T = to + 2r payloads read, to written
    for f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, f in cases.items():                                                   # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "tb_per_s": summary([nbytes[k] / (m * 1e-3) / 1e12 for m in v]), "bytes": nbytes[k]} for k, v in ms.items()}
    print(json.dumps({"part": "degrade", "mode": "kernels", "frames": T, "size": [H, W], "reps": a.reps, "inner": a.inner, **res}))


def degrade_forward(a):
    """--add_noise 10 --report on a clean stream against the same stream degraded beforehand and run with the clean one as gt: the difference is the stage."""
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(8, H, W, seed=2)
    rgb = ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0]
    truth = []
    for i in range(n):
        j = i % 14
        truth.append(egress_yuv(rgb[j if j < 8 else 14 - j][None], fmt, H, W)[0].cpu().numpy())
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    frames, seen = [], {}

    def run(stage):
        vr = restore.VideoRestorer(net, one_len, sigma=10.0, pipeline=True, report=True, **({"add_noise": 10.0} if stage else {}))
        stamps = []
        t0 = time.perf_counter()
        more = {"degraded": lambda p: frames.append(p.copy())} if stage and not frames else ({} if stage else {"gt": iter(truth)})
        for i, p in enumerate(vr.restore(iter(truth if stage else frames), fmt, H, W, **more)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[stage] = vr.stats["fullref_summary"]
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(True)                                                                        # warm-up: code objects, engine buffers; and the degraded stream for the other side
    run(False)
    runs = {"pre_degraded_gt": [], "add_noise": []}
    for _ in range(a.runs):
        runs["pre_degraded_gt"].append(run(False))
        runs["add_noise"].append(run(True))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "degrade", "mode": "forward", "variant": "denoise_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "runs": a.runs, "same_numbers": seen[True] == seen[False], "fullref_means": {k: round(v, 4) for k, v in seen[True]["mean"].items()}, **res}))


def grain_kernels(a):
    """3.38: sn_yuv_grain on 16 frames of 720p 8-bit 4:2:0 at size 0 and 0.8, chroma share 0 and 0.5, out of place and in place, beside a plain device
    copy of the same payloads and sn_yuv_degrade (three gathers per pixel), interleaved."""
    from shiftnet_amd import degrade, grain
    from shiftnet_amd.io_edges import degrade_yuv, grain_yuv
    T, H, W = 16, 720, 1280
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    rgb = ingest_u8(torch.from_numpy(np.concatenate([blur] * 4)).cuda(), torch.float32)[0]
    gauss = torch.from_numpy(degrade.gauss_table().copy()).cuda()
    knots = [10.0] * 16
    f = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    clean = egress_yuv(rgb, f, H, W)
    dst, own = torch.empty_like(clean), clean.clone()
    fb = f.frame_bytes(H, W)
    cases = {"copy_payloads": lambda: dst.copy_(clean, non_blocking=True),
             "degrade_yuv": lambda: degrade_yuv(clean, f, H, W, knots, 1, 0, gauss, out=dst)}
    nbytes = {"copy_payloads": 2 * T * fb, "degrade_yuv": 2 * T * fb}
    for size in (0.0, 0.8):
        taps = grain.grain_taps(size)
        for chroma in (0.0, 0.5):
            k = f"grain_yuv_size{size:g}_chroma{chroma:g}"
            cases[k] = (lambda taps=taps, chroma=chroma: grain_yuv(clean, f, H, W, knots, taps, chroma, 1, 0, gauss, out=dst))
            nbytes[k] = 2 * T * fb                                                        # every payload read once, written once
            cases[k + "_in_place"] = (lambda taps=taps, chroma=chroma: grain_yuv(own, f, H, W, knots, taps, chroma, 1, 0, gauss, out=own))
            nbytes[k + "_in_place"] = 2 * T * (fb if chroma else H * W)                   # share 0 in place: the chroma planes are not touched
    for fn in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, fn in cases.items():                                                  # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "tb_per_s": summary([nbytes[k] / (m * 1e-3) / 1e12 for m in v]), "bytes": nbytes[k]} for k, v in ms.items()}
    print(json.dumps({"part": "grain", "mode": "kernels", "frames": T, "size": [H, W], "reps": a.reps, "inner": a.inner,
                      "note": "in place the clip accumulates grain from launch to launch: the codes drift to the legal range's ends, the work per sample stays", **res}))


def grain_forward(a):
    """3.38: steady-state wall and forward time per 720p window of the pipelined denoiser (as the sigma part, sigma=10.0) without grain and with
    grain="auto:0.5", size 0.8, chroma share 0.5, runs of the two alternating in one process, the first two windows left out."""
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    blur, _ = synth.blurred_clip(8, H, W, seed=2)
    rgb = ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0]
    g = torch.Generator("cuda").manual_seed(1)
    frames = []
    for i in range(n):                                                               # fresh noise of sigma 10 on every frame, as the sigma part
        j = i % 14
        x = rgb[j if j < 8 else 14 - j][None]
        frames.append(egress_yuv((x + torch.randn(x.shape, device="cuda", generator=g) * (10.0 / 255)).clamp(0, 1), fmt, H, W)[0].cpu().numpy())
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    seen = {}

    def run(on):
        vr = restore.VideoRestorer(net, one_len, sigma=10.0, pipeline=True, **(dict(grain="auto:0.5", grain_size=0.8, grain_chroma=0.5) if on else {}))
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[on] = vr.stats.get("grain_launches")
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(False)                                                                       # warm-up: code objects, engine buffers
    run(True)
    runs = {"off": [], "grain": []}
    for _ in range(a.runs):
        runs["off"].append(run(False))
        runs["grain"].append(run(True))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "grain", "mode": "forward", "variant": "denoise_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "runs": a.runs, "grain_launches": seen[True], **res}))


def deflicker_kernels(a):
    """3.39: sn_yuv_code_hist and sn_yuv_apply_lut on 16 frames of 720p at 8-bit and 10-bit 4:2:0, on a noisy clip and on a flat one, beside a plain
    device copy of the same payloads and sn_yuv_degrade, interleaved."""
    from shiftnet_amd import degrade
    from shiftnet_amd.io_edges import apply_lut_yuv, code_hist_yuv, degrade_yuv
    T, H, W = 16, 720, 1280
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    rgb = ingest_u8(torch.from_numpy(np.concatenate([blur] * 4)).cuda(), torch.float32)[0]
    g = torch.Generator("cuda").manual_seed(1)
    noisy = (rgb + torch.randn(rgb.shape, device="cuda", generator=g) * (10.0 / 255)).clamp(0, 1)
    gauss = torch.from_numpy(degrade.gauss_table().copy()).cuda()
    cases, nbytes = {}, {}
    for bits in (8, 10):
        f = yuv_fmt(bits, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
        fb, esz, codes = f.frame_bytes(H, W), 1 if bits == 8 else 2, 1 << bits
        clips = {"noisy": egress_yuv(noisy, f, H, W), "flat": egress_yuv(torch.full_like(rgb, 0.5), f, H, W)}
        dst = torch.empty_like(clips["noisy"])
        hist = torch.empty((T, codes), dtype=torch.int32, device="cuda")
        lut = torch.from_numpy(np.tile(((np.arange(codes) * 15) // 16 + codes // 32).astype(np.uint16).view(np.int16), (T, 2, 1))).cuda()      # a gain of 15/16 about mid-grey
        cases[f"copy_payloads_{bits}"] = lambda src=clips["noisy"], dst=dst: dst.copy_(src, non_blocking=True)
        nbytes[f"copy_payloads_{bits}"] = 2 * T * fb
        if bits == 8:
            cases["degrade_yuv_8"] = lambda src=clips["noisy"], dst=dst, f=f: degrade_yuv(src, f, H, W, [10.0] * 16, 1, 0, gauss, out=dst)
            nbytes["degrade_yuv_8"] = 2 * T * fb
        for kind, src in clips.items():
            cases[f"code_hist_{bits}_{kind}"] = lambda src=src, f=f, hist=hist: code_hist_yuv(src, f, H, W, out=hist)
            nbytes[f"code_hist_{bits}_{kind}"] = T * H * W * esz                             # the luma planes, read once
            cases[f"apply_lut_{bits}_{kind}"] = lambda src=src, f=f, lut=lut, dst=dst: apply_lut_yuv(src, f, H, W, lut, out=dst)
            nbytes[f"apply_lut_{bits}_{kind}"] = 2 * T * fb                                  # every payload read once, written once
    for fn in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, fn in cases.items():                                                  # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "tb_per_s": summary([nbytes[k] / (m * 1e-3) / 1e12 for m in v]), "bytes": nbytes[k]} for k, v in ms.items()}
    ratio = {bits: round(statistics.median(ms[f"code_hist_{bits}_flat"]) / statistics.median(ms[f"code_hist_{bits}_noisy"]), 3) for bits in (8, 10)}
    print(json.dumps({"part": "deflicker", "mode": "kernels", "frames": T, "size": [H, W], "reps": a.reps, "inner": a.inner,
                      "note": "code_hist includes the memset of its destination", "hist_flat_to_noisy": ratio, **res}))


def deflicker_forward(a):
    """3.39: steady-state wall and forward time per 720p window of the pipelined deblurrer without and with deflicker=3 on a stream whose luma flickers
    by +-8 %, runs of the two alternating in one process, the first two windows left out."""
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    gains = 1.0 + np.random.default_rng(3).uniform(-0.08, 0.08, n)
    frames = []
    for p, gain in zip(_stream(H, W, n, fmt, n_src=8), gains):
        p = p.copy()
        p[:H * W] = np.clip(np.floor(16.0 + gain * (p[:H * W].astype(np.float64) - 16.0) + 0.5), 0, 255).astype(np.uint8)
        frames.append(p)
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    seen = {}

    def run(on):
        vr = restore.VideoRestorer(net, one_len, pipeline=True, **(dict(deflicker=3) if on else {}))
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[on] = vr.stats.get("deflicker_launches")
        if on:
            from shiftnet_amd.deflicker import mean_roughness
            fd = vr.stats["frame_deflicker"]
            seen["roughness"] = [round(mean_roughness([f[1] for f in fd]), 3), round(mean_roughness([f[2] for f in fd]), 3)]
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(False)                                                                       # warm-up: code objects, engine buffers
    run(True)
    runs = {"off": [], "deflicker": []}
    for _ in range(a.runs):
        runs["off"].append(run(False))
        runs["deflicker"].append(run(True))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "deflicker", "mode": "forward", "variant": "deblur_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "runs": a.runs, "deflicker_launches": seen[True], "mean_roughness_before_after": seen["roughness"], **res}))


def despot_kernels(a):
    """3.40: sn_yuv_despot on the 14 frames of 16 payloads of 720p that have two neighbours, and the two sn_yuv_block_motion launches that make its
    vectors (on the stack and on the time-reversed stack, as despot_vectors makes them), at 8-bit and 10-bit 4:2:0, beside a plain device copy of
    the 16 payloads, interleaved."""
    from shiftnet_amd.io_edges import despot_yuv
    T, H, W = 16, 720, 1280
    blur, _ = synth.blurred_clip(4, H, W, seed=1)
    rgb = ingest_u8(torch.from_numpy(np.concatenate([blur, blur[::-1]] * 2)).cuda(), torch.float32)[0]      # consecutive frames are neighbours
    g = torch.Generator("cuda").manual_seed(1)
    noisy = (rgb + torch.randn(rgb.shape, device="cuda", generator=g) * (5.0 / 255)).clamp(0, 1)
    cases, nbytes, replaced = {}, {}, {}
    for bits in (8, 10):
        f = yuv_fmt(bits, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
        fb, esz = f.frame_bytes(H, W), 1 if bits == 8 else 2
        src = egress_yuv(noisy, f, H, W)
        rev = src.flip(0).contiguous()
        dst = torch.empty_like(src)
        mvn, sad = block_motion_yuv(src, f, H, W)
        mvr, sadr = block_motion_yuv(rev, f, H, W)
        mvp = mvr.flip(0).contiguous()
        counts = torch.empty((T - 2, 2), dtype=torch.int32, device="cuda")
        cases[f"copy_payloads_{bits}"] = lambda src=src, dst=dst: dst.copy_(src, non_blocking=True)
        nbytes[f"copy_payloads_{bits}"] = 2 * T * fb
        cases[f"block_motion_both_ways_{bits}"] = lambda src=src, rev=rev, f=f, mvn=mvn, sad=sad, mvr=mvr, sadr=sadr: (
            block_motion_yuv(src, f, H, W, out_mv=mvn, out_sad=sad), block_motion_yuv(rev, f, H, W, out_mv=mvr, out_sad=sadr))
        nbytes[f"block_motion_both_ways_{bits}"] = 2 * T * H * W * esz                       # the luma planes, read once per direction
        for chroma in ("follow", "off"):
            cases[f"despot_{bits}_{chroma}"] = lambda src=src, f=f, mvp=mvp, mvn=mvn, dst=dst, counts=counts, chroma=chroma: despot_yuv(
                src, f, H, W, mvp, mvn, 1, T - 2, 24, 2, 1, chroma, out=dst[:T - 2], out_counts=counts)
            nbytes[f"despot_{bits}_{chroma}"] = (T - 2) * (2 * fb + 2 * H * W * esz)             # a frame read and written once, two neighbours' luma read
        despot_yuv(src, f, H, W, mvp, mvn, 1, T - 2, 24, 2, 1, "follow", out=dst[:T - 2], out_counts=counts)
        replaced[bits] = round(float(counts.cpu().numpy().view(np.uint32)[:, 1].mean()) / (H * W), 6)
    for fn in cases.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, fn in cases.items():                                                  # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    res = {k: {"us_per_call": summary([m * 1e3 for m in v]), "tb_per_s": summary([nbytes[k] / (m * 1e-3) / 1e12 for m in v]), "bytes": nbytes[k]} for k, v in ms.items()}
    print(json.dumps({"part": "despot", "mode": "kernels", "frames": T, "repaired": T - 2, "size": [H, W], "reps": a.reps, "inner": a.inner,
                      "note": "despot includes the memset of its counts; block_motion_both_ways is two launches", "mean_share_replaced": replaced, **res}))


def despot_forward(a):
    """3.40: steady-state wall and forward time per 720p window of the pipelined deblurrer without and with despot=24, runs of the two alternating in
    one process, the first two windows left out."""
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    frames = _stream(H, W, n, fmt, n_src=8)
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    seen = {}

    def run(on):
        vr = restore.VideoRestorer(net, one_len, pipeline=True, **(dict(despot=24) if on else {}))
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[on] = vr.stats.get("despot_launches")
        if on:
            from shiftnet_amd.despot import frames_kept, median_share
            seen["share"] = [round(median_share(vr.stats["frame_despot"]), 6), frames_kept(vr.stats["frame_despot"])]
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(False)                                                                       # warm-up: code objects, engine buffers
    run(True)
    runs = {"off": [], "despot": []}
    for _ in range(a.runs):
        runs["off"].append(run(False))
        runs["despot"].append(run(True))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "despot", "mode": "forward", "variant": "deblur_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "runs": a.runs, "despot_launches": seen[True], "median_share_and_frames_kept": seen["share"], **res}))


def _tile_word(word):
    return None if word == "full" else restore.tile_arg(word)


def _stream(H, W, n, fmt, n_src=4):
    """n payloads of H x W on the host: the blurred synthetic clip, its n_src frames walked back and forth so that consecutive frames are neighbours."""
    blur, _ = synth.blurred_clip(n_src, H, W, seed=2)
    pay = egress_yuv(ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0], fmt, H, W).cpu().numpy()
    period = 2 * n_src - 2
    return [pay[j if j < n_src else period - j] for j in (i % period for i in range(n))]


def tiles_forward(a):
    H, W = (int(v) for v in (a.size or "720x1280").split("x"))
    one_len, nwin = 16, a.windows
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    frames = _stream(H, W, one_len * nwin, fmt)
    net = restore.load_net(a.variant, "synthetic", "bf16")
    kw = {"sigma": 10.0} if "denoise" in a.variant else {}
    forms = a.tile or ["full"]
    plans = {}

    def run(word):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        vr = restore.VideoRestorer(net, one_len, pipeline=True, tile=_tile_word(word), tile_overlap=a.tile_overlap, **kw)
        t0 = time.perf_counter()
        for _ in vr.restore(iter(frames), fmt, H, W):
            pass
        total = time.perf_counter() - t0
        torch.cuda.synchronize()
        plans[word] = vr.stats.get("window_tiles", [None])[0]
        return {"total_s": total, "window_forward_ms": vr.stats["window_forward_ms"][1:], "peak_bytes": torch.cuda.max_memory_allocated()}

    runs = {w: [] for w in forms}
    for _ in range(a.runs):
        for w in forms:                                                              # alternating: every round runs every form
            runs[w].append(run(w))
    res = {}
    for w, rs in runs.items():
        fwd = [g for r in rs for g in r["window_forward_ms"]]
        res[w] = {"window_forward_ms": summary(fwd), "window_forward_ms_per_run": [round(statistics.median(r["window_forward_ms"]), 2) for r in rs],
                  "frames_per_s_forward": {k: round(one_len * 1e3 / v, 3) for k, v in (("median", statistics.median(fwd)), ("slowest", max(fwd)), ("fastest", min(fwd)))},
                  "frames_per_s_end_to_end": [round(one_len * nwin / r["total_s"], 2) for r in rs],
                  "peak_allocated_gb": [round(r["peak_bytes"] / 1e9, 3) for r in rs],
                  "tiles": None if plans[w] is None else {"count": len(plans[w]), "first": [list(t) for t in plans[w][:2]],
                                                           "pixels_over_picture": round(sum(t[2] * t[3] for t in plans[w]) / (H * W), 4)}}
    print(json.dumps({"part": "tiles", "mode": "forward", "variant": a.variant, "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "tile_overlap": a.tile_overlap, "runs": a.runs, "forms_in_this_process": forms, **res}))


def tiles_quality(a):
    """|tiled - full| of the written samples at a small size, 2 x 2 tiles, by overlap.  Synthetic weights: how the blend behaves, not how a trained
    network's seams look."""
    H, W = (int(v) for v in (a.size or "256x384").split("x"))
    one_len = 4
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    frames = _stream(H, W, 2 * one_len, fmt)
    net = restore.load_net(a.variant, "synthetic", "bf16")
    kw = {"sigma": 10.0} if "denoise" in a.variant else {}

    def run(tile, overlap):
        vr = restore.VideoRestorer(net, one_len, out_format="444p10", tile=tile, tile_overlap=overlap, **kw)
        out = np.stack(list(vr.restore(iter(frames), fmt, H, W))).view("<u2").astype(np.float64) / 4.0      # 10-bit codes in 8-bit code units
        return out.reshape(len(frames), 3, H, W), vr.stats.get("window_tiles", [None])[0]

    full, _ = run(None, 32)
    res = {}
    for v in (0, 16, 32, 64):
        up = lambda n: -(-n // 4) * 4      # noqa: E731
        tile = (up((H + v + 1) // 2), up((W + v + 1) // 2))                          # the smallest 2 x 2 tiles that overlap by at least v
        got, tiles = run(tile, v)
        d = np.abs(got - full)
        band = np.zeros((H, W), dtype=bool)                                          # within 16 samples of where a tile ends inside the picture
        for y0, x0, th, tw in tiles:
            for e in (y0, y0 + th):
                if 0 < e < H:
                    band[max(e - 16, 0):e + 16, :] = True
            for e in (x0, x0 + tw):
                if 0 < e < W:
                    band[:, max(e - 16, 0):e + 16] = True
        res[f"overlap_{v}"] = {"tile": list(tile), "tiles": [list(t) for t in tiles],
                               "luma_max": round(float(d[:, 0].max()), 3), "luma_rms": round(float(np.sqrt((d[:, 0] ** 2).mean())), 4),
                               "all_planes_max": round(float(d.max()), 3), "all_planes_rms": round(float(np.sqrt((d ** 2).mean())), 4),
                               "luma_rms_near_tile_edges": round(float(np.sqrt((d[:, 0][:, band] ** 2).mean())), 4),
                               "luma_rms_elsewhere": round(float(np.sqrt((d[:, 0][:, ~band] ** 2).mean())), 4)}
    print(json.dumps({"part": "tiles", "mode": "quality", "variant": a.variant, "dtype": "bf16", "size": [H, W], "frames": len(frames), "unit": "8-bit codes of Y'CbCr, "
                      "measured on 10 bit 4:4:4 output", "note": "synthetic weights: how the blend behaves, not how a trained network's seams look", **res}))


PICTURE = dict(H=1080, W=1920, rect=(0, 138, 1920, 804))


def overlap_forward(a):
    H, W, one_len, nwin = 720, 1280, 16, a.windows
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    frames = _stream(H, W, one_len * nwin, fmt)
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    forms = a.overlap or [0]

    def run(v):
        torch.cuda.synchronize()
        vr = restore.VideoRestorer(net, one_len, pipeline=True, window_overlap=v)
        t0 = time.perf_counter()
        for _ in vr.restore(iter(frames), fmt, H, W):
            pass
        total = time.perf_counter() - t0
        torch.cuda.synchronize()
        seams = [x for s in vr.stats.get("seam_rms", []) if s is not None for x in s]
        return {"total_s": total, "window_forward_ms": vr.stats["window_forward_ms"][1:], "windows": vr.stats["windows"],
                "seam_rms_median": statistics.median(seams) if seams else None}

    runs = {v: [] for v in forms}
    for _ in range(a.runs):
        for v in forms:                                                              # alternating: every round runs every form
            runs[v].append(run(v))
    res = {}
    for v, rs in runs.items():
        fwd = [g for r in rs for g in r["window_forward_ms"]]
        res[f"V={v}"] = {"window_forward_ms": summary(fwd), "windows": rs[0]["windows"], "total_s": [round(r["total_s"], 3) for r in rs],
                         "frames_per_s_end_to_end": [round(one_len * nwin / r["total_s"], 2) for r in rs],
                         "windows_over_no_overlap": round(rs[0]["windows"] / nwin, 4), "seam_rms_median_synthetic_weights": rs[0]["seam_rms_median"]}
    print(json.dumps({"part": "overlap", "mode": "forward", "variant": "deblur_small", "dtype": "bf16", "one_len": one_len, "frames": one_len * nwin,
                      "size": [H, W], "runs": a.runs, **res}))


def overlap_kernels(a):
    from shiftnet_amd.io_edges import time_crossfade
    from shiftnet_amd.windows import overlap_weights
    V, C, H, W = 4, 3, 720, 1280
    g = torch.Generator("cuda").manual_seed(0)
    prev = torch.rand((V, C, H, W), device="cuda", generator=g)
    cur = torch.rand((V, C, H, W), device="cuda", generator=g)
    spare = torch.empty_like(cur)
    wp, wc = (torch.from_numpy(w).cuda() for w in overlap_weights(V))
    sq = torch.zeros((V, C), dtype=torch.int64, device="cuda")
    # the same three on six sets of tensors taken in turn, 800 MB in all: more than the 256 MB Infinity Cache holds, so every launch reads HBM
    import itertools
    sets = itertools.cycle([(torch.rand((V, C, H, W), device="cuda", generator=g), torch.rand((V, C, H, W), device="cuda", generator=g)) for _ in range(6)])
    cases = {"time_crossfade": (12, lambda: time_crossfade(prev, cur, wp, wc, H, W)),
             "time_crossfade_sq": (12, lambda: time_crossfade(prev, cur, wp, wc, H, W, sq=sq)),
             "d2d_copy_f32": (8, lambda: spare.copy_(prev, non_blocking=True)),
             "time_crossfade_cold": (12, lambda: time_crossfade(*next(sets), wp, wc, H, W)),
             "time_crossfade_sq_cold": (12, lambda: time_crossfade(*next(sets), wp, wc, H, W, sq=sq)),
             "d2d_copy_f32_cold": (8, lambda: (lambda a, b: b.copy_(a, non_blocking=True))(*next(sets)))}
    for _, f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, (_, f) in cases.items():                                              # interleaved: every repetition times every case
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    px = V * C * H * W
    res = {k: {"us_per_launch": summary([m * 1e3 for m in v]), "tb_per_s_median": round(cases[k][0] * px / (statistics.median(v) * 1e-3) / 1e12, 3)}
           for k, v in ms.items()}
    print(json.dumps({"part": "overlap", "mode": "kernels", "shape": [V, C, H, W], "mbytes_moved": {k: round(b * px / 1e6, 1) for k, (b, _) in cases.items()},
                      "reps": a.reps, "inner": a.inner, **res}))


def boxed_1080p(fmt, n_src=8):
    """n_src payloads of a 1920 x 1080 stream on the device: the blurred synthetic clip at 804 rows inside PICTURE['rect'], bars at black (16 / 128)."""
    H, W, (x0, y0, w, h) = PICTURE["H"], PICTURE["W"], PICTURE["rect"]
    blur, _ = synth.blurred_clip(n_src, h, w, seed=2)
    full = torch.empty((n_src, fmt.frame_bytes(H, W)), dtype=torch.uint8, device="cuda")
    full[:, :H * W] = 16
    full[:, H * W:] = 128
    inner = ingest_u8(torch.from_numpy(blur).cuda(), torch.float32)[0]
    return egress_yuv(inner, fmt, H, W, dst=full, rect=PICTURE["rect"]), inner


def parent_cases(path, fmt, T, H, W, h, w, pay, crop, out_full, out_crop, x_full, x_crop, dst_full, dst_crop):
    """sn_ingest_yuv / sn_egress_yuv of ANOTHER build of csrc/sn_yuv.hip (--parent_lib: the parent commit's, compiled on its own into a shared
    library), called through ctypes on the same tensors, so that the two builds are timed interleaved in one process."""
    if not path:
        return {}
    import ctypes as C
    lib = C.CDLL(os.path.abspath(path))
    vp, ci = C.c_void_p, C.c_int
    lib.sn_ingest_yuv.argtypes = [vp, C.POINTER(L.YuvFmt), vp, ci, ci, ci, ci, ci, ci, vp]
    lib.sn_egress_yuv.argtypes = [vp, ci, C.POINTER(L.YuvFmt), vp, ci, ci, ci, ci, ci, vp]
    st = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731

    def ing(p, x, hh, ww):
        return lambda: L.check(lib.sn_ingest_yuv(p.data_ptr(), fmt, x.data_ptr(), L.SN_BF16, T, hh, ww, hh, ww, st()), "parent sn_ingest_yuv")

    def egr(o, d, hh, ww):
        return lambda: L.check(lib.sn_egress_yuv(o.data_ptr(), L.SN_BF16, fmt, d.data_ptr(), T, hh, ww, hh, ww, st()), "parent sn_egress_yuv")
    return {"parent_ingest_yuv_1080": (T * H * W, ing(pay, x_full, H, W)), "parent_ingest_yuv_804": (T * h * w, ing(crop, x_crop, h, w)),
            "parent_egress_yuv_1080": (T * H * W, egr(out_full, dst_full, H, W)), "parent_egress_yuv_804": (T * h * w, egr(out_crop, dst_crop, h, w))}


def picture_kernels(a):
    T, H, W, rect = 8, PICTURE["H"], PICTURE["W"], PICTURE["rect"]
    h, w = rect[3], rect[2]
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    pay, inner = boxed_1080p(fmt, T)
    whole = (0, 0, W, H)
    crop = egress_yuv(inner, fmt, h, w)                                              # the cropped stream: 804 rows, the same pixel count as the rectangle
    rgb_full = ingest_yuv(pay, fmt, H, W, H, W, torch.float32)[0]
    out_full, out_crop = rgb_full.to(torch.bfloat16), inner.to(torch.bfloat16)
    x_full = torch.empty((1, T, 3, H, W), dtype=torch.bfloat16, device="cuda")
    x_crop = torch.empty((1, T, 3, h, w), dtype=torch.bfloat16, device="cuda")
    dst_full, dst_crop = torch.empty_like(pay), torch.empty_like(crop)
    thumbs = torch.empty((T, (H + 7) // 8, (W + 7) // 8), dtype=torch.uint16, device="cuda")
    rows, cols = torch.empty((T, H), dtype=torch.uint32, device="cuda"), torch.empty((T, W), dtype=torch.uint32, device="cuda")
    cases = {                                                                        # name: (pixels per launch, the launch)
        "ingest_yuv_1080": (T * H * W, lambda: ingest_yuv(pay, fmt, H, W, H, W, torch.bfloat16, out=x_full)),
        "ingest_yuv_rect_whole_1080": (T * H * W, lambda: ingest_yuv(pay, fmt, H, W, H, W, torch.bfloat16, out=x_full, rect=whole)),
        "ingest_yuv_804": (T * h * w, lambda: ingest_yuv(crop, fmt, h, w, h, w, torch.bfloat16, out=x_crop)),
        "ingest_yuv_rect_804_of_1080": (T * h * w, lambda: ingest_yuv(pay, fmt, H, W, h, w, torch.bfloat16, out=x_crop, rect=rect)),
        "egress_yuv_1080": (T * H * W, lambda: egress_yuv(out_full, fmt, H, W, dst=dst_full)),
        "egress_yuv_rect_whole_1080": (T * H * W, lambda: egress_yuv(out_full, fmt, H, W, dst=dst_full, rect=whole)),
        "egress_yuv_804": (T * h * w, lambda: egress_yuv(out_crop, fmt, h, w, dst=dst_crop)),
        "egress_yuv_rect_804_of_1080": (T * h * w, lambda: egress_yuv(out_crop, fmt, H, W, dst=dst_full, rect=rect)),
        **parent_cases(a.parent_lib, fmt, T, H, W, h, w, pay, crop, out_full, out_crop, x_full, x_crop, dst_full, dst_crop),
        "d2d_copy_payloads_1080": (T * H * W, lambda: dst_full.copy_(pay, non_blocking=True)),       # what _run adds per restored frame of a rectangle
        "thumb_yuv_1080": (T * H * W, lambda: thumb_yuv(pay, fmt, H, W, out=thumbs)),
        "rowcol_sums_yuv_1080": (T * H * W, lambda: rowcol_sums_yuv(pay, fmt, H, W, out_rows=rows, out_cols=cols)),
    }
    for _, f in cases.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k, (_, f) in cases.items():                                              # interleaved: every repetition times every kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.inner)
    res = {k: {"us_per_frame": summary([m * 1e3 / T for m in v]), "ps_per_pixel": summary([m * 1e9 / cases[k][0] for m in v])} for k, v in ms.items()}
    print(json.dumps({"part": "picture", "mode": "kernels", "frames": T, "size": [H, W], "rect": list(rect), "reps": a.reps, "inner": a.inner,
                      "note": "rowcol_sums includes its two memsets", **res}))


def picture_forward(a):
    H, W, rect, one_len, nwin = PICTURE["H"], PICTURE["W"], PICTURE["rect"], 16, a.windows
    n = one_len * nwin
    fmt = yuv_fmt(8, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    pay8 = boxed_1080p(fmt, 8)[0].cpu().numpy()
    hd = y4m.Y4MHeader(width=W, height=H, chroma="420jpeg")
    buf = io.BytesIO()
    wr = y4m.Y4MWriter(buf, hd)
    for i in range(n):
        j = i % 14
        wr.write(pay8[j if j < 8 else 14 - j])
    data = buf.getvalue()
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    pic = "auto" if a.picture == "auto" else rect
    seen = {}

    def run(picture):
        vr = restore.VideoRestorer(net, one_len, pipeline=True, picture=picture)
        stamps = []
        t0 = time.perf_counter()
        for i, _ in enumerate(vr.restore(y4m.Y4MReader(io.BytesIO(data)), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[str(picture)] = vr.stats["window_picture"]
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:],
                "stager_wait_ms": vr.stats.get("picture_wait_ms", [])[2:]}

    run(None)                                                                        # warm-up: code objects, engine buffers and plans of both sizes
    run(pic)
    runs = {"full": [], "picture": []}
    for _ in range(a.runs):
        runs["full"].append(run(None))
        runs["picture"].append(run(pic))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]),
                  "window_forward_ms_per_run": [round(statistics.median(r["window_forward_ms"]), 2) for r in rs],
                  "window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "total_s": [round(r["total_s"], 3) for r in rs]}
        w = [g for r in rs for g in r["stager_wait_ms"]]
        if w:
            res[k]["stager_wait_ms"] = summary(w)
    ratio = res["picture"]["window_forward_ms"]["median"] / res["full"]["window_forward_ms"]["median"]
    print(json.dumps({"part": "picture", "mode": "forward", "variant": "deblur_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W],
                      "rect": list(rect), "picture": a.picture, "runs": a.runs, "pixel_ratio": rect[2] * rect[3] / (H * W), "forward_ratio": ratio,
                      "window_picture": [None if r is None else list(r) for r in seen[str(pic)][:3]], **res}))


def picture_part(a):
    {"forward": picture_forward, "kernels": picture_kernels}[a.mode](a)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernels", "pipeline", "sigma", "picture", "nlf", "report", "motion", "tiles", "overlap", "quality", "fullref", "degrade", "grain", "deflicker", "despot"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=["both", "pipelined", "serial"], default="both", help="pipeline part: one mode only (for a kernel trace of its own)")
    ap.add_argument("--scene_cuts", choices=["off", "auto", "listed"], default="off", help="pipeline part: VideoRestorer(scene_cuts=...)")
    ap.add_argument("--cut_every", type=int, default=0, help="pipeline part: a cut every N frames in the stream (0: none)")
    ap.add_argument("--parent_lib", default=None, metavar="SO", help="kernels part and picture part in kernels mode: a shared library built from another commit's "
                    "csrc/sn_yuv.hip alone; its sn_ingest_yuv / sn_egress_yuv are timed beside this build's.  nlf and motion parts in kernels mode: a library "
                    "built from another commit's whole csrc; its seven noise-histogram entry points are timed beside this build's, at 8 and 10 bit")
    ap.add_argument("--only_cases", default=None, metavar="WORDS", help="kernels part: time only the cases whose name contains one of these comma-separated words")
    ap.add_argument("--mode", choices=["forward", "kernels", "quality"], default="forward", help="picture, nlf, report, motion, tiles, overlap, quality, fullref, degrade, grain, deflicker and despot parts: which measurement "
                    "(quality: the tiles part alone)")
    ap.add_argument("--picture", choices=["auto", "fixed"], default="auto", help="picture part, forward mode: VideoRestorer(picture='auto') or the rectangle itself")
    ap.add_argument("--tile", action="append", default=None, metavar="{full,N,HxW}", help="tiles part, forward mode: a form to run (repeat for several, which then alternate)")
    ap.add_argument("--tile_overlap", type=int, default=32, help="tiles part, forward mode: VideoRestorer(tile_overlap=...)")
    ap.add_argument("--overlap", action="append", type=int, default=None, metavar="V", help="overlap part, forward mode: a window_overlap to run (repeat for several, which then alternate)")
    ap.add_argument("--size", default=None, metavar="HxW", help="tiles part: the stream's size (default 720x1280 forward, 256x384 quality)")
    ap.add_argument("--variant", choices=list(restore.VARIANTS), default="deblur_small", help="tiles part: the network")
    a = ap.parse_args()
    with torch.no_grad():
        {"kernels": kernels, "pipeline": pipeline, "sigma": sigma, "picture": picture_part,
         "nlf": nlf_kernels if a.mode == "kernels" else nlf_forward,
         "report": report_kernels if a.mode == "kernels" else report_forward,
         "motion": motion_kernels if a.mode == "kernels" else motion_forward,
         "tiles": tiles_quality if a.mode == "quality" else tiles_forward,
         "overlap": overlap_kernels if a.mode == "kernels" else overlap_forward,
         "quality": quality_kernels if a.mode == "kernels" else quality_forward,
         "fullref": fullref_kernels if a.mode == "kernels" else fullref_forward,
         "degrade": degrade_kernels if a.mode == "kernels" else degrade_forward,
         "grain": grain_kernels if a.mode == "kernels" else grain_forward,
         "deflicker": deflicker_kernels if a.mode == "kernels" else deflicker_forward,
         "despot": despot_kernels if a.mode == "kernels" else despot_forward}[a.part](a)
