#!/usr/bin/env python3
"""Measurements behind DESIGN.md 3.11, 3.13 and 3.14 (run on the MI355X from the repository root).

  kernels : time per pixel of sn_ingest_yuv / sn_egress_yuv / sn_yuv_thumb / sn_yuv_noise_hist (4:2:0 8 bit, 720p x 20 frames; the noise
            histogram on the same frames with noise of sigma 10 as well) beside sn_ingest_u8 / sn_egress_u8 on the same
            frames, interleaved in one process: REPS repetitions, each timing INNER back-to-back launches of every kernel with device events;
            median and min..max over the repetitions.
  pipeline: steady-state wall time per 720p window of the pipelined restorer (Shift-Net-s, one_len 16, bf16, Y4M held in memory) beside the
            forward-only time of the same windows (device events in the same runs) and beside pipeline=False, the two alternating.
            --scene_cuts auto: the same stream with the cut detector running (sn_yuv_thumb; 3.13).  --cut_every N: every second scene of N frames
            is inverted, so that the stream has a cut every N frames; with --scene_cuts off / auto / listed.
  sigma   : steady-state wall time per 720p window of the pipelined denoiser (Shift-Net-s denoise, one_len 16, bf16) with sigma=10.0 and with
            sigma="auto" (sn_yuv_noise_hist per window; 3.14), runs of the two alternating in one process, the first two windows left out.
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
from shiftnet_amd.io_edges import egress_u8, egress_yuv, ingest_u8, ingest_yuv, noise_hist_yuv, thumb_yuv, yuv_fmt  # noqa: E402


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
    pay_noisy = egress_yuv((rgb + torch.randn(rgb.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * (10.0 / 255)).clamp(0, 1), fmt, H, W)
    cases = {
        "ingest_yuv_bf16": lambda: ingest_yuv(pay, fmt, H, W, H, W, torch.bfloat16, out=x_bf),
        "thumb_yuv": lambda: thumb_yuv(pay, fmt, H, W, out=thumbs),
        "noise_hist_yuv": lambda: noise_hist_yuv(pay, fmt, H, W, out=hists),                 # a blurred clip: the mass sits in bins 0 .. 2
        "noise_hist_yuv_sigma10": lambda: noise_hist_yuv(pay_noisy, fmt, H, W, out=hists),   # spread over the first few dozen bins
        "ingest_u8_bf16": lambda: ingest_u8(u8, torch.bfloat16),
        "egress_yuv_bf16": lambda: egress_yuv(out_bf, fmt, H, W, dst=dst),
        "egress_u8_bf16": lambda: egress_u8(out_bf),
        "egress_yuv_fp32": lambda: egress_yuv(out_32, fmt, H, W, dst=dst),
        "egress_u8_fp32": lambda: egress_u8(out_32),
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

    def run(sig):
        vr = restore.VideoRestorer(net, one_len, sigma=sig, pipeline=True)
        stamps = []
        t0 = time.perf_counter()
        for i, p in enumerate(vr.restore(iter(frames), fmt, H, W)):
            if (i + 1) % one_len == 0:
                stamps.append(time.perf_counter())
        total = time.perf_counter() - t0
        seen[str(sig)] = vr.stats["window_sigma"]
        gaps = [(b - c) * 1e3 for b, c in zip(stamps[1:], stamps[:-1])]
        return {"total_s": total, "window_wall_ms": gaps[1:], "window_forward_ms": vr.stats["window_forward_ms"][2:]}

    run(10.0)                                                                        # warm-up: code objects, engine buffers
    run("auto")
    runs = {"fixed": [], "auto": []}
    for _ in range(a.runs):
        runs["fixed"].append(run(10.0))
        runs["auto"].append(run("auto"))
    res = {}
    for k, rs in runs.items():
        res[k] = {"window_wall_ms": summary([g for r in rs for g in r["window_wall_ms"]]),
                  "window_wall_ms_per_run": [round(statistics.median(r["window_wall_ms"]), 2) for r in rs],
                  "window_forward_ms": summary([g for r in rs for g in r["window_forward_ms"]]), "total_s": [round(r["total_s"], 3) for r in rs]}
    print(json.dumps({"part": "sigma", "variant": "denoise_small", "dtype": "bf16", "one_len": one_len, "windows": nwin, "size": [H, W], "runs": a.runs,
                      "window_sigma_auto": [round(s, 3) for s in seen["auto"]], **res}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kernels", "pipeline", "sigma"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=["both", "pipelined", "serial"], default="both", help="pipeline part: one mode only (for a kernel trace of its own)")
    ap.add_argument("--scene_cuts", choices=["off", "auto", "listed"], default="off", help="pipeline part: VideoRestorer(scene_cuts=...)")
    ap.add_argument("--cut_every", type=int, default=0, help="pipeline part: a cut every N frames in the stream (0: none)")
    a = ap.parse_args()
    with torch.no_grad():
        {"kernels": kernels, "pipeline": pipeline, "sigma": sigma}[a.part](a)
