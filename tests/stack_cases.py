"""The three maximal option stacks of tests/test_gpu_restorer_stack.py and tests/test_host_restorer_stack.py, not a test: their clips, their constructor
arguments, the maps from a written frame to its window and to its number in its scene (from the restatement's plan, tests/time_ref.py), and "the
input as written" built from tests/yuv_ref.py.  numpy only: nothing here touches a device.

  D  denoise_small, bf16, 8-bit centre-sited 4:2:0 in, 10-bit left-sited 4:2:0 out: deflicker, a listed cut, a fixed picture, sigma="auto" with the level curve, the min
     estimator along block vectors, dither, an amount per plane kind, tiles, overlapping windows, grain "auto", the whole report, a 10-bit truth.
  E  denoise_small, fp32, 10-bit 4:4:4 in and out: add_noise with a curve, cuts and picture found ("auto"), the temporal estimator, an ensemble of
     4 x 2 members, windows that share 2 frames, dither, an amount, grain from 16 knots, the whole report with the clean frames for the truth.
  B  deblur_small, bf16, 8-bit left-sited 4:2:0 in and out: add_blur with a listed cut, a fixed picture, an ensemble of 2, overlapping windows, dither,
     the removed view."""
from types import SimpleNamespace

import numpy as np

import deflicker_ref as DF
import picture_ref as P
import time_ref as TR
import yuv_ref as R
from shiftnet_amd import synth
from test_gpu_restorer_options import CUTS

ONE_LEN = 4
F8 = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)
F10 = R.Fmt(10, R.C420_LEFT, R.BT601, R.LIMITED)             # what out_format="420p10" writes: y4m.MODES has that tag left-sited
F10_444 = R.Fmt(10, R.C444, R.BT601, R.LIMITED)
F8_LEFT = R.Fmt(8, R.C420_LEFT, R.BT601, R.LIMITED)
# E's letterboxed clip: the boxed clip of tests/picture_ref.py grown to a picture of 96 x 192, the smallest with two whole NIQE blocks, in two scenes
BOX = dict(h=120, w=192, rect=(0, 12, 192, 96), scenes=((6, 3), (5, 11)))
NOISE_CURVE = [9.0 - 0.3 * b for b in range(16)]             # add_noise: 9 codes at black down to 4.5 at white
GRAIN_CURVE = [3.0 + 0.25 * ((5 * b) % 16) for b in range(16)]      # grain: 16 knots, not monotonic
GRAIN_KEYS = ("grain", "grain_size", "grain_chroma", "grain_seed")
REPORT_KEYS = ("report", "report_motion", "report_quality")


def level_clip(n=11, h=48, w=64, seed=5):
    """noisy_clip of tests/test_gpu_restorer_options.py grown for ``noise_model="level"``: a band of the curve needs 1024 blocks of 2 x 2 in the window
    (noise.NLF_MIN_BLOCKS) and the 22 x 26 rectangle of that file gives 143 a frame, so every curve there is the all-zero one of a window without an
    estimate.  Here the luma ramp moves through two bands only (codes 85 .. 111), the rectangle of the stack is 36 x 52, and its shortest window, of
    6 frames, has 1400 blocks in each."""
    rng = np.random.default_rng(seed)
    ch, cw = R.chroma_shape(F8, h, w)
    x = np.arange(w)[None, :]
    out = []
    for t in range(n):
        Y = 85.0 + 26.0 * ((x + 2 * t + (w // 2 if t >= CUTS[0] else 0)) % w) / w + rng.normal(0.0, 4.0, (h, w))
        U, V = (np.clip(np.rint(128 + rng.normal(0.0, 3.0, (ch, cw))), 16, 240).astype(np.int64) for _ in range(2))
        out.append(R.join_planes(np.clip(np.rint(Y), 16, 235).astype(np.int64), U, V, F8))
    return out


def flickering(pay, fmt, h, w, seed=7):
    """The payloads with their luma under a gain about black of 1 +- 8 %, another for every frame: what deflicker has to take out."""
    gains = 1.0 + np.random.default_rng(seed).uniform(-0.08, 0.08, len(pay))
    yo, top = 16 << (fmt.bits - 8), (1 << fmt.bits) - 1
    out = []
    for p, g in zip(pay, gains):
        Y, U, V = R.split_planes(p, fmt, h, w)
        out.append(R.join_planes(np.clip(np.floor(yo + g * (Y - yo) + 0.5), 0, top).astype(np.int64), U, V, fmt))
    return out


def clean10(n, h, w):
    """A truth for stack D in the format it writes: level_clip's luma ramp without its noise, neutral chroma, 10 bit."""
    ch, cw = R.chroma_shape(F10, h, w)
    x = np.arange(w)[None, :]
    out = []
    for t in range(n):
        Y = np.broadcast_to(85.0 + 26.0 * ((x + 2 * t + (w // 2 if t >= CUTS[0] else 0)) % w) / w, (h, w))
        out.append(R.join_planes(np.rint(4 * Y).astype(np.int64), np.full((ch, cw), 512), np.full((ch, cw), 512), F10))
    return out


def boxed_two_scenes(fmt):
    """BOX: the synthetic sharp clip of two seeds, one per scene, inside the rectangle; bars at black."""
    x0, y0, w, h = BOX["rect"]
    rgb = np.concatenate([synth.sharp_clip(n, h, w, seed) for n, seed in BOX["scenes"]])
    inner = R.egress_emu(np.ascontiguousarray(rgb.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255), fmt, h, w)
    full = np.stack([P.black_payload(fmt, BOX["h"], BOX["w"])] * len(inner))
    return list(P.paste_payloads(full, inner, fmt, BOX["h"], BOX["w"], BOX["rect"]))


def two_scenes(fmt, h, w, scenes=((5, 4), (6, 9))):
    rgb = np.concatenate([synth.sharp_clip(n, h, w, seed) for n, seed in scenes])
    return list(R.egress_emu(np.ascontiguousarray(rgb.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255), fmt, h, w))


def stack_d():
    pay = flickering(level_clip(), F8, 48, 64)
    kw = dict(sigma="auto", noise_model="level", sigma_estimator="min", sigma_motion="blocks", deflicker=2, scene_cuts=list(CUTS), picture=(6, 4, 52, 36),
              out_format="420p10", dither="tpdf", dither_seed=7, amount=(0.7, 0.4), tile=(16, 16), tile_overlap=4, window_overlap=1,
              grain="auto:0.5", grain_size=0.8, grain_chroma=0.5, grain_seed=5, report=True, report_motion="blocks", report_quality="niqe")
    return SimpleNamespace(name="D", variant="denoise_small", dtype="bf16", fmt=F8, ofmt=F10, h=48, w=64, pay=pay, gt=clean10(len(pay), 48, 64), kw=kw,
                           cuts=list(CUTS), V=1, rect=(6, 4, 52, 36), other_rect=(10, 8, 44, 32), stage="deflicker",
                           stage_keys=("deflicker", "deflicker_chroma"), stage_stats=("deflicker", "deflicker_chroma", "deflicker_launches", "frame_deflicker"),
                           tiled=True, mix=("amount", 0.7, 0.4))


def stack_e():
    pay = boxed_two_scenes(F10_444)
    kw = dict(sigma="auto", sigma_estimator="temporal", add_noise=list(NOISE_CURVE), add_noise_seed=11, scene_cuts="auto", picture="auto", bar_level=8.0,
              ensemble=4, ensemble_time=True, window_overlap=2, dither="tpdf", dither_seed=3, amount=0.6, grain=list(GRAIN_CURVE), grain_size=0.6,
              grain_chroma=0.25, grain_seed=9, report=True, report_motion="blocks", report_quality="niqe")
    return SimpleNamespace(name="E", variant="denoise_small", dtype="fp32", fmt=F10_444, ofmt=F10_444, h=BOX["h"], w=BOX["w"], pay=pay, gt=None, kw=kw,
                           cuts=[BOX["scenes"][0][0]], V=2, rect=BOX["rect"], other_rect=(16, 12, 160, 96), stage="add_noise",
                           stage_keys=("add_noise", "add_noise_seed"), stage_stats=("add_noise", "add_noise_seed", "degrade_launches"), tiled=False,
                           mix=("amount", 0.6, 0.6))


def stack_b():
    pay = two_scenes(F8_LEFT, 48, 64)
    kw = dict(add_blur=5, scene_cuts=[5], picture=(8, 6, 48, 36), ensemble=2, window_overlap=1, dither="tpdf", dither_seed=21, view="removed", removed_gain=4)
    return SimpleNamespace(name="B", variant="deblur_small", dtype="bf16", fmt=F8_LEFT, ofmt=F8_LEFT, h=48, w=64, pay=pay, gt=None, kw=kw, cuts=[5], V=1,
                           rect=(8, 6, 48, 36), other_rect=(4, 2, 40, 30), stage="add_blur", stage_keys=("add_blur", "add_blur_gamma"),
                           stage_stats=("add_blur", "add_blur_gamma", "blur_launches"), tiled=False, mix=("removed", 4.0, 4.0))


STACKS = {"D": stack_d, "E": stack_e, "B": stack_b}


# ---- the maps the GPU file uses -----------------------------------------------------------------------------------------------------------
def frame_maps(n, cuts, V, one_len=ONE_LEN):
    """From the restatement's plan: per written frame (its window, its number counted from the start of its scene), and per window (its first written
    frame, the frames it writes, the scene's first frame)."""
    frames, wins = [], []
    for k, (lo, cnt, idx, head, wr) in enumerate(TR.scene_plan(n, one_len, list(cuts), V)):
        a = max([0] + [c for c in cuts if c <= lo])
        assert lo == len(frames)                                   # every frame is written once and in order
        frames += [(k, f - a) for f in range(lo, lo + wr)]
        wins.append((lo, wr, a))
    assert len(frames) == n
    return frames, wins


def windows_before(n, cuts, V, cut, one_len=ONE_LEN):
    """How many windows of the plan lie in front of the scene start ``cut``."""
    return sum(1 for lo, *_ in TR.scene_plan(n, one_len, list(cuts), V) if lo < cut)


# ---- the references of the front stages and of "the input as written" -------------------------------------------------------------------------
def deflickered_ref(pay, fmt, h, w, radius, cuts=(), chroma="gain"):
    """(the payloads, the four numbers of every frame) that tests/deflicker_ref.py makes of the stream, every listed scene a clip of its own."""
    hists = DF.hist_ref(pay, fmt, h, w)
    starts = [0] + list(cuts) + [len(pay)]
    out, info = [], []
    for lo, hi in zip(starts[:-1], starts[1:]):
        lut, i = DF.tables_ref(hists, lo, hi, radius, fmt.bits, fmt.range == R.FULL, chroma)
        out += list(DF.apply_ref(pay[lo:hi], lut, fmt, h, w))
        info += i
    return out, info


def converted(pay, fmt, ofmt, h, w):
    """Payloads of ``fmt`` -> payloads of ``ofmt``: ``egress(out format, ingest_float32(in format, frame))``, undithered."""
    return R.egress_emu(R.ingest_emu(np.stack(pay), fmt, h, w, h, w), ofmt, h, w)


def as_written(st, fed, rects):
    """The input as written: per frame of ``fed`` (the payloads the stages in front hand on) the payload in the format written.  The payload itself
    where the format stays; else the whole frame converted, and under tiles, inside the frame's rectangle ``rects[i]``, the rectangle converted as the
    cropped stream's frames are."""
    if st.ofmt == st.fmt:
        return [np.asarray(p) for p in fed]
    out = list(converted(fed, st.fmt, st.ofmt, st.h, st.w))
    if st.tiled:
        for i, r in enumerate(rects):
            if r is not None:
                inner = converted(P.crop_payloads(np.stack([fed[i]]), st.fmt, st.h, st.w, r), st.fmt, st.ofmt, r[3], r[2])
                out[i] = P.paste_payloads(out[i][None], inner, st.ofmt, st.h, st.w, r)[0]
    return out
