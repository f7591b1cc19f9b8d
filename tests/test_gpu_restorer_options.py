"""-m gpu: the video restorer with every option on at once -- listed scene cuts, a picture, ``sigma="auto"``, ``noise_model="level"``, another output
format and dither -- against itself: the pipeline on and off, and a second ``restore()`` on the same object.  Bytes and the records in ``stats`` are
compared with ==: they come from the same kernels on the same inputs, so no tolerance appears.  What the bytes should be is the business of the
per-feature files (test_gpu_yuv / scenes / noise / picture / dither / nlf)."""
import numpy as np
import pytest

import picture_ref as P
import yuv_ref as R
from shiftnet_amd import restore, synth
from shiftnet_amd.io_edges import yuv_fmt

pytestmark = pytest.mark.gpu

FMT = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)
ONE_LEN, CUTS = 4, [5]
OPTIONS = dict(scene_cuts=CUTS, sigma="auto", noise_model="level", out_format="420p10", dither="tpdf", dither_seed=7)
TIMING = ("forward_s", "window_forward_ms", "picture_wait_ms")


def noisy_clip(n=11, h=40, w=48, seed=5):
    """n frames of h x w: a luma ramp from left to right that moves a little from frame to frame and jumps at the cut, noise of 4 codes, noisy chroma."""
    rng = np.random.default_rng(seed)
    ch, cw = R.chroma_shape(FMT, h, w)
    x = np.arange(w)[None, :]
    out = []
    for t in range(n):
        Y = 40.0 + 150.0 * ((x + 2 * t + (w // 2 if t >= CUTS[0] else 0)) % w) / w + rng.normal(0.0, 4.0, (h, w))
        U, V = (np.clip(np.rint(128 + rng.normal(0.0, 3.0, (ch, cw))), 16, 240).astype(np.int64) for _ in range(2))
        out.append(R.join_planes(np.clip(np.rint(Y), 16, 235).astype(np.int64), U, V, FMT))
    return out


def boxed_clip(seed=3, sigma=4.0):
    """The boxed clip of tests/picture_ref.py -- 7 frames of 96 x 128, the picture in (0, 12, 128, 72), bars at black -- with noise inside the picture."""
    b = P.BOXED
    rgb = synth.sharp_clip(b["n"], b["rect"][3], b["rect"][2], seed).astype(np.float64)
    rgb = np.clip(np.rint(rgb + np.random.default_rng(seed).normal(0.0, sigma, rgb.shape)), 0, 255).astype(np.uint8)
    return list(P.boxed_payloads(FMT, rgb))


# the clip, its size, the picture argument, the windows of scenes [0, 5) and [5, n) at one_len 4, the rectangle every window reports
CASES = {
    "listed_picture": lambda: (noisy_clip(), 40, 48, (6, 4, 26, 22), 4, (6, 4, 26, 22)),
    "auto_picture": lambda: (boxed_clip(), P.BOXED["h"], P.BOXED["w"], "auto", 3, P.BOXED["rect"]),
}


def records(stats):
    return {k: v for k, v in stats.items() if k not in TIMING}


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def net():
    return restore.load_net("denoise_small", "synthetic", "bf16")


@pytest.fixture(scope="module", params=list(CASES))
def runs(request, net):
    """Per pipeline setting, the (payloads, stats) of two restore() calls in a row on one object.  Shared by the tests below and left unchanged."""
    pay, h, w, picture, windows, rect = CASES[request.param]()
    got = {}
    for pipeline in (True, False):
        vr = restore.VideoRestorer(net, ONE_LEN, pipeline=pipeline, picture=picture, **OPTIONS)
        got[pipeline] = []
        for _ in range(2):
            out = list(vr.restore(iter(pay), yuv_fmt(*FMT), h, w))
            got[pipeline].append((out, dict(vr.stats)))
    return pay, h, w, picture, windows, rect, got


def test_every_option_is_on_and_recorded(runs):
    pay, h, w, picture, windows, rect, got = runs
    out, stats = got[True][0]
    assert len(out) == len(pay) == stats["frames"] and stats["windows"] == windows and stats["cuts"] == CUTS
    assert all(p.size == 2 * pay[0].size for p in out)                                          # 10 bit out of 8 bit in, the same chroma layout
    assert stats["window_picture"] == [rect] * windows and stats["picture_launches"] == (windows if picture == "auto" else 0)
    assert ("picture_wait_ms" in stats) == (picture == "auto")
    assert stats["noise_launches"] == stats["nlf_launches"] == stats["nlf_map_launches"] == windows
    assert len(stats["window_sigma"]) == len(stats["window_frame_sigma"]) == len(stats["window_nlf"]) == windows
    assert (stats["out_format"], stats["dither"], stats["dither_seed"]) == ("420p10", "tpdf", 7) and stats["cuts_ignored"] == []


def test_pipeline_on_and_off_give_the_same_bytes_and_records(runs):
    got = runs[-1]
    (piped, pstats), (serial, sstats) = got[True][0], got[False][0]
    assert same(piped, serial)
    assert records(pstats) == records(sstats) and set(pstats) == set(sstats)


@pytest.mark.parametrize("pipeline", [True, False])
def test_a_second_restore_on_the_same_object_repeats_the_first(runs, pipeline):
    (first, fstats), (second, sstats) = runs[-1][pipeline]
    assert same(first, second)
    assert records(fstats) == records(sstats) and set(fstats) == set(sstats)
