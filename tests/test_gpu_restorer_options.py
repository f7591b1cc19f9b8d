"""-m gpu: the video restorer with every option on at once -- listed scene cuts, a picture, ``sigma="auto"``, ``noise_model="level"``, another output
format and dither ("first"), and on top of those an amount, the temporal estimate along block vectors, the report with its motion part and tiles
("second") -- against itself: the pipeline on and off, and a second ``restore()`` on the same object.  Bytes and the records in ``stats`` are
compared with ==: they come from the same kernels on the same inputs, so no tolerance appears; the four records of the report that hold nan where a
pair crosses a window are compared by ``repr()``, which is as strict for every other float64.  What the bytes should be is the business of the
per-feature files (test_gpu_yuv / scenes / noise / picture / dither / nlf / mix / noise_pairs / motion / diff_stats / diff_stats_mv / tiles)."""
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
MORE = dict(OPTIONS, amount=0.7, sigma_estimator="min", sigma_motion="blocks", report=True, report_motion="blocks")      # ... plus the case's tiles
TIMING = ("forward_s", "window_forward_ms", "picture_wait_ms")
NAN_KEYS = ("frame_report", "report_summary", "frame_report_motion", "report_motion_summary")      # nan where a pair crosses a window


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


# the clip, its size, the picture argument, the windows of scenes [0, 5) and [5, n) at one_len 4, the rectangle every window reports, and the tiles of
# the second option set: the 22 x 26 rectangle pads to 24 x 28 and takes 2 x 2 tiles of 16 x 16 at y in {0, 8}, x in {0, 12} (its windows write 4, 1, 4
# and 2 frames: the report's pairs occur and do not); the 72 x 128 one takes 2 x 3 tiles of 40 x 64
CASES = {
    "listed_picture": lambda: (noisy_clip(), 40, 48, (6, 4, 26, 22), 4, (6, 4, 26, 22), dict(tile=(16, 16), tile_overlap=4), 4),
    "auto_picture": lambda: (boxed_clip(), P.BOXED["h"], P.BOXED["w"], "auto", 3, P.BOXED["rect"], dict(tile=(40, 64), tile_overlap=8), 6),
}


def records(stats):
    return {k: (repr(v) if k in NAN_KEYS else v) for k, v in stats.items() if k not in TIMING}


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def net():
    return restore.load_net("denoise_small", "synthetic", "bf16")


@pytest.fixture(scope="module", params=list(CASES) + [c + "-more" for c in CASES])
def runs(request, net):
    """Per pipeline setting, the (payloads, stats) of two restore() calls in a row on one object.  Shared by the tests below and left unchanged."""
    case, _, more = request.param.partition("-")
    pay, h, w, picture, windows, rect, tiles, per_window = CASES[case]()
    options = dict(MORE, **tiles) if more else OPTIONS
    got = {}
    for pipeline in (True, False):
        vr = restore.VideoRestorer(net, ONE_LEN, pipeline=pipeline, picture=picture, **options)
        got[pipeline] = []
        for _ in range(2):
            out = list(vr.restore(iter(pay), yuv_fmt(*FMT), h, w))
            got[pipeline].append((out, dict(vr.stats)))
    return pay, h, w, picture, windows, rect, (per_window if more else None), got


def test_every_option_is_on_and_recorded(runs):
    pay, h, w, picture, windows, rect, per_window, got = runs
    out, stats = got[True][0]
    assert len(out) == len(pay) == stats["frames"] and stats["windows"] == windows and stats["cuts"] == CUTS
    assert all(p.size == 2 * pay[0].size for p in out)                                          # 10 bit out of 8 bit in, the same chroma layout
    assert stats["window_picture"] == [rect] * windows and stats["picture_launches"] == (windows if picture == "auto" else 0)
    assert ("picture_wait_ms" in stats) == (picture == "auto")
    assert stats["nlf_launches"] == stats["nlf_map_launches"] == windows
    assert stats["noise_launches"] == (windows if per_window is None else 2 * windows)          # the second set's block matcher counts as one
    assert len(stats["window_sigma"]) == len(stats["window_frame_sigma"]) == len(stats["window_nlf"]) == windows
    assert (stats["out_format"], stats["dither"], stats["dither_seed"]) == ("420p10", "tpdf", 7) and stats["cuts_ignored"] == []
    if per_window is None:
        assert stats["amount"] is None and not any(k in stats for k in ("report_launches", "tile_launches", "window_pair_sigma", "window_pair_motion"))
        return
    assert stats["amount"] == (0.7, 0.7) and stats["sigma_estimator"] == "min" and stats["sigma_motion"] == stats["report_motion"] == "blocks"
    assert stats["report_launches"] == windows and len(stats["frame_sums"]) == len(stats["frame_report"]) == len(stats["pair_sums_mv"]) == len(pay)
    assert len(stats["window_pair_sigma"]) == len(stats["window_pair_motion"]) == windows
    assert stats["noise_pairs_launches"] == stats["nlf_pairs_launches"] == windows
    # every window runs its tiles once, and once more where the range guard tripped
    assert all(len(t) == per_window for t in stats["window_tiles"]) and len(stats["window_tiles"]) == windows
    assert stats["tile_launches"] % per_window == 0 and windows <= stats["tile_launches"] // per_window <= 2 * windows


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
