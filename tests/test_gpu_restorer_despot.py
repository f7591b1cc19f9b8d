"""-m gpu: the video restorer with ``despot``: a stage in front of everything else, behind ``deflicker``.  The chain equality: the run writes the bytes
of the plain restorer fed the payloads that the restatement (tests/despot_ref.py: its own vectors from motion_ref, the rule in numpy, clip ends and
the guard) makes of the stream -- whatever the chunks (one_len 4: every frame's neighbours straddle a chunk boundary somewhere), with a listed cut,
at 10 bit, with chroma off and behind deflicker; ``despotted=`` sees exactly those payloads and ``stats["frame_despot"]`` the restatement's records;
a static clip leaves as it came, a flash frame is kept by the guard; and a run without the option has the stats keys and the launches it had.
Shift-Net-s deblur with synthetic weights, bf16, a 48 x 64 stream of 14 frames of synth.sharp_clip (a pan) with square blotches planted, one_len 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

import despot_ref as DR
import scene_ref as S
import yuv_ref as R
from shiftnet_amd import restore, synth, y4m
from shiftnet_amd.io_edges import yuv_fmt
from test_gpu_restorer_deflicker import deflickered_ref, flickering
from test_gpu_restorer_degrade import DEFAULT_KEYS, same
from test_host_despot import plant, squares_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FRAMES, ONE_LEN, T = 48, 64, 14, 4, 24
F10 = R.Fmt(10, R.C420_CENTER, R.BT601, R.LIMITED)
KEYS = ("despot", "despot_support", "despot_grow", "despot_chroma", "despot_max_share", "frame_despot", "despot_launches")
DIRTY = (0, 2, 5, 6, 7, 9, 12, 13)                               # 0 and 13 are the stream's ends, 7 a listed scene's start, 5 and 6 follow each other


def dirty(pay, fmt):
    """The payloads with up to two square blotches planted in each frame of DIRTY, other ones in every frame -- and up to five in frame 12: more
    than a twentieth of a 48 x 64 frame, which the guard keeps."""
    out = [np.array(p, copy=True) for p in pay]
    for f in DIRTY:
        sq = squares_for(out[f], fmt, seed=40 + f, count=5 if f == 12 else 2, h=H, w=W)
        assert sq
        out[f] = plant(out[f], fmt, sq, h=H, w=W)
    return out


@pytest.fixture(scope="module")
def net():
    return restore.load_net("deblur_small", "synthetic", "bf16")


@pytest.fixture(scope="module")
def pay8():
    return dirty(S.payloads_of(synth.sharp_clip(FRAMES, H, W, 4), H, W, S.FMT420), S.FMT420)


def run(net, pay, fmt=S.FMT420, tap=False, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    seen = []
    more = {"despotted": lambda p: seen.append(p.copy())} if tap else {}
    return list(vr.restore(iter(pay), yuv_fmt(*fmt), H, W, **more)), vr.stats, seen, dict(vr.run.launches)


CASES = {"pipelined": (S.FMT420, {}), "serial": (S.FMT420, dict(pipeline=False)), "a listed cut": (S.FMT420, dict(scene_cuts=[7])),
         "420p10": (F10, {}), "chroma off": (S.FMT420, dict(despot_chroma="off")), "behind deflicker": (S.FMT420, dict(deflicker=3))}


@pytest.mark.parametrize("case", list(CASES))
def test_the_run_is_the_plain_run_on_the_restatements_payloads(net, pay8, case):
    fmt, kw = CASES[case]
    pay = pay8 if fmt is S.FMT420 else dirty(S.payloads_of(synth.sharp_clip(FRAMES, H, W, 4), H, W, fmt), fmt)
    cuts = kw.get("scene_cuts", ())
    first, launches_deflicker = pay, 0
    if "deflicker" in kw:                                            # flicker goes first: despot's restatement applied to deflicker's
        pay = dirty(flickering(fmt), fmt)
        first, _ = deflickered_ref(pay, fmt, radius=kw["deflicker"])
        launches_deflicker = 7                                       # test_gpu_restorer_deflicker.py derives it: 14 frames, R = 3, chunks of 4
        assert not same(first, pay)
    want, wrec = DR.despot_stream_ref(first, fmt, H, W, cuts=cuts, T=T, K=2, G=1, chroma=kw.get("despot_chroma", "follow"), max_share=0.05)
    assert not same(want, first) and sum(1 for r in wrec if r[1]) >= 4
    got, stats, seen, launches = run(net, pay, fmt, tap=True, despot=T, **kw)
    assert len(got) == len(seen) == FRAMES and same(seen, want)      # despotted= sees the stage's payloads, and they are the restatement's
    plain, pstats, _, plaunches = run(net, want, fmt, **{k: v for k, v in kw.items() if k not in ("despot_chroma", "deflicker")})
    assert same(got, plain)
    assert stats["frame_despot"] == wrec                             # (seeds, replaced, share, kept), the float bit for bit
    mine = set(KEYS) | ({"deflicker", "deflicker_chroma", "deflicker_launches", "frame_deflicker"} if "deflicker" in kw else set())
    assert set(stats) - mine == set(pstats) and not any(k in pstats for k in KEYS)
    assert (stats["despot"], stats["despot_support"], stats["despot_grow"], stats["despot_max_share"]) == (T, 2, 1, 0.05)
    assert stats["despot_chroma"] == kw.get("despot_chroma", "follow")
    # 14 frames in chunks of 4 with one read ahead: the chunks make frames 0 .. 3, 4 .. 7, 8 .. 11 and 12 .. 13.  Without a cut each is one scene
    # segment with a frame that has two neighbours (1 .. 3, 4 .. 7, 8 .. 11, 12): two motion launches and one repair launch each, 12.  With the cut
    # listed at 7 the second chunk has the segments 4 .. 6 (4 and 5 repaired, 6 the scene's last) and 7 (the scene's first: nothing but a copy, no
    # launch): again 2 + 1, and 12 in all.  A fifth pass reads nothing and makes nothing.
    assert stats["despot_launches"] == launches["despot"] == 12 and plaunches["despot"] == 0
    assert launches["deflicker"] == launches_deflicker
    rest = lambda d: {k: v for k, v in d.items() if k not in ("despot", "deflicker")}      # noqa: E731
    assert rest(launches) == rest(plaunches)
    ends = (0, 6, 7, 13) if cuts else (0, 13)                        # a clip's first and last frame are the source's, dirt and all
    assert all(wrec[f] == (0, 0, 0.0, False) and np.array_equal(seen[f], first[f]) for f in ends)


def test_a_static_clip_equals_the_run_without_the_option_and_the_guard_keeps_a_flash_frame(net, pay8):
    static = [pay8[3]] * 9
    base, bstats, _, _ = run(net, static)
    got, stats, seen, launches = run(net, static, tap=True, despot=1, despot_support=0, despot_grow=2)
    assert same(seen, static) and same(got, base) and stats["frame_despot"] == [(0, 0, 0.0, False)] * 9
    # the chunks make frames 0 .. 3, 4 .. 7 and 8: the last is nothing but the clip's last frame and launches nothing
    assert launches["despot"] == stats["despot_launches"] == 6
    Y, U, V = R.split_planes(pay8[3], S.FMT420, H, W)
    flash = list(static)
    flash[4] = R.join_planes(np.minimum(Y + 90, 255), U, V, S.FMT420)
    want, wrec = DR.despot_stream_ref(flash, S.FMT420, H, W, T=T, K=2, G=1, max_share=0.05)
    got, stats, seen, _ = run(net, flash, tap=True, despot=T)
    assert wrec[4][3] and same(want, flash)                          # the restatement keeps it ...
    assert same(seen, flash) and stats["frame_despot"] == wrec        # ... and the stage hands on the host's bytes
    want, wrec = DR.despot_stream_ref(flash, S.FMT420, H, W, T=T, K=2, G=1, max_share=1.0)
    got, stats, seen, _ = run(net, flash, tap=True, despot=T, despot_max_share=1.0)
    assert not wrec[4][3] and not same(want, flash) and same(seen, want) and stats["frame_despot"] == wrec


def test_a_run_without_the_option_has_the_keys_and_launches_it_had_and_the_refusals_name_both_options(net, pay8):
    dn = restore.load_net("denoise_small", "synthetic", "bf16")
    out, stats, _, launches = run(dn, pay8[:9], sigma=10.0)
    assert len(out) == 9 and sorted(stats) == DEFAULT_KEYS and launches["despot"] == 0
    out, stats, _, launches = run(net, pay8[:9])
    assert not any(k in stats for k in KEYS) and set(stats) <= set(DEFAULT_KEYS) and launches["despot"] == 0
    with pytest.raises(ValueError, match=r"despot together with add_noise"):
        restore.VideoRestorer(net, ONE_LEN, despot=T, add_noise=10)
    with pytest.raises(ValueError, match=r"despot together with add_blur"):
        restore.VideoRestorer(net, ONE_LEN, despot=T, add_blur=5)
    for bad in (0, 256, 2.5, "24", True):
        with pytest.raises(ValueError, match="despot"):
            restore.VideoRestorer(net, ONE_LEN, despot=bad)
    for kw, word in ((dict(despot_support=9), "despot_support"), (dict(despot_grow=3), "despot_grow"), (dict(despot_chroma="gain"), "despot_chroma"),
                     (dict(despot_max_share=0), "despot_max_share")):
        with pytest.raises(ValueError, match=word):
            restore.VideoRestorer(net, ONE_LEN, despot=T, **kw)
    with pytest.raises(ValueError, match=r"despot_grow.*needs despot"):
        restore.VideoRestorer(net, ONE_LEN, despot_grow=2)
    with pytest.raises(ValueError, match=r"despotted.*needs despot"):
        list(restore.VideoRestorer(net, ONE_LEN).restore(iter(pay8), yuv_fmt(*S.FMT420), H, W, despotted=print))


def test_restore_video_cli_writes_the_api_bytes_and_the_numbers_of_every_frame(net, pay8, tmp_path):
    out, stats, _, _ = run(net, pay8, despot=T)
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, dout = (tmp_path / n for n in ("in.y4m", "out.y4m", "despot.txt"))
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay8:
            wr.write(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic", "--dtype", "bf16",
                        "--one_len", str(ONE_LEN), "--despot", str(T), "--despot_out", str(dout), str(src), str(dst)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"despot (T {T}, K 2, G 1, chroma follow): median share replaced" in r.stderr
    with open(dst, "rb") as fh:
        rd = y4m.Y4MReader(fh)
        got = list(rd)
    assert rd.header.line() == hd.line() and same(got, out)          # 48 < 720: the CLI's default matrix is BT.601, as FMT420
    lines = open(dout).read().splitlines()
    assert len(lines) == FRAMES + 1 and lines[-1].startswith("# median share replaced: ")
    for line, (seeds, replaced, share, kept) in zip(lines, stats["frame_despot"]):
        assert line == "%d %d %.6f %d" % (seeds, replaced, share, kept)
