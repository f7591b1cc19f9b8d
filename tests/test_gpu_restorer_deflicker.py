"""-m gpu: the video restorer with ``deflicker``: a stage in front of everything else.  The chain equality: the run writes the bytes of the plain
restorer fed the payloads that the restatement's tables (tests/deflicker_ref.py), applied with numpy, make of the stream -- whatever the chunks (R = 3
and one_len 4: every window of the rule straddles a chunk boundary), with a listed cut, and at 10 bit; a static clip leaves as it came; and a run
without the option has the stats keys and the launches it had.  Shift-Net-s deblur with synthetic weights, bf16, a 48 x 64 stream of 14 frames whose
luma flickers by +-8 %, one_len 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

import deflicker_ref as DR
import scene_ref as S
import yuv_ref as R
from shiftnet_amd import restore, synth, y4m
from shiftnet_amd.io_edges import yuv_fmt
from test_gpu_restorer_degrade import DEFAULT_KEYS, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FRAMES, ONE_LEN, RADIUS = 48, 64, 14, 4, 3
F10 = R.Fmt(10, R.C420_CENTER, R.BT601, R.LIMITED)
KEYS = ("deflicker", "deflicker_chroma", "deflicker_launches", "frame_deflicker")


def flickering(fmt):
    """FRAMES payloads of a moving clip whose luma is under a gain about black of 1 +- 8 %, another for every frame."""
    pay = S.payloads_of(synth.sharp_clip(FRAMES, H, W, 4), H, W, fmt)
    gains = 1.0 + np.random.default_rng(7).uniform(-0.08, 0.08, FRAMES)
    yo, top = 16 << (fmt.bits - 8), (1 << fmt.bits) - 1
    out = []
    for p, g in zip(pay, gains):
        Y, U, V = R.split_planes(p, fmt, H, W)
        out.append(R.join_planes(np.clip(np.floor(yo + g * (Y - yo) + 0.5), 0, top).astype(np.int64), U, V, fmt))
    return out


def deflickered_ref(pay, fmt, radius=RADIUS, cuts=(), chroma="gain"):
    """(the payloads, the four numbers of every frame) that the restatement makes of the stream, every scene a clip of its own."""
    hists = DR.hist_ref(pay, fmt, H, W)
    starts = [0] + list(cuts) + [len(pay)]
    out, info = [], []
    for lo, hi in zip(starts[:-1], starts[1:]):
        lut, i = DR.tables_ref(hists, lo, hi, radius, fmt.bits, fmt.range == R.FULL, chroma)
        out += list(DR.apply_ref(pay[lo:hi], lut, fmt, H, W))
        info += i
    return out, info


@pytest.fixture(scope="module")
def net():
    return restore.load_net("deblur_small", "synthetic", "bf16")


@pytest.fixture(scope="module")
def pay8():
    return flickering(S.FMT420)


def run(net, pay, fmt=S.FMT420, tap=False, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    seen = []
    more = {"deflickered": lambda p: seen.append(p.copy())} if tap else {}
    return list(vr.restore(iter(pay), yuv_fmt(*fmt), H, W, **more)), vr.stats, seen, dict(vr.run.launches)


CASES = {"pipelined": (S.FMT420, {}), "serial": (S.FMT420, dict(pipeline=False)), "a listed cut": (S.FMT420, dict(scene_cuts=[7])),
         "420p10": (F10, {}), "chroma off": (S.FMT420, dict(deflicker_chroma="off"))}


@pytest.mark.parametrize("case", list(CASES))
def test_the_run_is_the_plain_run_on_the_restatements_payloads(net, pay8, case):
    fmt, kw = CASES[case]
    pay = pay8 if fmt is S.FMT420 else flickering(fmt)
    want, winfo = deflickered_ref(pay, fmt, cuts=kw.get("scene_cuts", ()), chroma=kw.get("deflicker_chroma", "gain"))
    assert not same(want, pay)
    got, stats, seen, launches = run(net, pay, fmt, tap=True, deflicker=RADIUS, **kw)
    assert len(got) == len(seen) == FRAMES and same(seen, want)      # deflickered= sees the stage's payloads, and they are the restatement's
    plain, pstats, _, plaunches = run(net, want, fmt, **{k: v for k, v in kw.items() if k != "deflicker_chroma"})
    assert same(got, plain)
    assert stats["frame_deflicker"] == winfo                         # (r, mean_in, mean_out, chroma_gain), floats bit for bit
    assert set(stats) - set(KEYS) == set(pstats) and not any(k in pstats for k in KEYS)
    assert stats["deflicker"] == RADIUS and stats["deflicker_chroma"] == kw.get("deflicker_chroma", "gain")
    # 14 frames in chunks of 4 with 3 read ahead: 7, 4 and 3 new frames, then a closing chunk with none -- two launches per chunk, one for that one
    assert stats["deflicker_launches"] == launches["deflicker"] == 7 and plaunches["deflicker"] == 0
    assert {k: v for k, v in launches.items() if k != "deflicker"} == {k: v for k, v in plaunches.items() if k != "deflicker"}
    if "scene_cuts" in kw:                                            # the window does not cross the cut: the frames beside it leave as they came
        assert [i[0] for i in winfo] == [0, 1, 2, 3, 2, 1, 0] * 2 and same([seen[6], seen[7]], [pay[6], pay[7]])


def test_two_launches_per_chunk_where_every_chunk_has_new_frames(net, pay8):
    got, stats, seen, _ = run(net, pay8, tap=True, deflicker=1)      # 5, 4, 4 and 1 new frames
    assert stats["deflicker_launches"] == 8 and stats["windows"] == 4 and same(seen, deflickered_ref(pay8, S.FMT420, radius=1)[0])
    got, stats, seen, _ = run(net, pay8[:2], tap=True, deflicker=15)      # a stream shorter than R, and than the chunk
    assert len(got) == 2 and stats["deflicker_launches"] == 2 and same(seen, pay8[:2]) and [i[0] for i in stats["frame_deflicker"]] == [0, 0]


def test_a_static_clip_equals_the_run_without_the_option_byte_for_byte(net, pay8):
    static = [pay8[3]] * 9
    base, bstats, _, _ = run(net, static)
    got, stats, seen, _ = run(net, static, tap=True, deflicker=RADIUS)
    assert same(seen, static) and same(got, base)
    assert all(i[3] == 1.0 and i[1] == i[2] for i in stats["frame_deflicker"])


def test_a_run_without_the_option_has_the_keys_and_launches_it_had_and_the_refusals_name_both_options(net, pay8):
    dn = restore.load_net("denoise_small", "synthetic", "bf16")
    out, stats, _, launches = run(dn, pay8[:9], sigma=10.0)
    assert len(out) == 9 and sorted(stats) == DEFAULT_KEYS and launches["deflicker"] == 0
    out, stats, _, launches = run(net, pay8[:9])
    assert not any(k in stats for k in KEYS) and set(stats) <= set(DEFAULT_KEYS) and launches["deflicker"] == 0
    with pytest.raises(ValueError, match=r"deflicker together with add_noise"):
        restore.VideoRestorer(net, ONE_LEN, deflicker=3, add_noise=10)
    with pytest.raises(ValueError, match=r"deflicker together with add_blur"):
        restore.VideoRestorer(net, ONE_LEN, deflicker=3, add_blur=5)
    for bad in (0, 16, 2.5, "3", True):
        with pytest.raises(ValueError, match="deflicker"):
            restore.VideoRestorer(net, ONE_LEN, deflicker=bad)
    with pytest.raises(ValueError, match="deflicker_chroma"):
        restore.VideoRestorer(net, ONE_LEN, deflicker=3, deflicker_chroma="mean")
    with pytest.raises(ValueError, match=r"deflickered.*needs deflicker"):
        list(restore.VideoRestorer(net, ONE_LEN).restore(iter(pay8), yuv_fmt(*S.FMT420), H, W, deflickered=print))


def test_restore_video_cli_writes_the_api_bytes_and_the_numbers_of_every_frame(net, pay8, tmp_path):
    out, stats, _, _ = run(net, pay8, deflicker=RADIUS)
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, dout = (tmp_path / n for n in ("in.y4m", "out.y4m", "deflicker.txt"))
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay8:
            wr.write(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic", "--dtype", "bf16",
                        "--one_len", str(ONE_LEN), "--deflicker", str(RADIUS), "--deflicker_out", str(dout), str(src), str(dst)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"deflicker (R {RADIUS}, chroma gain): rms second difference of the frame means" in r.stderr
    with open(dst, "rb") as fh:
        rd = y4m.Y4MReader(fh)
        got = list(rd)
    assert rd.header.line() == hd.line() and same(got, out)          # 48 < 720: the CLI's default matrix is BT.601, as FMT420
    lines = open(dout).read().splitlines()
    assert len(lines) == FRAMES + 1 and lines[-1].startswith("# rms second difference of the frame means: ")
    for line, (rr, m_in, m_out, k) in zip(lines, stats["frame_deflicker"]):
        assert line == "%d %.4f %.4f %.6f" % (rr, m_in, m_out, k)
