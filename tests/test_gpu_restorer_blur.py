"""-m gpu: the video restorer with ``add_blur``: a stage in front of everything else.  The run is the plain run on the blurred payloads with the sharp
ones as ``gt``; the blurred payloads are the numpy restatement's of the whole stream (tests/blur_ref.py), whatever the chunks -- at n = 5 and one_len 4
every window of the blur straddles a chunk boundary; a listed cut makes two streams of it; and a run without the option has the stats keys it had.
Shift-Net-s deblur with synthetic weights, bf16, the 48 x 64 stream of 9 frames of test_gpu_restorer_degrade.py, one_len 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

import blur_ref as B
import scene_ref as S
from shiftnet_amd import report, restore, synth, y4m
from shiftnet_amd.io_edges import yuv_fmt
from test_gpu_restorer_degrade import DEFAULT_KEYS, FRAMES, H, ONE_LEN, W, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, GAMMA = 5, 2.2
KEYS = ("add_blur", "add_blur_gamma", "blur_launches")


@pytest.fixture(scope="module")
def clip():
    """(the network, the sharp payloads)."""
    return restore.load_net("deblur_small", "synthetic", "bf16"), list(S.payloads_of(synth.sharp_clip(FRAMES, H, W, 4), H, W))


def run(net, pay, one_len=ONE_LEN, gt=None, tap=False, **kw):
    vr = restore.VideoRestorer(net, one_len, **kw)
    seen = []
    more = ({} if gt is None else {"gt": iter(gt)})
    if tap:
        more["degraded"] = lambda p: seen.append(p.copy())
    return list(vr.restore(iter(pay), yuv_fmt(*S.FMT420), H, W, **more)), vr.stats, seen


@pytest.fixture(scope="module")
def blurred(clip):
    net, pay = clip
    return run(net, pay, tap=True, add_blur=N, report=True)


def test_the_run_is_the_plain_run_on_the_blurred_payloads_with_the_sharp_ones_as_truth(clip, blurred):
    net, pay = clip
    out, stats, seen = blurred
    assert len(out) == len(seen) == FRAMES and not same(seen, pay)
    # the stage's payloads are the restatement's of the whole stream: chunks of one_len, every window across a chunk boundary
    assert same(seen, list(B.blur_stream(pay, S.FMT420, H, W, N, GAMMA)))
    plain, pstats, _ = run(net, seen, gt=pay, report=True)
    assert same(out, plain) and stats["frame_fullref"] == pstats["frame_fullref"] and stats["fullref_summary"] == pstats["fullref_summary"]
    assert stats["frame_report"] == pstats["frame_report"] and stats["fullref_launches"] == pstats["fullref_launches"]
    assert set(stats) - set(KEYS) == set(pstats) and not any(k in pstats for k in KEYS)
    assert stats["add_blur"] == N and stats["add_blur_gamma"] == GAMMA and stats["blur_launches"] == 3


def test_serial_scenes_and_overlapping_windows(clip, blurred):
    net, pay = clip
    out, stats, seen = blurred
    serial, sstats, sseen = run(net, pay, tap=True, add_blur=N, report=True, pipeline=False)
    assert same(serial, out) and same(sseen, seen) and sstats["frame_fullref"] == stats["frame_fullref"]
    # a listed cut: the payloads of two separate streams, one launch more (the chunk the cut lies in has two segments), and the same under window_overlap
    two = list(B.blur_stream(pay, S.FMT420, H, W, N, GAMMA, cuts=[4]))
    assert same(two, list(B.blur_stream(pay[:4], S.FMT420, H, W, N, GAMMA)) + list(B.blur_stream(pay[4:], S.FMT420, H, W, N, GAMMA))) and not same(two, seen)
    for kw in (dict(scene_cuts=[4]), dict(scene_cuts=[4], window_overlap=1), dict(scene_cuts=[5], report=True)):
        got, st, s = run(net, pay, tap=True, add_blur=N, **kw)
        cuts = kw["scene_cuts"]
        assert len(got) == FRAMES and same(s, list(B.blur_stream(pay, S.FMT420, H, W, N, GAMMA, cuts=cuts))), kw
        assert st["blur_launches"] == (3 if cuts == [4] else 4), kw                            # [4] is a chunk boundary; [5] splits the second chunk
        plain, _, _ = run(net, s, **kw, **({"gt": pay} if kw.get("report") else {}))
        assert same(got, plain), kw
    _, _, s = run(net, pay, tap=True, add_blur=N, window_overlap=1)
    assert same(s, seen)
    # gamma 1, another length, chunks longer than the stream and shorter than r
    for kw, one_len in ((dict(add_blur=N, add_blur_gamma=1.0), ONE_LEN), (dict(add_blur=3), ONE_LEN), (dict(add_blur=7), 16), (dict(add_blur=7), 2)):
        _, st, s = run(net, pay, one_len=one_len, tap=True, **kw)
        assert same(s, list(B.blur_stream(pay, S.FMT420, H, W, kw["add_blur"], kw.get("add_blur_gamma", GAMMA)))), (kw, one_len)
        assert st["blur_launches"] == -(-FRAMES // one_len)


def test_a_stream_of_two_frames_at_five_taps(clip):
    net, pay = clip
    out, stats, seen = run(net, pay[:2], tap=True, add_blur=N, report=True)
    assert len(out) == 2 and same(seen, list(B.blur_stream(pay[:2], S.FMT420, H, W, N, GAMMA))) and len(stats["frame_fullref"]) == 2


def luma_psnr(a, b):
    d = a[:H * W].astype(np.float64) - b[:H * W].astype(np.float64)
    return 10.0 * np.log10(255.0 ** 2 / np.mean(d * d))


def test_more_taps_blur_more(clip, blurred):
    net, pay = clip
    # the restatement alone shows it on this clip (every frame moves by a pixel): PSNR of the luma against the sharp frame, n = 5 below n = 3
    r3, r5 = (list(B.blur_stream(pay, S.FMT420, H, W, n, GAMMA)) for n in (3, 5))
    assert all(luma_psnr(b5, p) < luma_psnr(b3, p) for b3, b5, p in zip(r3, r5, pay))
    _, s3, _ = run(net, pay, add_blur=3, report=True)
    p3, p5 = [f.psnr_y_in for f in s3["frame_fullref"]], [f.psnr_y_in for f in blurred[1]["frame_fullref"]]
    print("psnr_y_in at n = 3:", p3, "at n = 5:", p5)
    assert len(p3) == len(p5) == FRAMES and all(b < a for a, b in zip(p3, p5))


def test_a_run_without_the_option_has_the_keys_it_had_and_the_refusals_name_the_options(clip):
    net, pay = clip
    dn = restore.load_net("denoise_small", "synthetic", "bf16")
    out, stats, _ = run(dn, pay, sigma=10.0)
    assert len(out) == FRAMES and sorted(stats) == DEFAULT_KEYS
    out, stats, _ = run(net, pay)
    assert len(out) == FRAMES and not any(k in stats for k in KEYS) and set(stats) <= set(DEFAULT_KEYS)
    fmt = yuv_fmt(*S.FMT420)
    with pytest.raises(ValueError, match=r"add_blur.*add_noise"):
        restore.VideoRestorer(net, ONE_LEN, add_blur=N, add_noise=10)
    with pytest.raises(ValueError, match=r"add_blur.*gt"):
        list(restore.VideoRestorer(net, ONE_LEN, add_blur=N, report=True).restore(iter(pay), fmt, H, W, gt=iter(pay)))
    with pytest.raises(ValueError, match=r"add_blur.*report.*out_format"):
        list(restore.VideoRestorer(net, ONE_LEN, add_blur=N, report=True, out_format="444p10").restore(iter(pay), fmt, H, W))
    with pytest.raises(ValueError, match=r"degraded.*add_noise"):
        list(restore.VideoRestorer(net, ONE_LEN).restore(iter(pay), fmt, H, W, degraded=print))
    for bad in (4, 0, 17, 5.0, "5"):
        with pytest.raises(ValueError, match="add_blur"):
            restore.VideoRestorer(net, ONE_LEN, add_blur=bad)
    with pytest.raises(ValueError, match="add_blur_gamma"):
        restore.VideoRestorer(net, ONE_LEN, add_blur=N, add_blur_gamma=0.5)
    # without a report another format out is fine: nothing needs the truth
    assert len(list(restore.VideoRestorer(net, ONE_LEN, add_blur=N, out_format="444p10").restore(iter(pay), fmt, H, W))) == FRAMES


def test_restore_video_cli_writes_the_blurred_stream_the_report_and_the_api_bytes(clip, blurred, tmp_path):
    _, pay = clip
    out, stats, seen = blurred
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, deg, rep = (tmp_path / n for n in ("sharp.y4m", "out.y4m", "blurred.y4m", "r.txt"))
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic", "--dtype", "bf16",
                        "--one_len", str(ONE_LEN), "--add_blur", str(N), "--degraded_out", str(deg), "--report", str(rep), str(src), str(dst)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"added blur: the mean of {N} frames" in r.stderr and "gamma 2.2" in r.stderr and "the clean input" in r.stderr
    got = {}
    for name, path in (("out", dst), ("blurred", deg)):
        with open(path, "rb") as fh:
            rd = y4m.Y4MReader(fh)
            got[name] = list(rd)
        assert rd.header.line() == hd.line()
    assert same(got["out"], out) and same(got["blurred"], seen)                     # 48 < 720: the CLI's default matrix is BT.601, as FMT420
    assert report.parse_report_fullref(open(rep).read()) == stats["frame_fullref"]
