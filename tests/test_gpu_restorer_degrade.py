"""-m gpu: the video restorer with ``add_noise``: a stage in front of everything else.  The run is the plain run on the degraded payloads with the
clean ones as ``gt``; the degraded payloads are ``sn_yuv_degrade``'s for every frame's index in the stream, whatever the windows make of the frame;
``sigma="auto"`` reads the injected level; and a run without the option has the stats keys it had.  Shift-Net-s denoise with synthetic weights,
bf16, a 48 x 64 stream of 9 frames, one_len 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

import degrade_ref as DR
import noise_ref as N
import scene_ref as S
import yuv_ref as R
from shiftnet_amd import report, restore, synth, y4m
from shiftnet_amd.io_edges import yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FRAMES, ONE_LEN, SEED = 48, 64, 9, 4, 5
KEYS = ("add_noise", "add_noise_seed", "degrade_launches")
# sorted(stats) of VideoRestorer(net, 4, sigma=10.0).restore(...) on this clip, taken from a run of the commit before the option existed
DEFAULT_KEYS = ["amount", "dither", "dither_seed", "forward_s", "frames", "noise_launches", "out_format", "picture_launches", "view", "window_forward_ms",
                "window_picture", "window_sigma", "windows"]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def clip():
    """(the network, the clean payloads)."""
    return restore.load_net("denoise_small", "synthetic", "bf16"), list(S.payloads_of(synth.sharp_clip(FRAMES, H, W, 4), H, W))


def run(net, pay, fmt=S.FMT420, h=H, w=W, one_len=ONE_LEN, gt=None, tap=False, sigma=10.0, **kw):
    vr = restore.VideoRestorer(net, one_len, sigma=sigma, **kw)
    seen = []
    more = ({} if gt is None else {"gt": iter(gt)})
    if tap:
        more["degraded"] = lambda p: seen.append(p.copy())
    return list(vr.restore(iter(pay), yuv_fmt(*fmt), h, w, **more)), vr.stats, seen


@pytest.fixture(scope="module")
def noisy(clip):
    net, pay = clip
    return run(net, pay, tap=True, add_noise=10, add_noise_seed=SEED, report=True)


def test_the_run_is_the_plain_run_on_the_degraded_payloads_with_the_clean_ones_as_truth(clip, noisy):
    net, pay = clip
    out, stats, seen = noisy
    assert len(out) == len(seen) == FRAMES and not same(seen, pay)
    # the stage's payloads are the kernel's for every frame's index in the stream: chunks of one_len, t0 = 0, 4, 8
    assert same(seen, list(DR.degrade_ref(np.stack(pay), S.FMT420, H, W, [10.0] * 16, SEED, 0)))
    plain, pstats, _ = run(net, seen, gt=pay, report=True)
    assert same(out, plain) and stats["frame_fullref"] == pstats["frame_fullref"] and stats["fullref_summary"] == pstats["fullref_summary"]
    assert stats["frame_report"] == pstats["frame_report"] and stats["fullref_launches"] == pstats["fullref_launches"] == 4 * stats["windows"]
    assert set(stats) - set(KEYS) == set(pstats) and not any(k in pstats for k in KEYS)
    assert stats["add_noise"] == [10.0] * 16 and stats["add_noise_seed"] == SEED and stats["degrade_launches"] == 3
    assert all(25.0 < f.psnr_y_in < 40.0 for f in stats["frame_fullref"])                     # the input side is the degraded stream: about 33 dB at sigma 10


def test_serial_scenes_and_overlapping_windows_see_the_same_degraded_stream(clip, noisy):
    net, pay = clip
    out, stats, seen = noisy
    serial, sstats, sseen = run(net, pay, tap=True, add_noise=10, add_noise_seed=SEED, report=True, pipeline=False)
    assert same(serial, out) and same(sseen, seen) and sstats["frame_fullref"] == stats["frame_fullref"]
    for kw in (dict(scene_cuts=[4]), dict(window_overlap=1), dict(scene_cuts=[4], window_overlap=1, report=True)):
        got, st, s = run(net, pay, tap=True, add_noise=10, add_noise_seed=SEED, **kw)
        assert len(got) == FRAMES and same(s, seen), kw                                       # noise per frame of the stream
        plain, _, _ = run(net, seen, **kw, **({"gt": pay} if kw.get("report") else {}))
        assert same(got, plain), kw
    # a curve, another seed
    curve, _, cseen = run(net, pay, tap=True, add_noise=DR.FALLING, add_noise_seed=SEED)
    assert same(cseen, list(DR.degrade_ref(np.stack(pay), S.FMT420, H, W, DR.FALLING, SEED, 0))) and not same(cseen, seen)
    _, _, other = run(net, pay, tap=True, add_noise=10, add_noise_seed=SEED + 1)
    assert not same(other, seen)


def test_sigma_auto_reads_the_injected_level(clip):
    net = clip[0]
    h, w, fmt = 180, 320, N.FORMATS["8-bit 709 limited 4:2:0"]
    rgb = np.stack([N.smooth_rgb(h, w, 0.05 * t) for t in range(6)]).astype(np.float32)
    pay = list(R.egress_emu(rgb, fmt, h, w))
    out, stats, _ = run(net, pay, fmt=fmt, h=h, w=w, one_len=5, sigma="auto", add_noise=10)
    assert len(out) == 6 and stats["windows"] == 2
    print("window_sigma", stats["window_sigma"])
    assert all(abs(s - 10.0) <= N.margin(10) for s in stats["window_sigma"])


def test_a_run_without_the_option_has_the_keys_it_had_and_the_refusals_name_both_options(clip):
    net, pay = clip
    out, stats, _ = run(net, pay)
    assert len(out) == FRAMES and sorted(stats) == DEFAULT_KEYS
    fmt = yuv_fmt(*S.FMT420)
    with pytest.raises(ValueError, match=r"add_noise.*gt"):
        list(restore.VideoRestorer(net, ONE_LEN, sigma=10.0, add_noise=10, report=True).restore(iter(pay), fmt, H, W, gt=iter(pay)))
    with pytest.raises(ValueError, match=r"add_noise.*report.*out_format"):
        list(restore.VideoRestorer(net, ONE_LEN, sigma=10.0, add_noise=10, report=True, out_format="444p10").restore(iter(pay), fmt, H, W))
    with pytest.raises(ValueError, match=r"degraded.*add_noise"):
        list(restore.VideoRestorer(net, ONE_LEN, sigma=10.0).restore(iter(pay), fmt, H, W, degraded=print))
    with pytest.raises(ValueError, match="add_noise"):
        restore.VideoRestorer(net, ONE_LEN, sigma=10.0, add_noise=-1.0)
    # without a report another format out is fine: nothing needs the truth
    assert len(list(restore.VideoRestorer(net, ONE_LEN, sigma=10.0, add_noise=10, out_format="444p10").restore(iter(pay), fmt, H, W))) == FRAMES


def test_restore_video_cli_writes_the_degraded_stream_the_report_and_the_api_bytes(clip, noisy, tmp_path):
    _, pay = clip
    out, stats, seen = noisy
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, deg, rep = (tmp_path / n for n in ("clean.y4m", "out.y4m", "degraded.y4m", "r.txt"))
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "denoise_small", "--checkpoint", "synthetic", "--dtype", "bf16",
                        "--one_len", str(ONE_LEN), "--sigma", "10", "--add_noise", "10", "--add_noise_seed", str(SEED), "--degraded_out", str(deg),
                        "--report", str(rep), str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"added noise: sigma 10 in 8-bit R'G'B' codes, seed {SEED}" in r.stderr and "injected 10" in r.stderr and "the clean input" in r.stderr
    got = {}
    for name, path in (("out", dst), ("degraded", deg)):
        with open(path, "rb") as fh:
            rd = y4m.Y4MReader(fh)
            got[name] = list(rd)
        assert rd.header.line() == hd.line()
    assert same(got["out"], out) and same(got["degraded"], seen)                    # 48 < 720: the CLI's default matrix is BT.601, as FMT420
    assert report.parse_report_fullref(open(rep).read()) == stats["frame_fullref"]
