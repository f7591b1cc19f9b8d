"""-m gpu: ``sn_yuv_diff_stats`` against its numpy restatement (tests/diff_stats_ref.py) word for word -- the sums are integers, so every comparison
is ``==`` -- and the video restorer with ``report=True``: the bytes of ``report=False``, the sums of the restatement on the payloads that went in and
came out, window by window, and the host function of shiftnet_amd/report.py on those sums."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import diff_stats_ref as D
import scene_ref as S
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import report, restore, y4m
from shiftnet_amd.io_edges import diff_stats_yuv, yuv_fmt
from test_gpu_noise import FRAMES, H, ONE_LEN, W, noisy_clip, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = [R.Fmt(bits, chroma, R.BT709, R.LIMITED) for bits in (8, 10) for chroma in (R.C444, R.C420_CENTER, R.C420_LEFT)]
IDS = [f"{f.bits}bit-{('444', '420c', '420l')[f.chroma]}" for f in FORMATS]
GARBAGE = -0x5A5A5A5A5A5A5A5B                                  # what dst holds before a call
ABOVE = 2 * 65535 + 1                                          # an edge threshold above every e


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
def _pair(fmt, T, h, w, seed, wild=True):
    """(a, b) uint8 [T, frame_bytes]: b a ramp with steps and noise (so that the edge rule splits the pixels at every threshold used), a = b plus other
    noise, both clipped to the codes of the format; at 10 bit with ``wild`` a few words of both hold anything up to 65535 (samples are taken as stored)."""
    rng = np.random.default_rng(seed)
    top = (1 << fmt.bits) - 1
    n = R.frame_bytes(fmt, h, w) // (1 if fmt.bits == 8 else 2)
    y, x = np.mgrid[0:h, 0:w]
    b = rng.integers(0, top + 1, (T, n))
    for t in range(T):
        Y = top * (0.2 + 0.5 * ((x // 5) * 5 + y) / max(h + w - 2, 1)) + rng.normal(0.0, 0.004 * top, (h, w)) + 0.2 * top * ((y // 7 + t) & 1)
        b[t, :h * w] = np.clip(np.rint(Y), 0, top).reshape(-1)
    a = np.clip(b + np.rint(rng.normal(0.0, 0.03 * top, b.shape)).astype(np.int64), 0, top)
    if fmt.bits == 10 and wild:
        for p in (a, b):
            k = rng.integers(0, p.size, max(p.size // 50, 1))
            p.reshape(-1)[k] = rng.integers(1024, 65536, k.size)
    as_bytes = (lambda p: p.astype(np.uint8)) if fmt.bits == 8 else (lambda p: p.astype("<u2").view(np.uint8).reshape(T, -1))
    return as_bytes(a), as_bytes(b)


def _at(p, off):
    """The payloads on the device, their first byte ``off`` bytes past a 16-byte boundary."""
    T, fb = p.shape
    buf = torch.zeros(T * fb + 32, dtype=torch.uint8, device="cuda")
    base = (-buf.data_ptr()) % 16 + off
    dev = buf[base:base + T * fb].view(T, fb)
    dev.copy_(torch.from_numpy(p))
    assert dev.data_ptr() % 16 == off
    return dev


def _guarded(T):
    """dst as garbage between guard words -> (the whole buffer, the [T, 16] view inside)."""
    g = torch.full((T * 16 + 16,), GARBAGE, dtype=torch.int64, device="cuda")
    return g, g[8:8 + T * 16].view(T, 16)


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_diff_stats_equals_the_numpy_restatement_exactly_overwrites_and_writes_nothing_else(fmt):
    f = yuv_fmt(*fmt)
    offsets = (0, 1, 3) if fmt.bits == 8 else (0, 2)
    split = set()
    for (h, w), T in [(s, t) for s in [(1, 1), (1, 9), (9, 1), (2, 2), (37, 53), (64, 64), (66, 130)] for t in (1, 2, 5)] + [((256, 512), 2)]:
        a, b = _pair(fmt, T, h, w, seed=h * 1000 + w + T)
        want = {edge: D.diff_stats_ref(a, b, fmt, h, w, edge=edge) for edge in (0, 1, 16, ABOVE)}
        assert (want[0][:, 8] == h * w).all() and (want[ABOVE][:, 8] == 0).all() and (want[0][:, 9] == want[0][:, 2]).all()
        split.update(int(v) for v in want[16][:, 8] if 0 < v < h * w)
        for off in (offsets if (h, w) != (256, 512) else offsets[:2]):
            da, db = _at(a, off), _at(b, off)
            for edge in (0, 1, 16, ABOVE):
                g, out = _guarded(T)
                got = diff_stats_yuv(da, db, f, h, w, edge=edge, out_sums=out)
                assert got.shape == (T, 16) and got.dtype == torch.int64
                assert np.array_equal(got.cpu().numpy(), want[edge]), (fmt, h, w, T, off, edge)
                if edge == 16:
                    diff_stats_yuv(da, db, f, h, w, edge=edge, out_sums=out)        # a second call into what is now there: the same words
                    assert np.array_equal(out.cpu().numpy(), want[edge]), (fmt, h, w, T, off, "second call")
                    ends = g.cpu().numpy()
                    assert (ends[:8] == GARBAGE).all() and (ends[8 + T * 16:] == GARBAGE).all()
    assert len(split) >= 8                                                            # the threshold of 16 does split the pixels of the larger shapes
    got = diff_stats_yuv(da, db, f, h, w)                                             # allocating form: edge 0
    assert np.array_equal(got.cpu().numpy(), want[0])


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_a_rectangle_gives_the_sums_of_the_cropped_stream(fmt):
    f = yuv_fmt(*fmt)
    h, w, T = 37, 53, 2
    a, b = _pair(fmt, T, h, w, seed=5)
    whole = D.diff_stats_ref(a, b, fmt, h, w, edge=16)
    for off in ((0, 1, 3) if fmt.bits == 8 else (0, 2)):
        da, db = _at(a, off), _at(b, off)
        # even origin and size; odd w and h that reach the far edge; two rows; the one pixel in the far corner (its origin is even: legal at 4:2:0 too)
        for rect in [(4, 6, 20, 12), (10, 8, w - 10, h - 8), (0, 0, 8, 2), (w - 1, h - 1, 1, 1)]:
            want = D.diff_stats_ref(a, b, fmt, h, w, rect=rect, edge=16)
            assert want[0][0] == rect[2] * rect[3]
            g, out = _guarded(T)
            got = diff_stats_yuv(da, db, f, h, w, rect=rect, edge=16, out_sums=out)
            assert np.array_equal(got.cpu().numpy(), want), (fmt, rect, off)
            ends = g.cpu().numpy()
            assert (ends[:8] == GARBAGE).all() and (ends[8 + T * 16:] == GARBAGE).all()
        assert np.array_equal(diff_stats_yuv(da, db, f, h, w, rect=(0, 0, w, h), edge=16).cpu().numpy(), whole)
        assert np.array_equal(diff_stats_yuv(da, db, f, h, w, edge=16).cpu().numpy(), whole)


@pytest.mark.parametrize("bits", [8, 10])
def test_extremes_are_exact_where_a_32_bit_partial_sum_is_not(bits):
    fmt = R.Fmt(bits, R.C420_CENTER, R.BT709, R.FULL)
    f = yuv_fmt(*fmt)
    top = (1 << bits) - 1
    cases = [(66, 130, 2, top)] + ([(256, 512, 2, 0xFFFF)] if bits == 10 else [(256, 512, 2, top)])
    for h, w, T, code in cases:
        fb = R.frame_bytes(fmt, h, w)
        a = np.zeros((T, fb), np.uint8)
        b = np.full((T, fb // 2), code, "<u2").view(np.uint8).reshape(T, fb) if bits == 10 else np.full((T, fb), code, np.uint8)
        want = D.diff_stats_ref(a, b, fmt, h, w, edge=0)
        n, c2 = h * w, code * code
        assert list(want[0]) == [n, n * code, n * c2, h * (w - 1), h * (w - 1) * c2, (h - 1) * w, (h - 1) * w * c2, n * c2, n, n * c2,
                                 (h // 2) * (w // 2), (h // 2) * (w // 2) * code, (h // 2) * (w // 2) * c2, (h // 2) * (w // 2) * code,
                                 (h // 2) * (w // 2) * c2, 0]
        assert code != 0xFFFF or n * c2 > 2 ** 48                                     # far beyond 32 bit: one lane's 64 pixels already are
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        assert np.array_equal(diff_stats_yuv(da, db, f, h, w, edge=0).cpu().numpy(), want)
        assert np.array_equal(diff_stats_yuv(db, da, f, h, w, edge=1).cpu().numpy(), D.diff_stats_ref(b, a, fmt, h, w, edge=1))      # d = -code: negative sums
        got = diff_stats_yuv(db, db, f, h, w, edge=0).cpu().numpy()                   # the same tensor twice
        zero = [n, 0, 0, h * (w - 1), 0, (h - 1) * w, 0, 0, n, 0, (h // 2) * (w // 2), 0, 0, 0, 0, 0]
        assert [list(r) for r in got] == [zero] * T


def test_one_launch_equals_overlapping_launches_apart_from_the_last_frames_pair():
    fmt = R.Fmt(8, R.C420_LEFT, R.BT601, R.LIMITED)
    f = yuv_fmt(*fmt)
    h, w = 37, 53
    a, b = _pair(fmt, 5, h, w, seed=9)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    all5 = diff_stats_yuv(da, db, f, h, w, edge=16).cpu().numpy()
    lo = diff_stats_yuv(da[0:3], db[0:3], f, h, w, edge=16).cpu().numpy()
    hi = diff_stats_yuv(da[2:5], db[2:5], f, h, w, edge=16).cpu().numpy()
    assert (all5[:4, 7] != 0).all() and all5[4, 7] == 0 and lo[2, 7] == 0 and hi[2, 7] == 0
    assert np.array_equal(lo[:2], all5[:2]) and np.array_equal(hi, all5[2:])           # hi's last frame is the stream's last: its slot 7 is 0 in both
    keep = [i for i in range(16) if i != 7]
    assert np.array_equal(lo[2, keep], all5[2, keep])


def test_bad_arguments_return_einval_and_leave_dst_untouched():
    lib = L.load()
    f420, f10 = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0), yuv_fmt(10, L.SN_YUV_444, 0, 0)
    h, w = 16, 24
    buf = torch.zeros(2 * 3 * h * w * 2 + 64, dtype=torch.uint8, device="cuda")
    g, out = _guarded(2)
    s = torch.cuda.current_stream().cuda_stream
    a, b, d = buf.data_ptr(), buf.data_ptr() + 3 * h * w * 2 + 32, out.data_ptr()
    call = lib.sn_yuv_diff_stats
    rect = L.YuvRect
    bad = [
        (None, b, f420, None, 16, d, 1, h, w), (a, None, f420, None, 16, d, 1, h, w), (a, b, f420, None, 16, None, 1, h, w),      # null a, b, dst
        (a, b, None, None, 16, d, 1, h, w),                                                                                          # null fmt
        (a, b, yuv_fmt(12, 0, 0, 0), None, 16, d, 1, h, w), (a, b, yuv_fmt(8, 3, 0, 0), None, 16, d, 1, h, w),                       # bits 12, chroma code
        (a + 1, b, f10, None, 16, d, 1, h, w), (a, b + 1, f10, None, 16, d, 1, h, w),                                                # 10 bit at an odd address
        (a, b, f420, rect(8, 8, 24, 8), 16, d, 1, h, w), (a, b, f420, rect(0, 0, 8, 17), 16, d, 1, h, w),                            # a rect off the frame
        (a, b, f420, rect(0, 0, 0, 8), 16, d, 1, h, w),
        (a, b, f420, rect(1, 0, 8, 8), 16, d, 1, h, w), (a, b, f420, rect(0, 1, 8, 8), 16, d, 1, h, w),                              # an odd origin at 4:2:0
        (a, b, f420, rect(0, 0, 7, 8), 16, d, 1, h, w),                                                                              # an odd width inside
        (a, b, f420, None, -1, d, 1, h, w),                                                                                          # edge
        (a, b, f420, None, 16, d, 0, h, w), (a, b, f420, None, 16, d, -1, h, w), (a, b, f420, None, 16, d, 65536, h, w),             # T
        (a, b, f420, None, 16, d, 1, 0, w), (a, b, f420, None, 16, d, 1, h, 0),                                                      # H, W
        (a, b, f420, None, 16, d + 4, 1, h, w),                                                                                      # dst is int64
    ]
    for args in bad:
        assert call(*args, s) == -22, args
    torch.cuda.synchronize()
    assert (g.cpu().numpy() == GARBAGE).all()
    assert call(a + 1, b + 3, f420, rect(2, 2, 8, 8), 0, d, 2, h, w, s) == 0            # 8-bit payloads may lie anywhere; a legal rect
    assert call(a, b, f10, rect(1, 1, 7, 7), 0, d, 1, h, w, s) == 0                      # 4:4:4 takes any rectangle
    torch.cuda.synchronize()
    ends = g.cpu().numpy()
    assert (ends[:8] == GARBAGE).all() and (ends[8 + 32:] == GARBAGE).all() and ends[8] == 49 and ends[8 + 16] == 64      # zeros minus zeros: the counts


# ---- the restorer -------------------------------------------------------------------------------------------------------------------------
SIGMA = 10.0
RECT = (8, 6, 64, 48)


@pytest.fixture(scope="module")
def clip():
    return restore.load_net("denoise_small", "synthetic", "bf16"), noisy_clip()


def run(net, pay, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, sigma=SIGMA, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*S.FMT420), H, W))
    return out, vr.stats, vr


def windows_of(cuts=()):
    """(first frame, frames) of every window, in the order restored."""
    plan = restore.plan_scene_windows(FRAMES, ONE_LEN, cuts) if cuts else restore.plan_windows(FRAMES, ONE_LEN)
    return [(lo, n) for lo, n, _ in plan]


def host_sums(ref, out, fmt, cuts=(), rect=None, edge=16):
    """What the restorer must report: the restatement on the frames each window wrote, one launch per window."""
    ref, out = np.stack(ref), np.stack(out)
    rows, wins = [], []
    for k, (lo, n) in enumerate(windows_of(cuts)):
        rows += [[int(v) for v in r] for r in D.diff_stats_ref(ref[lo:lo + n], out[lo:lo + n], fmt, H, W, rect=rect, edge=edge)]
        wins += [k] * n
    return rows, wins


def check_report(stats, ref, out, fmt, cuts=(), rect=None, edge=16, sigma=SIGMA):
    rows, wins = host_sums(ref, out, fmt, cuts, rect, edge)
    assert stats["frame_sums"] == rows
    want = report.frames_report(rows, wins, [sigma] * len(rows), fmt.bits, fmt.matrix, fmt.range)
    assert stats["frame_report"] == want and [f.frame for f in stats["frame_report"]] == list(range(FRAMES))
    assert stats["report_summary"].keys() == report.summarize(want).keys()
    assert all(report._same(stats["report_summary"][k], v) for k, v in report.summarize(want).items())
    assert stats["report_launches"] == stats["windows"] == len(windows_of(cuts))
    last = {lo + n - 1 for lo, n in windows_of(cuts)}
    assert all(np.isnan(f.rho_t) == (f.frame in last) for f in stats["frame_report"])  # a pair inside a window always has variance on this clip


NEW_KEYS = ("frame_sums", "frame_report", "report_summary", "report_launches")


@pytest.fixture(scope="module")
def plain(clip):
    """The run every other is compared with: no report.  And the reported run of the same arguments."""
    net, pay = clip
    off, stats_off, vr_off = run(net, pay)
    assert not any(k in stats_off for k in NEW_KEYS) and vr_off.run.launches["report"] == 0
    on, stats_on, vr_on = run(net, pay, report=True)
    assert vr_on.run.launches["report"] == 6
    return off, on, stats_on


def test_the_report_changes_no_byte_and_equals_the_restatement_pipelined_and_not(clip, plain):
    net, pay = clip
    off, on, stats = plain
    assert len(off) == FRAMES and same(on, off) and not same(off, pay)
    check_report(stats, pay, on, S.FMT420)
    assert all(0.0 < f.removed_sigma < 3 * SIGMA and f.sigma == SIGMA for f in stats["frame_report"])
    serial, stats2, _ = run(net, pay, report=True, pipeline=False)
    assert same(serial, off) and stats2["frame_sums"] == stats["frame_sums"] and stats2["frame_report"] == stats["frame_report"]
    other, stats3, _ = run(net, pay, report=True, report_edge=4.0)                    # the threshold reaches the kernel: other edge words, the rest the same
    check_report(stats3, pay, other, S.FMT420, edge=4)
    assert stats3["frame_sums"] != stats["frame_sums"]


def test_the_report_of_a_picture_is_over_its_rectangle(clip):
    net, pay = clip
    off, stats_off, _ = run(net, pay, picture=RECT)
    on, stats, _ = run(net, pay, picture=RECT, report=True)
    assert same(on, off) and not any(k in stats_off for k in NEW_KEYS)
    check_report(stats, pay, on, S.FMT420, rect=RECT)
    assert all(r[0] == RECT[2] * RECT[3] for r in stats["frame_sums"])


def test_the_report_with_scene_cuts_follows_the_windows_of_the_scenes(clip):
    net, pay = clip
    cuts = [7, 12]
    off, _, _ = run(net, pay, scene_cuts=cuts)
    on, stats, _ = run(net, pay, scene_cuts=cuts, report=True)
    assert same(on, off) and windows_of(cuts) == [(0, 5), (5, 2), (7, 5), (12, 5), (17, 5), (22, 4)]
    check_report(stats, pay, on, S.FMT420, cuts=cuts)
    serial, stats2, _ = run(net, pay, scene_cuts=cuts, report=True, pipeline=False)
    assert same(serial, off) and stats2["frame_sums"] == stats["frame_sums"]


def test_another_output_format_is_compared_with_the_converted_input(clip):
    net, pay = clip
    tag = "444p10"
    ofmt = R.Fmt(10, R.C444, S.FMT420.matrix, S.FMT420.range)
    conv, _, _ = run(net, pay, out_format=tag, amount=0.0)                            # amount 0 returns the converted input byte for byte
    off, _, _ = run(net, pay, out_format=tag)
    on, stats, _ = run(net, pay, out_format=tag, report=True)
    assert same(on, off) and len(on[0]) == R.frame_bytes(ofmt, H, W)
    check_report(stats, conv, on, ofmt, edge=64)                                      # 16 8-bit codes in 10-bit codes
    boxed, stats_b, _ = run(net, pay, out_format=tag, report=True, picture=RECT)
    assert same(boxed, run(net, pay, out_format=tag, picture=RECT)[0])
    check_report(stats_b, conv, boxed, ofmt, rect=RECT, edge=64)


def test_amount_zero_reports_no_difference(clip):
    net, pay = clip
    out, stats, _ = run(net, pay, amount=0.0, report=True)
    assert same(out, pay)
    check_zero = [i for i in range(16) if i not in (0, 3, 5, 8, 10)]
    assert all(r[i] == 0 for r in stats["frame_sums"] for i in check_zero)
    assert all(r[0] == H * W and r[10] == ((H + 1) // 2) * ((W + 1) // 2) for r in stats["frame_sums"])
    assert all(f.removed_sigma == 0.0 and np.isnan(f.rho_x) and np.isnan(f.rho_t) for f in stats["frame_report"])
    half, stats_h, _ = run(net, pay, amount=0.5, report=True)                         # the report describes the stream written: the blended one
    assert same(half, run(net, pay, amount=0.5)[0])
    rows, wins = host_sums(pay, half, S.FMT420)
    assert stats_h["frame_sums"] == rows


def test_argument_errors_of_the_restorer(clip):
    net, _ = clip
    with pytest.raises(ValueError, match=r"report=True.*view='removed'"):
        restore.VideoRestorer(net, ONE_LEN, sigma=SIGMA, report=True, view="removed")
    with pytest.raises(ValueError, match="report_edge"):
        restore.VideoRestorer(net, ONE_LEN, sigma=SIGMA, report=True, report_edge=-1.0)
    assert restore.VideoRestorer(net, ONE_LEN, sigma=SIGMA, view="removed").report is False


# ---- the command line -------------------------------------------------------------------------------------------------------------------------
def test_restore_video_cli_writes_the_report_of_the_api(clip, plain, tmp_path):
    _, pay = clip
    off, _, stats = plain
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, rep = tmp_path / "in.y4m", tmp_path / "out.y4m", tmp_path / "r.txt"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    cmd = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "denoise_small", "--checkpoint", "synthetic",
           "--dtype", "bf16", "--one_len", str(ONE_LEN), "--sigma", str(SIGMA), "--report", str(rep), str(src), str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "done: 26 frames" in r.stderr and "report (written minus input" in r.stderr and "removed_sigma" in r.stderr
    text = rep.read_text()
    assert report.parse_report(text) == stats["frame_report"]                          # 71 < 720: the CLI's default matrix is BT.601, as S.FMT420
    assert text.splitlines()[-1].startswith("# median ")
    with open(dst, "rb") as fh:
        assert same(list(y4m.Y4MReader(fh)), off)
