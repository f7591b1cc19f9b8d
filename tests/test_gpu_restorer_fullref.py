"""-m gpu: the video restorer with ``restore(gt=...)``: the bytes of the run without it, per written frame the numbers of ``diff_stats_yuv`` and
``ssim_sums_yuv`` plus shiftnet_amd/fullref.py called directly on the payloads that went in, came out and were given as truth, four launches per
window, and nothing of it when the option is off.  Shift-Net-s with synthetic weights on a 40 x 72 stream, one_len 4: a clean clip is the truth, a
noisy copy of it the input."""
import math

import numpy as np
import pytest
import torch

import scene_ref as S
import yuv_ref as R
from shiftnet_amd import fullref as F
from shiftnet_amd import report, restore, synth
from shiftnet_amd.io_edges import diff_stats_yuv, egress_yuv, ingest_yuv, ssim_sums_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

H, W, FRAMES, ONE_LEN = 40, 72, 6, 4
KEYS = ("frame_fullref", "fullref_summary", "fullref_launches")
FMT_10 = R.Fmt(10, R.C444, R.BT601, R.LIMITED)                 # what out_format="444p10" writes for S.FMT420


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def clean_and_noisy(frames, seed):
    clean = synth.sharp_clip(frames, H, W, seed)
    noisy = np.clip(np.rint(clean.astype(np.float64) + np.random.default_rng(seed).normal(0.0, 8.0, clean.shape)), 0, 255).astype(np.uint8)
    return clean, noisy


@pytest.fixture(scope="module")
def clip():
    """(the network, the input's payloads, the truth's payloads, the truth's payloads in 10-bit 4:4:4)."""
    clean, noisy = clean_and_noisy(FRAMES, 9)
    return (restore.load_net("deblur_small", "synthetic", "bf16"), list(S.payloads_of(noisy, H, W)), list(S.payloads_of(clean, H, W)),
            list(S.payloads_of(clean, H, W, FMT_10)))


def run(net, pay, gt=None, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    return list(vr.restore(iter(pay), yuv_fmt(*S.FMT420), H, W, **({} if gt is None else {"gt": iter(gt)}))), vr.stats


def direct(inp, out, truth, fmt=S.FMT420, rect=None):
    """One FullRef per frame from the bindings and the host arithmetic: ``inp`` (the input in the format written), ``out`` and ``truth`` are payloads."""
    f = yuv_fmt(*fmt)
    g, a, b = (torch.from_numpy(np.stack(p)).cuda() for p in (truth, inp, out))
    h, w = (H, W) if rect is None else (rect[3], rect[2])
    si, so = (diff_stats_yuv(g, x, f, H, W, rect=rect, edge=0).cpu().numpy() for x in (a, b))
    ti, to = (ssim_sums_yuv(g, x, f, H, W, rect=rect).cpu().numpy() for x in (a, b))
    return [F.frame_fullref(si[i], so[i], ti[i], to[i], fmt.bits, h, w) for i in range(len(truth))]


@pytest.fixture(scope="module")
def runs(clip):
    net, pay, truth, _ = clip
    off, stats_off = run(net, pay, report=True)
    on, stats_on = run(net, pay, truth, report=True)
    return off, stats_off, on, stats_on


def test_the_option_changes_no_byte_and_adds_its_keys_only_when_on(clip, runs):
    net, pay, truth, _ = clip
    off, stats_off, on, stats_on = runs
    assert len(off) == FRAMES and same(on, off) and not same(off, pay)
    assert not any(k in stats_off for k in KEYS) and all(k in stats_on for k in KEYS)
    assert set(stats_on) - set(KEYS) == set(stats_off) and stats_on["frame_sums"] == stats_off["frame_sums"]
    assert stats_on["frame_report"] == stats_off["frame_report"] and stats_on["report_launches"] == stats_off["report_launches"] == 2
    # a restorer that has run with gt runs without it as one that never has: no key, no launch, the same bytes and the same report file
    vr = restore.VideoRestorer(net, ONE_LEN, report=True)
    first = list(vr.restore(iter(pay), yuv_fmt(*S.FMT420), H, W, gt=iter(truth)))
    assert vr.stats["fullref_launches"] == 4 * vr.stats["windows"]
    again = list(vr.restore(iter(pay), yuv_fmt(*S.FMT420), H, W))
    assert same(first, off) and same(again, off) and not any(k in vr.stats for k in KEYS) and set(vr.stats) == set(stats_off)
    assert report.format_report(vr.stats["frame_report"], "edge 16") == report.format_report(stats_off["frame_report"], "edge 16")
    text = report.format_report(stats_on["frame_report"], "edge 16", None, None, stats_on["frame_fullref"])
    assert report.parse_report_fullref(text) == stats_on["frame_fullref"]


def test_the_numbers_are_those_of_the_bindings_and_the_host_arithmetic_on_what_went_in_came_out_and_was_given(clip, runs):
    _, pay, truth, _ = clip
    _, _, on, stats = runs
    want = direct(pay, on, truth)
    got = stats["frame_fullref"]
    assert len(got) == FRAMES and all(isinstance(f, F.FullRef) for f in got) and got == want
    assert all(math.isfinite(v) for f in got for v in f) and all(10.0 < f.psnr_y_in < 60.0 and 0.0 < f.ssim_in < 1.0 and 0.0 < f.ssim_out < 1.0 for f in got)
    assert stats["windows"] == 2 and stats["fullref_launches"] == 4 * stats["windows"]
    assert stats["fullref_summary"] == F.summarize_fullref(want)
    assert stats["fullref_summary"]["median"]["ssim_in"] == float(np.median([f.ssim_in for f in want]))


def test_serial_gives_the_same_numbers_and_a_rectangle_its_own(clip, runs):
    net, pay, truth, _ = clip
    _, _, on, stats = runs
    serial, stats2 = run(net, pay, truth, report=True, pipeline=False)
    assert same(serial, on) and stats2["frame_fullref"] == stats["frame_fullref"] and stats2["fullref_launches"] == 8
    rect = (8, 4, 48, 32)
    out, st = run(net, pay, truth, report=True, picture=rect)
    plain, _ = run(net, pay, report=True, picture=rect)
    assert same(out, plain) and st["frame_fullref"] == direct(pay, out, truth, rect=rect) and st["frame_fullref"] != direct(pay, out, truth)


def test_another_format_out_compares_in_the_format_written(clip):
    net, pay, _, truth10 = clip
    out, st = run(net, pay, truth10, report=True, out_format="444p10")
    plain, _ = run(net, pay, report=True, out_format="444p10")
    assert same(out, plain) and out[0].size == R.frame_bytes(FMT_10, H, W)
    d = torch.from_numpy(np.stack(pay)).cuda()
    own = egress_yuv(ingest_yuv(d, yuv_fmt(*S.FMT420), H, W, H, W, torch.float32)[0], yuv_fmt(*FMT_10), H, W).cpu().numpy()
    want = direct(list(own), out, truth10, fmt=FMT_10)
    assert st["frame_fullref"] == want and all(20.0 < f.psnr_y_in < 60.0 for f in want)


def test_overlapping_windows_and_a_scene_cut_take_the_truths_frames_in_step(clip):
    net = clip[0]
    clean, noisy = clean_and_noisy(9, 11)
    pay, truth = list(S.payloads_of(noisy, H, W)), list(S.payloads_of(clean, H, W))
    kw = dict(report=True, window_overlap=1, scene_cuts=[5])
    out, st = run(net, pay, truth, **kw)
    plain, stp = run(net, pay, **kw)
    assert len(out) == 9 and same(out, plain) and st["window_written"] == stp["window_written"] and sum(st["window_written"]) == 9
    assert any(n < ONE_LEN for n in st["window_written"][:-1])                               # a window did keep a frame back
    assert st["frame_fullref"] == direct(pay, out, truth) and st["fullref_launches"] == 4 * st["windows"]
    # a truth shifted by one frame reads worse on every frame: the frames are taken in step, not merely counted
    _, shifted = run(net, pay, truth[1:] + truth[:1], **kw)
    assert all(a.psnr_y_in > b.psnr_y_in for a, b in zip(st["frame_fullref"], shifted["frame_fullref"]))


def test_a_truth_equal_to_the_input_reads_ssim_one_and_psnr_inf_on_the_input_side(clip):
    net, pay, _, _ = clip
    out, st = run(net, pay, pay, report=True)
    got = st["frame_fullref"]
    assert all(f.ssim_in == 1.0 and f.psnr_y_in == f.psnr_u_in == f.psnr_v_in == math.inf for f in got)
    assert all(math.isfinite(f.psnr_y_out) and f.ssim_out < 1.0 for f in got)
    s = st["fullref_summary"]
    assert s["inf"]["psnr_y_in"] == FRAMES and math.isnan(s["mean"]["psnr_y_in"]) and s["median"]["psnr_y_in"] == math.inf and s["inf"]["psnr_y_out"] == 0


def test_argument_errors(clip):
    net, pay, truth, truth10 = clip
    fmt = yuv_fmt(*S.FMT420)
    with pytest.raises(ValueError, match="report=True"):
        list(restore.VideoRestorer(net, ONE_LEN).restore(iter(pay), fmt, H, W, gt=iter(truth)))
    for pipeline in (True, False):
        with pytest.raises(ValueError, match=r"gt ended early.*frame 5"):
            list(restore.VideoRestorer(net, ONE_LEN, report=True, pipeline=pipeline).restore(iter(pay), fmt, H, W, gt=iter(truth[:-1])))
    with pytest.raises(ValueError, match=r"gt: frame 0 .* bytes"):
        list(restore.VideoRestorer(net, ONE_LEN, report=True).restore(iter(pay), fmt, H, W, gt=iter(truth10)))
    # payloads beyond the input's last frame are not looked for
    out = list(restore.VideoRestorer(net, ONE_LEN, report=True).restore(iter(pay), fmt, H, W, gt=iter(truth + truth)))
    assert len(out) == FRAMES
