"""-m gpu: the video restorer with ``report_quality="niqe"``: the bytes of the run without it, per written frame the score of ``niqe_sums_yuv`` plus
the host arithmetic called directly on the payloads that went in and came out, two launches per window, the report file's two columns, and nothing of
it when the option is off.  Shift-Net-s with synthetic weights on a 96 x 192 stream of 6 frames (two blocks: the fewest that give a score), one_len 4."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_ref as S
from shiftnet_amd import niqe as N
from shiftnet_amd import report, restore, synth, y4m
from shiftnet_amd.io_edges import niqe_sums_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FRAMES, ONE_LEN = 96, 192, 6, 4
KEYS = ("report_quality", "frame_niqe", "report_quality_summary", "report_quality_launches")


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def same_pairs(a, b):
    """Two lists of (niqe_in, niqe_out), nan equal to nan."""
    return len(a) == len(b) and np.array_equal(np.array(a, np.float64).reshape(-1, 2), np.array(b, np.float64).reshape(-1, 2), equal_nan=True)


@pytest.fixture(scope="module")
def clip():
    rgb = synth.sharp_clip(FRAMES, H, W, 9).astype(np.float64)
    rgb = np.clip(np.rint(rgb + np.random.default_rng(9).normal(0.0, 8.0, rgb.shape)), 0, 255).astype(np.uint8)
    return restore.load_net("deblur_small", "synthetic", "bf16"), list(S.payloads_of(rgb, H, W))


def run(net, pay, h=H, w=W, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    return list(vr.restore(iter(pay), yuv_fmt(*S.FMT420), h, w)), vr.stats


def direct(pay, h=H, w=W, rect=None):
    """The score of every payload: the kernel through its binding, then the host arithmetic."""
    mu, cov, win7 = N.load_params(N.default_params_path())
    taps = torch.from_numpy(win7.astype(np.float32)).cuda()
    sums = niqe_sums_yuv(torch.from_numpy(np.stack(pay)).cuda(), yuv_fmt(*S.FMT420), h, w, taps, rect=rect).cpu().numpy()
    return [N.frame_score(s, mu, cov) for s in sums]


@pytest.fixture(scope="module")
def runs(clip):
    net, pay = clip
    off, stats_off = run(net, pay, report=True)
    on, stats_on = run(net, pay, report=True, report_quality="niqe")
    return off, stats_off, on, stats_on


def test_the_option_changes_no_byte_and_adds_its_keys_only_when_on(clip, runs):
    net, pay = clip
    off, stats_off, on, stats_on = runs
    assert len(off) == FRAMES and same(on, off) and not same(off, pay)
    assert not any(k in stats_off for k in KEYS) and all(k in stats_on for k in KEYS)
    assert set(stats_on) - set(KEYS) == set(stats_off) and stats_on["frame_sums"] == stats_off["frame_sums"]
    assert stats_on["frame_report"] == stats_off["frame_report"] and stats_on["report_launches"] == stats_off["report_launches"] == 2
    bare, stats_bare = run(net, pay)
    assert same(bare, off) and not any(k in stats_bare for k in KEYS)


def test_the_scores_are_those_of_the_kernel_and_the_host_arithmetic_on_what_went_in_and_came_out(clip, runs):
    _, pay = clip
    _, _, on, stats = runs
    want = list(zip(direct(pay), direct(on)))
    assert len(stats["frame_niqe"]) == FRAMES and same_pairs(stats["frame_niqe"], want)
    assert all(np.isfinite(v) and 1.0 < v < 100.0 for p in stats["frame_niqe"] for v in p)
    assert stats["windows"] == 2 and stats["report_quality_launches"] == 2 * stats["windows"] and stats["report_quality"] == "niqe"
    med = stats["report_quality_summary"]
    assert med == {"niqe_in": float(np.median([p[0] for p in want])), "niqe_out": float(np.median([p[1] for p in want]))}


def test_serial_and_a_rectangle_and_a_picture_below_two_blocks(clip, runs):
    net, pay = clip
    _, _, on, stats = runs
    serial, stats2 = run(net, pay, report=True, report_quality="niqe", pipeline=False)
    assert same(serial, on) and same_pairs(stats2["frame_niqe"], stats["frame_niqe"])
    # one block: a launch and no score; no block: no launch and no score -- neither fails
    rect = (0, 0, 100, 96)
    out, st = run(net, pay, report=True, report_quality="niqe", picture=rect)
    assert len(out) == FRAMES and st["report_quality_launches"] == 4 and all(np.isnan(v) for p in st["frame_niqe"] for v in p)
    assert all(np.isnan(v) for v in st["report_quality_summary"].values())
    out, st = run(net, pay, report=True, report_quality="niqe", picture=(0, 0, 192, 64))
    assert len(out) == FRAMES and st["report_quality_launches"] == 0 and len(st["frame_niqe"]) == FRAMES
    assert all(np.isnan(v) for p in st["frame_niqe"] for v in p)


def test_argument_errors_of_the_restorer(clip):
    net, _ = clip
    with pytest.raises(ValueError, match="report=True"):
        restore.VideoRestorer(net, ONE_LEN, report_quality="niqe")
    with pytest.raises(ValueError, match="report_quality"):
        restore.VideoRestorer(net, ONE_LEN, report=True, report_quality="brisque")
    with pytest.raises(ValueError, match="niqe_params"):
        restore.VideoRestorer(net, ONE_LEN, report=True, report_quality="niqe", niqe_params="/nonexistent/model.npz")
    assert restore.VideoRestorer(net, ONE_LEN, report=True).report_quality is None


def test_restore_video_cli_writes_the_two_columns_and_the_median_line(clip, runs, tmp_path):
    _, pay = clip
    off, _, _, stats = runs
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, rep = tmp_path / "in.y4m", tmp_path / "out.y4m", tmp_path / "r.txt"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    cmd = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic",
           "--dtype", "bf16", "--one_len", str(ONE_LEN), "--report", str(rep), "--report_quality", "niqe", str(src), str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "quality (NIQE" in r.stderr and "niqe_in" in r.stderr and "niqe_out" in r.stderr
    text = rep.read_text()
    lines = text.splitlines()
    assert [ln for ln in lines if ln.startswith("# frame ")][0].split()[-2:] == ["niqe_in", "niqe_out"]
    assert same_pairs(report.parse_report_quality(text), stats["frame_niqe"])          # 96 < 720: the CLI's default matrix is BT.601, as S.FMT420
    med = stats["report_quality_summary"]
    assert lines[-1].startswith("# median ") and lines[-1].split()[-2:] == [repr(med["niqe_in"]), repr(med["niqe_out"])]
    with open(dst, "rb") as fh:
        assert same(list(y4m.Y4MReader(fh)), off)
