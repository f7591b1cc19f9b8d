"""-m gpu: ``VideoRestorer(window_overlap=V)`` against a hand assembly written out here: every window of the restatement's plan (tests/time_ref.py)
through the network on its own, the shared frames cross-faded by the restatement, the planned prefix written by the existing egress -- byte for byte,
and ``stats["seam_rms"]`` number for number."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import time_ref as TR
import yuv_ref as R
from shiftnet_amd import restore, restore_parts, synth, windows, y4m
from shiftnet_amd.io_edges import egress_yuv, ingest_u8, ingest_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)
H, W, FRAMES, ONE_LEN = 35, 50, 11, 4                       # 35 x 50 is padded to 36 x 52: the statistic has padding to leave out
SIGMA = 10.0
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
NEW_KEYS = {"window_overlap", "window_written", "seam_rms", "overlap_launches"}


def clip(sigma=0.0, seed=3):
    """FRAMES payloads of the synthetic sharp clip, 4:2:0 8 bit, made by the existing egress."""
    rgb = synth.sharp_clip(FRAMES, H, W, seed)
    if sigma:
        rgb = np.clip(np.rint(rgb.astype(np.float64) + np.random.default_rng(seed).normal(0.0, sigma, rgb.shape)), 0, 255).astype(np.uint8)
    x = ingest_u8(torch.from_numpy(rgb).cuda(), torch.float32)[0]
    return list(egress_yuv(x, yuv_fmt(*FMT), H, W).cpu().numpy())


def run(net, pay, **kw):
    if net.V.denoise:
        kw.setdefault("sigma", SIGMA)
    vr = restore.VideoRestorer(net, ONE_LEN, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*FMT), H, W))
    return out, vr.stats, vr


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def plain(net, x, x32, nm):
    """One window through the network: float32 [cnt, 3, hp, wp]."""
    args = (x,) if nm is None else (x, nm)
    return net.forward_fp32_out(*args, **({"shortcut": x32} if x32 is not None else {}))


def assembled(net, pay, V, forward=plain, cuts=(), dither_seed=None, pictures=None):
    """What the restorer must write and report, window by window of the restatement's plan: the existing ingest, ``forward`` on the window alone, the
    restatement's statistic and cross-fade on the host against the predecessor's last V frames -- where there is a predecessor in the scene with the same
    picture rectangle --, the existing egress on the planned prefix.  -> (payloads, seam_rms per window, frames written per window)."""
    f = yuv_fmt(*FMT)
    dt = next(net.parameters()).dtype
    w_old, w_new = TR.weights(V)
    out, seams, counts = [], [], []
    carry, carry_rect = None, None
    for k, (lo, cnt, idx, head, wr) in enumerate(TR.scene_plan(len(pay), ONE_LEN, list(cuts), V)):
        rect = pictures[k] if pictures is not None else None
        h, w = (H, W) if rect is None else (rect[3], rect[2])
        hp, wp = windows.padded_size(h, w, net.V.topo)
        dev = torch.from_numpy(np.stack([pay[i] for i in idx])).cuda()
        x = ingest_yuv(dev, f, H, W, hp, wp, dt, rect=rect)
        x32 = ingest_yuv(dev, f, H, W, hp, wp, torch.float32, rect=rect) if dt != torch.float32 else None
        nm = torch.full((1, 1, 1, 1, 1), SIGMA / 255.0, dtype=dt, device="cuda").expand(1, len(idx), 1, hp, wp) if net.V.denoise else None
        o = forward(net, x, x32, nm)
        assert o.dtype == torch.float32 and tuple(o.shape) == (cnt, 3, hp, wp)
        o = o.cpu().numpy().copy()
        if head and carry is not None and carry_rect == (rect,):
            seams.append([TR.seam_rms(row, h, w) for row in TR.seam_sq(carry, o[:V], h, w)])
            o[:V] = TR.crossfade(carry, o[:V], w_old, w_new)
        else:
            seams.append(None)
        carry, carry_rect = (o[cnt - V:].copy(), (rect,)) if wr < cnt else (None, None)
        scene = max([0] + [c for c in cuts if c <= lo])
        dither = None if dither_seed is None else (dither_seed, lo - scene)          # the frame's number in its clip
        dst = dev[windows.PAST:windows.PAST + wr].clone() if rect is not None else None      # outside a picture the frames leave as they came in
        out += list(egress_yuv(torch.from_numpy(o[:wr]).cuda(), f, H, W, dst=dst, rect=rect, dither=dither).cpu().numpy())
        counts.append(wr)
    return out, seams, counts


@pytest.fixture(scope="module")
def nets():
    """Per (variant, dtype): the net, its clip, the run without overlap."""
    pays = {"deblur_small": clip(), "denoise_small": clip(sigma=SIGMA)}
    made = {}

    def get(variant, name):
        if (variant, name) not in made:
            net = restore.load_net(variant, "synthetic", name)
            full, stats, vr = run(net, pays[variant])
            assert not (NEW_KEYS & set(stats)) and vr.run.launches["overlap"] == 0 and not same(full, pays[variant])
            made[variant, name] = (net, pays[variant], full, stats)
        return made[variant, name]
    return get


@pytest.mark.parametrize("V", [1, 2])
@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("variant", ["deblur_small", "denoise_small"])
def test_the_bytes_and_the_seams_are_those_of_the_hand_assembly(nets, variant, name, V):
    net, pay, full, _ = nets(variant, name)
    want, seams, counts = assembled(net, pay, V)
    assert len(want) == FRAMES and sum(counts) == FRAMES
    got, stats, _ = run(net, pay, window_overlap=V)
    print(f"{variant} {name} V={V}: seam_rms {stats['seam_rms']}")
    assert same(got, want)
    assert stats["seam_rms"] == seams and stats["window_written"] == counts and sum(stats["window_written"]) == FRAMES
    assert stats["window_overlap"] == V and stats["frames"] == FRAMES and stats["windows"] == len(counts) == {1: 4, 2: 5}[V]
    assert stats["overlap_launches"] == len(counts) - 1 and seams[0] is None and all(s is not None and len(s) == V for s in seams[1:])
    assert all(v > 0.0 for s in seams[1:] for v in s)                                 # the two answers differ: a window's edge is not an interior
    assert not same(got, full)
    if net.V.denoise:
        assert stats["window_sigma"] == [SIGMA] * len(counts)                        # the per-window statistics stay per window: there are more windows
    serial, stats2, _ = run(net, pay, window_overlap=V, pipeline=False)
    assert same(serial, want) and stats2["seam_rms"] == seams and stats2["window_written"] == counts


def test_scenes_restart_the_overlap(nets):
    net, pay, _, _ = nets("deblur_small", "bf16")
    for V in (1, 2):
        got, stats, _ = run(net, pay, window_overlap=V, scene_cuts=[5])
        first, s1, _ = run(net, pay[:5], window_overlap=V)
        second, s2, _ = run(net, pay[5:], window_overlap=V)
        assert same(got, first + second)                                             # the two scenes restored as separate videos with the same overlap
        assert stats["seam_rms"] == s1["seam_rms"] + s2["seam_rms"] and stats["window_written"] == s1["window_written"] + s2["window_written"]
        assert s2["seam_rms"][0] is None and stats["cuts"] == [5]
        want, seams, counts = assembled(net, pay, V, cuts=[5])
        assert same(got, want) and stats["seam_rms"] == seams and stats["window_written"] == counts


def test_a_clip_of_one_window_and_an_overlap_of_zero_are_todays_bytes(nets):
    net, pay, full, stats_full = nets("deblur_small", "bf16")
    short, _, _ = run(net, pay[:4])
    got, stats, _ = run(net, pay[:4], window_overlap=2)                              # one window: nothing is shared
    assert same(got, short) and stats["seam_rms"] == [None] and stats["window_written"] == [4] and stats["overlap_launches"] == 0
    zero, stats0, vr = run(net, pay, window_overlap=0)
    assert same(zero, full) and set(stats0) == set(stats_full) and vr.overlap is None and vr.run.launches["overlap"] == 0
    assert {k: v for k, v in stats0.items() if k.endswith("_launches")} == {k: v for k, v in stats_full.items() if k.endswith("_launches")}
    with_v, stats_v, _ = run(net, pay, window_overlap=2)
    assert set(stats_v) - set(stats_full) == NEW_KEYS and set(stats_full) <= set(stats_v)


def test_a_seam_between_two_picture_rectangles_is_the_later_windows_alone(nets):
    net, pay, _, _ = nets("deblur_small", "bf16")
    rect = (4, 2, 40, 30)
    pictures = [None, None, rect, rect, rect]                                        # V = 2: five windows; the rectangle changes between windows 1 and 2
    want, seams, counts = assembled(net, pay, 2, pictures=pictures)
    assert seams[2] is None and seams[1] is not None and seams[3] is not None and seams[4] is not None
    got, stats, _ = run(net, pay, window_overlap=2, picture=pictures)
    assert same(got, want) and stats["seam_rms"] == seams and stats["window_written"] == counts and stats["overlap_launches"] == 3
    assert stats["window_picture"] == pictures
    # frames 4 and 5, shared by windows 1 and 2, are window 2's alone: what it writes when it has no predecessor to blend with
    lone = torch.from_numpy(np.stack([pay[i] for i in TR.plan(FRAMES, ONE_LEN, 2)[2][2]])).cuda()
    f = yuv_fmt(*FMT)
    hp, wp = windows.padded_size(rect[3], rect[2], net.V.topo)
    x = ingest_yuv(lone, f, H, W, hp, wp, torch.bfloat16, rect=rect)
    x32 = ingest_yuv(lone, f, H, W, hp, wp, torch.float32, rect=rect)
    o = net.forward_fp32_out(x, shortcut=x32)
    two = egress_yuv(o[:2].contiguous(), f, H, W, dst=lone[windows.PAST:windows.PAST + 2].clone(), rect=rect).cpu().numpy()
    assert same(got[4:6], list(two))


def test_the_ensemble_runs_inside_every_window(nets):
    net, pay, _, _ = nets("deblur_small", "bf16")

    def forward(net, x, x32, nm):
        return net.forward_ensemble_fp32_out(x, shortcut=x32, ensemble=2)
    want, seams, counts = assembled(net, pay, 2, forward=forward)
    got, stats, _ = run(net, pay, window_overlap=2, ensemble=2)
    assert same(got, want) and stats["seam_rms"] == seams and stats["window_written"] == counts
    assert stats["ensemble"] == 2 and stats["ensemble_members"] == [0, 1]
    assert not same(got, run(net, pay, window_overlap=2)[0])


def test_tiles_run_inside_every_window(nets):
    net, pay, _, _ = nets("deblur_small", "bf16")
    tile = (24, 32, 8)                                                               # smaller than the 36 x 52 picture: 2 x 2 tiles
    part = restore_parts.Tiles(torch, net, torch.device("cuda", torch.cuda.current_device()), tile)
    hp, wp = windows.padded_size(H, W, net.V.topo)
    part.prepare(ONE_LEN, hp, wp)
    record = restore._Run()

    def forward(net, x, x32, nm):
        def one(crop):
            return net.forward_fp32_out(x[crop].contiguous(), shortcut=x32[crop].contiguous())
        canvas = part.forward(one, x.shape[1] - windows.PAST - windows.FUTURE, hp, wp, record)
        assert canvas is not None
        return canvas.clone()
    want, seams, counts = assembled(net, pay, 2, forward=forward)
    got, stats, _ = run(net, pay, window_overlap=2, tile=tile[:2], tile_overlap=tile[2])
    assert same(got, want) and stats["seam_rms"] == seams and stats["window_written"] == counts
    assert stats["tile_launches"] == 4 * len(counts) == record.launches["tile"] and stats["window_tiles"] == record.window_tiles
    assert not same(got, run(net, pay, window_overlap=2)[0])


def test_dithered_bytes_count_the_frames_in_the_clip(nets):
    net, pay, _, _ = nets("denoise_small", "bf16")
    want, seams, counts = assembled(net, pay, 2, dither_seed=77)
    got, stats, _ = run(net, pay, window_overlap=2, dither="tpdf", dither_seed=77)
    assert same(got, want) and stats["seam_rms"] == seams
    assert not same(got, run(net, pay, window_overlap=2)[0])
    want, seams, _ = assembled(net, pay, 2, dither_seed=77, cuts=[5])
    got, stats, _ = run(net, pay, window_overlap=2, dither="tpdf", dither_seed=77, scene_cuts=[5])
    assert same(got, want) and stats["seam_rms"] == seams


def test_illegal_overlaps_are_refused_at_construction(nets):
    net = nets("deblur_small", "bf16")[0]
    for bad in (-1, 3, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="window_overlap"):
            restore.VideoRestorer(net, ONE_LEN, window_overlap=bad)
    assert restore.VideoRestorer(net, ONE_LEN).window_overlap == 0 and restore.VideoRestorer(net, ONE_LEN, window_overlap=2).window_overlap == 2


# ---- the command line -------------------------------------------------------------------------------------------------------------------------
def test_restore_video_cli_with_an_overlap_writes_the_restorers_bytes_and_the_seams(tmp_path, nets):
    net, pay, _, _ = nets("deblur_small", "bf16")
    want, stats, _ = run(net, pay, window_overlap=2)
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, seams = tmp_path / "in.y4m", tmp_path / "out.y4m", tmp_path / "seams.txt"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic", "--dtype", "bf16",
                        "--one_len", str(ONE_LEN), "--window_overlap", "2", "--seams_out", str(seams), str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "window overlap: 2 of 4 frames shared" in r.stderr and "seams: 4 cross-faded over 5 windows, median difference" in r.stderr
    with open(dst, "rb") as fh:
        assert same(list(y4m.Y4MReader(fh)), want)                                  # 35 < 720: the CLI's default matrix is BT.601, as FMT
    assert windows.parse_seams(seams.read_text()) == stats["seam_rms"]
