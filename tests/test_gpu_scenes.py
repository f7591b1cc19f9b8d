"""-m gpu: ``sn_yuv_thumb`` against its numpy restatement (tests/scene_ref.py) exactly, and the video restorer with scene cuts against every
scene restored as a video of its own, byte for byte.  No tolerance anywhere: integers, and bytes produced by the same kernels on the same inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_ref as S
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import restore, scenes, y4m
from shiftnet_amd.io_edges import thumb_yuv, yuv_fmt
from test_gpu_yuv import by_hand

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = S.CUTS26
SCENES = list(zip([0] + CUTS, CUTS + [26]))


# ---- 6. the kernel ----------------------------------------------------------------------------------------------------------------------
def _random_payloads(fmt, T, H, W, seed):
    rng = np.random.default_rng(seed)
    n = R.frame_bytes(fmt, H, W)
    if fmt.bits == 8:
        return rng.integers(0, 256, (T, n), dtype=np.uint8)
    p = rng.integers(0, 1024, (T, n // 2))
    p[0, :min(64, H * W)] = 1023                                  # a block of the largest code: 64 x 1023 must not wrap
    return p.astype("<u2").view(np.uint8).reshape(T, n)


@pytest.mark.parametrize("chroma", [R.C444, R.C420_CENTER, R.C420_LEFT], ids=["444", "420c", "420l"])
@pytest.mark.parametrize("bits", [8, 10])
def test_yuv_thumb_equals_the_numpy_restatement_exactly_and_writes_nothing_else(bits, chroma):
    fmt = R.Fmt(bits, chroma, R.BT709, R.LIMITED)
    f = yuv_fmt(*fmt)
    GUARD = 32                                                    # uint16 words before and after dst
    for (H, W), T in [(s, t) for s in [(8, 8), (67, 101), (70, 98), (1, 1), (16, 256), (135, 241)] for t in (1, 5)]:
        p = _random_payloads(fmt, T, H, W, seed=H * 1000 + W + T)
        fb = R.frame_bytes(fmt, H, W)
        hb, wb = (H + 7) // 8, (W + 7) // 8
        want = S.thumb_ref(p, fmt, H, W)
        for off in ((0, 1, 3) if bits == 8 else (0, 2)):          # 8 bit: payloads at odd byte offsets as well (the element-wise loads)
            buf = torch.zeros(T * fb + 16, dtype=torch.uint8, device="cuda")
            src = buf[off:off + T * fb].view(T, fb)
            src.copy_(torch.from_numpy(p))
            assert src.data_ptr() % 16 == off
            g = torch.from_numpy(np.full(T * hb * wb + 2 * GUARD, 0xA5A5, np.uint16)).cuda()
            got = thumb_yuv(src, f, H, W, out=g[GUARD:GUARD + T * hb * wb].view(T, hb, wb))
            assert got.shape == (T, hb, wb) and got.dtype == torch.uint16
            assert np.array_equal(got.cpu().numpy(), want), (fmt, H, W, T, off)
            b = g.cpu().numpy()
            assert (b[:GUARD] == 0xA5A5).all() and (b[GUARD + T * hb * wb:] == 0xA5A5).all()
    got = thumb_yuv(torch.from_numpy(p).cuda(), f, H, W)                              # allocating form
    assert np.array_equal(got.cpu().numpy(), want)


def test_yuv_thumb_refuses_bad_arguments():
    lib = L.load()
    f = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(64, dtype=torch.int16, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    src, d = buf.data_ptr(), dst.data_ptr()
    assert lib.sn_yuv_thumb(src, f, d, 1, 8, 8, s) == 0
    assert lib.sn_yuv_thumb(src, yuv_fmt(9, 0, 0, 0), d, 1, 8, 8, s) == -22             # bits
    assert lib.sn_yuv_thumb(src, yuv_fmt(12, 0, 0, 0), d, 1, 8, 8, s) == -22
    assert lib.sn_yuv_thumb(src, yuv_fmt(8, 3, 0, 0), d, 1, 8, 8, s) == -22              # chroma code
    assert lib.sn_yuv_thumb(src, yuv_fmt(8, -1, 0, 0), d, 1, 8, 8, s) == -22
    for T, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert lib.sn_yuv_thumb(src, f, d, T, H, W, s) == -22
    assert lib.sn_yuv_thumb(src, f, d + 1, 1, 8, 8, s) == -22                            # dst is uint16
    assert lib.sn_yuv_thumb(src + 1, yuv_fmt(10, 0, 0, 0), d, 1, 8, 8, s) == -22         # 16-bit samples at an odd address
    assert lib.sn_yuv_thumb(src + 1, f, d, 1, 8, 8, s) == 0                              # 8-bit samples may lie anywhere
    assert lib.sn_yuv_thumb(None, f, d, 1, 8, 8, s) == -22 and lib.sn_yuv_thumb(src, f, None, 1, 8, 8, s) == -22
    assert lib.sn_yuv_thumb(src, None, d, 1, 8, 8, s) == -22
    torch.cuda.synchronize()
    assert int(dst[1:].abs().sum()) == 0                                                  # one 8 x 8 frame: one word


# ---- the restorer -------------------------------------------------------------------------------------------------------------------------
def clip(h, w):
    return list(S.payloads_of(S.clip26("blurred", h, w), h, w))


def run(net, pay, h, w, one_len, sigma, **kw):
    vr = restore.VideoRestorer(net, one_len, sigma=sigma, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*S.FMT420), h, w))
    return out, vr.stats


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 7. explicit cuts: the bytes of every scene restored as a video of its own -----------------------------------------------------------
@pytest.mark.parametrize("variant,dtype,h,w", [("deblur_small", "bf16", 70, 98), ("deblur_small", "fp32", 70, 98), ("denoise_small", "bf16", 70, 98),
                                               ("deblur", "bf16", 72, 104)])
def test_explicit_cuts_give_the_bytes_of_every_scene_restored_on_its_own(variant, dtype, h, w):
    one_len = 4
    sigma = 10.0 if "denoise" in variant else None
    pay = clip(h, w)
    assert len(pay) == 26
    net = restore.load_net(variant, "synthetic", dtype)
    want = []
    for a, b in SCENES:
        want += run(net, pay[a:b], h, w, one_len, sigma)[0]
    assert len(want) == 26
    for pipe in (True, False):
        got, stats = run(net, pay, h, w, one_len, sigma, pipeline=pipe, scene_cuts=[7, 12, 18, 22, 23])
        assert len(got) == 26 and stats["frames"] == 26
        for i in range(26):
            assert got[i].shape == (R.frame_bytes(S.FMT420, h, w),) and got[i].dtype == np.uint8
            assert np.array_equal(got[i], want[i]), (i, "pipeline" if pipe else "serial")
        assert stats["cuts"] == CUTS and stats["windows"] == len(restore.plan_scene_windows(26, one_len, CUTS)) == 9


# ---- 8. the feature does something, and off is what it was --------------------------------------------------------------------------------
def test_cuts_change_the_frames_on_both_sides_of_every_cut_and_off_equals_the_hand_assembled_windows():
    h, w, one_len = 70, 98, 4
    pay = clip(h, w)
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    off, stats = run(net, pay, h, w, one_len, None, scene_cuts=None)
    assert "cuts" not in stats or stats["cuts"] == []
    assert same(off, by_hand(net, pay, S.FMT420, h, w, one_len, None))
    assert same(off, run(net, pay, h, w, one_len, None)[0])                               # the default is off
    cut, _ = run(net, pay, h, w, one_len, None, scene_cuts=CUTS)
    for c in CUTS:
        assert not np.array_equal(cut[c - 1], off[c - 1]), c
        assert not np.array_equal(cut[c], off[c]), c
    _, stats = run(net, pay[:10], h, w, one_len, None, scene_cuts=[7, 10, 12])            # cuts at or beyond the end: ignored and reported
    assert stats["cuts"] == [7] and stats["cuts_ignored"] == [10, 12]
    for bad in ([0], [5, 5], "sometimes"):
        with pytest.raises(ValueError):
            restore.VideoRestorer(net, one_len, scene_cuts=bad)


# ---- 9. detection on the device ----------------------------------------------------------------------------------------------------------
def test_auto_finds_the_five_cuts_and_gives_the_bytes_of_the_listed_cuts_and_nothing_on_a_clip_without():
    h, w, one_len = 70, 98, 4
    pay = clip(h, w)
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    listed, _ = run(net, pay, h, w, one_len, None, scene_cuts=CUTS)
    m_host = scenes.cut_measure(S.thumb_ref(np.stack(pay), S.FMT420, h, w), h, w, 8)
    for pipe in (True, False):
        auto, stats = run(net, pay, h, w, one_len, None, pipeline=pipe, scene_cuts="auto")
        assert stats["cuts"] == [7, 12, 18, 22, 23]
        assert same(auto, listed), pipe
        assert stats["cut_measure"] == m_host                                             # the device's thumbnails are the host's, frame by frame
        assert stats["thumb_frames"] == 26                                                # every frame thumbnailed exactly once
    plain = list(S.payloads_of(S._mk("blurred", 13, h, w, 7), h, w))
    off, _ = run(net, plain, h, w, one_len, None)
    auto, stats = run(net, plain, h, w, one_len, None, scene_cuts="auto")
    assert stats["cuts"] == [] and same(auto, off) and stats["thumb_frames"] == 13
    none, stats = run(net, plain, h, w, one_len, None, scene_cuts="auto", cut_threshold=0.5, cut_ratio=0.5)     # the knobs reach the rule
    assert stats["cuts"] == scenes.detect_cuts(stats["cut_measure"], 0.5, 0.5) != []


# ---- 10. the command line ------------------------------------------------------------------------------------------------------------------
def test_restore_video_cli_with_scene_cuts_in_a_child_process_gives_the_api_bytes(tmp_path):
    h, w, one_len = 70, 98, 4
    pay = clip(h, w)
    hd = y4m.Y4MHeader(width=w, height=h, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, dst2, cuts_file = tmp_path / "in.y4m", tmp_path / "out.y4m", tmp_path / "out2.y4m", tmp_path / "cuts.txt"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    base = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic",
            "--dtype", "bf16", "--one_len", str(one_len)]
    r = subprocess.run(base + ["--scene_cuts", "auto", "--cuts_out", str(cuts_file), str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "done: 26 frames" in r.stderr and "6 scenes" in r.stderr
    assert scenes.parse_cuts(cuts_file.read_text()) == CUTS

    def read(path):
        with open(path, "rb") as fh:
            rd = y4m.Y4MReader(fh)
            return list(rd)
    got = read(dst)
    net = restore.load_net("deblur_small", "synthetic", "bf16")
    api, stats = run(net, pay, h, w, one_len, None, scene_cuts="auto")
    assert stats["cuts"] == CUTS and same(got, api)
    r = subprocess.run(base + ["--scene_cuts", str(cuts_file), str(src), str(dst2)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert same(read(dst2), got)
