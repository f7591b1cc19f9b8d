"""-m gpu: ``sn_yuv_noise_hist`` against its numpy restatement (tests/noise_ref.py) bit for bit, and the video restorer with ``sigma="auto"``
against the host restatement on the same payloads exactly (integer histograms through the same float64 function) and against a second run
that is handed the sigmas as a list, byte for byte.  The only tolerance is the margin of tests/test_host_noise.py, on the injected sigma."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import noise_ref as N
import scene_ref as S
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import noise, restore, synth, y4m
from shiftnet_amd.io_edges import noise_hist_yuv, yuv_fmt
from test_gpu_yuv import by_hand

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the kernel -------------------------------------------------------------------------------------------------------------------------
def _payloads(fmt, T, H, W, seed):
    """Noisy content, so that many bins fill: a ramp plus Gaussian noise whose level differs from frame to frame, codes over the whole range
    (clipped ones included).  With T = 5: frame 2 is one constant code (all mass in bin 0) and frame 3 is black (no block counts: N = 0)."""
    rng = np.random.default_rng(seed)
    top = (1 << fmt.bits) - 1
    n = R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)
    p = rng.integers(0, top + 1, (T, n))                                        # the chroma part: anything
    y, x = np.mgrid[0:H, 0:W]
    for t in range(T):
        s = (3.0, 25.0, 0.0, 0.0, 90.0)[t % 5] * (top / 255.0)
        Y = np.clip(np.rint(top * (0.1 + 0.8 * (x + y) / max(H + W - 2, 1)) + rng.normal(0.0, 1.0, (H, W)) * s), 0, top)
        if T == 5 and t == 2:
            Y[:] = top // 2
        if T == 5 and t == 3:
            Y[:] = 0
        p[t, :H * W] = Y.reshape(-1)
    return p.astype(np.uint8) if fmt.bits == 8 else p.astype("<u2").view(np.uint8).reshape(T, -1)


@pytest.mark.parametrize("chroma", [R.C444, R.C420_CENTER, R.C420_LEFT], ids=["444", "420c", "420l"])
@pytest.mark.parametrize("bits", [8, 10])
def test_noise_hist_equals_the_numpy_restatement_exactly_overwrites_and_writes_nothing_else(bits, chroma):
    fmt = R.Fmt(bits, chroma, R.BT709, R.LIMITED)
    f = yuv_fmt(*fmt)
    nb = N.nbins(bits)
    assert nb == noise.nbins(bits)
    GUARD = 64                                                                  # uint32 words before and after dst
    ranges = [N.clip_codes(R.Fmt(bits, chroma, 0, R.LIMITED)), N.clip_codes(R.Fmt(bits, chroma, 0, R.FULL))]
    filled = 0
    for (H, W), T in [(s, t) for s in [(64, 64), (37, 53), (2, 2), (1, 9), (9, 1), (66, 130), (720, 1280)] for t in (1, 5)]:
        p = _payloads(fmt, T, H, W, seed=H * 1000 + W + T)
        fb = R.frame_bytes(fmt, H, W)
        for lo, hi in ranges:
            want = N.hist_ref(p, fmt, H, W, lo, hi)
            assert want.shape == (T, nb) and int(want.sum(dtype=np.int64)) <= T * (H // 2) * (W // 2)
            filled = max(filled, int((want > 0).sum(axis=1).max()))
            if T == 5 and H >= 2 and W >= 2:
                assert want[2, 0] == (H // 2) * (W // 2) and want[3].sum() == 0             # the constant frame and the frame without an estimate
            for off in ((0, 1, 3) if bits == 8 else (0, 2)):                    # 8 bit: payloads at odd addresses as well (element-wise loads)
                if (H, W) == (720, 1280) and off == 3:
                    continue
                buf = torch.zeros(T * fb + 16, dtype=torch.uint8, device="cuda")
                src = buf[off:off + T * fb].view(T, fb)
                src.copy_(torch.from_numpy(p))
                assert src.data_ptr() % 16 == off
                g = torch.from_numpy(np.full(T * nb + 2 * GUARD, 0xA5A5A5A5, np.uint32)).cuda()      # dst starts as garbage: overwritten, not added to
                out = g[GUARD:GUARD + T * nb].view(T, nb)
                got = noise_hist_yuv(src, f, H, W, lo, hi, out=out)
                assert got.shape == (T, nb) and got.dtype == torch.uint32
                first = got.cpu().numpy().copy()
                assert np.array_equal(first, want), (fmt, H, W, T, lo, hi, off)
                noise_hist_yuv(src, f, H, W, lo, hi, out=out)                   # a second call into what is now there: the same words
                b = g.cpu().numpy()
                assert np.array_equal(b[GUARD:GUARD + T * nb].reshape(T, nb), want), (fmt, H, W, T, lo, hi, off, "second call")
                assert (b[:GUARD] == 0xA5A5A5A5).all() and (b[GUARD + T * nb:] == 0xA5A5A5A5).all()
    assert filled >= nb // 2                                                    # the noisy frames do reach the high bins
    fmt_full = R.Fmt(bits, chroma, R.BT601, R.FULL)
    got = noise_hist_yuv(torch.from_numpy(p).cuda(), yuv_fmt(*fmt_full), H, W)                      # allocating form, the format's own lo / hi
    assert got.dtype == torch.uint32 and np.array_equal(got.cpu().numpy(), N.hist_ref(p, fmt_full, H, W, *N.clip_codes(fmt_full)))


def test_noise_hist_refuses_bad_arguments():
    lib = L.load()
    f = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(2 * 2047 + 8, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    src, d = buf.data_ptr(), dst.data_ptr()
    call = lib.sn_yuv_noise_hist
    assert call(src, f, d, 16, 235, 1, 8, 8, s) == 0
    assert call(src, yuv_fmt(9, 0, 0, 0), d, 16, 235, 1, 8, 8, s) == -22                 # bits
    assert call(src, yuv_fmt(12, 0, 0, 0), d, 16, 235, 1, 8, 8, s) == -22
    assert call(src, yuv_fmt(8, 3, 0, 0), d, 16, 235, 1, 8, 8, s) == -22                  # chroma code
    assert call(src, yuv_fmt(8, -1, 0, 0), d, 16, 235, 1, 8, 8, s) == -22
    for T, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8)):
        assert call(src, f, d, 16, 235, T, H, W, s) == -22
    for k in (1, 2, 3):
        assert call(src, f, d + k, 16, 235, 1, 8, 8, s) == -22                           # dst is uint32
    assert call(src + 1, yuv_fmt(10, 0, 0, 0), d, 64, 940, 1, 8, 8, s) == -22             # 16-bit samples at an odd address
    assert call(src + 1, f, d, 16, 235, 1, 8, 8, s) == 0                                  # 8-bit samples may lie anywhere
    assert call(None, f, d, 16, 235, 1, 8, 8, s) == -22 and call(src, f, None, 16, 235, 1, 8, 8, s) == -22
    assert call(src, None, d, 16, 235, 1, 8, 8, s) == -22
    assert call(src, f, d, 236, 235, 1, 8, 8, s) == -22                                   # lo > hi
    assert call(src, f, d, 235, 235, 1, 8, 8, s) == 0                                     # lo == hi: legal, nothing counts
    assert call(src, f, d, 16, 235, 1, 1, 9, s) == 0 and call(src, f, d, 16, 235, 1, 9, 1, s) == 0     # no whole block: legal, zeros
    torch.cuda.synchronize()
    assert int(dst.abs().sum()) == 0                                                      # every legal call above counted nothing (codes 0) ...
    assert call(src, f, d, -1, 235, 2, 8, 8, s) == 0
    torch.cuda.synchronize()
    h = dst.cpu().numpy()
    assert h[0] == 16 and h[511] == 16 and int(np.abs(h).sum()) == 32                      # ... and with lo = -1 two frames of 16 blocks land in bin 0


# ---- the restorer -----------------------------------------------------------------------------------------------------------------------------
H, W, ONE_LEN, FRAMES = 71, 99, 5, 26


def noisy_clip(sigma=10.0, seed=4):
    """26 frames of the synthetic sharp clip at 71 x 99 with Gaussian noise added to the 8-bit R'G'B' codes, as 4:2:0 payloads."""
    rgb = synth.sharp_clip(FRAMES, H, W, seed).astype(np.float64)
    rgb = np.clip(np.rint(rgb + np.random.default_rng(seed).normal(0.0, sigma, rgb.shape)), 0, 255).astype(np.uint8)
    return list(S.payloads_of(rgb, H, W))


def run(net, pay, h, w, one_len, sigma, **kw):
    vr = restore.VideoRestorer(net, one_len, sigma=sigma, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*S.FMT420), h, w))
    return out, vr.stats


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def host_sigmas(pay, h, w, one_len, cuts=(), clamp=(0.0, 50.0)):
    """What the restorer must report: the histograms restated in numpy, through the same float64 function, over the frames each window is fed."""
    fmt = S.FMT420
    hist = N.hist_ref(np.stack(pay), fmt, h, w, *N.clip_codes(fmt))
    per = [noise.frame_sigma(x, fmt.bits, fmt.matrix, fmt.range) for x in hist]
    frames = [[per[i] for i in idx] for idx in N.window_inputs(len(pay), one_len, cuts)]
    return frames, [noise.window_sigma(f, clamp) for f in frames]


@pytest.mark.parametrize("cuts", [None, [7, 12]], ids=["one clip", "cuts 7 12"])
def test_auto_sigma_equals_the_host_restatement_and_the_bytes_of_the_listed_sigmas(cuts):
    pay = noisy_clip()
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    want_frames, want = host_sigmas(pay, H, W, ONE_LEN, cuts or ())
    assert len(want) == 6 and len(set(want)) > 1 and all(0.0 < s < 50.0 for s in want)
    outs = {}
    for pipe in (True, False):
        out, stats = run(net, pay, H, W, ONE_LEN, "auto", pipeline=pipe, scene_cuts=cuts)
        assert len(out) == FRAMES and stats["frames"] == FRAMES
        assert stats["window_frame_sigma"] == want_frames                                 # floats compared with ==: the same integers, the same function
        assert stats["window_sigma"] == want
        assert stats["noise_launches"] == stats["windows"] == len(want)
        outs[pipe] = out
    assert same(outs[True], outs[False])
    listed, stats = run(net, pay, H, W, ONE_LEN, list(want), scene_cuts=cuts)
    assert same(listed, outs[True])
    assert stats["window_sigma"] == want and stats["noise_launches"] == 0 and "window_frame_sigma" not in stats
    fixed, _ = run(net, pay, H, W, ONE_LEN, 10.0, scene_cuts=cuts)
    assert not same(fixed, outs[True])                                                    # the sigma does reach the network
    with pytest.raises(ValueError, match=f"window {len(want) - 1}"):
        run(net, pay, H, W, ONE_LEN, list(want[:-1]), scene_cuts=cuts)


def test_a_number_gives_the_bytes_of_the_hand_assembled_windows_without_touching_the_estimator():
    pay = noisy_clip()
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    want = by_hand(net, pay, S.FMT420, H, W, ONE_LEN, 10.0)                               # ingest -> forward(noise_map = 10 / 255) -> egress, nothing else
    for pipe in (True, False):
        got, stats = run(net, pay, H, W, ONE_LEN, 10.0, pipeline=pipe)
        assert same(got, want), pipe
        assert stats["noise_launches"] == 0 and stats["window_sigma"] == [10.0] * 6 and "window_frame_sigma" not in stats
    got, stats = run(net, pay, H, W, ONE_LEN, [10.0] * 6)                                 # the list form of the same number: the same bytes
    assert same(got, want)
    clamped, stats = run(net, pay, H, W, ONE_LEN, "auto", sigma_clamp=(10.0, 10.0))        # and auto clamped onto it
    assert stats["window_sigma"] == [10.0] * 6 and stats["noise_launches"] == 6 and same(clamped, want)
    deblur = restore.load_net("deblur_small", "synthetic", "bf16")
    for bad in ("auto", [10.0]):
        with pytest.raises(ValueError, match="denoise"):
            restore.VideoRestorer(deblur, ONE_LEN, sigma=bad)
    out, stats = run(deblur, pay[:6], H, W, ONE_LEN, 10.0)                                # a number stays ignored there
    assert len(out) == 6 and stats["noise_launches"] == 0 and "window_sigma" not in stats


def test_two_noise_levels_in_one_clip_give_window_sigmas_near_each():
    c = N.TWO_LEVEL
    pay = list(N.two_level_payloads())
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    out, stats = run(net, pay, c["h"], c["w"], c["one_len"], "auto")
    ws = stats["window_sigma"]
    print("two-level clip, window sigmas on the device:", [round(x, 3) for x in ws])
    assert len(out) == c["n"] and ws == host_sigmas(pay, c["h"], c["w"], c["one_len"])[1]
    for k in (0, 1):                                                                      # input frames 0 .. 11: sigma 5
        assert abs(ws[k] - 5.0) <= N.margin(5.0), (k, ws[k])
    for k in (3, 4, 5):                                                                   # input frames 13 .. 25: sigma 30
        assert abs(ws[k] - 30.0) <= N.margin(30.0), (k, ws[k])


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_restore_video_cli_with_sigma_auto_in_a_child_process_gives_the_api_bytes(tmp_path):
    pay = noisy_clip()
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, dst2, sig = tmp_path / "in.y4m", tmp_path / "out.y4m", tmp_path / "out2.y4m", tmp_path / "sigma.txt"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in pay:
            wr.write(p)
    base = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "denoise_small", "--checkpoint", "synthetic",
            "--dtype", "bf16", "--one_len", str(ONE_LEN)]
    r = subprocess.run(base + ["--sigma", "auto", "--sigma_out", str(sig), str(src), str(dst)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "done: 26 frames" in r.stderr and "sigma (auto" in r.stderr
    want = host_sigmas(pay, H, W, ONE_LEN)[1]                                             # 71 < 720: the CLI's default matrix is BT.601, as S.FMT420
    assert noise.parse_sigmas(sig.read_text()) == want

    def read(path):
        with open(path, "rb") as fh:
            return list(y4m.Y4MReader(fh))
    got = read(dst)
    net = restore.load_net("denoise_small", "synthetic", "bf16")
    api, _ = run(net, pay, H, W, ONE_LEN, "auto")
    assert same(got, api)
    r = subprocess.run(base + ["--sigma", str(sig), str(src), str(dst2)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "sigma (listed" in r.stderr and same(read(dst2), got)
