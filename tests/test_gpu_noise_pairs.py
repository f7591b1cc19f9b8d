"""-m gpu: ``sn_yuv_noise_hist_pairs`` and ``sn_yuv_noise_hist_pairs_bands`` against their numpy restatements (tests/noise_pairs_ref.py) bit for bit,
and the video restorer with ``sigma_estimator="temporal"`` / ``"min"`` against the host restatement on the same payloads exactly (integer histograms
through the same float64 functions) and against runs that are handed the sigmas or the curves as lists, byte for byte.  No tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nlf_ref as F
import noise_pairs_ref as NP
import noise_ref as N
import picture_ref as P
import scene_ref as S
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import noise, restore, y4m
from shiftnet_amd.io_edges import noise_hist_pairs_bands_yuv, noise_hist_pairs_yuv, yuv_fmt
from test_gpu_noise import FRAMES, H, ONE_LEN, W, _payloads, noisy_clip, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                                                                      # uint32 words before and after dst
GARBAGE = 0xA5A5A5A5


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
def pair_payloads(fmt, T, H, W, seed):
    """``_payloads`` of tests/test_gpu_noise.py (a ramp plus noise whose level differs from frame to frame, clipped codes included; with T = 5 frame 2
    is one constant code and frame 3 is black, so pairs 2 and 3 count nothing), and with T = 5 frame 1 repeats frame 0: pair 0 has all its mass in bin 0."""
    p = _payloads(fmt, T, H, W, seed)
    if T == 5:
        p[1] = p[0]
    return p


def uniform_payloads(fmt, T, H, W, seed):
    """Every code equally likely, independently: noise as strong as the format can hold.  v reaches far beyond NBV and fills more than half of NBP's bins."""
    rng = np.random.default_rng(seed)
    n = R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)
    p = rng.integers(0, 1 << fmt.bits, (T, n))
    return p.astype(np.uint8) if fmt.bits == 8 else p.astype("<u2").view(np.uint8).reshape(T, -1)


def check_both(p, fmt, H, W, lo, hi, off=0, rect=None):
    """Both kernels on payloads ``p`` placed ``off`` bytes from 16-byte alignment against the restatement: dst starts as garbage inside guard words,
    is overwritten, a second call gives the same words, the guards stay.  Returns the two expected arrays."""
    f = yuv_fmt(*fmt)
    T, fb = p.shape
    buf = torch.zeros(T * fb + 16, dtype=torch.uint8, device="cuda")
    src = buf[off:off + T * fb].view(T, fb)
    src.copy_(torch.from_numpy(p))
    assert src.data_ptr() % 16 == off
    wants = []
    for call, ref, shape in ((noise_hist_pairs_yuv, NP.hist_pairs_ref, (NP.nbp(fmt.bits),)),
                             (noise_hist_pairs_bands_yuv, NP.hist_pairs_bands_ref, (16, F.nbv(fmt.bits)))):
        want = ref(p, fmt, H, W, lo, hi, rect)
        words = (T - 1) * int(np.prod(shape))
        assert want.shape == (T - 1,) + shape
        g = torch.from_numpy(np.full(words + 2 * GUARD, GARBAGE, np.uint32)).cuda()
        out = g[GUARD:GUARD + words].view((T - 1,) + shape)
        for nth in (1, 2):
            got = call(src, f, H, W, lo, hi, out=out, rect=rect)
            assert got is out and got.dtype == torch.uint32
            b = g.cpu().numpy()
            assert np.array_equal(b[GUARD:GUARD + words].reshape(want.shape), want), (call.__name__, fmt, H, W, T, lo, hi, off, rect, nth)
            assert (b[:GUARD] == GARBAGE).all() and (b[GUARD + words:] == GARBAGE).all()
        wants.append(want)
    return wants


@pytest.mark.parametrize("chroma", [R.C444, R.C420_CENTER, R.C420_LEFT], ids=["444", "420c", "420l"])
@pytest.mark.parametrize("bits", [8, 10])
def test_pair_histograms_equal_the_numpy_restatement_exactly_overwrite_and_write_nothing_else(bits, chroma):
    fmt = R.Fmt(bits, chroma, R.BT709, R.LIMITED)
    ranges = [N.clip_codes(R.Fmt(bits, chroma, 0, R.LIMITED)), N.clip_codes(R.Fmt(bits, chroma, 0, R.FULL))]
    # (2, 2): one block; (1, 9), (9, 1): no whole block; (37, 53): odd, a right-edge unit of two blocks; (66, 130): 33 x 17 = 561 units, a last unit of one block
    for (H, W), T in [(s, t) for s in [(64, 64), (37, 53), (2, 2), (1, 9), (9, 1), (66, 130)] for t in (2, 5)]:
        p = pair_payloads(fmt, T, H, W, seed=H * 1000 + W + T)
        blocks = (H // 2) * (W // 2)
        for lo, hi in ranges:
            for off in ((0, 1, 3) if bits == 8 else (0, 2)):                    # 8 bit: payloads at odd addresses as well (element-wise loads)
                flat, bands = check_both(p, fmt, H, W, lo, hi, off)
            assert int(flat.sum(dtype=np.int64)) <= (T - 1) * blocks
            assert np.array_equal(bands.sum(axis=1, dtype=np.int64)[:, :-1], flat[:, :bands.shape[2] - 1])      # the same blocks, split and saturated
            if blocks == 0:
                assert flat.sum() == 0 and bands.sum() == 0
            elif T == 5:
                assert flat[0, 0] == flat[0].sum() and (flat[0, 0] > 0 or blocks < 4)      # the repeated frame: every counted block in bin 0
                assert flat[2].sum() == 0 and flat[3].sum() == 0                 # the black frame: its two pairs count nothing
                assert flat[1, 1:].sum() > 0 or blocks < 4
    # the allocating forms, the format's own lo / hi
    fmt_full = R.Fmt(bits, chroma, R.BT601, R.FULL)
    dev = torch.from_numpy(p).cuda()
    got = noise_hist_pairs_yuv(dev, yuv_fmt(*fmt_full), H, W)
    assert got.dtype == torch.uint32 and np.array_equal(got.cpu().numpy(), NP.hist_pairs_ref(p, fmt_full, H, W, *N.clip_codes(fmt_full)))
    got = noise_hist_pairs_bands_yuv(dev, yuv_fmt(*fmt_full), H, W)
    assert got.dtype == torch.uint32 and np.array_equal(got.cpu().numpy(), NP.hist_pairs_bands_ref(p, fmt_full, H, W, *N.clip_codes(fmt_full)))


@pytest.mark.parametrize("bits", [8, 10])
def test_pair_histograms_of_the_strongest_noise_fill_the_high_bins_and_come_from_several_workgroups(bits):
    """256 x 512 of uniformly random codes, every block counting (lo = -1, hi = 2^bits): 128 block rows x 64 units = 8192 units, which is four
    workgroups per pair for the flat kernel and two for the band kernel adding into dst."""
    fmt = R.Fmt(bits, R.C420_CENTER, R.BT709, R.FULL)
    H, W, T = 256, 512, 3
    p = uniform_payloads(fmt, T, H, W, seed=bits)
    flat, bands = check_both(p, fmt, H, W, -1, 1 << bits)
    assert (flat.sum(axis=1) == (H // 2) * (W // 2)).all()
    assert int((flat > 0).sum(axis=1).max()) >= NP.nbp(bits) // 2                # at least half of NBP's bins fill
    assert (bands[:, :, -1].sum(axis=1) > 0).all() and (bands.sum(axis=2) > 0).sum() >= 2 * 4      # the saturating bin is hit; several bands


@pytest.mark.parametrize("bits", [8, 10])
def test_pair_histograms_of_a_rectangle_are_the_cropped_streams(bits):
    f420, f444 = R.Fmt(bits, R.C420_CENTER, R.BT709, R.LIMITED), R.Fmt(bits, R.C444, R.BT709, R.LIMITED)
    # (16, 2, 32, 20) inside 64 x 64: rows of the rectangle start 16-byte aligned, the wide loads; (3, 1, 41, 29) inside 37 x 53 at 4:4:4: element-wise
    for fmt, (H, W), rect in ((f420, (64, 64), (16, 2, 32, 20)), (f444, (64, 64), (16, 2, 32, 20)), (f444, (37, 53), (3, 1, 41, 29))):
        p = pair_payloads(fmt, 5, H, W, seed=H + W + bits)
        lo, hi = N.clip_codes(fmt)
        flat, bands = check_both(p, fmt, H, W, lo, hi, rect=rect)
        crop = P.crop_payloads(p, fmt, H, W, rect)
        assert np.array_equal(flat, NP.hist_pairs_ref(crop, fmt, rect[3], rect[2], lo, hi)) and flat[1].sum() > 0
        assert np.array_equal(bands, NP.hist_pairs_bands_ref(crop, fmt, rect[3], rect[2], lo, hi))
    with pytest.raises(ValueError):                                             # the illegal odd origin at 4:2:0
        noise_hist_pairs_yuv(torch.from_numpy(p[:, :R.frame_bytes(f420, 37, 53)].copy()).cuda(), yuv_fmt(*f420), 37, 53, rect=(3, 2, 40, 28))


@pytest.mark.parametrize("name", ["sn_yuv_noise_hist_pairs", "sn_yuv_noise_hist_pairs_bands"])
def test_pair_histograms_refuse_bad_arguments(name):
    lib = L.load()
    f = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(2 * 16 * 512 + 8, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    src, d = buf.data_ptr(), dst.data_ptr()
    call = getattr(lib, name)
    assert call(src, f, None, d, 16, 235, 2, 8, 8, s) == 0
    assert call(src, f, L.YuvRect(2, 2, 4, 4), d, 16, 235, 2, 8, 8, s) == 0
    for bad in (L.YuvRect(1, 2, 4, 4), L.YuvRect(2, 1, 4, 4), L.YuvRect(2, 2, 3, 4), L.YuvRect(2, 2, 8, 4), L.YuvRect(-2, 0, 4, 4), L.YuvRect(0, 0, 0, 4)):
        assert call(src, f, bad, d, 16, 235, 2, 8, 8, s) == -22                              # 4:2:0: odd origin, odd w inside, outside the frame, empty
    assert call(src, yuv_fmt(8, 0, 0, 0), L.YuvRect(1, 3, 3, 5), d, 16, 235, 2, 8, 8, s) == 0   # 4:4:4: any integers
    assert call(src, yuv_fmt(9, 0, 0, 0), None, d, 16, 235, 2, 8, 8, s) == -22
    assert call(src, yuv_fmt(12, 0, 0, 0), None, d, 16, 235, 2, 8, 8, s) == -22
    assert call(src, yuv_fmt(8, 3, 0, 0), None, d, 16, 235, 2, 8, 8, s) == -22
    for T, H, W in ((1, 8, 8), (0, 8, 8), (-1, 8, 8), (65537, 8, 8), (65536, 8, 8), (2, 0, 8), (2, 8, 0)):   # T = 1: no pair; T - 1 > 65535
        assert call(src, f, None, d, 16, 235, T, H, W, s) == -22
    for k in (1, 2, 3):
        assert call(src, f, None, d + k, 16, 235, 2, 8, 8, s) == -22                         # dst is uint32
    assert call(src + 1, yuv_fmt(10, 0, 0, 0), None, d, 64, 940, 2, 8, 8, s) == -22           # 16-bit samples at an odd address
    assert call(src + 1, f, None, d, 16, 235, 2, 8, 8, s) == 0                                # 8-bit samples may lie anywhere
    assert call(None, f, None, d, 16, 235, 2, 8, 8, s) == -22 and call(src, f, None, None, 16, 235, 2, 8, 8, s) == -22
    assert call(src, None, None, d, 16, 235, 2, 8, 8, s) == -22
    assert call(src, f, None, d, 236, 235, 2, 8, 8, s) == -22                                 # lo > hi
    assert call(src, f, None, d, -(1 << 24) - 1, 235, 2, 8, 8, s) == -22 and call(src, f, None, d, 16, (1 << 24) + 1, 2, 8, 8, s) == -22
    assert call(src, f, None, d, 235, 235, 2, 8, 8, s) == 0                                   # lo == hi: legal, nothing counts
    assert call(src, f, None, d, 16, 235, 2, 1, 9, s) == 0 and call(src, f, None, d, 16, 235, 2, 9, 1, s) == 0     # no whole block: legal, zeros
    torch.cuda.synchronize()
    assert int(dst.abs().sum()) == 0                                                          # every legal call above counted nothing (codes 0) ...
    assert call(src, f, None, d, -1, 235, 3, 8, 8, s) == 0
    torch.cuda.synchronize()
    h = dst.cpu().numpy()
    words = 1021 if name == "sn_yuv_noise_hist_pairs" else 16 * 128
    assert h[0] == 16 and h[words] == 16 and int(np.abs(h).sum()) == 32                        # ... with lo = -1: S + 8 = 8 -> band 0, bin 0, two pairs
    with pytest.raises(ValueError, match="two payloads"):
        noise_hist_pairs_yuv(buf[:96].view(1, 96), f, 8, 8)


# ---- the restorer -----------------------------------------------------------------------------------------------------------------------------
FMT = S.FMT420
RECT = (8, 6, 64, 48)                                                                          # 4:2:0: even origin and size, inside 99 x 71


@pytest.fixture(scope="module")
def net():
    return restore.load_net("denoise_small", "synthetic", "bf16")


@pytest.fixture(scope="module")
def clip():
    return noisy_clip()


def run(net, pay, sigma="auto", h=H, w=W, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, sigma=sigma, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*FMT), h, w))
    return out, vr.stats


@pytest.fixture(scope="module")
def spatial(net, clip):
    """The clip restored without the argument: shared by the tests below and left unchanged."""
    return run(net, clip)


@pytest.fixture(scope="module")
def by_min(net, clip):
    return run(net, clip, sigma_estimator="min")


def check_stats(stats, est, estimator, level=False):
    """Every new stats entry equals the host restatement exactly (floats compared with ==: the same integers through the same functions)."""
    n = len(est["sigma"])
    assert stats["sigma_estimator"] == estimator and stats["windows"] == n
    assert stats["window_frame_sigma"] == est["frame_sigma"] and stats["window_pair_sigma"] == est["pair_sigma"]
    assert stats["window_sigma_spatial"] == est["spatial"] and stats["window_sigma_temporal"] == est["temporal"]
    assert stats["window_sigma"] == est["sigma"]
    assert stats["noise_launches"] == stats["noise_pairs_launches"] == n
    assert all(len(ps) == len(fs) - 1 for ps, fs in zip(stats["window_pair_sigma"], stats["window_frame_sigma"]))
    if level:
        assert stats["window_nlf"] == est["nlf"] and stats["nlf_launches"] == stats["nlf_pairs_launches"] == stats["nlf_map_launches"] == n
    else:
        assert "nlf_pairs_launches" not in stats and "window_nlf" not in stats


@pytest.mark.parametrize("estimator", ["min", "temporal"])
def test_estimator_stats_equal_the_host_restatement_and_the_bytes_of_the_listed_sigmas(net, clip, spatial, by_min, estimator):
    est = NP.window_estimates(clip, FMT, H, W, ONE_LEN, estimator)
    assert len(est["sigma"]) == 6 and all(t is not None for t in est["temporal"]) and all(0.0 < s < 50.0 for s in est["sigma"])
    out, stats = by_min if estimator == "min" else run(net, clip, sigma_estimator=estimator)
    assert len(out) == FRAMES and stats["frames"] == FRAMES
    check_stats(stats, est, estimator)
    want = [min(a, b) for a, b in zip(est["spatial"], est["temporal"])] if estimator == "min" else est["temporal"]
    assert stats["window_sigma"] == want                                                      # nothing is clamped on this clip
    assert stats["window_frame_sigma"] == spatial[1]["window_frame_sigma"]                     # the spatial statistic still runs, unchanged
    listed, lstats = run(net, clip, sigma=list(stats["window_sigma"]))
    assert same(listed, out) and lstats["noise_launches"] == 0 and "sigma_estimator" not in lstats
    if estimator == "temporal":                                                               # the content of this clip moves: temporal reads higher
        assert all(t > s for t, s in zip(est["temporal"], est["spatial"]))
        assert stats["window_sigma"] != spatial[1]["window_sigma"] and not same(out, spatial[0])       # the estimator does reach the network
    else:                                                                                     # ... and the lower of the two is the spatial one: its bytes
        assert stats["window_sigma"] == spatial[1]["window_sigma"] and same(out, spatial[0])


def test_estimator_with_scene_cuts_a_fixed_picture_and_serial(net, clip, by_min):
    cuts = [7, 12]
    est = NP.window_estimates(clip, FMT, H, W, ONE_LEN, "min", cuts=cuts)
    out, stats = run(net, clip, sigma_estimator="min", scene_cuts=cuts)
    check_stats(stats, est, "min")
    assert len(est["sigma"]) == 6 and same(run(net, clip, sigma=list(stats["window_sigma"]), scene_cuts=cuts)[0], out)         # scenes of 7, 5 and 14 frames
    est = NP.window_estimates(clip, FMT, H, W, ONE_LEN, "min", rect=RECT)                     # the pair statistic sees the window's rectangle
    out, stats = run(net, clip, sigma_estimator="min", picture=RECT)
    check_stats(stats, est, "min")
    assert est["pair_sigma"] != NP.window_estimates(clip, FMT, H, W, ONE_LEN, "min")["pair_sigma"]
    assert est["sigma"][0] == est["temporal"][0] < est["spatial"][0]                          # inside the rectangle the first window takes the temporal one
    assert same(run(net, clip, sigma=list(stats["window_sigma"]), picture=RECT)[0], out)
    crop = list(P.crop_payloads(np.stack(clip), FMT, H, W, RECT))                             # ... which is the cropped stream's estimate
    assert run(net, crop, h=RECT[3], w=RECT[2], sigma_estimator="min")[1]["window_pair_sigma"] == stats["window_pair_sigma"]
    serial, sstats = run(net, clip, sigma_estimator="min", pipeline=False)
    assert same(serial, by_min[0]) and {k: v for k, v in sstats.items() if "_ms" not in k and k != "forward_s"} == \
        {k: v for k, v in by_min[1].items() if "_ms" not in k and k != "forward_s"}


@pytest.mark.parametrize("frames", [1, 2])
def test_clips_of_one_and_two_frames_have_only_repeat_pairs_and_the_bytes_of_spatial(net, clip, frames):
    """The planner clamps where n <= 2: a clip of one frame is fed as that frame five times.  The clip of two frames here is one frame twice -- a
    duplicated frame in the footage -- fed as six copies.  Every pair is a repeat, there is no temporal estimate, and the spatial one is used."""
    pay = [clip[0]] * frames
    est = NP.window_estimates(pay, FMT, H, W, ONE_LEN, "min")
    for estimator in ("min", "temporal"):
        out, stats = run(net, pay, sigma_estimator=estimator)
        check_stats(stats, est, estimator)                                                   # no temporal estimate: both words give the spatial sigma
        assert stats["window_pair_sigma"] == [[None] * (3 + frames)] and stats["window_sigma_temporal"] == [None]
        ref, rstats = run(net, pay)
        assert stats["window_sigma"] == rstats["window_sigma"] and len(out) == frames and same(out, ref)


def test_a_clip_of_two_different_frames_has_one_real_pair_among_the_clamped_repeats(net, clip):
    pay = clip[:2]                                                                            # fed as 0 0 0 1 1 1: only the pair (0, 1) is not a repeat
    est = NP.window_estimates(pay, FMT, H, W, ONE_LEN, "temporal")
    out, stats = run(net, pay, sigma_estimator="temporal")
    check_stats(stats, est, "temporal")
    ps = stats["window_pair_sigma"][0]
    assert [x is None for x in ps] == [True, True, False, True, True] and stats["window_sigma_temporal"] == [ps[2]] == stats["window_sigma"]


def test_level_with_min_equals_the_host_restatement_and_the_bytes_of_the_listed_curves(net, clip):
    est = NP.window_estimates(clip, FMT, H, W, ONE_LEN, "min", level=True)
    out, stats = run(net, clip, sigma_estimator="min", noise_model="level")
    check_stats(stats, est, "min", level=True)
    assert all(max(c) > 0.0 for c in stats["window_nlf"])
    lo, hi = N.clip_codes(FMT)
    flat_curves = [noise.window_curve(F.hist_bands_ref(np.stack([clip[i] for i in idx]), FMT, H, W, lo, hi), FMT.bits, FMT.matrix, FMT.range)
                   for idx in N.window_inputs(FRAMES, ONE_LEN)]
    assert stats["window_nlf"] != flat_curves                                                 # the pair statistic does reach the curve
    listed, lstats = run(net, clip, sigma=10.0, noise_model=stats["window_nlf"])
    assert same(listed, out) and lstats["nlf_launches"] == 0 and "nlf_pairs_launches" not in lstats


def test_a_second_restore_on_the_same_object_and_the_spatial_default(net, clip, spatial, by_min):
    vr = restore.VideoRestorer(net, ONE_LEN, sigma="auto", sigma_estimator="min")
    first = list(vr.restore(iter(clip), yuv_fmt(*FMT), H, W))
    s1 = dict(vr.stats)
    second = list(vr.restore(iter(clip), yuv_fmt(*FMT), H, W))
    assert same(first, by_min[0]) and same(second, first)
    for k in ("window_sigma", "window_pair_sigma", "window_sigma_temporal", "window_sigma_spatial", "noise_pairs_launches", "noise_launches"):
        assert vr.stats[k] == s1[k] == by_min[1][k], k
    # default or explicit "spatial": the bytes and the stats keys of a restorer built without the argument, and no pair kernel
    out, stats = run(net, clip, sigma_estimator="spatial")
    assert same(out, spatial[0]) and set(stats) == set(spatial[1]) and stats["window_sigma"] == spatial[1]["window_sigma"]
    assert not any("pair" in k or "estimator" in k or k in ("window_sigma_spatial", "window_sigma_temporal") for k in stats)
    vr = restore.VideoRestorer(net, ONE_LEN, sigma="auto")
    list(vr.restore(iter(clip[:6]), yuv_fmt(*FMT), H, W))
    assert vr.run.launches["noise_pairs"] == 0 and vr.run.launches["nlf_pairs"] == 0 and all(s.noise.pairs is None and s.noise.pair_bands is None for s in vr.slots)
    fixed, fstats = run(net, clip[:6], sigma=10.0, sigma_estimator="spatial")                 # with a number "spatial" is today's call
    assert fstats["noise_launches"] == 0 and "sigma_estimator" not in fstats


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_restore_video_cli_with_sigma_estimator_min_in_a_child_process_gives_the_api_bytes(tmp_path, clip, by_min):
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, sig = tmp_path / "in.y4m", tmp_path / "out.y4m", tmp_path / "sigma.txt"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in clip:
            wr.write(p)
    cmd = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "denoise_small", "--checkpoint", "synthetic",
           "--dtype", "bf16", "--one_len", str(ONE_LEN), "--sigma", "auto", "--sigma_estimator", "min", "--sigma_out", str(sig), str(src), str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)                      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    assert "done: 26 frames" in r.stderr and "sigma (auto, min" in r.stderr
    assert noise.parse_sigmas(sig.read_text()) == by_min[1]["window_sigma"]                   # 71 < 720: the CLI's default matrix is BT.601, as FMT
    with open(dst, "rb") as fh:
        assert same(list(y4m.Y4MReader(fh)), by_min[0])
