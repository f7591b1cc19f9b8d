"""-m gpu: ``sn_yuv_block_motion``, ``sn_yuv_noise_hist_pairs_mv`` and ``sn_yuv_noise_hist_pairs_bands_mv`` against their numpy restatements
(tests/motion_ref.py) word for word, and the video restorer with ``sigma_motion="blocks"`` against the host restatement on the same payloads
exactly (integer vectors and histograms through the same float64 functions) and against runs that are handed the sigmas or the curves as lists,
byte for byte.  No tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import motion_ref as M
import noise_pairs_ref as NP
import noise_ref as N
import picture_ref as P
import scene_ref as S
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import noise, restore, y4m
from shiftnet_amd.io_edges import block_motion_yuv, noise_hist_pairs_bands_mv_yuv, noise_hist_pairs_mv_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                                                                      # words (bytes for mv) before and after every output
GARBAGE, GARBAGE8 = 0xA5A5A5A5, 0x5A
F8, F8_420, F10 = R.Fmt(8, R.C444, R.BT709, R.LIMITED), R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED), R.Fmt(10, R.C420_LEFT, R.BT709, R.LIMITED)
# (2, 2): one 2 x 2 block; (16, 16): one full vector block, only (0, 0) admissible; (18, 34), (37, 70): ragged blocks at the right and lower edge, odd
# sizes; (64, 96): 4 x 6 full blocks, one full run of four and a run of two; (32, 288): 18 blocks per row, four full runs and one of two
SIZES = [(2, 2), (16, 16), (18, 34), (37, 70), (64, 96), (32, 288)]


# ---- payloads -------------------------------------------------------------------------------------------------------------------------------
def payloads(fmt, T, H, W, kind, seed=0):
    """``texture``: a random texture with features of a few pixels, moving (2, -3) per frame, plus noise; at 10 bit a sprinkling of stored words above
    1023, up to 65535.  ``constant``: one code everywhere.  ``stripes``: vertical stripes of period 4 that move 6 to the right per frame."""
    rng = np.random.default_rng(seed + 17 * H + W)
    top = (1 << fmt.bits) - 1
    ch, cw = R.chroma_shape(fmt, H, W)
    out = []
    if kind == "texture":
        m = 4 * T + 8
        canvas = np.kron(rng.integers(top // 8, top - top // 8, ((H + 2 * m) // 3 + 1, (W + 2 * m) // 3 + 1)), np.ones((3, 3), np.int64))
    for t in range(T):
        if kind == "texture":
            Y = canvas[m - 2 * t:m - 2 * t + H, m + 3 * t:m + 3 * t + W] + np.rint(rng.normal(0.0, top / 64.0, (H, W))).astype(np.int64)
            Y = np.clip(Y, 0, top)
            if fmt.bits == 10:
                wild = rng.random((H, W)) < 0.02
                Y = np.where(wild, rng.integers(1024, 65536, (H, W)), Y)
        elif kind == "constant":
            Y = np.full((H, W), top // 3, np.int64)
        else:
            Y = np.repeat(((top // 4) + (top // 8) * ((np.arange(W) - 6 * t) % 4))[None], H, axis=0)
        out.append(R.join_planes(Y, rng.integers(0, top + 1, (ch, cw)), rng.integers(0, top + 1, (ch, cw)), fmt))
    return np.stack(out)


def on_device(p, off=0, slack=0):
    """The payloads on the device, ``off`` bytes from 16-byte alignment, with ``slack`` bytes of zeros allocated before and after."""
    T, fb = p.shape
    lead = (slack + 15) // 16 * 16
    buf = torch.zeros(lead + off + T * fb + slack + 16, dtype=torch.uint8, device="cuda")
    src = buf[lead + off:lead + off + T * fb].view(T, fb)
    src.copy_(torch.from_numpy(p))
    assert src.data_ptr() % 16 == off
    return src


def guarded(shape, dtype):
    """A tensor of ``shape`` full of garbage inside GUARD guard elements on both sides -> (the whole buffer, the view)."""
    n = int(np.prod(shape))
    if dtype == torch.int8:
        g = torch.full((n + 2 * GUARD,), GARBAGE8, dtype=torch.int8, device="cuda")
    else:
        g = torch.from_numpy(np.full(n + 2 * GUARD, GARBAGE, np.uint32)).cuda()
    return g, g[GUARD:GUARD + n].view(shape)


def guards_intact(g, n):
    b = g.cpu().numpy()
    mark = GARBAGE8 if b.dtype == np.int8 else GARBAGE
    return bool((b[:GUARD] == mark).all() and (b[GUARD + n:] == mark).all())


def check_motion(p, fmt, H, W, off=0, rect=None):
    """The matcher on payloads ``p`` against the restatement: mv and sad start as garbage inside guards, are overwritten, a second call gives the same
    words, the guards stay.  Returns the device vectors (a contiguous copy) and the expected arrays."""
    src, f = on_device(p, off), yuv_fmt(*fmt)
    want_mv, want_sad = M.block_motion_ref(p, fmt, H, W, rect)
    gm, mv = guarded(want_mv.shape, torch.int8)
    gs, sad = guarded(want_sad.shape, torch.uint32)
    for nth in (1, 2):
        got = block_motion_yuv(src, f, H, W, rect=rect, out_mv=mv, out_sad=sad)
        assert got[0] is mv and got[1] is sad
        if want_sad.size:
            assert np.array_equal(mv.cpu().numpy(), want_mv), (fmt, H, W, len(p), off, rect, nth)
            assert np.array_equal(sad.cpu().numpy(), want_sad), (fmt, H, W, len(p), off, rect, nth)
        assert guards_intact(gm, want_mv.size) and guards_intact(gs, want_sad.size)
    return src, mv.clone(), want_mv, want_sad


def check_hists(src, p, mv_dev, mv_host, fmt, H, W, lo, hi, rect=None):
    """Both histograms along ``mv`` against the restatement: dst starts as garbage inside guards and is overwritten, twice."""
    f = yuv_fmt(*fmt)
    wants = []
    for call, ref in ((noise_hist_pairs_mv_yuv, M.hist_pairs_mv_ref), (noise_hist_pairs_bands_mv_yuv, M.hist_pairs_bands_mv_ref)):
        want = ref(p, mv_host, fmt, H, W, lo, hi, rect)
        g, out = guarded(want.shape, torch.uint32)
        for nth in (1, 2):
            got = call(src, f, H, W, mv_dev, lo, hi, out=out, rect=rect)
            assert got is out and got.dtype == torch.uint32
            assert np.array_equal(out.cpu().numpy(), want), (call.__name__, fmt, H, W, len(p), lo, hi, rect, nth)
            assert guards_intact(g, want.size)
        wants.append(want)
    return wants


# ---- the matcher --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F8, F8_420, F10], ids=["8bit444", "8bit420", "10bit420"])
def test_block_motion_equals_the_numpy_restatement_exactly_and_writes_nothing_else(fmt):
    for H, W in SIZES:
        for T in (2, 4):
            p = payloads(fmt, T, H, W, "texture", seed=T)
            _, _, mv, sad = check_motion(p, fmt, H, W)
            assert mv.shape == (T - 1,) + noise.motion_grid(H, W) + (2,)
            if (H, W) == (16, 16):
                assert not mv.any() and sad.all()                                # only (0, 0) is admissible
            if (H, W) in ((64, 96), (32, 288)) and fmt.bits == 8:                # the content moves (2, -3): every block that can follow does (at 10 bit
                inner = mv[:, 1:-1, 1:-1] if H == 64 else mv[:, 0, 1:-1]         # the words above 1023 decide; the lower block row of two cannot look down)
                assert (inner == (2, -3)).all()
            if fmt.bits == 10 and H * W >= 1024:
                assert int(sad.max()) > 128 * 1023                               # the stored words above 1023 reach the SAD as they are
    src = on_device(payloads(fmt, 3, 37, 70, "texture"))                         # the allocating form
    mv, sad = block_motion_yuv(src, yuv_fmt(*fmt), 37, 70)
    assert mv.dtype == torch.int8 and sad.dtype == torch.uint32 and tuple(mv.shape) == (2, 3, 5, 2) and tuple(sad.shape) == (2, 3, 5)
    for H, W in ((1, 5), (5, 1)):                                                # no whole 2 x 2 block: empty grids, nothing launched
        mv, sad = block_motion_yuv(on_device(payloads(fmt, 2, H, W, "constant")), yuv_fmt(*fmt), H, W)
        assert tuple(mv.shape) == (1, 0, 0, 2) and tuple(sad.shape) == (1, 0, 0)
        check_motion(payloads(fmt, 2, H, W, "constant"), fmt, H, W)


@pytest.mark.parametrize("fmt", [F8, F10], ids=["8bit", "10bit"])
def test_block_motion_of_constant_frames_and_stripes_follows_the_tie_rule(fmt):
    for H, W in ((18, 34), (37, 70), (32, 288)):
        _, _, mv, sad = check_motion(payloads(fmt, 3, H, W, "constant"), fmt, H, W)
        assert not mv.any() and not sad.any()                                    # 225 equal keys but for the rank: (0, 0)
        _, _, mv, sad = check_motion(payloads(fmt, 3, H, W, "stripes"), fmt, H, W)
        assert not sad.any() and (mv[:, :, 1:] == (0, -2)).all() and (mv[:, :, 0] == (0, 2)).all()      # the nearest alias, the first in the order


def test_block_motion_from_a_payload_base_that_is_not_16_byte_aligned():
    for fmt, offs in ((F8, (1, 3, 8)), (F10, (2, 6))):
        p = payloads(fmt, 3, 37, 70, "texture", seed=9)
        for off in offs:
            check_motion(p, fmt, 37, 70, off)


@pytest.mark.parametrize("bits", [8, 10])
def test_block_motion_and_the_histograms_of_a_rectangle_are_the_cropped_streams(bits):
    f444, f420 = R.Fmt(bits, R.C444, R.BT709, R.LIMITED), R.Fmt(bits, R.C420_CENTER, R.BT709, R.LIMITED)
    for fmt, (H, W), rect in ((f444, (37, 70), (16, 2, 40, 30)), (f420, (64, 96), (16, 2, 64, 44))):
        p = payloads(fmt, 3, H, W, "texture", seed=bits)
        lo, hi = N.clip_codes(fmt)
        src, mv_dev, mv, sad = check_motion(p, fmt, H, W, rect=rect)
        crop = P.crop_payloads(p, fmt, H, W, rect)
        cmv, csad = M.block_motion_ref(crop, fmt, rect[3], rect[2])
        assert np.array_equal(mv, cmv) and np.array_equal(sad, csad) and mv.any()
        flat, bands = check_hists(src, p, mv_dev, mv, fmt, H, W, lo, hi, rect=rect)
        assert np.array_equal(flat, M.hist_pairs_mv_ref(crop, cmv, fmt, rect[3], rect[2], lo, hi)) and flat.sum() > 0
        assert np.array_equal(bands, M.hist_pairs_bands_mv_ref(crop, cmv, fmt, rect[3], rect[2], lo, hi))


# ---- the histograms along the vectors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [F8, F8_420, F10], ids=["8bit444", "8bit420", "10bit420"])
def test_mv_histograms_with_the_matchers_vectors_equal_the_restatement_exactly(fmt):
    ranges = [N.clip_codes(fmt), (-1, 1 << 16)]                                  # the format's codes; every stored word (v saturates at NBP - 1 then)
    # (200, 340): 100 block rows x 43 units = 4300 units, three workgroups per pair for the flat histogram (2048 units each) and two for the band one (4096)
    for (H, W), Ts in [(s, (2, 4)) for s in SIZES + [(1, 5)]] + [((200, 340), (2,))]:
        for T in Ts:
            p = payloads(fmt, T, H, W, "texture", seed=T + 3)
            src = on_device(p)
            mv_dev, _ = block_motion_yuv(src, yuv_fmt(*fmt), H, W)
            mv, _ = M.block_motion_ref(p, fmt, H, W)
            for lo, hi in ranges:
                flat, bands = check_hists(src, p, mv_dev, mv, fmt, H, W, lo, hi)
                blocks = (H // 2) * (W // 2)
                assert int(flat.sum(dtype=np.int64)) <= (T - 1) * ((blocks + 1) // 2)      # measuring blocks only
                assert np.array_equal(bands.sum(axis=1, dtype=np.int64)[:, :-1], flat[:, :bands.shape[2] - 1])
            if (H, W) == (64, 96) and fmt.bits == 8:
                assert flat.sum() > (T - 1) * blocks // 4                        # most measuring blocks count


@pytest.mark.parametrize("fmt", [F8, F10], ids=["8bit", "10bit"])
def test_mv_histograms_are_safe_and_exact_for_arbitrary_int8_vectors(fmt):
    """The payloads lie in the middle of a larger allocation, 130 rows plus 130 samples of zeros on both sides: a kernel that forgot its bounds test
    would count blocks it must not count, and still stay inside allocated memory.  The test checks counts; it cannot provoke a fault."""
    rng = np.random.default_rng(11)
    for (H, W), T in (((37, 70), 3), ((64, 96), 2), ((18, 34), 4)):
        p = payloads(fmt, T, H, W, "texture", seed=5)
        src = on_device(p, slack=(130 * W + 130) * (1 if fmt.bits == 8 else 2))
        gy, gx = noise.motion_grid(H, W)
        mv = rng.integers(-128, 128, (T - 1, gy, gx, 2)).astype(np.int8)
        mv[0, 0, 0], mv[0, 0, -1], mv[-1, -1, 0], mv[-1, -1, -1] = (127, 127), (-128, 127), (127, -128), (-128, -128)
        mv[0, -1, 1], mv[0, 0, 1] = (0, 0), (-1, 1)
        lo, hi = -1, 1 << 16
        flat, bands = check_hists(src, p, torch.from_numpy(mv).cuda(), mv, fmt, H, W, lo, hi)
        inside = sum(len(M._pair_mv(p[k], p[k + 1], mv[k], fmt, H, W, lo, hi, None)[0]) for k in range(T - 1))
        assert int(flat.sum()) == inside and 0 < inside < (T - 1) * (H // 2) * (W // 2) // 2      # some blocks count, many do not
        small = rng.integers(-7, 8, mv.shape).astype(np.int8)                    # vectors of the matcher's range that the matcher would not have chosen
        check_hists(src, p, torch.from_numpy(small).cuda(), small, fmt, H, W, *N.clip_codes(fmt))


def test_the_three_entry_points_refuse_bad_arguments_and_an_empty_grid_writes_nothing():
    lib = L.load()
    f = yuv_fmt(8, L.SN_YUV_420_CENTER, 0, 0)
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    gm, mvt = guarded((64,), torch.int8)
    gs, sadt = guarded((32,), torch.uint32)
    dst = torch.zeros(2 * 16 * 512 + 8, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    src, mv, sad, d = buf.data_ptr(), mvt.data_ptr(), sadt.data_ptr(), dst.data_ptr()
    motion = lambda src_, f_, r_, mv_, T, H, W: lib.sn_yuv_block_motion(src_, f_, r_, mv_, sad, T, H, W, s)                 # noqa: E731
    hists = [lambda src_, f_, r_, mv_, T, H, W, call=getattr(lib, n): call(src_, f_, r_, mv_, d, 16, 235, T, H, W, s)       # noqa: E731
             for n in ("sn_yuv_noise_hist_pairs_mv", "sn_yuv_noise_hist_pairs_bands_mv")]
    for call in [motion] + hists:
        assert call(src, f, None, mv, 2, 1, 5) == 0 and call(src, f, None, mv, 2, 5, 1) == 0      # no whole block: legal
    torch.cuda.synchronize()
    assert guards_intact(gm, 64) and guards_intact(gs, 32)
    assert (mvt.cpu().numpy() == GARBAGE8).all() and (sadt.cpu().numpy() == GARBAGE).all()        # ... and the matcher wrote nothing at all
    mvt.zero_()
    for call in [motion] + hists:
        assert call(src, f, None, mv, 2, 8, 8) == 0
        assert call(src, f, L.YuvRect(2, 2, 4, 4), mv, 2, 8, 8) == 0
        for bad in (L.YuvRect(1, 2, 4, 4), L.YuvRect(2, 1, 4, 4), L.YuvRect(2, 2, 3, 4), L.YuvRect(2, 2, 8, 4), L.YuvRect(-2, 0, 4, 4), L.YuvRect(0, 0, 0, 4)):
            assert call(src, f, bad, mv, 2, 8, 8) == -22                         # 4:2:0: odd origin, odd w inside, outside the frame, empty
        assert call(src, yuv_fmt(8, 0, 0, 0), L.YuvRect(1, 3, 3, 5), mv, 2, 8, 8) == 0              # 4:4:4: any integers
        for bad in (yuv_fmt(9, 0, 0, 0), yuv_fmt(12, 0, 0, 0), yuv_fmt(8, 3, 0, 0)):
            assert call(src, bad, None, mv, 2, 8, 8) == -22
        for T, H, W in ((1, 8, 8), (0, 8, 8), (-1, 8, 8), (65537, 8, 8), (65536, 8, 8), (2, 0, 8), (2, 8, 0)):
            assert call(src, f, None, mv, T, H, W) == -22
        assert call(src + 1, yuv_fmt(10, 0, 0, 0), None, mv, 2, 8, 8) == -22                       # 16-bit samples at an odd address
        assert call(src + 1, f, None, mv, 2, 8, 8) == 0                                            # 8-bit samples may lie anywhere
        assert call(src, f, None, mv + 1, 2, 8, 8) == 0                                            # ... and so may the vectors
        assert call(None, f, None, mv, 2, 8, 8) == -22 and call(src, None, None, mv, 2, 8, 8) == -22 and call(src, f, None, None, 2, 8, 8) == -22
    assert lib.sn_yuv_block_motion(src, f, None, mv, None, 2, 8, 8, s) == -22                       # a null sad
    for k in (1, 2, 3):
        assert lib.sn_yuv_block_motion(src, f, None, mv, sad + k, 2, 8, 8, s) == -22               # sad is uint32
    for name in ("sn_yuv_noise_hist_pairs_mv", "sn_yuv_noise_hist_pairs_bands_mv"):
        call = getattr(lib, name)
        assert call(src, f, None, mv, None, 16, 235, 2, 8, 8, s) == -22                            # a null dst
        for k in (1, 2, 3):
            assert call(src, f, None, mv, d + k, 16, 235, 2, 8, 8, s) == -22                       # dst is uint32
        assert call(src, f, None, mv, d, 236, 235, 2, 8, 8, s) == -22                              # lo > hi
        assert call(src, f, None, mv, d, -(1 << 24) - 1, 235, 2, 8, 8, s) == -22 and call(src, f, None, mv, d, 16, (1 << 24) + 1, 2, 8, 8, s) == -22
        assert call(src, f, None, mv, d, 235, 235, 2, 8, 8, s) == 0                                # lo == hi: legal, nothing counts
        torch.cuda.synchronize()
        assert int(dst.abs().sum()) == 0                                                          # every legal call so far counted nothing (codes 0) ...
        assert call(src, f, None, mv, d, -1, 235, 3, 8, 8, s) == 0
        torch.cuda.synchronize()
        h = dst.cpu().numpy()
        words = 1021 if name == "sn_yuv_noise_hist_pairs_mv" else 16 * 128
        assert h[0] == 8 and h[words] == 8 and int(np.abs(h).sum()) == 16                          # ... with lo = -1: the 8 measuring blocks of 16, two pairs
        dst.zero_()
    torch.cuda.synchronize()
    assert guards_intact(gm, 64) and guards_intact(gs, 32)
    with pytest.raises(ValueError, match="two payloads"):
        block_motion_yuv(buf[:96].view(1, 96), f, 8, 8)
    with pytest.raises(ValueError, match="two payloads"):
        noise_hist_pairs_mv_yuv(buf[:96].view(1, 96), f, 8, 8, torch.zeros((0, 1, 1, 2), dtype=torch.int8, device="cuda"))


# ---- the restorer -----------------------------------------------------------------------------------------------------------------------------
FMT = S.FMT420
H, W, ONE_LEN, FRAMES = 71, 99, 5, 13                                                          # three windows: 5 + 5 + 3 frames
RECT = (8, 6, 64, 48)                                                                          # 4:2:0: even origin and size, inside 71 x 99
TIMING = lambda stats: {k: v for k, v in stats.items() if "_ms" not in k and k != "forward_s"}   # noqa: E731


@pytest.fixture(scope="module")
def net():
    return restore.load_net("denoise_small", "synthetic", "bf16")


@pytest.fixture(scope="module")
def clip():
    """The texture of the accuracy table moving 1 px per frame, sigma 10 injected on R'G'B'."""
    return list(N.noisy_payloads(NP.texture_clip(FRAMES, H, W, 1), 10.0, FMT, seed=3))


def run(net, pay, sigma="auto", h=H, w=W, **kw):
    vr = restore.VideoRestorer(net, ONE_LEN, sigma=sigma, **kw)
    out = list(vr.restore(iter(pay), yuv_fmt(*FMT), h, w))
    return out, vr.stats


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def by_blocks(net, clip):
    """The clip restored with the option: shared by the tests below and left unchanged."""
    return run(net, clip, sigma_estimator="min", sigma_motion="blocks")


def check_stats(stats, est, level=False):
    """Every stats entry of the option equals the host restatement exactly (floats compared with ==: the same integers through the same functions)."""
    n = len(est["sigma"])
    assert stats["sigma_motion"] == "blocks" and stats["sigma_estimator"] == "min" and stats["windows"] == n
    assert stats["window_pair_sigma"] == est["pair_sigma"] and stats["window_sigma_temporal"] == est["temporal"]
    assert stats["window_frame_sigma"] == est["frame_sigma"] and stats["window_sigma_spatial"] == est["spatial"]
    assert stats["window_sigma"] == est["sigma"]
    assert stats["window_pair_motion"] == est["pair_motion"]
    assert all(len(pm) == len(ps) == len(fs) - 1 for pm, ps, fs in zip(stats["window_pair_motion"], stats["window_pair_sigma"], stats["window_frame_sigma"]))
    assert stats["noise_launches"] == 2 * n and stats["noise_pairs_launches"] == n              # the spatial histogram and the matcher; the _mv histogram
    if level:
        assert stats["window_nlf"] == est["nlf"] and stats["nlf_launches"] == stats["nlf_pairs_launches"] == stats["nlf_map_launches"] == n


def test_blocks_stats_equal_the_host_restatement_and_the_bytes_of_the_listed_sigmas(net, clip, by_blocks):
    est = M.window_estimates(clip, FMT, H, W, ONE_LEN, "min")
    plain = NP.window_estimates(clip, FMT, H, W, ONE_LEN, "min")
    out, stats = by_blocks
    assert len(out) == FRAMES and stats["frames"] == FRAMES and len(est["sigma"]) == 3
    check_stats(stats, est)
    # the clip is what the option is for: the plain pair statistic reads the motion, the compensated one the noise, and "min" takes it
    assert all(t < 0.9 * q < q < s for t, q, s in zip(est["temporal"], plain["temporal"], est["spatial"])) and stats["window_sigma"] == est["temporal"]
    assert all(abs(t - 10.0) < 1.0 for t in est["temporal"])
    # the texture moves horizontally, and its period of 2 pi / 0.9 = 6.98 px makes -6 as good a vector as +1: the medians are not asserted beyond dy
    assert all(share > 0.5 and dy == 0.0 and dx != 0.0 for pm in stats["window_pair_motion"] for share, dy, dx in pm)
    listed, lstats = run(net, clip, sigma=list(stats["window_sigma"]))
    assert same(listed, out) and lstats["noise_launches"] == 0 and "sigma_motion" not in lstats
    without, wstats = run(net, clip, sigma_estimator="min")
    assert wstats["window_sigma"] == plain["sigma"] != stats["window_sigma"] and not same(without, out)      # the option does reach the network


def test_blocks_with_level_equals_the_host_restatement_and_the_bytes_of_the_listed_curves(net, clip):
    est = M.window_estimates(clip, FMT, H, W, ONE_LEN, "min", level=True)
    out, stats = run(net, clip, sigma_estimator="min", sigma_motion="blocks", noise_model="level")
    check_stats(stats, est, level=True)
    assert all(max(c) > 0.0 for c in stats["window_nlf"])
    assert stats["window_nlf"] != NP.window_estimates(clip, FMT, H, W, ONE_LEN, "min", level=True)["nlf"]      # the vectors do reach the curve
    listed, lstats = run(net, clip, sigma=10.0, noise_model=stats["window_nlf"])
    assert same(listed, out) and lstats["nlf_launches"] == 0 and "nlf_pairs_launches" not in lstats


def test_blocks_serial_a_fixed_picture_and_scene_cuts(net, clip, by_blocks):
    serial, sstats = run(net, clip, sigma_estimator="min", sigma_motion="blocks", pipeline=False)
    assert same(serial, by_blocks[0]) and TIMING(sstats) == TIMING(by_blocks[1])
    est = M.window_estimates(clip, FMT, H, W, ONE_LEN, "min", rect=RECT)                        # the matcher and the statistic see the window's rectangle
    out, stats = run(net, clip, sigma_estimator="min", sigma_motion="blocks", picture=RECT)
    check_stats(stats, est)
    assert est["pair_sigma"] != M.window_estimates(clip, FMT, H, W, ONE_LEN, "min")["pair_sigma"]
    crop = list(P.crop_payloads(np.stack(clip), FMT, H, W, RECT))                              # ... which are the cropped stream's numbers
    cstats = run(net, crop, h=RECT[3], w=RECT[2], sigma_estimator="min", sigma_motion="blocks")[1]
    for k in ("window_pair_sigma", "window_pair_motion", "window_sigma_temporal", "window_sigma_spatial", "window_sigma", "window_frame_sigma"):
        assert cstats[k] == stats[k], k
    cuts = [7]                                                                                  # scenes of 7 and 6 frames: windows of 5 + 2 and 5 + 1
    est = M.window_estimates(clip, FMT, H, W, ONE_LEN, "min", cuts=cuts)
    out, stats = run(net, clip, sigma_estimator="min", sigma_motion="blocks", scene_cuts=cuts)
    check_stats(stats, est)
    assert len(out) == FRAMES and len(est["sigma"]) == 4


def test_without_the_option_everything_is_todays(net, clip):
    ref, rstats = run(net, clip, sigma_estimator="min")
    out, stats = run(net, clip, sigma_estimator="min", sigma_motion=None)
    assert same(out, ref) and list(stats) == list(rstats) and TIMING(stats) == TIMING(rstats)
    assert stats["noise_launches"] == stats["noise_pairs_launches"] == 3 and "sigma_motion" not in stats and "window_pair_motion" not in stats
    vr = restore.VideoRestorer(net, ONE_LEN, sigma="auto", sigma_estimator="min")
    list(vr.restore(iter(clip[:6]), yuv_fmt(*FMT), H, W))
    assert vr.run.launches["motion"] == 0 and all(s.noise.vectors is None for s in vr.slots)      # today's slots
    vr = restore.VideoRestorer(net, ONE_LEN, sigma="auto", sigma_estimator="min", sigma_motion="blocks")
    list(vr.restore(iter(clip[:6]), yuv_fmt(*FMT), H, W))
    gy, gx = noise.motion_grid(H, W)
    assert vr.run.launches["motion"] == 2 and all(s.noise.vectors.mv.numel() == 8 * gy * gx * 2 and s.noise.vectors.sad.numel() == 8 * gy * gx for s in vr.slots)


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def test_restore_video_cli_with_sigma_motion_blocks_in_a_child_process_gives_the_api_bytes(tmp_path, clip, by_blocks):
    hd = y4m.Y4MHeader(width=W, height=H, fps="24:1", aspect="1:1", chroma="420jpeg", extensions=["COLORRANGE=LIMITED"])
    src, dst, sig = tmp_path / "in.y4m", tmp_path / "out.y4m", tmp_path / "sigma.txt"
    with open(src, "wb") as fh:
        wr = y4m.Y4MWriter(fh, hd)
        for p in clip:
            wr.write(p)
    cmd = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "denoise_small", "--checkpoint", "synthetic",
           "--dtype", "bf16", "--one_len", str(ONE_LEN), "--sigma", "auto", "--sigma_estimator", "min", "--sigma_motion", "blocks",
           "--sigma_out", str(sig), str(src), str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)                      # a fresh child process
    assert r.returncode == 0, r.stderr[-2000:]
    assert "done: 13 frames" in r.stderr and "sigma (auto, min, motion blocks" in r.stderr
    assert noise.parse_sigmas(sig.read_text()) == by_blocks[1]["window_sigma"]                 # 71 < 720: the CLI's default matrix is BT.601, as FMT
    with open(dst, "rb") as fh:
        assert same(list(y4m.Y4MReader(fh)), by_blocks[0])
