"""CPU tests of the output format of the video restorer: the dither's hash and what it does to the rounding (tests/dither_ref.py), and the
planning of a stream written in another format than it was read (shiftnet_amd/restore.py, y4m.py, picture.py).  No GPU."""
import os
import re

import numpy as np
import pytest

import dither_ref as D
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import picture, restore, y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 12345)
FMT444 = R.Fmt(8, R.C444, R.BT601, R.LIMITED)


def corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


# ---- the hash -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_the_hash_is_triangular_noise_of_one_code_white_in_space_time_plane_and_seed(seed):
    n = 1024                                                   # 2^20 samples: sigma of a mean sqrt(1/6 / 2^20) = 4e-4, of a correlation 2^-10
    a = D.d(seed, 0, 0, n, n)
    assert a.dtype == np.float32 and a.shape == (n, n)
    assert float(np.abs(a).max()) < 1.0
    assert np.array_equal(a * np.float32(4096), np.rint(a * np.float32(4096)))                # multiples of 1/4096: exact in float32
    mean, var = float(a.astype(np.float64).mean()), float(a.astype(np.float64).var())
    print(f"seed {seed}: mean {mean:.2e} variance {var:.5f}")
    assert abs(mean) <= 2e-3                                   # 5 sigma
    assert abs(var - 1.0 / 6.0) <= 1e-3
    pairs = {}
    for lag in (1, 2):
        pairs[f"x{lag}"] = (a[:, lag:], a[:, :-lag])
        pairs[f"y{lag}"] = (a[lag:], a[:-lag])
        pairs[f"diag{lag}"] = (a[lag:, lag:], a[:-lag, :-lag])
        pairs[f"anti{lag}"] = (a[lag:, :-lag], a[:-lag, lag:])
    pairs["next frame"] = (a, D.d(seed, 1, 0, n, n))
    pairs["Cb"] = (a, D.d(seed, 0, 1, n, n))
    pairs["Cr"] = (a, D.d(seed, 0, 2, n, n))
    pairs["Cb Cr"] = (D.d(seed, 0, 1, n, n), D.d(seed, 0, 2, n, n))
    pairs["next seed"] = (a, D.d(seed + 1, 0, 0, n, n))
    for name, (p, q) in pairs.items():
        c = corr(p, q)
        print(f"seed {seed}: correlation {name} {c:+.2e}")
        assert abs(c) <= 5e-3, (name, c)                       # 5 sigma


def test_the_hash_wraps_as_uint32_and_its_histogram_is_a_triangle():
    # a python-int restatement of one sample, with every product reduced mod 2^32
    def one(seed, f, p, y, x):
        m = 0xFFFFFFFF
        k = ((y * 0x9E3779B1) & m) ^ ((x * 0x85EBCA77) & m) ^ ((f * 0xC2B2AE3D) & m) ^ ((p * 0x27D4EB2F) & m) ^ seed
        k ^= k >> 16
        k = (k * 0x85EBCA6B) & m
        k ^= k >> 13
        k = (k * 0xC2B2AE35) & m
        k ^= k >> 16
        return ((k & 0xFFF) + ((k >> 12) & 0xFFF) - 4095) / 4096
    for seed, f, p, y, x in [(0, 0, 0, 0, 0), (0xDEADBEEF, 7, 2, 1079, 1919), (12345, 2 ** 31 - 1, 1, 65535, 2), (7, 2 ** 31 - 1, 2, 1, 65535), (2 ** 32 - 1, 5, 0, 3, 2)]:
        assert float(D.d(seed, f, p, y + 1, x + 1)[y, x]) == one(seed, f, p, y, x)
    a = D.d(3, 0, 0, 1024, 1024).astype(np.float64)
    h, _ = np.histogram(a, bins=8, range=(-1, 1))
    tri = np.array([1, 3, 5, 7, 7, 5, 3, 1]) / 32 * a.size     # the triangle's mass per eighth
    assert np.abs(h - tri).max() <= 5 * np.sqrt(tri.max())


# ---- the reference egress ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [R.Fmt(b, c, m, r) for b, c in ((8, 0), (8, 1), (8, 2), (10, 0), (10, 2)) for m, r in ((0, 0), (1, 1))])
def test_with_the_dither_term_at_zero_the_reference_is_the_undithered_restatement(fmt):
    rng = np.random.default_rng(5)
    for H, W, Hp, Wp in [(1, 1, 4, 4), (35, 67, 40, 72), (16, 64, 16, 64)]:
        x = (rng.random((3, 3, Hp, Wp)) * 1.4 - 0.2).astype(np.float32)
        assert np.array_equal(D.egress(x, fmt, H, W, 9, 5, noise=D.zero), R.egress_emu(x, fmt, H, W))
        assert not np.array_equal(D.egress(x, fmt, H, W, 9, 5), R.egress_emu(x, fmt, H, W)) or H == 1
        two = np.concatenate([D.egress(x[:1], fmt, H, W, 9, 5), D.egress(x[1:], fmt, H, W, 9, 6)])
        assert np.array_equal(D.egress(x, fmt, H, W, 9, 5), two)                               # frame t of a launch at t0 is frame number t0 + t


def flat_luma(raw_code, H, W):
    """[1,3,H,W] float32 grey whose limited-range 8-bit luma is raw_code (not rounded), and the float32 value the egress computes for it."""
    v = np.full((1, 3, H, W), (np.asarray(raw_code, np.float64) - 16.0) / 219.0).astype(np.float32)
    raw = R.rgb_to_yuv444_emu(v[0], FMT444)[0][0]
    return v, raw.astype(np.float64)


@pytest.mark.parametrize("frac", [0.0, 0.25, 0.5, 0.73])
def test_dither_makes_the_mean_code_of_a_flat_area_follow_its_value(frac):
    H = W = 64
    x, raw = flat_luma(np.full((H, W), 100.0 + frac), H, W)
    assert abs(float(raw.mean()) - (100.0 + frac)) < 1e-4
    plain = R.split_planes(R.egress_emu(x, FMT444, H, W)[0], FMT444, H, W)[0]
    assert len(np.unique(plain)) == 1
    off = abs(float(plain.mean()) - float(raw.mean()))
    assert abs(off - min(frac, 1.0 - frac)) < 1e-4             # without dither the mean is off by the fraction (0.5 rounds to even)
    for seed in SEEDS:
        for f in (0, 3):
            y = R.split_planes(D.egress(x, FMT444, H, W, seed, f)[0], FMT444, H, W)[0]
            err = float(y.mean()) - float(raw.mean())
            print(f"frac {frac} seed {seed} frame {f}: mean code {y.mean():.4f}, error {err:+.4f}")
            assert abs(err) <= 0.04                            # 5 x 0.5 / 64: the total error of TPDF dither has variance 1/4 whatever the value
            assert set(np.unique(y)) <= {99, 100, 101, 102}


def test_a_ramp_between_two_codes_is_one_step_without_dither_and_a_ramp_with_it():
    H, W = 256, 256
    x, raw = flat_luma(np.broadcast_to(100.0 + (np.arange(W) + 0.5) / W, (H, W)), H, W)          # 256 columns spanning code 100 .. 101
    plain = R.split_planes(R.egress_emu(x, FMT444, H, W)[0], FMT444, H, W)[0]
    cols = plain.mean(axis=0)
    assert set(np.unique(plain)) == {100, 101} and int(np.count_nonzero(np.diff(cols))) == 1      # a single step: the band edge
    assert np.abs(cols - raw.mean(axis=0)).max() >= 0.49
    for seed in SEEDS:
        y = R.split_planes(D.egress(x, FMT444, H, W, seed, 0)[0], FMT444, H, W)[0]
        err = y.mean(axis=0) - raw.mean(axis=0)
        print(f"seed {seed}: column means off by at most {np.abs(err).max():.4f}, rms {np.sqrt((err ** 2).mean()):.4f}; per-sample rms "
              f"{np.sqrt(((y - raw) ** 2).mean()):.4f}")
        assert np.abs(err).max() <= 5 * 0.5 / np.sqrt(H)       # every column mean within 5 sigma of the ramp
        assert abs(np.sqrt(((y - raw) ** 2).mean()) - 0.5) <= 0.01                             # the price: noise of 0.5 code rms


# ---- planning the output ------------------------------------------------------------------------------------------------------------------------
def test_the_output_header_carries_the_new_c_tag_and_everything_else_of_the_input():
    for tin in y4m.MODES:
        hd = y4m.parse_header(f"YUV4MPEG2 W70 H37 F30000:1001 Ip A4:3 C{tin} XYSCSS={tin.upper()} XCOLORRANGE=FULL".encode())
        assert y4m.output_header(hd, None) is hd
        for tout in y4m.MODES:
            out = y4m.output_header(hd, tout)
            assert out.line() == f"YUV4MPEG2 W70 H37 F30000:1001 Ip A4:3 C{tout} XYSCSS={tin.upper()} XCOLORRANGE=FULL\n".encode()
            assert hd.chroma == tin                            # the input's header is not touched
            bits, chroma = y4m.MODES[tout]
            assert out.frame_bytes == R.frame_bytes(R.Fmt(bits, chroma, 0, 0), 37, 70)
            ofmt, dither, seed = restore.plan_output(L.YuvFmt(hd.bits, hd.chroma_code, L.SN_YUV_BT709, L.SN_YUV_FULL), tout, "tpdf", 7)
            assert (ofmt.bits, ofmt.chroma, ofmt.matrix, ofmt.range) == (bits, chroma, L.SN_YUV_BT709, L.SN_YUV_FULL)      # matrix and range: the input's
            assert ofmt.frame_bytes(37, 70) == out.frame_bytes and (dither, seed) == ("tpdf", 7)
    with pytest.raises(y4m.Y4MError, match="C422"):
        y4m.output_header(hd, "422")


def test_the_inputs_own_format_is_todays_path_and_bad_arguments_are_refused():
    fmt = L.YuvFmt(8, L.SN_YUV_420_LEFT, 0, 0)
    assert restore.plan_output(fmt) == (fmt, None, 0)
    for same in ("420mpeg2", "420", "420paldv"):               # three tags, one layout
        assert restore.plan_output(fmt, same)[0] is fmt
    assert restore.plan_output(fmt, "420jpeg")[0] is not fmt
    assert restore.plan_output(R.Fmt(8, 1, 1, 0), "444p10")[0] == R.Fmt(10, 0, 1, 0)
    assert restore.plan_output(fmt, None, None, 2 ** 32 - 1)[2] == 2 ** 32 - 1
    for bad in ("422", "C444", "", 444):
        with pytest.raises(ValueError, match="out_format"):
            restore.plan_output(fmt, bad)
    for bad in ("none", "floyd", "TPDF", True):
        with pytest.raises(ValueError, match="dither"):
            restore.plan_output(fmt, None, bad)
    for bad in (-1, 2 ** 32, 1.5, "3"):
        with pytest.raises(ValueError, match="dither_seed"):
            restore.plan_output(fmt, None, "tpdf", bad)
    ap = restore.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["in", "out"])
    assert (a.out_format, a.dither, a.dither_seed) == (None, "none", 0)
    a = ap.parse_args(base + ["--out_format", "444p10", "--dither", "tpdf", "--dither_seed", "3", "in", "out"])
    assert (a.out_format, a.dither, a.dither_seed) == ("444p10", "tpdf", 3)
    for bad in (["--out_format", "422"], ["--dither", "floyd"], ["--dither_seed", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + bad + ["in", "out"])


def test_a_rectangle_must_be_legal_in_the_format_read_and_in_the_format_written():
    f444, f420 = R.Fmt(8, R.C444, 0, 0), R.Fmt(10, R.C420_LEFT, 0, 0)
    H, W = 37, 70
    odd = (1, 3, 39, 21)
    assert picture.check_rect(odd, f444, H, W) == odd
    assert picture.check_rect(odd, f444, H, W, out_fmt=f444) == odd
    for fin, fout in ((f444, f420), (f420, f444), (f420, f420)):
        for bad, word in [((1, 4, 40, 22), "even"), ((2, 3, 40, 22), "even"), ((2, 4, 39, 22), "odd w"), ((2, 4, 40, 21), "odd h")]:
            with pytest.raises(ValueError, match=word):
                picture.check_rect(bad, fin, H, W, out_fmt=fout)
        assert picture.check_rect((8, 0, 62, 37), fin, H, W, out_fmt=fout) == (8, 0, 62, 37)    # odd w and h that reach the far edges
        assert picture.check_pictures([None, (2, 4, 40, 22)], fin, H, W, 5, out_fmt=fout) == [None, (2, 4, 40, 22)]
        with pytest.raises(ValueError, match="even"):
            picture.check_pictures([None, odd], fin, H, W, 5, out_fmt=fout)


def test_decide_picture_aligns_to_even_when_only_the_output_is_420():
    H, W, T = 40, 64, 2
    f444, f420 = R.Fmt(8, R.C444, 0, 0), R.Fmt(8, R.C420_CENTER, 0, 0)
    Y = np.full((T, H, W), 16, np.int64)
    Y[:, 3:34, 5:58] = 120                                     # bars: 3 rows on top, 6 below, 5 columns left, 6 right
    rows, cols = Y.sum(axis=2), Y.sum(axis=1)
    assert picture.decide_picture(rows, cols, f444, H, W) == (5, 3, 53, 31)
    assert picture.decide_picture(rows, cols, f444, H, W, out_fmt=f444) == (5, 3, 53, 31)
    want = (6, 4, 52, 30)                                      # near edges up to even, far edges down to even
    assert picture.decide_picture(rows, cols, f444, H, W, out_fmt=f420) == want
    assert picture.decide_picture(rows, cols, f420, H, W, out_fmt=f444) == want
    assert picture.decide_picture(rows, cols, f420, H, W) == want
    assert picture.check_rect(want, f444, H, W, out_fmt=f420) == want


def test_windows_know_the_number_of_their_first_frame_in_their_clip():
    from shiftnet_amd.scenes import ListedCuts
    frames = [np.full(4, i, np.uint8) for i in range(12)]
    src = restore._Frames(iter(frames))
    got = []
    for k in range(4):
        win = src.window(k, 4)
        got.append(None if win is None else (win[0], src.clip_lo))
    assert got == [(0, 0), (4, 4), (8, 8), None]
    src = restore._SceneFrames(iter(frames), ListedCuts([5]))
    got, k = [], 0
    while True:
        win = src.window(k, 4)
        if win is None:
            break
        got.append((win[0], win[1], src.clip_lo))
        k += 1
    assert got == [(0, 4, 0), (4, 1, 4), (5, 4, 0), (9, 3, 4)]   # the scene that starts at 5 counts from 0 again


def test_the_symbol_and_its_formula_are_declared():
    assert "sn_egress_yuv_dither" in L.SYMBOLS and (L.SN_DITHER_NONE, L.SN_DITHER_TPDF) == (0, 1)
    with open(os.path.join(ROOT, "include", "shiftnet_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define SN_ABI_VERSION 20\b", header)
    assert "typedef struct sn_yuv_dither { int mode; uint32_t seed; int t0; } sn_yuv_dither;" in header
    for const in ("0x9E3779B1", "0x85EBCA77", "0xC2B2AE3D", "0x27D4EB2F", "0x85EBCA6B", "0xC2B2AE35"):
        assert const in header
    import ctypes
    assert ctypes.sizeof(L.YuvDither) == 12
