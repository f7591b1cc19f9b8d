"""CPU tests of the grain put back (shiftnet_amd/grain.py, ``--grain``): the option's grammar and refusals, the taps, the new symbol and struct, the
refusals of the C entry point, the statistics of the field as numpy restates it (tests/grain_ref.py), and the closed loop: the project's own noise
estimator reads the level that was put on a flat plane.

Bounds.  A prototype of exactly this arithmetic read, on 180 x 320 x 8 frames at sizes 0 / 0.5 / 0.8 / 1.2: a field standard deviation of 0.986 ..
1.009, lag-1 correlations within 0.007 of rho_1 = 2 w0 w1 + 2 w1 w2, |mean| <= 0.03; asserted are 3 %, 0.015 and 0.05, roughly twice that, for another
seed.  The closed loop read 2.02 .. 2.03, 5.04, 10.07 .. 10.13, 25.16 .. 25.23 for white grain of 2, 5, 10, 25, and (1 - rho_1) G within 0.6 % at size
0.8: asserted is 3 %, the estimator's own margin for injected noise (noise_ref.margin)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import grain_ref as GR
import noise_ref as N
import yuv_ref as R
from shiftnet_amd import grain, noise, restore_cli, y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0.0, 0.5, 0.8, 1.2)
RHO1 = (0.0, 0.2612, 0.6717, 0.8317)


def test_parse_grain_and_the_restorers_form():
    assert grain.parse_grain("4") == [4.0] * 16 and grain.parse_grain(" 2.5 ") == [2.5] * 16 and grain.parse_grain("0") == [0.0] * 16
    curve = [float(i) / 2 for i in range(16)]
    assert grain.parse_grain(",".join(repr(v) for v in curve)) == curve
    assert grain.parse_grain("auto") == ("auto", 0.5) and grain.parse_grain("auto:0.25") == ("auto", 0.25)
    assert grain.parse_grain("auto:0") == ("auto", 0.0) and grain.parse_grain("auto:4") == ("auto", 4.0)
    for bad in ("", "much", "-1", "nan", "inf", "1,2", ",".join(["1"] * 15), ",".join(["1"] * 17), ",".join(["1"] * 15 + ["-0.5"]), "1;2",
                "auto:", "auto:-0.1", "auto:4.5", "auto:nan", "auto:half", "automatic", "auto,auto"):
        with pytest.raises(ValueError):
            grain.parse_grain(bad)
    assert grain.grain_form(None) == (None, None, 0.0, 0.0, 0)
    assert grain.grain_form(4.0) == ("knots", [4.0] * 16, 0.0, 0.0, 0) and grain.grain_form(4, 0.8, 0.5, 7) == ("knots", [4.0] * 16, 0.8, 0.5, 7)
    assert grain.grain_form(curve, 1.2, 0.0, 2 ** 32 - 1) == ("knots", curve, 1.2, 0.0, 2 ** 32 - 1)
    assert grain.grain_form("auto") == ("auto", 0.5, 0.0, 0.0, 0) and grain.grain_form("auto:1.5", 0.5) == ("auto", 1.5, 0.5, 0.0, 0)
    assert grain.grain_form(("auto", 0.25)) == ("auto", 0.25, 0.0, 0.0, 0) and grain.grain_form("3") == ("knots", [3.0] * 16, 0.0, 0.0, 0)
    for bad in (-1.0, float("nan"), [1.0] * 15, True, [1.0] * 15 + [float("inf")], "auto:5", "much", ("auto", -1.0), ("auto", True)):
        with pytest.raises(ValueError, match="grain"):
            grain.grain_form(bad)
    for kw, name in ((dict(grain_size=-0.1), "grain_size"), (dict(grain_size=1.3), "grain_size"), (dict(grain_size=float("nan")), "grain_size"),
                     (dict(grain_size="0.5"), "grain_size"), (dict(grain_chroma=-1.0), "grain_chroma"), (dict(grain_chroma=float("inf")), "grain_chroma"),
                     (dict(grain_seed=-1), "grain_seed"), (dict(grain_seed=2 ** 32), "grain_seed"), (dict(grain_seed=0.5), "grain_seed")):
        with pytest.raises(ValueError, match=name):
            grain.grain_form(4.0, **kw)
    for kw in (dict(grain_size=0.8), dict(grain_chroma=0.5), dict(grain_seed=3)):
        with pytest.raises(ValueError, match=r"grain_size / grain_chroma / grain_seed.*need grain"):
            grain.grain_form(None, **kw)


@pytest.mark.parametrize("size, rho", list(zip(SIZES, RHO1)))
def test_the_taps_have_unit_energy_and_the_stated_neighbour_correlation(size, rho):
    w0, w1, w2 = grain.grain_taps(size)
    assert all(float(np.float32(w)) == w for w in (w0, w1, w2))                      # float32 values
    assert abs(w0 * w0 + 2 * w1 * w1 + 2 * w2 * w2 - 1.0) <= 1e-6
    assert abs(grain.lag1((w0, w1, w2)) - rho) <= 5e-5 and w0 > w1 >= w2 >= 0.0
    if size == 0.0:
        assert (w0, w1, w2) == (1.0, 0.0, 0.0)
    else:                                                                          # the formula, stated on its own
        e = [math.exp(-k * k / (2 * size * size)) for k in (-2, -1, 0, 1, 2)]
        norm = math.sqrt(sum(math.exp(-k * k / (size * size)) for k in (-2, -1, 0, 1, 2)))
        assert [w2, w1, w0] == [float(np.float32(v / norm)) for v in e[:3]]


def test_the_taps_and_the_knots_refuse_what_they_cannot_take():
    for bad in (-0.1, 1.21, float("nan"), float("inf"), "0.8", True):
        with pytest.raises(ValueError, match="size"):
            grain.grain_taps(bad)
    f = R.Fmt(10, R.C420_LEFT, R.BT601, R.LIMITED)
    k = grain.luma_knots([float(i) for i in range(16)], f)
    g = noise.luma_gain(R.BT601) * noise.code_scale(10, R.LIMITED)
    assert k == [float(np.float32(i * g)) for i in range(16)] and abs(g - math.sqrt(0.299 ** 2 + 0.587 ** 2 + 0.114 ** 2) * 876 / 255) < 1e-12
    for bad in ([1.0] * 15, [1.0] * 15 + [-1.0], [1.0] * 15 + [float("nan")]):
        with pytest.raises(ValueError):
            grain.luma_knots(bad, f)


def corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(np.mean(a * b) / math.sqrt(np.mean(a * a) * np.mean(b * b)))


@pytest.mark.parametrize("size, rho", list(zip(SIZES, RHO1)))
def test_the_field_has_unit_variance_and_the_filters_neighbour_correlation(size, rho):
    taps = grain.grain_taps(size)
    c = np.stack([GR.field(20240, f, 6, 180, 320, taps) for f in range(8)])
    assert c.dtype == np.float32 and c.shape == (8, 180, 320)
    c64 = c.astype(np.float64)
    mean, sd = float(c64.mean()), float(c64.std())
    rx, ry = corr(c[..., :-1], c[..., 1:]), corr(c[:, :-1], c[:, 1:])
    rt, rp = corr(c[:-1], c[1:]), corr(c, np.stack([GR.field(20240, f, 7, 180, 320, taps) for f in range(8)]))
    print(f"size {size}: mean {mean:+.4f}, sd {sd:.4f}, rho_x {rx:.4f}, rho_y {ry:.4f} (rho_1 {rho}), next frame {rt:+.4f}, next plane {rp:+.4f}")
    assert abs(mean) <= 0.05 and abs(sd - 1.0) <= 0.03
    assert abs(rx - rho) <= 0.015 and abs(ry - rho) <= 0.015
    # frames and planes are independent: two independent fields of N samples whose own correlations are rho(k) correlate with a standard deviation of
    # sqrt(sum_k rho(k)^2 / N), at most sqrt(8.4 / 460800) = 0.0043 here (size 1.2); the bound is that of the mean, ten of those
    assert abs(rt) <= 0.05 and abs(rp) <= 0.05
    # a pure function of the place: a window of the field is the field of that window; white grain is the hash's own samples
    part = GR._fir(GR._fir(GR.white_field(20240, 3, 6, np.arange(40 - 2, 60 + 2), np.arange(100 - 2, 130 + 2)), 1, taps), 0, taps)
    assert np.array_equal(part, GR.field(20240, 3, 6, 180, 320, taps)[40:60, 100:130])
    if size == 0.0:
        assert np.array_equal(c[3], GR.white_field(20240, 3, 6, np.arange(180), np.arange(320)))


LOOP_FORMATS = [R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED), R.Fmt(10, R.C420_LEFT, R.BT601, R.LIMITED), R.Fmt(8, R.C444, R.BT601, R.FULL)]


def flat_payloads(fmt, h=180, w=320, t=8):
    c = R.constants(fmt)
    ch, cw = R.chroma_shape(fmt, h, w)
    one = R.join_planes(np.full((h, w), (c["ylo"] + c["yhi"]) // 2), np.full((ch, cw), 128 << (fmt.bits - 8)), np.full((ch, cw), 128 << (fmt.bits - 8)), fmt)
    return np.stack([one] * t)


def read_back(p, fmt, h=180, w=320):
    lo, hi = N.clip_codes(fmt)
    return float(np.median([noise.frame_sigma(hh, fmt.bits, fmt.matrix, fmt.range) for hh in N.hist_ref(p, fmt, h, w, lo, hi)]))


@pytest.mark.parametrize("fmt", LOOP_FORMATS, ids=lambda f: "%d-%d-%d-%d" % f)
def test_the_estimator_reads_the_level_that_was_put_on_a_flat_plane(fmt):
    flat = flat_payloads(fmt)
    assert np.array_equal(GR.grain_ref(flat, fmt, 180, 320, [0.0] * 16, grain.grain_taps(0.8), 0.5, 3, 0), flat)      # level 0: the input bytes
    sized = grain.grain_taps(0.8)
    for G in (2.0, 5.0, 10.0, 25.0):
        est = read_back(GR.grain_ref(flat, fmt, 180, 320, [G] * 16, grain.grain_taps(0.0), 0.0, 11, 0), fmt)
        print(f"{fmt}: white grain of {G:g} reads {est:.3f}")
        assert abs(est - G) <= 0.03 * G
        if G >= 5.0:
            want = (1.0 - grain.lag1(sized)) * G
            est = read_back(GR.grain_ref(flat, fmt, 180, 320, [G] * 16, sized, 0.0, 11, 0), fmt)
            print(f"{fmt}: grain of {G:g} at size 0.8 reads {est:.3f}, (1 - rho_1) G = {want:.3f}")
            assert abs(est - want) <= 0.03 * want


def test_level_zero_and_chroma_zero_leave_what_they_should():
    fmt, h, w = R.Fmt(8, R.C420_LEFT, R.BT709, R.LIMITED), 37, 53
    n = R.frame_bytes(fmt, h, w)
    src = np.random.default_rng(5).integers(0, 256, (2, n)).astype(np.uint8)      # illegal codes included
    taps = grain.grain_taps(0.8)
    assert np.array_equal(GR.grain_ref(src, fmt, h, w, [0.0] * 16, taps, 0.5, 1, 0), src)
    got = GR.grain_ref(src, fmt, h, w, GR.BUMPY, taps, 0.0, 1, 0)
    assert np.array_equal(got[:, h * w:], src[:, h * w:]) and not np.array_equal(got[:, :h * w], src[:, :h * w])
    both = GR.grain_ref(src, fmt, h, w, GR.BUMPY, taps, 0.5, 1, 0)
    assert np.array_equal(both[:, :h * w], got[:, :h * w]) and not np.array_equal(both[:, h * w:], src[:, h * w:])
    # a legal code never leaves the legal range, an illegal one never moves further out
    Y, Yn = src[:, :h * w].astype(int), both[:, :h * w].astype(int)
    assert np.all(Yn >= np.minimum(Y, 16)) and np.all(Yn <= np.maximum(Y, 235))
    # a rectangle is the cropped stream, and nothing outside it moves
    rect = (10, 6, 30, 20)
    boxed = GR.grain_ref(src, fmt, h, w, GR.BUMPY, taps, 0.5, 1, 4, rect=rect)
    for t in range(2):
        Y0, U0, V0 = R.split_planes(src[t], fmt, h, w)
        crop = R.join_planes(Y0[6:26, 10:40], U0[3:13, 5:20], V0[3:13, 5:20], fmt)
        want = R.split_planes(GR.grain_ref(crop[None], fmt, 20, 30, GR.BUMPY, taps, 0.5, 1, 4 + t)[0], fmt, 20, 30)
        Yb, Ub, Vb = R.split_planes(boxed[t], fmt, h, w)
        assert np.array_equal(Yb[6:26, 10:40], want[0]) and np.array_equal(Ub[3:13, 5:20], want[1]) and np.array_equal(Vb[3:13, 5:20], want[2])
        Yb[6:26, 10:40], Ub[3:13, 5:20], Vb[3:13, 5:20] = Y0[6:26, 10:40], U0[3:13, 5:20], V0[3:13, 5:20]
        assert np.array_equal(R.join_planes(Yb, Ub, Vb, fmt), src[t])


def _write(path, header, payloads):
    with open(path, "wb") as fh:
        wr = y4m.Y4MWriter(fh, header)
        for p in payloads:
            wr.write(p)


def test_the_command_line_takes_the_options_and_refuses_what_does_not_go_together(capsys):
    ap = restore_cli.make_parser()
    base = ["--variant", "denoise_small", "--checkpoint", "synthetic", "--sigma", "auto"]
    a = ap.parse_args(base + ["in.y4m", "out.y4m"])
    assert a.grain is None and a.grain_size == 0.0 and a.grain_chroma == 0.0 and a.grain_seed == 0 and a.grain_out is None
    a = ap.parse_args(base + ["--grain", "4", "--grain_size", "0.8", "--grain_chroma", "0.5", "--grain_seed", "7", "--grain_out", "g.txt", "in.y4m", "out.y4m"])
    assert a.grain == [4.0] * 16 and (a.grain_size, a.grain_chroma, a.grain_seed, a.grain_out) == (0.8, 0.5, 7, "g.txt")
    assert ap.parse_args(base + ["--grain", "auto:0.25", "in.y4m", "out.y4m"]).grain == ("auto", 0.25)
    assert ap.parse_args(base + ["--grain", ",".join(str(i) for i in range(16)), "in.y4m", "out.y4m"]).grain == [float(i) for i in range(16)]
    for bad in ("-3", "1,2,3", "much", "auto:9"):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(base + ["--grain", bad, "in.y4m", "out.y4m"])
        assert e.value.code == 2 and "--grain" in capsys.readouterr().err
    # judged before any file is opened: the files named here do not exist
    gone = ["/nonexistent/in.y4m", "/nonexistent/out.y4m"]
    for more, words in ((["--grain_size", "0.8"], ["need grain"]), (["--grain_chroma", "0.5"], ["need grain"]), (["--grain_seed", "3"], ["need grain"]),
                        (["--grain_out", "/nonexistent/g.txt"], ["--grain_out needs --grain"]),
                        (["--grain", "4", "--grain_size", "1.5"], ["--grain_size", "grain_size"]),
                        (["--grain", "4", "--grain_chroma", "-1"], ["grain_chroma"]),
                        (["--grain", "4", "--grain_seed", str(2 ** 32)], ["grain_seed"]),
                        (["--grain", "4", "--view", "removed"], ["--grain", "--view removed"])):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(base + more + gone)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (more, err)
    with pytest.raises(SystemExit) as e:
        restore_cli.main(["--variant", "deblur_small", "--checkpoint", "synthetic", "--grain", "auto"] + gone)
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--grain auto" in err and "denoise" in err


def test_header_build_list_and_library_have_the_new_symbol_and_the_entry_point_refuses_on_the_host():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_grain.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_grain.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    from shiftnet_amd.io_edges import yuv_fmt
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^typedef struct sn_yuv_grain_noise \{ uint32_t seed; int t0; float knots\[16\]; float chroma; float taps\[3\]; \} sn_yuv_grain_noise;",
                     header, flags=re.M)
    assert re.search(r"^int sn_yuv_grain\(const uint8_t\* src, const sn_yuv_fmt\* fmt, const sn_yuv_rect\* rect /\* or NULL \*/, const sn_yuv_grain_noise\* grain,\s+"
                     r"const float\* gauss /\* device, 65536 \*/, uint8_t\* dst, int T, int H, int W, void\* stream\);", header, flags=re.M)
    assert hasattr(lib, "sn_yuv_grain") and "sn_yuv_grain" in L.SYMBOLS
    vp, ci = C.c_void_p, C.c_int
    assert lib.sn_yuv_grain.argtypes == [vp, C.POINTER(L.YuvFmt), C.POINTER(L.YuvRect), C.POINTER(L.YuvGrainNoise), vp, vp, ci, ci, ci, vp]
    assert lib.sn_yuv_grain.restype is ci
    assert C.sizeof(L.YuvGrainNoise) == 88 and [f[0] for f in L.YuvGrainNoise._fields_] == ["seed", "t0", "knots", "chroma", "taps"]
    assert L.YuvGrainNoise.knots.offset == 8 and L.YuvGrainNoise.chroma.offset == 72 and L.YuvGrainNoise.taps.offset == 76
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    # the argument checks are host side and need no GPU: host memory is refused before anything would read it
    arr = np.zeros(1 << 20, np.uint8)
    buf = arr.ctypes.data + (-arr.ctypes.data) % 16
    src, dst, gauss = buf, buf + (1 << 18), buf + (1 << 19)                  # 40 x 72 x 3 samples x 2 bytes x 2 frames < 2^18
    f8, f10 = yuv_fmt(8, L.SN_YUV_444, L.SN_YUV_BT709, L.SN_YUV_LIMITED), yuv_fmt(10, L.SN_YUV_420_LEFT, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    w = grain.grain_taps(0.8)

    def gr(t0=0, chroma=0.5, taps=w, **knots):
        k = [10.0] * 16
        for i, v in knots.items():
            k[int(i[1:])] = v
        return L.YuvGrainNoise(3, t0, (C.c_float * 16)(*k), chroma, (C.c_float * 3)(*taps))

    ok = gr()
    nan, inf = float("nan"), float("inf")
    fb8 = f8.frame_bytes(40, 72)
    R_ = L.YuvRect
    refused = [
        (None, f8, None, ok, gauss, dst, 1, 40, 72), (src, None, None, ok, gauss, dst, 1, 40, 72), (src, f8, None, None, gauss, dst, 1, 40, 72),      # null pointers
        (src, f8, None, ok, None, dst, 1, 40, 72), (src, f8, None, ok, gauss, None, 1, 40, 72),
        (src, yuv_fmt(12, 0, 0, 0), None, ok, gauss, dst, 1, 40, 72), (src, yuv_fmt(8, 3, 0, 0), None, ok, gauss, dst, 1, 40, 72),      # bits, chroma code
        (src, yuv_fmt(8, 0, 2, 0), None, ok, gauss, dst, 1, 40, 72), (src, yuv_fmt(8, 0, 0, 2), None, ok, gauss, dst, 1, 40, 72),       # matrix, range
        (src + 1, f10, None, ok, gauss, dst, 1, 40, 72), (src, f10, None, ok, gauss, dst + 1, 1, 40, 72),                               # 10 bit: an odd address
        (src, f8, R_(-1, 0, 8, 8), ok, gauss, dst, 1, 40, 72), (src, f8, R_(0, 0, 73, 8), ok, gauss, dst, 1, 40, 72),                   # a rectangle outside
        (src, f8, R_(0, 0, 8, 0), ok, gauss, dst, 1, 40, 72), (src, f8, R_(70, 38, 8, 8), ok, gauss, dst, 1, 40, 72),
        (src, f10, R_(1, 0, 8, 8), ok, gauss, dst, 1, 40, 72), (src, f10, R_(0, 2, 7, 8), ok, gauss, dst, 1, 40, 72),                   # 4:2:0: odd origin, odd size inside
        (src, f8, None, ok, gauss + 2, dst, 1, 40, 72),                                                                                 # gauss not 4-byte aligned
        (src, f8, None, gr(t0=-1), gauss, dst, 1, 40, 72),                                                                              # t0
        (src, f8, None, gr(k0=-1.0), gauss, dst, 1, 40, 72), (src, f8, None, gr(k15=nan), gauss, dst, 1, 40, 72),                       # a knot
        (src, f8, None, gr(k7=inf), gauss, dst, 1, 40, 72),
        (src, f8, None, gr(chroma=-0.5), gauss, dst, 1, 40, 72), (src, f8, None, gr(chroma=nan), gauss, dst, 1, 40, 72),                # the chroma share
        (src, f8, None, gr(chroma=inf), gauss, dst, 1, 40, 72),
        (src, f8, None, gr(taps=(nan, 0.0, 0.0)), gauss, dst, 1, 40, 72), (src, f8, None, gr(taps=(1.0, inf, 0.0)), gauss, dst, 1, 40, 72),      # the taps
        (src, f8, None, gr(taps=(1.0, -0.01, 0.0)), gauss, dst, 1, 40, 72), (src, f8, None, gr(taps=(1.0, 0.0, -0.01)), gauss, dst, 1, 40, 72),
        (src, f8, None, gr(taps=(0.0, 0.70710678, 0.0)), gauss, dst, 1, 40, 72),                                                        # unit energy, but w0 = 0
        (src, f8, None, gr(taps=(1.002, 0.0, 0.0)), gauss, dst, 1, 40, 72), (src, f8, None, gr(taps=(0.998, 0.0, 0.0)), gauss, dst, 1, 40, 72),      # energy off by 4e-3
        (src, f8, None, gr(taps=(0.5, 0.5, 0.5)), gauss, dst, 1, 40, 72),
        (src, f8, None, ok, gauss, src + fb8, 2, 40, 72), (src + 2 * fb8 - 1, f8, None, ok, gauss, src, 2, 40, 72),                     # overlap that is not in place
        (src, f8, None, ok, gauss, src + 1, 1, 40, 72),
        (src, f8, None, ok, gauss, dst, 0, 40, 72), (src, f8, None, ok, gauss, dst, 65536, 40, 72),                                     # T
        (src, f8, None, ok, gauss, dst, 1, 0, 72), (src, f8, None, ok, gauss, dst, 1, 40, 0),                                           # H, W
        (src, f8, None, ok, gauss, src + (1 << 30), 1, 16 * 65535 + 1, 8),                                                              # more rows of workgroups than a grid has
    ]
    for args in refused:
        r, g = args[2], args[3]
        rc = lib.sn_yuv_grain(args[0], args[1], None if r is None else C.byref(r), None if g is None else C.byref(g), *args[4:], None)
        assert rc == -22, args
