"""CPU tests of the motion blur (shiftnet_amd/degrade.py, ``--add_blur``): the gamma tables and the table arithmetic, the option's grammar, the plan of
the stage's launches, the refusals of the command line and of the C entry point, the new symbol, and the float32 restatement the kernel must equal
(tests/blur_ref.py: blur_ref) against the definition in float64 (blur_f64).

Bounds.  The round trip through the tables: 1e-3 of a 10-bit code (the tables have four times the levels, and both directions interpolate).  The
restatement against float64: both round a value to a code, so they differ where float32 and float64 land on two sides of a rounding boundary -- by
one code, never more -- and the share of such samples is capped at ten times what this test measured when it was written (SHARE), never above 1e-3."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import blur_ref as B
import yuv_ref as R
from shiftnet_amd import degrade, restore_cli, y4m
from test_gpu_degrade import FORMATS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_the_tables_are_monotonic_and_the_round_trip_returns_every_ten_bit_level():
    lin, rinv = degrade.gamma_tables(2.2)
    assert lin.dtype == rinv.dtype == np.float32 and lin.shape == (4096,) and rinv.shape == (4095,)
    assert not lin.flags.writeable and not rinv.flags.writeable and degrade.gamma_tables(2.2)[0] is lin
    for g in (1.0, 1.8, 2.2, 2.4, 3.0):
        lin, rinv = degrade.gamma_tables(g)
        assert lin[0] == 0.0 and lin[-1] == 1.0 and np.all(np.diff(lin) > 0) and np.all(np.isfinite(rinv)) and np.all(rinv > 0)
        assert np.array_equal(lin, ((np.arange(4096) / 4095.0) ** g).astype(f32))
        assert np.array_equal(rinv, (1.0 / np.diff(lin.astype(np.float64))).astype(f32))
        x = (np.arange(1024, dtype=np.float64) / 1023.0).astype(f32)
        back = B.encode(B.decode(x, lin), lin, rinv)
        err = float(np.max(np.abs(back.astype(np.float64) - x.astype(np.float64))) * 1023.0)
        print(f"gamma {g}: encode(decode(level)) is off by at most {err:.2e} of a 10-bit code")      # 6e-5 at 2.2
        assert err <= 1e-3
        # the mean of n equal values is the value: the decode's value goes through the mean and the encode
        for n in (3, 7, 15):
            v = B.decode(x, lin)
            acc = v.copy()
            for _ in range(n - 1):
                acc = acc + v
            err = float(np.max(np.abs(B.encode(acc * f32(1.0 / n), lin, rinv).astype(np.float64) - x.astype(np.float64))) * 1023.0)
            assert err <= 1e-3, (g, n, err)
    for bad in (0.99, 3.01, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            degrade.gamma_tables(bad)


def test_parse_add_blur_and_the_restorers_form():
    assert [degrade.parse_add_blur(w) for w in ("1", "7", " 15 ")] == [1, 7, 15]
    for bad in ("", "0", "2", "-3", "17", "3.0", "five", "3,5"):
        with pytest.raises(ValueError, match="odd"):
            degrade.parse_add_blur(bad)
    assert degrade.add_blur_form(None) == (None, 2.2) and degrade.add_blur_form(5) == (5, 2.2) and degrade.add_blur_form(np.int64(15), 1) == (15, 1.0)
    assert degrade.add_blur_form(1, 3.0) == (1, 3.0)
    for bad in (0, 2, 17, -1, 5.0, "5", True, [5]):
        with pytest.raises(ValueError, match="add_blur "):
            degrade.add_blur_form(bad)
    for bad in (0.5, 3.5, float("nan"), float("inf"), "2.2", None, True):
        with pytest.raises(ValueError, match="add_blur_gamma"):
            degrade.add_blur_form(5, bad)
        with pytest.raises(ValueError, match="add_blur_gamma"):
            degrade.add_blur_form(None, bad)


def test_the_plan_of_the_launches():
    plan = degrade.plan_blur
    # the stream's start, its middle (frames read r past the chunk) and its end
    assert plan(0, 4, 5, None, 5, False) == [(0, 4, 0, 5)]
    assert plan(4, 4, 5, None, 9, False) == [(4, 4, 0, 9)]
    assert plan(8, 1, 5, (), 8, True) == [(8, 1, 0, 8)]
    assert plan(4, 4, 5, None, 8, True) == [(4, 4, 0, 8)]                     # the end inside the read-ahead: the window is clamped there
    # a listed cut inside the chunk: one launch per scene segment, each clamped to its scene
    assert plan(4, 4, 5, [6], 9, False) == [(4, 2, 0, 5), (6, 2, 6, 9)]
    assert plan(0, 4, 5, [4], 5, False) == [(0, 4, 0, 3)]                     # a cut in the read-ahead only: the chunk's last windows stop there
    assert plan(4, 4, 5, [4, 20], 9, False) == [(4, 4, 4, 9)]                 # a cut past what has been read does not take part yet
    assert plan(8, 4, 3, [2, 9, 10], 12, False) == [(8, 1, 2, 8), (9, 1, 9, 9), (10, 2, 10, 12)]      # a scene of one frame: lo == hi
    # a stream shorter than r
    assert plan(0, 2, 5, None, 1, True) == [(0, 2, 0, 1)] and plan(0, 1, 15, None, 0, True) == [(0, 1, 0, 0)]
    assert plan(0, 4, 1, [2], 3, False) == [(0, 2, 0, 1), (2, 2, 2, 3)]       # n = 1 reads nothing ahead
    # every launch is one the entry point takes: lo <= first, first + count - 1 <= hi; the chunk is covered once, in order
    for cuts in (None, [1], [3, 4, 11], [5, 8]):
        for first in (0, 4, 8):
            got = plan(first, 4, 7, cuts, first + 6, False)
            assert [f for a, c, _, _ in got for f in range(a, a + c)] == list(range(first, first + 4))
            assert all(lo <= a and a + c - 1 <= hi for a, c, lo, hi in got)
    for bad in ((0, 4, 5, None, 4, False), (0, 4, 5, None, 2, True), (0, 0, 5, None, 4, True), (-1, 2, 5, None, 4, True)):
        with pytest.raises(ValueError):
            plan(*bad)


def _write(path, header, payloads):
    with open(path, "wb") as fh:
        wr = y4m.Y4MWriter(fh, header)
        for p in payloads:
            wr.write(p)


def test_the_command_line_takes_the_options_and_refuses_what_does_not_go_together(tmp_path, capsys):
    ap = restore_cli.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["in.y4m", "out.y4m"])
    assert a.add_blur is None and a.add_blur_gamma == 2.2 and a.degraded_out is None
    a = ap.parse_args(base + ["--add_blur", "7", "--add_blur_gamma", "1", "--degraded_out", "d.y4m", "in.y4m", "out.y4m"])
    assert a.add_blur == 7 and a.add_blur_gamma == 1.0 and a.degraded_out == "d.y4m"
    for bad in ("4", "0", "17", "3.5", "some"):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(base + ["--add_blur", bad, "in.y4m", "out.y4m"])
        assert e.value.code == 2 and "--add_blur" in capsys.readouterr().err
    helptext = " ".join(ap.format_help().split())
    for words in ("N / fps", "no frame is dropped", "pure power law, not the sRGB curve", "not a lens and not a rolling shutter", "N = 1 still runs",
                  "bars are averaged too", "the blur crosses them"):
        assert words in helptext, words
    # judged before any file is opened: the files named here do not exist
    gone = ["/nonexistent/in.y4m", "/nonexistent/out.y4m"]

    def refused(args, *words):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(base + args + gone)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err

    refused(["--add_blur", "5", "--report", "/nonexistent/r.txt", "--gt", "/nonexistent/t.y4m"], "--add_blur", "--gt")
    refused(["--add_blur", "5", "--add_noise", "10"], "--add_blur", "--add_noise")
    refused(["--add_blur_gamma", "1.8"], "--add_blur_gamma needs --add_blur")
    refused(["--add_blur", "5", "--add_blur_gamma", "0.5"], "--add_blur_gamma")
    refused(["--add_blur", "5", "--add_blur_gamma", "nan"], "--add_blur_gamma")
    refused(["--degraded_out", "/nonexistent/d.y4m"], "need --add_noise")
    refused(["--add_noise_seed", "3"], "need --add_noise")
    refused(["--add_blur", "5", "--add_noise_seed", "3"], "need --add_noise")
    # --degraded_out goes with --add_blur: the refusal that remains is the input that is not there
    with pytest.raises(FileNotFoundError):
        restore_cli.main(base + ["--add_blur", "5", "--degraded_out", "/nonexistent/d.y4m"] + gone)
    # judged against the header of the stream read, before the network is loaded (no GPU here)
    hd = y4m.Y4MHeader(width=72, height=40, chroma="420jpeg")
    src = tmp_path / "in.y4m"
    _write(src, hd, [np.zeros(hd.frame_bytes, np.uint8)])
    with pytest.raises(SystemExit) as e:
        restore_cli.main(base + ["--add_blur", "5", "--report", str(tmp_path / "r.txt"), "--out_format", "444p10", str(src), str(tmp_path / "out.y4m")])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--add_blur" in err and "--out_format" in err and "C420jpeg" in err and "C444p10" in err


def test_header_build_list_and_library_have_the_new_symbol_and_the_entry_point_refuses_on_the_host():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_blur.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_blur.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    from shiftnet_amd.io_edges import yuv_fmt
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^typedef struct sn_yuv_blur_window \{ int n; int c0; int lo; int hi; \} sn_yuv_blur_window;", header, flags=re.M)
    assert re.search(r"^int sn_yuv_blur\(const uint8_t\* src, int S, const sn_yuv_fmt\* fmt, const sn_yuv_blur_window\* win,\s+"
                     r"const float\* lin /\* device, 4096, or NULL \*/, const float\* rinv /\* device, 4095, or NULL \*/,\s+"
                     r"uint8_t\* dst, int T, int H, int W, void\* stream\);", header, flags=re.M)
    assert re.search(r"^#define SN_BLUR_MAX_TAPS 15\b", header, flags=re.M) and L.SN_BLUR_MAX_TAPS == degrade.BLUR_MAX_TAPS == 15
    assert hasattr(lib, "sn_yuv_blur") and "sn_yuv_blur" in L.SYMBOLS and len(lib.sn_yuv_blur.argtypes) == 11
    assert C.sizeof(L.YuvBlurWindow) == 16 and [f[0] for f in L.YuvBlurWindow._fields_] == ["n", "c0", "lo", "hi"]
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    # the argument checks are host side and need no GPU: host memory is refused before anything would read it
    arr = np.zeros(1 << 20, np.uint8)
    buf = arr.ctypes.data + (-arr.ctypes.data) % 16
    src, dst, lin = buf, buf + (1 << 19), buf + (1 << 19) + (1 << 18)       # 40 x 72 x 3 samples x 2 bytes x 7 frames < 2^18
    rinv = lin + 4096 * 4
    f8, f10 = yuv_fmt(8, L.SN_YUV_444, L.SN_YUV_BT709, L.SN_YUV_LIMITED), yuv_fmt(10, L.SN_YUV_420_LEFT, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    fb8 = f8.frame_bytes(40, 72)
    S = 7

    def win(n=5, c0=2, lo=0, hi=6):
        return L.YuvBlurWindow(n, c0, lo, hi)

    ok = win()
    # (src, S, fmt, win, lin, rinv, dst, T, H, W)
    refused = [
        (None, S, f8, ok, lin, rinv, dst, 3, 40, 72), (src, S, None, ok, lin, rinv, dst, 3, 40, 72), (src, S, f8, None, lin, rinv, dst, 3, 40, 72),     # null pointers
        (src, S, f8, ok, lin, rinv, None, 3, 40, 72),
        (src, S, yuv_fmt(12, 0, 0, 0), ok, lin, rinv, dst, 3, 40, 72), (src, S, yuv_fmt(8, 3, 0, 0), ok, lin, rinv, dst, 3, 40, 72),                    # bits, chroma code
        (src, S, yuv_fmt(8, 0, 2, 0), ok, lin, rinv, dst, 3, 40, 72), (src, S, yuv_fmt(8, 0, 0, 2), ok, lin, rinv, dst, 3, 40, 72),                     # matrix, range
        (src + 1, S, f10, ok, lin, rinv, dst, 3, 40, 72), (src, S, f10, ok, lin, rinv, dst + 1, 3, 40, 72),                                             # 10 bit: an odd address
        (src, 0, f8, ok, lin, rinv, dst, 3, 40, 72), (src, -1, f8, ok, lin, rinv, dst, 3, 40, 72),                                                      # S
        (src, S, f8, win(n=4), lin, rinv, dst, 3, 40, 72), (src, S, f8, win(n=0), lin, rinv, dst, 3, 40, 72),                                           # n
        (src, S, f8, win(n=17), lin, rinv, dst, 3, 40, 72), (src, S, f8, win(n=-3), lin, rinv, dst, 3, 40, 72),
        (src, S, f8, win(lo=-1), lin, rinv, dst, 3, 40, 72), (src, S, f8, win(hi=7), lin, rinv, dst, 3, 40, 72),                                        # 0 <= lo <= hi < S
        (src, S, f8, win(c0=5, lo=6, hi=5), lin, rinv, dst, 1, 40, 72), (src, S, f8, win(hi=2 ** 31 - 1), lin, rinv, dst, 3, 40, 72),
        (src, S, f8, win(c0=2, lo=3), lin, rinv, dst, 3, 40, 72), (src, S, f8, win(c0=4, hi=5), lin, rinv, dst, 3, 40, 72),                             # c0 < lo, c0 + T - 1 > hi
        (src, S, f8, win(c0=5), lin, rinv, dst, 3, 40, 72), (src, S, f8, win(c0=-1), lin, rinv, dst, 3, 40, 72),
        (src, S, f8, ok, lin, None, dst, 3, 40, 72), (src, S, f8, ok, None, rinv, dst, 3, 40, 72),                                                      # one table of two
        (src, S, f8, ok, lin + 2, rinv, dst, 3, 40, 72), (src, S, f8, ok, lin, rinv + 1, dst, 3, 40, 72),                                               # a table not 4-byte aligned
        (src, S, f8, ok, lin, rinv, src, 3, 40, 72), (src, S, f8, ok, None, None, src + S * fb8 - 1, 3, 40, 72),                                        # overlap: S frames of src ...
        (src + 3 * fb8 - 1, S, f8, ok, None, None, src, 3, 40, 72),                                                                                     # ... T frames of dst
        (src, S, f8, ok, lin, rinv, dst, 0, 40, 72), (src, S, f8, ok, lin, rinv, dst, 65536, 40, 72),                                                   # T
        (src, S, f8, ok, lin, rinv, dst, 3, 0, 72), (src, S, f8, ok, lin, rinv, dst, 3, 40, 0),                                                         # H, W
        (src, S, f8, ok, None, None, src + (1 << 30), 3, 2 * 8 * 65535 + 1, 8),                                                                         # more rows of workgroups than a grid has
    ]
    for args in refused:
        w = args[3]
        assert lib.sn_yuv_blur(args[0], args[1], args[2], None if w is None else C.byref(w), *args[4:], None) == -22, args


# ---- the restatement against the definition ---------------------------------------------------------------------------------------------
SIZES = [(16, 64), (37, 53)]
# The share of samples (all planes, all outputs, both sizes, gamma 2.2 and 1) at which blur_ref and blur_f64 differ, the largest over the eight formats,
# as this test measured it when it was written: 8 of 53730 at 10-bit 4:4:4 BT.709 limited.  The others: 0, 0, 2 and 0 of 27138 / 53730 at 8 bit (at most
# 7.4e-5), 2, 1 and 0 of 27138 at 10-bit 4:2:0 (at most 7.4e-5).  Ten times the largest is above 1e-3, so 1e-3 is the cap.  DESIGN.md 3.37.
SHARE = 8 / 53730                                                            # 1.49e-4
CAP = min(10 * SHARE, 1e-3)


def smooth_sources(fmt, H, W, S=9):
    """uint8 [S, frame_bytes]: a smooth base with dark regions (a quarter of the frame is near black) plus small per-frame variation -- a slow drift
    and a brightness flicker of a few per cent, not white noise in time."""
    yy, xx = np.meshgrid(np.arange(H) / max(H - 1, 1), np.arange(W) / max(W - 1, 1), indexing="ij")
    frames = []
    for t in range(S):
        d = 0.01 * t
        dark = np.clip(2.0 * (xx + d) - 0.5, 0.0, 1.0) ** 2                  # 0 on the left quarter, rising to 1
        gain = 1.0 + 0.03 * np.sin(1.7 * t)
        rgb = np.stack([dark * gain * (0.5 + 0.45 * np.sin(5.0 * (xx + d) + 3.0 * yy)),
                        dark * gain * (0.5 + 0.45 * np.cos(4.0 * yy - 2.0 * (xx + d))),
                        dark * gain * (0.3 + 0.6 * yy * (1.0 - xx) + 0.02 * np.sin(0.9 * t))])
        frames.append(np.clip(rgb, 0.0, 1.0))
    return R.egress_f64(np.stack(frames), fmt, H, W)


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: "%d-%d-%d-%d" % f)
def test_the_restatement_is_within_one_code_of_the_float64_definition(fmt):
    differ = total = 0
    for H, W in SIZES:
        src = smooth_sources(fmt, H, W)
        for gamma in (2.2, 1.0):
            a = B.blur_ref(src, fmt, H, W, 7, 3, 3, 0, 8, gamma)
            b = B.blur_f64(src, fmt, H, W, 7, 3, 3, 0, 8, gamma)
            qa = np.concatenate([p.ravel() for fr in a for p in R.split_planes(fr, fmt, H, W)])
            qb = np.concatenate([p.ravel() for fr in b for p in R.split_planes(fr, fmt, H, W)])
            d = np.abs(qa - qb)
            assert d.max() <= 1, (H, W, gamma, int(d.max()))
            differ, total = differ + int(np.count_nonzero(d)), total + d.size
            assert not np.array_equal(a[0], src[3])                          # it is a blur: the output is not the centre frame
    print(f"{fmt}: {differ} of {total} samples differ by one code, a share of {differ / total:.2e} (cap {CAP:.2e})")
    assert differ / total <= CAP
