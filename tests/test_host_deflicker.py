"""CPU tests of the deflicker rule (shiftnet_amd/deflicker.py, ``--deflicker``): ``tables`` against the restatement with plain loops and Python
integers (tests/deflicker_ref.py) bit for bit, the properties the rule is chosen for on synthetic 90 x 160 clips, the tables' shape, the chroma factor,
the option's grammar and refusals, the two new symbols and the refusals of the C entry points.

Bounds.  Measured on the CPU with tests/deflicker_ref.py on exactly these clips: the linear fade shifts no frame mean at all (0.0 codes; asserted is
that plus 0.25 code), and the rms second difference of the frame means of the +-8 % flicker clip falls to 0.3997 / 0.2053 / 0.0718 of what it was
at R = 1 / 3 / 7 on frames R .. T - R (11.10 -> 4.44, 11.40 -> 2.34, 11.27 -> 0.81 codes); asserted is twice each ratio, and below 1."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deflicker_ref as DR
import yuv_ref as R
from shiftnet_amd import deflicker as D
from shiftnet_amd import restore_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = R.Fmt(8, R.C420_LEFT, R.BT601, R.LIMITED)
F8FULL = R.Fmt(8, R.C444, R.BT709, R.FULL)
F10 = R.Fmt(10, R.C420_LEFT, R.BT709, R.LIMITED)
H, W = 90, 160
FADE_SHIFT = 0.0                                                  # measured with the restatement (the docstring)
FLICKER_RATIO = {1: 0.3997, 3: 0.2053, 7: 0.0718}


def random_hists(rng, T, L, n, kind):
    """[T][L] histograms of n samples each.  kind: "dense", "gaps" (most bins empty, other ones in every frame), "single" (some one-bin frames)."""
    out = np.zeros((T, L), dtype=np.int64)
    for t in range(T):
        if kind == "dense":
            p = rng.random(L) ** 3
        elif kind == "gaps":
            p = np.where(rng.random(L) < 0.1, rng.random(L), 0.0)
            p[rng.integers(0, L)] += 0.5
        else:
            p = np.zeros(L)
            if t % 3 == 0:
                p[rng.integers(0, L)] = 1.0                         # a flat frame
            else:
                p[rng.integers(0, L, 5)] = rng.random(5) + 0.1
        out[t] = rng.multinomial(n, p / p.sum())
    return out


@pytest.mark.parametrize("fmt", [F8, F8FULL, F10], ids=lambda f: "%d-%d-%d-%d" % f)
@pytest.mark.parametrize("kind", ["dense", "gaps", "single"])
@pytest.mark.parametrize("radius", [1, 3, 15])
def test_tables_equal_the_restatement_bit_for_bit(fmt, kind, radius):
    L = 1 << fmt.bits
    rng = np.random.default_rng(fmt.bits * 100 + radius + len(kind))
    hists = random_hists(rng, 9, L, 90 * 160, kind)
    for lo, hi in ((0, 9), (2, 8)):                                # the list is the clip; a clip inside the list
        for chroma in ("gain", "off"):
            lut, info = D.tables(hists, lo, hi, radius, fmt, chroma)
            want, winfo = DR.tables_ref(hists, lo, hi, radius, fmt.bits, fmt.range == R.FULL, chroma)
            assert lut.dtype == np.uint16 and lut.shape == (hi - lo, 2, L) and np.array_equal(lut, want)
            assert info == winfo                                    # floats compared with ==: bit for bit
            assert [i[0] for i in info] == [min(radius, t - lo, hi - 1 - t) for t in range(lo, hi)]
            assert np.all(np.diff(lut[:, 0].astype(int), axis=1) >= 0)      # every lutY is non-decreasing
    # a part of the clip is that part of the whole
    lut, info = D.tables(hists, 1, 9, radius, fmt)
    part, pinfo = D.tables(hists, 1, 9, radius, fmt, "gain", 3, 4)
    assert np.array_equal(part, lut[2:6]) and pinfo == info[2:6]


def test_absent_codes_take_the_nearest_present_code_below_or_the_first_present_one():
    hists = np.zeros((3, 256), dtype=np.int64)
    hists[0, [40, 100, 200]] = (10, 20, 30)
    hists[1, [50, 120, 220]] = (10, 20, 30)
    hists[2, [60, 140, 240]] = (10, 20, 30)
    lut, info = D.tables(hists, 0, 3, 1, F8)
    assert info[0][0] == 0 and info[2][0] == 0 and info[1][0] == 1
    # r = 0: every present code maps to itself, an absent one to the present code below, the ones below the first to the first
    ly = lut[0, 0].astype(int)
    assert list(ly[[40, 100, 200]]) == [40, 100, 200] and np.all(ly[:40] == 40) and np.all(ly[41:100] == 40) and np.all(ly[100:200] == 100) and np.all(ly[200:] == 200)
    # the middle frame: the median of (40, 50, 60) and so on is the frame itself
    ly = lut[1, 0].astype(int)
    assert list(ly[[50, 120, 220]]) == [50, 120, 220] and np.all(ly[:50] == 50) and np.all(ly[51:120] == 50) and np.all(ly[221:] == 220)
    want, _ = DR.tables_ref(hists, 0, 3, 1, 8, False)
    assert np.array_equal(lut, want)


def tables_refuse(**kw):
    args = dict(hists=np.full((3, 256), 4, dtype=np.int64), lo=0, hi=3, R=1, fmt=F8, chroma="gain")
    args.update(kw)
    with pytest.raises(ValueError):
        D.tables(**args)


def test_tables_refuse_what_they_cannot_take():
    uneven = np.full((3, 256), 4, dtype=np.int64)
    uneven[1, 0] += 1
    for kw in (dict(hists=np.zeros((3, 255))), dict(hists=np.zeros((3, 256))), dict(hists=uneven), dict(lo=2, hi=2), dict(hi=4), dict(lo=-1), dict(R=0),
               dict(R=16), dict(chroma="mean"), dict(first=0, count=4), dict(lo=1, first=0), dict(fmt=F10)):
        tables_refuse(**kw)


# ---- synthetic clips ---------------------------------------------------------------------------------------------------------------------
def picture(seed=3):
    """A textured 90 x 160 luma picture in the limited range, float64: smooth structure plus texture."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 110.0 + 60.0 * np.sin(x / 23.0) * np.cos(y / 17.0) + 25.0 * np.sin((x + 2 * y) / 5.0)
    return np.clip(base + rng.normal(0.0, 6.0, (H, W)), 20.0, 230.0)


def gained(pic, g):
    """The picture under a gain about black, as 8-bit codes."""
    return np.clip(np.floor(16.0 + g * (pic - 16.0) + 0.5), 0, 255).astype(np.int64)


def hists_of(frames):
    return np.stack([np.bincount(f.ravel(), minlength=256) for f in frames])


def applied(frames, lut):
    return [lut[t, 0].astype(np.int64)[f] for t, f in enumerate(frames)]


def test_a_static_clip_and_an_unlisted_cut_between_static_scenes_leave_as_they_came():
    a, b = gained(picture(3), 1.0), gained(picture(4), 0.6)
    for frames, radius in (([a] * 9, 3), ([a] * 6 + [b] * 6, 3), ([a] * 6 + [b] * 6, 1)):
        hists = hists_of(frames)
        lut, info = D.tables(hists, 0, len(frames), radius, F8)
        for t, f in enumerate(frames):                              # every frame maps to itself: identity on present codes
            present = hists[t] > 0
            assert np.array_equal(lut[t, 0][present], np.arange(256)[present]), t
            assert np.array_equal(lut[t, 1], np.arange(256)) and info[t][3] == 1.0 and info[t][1] == info[t][2]      # k = 1, identity lutC
        assert all(np.array_equal(g, f) for g, f in zip(applied(frames, lut), frames))


def test_a_linear_fade_passes():
    pic = picture(3)
    frames = [gained(pic, 0.5 + 0.5 * t / 23.0) for t in range(24)]
    lut, info = D.tables(hists_of(frames), 0, 24, 3, F8)
    shift = max(abs(i[2] - i[1]) for i in info)
    print(f"linear fade, 24 frames, R = 3: the largest shift of a frame mean is {shift:.4f} codes")
    assert shift <= FADE_SHIFT + 0.25


@pytest.mark.parametrize("radius", [1, 3, 7])
def test_uniform_gain_flicker_is_taken_out(radius):
    pic = picture(3)
    gains = 1.0 + np.random.default_rng(11).uniform(-0.08, 0.08, 48)
    frames = [gained(pic, g) for g in gains]
    lut, info = D.tables(hists_of(frames), 0, 48, radius, F8)
    sl = slice(radius, 48 - radius + 1)                            # frames R .. T - R
    before, after = DR.roughness([i[1] for i in info][sl]), DR.roughness([i[2] for i in info][sl])
    assert [i[2] for i in info] == [float(np.mean(f)) for f in applied(frames, lut)]      # mean_out is the mean of the frame the table makes
    print(f"+-8 % flicker, 48 frames, R = {radius}: rms second difference of the frame means {before:.3f} -> {after:.3f}, ratio {after / before:.4f}")
    assert after / before <= 2.0 * FLICKER_RATIO[radius] and after / before < 1.0


# ---- chroma ------------------------------------------------------------------------------------------------------------------------------
def test_the_chroma_factor_clamps_follows_a_pure_gain_and_can_be_off():
    ramp = np.repeat(np.arange(16, 81), 64).reshape(-1, 64).astype(np.float64)      # a ramp from black up, low enough that a gain of 3 clips nothing
    for g, want in ((0.8, 0.8), (1.25, 1.25), (0.3, 0.5), (3.0, 2.0)):
        dark = np.clip(np.floor(16.0 + g * (ramp - 16.0) + 0.5), 0, 255).astype(np.int64)
        frames = [ramp.astype(np.int64), dark, ramp.astype(np.int64)]      # the flickering frame in the middle: the median is the ramp
        lut, info = D.tables(hists_of(frames), 0, 3, 1, F8)
        k = info[1][3]
        ratio = (info[1][2] - 16.0) / (info[1][1] - 16.0)          # what the means did
        print(f"gain {g}: k {k:.4f}, the means' ratio {ratio:.4f}, 1 / g {1 / g:.4f}")
        if 0.5 <= 1.0 / g <= 2.0:
            assert abs(k - 1.0 / g) <= 0.01 / g                    # within 1 % of the gain that undoes the flicker
        else:
            assert k == (0.5 if g > 1 else 2.0)
        co = 128.0
        assert np.array_equal(lut[1, 1], np.clip(np.floor(co + k * (np.arange(256) - co) + 0.5), 0, 255).astype(np.uint16))
        off, oinfo = D.tables(hists_of(frames), 0, 3, 1, F8, "off")
        assert np.array_equal(off[:, 1], np.tile(np.arange(256, dtype=np.uint16), (3, 1))) and np.array_equal(off[:, 0], lut[:, 0])
        assert [i[3] for i in oinfo] == [1.0] * 3 and [i[:3] for i in oinfo] == [i[:3] for i in info]
    # a frame at black: m - yo < 1 gives k = 1 whatever the table does
    black, grey = np.full((8, 8), 16, dtype=np.int64), np.full((8, 8), 120, dtype=np.int64)
    lut, info = D.tables(hists_of([grey, black, grey]), 0, 3, 1, F8)
    assert lut[1, 0][16] == 120 and info[1][3] == 1.0 and np.array_equal(lut[1, 1], np.arange(256))
    assert D.black_code(8, R.LIMITED) == 16 and D.black_code(10, R.LIMITED) == 64 and D.black_code(10, R.FULL) == 0


# ---- surface -----------------------------------------------------------------------------------------------------------------------------
def test_the_grammar_and_the_refusals():
    assert D.parse_deflicker("3") == 3 and D.parse_deflicker(" 15 ") == 15 and D.parse_deflicker("1") == 1
    for bad in ("0", "16", "-1", "2.5", "", "auto"):
        with pytest.raises(ValueError):
            D.parse_deflicker(bad)
    assert D.deflicker_form(None) == (None, "gain") and D.deflicker_form(3) == (3, "gain") and D.deflicker_form(15, "off") == (15, "off")
    for bad in (0, 16, -1, 2.5, "3", True):
        with pytest.raises(ValueError, match="deflicker"):
            D.deflicker_form(bad)
    with pytest.raises(ValueError, match="deflicker_chroma"):
        D.deflicker_form(3, "mean")
    with pytest.raises(ValueError, match="deflicker_chroma.*needs deflicker"):
        D.deflicker_form(None, "off")
    with pytest.raises(ValueError, match="deflicker together with add_noise"):
        D.deflicker_form(3, "gain", [5.0] * 16, None)
    with pytest.raises(ValueError, match="deflicker together with add_blur"):
        D.deflicker_form(3, "gain", None, 7)
    assert D.deflicker_form(None, "gain", [5.0] * 16, 7) == (None, "gain")      # without the option nothing of it is judged
    assert D.mean_roughness([1.0, 2.0, 3.0, 4.0]) == 0.0 and D.mean_roughness([0.0, 1.0, 0.0]) == 2.0 and D.mean_roughness([5.0]) == 0.0
    text = D.format_deflicker([(0, 100.0, 100.0, 1.0), (1, 110.0, 100.5, 0.9), (0, 100.0, 100.0, 1.0)])
    assert text.splitlines()[:2] == ["0 100.0000 100.0000 1.000000", "1 110.0000 100.5000 0.900000"] and len(text.splitlines()) == 4
    assert "20.0000 before, 1.0000 after" in text.splitlines()[-1]


def test_the_command_line_takes_the_options_and_refuses_what_does_not_go_together(capsys):
    ap = restore_cli.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["in.y4m", "out.y4m"])
    assert a.deflicker is None and a.deflicker_chroma == "gain" and a.deflicker_out is None
    a = ap.parse_args(base + ["--deflicker", "3", "--deflicker_chroma", "off", "--deflicker_out", "d.txt", "in.y4m", "out.y4m"])
    assert (a.deflicker, a.deflicker_chroma, a.deflicker_out) == (3, "off", "d.txt")
    for more, word in ((["--deflicker", "0"], "--deflicker"), (["--deflicker", "16"], "--deflicker"), (["--deflicker", "3", "--deflicker_chroma", "mean"], "--deflicker_chroma")):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(base + more + ["in.y4m", "out.y4m"])
        assert e.value.code == 2 and word in capsys.readouterr().err
    gone = ["/nonexistent/in.y4m", "/nonexistent/out.y4m"]          # judged before any file is opened
    for more, words in ((["--deflicker", "3", "--add_noise", "5"], ["--deflicker", "--add_noise"]),
                        (["--deflicker", "3", "--add_blur", "7"], ["--deflicker", "--add_blur"]),
                        (["--deflicker_out", "/nonexistent/d.txt"], ["--deflicker_out needs --deflicker"]),
                        (["--deflicker_chroma", "off"], ["needs deflicker"])):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(base + more + gone)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), (more, err)


def test_header_build_list_and_library_have_the_new_symbols_and_the_entry_points_refuse_on_the_host():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_deflicker.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_deflicker.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    from shiftnet_amd.io_edges import yuv_fmt
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^int sn_yuv_code_hist\(const uint8_t\* src, const sn_yuv_fmt\* fmt, const sn_yuv_rect\* rect /\* or NULL \*/,\s+"
                     r"uint32_t\* dst /\* \[T\]\[1 << bits\] \*/, int T, int H, int W, void\* stream\);", header, flags=re.M)
    assert re.search(r"^int sn_yuv_apply_lut\(const uint8_t\* src, const sn_yuv_fmt\* fmt, const sn_yuv_rect\* rect /\* or NULL \*/,\s+"
                     r"const uint16_t\* lut /\* device, \[T\]\[2\]\[1 << bits\]: Y, then Cb and Cr \*/, uint8_t\* dst,\s+"
                     r"int T, int H, int W, void\* stream\);", header, flags=re.M)
    vp, ci = C.c_void_p, C.c_int
    for name, argtypes in (("sn_yuv_code_hist", [vp, C.POINTER(L.YuvFmt), C.POINTER(L.YuvRect), vp, ci, ci, ci, vp]),
                           ("sn_yuv_apply_lut", [vp, C.POINTER(L.YuvFmt), C.POINTER(L.YuvRect), vp, vp, ci, ci, ci, vp])):
        assert hasattr(lib, name) and name in L.SYMBOLS
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is ci
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    # the argument checks are host side and need no GPU: host memory is refused before anything would read it
    arr = np.zeros(1 << 20, np.uint8)
    buf = arr.ctypes.data + (-arr.ctypes.data) % 16
    src, dst, aux = buf, buf + (1 << 18), buf + (1 << 19)          # 40 x 72 x 3 samples x 2 bytes x 2 frames < 2^18; aux: the histograms or the tables
    f8, f10 = yuv_fmt(8, L.SN_YUV_444, L.SN_YUV_BT709, L.SN_YUV_LIMITED), yuv_fmt(10, L.SN_YUV_420_LEFT, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    fb8 = f8.frame_bytes(40, 72)
    R_ = L.YuvRect
    bad_fmt = [yuv_fmt(12, 0, 0, 0), yuv_fmt(8, 3, 0, 0), yuv_fmt(8, 0, 2, 0), yuv_fmt(8, 0, 0, 2)]      # bits, chroma code, matrix, range
    bad_rect8 = [R_(-1, 0, 8, 8), R_(0, 0, 73, 8), R_(0, 0, 8, 0), R_(70, 38, 8, 8)]                     # a rectangle outside
    bad_rect10 = [R_(1, 0, 8, 8), R_(0, 2, 7, 8)]                                                        # 4:2:0: odd origin, odd size inside
    hist = [(None, f8, None, aux, 1, 40, 72), (src, None, None, aux, 1, 40, 72), (src, f8, None, None, 1, 40, 72)]      # null pointers
    hist += [(src, f, None, aux, 1, 40, 72) for f in bad_fmt]
    hist += [(src, f8, None, aux, 0, 40, 72), (src, f8, None, aux, 65536, 40, 72), (src, f8, None, aux, 1, 0, 72), (src, f8, None, aux, 1, 40, 0)]      # T, H, W
    hist += [(src + 1, f10, None, aux, 1, 40, 72), (src, f8, None, aux + 2, 1, 40, 72)]                 # 10 bit: an odd address; dst not 4-byte aligned
    hist += [(src, f8, r, aux, 1, 40, 72) for r in bad_rect8] + [(src, f10, r, aux, 1, 40, 72) for r in bad_rect10]
    hist += [(src, f8, None, aux, 1, 1 << 17, 1 << 16)]                                                 # 2^33 samples: a count is 32 bits
    for args in hist:
        r = args[2]
        assert lib.sn_yuv_code_hist(args[0], args[1], None if r is None else C.byref(r), *args[3:], None) == -22, args
    lut = [(None, f8, None, aux, dst, 1, 40, 72), (src, None, None, aux, dst, 1, 40, 72), (src, f8, None, None, dst, 1, 40, 72),
           (src, f8, None, aux, None, 1, 40, 72)]
    lut += [(src, f, None, aux, dst, 1, 40, 72) for f in bad_fmt]
    lut += [(src, f8, None, aux, dst, 0, 40, 72), (src, f8, None, aux, dst, 65536, 40, 72), (src, f8, None, aux, dst, 1, 0, 72),
            (src, f8, None, aux, dst, 1, 40, 0)]
    lut += [(src + 1, f10, None, aux, dst, 1, 40, 72), (src, f10, None, aux, dst + 1, 1, 40, 72), (src, f8, None, aux + 2, dst, 1, 40, 72)]
    lut += [(src, f8, r, aux, dst, 1, 40, 72) for r in bad_rect8] + [(src, f10, r, aux, dst, 1, 40, 72) for r in bad_rect10]
    lut += [(src, f8, None, aux, src + fb8, 2, 40, 72), (src + 2 * fb8 - 1, f8, None, aux, src, 2, 40, 72), (src, f8, None, aux, src + 1, 1, 40, 72)]      # overlap that is not in place
    lut += [(src, f8, None, aux, src + (1 << 30), 1, 64 * 65535 + 1, 8)]                                # more rows of workgroups than a grid has
    for args in lut:
        r = args[2]
        assert lib.sn_yuv_apply_lut(args[0], args[1], None if r is None else C.byref(r), *args[3:], None) == -22, args
