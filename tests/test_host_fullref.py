"""CPU tests of the full-reference part of the report (shiftnet_amd/fullref.py, ``--gt``) against what the reference implementation recorded
(tests/golden/ssim_cases.npz, made by tools/make_ssim_golden.py from the generators of tests/ssim_cases.py): the float64 restatement of the device
sums (tests/ssim_ref.py) plus ``ssim_from_tiles``, ``psnr_from_sums`` on the rows of tests/diff_stats_ref.py, ``inf`` at zero error, the summary, the
report file's eight columns, the new symbol, and the refusals of the C entry point and of the command line.

Tolerances, measured here against the fixture (DESIGN.md 3.34 has the table).  Restatement and reference are both float64 and differ in the order of
their sums only (separable filter and tile sums here, one 11 x 11 correlation and one mean there):
  * SSIM: largest relative difference 6.3e-14 (3x7) on the textured pairs, asserted at SSIM_RTOL = 6.3e-13, ten times that; the near-flat pairs
    (``Case.level``) are held to the same figure and read 4.0e-13 at most (code 250, one code of noise: G(a a) - G(a)^2 cancels twelve digits);
  * PSNR: largest relative difference 3.3e-16, asserted at PSNR_RTOL = 3.3e-15, ten times that -- the sums are exact integers, what is left is a logarithm."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import diff_stats_ref as D
import ssim_cases as K
import ssim_ref as SR
from shiftnet_amd import fullref as F
from shiftnet_amd import report as rep
from shiftnet_amd import restore_cli, y4m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_RTOL = 6.3e-13
PSNR_RTOL = 3.3e-15


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(ROOT, "tests", "golden", "ssim_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def size(c):
    return (c.H, c.W) if c.rect is None else (c.rect[3], c.rect[2])


def test_the_fixture_has_every_case_and_the_taps_are_the_definition(recorded):
    assert set(recorded) == {k + c.name for c in K.CASES for k in ("ssim/", "psnr/")}
    for c in K.CASES:
        assert recorded["ssim/" + c.name].shape == (len(c.seeds),) and recorded["psnr/" + c.name].shape == (len(c.seeds), 3)
    g = F.ssim_taps()
    want = np.array([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)])
    assert g.dtype == np.float64 and np.allclose(g, want / want.sum(), rtol=1e-15, atol=0) and np.array_equal(g, g[::-1])
    assert F.ssim_constants(8) == ((0.01 * 255) ** 2, (0.03 * 255) ** 2) and F.ssim_constants(10) == ((0.01 * 1023) ** 2, (0.03 * 1023) ** 2)
    assert F.FullRef._fields == rep.COLUMNS_F == F.FIELDS


def test_the_float64_restatement_gives_the_references_ssim(recorded):
    worst = 0.0
    for c in K.CASES:
        a, b = K.payloads(c)
        tiles = SR.ssim_sums_ref(a, b, c.fmt, c.H, c.W, c.rect)
        h, w = size(c)
        assert tiles.shape == (len(c.seeds), -(-h // 32), -(-w // 32))
        for t in range(len(c.seeds)):
            got, want = F.ssim_from_tiles(tiles[t], h, w), float(recorded["ssim/" + c.name][t])
            rel = abs(got - want) / abs(want)
            print(f"{c.name}[{t}]: reference {want:.9f}, relative difference {rel:.3g}")
            worst = max(worst, rel)
        if c.same:
            assert np.array_equal(tiles[0], SR.tile_counts(h, w)) and F.ssim_from_tiles(tiles[0], h, w) == 1.0
    print(f"largest relative difference of an SSIM: {worst:.3g}")
    assert worst <= SSIM_RTOL


def test_psnr_from_the_exact_sums_is_the_references_psnr_and_inf_at_zero_error(recorded):
    worst = 0.0
    for c in K.CASES:
        a, b = K.payloads(c)
        rows = D.diff_stats_ref(a, b, c.fmt, c.H, c.W, rect=c.rect)
        for t in range(len(c.seeds)):
            got, want = F.psnr_from_sums(rows[t], c.fmt.bits), recorded["psnr/" + c.name][t]
            if c.same:
                assert got == (math.inf,) * 3 and np.isinf(want).all()
                continue
            rel = max(abs(g - w) / w for g, w in zip(got, want))
            print(f"{c.name}[{t}]: reference {want}, relative difference {rel:.3g}")
            worst = max(worst, rel)
    print(f"largest relative difference of a PSNR: {worst:.3g}")
    assert worst <= PSNR_RTOL
    # by hand: N = 100 samples, sum d^2 = 400 -> mse 4 -> 10 log10(255^2 / 4); 25 chroma samples with sums 0 and 25
    row = [100, 0, 400, 0, 0, 0, 0, 0, 0, 0, 25, 0, 0, 0, 25, 0]
    y, u, v = F.psnr_from_sums(row, 8)
    assert y == 10 * math.log10(255.0 ** 2 / 4.0) and u == math.inf and v == 10 * math.log10(255.0 ** 2)
    assert F.psnr_from_sums(row, 10)[0] == 10 * math.log10(1023.0 ** 2 / 4.0)
    with pytest.raises(ValueError, match="16 words"):
        F.psnr_from_sums(row[:8], 8)


def test_the_summary_has_means_without_inf_and_medians_with():
    f = [F.FullRef(30.0, 40.0, 35.0, math.inf, 36.0, 37.0, 0.9, 0.95), F.FullRef(32.0, math.inf, 35.0, math.inf, 36.0, 39.0, 0.8, 1.0),
         F.FullRef(31.0, 44.0, 38.0, math.inf, 33.0, 38.0, 0.7, 0.99)]
    s = F.summarize_fullref(f)
    assert s["mean"]["psnr_y_in"] == 31.0 and s["median"]["psnr_y_in"] == 31.0 and s["inf"]["psnr_y_in"] == 0
    assert s["mean"]["psnr_y_out"] == 42.0 and s["median"]["psnr_y_out"] == 44.0 and s["inf"]["psnr_y_out"] == 1
    assert math.isnan(s["mean"]["psnr_u_out"]) and s["median"]["psnr_u_out"] == math.inf and s["inf"]["psnr_u_out"] == 3
    assert s["mean"]["ssim_in"] == math.fsum([0.9, 0.8, 0.7]) / 3 and s["median"]["ssim_out"] == 0.99
    empty = F.summarize_fullref([])
    assert all(math.isnan(v) for v in empty["mean"].values()) and all(math.isnan(v) for v in empty["median"].values())
    line = F.summary_line_fullref(s)
    assert "psnr_y_in mean 31.00 median 31.00" in line and "ssim_out mean 0.9800 median 0.9900" in line and "1 inf left out" in line


def test_the_report_file_gains_eight_columns_and_reads_back():
    sums = [1000, 10, 5000, 990, 100, 980, 90, 50, 200, 1500, 250, 1, 300, -2, 280, 0]
    frames = rep.frames_report([sums, sums, sums], [0, 0, 1], [None] * 3, 8, 1, 0)
    full = [F.FullRef(30.125, 40.5, 35.0, math.inf, 36.0, 37.0, 0.9, 0.95), F.FullRef(32.0, math.inf, 35.5, math.inf, 36.25, 39.0, 0.8, 1.0),
            F.FullRef(31.0, 44.0, 38.0, math.inf, 33.0, 38.0, 0.7, 0.99)]
    pairs = [(5.25, 4.5), (float("nan"), 6.0), (7.75, float("nan"))]
    plain = rep.format_report(frames, "edge 16")
    for quality in (None, pairs):
        text = rep.format_report(frames, "edge 16", None, quality, full)
        lines = text.splitlines()
        cols = [ln for ln in lines if ln.startswith("# frame ")]
        assert len(cols) == 1 and tuple(cols[0].split()[-8:]) == F.FIELDS
        assert lines[-1].startswith("# median ") and lines[-1].split()[-8:] == [repr(v) for v in (31.0, 44.0, 35.5, math.inf, 36.0, 38.0, 0.8, 0.99)]
        body = [ln for ln in lines if not ln.startswith("#")]
        assert [ln.split()[-8:] for ln in body] == [[repr(float(v)) for v in f] for f in full]
        without = rep.format_report(frames, "edge 16", None, quality)
        assert [ln.split()[:-8] for ln in body] == [ln.split() for ln in without.splitlines() if not ln.startswith("#")]
        assert rep.parse_report_fullref(text) == full and all(isinstance(f, F.FullRef) for f in rep.parse_report_fullref(text))
        assert [f.frame for f in rep.parse_report(text)] == [f.frame for f in frames] and rep.parse_report(text) == rep.parse_report(plain)
        got = rep.parse_report_quality(text)
        assert got == [None] * 3 if quality is None else (got[0] == pairs[0] and np.isnan(got[1][0]) and got[2][0] == 7.75)
    assert rep.parse_report_fullref(plain) == [None] * 3 and rep.parse_report_fullref(rep.format_report(frames, "", None, pairs)) == [None] * 3
    assert rep.format_report(frames, "edge 16", None, None, None) == plain
    with pytest.raises(ValueError):
        rep.format_report(frames, "", None, None, full[:2])


def test_header_build_list_and_library_have_the_new_symbol_and_the_entry_point_refuses_on_the_host():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_ssim.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_ssim.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    from shiftnet_amd.io_edges import ssim_tiles, yuv_fmt
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^int sn_yuv_ssim_sums\(const uint8_t\* a, const uint8_t\* b, const sn_yuv_fmt\* fmt, const sn_yuv_rect\* rect /\* NULL: whole frame \*/,\s+"
                     r"double\* dst /\* \[T\]\[nty\]\[ntx\] \*/, int T, int H, int W, void\* stream\);", header, flags=re.M)
    assert re.search(r"#define SN_SSIM_TILE 32\b", header) and L.SN_SSIM_TILE == 32 == SR.TILE
    assert ssim_tiles(33, 65) == (2, 3) and ssim_tiles(32, 32) == (1, 1) and ssim_tiles(1, 1) == (1, 1)
    assert hasattr(lib, "sn_yuv_ssim_sums") and "sn_yuv_ssim_sums" in L.SYMBOLS and len(lib.sn_yuv_ssim_sums.argtypes) == 9
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    # the argument checks are host side and need no GPU: host memory is refused before anything would read it
    arr = np.zeros(1 << 16, np.uint8)
    buf = arr.ctypes.data + (-arr.ctypes.data) % 16
    a, b, dst = buf, buf + 16384, buf + 49152
    f8, f10 = yuv_fmt(8, L.SN_YUV_444, L.SN_YUV_BT709, L.SN_YUV_LIMITED), yuv_fmt(10, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    R = L.YuvRect
    big = 2 ** 31 - 1
    refused = [
        (None, b, f8, None, dst, 1, 40, 72), (a, None, f8, None, dst, 1, 40, 72), (a, b, None, None, dst, 1, 40, 72), (a, b, f8, None, None, 1, 40, 72),      # null pointers
        (a, b, yuv_fmt(12, 0, 0, 0), None, dst, 1, 40, 72), (a, b, yuv_fmt(8, 3, 0, 0), None, dst, 1, 40, 72),                   # bits, chroma code
        (a + 1, b, f10, None, dst, 1, 40, 72), (a, b + 1, f10, None, dst, 1, 40, 72),                                            # 10 bit: an odd address
        (a, b, f8, None, dst + 4, 1, 40, 72),                                                                                    # dst not 8-byte aligned
        (a, b, f8, R(0, 0, 0, 40), dst, 1, 40, 72), (a, b, f8, R(40, 0, 40, 40), dst, 1, 40, 72),                                # an empty rectangle, one past the frame
        (a, b, f10, R(1, 0, 40, 40), dst, 1, 40, 72), (a, b, f10, R(0, 0, 39, 40), dst, 1, 40, 72),                              # 4:2:0: shared chroma samples
        (a, b, f8, None, dst, 0, 40, 72), (a, b, f8, None, dst, 65536, 40, 72),                                                  # T
        (a, b, f8, None, dst, 1, 0, 72), (a, b, f8, None, dst, 1, 40, 0),                                                        # H, W
        (a, b, f8, None, dst, 1, big, big),                                                                                      # 2^52 tiles: beyond the bound on units
    ]
    for args in refused:
        rect = args[3]
        assert lib.sn_yuv_ssim_sums(args[0], args[1], args[2], None if rect is None else C.byref(rect), *args[4:], None) == -22, args


def _write(path, header, payloads):
    with open(path, "wb") as fh:
        wr = y4m.Y4MWriter(fh, header)
        for p in payloads:
            wr.write(p)


def test_the_command_line_refuses_gt_without_a_report_and_a_truth_of_another_size_or_tag(tmp_path, capsys):
    ap = restore_cli.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    assert ap.parse_args(base + ["in.y4m", "out.y4m"]).gt is None
    assert ap.parse_args(base + ["--report", "r.txt", "--gt", "t.y4m", "in.y4m", "out.y4m"]).gt == "t.y4m"
    # judged before any file is opened: the files named here do not exist
    with pytest.raises(SystemExit) as e:
        restore_cli.main(base + ["--gt", "/nonexistent/t.y4m", "/nonexistent/in.y4m", "/nonexistent/out.y4m"])
    assert e.value.code == 2 and "needs --report" in capsys.readouterr().err
    # judged against the header of the stream written, before the network is loaded (no GPU here)
    hd = y4m.Y4MHeader(width=72, height=40, chroma="420jpeg")
    src = tmp_path / "in.y4m"
    _write(src, hd, [np.zeros(hd.frame_bytes, np.uint8)])
    truths = {"size": (y4m.Y4MHeader(width=72, height=42, chroma="420jpeg"), [], ("72x42", "72x40")),
              "tag": (y4m.Y4MHeader(width=72, height=40, chroma="444"), [], ("C444", "C420jpeg")),
              "siting": (y4m.Y4MHeader(width=72, height=40, chroma="420mpeg2"), [], ("C420mpeg2", "C420jpeg")),
              "out_format": (hd, ["--out_format", "444p10"], ("C420jpeg", "C444p10"))}
    for name, (thd, more, words) in truths.items():
        gt = tmp_path / f"{name}.y4m"
        _write(gt, thd, [np.zeros(thd.frame_bytes, np.uint8)])
        with pytest.raises(SystemExit) as e:
            restore_cli.main(base + more + ["--report", str(tmp_path / "r.txt"), "--gt", str(gt), str(src), str(tmp_path / "out.y4m")])
        err = capsys.readouterr().err
        assert e.value.code == 2 and "--gt" in err and all(w in err for w in words), (name, err)
    with pytest.raises(SystemExit) as e:
        restore_cli.main(base + ["--report", str(tmp_path / "r.txt"), "--gt", str(tmp_path / "missing.y4m"), str(src), str(tmp_path / "out.y4m")])
    assert e.value.code == 2 and "--gt" in capsys.readouterr().err
