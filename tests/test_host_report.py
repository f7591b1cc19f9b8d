"""The method-noise report without a GPU: the ABI of ``sn_yuv_diff_stats``, the host arithmetic of shiftnet_amd/report.py on hand-computed sums and on
synthetic differences through the numpy restatement (tests/diff_stats_ref.py), the report file, and the option forms of the restorer and its CLI."""
import math
import os

import numpy as np
import pytest

import diff_stats_ref as D
import yuv_ref as R
from shiftnet_amd import noise, report, restore_cli, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)
nan = float("nan")


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_symbol_the_library_exports_it_and_the_abi_version_stays():
    from shiftnet_amd import lib as L
    lib = L.load()
    assert hasattr(lib, "sn_yuv_diff_stats") and "sn_yuv_diff_stats" in L.SYMBOLS
    assert L.SN_DIFF_STATS == 16 == D.WORDS == len(report.SUMS)
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20
    with open(os.path.join(ROOT, "include", "shiftnet_hip.h")) as fh:
        header = fh.read()
    assert "#define SN_ABI_VERSION 20 " in header and "#define SN_DIFF_STATS 16\n" in header
    assert ("int sn_yuv_diff_stats(const uint8_t* a, const uint8_t* b, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */,\n"
            "                      int edge, int64_t* dst /* [T][SN_DIFF_STATS] */, int T, int H, int W, void* stream);") in header


# ---- hand-computed sums -----------------------------------------------------------------------------------------------------------------
HAND_D = np.array([[1, -2, 0, 3], [2, 2, -1, 0], [-3, 1, 1, 2]])
# N, S1, S2 | Nx, Sx | Ny, Sy | St | Ne, S2e | Nc, Su, Su2, Sv, Sv2 | 0: the luma words are those of HAND_D, worked out by hand:
#   S1 = 2 + 3 + 1;  S2 = 14 + 9 + 15;  Sx = -2 + 2 + 0;  Sy = (2 - 4 + 0 + 0) + (-6 + 2 - 1 + 0)
HAND = [12, 6, 38, 9, 0, 8, -7, 0, 4, 20, 4, 2, 6, -4, 4, 0]


def test_the_numpy_restatement_gives_the_hand_sums_of_a_3_x_4_array():
    flat = np.zeros((3, 4), np.int64)
    got = D.sums_of_planes(HAND_D, flat, np.array([[1, 1], [-1, 1]]), np.array([[-1, -1], [-1, -1]]), edge=0, dY_next=HAND_D)
    assert got[:8] == HAND[:7] + [38]                                                 # with itself as the next frame St is S2
    assert got[8:10] == [12, 38] and got[10:] == [4, 2, 4, -4, 4, 0]                  # edge 0: every pixel is an edge pixel
    assert D.sums_of_planes(HAND_D, flat, HAND_D[:2, :2], HAND_D[:2, :2], edge=1)[7:10] == [0, 0, 0]      # a flat picture has no edge at 1; no next frame
    b = np.array([[10, 10, 10, 30], [10, 10, 10, 30], [10, 50, 10, 30]])              # e: 20 at (0,2), (1,2), (2,2); 40 at (1,1); 40 + 0 and 40 at (2,0), (2,1)
    got = D.sums_of_planes(HAND_D, b, flat[:2, :2], flat[:2, :2], edge=20)
    assert got[8:10] == [6, 0 + 1 + 1 + 4 + 9 + 1]
    assert D.sums_of_planes(HAND_D, b, flat[:2, :2], flat[:2, :2], edge=21)[8:10] == [3, 4 + 9 + 1]


@pytest.mark.parametrize("bits", [8, 10])
def test_frame_measures_of_the_hand_sums_are_the_hand_values_exactly(bits):
    r = report.frame_measures(HAND, bits, R.BT601, R.LIMITED)
    c = 1 << (bits - 8)
    assert (r.frame, r.window, r.sigma) == (0, 0, None) and math.isnan(r.rho_t)
    assert r.m == 0.5 and r.var == 35 / 12                                            # 38 / 12 - 1 / 4
    assert r.mean_y == 0.5 / c and r.rms_y == math.sqrt(38 / 12) / c
    g = math.sqrt(0.299 ** 2 + 0.587 ** 2 + 0.114 ** 2)
    assert abs(g - noise.luma_gain(R.BT601)) < 1e-15
    assert r.removed_sigma == math.sqrt(35 / 12) / (noise.luma_gain(R.BT601) * (219.0 * c / 255.0))
    assert r.rho_x == -3 / 35                                                         # (0 / 9 - 1 / 4) / (35 / 12)
    assert r.rho_y == -27 / 70                                                        # (-7 / 8 - 1 / 4) / (35 / 12)
    assert r.edge_share == 1 / 3 and r.edge_ratio == 20 / 9                           # (20 / 4) / (18 / 8)
    assert (r.mean_u, r.rms_u, r.mean_v, r.rms_v) == (0.5 / c, math.sqrt(1.5) / c, -1.0 / c, 1.0 / c)
    full = report.frame_measures(HAND, bits, R.BT709, R.FULL)
    assert full.removed_sigma == math.sqrt(35 / 12) / (noise.luma_gain(R.BT709) * (((1 << bits) - 1) / 255.0))
    with pytest.raises(ValueError, match="16 words"):
        report.frame_measures(HAND[:15], 8, 0, 0)


# ---- synthetic differences through the restatement ---------------------------------------------------------------------------------------
H = W = 64


def _payloads(Y, fmt=FMT):
    """[T, H, W] luma codes -> payloads with neutral chroma."""
    ch, cw = R.chroma_shape(fmt, H, W)
    c = np.full((ch, cw), 128 << (fmt.bits - 8))
    return np.stack([R.join_planes(y, c, c, fmt) for y in Y])


def test_iid_noise_reads_white_in_space_and_time_and_at_its_level():
    sigma = 10.0                                                                      # of 8-bit R'G'B'; on the luma codes that is sigma g s
    sd = sigma * noise.luma_gain(FMT.matrix) * noise.code_scale(FMT.bits, FMT.range)
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H, 0:W]
    clean = np.stack([90 + x + (y // 8) * 4] * 2)                                     # a ramp with steps: there are edge pixels and flat ones
    d = np.rint(rng.normal(0.0, sd, clean.shape)).astype(np.int64)
    assert np.abs(d).max() < 60
    sums = D.diff_stats_ref(_payloads(clean - d), _payloads(clean), FMT, H, W, edge=4)
    frames = report.frames_report(sums, [0, 0], [sigma, sigma], FMT.bits, FMT.matrix, FMT.range)
    bound = 5.0 / math.sqrt(H * W)
    for f in frames:
        assert abs(f.rho_x) <= bound and abs(f.rho_y) <= bound
        assert abs(f.removed_sigma - sigma) <= 0.03 * sigma
        assert 0.0 < f.edge_share < 1.0 and abs(f.edge_ratio - 1.0) <= 0.25          # 5 / sqrt(Ne) of a ratio of two means of chi-square variables
        assert f.sigma == sigma and f.mean_u == 0.0 and f.rms_v == 0.0
    assert abs(frames[0].rho_t) <= bound and math.isnan(frames[1].rho_t)
    assert frames[0].rho_t == report.pair_rho(sums[0], sums[1])
    med = report.summarize(frames)
    assert med["rho_t"] == frames[0].rho_t and med["removed_sigma"] == (frames[0].removed_sigma + frames[1].removed_sigma) / 2


def test_a_static_texture_removed_from_two_frames_is_fully_correlated_in_time():
    rng = np.random.default_rng(3)
    texture = rng.integers(-20, 21, (H, W))
    clean = np.stack([rng.integers(60, 180, (H, W)) for _ in range(2)])              # the pictures differ, what was taken out does not
    sums = D.diff_stats_ref(_payloads(clean + texture), _payloads(clean), FMT, H, W, edge=16)
    assert abs(report.pair_rho(sums[0], sums[1]) - 1.0) <= 1e-12
    assert math.isnan(report.pair_rho(sums[1], None))
    two = report.frames_report(sums, [0, 1], [None, None], 8, 0, 0)                   # in different windows: no pair
    assert math.isnan(two[0].rho_t) and two[0].sigma is None and (two[1].frame, two[1].window) == (1, 1)


def test_measures_without_a_denominator_are_nan():
    clean = np.full((2, H, W), 100)
    clean[:, :, W // 2:] = 140                                                        # one vertical edge
    sums = D.diff_stats_ref(_payloads(clean - 3), _payloads(clean), FMT, H, W, edge=16)
    r = report.frame_measures(sums[0], 8, 0, 0)
    assert r.m == 3.0 and r.var == 0.0 and r.removed_sigma == 0.0 and r.rms_y == 3.0
    assert math.isnan(r.rho_x) and math.isnan(r.rho_y) and math.isnan(report.pair_rho(sums[0], sums[1]))
    assert r.edge_share == 1 / W and r.edge_ratio == 1.0                              # d^2 is 9 on both sides of the threshold
    for edge, ne in ((0, H * W), (41, 0)):
        s = D.diff_stats_ref(_payloads(clean - 3), _payloads(clean), FMT, H, W, edge=edge)[0]
        assert s[8] == ne and math.isnan(report.frame_measures(s, 8, 0, 0).edge_ratio)
    same = D.diff_stats_ref(_payloads(clean), _payloads(clean), FMT, H, W, edge=16)[0]
    assert list(same) == [H * W, 0, 0, H * (W - 1), 0, (H - 1) * W, 0, 0, H, 0, (H // 2) * (W // 2), 0, 0, 0, 0, 0]
    z = report.frame_measures(same, 8, 0, 0)
    assert z.removed_sigma == 0.0 and math.isnan(z.rho_x) and math.isnan(z.edge_ratio)
    one = report.frame_measures([1, 5, 25, 0, 0, 0, 0, 0, 1, 25, 1, 0, 0, 0, 0, 0], 8, 0, 0)      # a picture of one pixel: no neighbour at all
    assert one.m == 5.0 and one.var == 0.0 and math.isnan(one.rho_x) and math.isnan(one.rho_y) and math.isnan(one.edge_ratio)
    assert all(math.isnan(v) for v in report.summarize([]).values())


# ---- the file -----------------------------------------------------------------------------------------------------------------------------
def test_the_report_file_reads_back_to_what_was_written_nan_and_dash_included():
    rng = np.random.default_rng(11)
    frames = []
    for i in range(7):
        f = report.FrameReport(i, i // 3, None if i < 3 else 12.5 + i / 3.0, *[float(v) for v in rng.normal(0.0, 1.0, len(report.MEASURES))])
        frames.append(f)
    frames[2].rho_t = frames[5].rho_t = frames[6].rho_t = nan
    frames[4].edge_ratio = nan
    frames[1].var = 1.0 / 3.0
    frames[6].rms_y = 1e-300
    text = report.format_report(frames, "edge 16")
    lines = text.splitlines()
    assert lines[0].startswith("#") and lines[2] == "# " + " ".join(report.COLUMNS) and lines[-1].startswith("# median ")
    assert len([ln for ln in lines if not ln.startswith("#")]) == 7
    assert lines[3].split()[2] == "-" and " nan" in lines[5]
    back = report.parse_report(text)
    assert back == frames and back[0] != frames[1]
    assert [float(w) for w in lines[-1].split()[5:]] == pytest.approx(list(report.summarize(frames).values()), nan_ok=True, rel=0, abs=0)
    assert report.parse_report("# nothing\n\n") == []
    with pytest.raises(ValueError, match="line 2"):
        report.parse_report("# header\n0 0 - 1.0\n")
    with pytest.raises(ValueError, match="line 1"):
        report.parse_report(" ".join(["x"] * len(report.COLUMNS)))
    assert "removed_sigma" in report.summary_line(report.summarize(frames))


# ---- the options ----------------------------------------------------------------------------------------------------------------------------
BASE = ["--variant", "denoise_small", "--checkpoint", "synthetic", "--sigma", "10", "in.y4m", "out.y4m"]


def test_the_parser_takes_the_report_and_refuses_a_bad_edge(capsys):
    ap = restore_cli.make_parser()
    a = ap.parse_args(BASE)
    assert a.report is None and a.report_edge == 16.0
    a = ap.parse_args(["--report", "r.txt", "--report_edge", "7.5"] + BASE)
    assert a.report == "r.txt" and a.report_edge == 7.5
    assert ap.parse_args(["--report_edge", "0"] + BASE).report_edge == 0.0
    for bad in ("-1", "nan", "inf", "sixteen"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--report", "r.txt", "--report_edge", bad] + BASE)
        assert "--report_edge" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                                   # judged before the input is opened or a device is touched
        restore_cli.main(["--report", "r.txt", "--view", "removed"] + BASE)
    err = capsys.readouterr().err
    assert "--report" in err and "removed" in err


def test_the_option_form_refuses_the_removed_view_and_a_bad_edge():
    assert windows.report_form() == (False, 16.0)
    assert windows.report_form(True, 0, None) == (True, 0.0)
    assert windows.report_form(False, 3, "removed") == (False, 3.0)                   # without a report the view is nobody's business here
    with pytest.raises(ValueError, match=r"report=True.*view='removed'"):
        windows.report_form(True, 16.0, "removed")
    for bad in (-1, -0.001, nan, float("inf"), "16", None, True):
        with pytest.raises(ValueError, match="report_edge"):
            windows.report_form(True, bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="report must be"):
            windows.report_form(bad)
