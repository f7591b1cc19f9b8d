"""The report's temporal correlation along block motion without a GPU: the ABI of ``sn_yuv_diff_stats_mv``, its numpy restatement
(tests/diff_stats_mv_ref.py) on a case worked out by hand and against the restatement of ``sn_yuv_diff_stats``, the host arithmetic of
shiftnet_amd/report.py, the claim the option rests on -- on a panning clip removed co-moving texture reads as correlated along the vectors and as
uncorrelated at the same place, removed noise as uncorrelated both ways -- on the restatement alone, the report file with and without the motion
columns, and the option forms of the restorer and its CLI."""
import math
import os

import numpy as np
import pytest

import diff_stats_mv_ref as DM
import diff_stats_ref as D
import motion_ref as M
import yuv_ref as R
from shiftnet_amd import report, restore_cli, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
nan = float("nan")


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_symbol_the_library_exports_it_and_the_abi_version_stays():
    from shiftnet_amd import lib as L
    lib = L.load()
    assert hasattr(lib, "sn_yuv_diff_stats_mv") and "sn_yuv_diff_stats_mv" in L.SYMBOLS
    assert L.SN_DIFF_STATS_MV == 8 == DM.WORDS == len(report.SUMS_MV)
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20
    with open(os.path.join(ROOT, "include", "shiftnet_hip.h")) as fh:
        header = fh.read()
    assert "#define SN_ABI_VERSION 20 " in header and "#define SN_DIFF_STATS_MV 8\n" in header and "#define SN_DIFF_STATS 16\n" in header
    assert ("int sn_yuv_diff_stats_mv(const uint8_t* a, const uint8_t* b, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */,\n"
            "                         const int8_t* mv, int64_t* dst /* [T - 1][SN_DIFF_STATS_MV] */, int T, int H, int W, void* stream);") in header


# ---- a case small enough for paper --------------------------------------------------------------------------------------------------------
# A 4 x 6 picture: 2 x 3 blocks in one vector block with the vector (0, 2).  Blocks (0, 1), (1, 0) and (1, 2) measure; (1, 2) would be read at columns
# 6, 7 and does not count.  a0 = 0 and b0 = 6 y + x, so d0 = 6 y + x; a1 = 1 and b1 = x, so d1 = x + 2 - 1 at the displaced place; g = (x + 2) - (6 y + x).
#   block (0, 1), samples (0, 2) (0, 3) (1, 2) (1, 3): d0 = 2 3 8 9,     d1 = 3 4 3 4, g = 2 2 -4 -4
#   block (1, 0), samples (2, 0) (2, 1) (3, 0) (3, 1): d0 = 12 13 18 19, d1 = 1 2 1 2, g = -10 -10 -16 -16
HAND = [8, 84, 4 + 9 + 64 + 81 + 144 + 169 + 324 + 361, 20, 9 + 16 + 9 + 16 + 1 + 4 + 1 + 4, 6 + 12 + 24 + 36 + 12 + 26 + 18 + 38,
        4 + 4 + 16 + 16 + 100 + 100 + 256 + 256, 8]


def _hand_planes():
    y, x = np.mgrid[0:4, 0:6]
    return np.zeros((4, 6), np.int64), 6 * y + x, np.ones((4, 6), np.int64), x + 0 * y


def test_the_numpy_restatement_gives_the_hand_sums_of_a_4_x_6_picture():
    a0, b0, a1, b1 = _hand_planes()
    assert HAND == [8, 84, 1156, 20, 60, 172, 752, 8]
    assert DM.sums_of_pair(a0, b0, a1, b1, np.array([[[0, 2]]], np.int8)) == HAND
    zero = DM.sums_of_pair(a0, b0, a1, b1, np.zeros((1, 1, 2), np.int8))              # all three measuring blocks count and none has moved
    assert zero[0] == 12 and zero[7] == 0 and zero[1] == 84 + 16 + 17 + 22 + 23
    assert DM.sums_of_pair(a0, b0, a1, b1, np.array([[[-128, 127]]], np.int8)) == [0] * 8      # every block pushed out
    assert DM.sums_of_pair(a0, b0, a1, b1, np.array([[[1, 0]]], np.int8))[0] == 4     # rows 3, 4 do not exist: only block (0, 1) counts
    assert DM.sums_of_pair(a0[:1], b0[:1], a1[:1], b1[:1], np.zeros((0, 0, 2), np.int8)) == [0] * 8      # no whole block
    # through the payload form, with a rectangle: the same picture inside a larger 4:4:4 frame
    fmt = R.Fmt(8, R.C444, R.BT601, R.FULL)
    H, W, rect = 7, 9, (2, 1, 6, 4)
    pay = np.zeros((2, 2, R.frame_bytes(fmt, H, W)), np.uint8)                        # [a | b][payload]
    for k, plane in enumerate((a0, a1)):
        Y = np.full((H, W), 77, np.uint8)
        Y[1:5, 2:8] = plane
        pay[0, k, :H * W] = Y.reshape(-1)
    for k, plane in enumerate((b0, b1)):
        Y = np.full((H, W), 200, np.uint8)
        Y[1:5, 2:8] = plane
        pay[1, k, :H * W] = Y.reshape(-1)
    assert [list(r) for r in DM.diff_stats_mv_ref(pay[0], pay[1], np.array([[[[0, 2]]]], np.int8), fmt, H, W, rect=rect)] == [HAND]


@pytest.mark.parametrize("bits", [8, 10])
def test_all_blocks_and_zero_vectors_give_the_words_of_the_plain_restatement(bits):
    fmt = R.Fmt(bits, R.C420_CENTER, R.BT709, R.LIMITED)
    h, w, T = 22, 36, 3
    rng = np.random.default_rng(bits)
    n = R.frame_bytes(fmt, h, w) // (1 if bits == 8 else 2)
    top = 255 if bits == 8 else 65535                                                 # samples are taken as stored
    a, b = (rng.integers(0, top + 1, (T, n)) for _ in range(2))
    as_bytes = (lambda p: p.astype(np.uint8)) if bits == 8 else (lambda p: p.astype("<u2").view(np.uint8).reshape(T, -1))
    a, b = as_bytes(a), as_bytes(b)
    mv = np.zeros((T - 1,) + M.grid(h, w) + (2,), np.int8)
    got = DM.diff_stats_mv_ref(a, b, mv, fmt, h, w, split=False)
    plain = D.diff_stats_ref(a, b, fmt, h, w)
    for p in range(T - 1):
        assert got[p, 0] == h * w and got[p, 7] == 0
        assert list(got[p, [1, 2, 5]]) == list(plain[p, [1, 2, 7]])                   # S1, S2, St of payload p
        assert list(got[p, [3, 4]]) == list(plain[p + 1, [1, 2]])                     # S1, S2 of payload p + 1
    half = DM.diff_stats_mv_ref(a, b, mv, fmt, h, w)
    assert (half[:, 0] == 4 * ((h // 2) * (w // 2) // 2)).all() and (half[:, 2] < got[:, 2]).all()


# ---- the host arithmetic ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
def test_pair_measures_of_the_hand_sums_and_every_nan_case(bits):
    c = 1 << (bits - 8)
    r = report.pair_measures_mv(HAND, bits, 4, 6)
    assert r.rho_t_mv == (8 * 172 - 84 * 20) / math.sqrt((8 * 1156 - 84 * 84) * (8 * 60 - 20 * 20))
    assert r.mv_match_rms == math.sqrt(752 / 8) / c and r.mv_moved == 1.0 and r.mv_counted == 8 / 24
    assert report.pair_measures_mv(np.array(HAND, np.int64), bits, 4, 6) == r
    none = report.pair_measures_mv([0] * 8, bits, 4, 6)                               # nothing counted
    assert math.isnan(none.rho_t_mv) and math.isnan(none.mv_match_rms) and math.isnan(none.mv_moved) and none.mv_counted == 0.0
    flat0 = report.pair_measures_mv([4, 8, 16, 3, 5, 6, 0, 0], bits, 2, 4)            # d0 = 2 everywhere: no variance in the first frame
    assert math.isnan(flat0.rho_t_mv) and flat0.mv_match_rms == 0.0 and flat0.mv_moved == 0.0 and flat0.mv_counted == 0.5
    flat1 = report.pair_measures_mv([4, 3, 5, -8, 16, -6, 4, 4], bits, 2, 4)          # d1 = -2 everywhere: none in the second
    assert math.isnan(flat1.rho_t_mv) and flat1.mv_match_rms == 1.0 / c and flat1.mv_moved == 1.0
    same = report.pair_measures_mv([4, 2, 6, 2, 6, 6, 0, 0], bits, 2, 4)              # d1 = d0
    assert same.rho_t_mv == 1.0
    assert report.pair_measures_mv(None, bits, 4, 6) == report.MotionReport()
    assert all(math.isnan(getattr(report.MotionReport(), k)) for k in report.COLUMNS_MV)
    with pytest.raises(ValueError, match="8 words"):
        report.pair_measures_mv([0] * 16, bits, 4, 6)
    got = report.frames_report_motion([HAND, None, [0] * 8], bits, [(4, 6)] * 3)
    assert got == [r, report.MotionReport(), none] and got[0] != got[1]
    med = report.summarize_motion(got)
    assert med["rho_t_mv"] == r.rho_t_mv and med["mv_counted"] == (8 / 24) / 2 and list(med) == list(report.COLUMNS_MV)
    assert "rho_t_mv" in report.summary_line_motion(med)
    assert all(math.isnan(v) for v in report.summarize_motion([]).values())


# ---- the claim: a pan hides removed detail from rho_t and not from rho_t_mv -----------------------------------------------------------------
SIZES = [(64, 96), (70, 98)]
PANS = [(3, -2), (-7, 7), (1, 0), (0, 0)]
SEED = 20261019


def _pan(canvas, t, v, h, w):
    """The h x w picture of frame t: the canvas seen through a window that moves by -v per frame, so the content moves by v = (vy, vx)."""
    y0, x0 = 16 - t * v[0], 16 - t * v[1]
    return canvas[y0:y0 + h, x0:x0 + w]


def _clip(h, w, v, what, seed):
    """Two frames of (input, written) luma planes: the written picture is white random codes 40 .. 215 panning by v; the input is the written
    picture plus what was removed -- a +-20 code texture that moves with it, or noise of its own in every frame."""
    rng = np.random.default_rng(seed)
    pic = rng.integers(40, 216, (h + 32, w + 32))
    tex = rng.integers(-20, 21, (h + 32, w + 32))
    b = [_pan(pic, t, v, h, w) for t in (0, 1)]
    if what == "texture":
        a = [b[t] + _pan(tex, t, v, h, w) for t in (0, 1)]
    else:
        a = [b[t] + rng.integers(-20, 21, (h, w)) for t in (0, 1)]
    return a, b


def _plain_rho(a, b):
    d = [b[t] - a[t] for t in (0, 1)]
    z = np.zeros((1, 1), np.int64)
    rows = [D.sums_of_planes(d[0], b[0], z, z, 0, d[1]), D.sums_of_planes(d[1], b[1], z, z, 0, None)]
    return report.pair_rho(rows[0], rows[1])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("v", PANS, ids=lambda v: f"pan{v[0]},{v[1]}")
def test_removed_texture_that_pans_reads_correlated_along_the_vectors_only_and_noise_never(size, v):
    h, w = size
    a, b = _clip(h, w, v, "texture", SEED)
    mv, _ = M.motion_pair(b[0], b[1])                                                 # the vectors of the written picture, found on the matching blocks
    sums = DM.sums_of_pair(a[0], b[0], a[1], b[1], mv)
    r = report.pair_measures_mv(sums, 8, h, w)
    plain = _plain_rho(a, b)
    print(f"texture {size} pan {v}: rho_t_mv {r.rho_t_mv:.4f} rho_t {plain:.4f} match {r.mv_match_rms:.3f} moved {r.mv_moved:.3f} counted {r.mv_counted:.3f}")
    i, j = np.mgrid[0:h // 2, 0:w // 2]
    vec = mv.astype(np.int64)[i // 8, j // 8]
    ok = ((i + j) & 1 == 1) & (2 * i + vec[..., 0] >= 0) & (2 * i + vec[..., 0] + 2 <= h) & (2 * j + vec[..., 1] >= 0) & (2 * j + vec[..., 1] + 2 <= w)
    assert sums[0] == 4 * int(ok.sum()) and sums[7] == 4 * int((ok & (vec != 0).any(axis=-1)).sum())
    assert r.mv_moved == sums[7] / sums[0] and r.mv_counted == sums[0] / (h * w)
    if v == (0, 0):
        assert r.rho_t_mv >= 0.999 and plain >= 0.999                                 # static: both see the removed texture
        assert (mv == 0).all() and r.mv_match_rms == 0.0 and r.mv_moved == 0.0        # every counted block has the true vector
    else:
        assert r.rho_t_mv >= 0.5 and abs(plain) <= 0.05                               # the pan hides it from the plain measure alone
        assert r.mv_moved > 0.5
    a, b = _clip(h, w, v, "noise", SEED)
    n = report.pair_measures_mv(DM.sums_of_pair(a[0], b[0], a[1], b[1], M.motion_pair(b[0], b[1])[0]), 8, h, w)
    print(f"noise   {size} pan {v}: rho_t_mv {n.rho_t_mv:.4f} rho_t {_plain_rho(a, b):.4f}")
    assert abs(n.rho_t_mv) <= 0.05 and abs(_plain_rho(a, b)) <= 0.05


# ---- the file -----------------------------------------------------------------------------------------------------------------------------
def _frames(n=6):
    rng = np.random.default_rng(3)
    frames = [report.FrameReport(i, i // 3, None if i < 3 else 7.5, *[float(x) for x in rng.normal(0.0, 1.0, len(report.MEASURES))]) for i in range(n)]
    frames[2].rho_t = frames[5].rho_t = nan
    motion = [report.MotionReport(*[float(x) for x in rng.normal(0.0, 1.0, 4)]) for _ in range(n)]
    motion[2] = motion[5] = report.MotionReport()
    motion[4].rho_t_mv = nan
    motion[1].mv_counted = 1.0 / 3.0
    return frames, motion


def test_the_report_file_without_motion_is_what_it_was_and_with_motion_reads_back_through_both_parsers():
    frames, motion = _frames()
    plain = report.format_report(frames, "edge 16")
    med = report.summarize(frames)
    want = ["# method noise: written minus input, one line per written frame (edge 16)",
            "# m, var: luma codes of the format written; sigma, removed_sigma: 8-bit R'G'B' codes; mean_*, rms_*: 8-bit codes; rho_t: to the next frame",
            "# " + " ".join(report.COLUMNS)]
    want += [" ".join(report._word(getattr(f, c)) for c in report.COLUMNS) for f in frames]
    want.append("# median - - - " + " ".join(report._word(med[c]) for c in report.MEASURES))
    assert plain == "\n".join(want) + "\n" and report.format_report(frames, "edge 16", None) == plain
    assert report.parse_report(plain) == frames and report.parse_report_motion(plain) == [None] * len(frames)
    text = report.format_report(frames, "edge 16", motion)
    lines = text.splitlines()
    cols = [ln for ln in lines if ln.startswith("# frame ")]
    assert cols == ["# " + " ".join(report.COLUMNS + report.COLUMNS_MV)] and report.COLUMNS_MV == ("rho_t_mv", "mv_match_rms", "mv_moved", "mv_counted")
    body = [ln for ln in lines if not ln.startswith("#")]
    assert len(body) == len(frames) and all(len(ln.split()) == len(report.COLUMNS) + 4 for ln in body)
    assert [ln.rsplit(" ", 4)[0] for ln in body] == [ln for ln in plain.splitlines() if not ln.startswith("#")]      # the frame columns are untouched
    assert report.parse_report(text) == frames and report.parse_report_motion(text) == motion
    assert report.parse_report_motion(text)[2] == report.MotionReport() and body[2].endswith(" nan nan nan nan")
    last = lines[-1].split()
    assert lines[-1].startswith("# median - - - ") and len(last) == 5 + len(report.MEASURES) + 4
    mmed = report.summarize_motion(motion)
    assert [float(x) for x in last[-4:]] == pytest.approx([mmed[c] for c in report.COLUMNS_MV], nan_ok=True, rel=0, abs=0)
    assert [float(x) for x in last[5:-4]] == pytest.approx(list(med.values()), nan_ok=True, rel=0, abs=0)
    with pytest.raises(ValueError, match="motion"):
        report.format_report(frames, "", motion[:-1])
    for words in (-5, -3, -1, 1, 2, 5):                                               # a line of any other width, with its number
        bad = text.replace(body[1], body[1] + " 0.5" * words if words > 0 else body[1].rsplit(" ", -words)[0])
        with pytest.raises(ValueError, match=f"line {lines.index(body[1]) + 1}:"):
            report.parse_report(bad)
        with pytest.raises(ValueError, match=f"line {lines.index(body[1]) + 1}:"):
            report.parse_report_motion(bad)
    with pytest.raises(ValueError, match="line 1"):
        report.parse_report_motion(" ".join(["x"] * (len(report.COLUMNS) + 4)))


# ---- the options ----------------------------------------------------------------------------------------------------------------------------
BASE = ["--variant", "denoise_small", "--checkpoint", "synthetic", "--sigma", "10", "in.y4m", "out.y4m"]


def test_the_option_form_needs_the_report_and_refuses_other_words():
    assert windows.report_motion_form() is None and windows.report_motion_form(None, False) is None and windows.report_motion_form(None, True) is None
    assert windows.report_motion_form("blocks", True) == "blocks"
    with pytest.raises(ValueError, match="needs report=True"):
        windows.report_motion_form("blocks")
    with pytest.raises(ValueError, match="needs report=True"):
        windows.report_motion_form("blocks", False)
    for bad in ("none", "block", "", True, 1, ("blocks",)):
        with pytest.raises(ValueError, match="report_motion must be"):
            windows.report_motion_form(bad, True)
    assert windows.report_form() == (False, 16.0) and len(windows.report_form(True, 4)) == 2      # its signature and its 2-tuple stay


def test_the_parser_takes_the_option_and_the_cli_refuses_it_without_the_report(capsys):
    ap = restore_cli.make_parser()
    assert ap.parse_args(BASE).report_motion == "none"
    a = ap.parse_args(["--report", "r.txt", "--report_motion", "blocks"] + BASE)
    assert a.report_motion == "blocks" and a.report == "r.txt"
    for bad in ("auto", "Blocks", ""):
        with pytest.raises(SystemExit):
            ap.parse_args(["--report", "r.txt", "--report_motion", bad] + BASE)
        assert "--report_motion" in capsys.readouterr().err
    assert not os.path.exists("in.y4m")
    with pytest.raises(SystemExit):                                                   # judged before the input is opened or a device is touched
        restore_cli.main(["--report_motion", "blocks"] + BASE)
    err = capsys.readouterr().err
    assert "--report_motion blocks needs --report" in err
    assert not os.path.exists("out.y4m")
