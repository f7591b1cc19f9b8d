"""The active picture on the host (no GPU): the rectangle rules, the letterbox rule on hand-made sums, the cropped stream and its inverse, and
the per-window file."""
import numpy as np
import pytest

import picture_ref as P
import yuv_ref as R
from shiftnet_amd import picture

F420 = R.Fmt(8, R.C420_CENTER, R.BT601, R.LIMITED)
F420L10 = R.Fmt(10, R.C420_LEFT, R.BT709, R.LIMITED)
F444 = R.Fmt(8, R.C444, R.BT709, R.FULL)


# ---- check_rect ---------------------------------------------------------------------------------------------------------------------------
def test_check_rect_accepts_what_the_contract_says():
    H, W = 37, 70
    for fmt in (F420, F420L10):
        for rect in [(0, 0, 70, 37), (2, 4, 40, 22), (8, 0, 62, 37), (16, 2, 10, 6), (0, 32, 70, 5), (64, 0, 6, 6)]:
            assert picture.check_rect(rect, fmt, H, W) == rect
        for rect in [(16, 2, 10, 4), (0, 36, 70, 1), (68, 0, 2, 2)]:                            # the kernels' limit, not the restorer's
            assert picture.check_rect(rect, fmt, H, W, smallest=1) == rect
        assert picture.check_rect([2, 4, 40, 22], fmt, H, W) == (2, 4, 40, 22)                  # any sequence, numpy integers included
        assert picture.check_rect(np.array([2, 4, 40, 22]), fmt, H, W) == (2, 4, 40, 22)
        assert picture.check_rect((60, 30, 10, 7), fmt, H, W) == (60, 30, 10, 7)                # odd h reaching the bottom edge
        assert picture.check_rect((0, 0, 69, 36), R.Fmt(8, R.C420_CENTER, 0, 0), 36, 69) == (0, 0, 69, 36)   # odd w reaching the right edge
    for rect in [(1, 3, 5, 7), (65, 32, 5, 5), (0, 0, 70, 37), (3, 0, 7, 9)]:                   # 4:4:4 takes any integers
        assert picture.check_rect(rect, F444, H, W) == rect
    assert picture.check_rect((69, 36, 1, 1), F444, H, W, smallest=1) == (69, 36, 1, 1)


@pytest.mark.parametrize("rect,word", [
    ((1, 4, 40, 22), "x0 and y0 must be even"), ((2, 3, 40, 22), "x0 and y0 must be even"),
    ((2, 4, 39, 22), "odd w"), ((2, 4, 40, 21), "odd h"),
    ((-2, 4, 40, 22), "inside"), ((2, 4, 70, 22), "inside"), ((2, 4, 40, 34), "inside"), ((0, 0, 72, 37), "inside"),
    ((0, 0, 0, 10), "smallest"), ((0, 0, 10, 0), "smallest"), ((0, 0, -4, 10), "smallest"), ((0, 0, 4, 10), "smallest"), ((0, 0, 10, 4), "smallest"),
    ((0, 0, 10), "integers"), ((0, 0, 10.5, 10), "integers"), ("auto", "integers"), (None, "integers"), ((0, 0, True, 10), "integers"),
])
def test_check_rect_refuses_at_420(rect, word):
    with pytest.raises(ValueError, match=word):
        picture.check_rect(rect, F420, 37, 70)


def test_the_smallest_picture_is_named_and_is_what_a_whole_frame_may_be():
    from shiftnet_amd import restore
    # a CAB's channel attention wants 2 x 2 at the coarsest level (1/4 "small", 1/8 "plus") of the frame padded to a multiple of 4 / 8
    assert picture.SMALLEST == {"small": 5, "plus": 9} and picture.MIN_SIDE == 5
    for topo, div in (("small", 4), ("plus", 8)):
        n = picture.smallest_picture(topo)
        assert restore.padded_size(n, n, topo) == (2 * div, 2 * div) and restore.padded_size(n - 1, n - 1, topo) == (div, div)
        assert picture.check_rect((0, 0, n, n), F444, 37, 70, n) == (0, 0, n, n)
        for bad in [(0, 0, n - 1, n), (0, 0, n, n - 1)]:
            with pytest.raises(ValueError, match=f"smallest picture the restorer takes is {n} x {n}"):
                picture.check_rect(bad, F444, 37, 70, n)
        _, r, c = sums(F444, 40, 40, 2, top=40 - n, left=40 - n)                                # a picture of exactly n x n is found ...
        assert picture.decide_picture(r, c, F444, 40, 40, 1.0, n) == (40 - n, 40 - n, n, n)
        _, r, c = sums(F444, 40, 40, 2, top=41 - n, left=40 - n)                                # ... one row less is the full frame
        assert picture.decide_picture(r, c, F444, 40, 40, 1.0, n) is None
    for bad in [(70, 0, 1, 1), (0, 37, 1, 1), (-1, 0, 2, 2)]:
        with pytest.raises(ValueError, match="inside"):
            picture.check_rect(bad, F444, 37, 70, smallest=1)


# ---- decide_picture -------------------------------------------------------------------------------------------------------------------------
def sums(fmt, H, W, T, top=0, bottom=0, left=0, right=0, inside=None):
    """Row and column sums of T frames: bars at the black code, the inside at ``inside`` (default: mid grey)."""
    s = 1 << (fmt.bits - 8)
    black = 0 if fmt.range == R.FULL else 16 * s
    Y = np.full((T, H, W), black, np.int64)
    Y[:, top:H - bottom, left:W - right] = 128 * s if inside is None else inside
    return Y, Y.sum(axis=2), Y.sum(axis=1)


@pytest.mark.parametrize("fmt", [F420, F420L10, F444], ids=["420", "420p10", "444"])
def test_decide_picture_on_hand_made_sums(fmt):
    H, W, T = 96, 128, 7
    _, r, c = sums(fmt, H, W, T, top=10, bottom=12)
    assert picture.decide_picture(r, c, fmt, H, W, 1.0) == (0, 10, W, H - 22)
    _, r, c = sums(fmt, H, W, T, left=16, right=14)                                            # pillarbox
    assert picture.decide_picture(r, c, fmt, H, W, 1.0) == (16, 0, W - 30, H)
    _, r, c = sums(fmt, H, W, T, top=10, bottom=12, left=16, right=14)                          # both ("windowbox")
    assert picture.decide_picture(r, c, fmt, H, W, 1.0) == (16, 10, W - 30, H - 22)
    _, r, c = sums(fmt, H, W, T, top=11, bottom=13, left=3, right=5)                            # odd bars snap inward at 4:2:0 only
    want = (3, 11, W - 8, H - 24) if fmt.chroma == R.C444 else (4, 12, W - 10, H - 26)
    assert picture.decide_picture(r, c, fmt, H, W, 1.0) == want
    assert picture.decide_picture(r.astype(np.uint32), c.astype(np.uint32), fmt, H, W, 1.0) == want     # as the device writes them
    _, r, c = sums(fmt, H, W, T)                                                                # no bars
    assert picture.decide_picture(r, c, fmt, H, W, 1.0) is None
    _, r, c = sums(fmt, H, W, T, top=H)                                                         # everything black
    assert picture.decide_picture(r, c, fmt, H, W, 1.0) is None
    _, r, c = sums(fmt, H, W, T, left=W)
    assert picture.decide_picture(r, c, fmt, H, W, 1.0) is None


def test_one_frame_of_the_window_above_the_level_ends_the_bar_there():
    fmt, H, W, T = F420, 96, 128, 7
    Y, _, _ = sums(fmt, H, W, T, top=10, bottom=12)
    Y[4, 6, :] = 40                                                                             # frame 4 has a bright row 6 inside the top bar
    assert picture.decide_picture(Y.sum(axis=2), Y.sum(axis=1), fmt, H, W, 1.0) == (0, 6, W, H - 18)
    Y[4, 6, :] = 16
    Y[2, H - 5, :64] = 20                                                                       # mean 18 > 16 + 1 in frame 2: the bottom bar ends at row H - 4
    assert picture.decide_picture(Y.sum(axis=2), Y.sum(axis=1), fmt, H, W, 1.0) == (0, 10, W, H - 14)
    assert picture.decide_picture(Y.sum(axis=2), Y.sum(axis=1), fmt, H, W, 2.0) == (0, 10, W, H - 22)   # ... unless the level allows it
    assert picture.decide_picture(Y.sum(axis=2)[:2], Y.sum(axis=1)[:2], fmt, H, W, 1.0) == (0, 10, W, H - 22)   # a window without that frame


def test_the_level_is_in_eight_bit_codes_and_compares_with_less_or_equal():
    for fmt in (F420, F420L10, F444):
        H, W, T = 32, 48, 2
        s = 1 << (fmt.bits - 8)
        black = 0 if fmt.range == R.FULL else 16 * s
        Y, _, _ = sums(fmt, H, W, T, top=4, bottom=4)
        Y[:, :4] = black + s                                                                    # exactly one 8-bit code above black: still bar
        assert picture.decide_picture(Y.sum(axis=2), Y.sum(axis=1), fmt, H, W, 1.0) == (0, 4, W, H - 8)
        Y[1, 3, 0] += 1                                                                         # one code more in one sample of one frame: not any more
        assert picture.decide_picture(Y.sum(axis=2), Y.sum(axis=1), fmt, H, W, 1.0) == ((0, 3, W, H - 7) if fmt.chroma == R.C444 else (0, 4, W, H - 8))
        assert picture.decide_picture(Y.sum(axis=2), Y.sum(axis=1), fmt, H, W, 0.0) == (0, 0, W, H - 4)     # level 0: the top bar is no bar
    with pytest.raises(ValueError, match="T >= 1"):
        picture.decide_picture(np.zeros((0, 8)), np.zeros((0, 8)), F444, 8, 8, 1.0)


def test_a_picture_that_is_black_at_its_far_edge_keeps_an_odd_edge_only_at_the_frames_edge():
    fmt, H, W, T = F420, 37, 71, 3                                                              # odd frame: the far edges may stay odd
    _, r, c = sums(fmt, H, W, T, top=4, left=6)
    assert picture.decide_picture(r, c, fmt, H, W, 1.0) == (6, 4, W - 6, H - 4)
    assert picture.check_rect((6, 4, W - 6, H - 4), fmt, H, W)
    _, r, c = sums(fmt, H, W, T, top=4, left=6, bottom=2, right=2)                              # far edges at 35 and 69: snapped down to 34 and 68
    got = picture.decide_picture(r, c, fmt, H, W, 1.0)
    assert got == (6, 4, 62, 30) and picture.check_rect(got, fmt, H, W)


# ---- crop and paste -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(36, 70), (37, 71), (37, 70), (36, 71)])
@pytest.mark.parametrize("fmt", [R.Fmt(8, R.C420_CENTER, 0, 0), R.Fmt(8, R.C420_LEFT, 0, 0), R.Fmt(8, R.C444, 0, 0), R.Fmt(10, R.C420_LEFT, 0, 0),
                                 R.Fmt(10, R.C444, 0, 0)], ids=["420jpeg", "420mpeg2", "444", "420p10", "444p10"])
def test_crop_then_paste_is_the_identity(fmt, H, W):
    rng = np.random.default_rng(H * 100 + W)
    n = R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)
    codes = rng.integers(0, 1 << fmt.bits, (3, n))
    pay = codes.astype(np.uint8) if fmt.bits == 8 else codes.astype("<u2").view(np.uint8).reshape(3, -1)
    other = np.zeros_like(pay)
    for rect in [(0, 0, W, H), (2, 4, 40, 22), (8, 0, W - 8, H), (16, 2, 10, 4), (W - (W % 2) - 2, H - (H % 2) - 2, 2 + W % 2, 2 + H % 2)]:
        picture.check_rect(rect, fmt, H, W, smallest=1)
        crop = P.crop_payloads(pay, fmt, H, W, rect)
        assert crop.shape == (3, R.frame_bytes(fmt, rect[3], rect[2]))
        assert np.array_equal(P.paste_payloads(pay, crop, fmt, H, W, rect), pay)
        back = P.paste_payloads(other, crop, fmt, H, W, rect)                                   # pasted into zeros: the crop again, zeros elsewhere
        assert np.array_equal(P.crop_payloads(back, fmt, H, W, rect), crop)
        assert int(np.count_nonzero(back)) == int(np.count_nonzero(crop))
        if rect == (0, 0, W, H):
            assert np.array_equal(crop, pay)
    Y = R.split_planes(pay[0], fmt, H, W)[0]
    r, c = P.rowcol_ref(pay, fmt, H, W)
    assert r.dtype == np.uint32 and r.shape == (3, H) and c.shape == (3, W) and int(r[0].sum()) == int(c[0].sum()) == int(Y.sum())


# ---- the file -------------------------------------------------------------------------------------------------------------------------------
def test_file_round_trip_and_malformed_lines_name_their_line(tmp_path):
    rects = [(0, 12, 128, 72), None, (16, 0, 96, 96), (0, 12, 128, 72)]
    path = tmp_path / "pictures.txt"
    picture.write_pictures(path, rects, "auto")
    text = path.read_text()
    assert text.startswith("#") and "4 windows" in text and "auto" in text.splitlines()[0]
    assert picture.read_pictures(path) == rects
    assert picture.parse_pictures("# nothing\n\n  0 12 128 72  # the film\nfull\n") == [(0, 12, 128, 72), None]
    assert picture.parse_pictures("") == []
    for bad, no in [("0 12 128 72\n0 12 128\n", 2), ("# c\n\n0 12 128 x\n", 3), ("0 12 128 72 5\n", 1), ("0:12:128:72\n", 1), ("0 12 0 72\n", 1),
                    ("full\n-2 12 128 72\n", 2), ("0 12 128 7.5\n", 1)]:
        with pytest.raises(ValueError, match=f"line {no}:"):
            picture.parse_pictures(bad)
    with pytest.raises(ValueError, match="inside"):                                             # the stream is known later: check_pictures judges the fit
        picture.check_pictures(picture.parse_pictures("0 12 128 100\n"), F420, 96, 128)
    assert picture.check_pictures(rects, F420, 96, 128) == rects


def test_the_command_line_words():
    from shiftnet_amd import restore
    assert restore.picture_arg("full") is None and restore.picture_arg("auto") == "auto"
    assert restore.picture_arg("0:138:1920:804") == (0, 138, 1920, 804)
    assert restore.picture_arg("bars.txt") == "bars.txt" and restore.picture_arg("1:2:3") == "1:2:3"
    a = restore.make_parser().parse_args(["--variant", "deblur", "--checkpoint", "synthetic", "in.y4m", "out.y4m"])
    assert a.picture == "full" and a.bar_level == 1.0 and a.picture_out is None


def test_per_window_list_of_pictures_running_short_names_the_window():
    from shiftnet_amd import restore
    rects = [(0, 12, 128, 72), None]
    mode, listed = restore.picture_form(rects)
    assert mode == "list" and listed == rects
    assert restore.picture_form((0, 12, 128, 72)) == ("fixed", (0, 12, 128, 72)) and restore.picture_form([rects[0]] * 4)[0] == "list"
    pics = restore.PerWindow("picture", picture.check_pictures(listed, F420, 96, 128), True)
    assert pics.at(0) == rects[0] and pics.at(1) is None
    with pytest.raises(ValueError, match="picture lists 2 windows, window 2 has no entry"):
        pics.at(2)
    one = restore.PerWindow("picture", [rects[0]], True)
    with pytest.raises(ValueError, match="picture lists 1 window, window 1 has no entry"):
        one.at(1)
    vr = restore.VideoRestorer.__new__(restore.VideoRestorer)                                   # the stager's count of the windows it has taken on
    vr.picture_mode, vr._pics, vr.run = mode, pics, restore._Run()
    assert vr._window_picture() == rects[0] and vr._window_picture() is None
    with pytest.raises(ValueError, match="window 2"):
        vr._window_picture()
    assert vr.run.staged == 2 and vr.run.window_picture == []
