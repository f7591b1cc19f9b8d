"""CPU tests of the pure parts of the restorer's windows that overlap in time: windows.plan_overlap_windows against the frame-by-frame restatement of
tests/time_ref.py, the properties the plan promises, the cross-fade's weights, the streaming source with the overlap, the accepted forms of
``window_overlap`` in Python and on the command line, and the new symbol in header, build list and library."""
import itertools
import os
import re

import numpy as np
import pytest

import time_ref as TR
from shiftnet_amd import restore_cli, scenes, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases(n_max=40, len_max=9):
    for L in range(1, len_max + 1):
        for V in range(0, L // 2 + 1):
            for n in range(1, n_max + 1):
                yield n, L, V


def test_the_planner_equals_the_restatement():
    for n, L, V in cases():
        assert windows.plan_overlap_windows(n, L, V) == TR.plan(n, L, V), (n, L, V)
    assert windows.plan_overlap_windows(11, 4, 2) == [(0, 4, [2, 1, 0, 1, 2, 3, 4, 5], 0, 2), (2, 4, [0, 1, 2, 3, 4, 5, 6, 7], 2, 2),
                                                      (4, 4, [2, 3, 4, 5, 6, 7, 8, 9], 2, 2), (6, 4, [4, 5, 6, 7, 8, 9, 10, 9], 2, 2),
                                                      (8, 3, [6, 7, 8, 9, 10, 9, 8], 2, 3)]


def test_every_frame_is_written_once_and_in_order_and_covered_by_at_most_two_windows():
    for n, L, V in cases():
        plan = windows.plan_overlap_windows(n, L, V)
        written, cover = [], [0] * n
        for k, (lo, cnt, idx, head, wr) in enumerate(plan):
            last = k == len(plan) - 1
            assert head == (V if k else 0) and wr == (cnt if last else cnt - V) and 1 <= wr <= cnt <= L, (n, L, V, k)
            assert (lo + cnt == n) == last, (n, L, V, k)
            assert len(idx) == cnt + windows.PAST + windows.FUTURE and idx[windows.PAST:windows.PAST + cnt] == list(range(lo, lo + cnt)), (n, L, V, k)
            if k:
                plo, pcnt = plan[k - 1][:2]
                assert cnt >= V + 1 and lo == plo + pcnt - V, (n, L, V, k)              # the shared frames are the predecessor's last V
            written += list(range(lo, lo + wr))                                     # a prefix of its frames
            for f in range(lo, lo + cnt):
                cover[f] += 1
        assert written == list(range(n)), (n, L, V)
        assert max(cover) <= 2 and min(cover) >= 1, (n, L, V)
        assert sum(c == 2 for c in cover) == V * (len(plan) - 1), (n, L, V)


def test_no_overlap_is_todays_plan_and_scenes_restart_the_overlap():
    for n, L, _ in cases(n_max=30):
        assert [w[:3] for w in windows.plan_overlap_windows(n, L, 0)] == windows.plan_windows(n, L), (n, L)
        assert all(w[3] == 0 and w[4] == w[1] for w in windows.plan_overlap_windows(n, L, 0))
        for cuts in ([], [1], [5], [3, 4], [4, 8, 29]):
            assert [w[:3] for w in windows.plan_scene_overlap_windows(n, L, cuts, 0)] == windows.plan_scene_windows(n, L, cuts), (n, L, cuts)
    for n, L, V in cases(n_max=30, len_max=6):
        for cuts in ([5], [3, 4], [4, 8, 29], [40]):
            plan = windows.plan_scene_overlap_windows(n, L, cuts, V)
            assert plan == TR.scene_plan(n, L, cuts, V), (n, L, V, cuts)
            starts = [0] + [c for c in cuts if c < n]
            for lo, cnt, idx, head, wr in plan:
                a = max(s for s in starts if s <= lo)
                b = min([s for s in starts if s > lo] + [n])
                assert head == (0 if lo == a else V) and lo + cnt <= b and all(a <= i < b for i in idx), (n, L, V, cuts)      # nothing crosses a scene start
            assert [f for lo, _, _, _, wr in plan for f in range(lo, lo + wr)] == list(range(n))
    assert windows.plan_scene_overlap_windows(11, 4, [5], 2) == [(0, 4, [2, 1, 0, 1, 2, 3, 4, 3], 0, 2), (2, 3, [0, 1, 2, 3, 4, 3, 2], 2, 3),
                                                                 (5, 4, [7, 6, 5, 6, 7, 8, 9, 10], 0, 2), (7, 4, [5, 6, 7, 8, 9, 10, 9, 8], 2, 4)]


def test_the_weights_are_the_ramp_of_two_tiles_that_overlap_by_v():
    for L in range(2, 25):
        for V in range(1, L // 2 + 1):
            old, new = windows.overlap_weights(V)
            assert old.dtype == new.dtype == np.float32 and old.shape == new.shape == (V,)
            origins, w = windows.tile_axis(2 * L - V, L, V)
            assert origins == [0, L - V] and w.shape == (2, L)
            assert np.array_equal(w[0, L - V:].astype(np.float32), old) and np.array_equal(w[1, :V].astype(np.float32), new), (L, V)
            ref_old, ref_new = TR.weights(V)
            assert np.array_equal(old, ref_old) and np.array_equal(new, ref_new)
            assert np.array_equal(old, new[::-1])
            assert np.abs(old.astype(np.float64) + new.astype(np.float64) - 1.0).max() <= 2.0 ** -24
    old, new = windows.overlap_weights(0)
    assert old.shape == new.shape == (0,)
    assert [float(v) for v in windows.overlap_weights(1)[1]] == [0.5] and [float(v) for v in windows.overlap_weights(3)[0]] == [0.75, 0.5, 0.25]


class _LateCuts:
    """A decider that knows the cuts but releases the decision for frame t only once frame t + 3 has been fed or the stream has ended."""
    lookahead = 3

    def __init__(self, cuts):
        self.cuts, self.fed, self.ended = set(cuts), [], False

    @property
    def decided(self):
        return len(self.fed) if self.ended else max(0, len(self.fed) - 3)

    def feed(self, frames):
        assert not self.ended
        self.fed += [int(f[0]) for f in frames]

    def finish(self):
        assert not self.ended
        self.ended = True

    def is_cut(self, t):
        assert t < self.decided, (t, self.decided)
        return t in self.cuts


def _drain(src, L, V, lookahead):
    got, k = [], 0
    while True:
        w = src.window(k, L, V)
        if w is None:
            return got
        got.append((w[0], w[1], [int(f[0]) for f in w[2]], src.head, src.written))
        assert len(src.buf) <= L + windows.PAST + windows.FUTURE + lookahead + 1 + V, (len(src.buf), L, V)      # the documented bound plus V
        k += 1


CUT_SETS = [[], [1], [4], [5], [3, 4], [2, 9, 10, 17], [8, 24, 32, 40]]


def test_the_streaming_source_hands_out_the_planned_windows_for_listed_and_for_late_decisions():
    clip_los = []
    for n, L, cuts in itertools.product((1, 2, 3, 5, 8, 9, 11, 26, 33), (2, 4, 5, 9), CUT_SETS):
        for V in range(0, L // 2 + 1):
            frames = [np.array([i]) for i in range(n)]
            want = windows.plan_scene_overlap_windows(n, L, cuts, V)
            listed = windows._SceneFrames(iter(frames), scenes.ListedCuts(cuts))
            assert _drain(listed, L, V, 0) == want, (n, L, V, cuts)
            assert listed.cuts == [c for c in cuts if c < n]
            late = _LateCuts(cuts)
            src = windows._SceneFrames(iter(frames), late)
            assert _drain(src, L, V, 3) == want, (n, L, V, cuts)
            assert late.fed == list(range(n)) and late.ended and src.cuts == [c for c in cuts if c < n]      # every frame fed once, in order
    # the frame number handed to the dither is that of the window's first written frame, counted in its scene
    src = windows._SceneFrames(iter([np.array([i]) for i in range(11)]), scenes.ListedCuts([5]))
    for k, _, clip_lo in src.windows(4, 2):
        clip_los.append((clip_lo, src.head, src.written))
    assert clip_los == [(0, 0, 2), (2, 2, 3), (0, 0, 2), (2, 2, 4)]
    # the default is no overlap: the three-field windows of before
    src = windows._Frames(iter([np.array([i]) for i in range(6)]))
    assert [(k, [int(f[0]) for f in w], c) for k, w, c in src.windows(4)] == [(0, [2, 1, 0, 1, 2, 3, 4, 5], 0), (1, [2, 3, 4, 5, 4, 3], 4)]


@pytest.mark.parametrize("bad,one_len", [(-1, 4), (3, 4), (3, 5), (1, 1), (2.0, 8), (1.5, 8), ("2", 8), (None, 8), (True, 8), ([1], 8)])
def test_illegal_overlaps_are_value_errors(bad, one_len):
    with pytest.raises(ValueError, match="window_overlap"):
        windows.window_overlap_form(bad, one_len)
    if isinstance(bad, int) and not isinstance(bad, bool):
        with pytest.raises(ValueError, match="window_overlap"):
            windows.plan_overlap_windows(10, one_len, bad)


def test_legal_overlaps_and_the_seam_file():
    assert windows.window_overlap_form(0, 1) == 0 and windows.window_overlap_form(2, 4) == 2 and windows.window_overlap_form(np.int64(8), 16) == 8
    assert windows.window_overlap_form(2, 5) == 2 and type(windows.window_overlap_form(np.int32(1), 2)) is int
    seams = [None, [0.1, 1.0 / 3.0], [2.5e-7, 123.456], None]
    assert windows.parse_seams(windows.format_seams(seams)) == seams
    assert windows.parse_seams("# c\n-\n\n0.5 0.25 # two\n") == [None, [0.5, 0.25]] and windows.parse_seams(windows.format_seams([])) == []


def test_the_command_line_takes_the_overlap_and_refuses_what_the_restorer_refuses(capsys):
    ap = restore_cli.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["--window_overlap", "2", "--seams_out", "s.txt", "in.y4m", "out.y4m"])
    assert a.window_overlap == 2 and a.seams_out == "s.txt"
    a = ap.parse_args(base + ["in.y4m", "out.y4m"])
    assert a.window_overlap == 0 and a.seams_out is None
    for bad in (["--window_overlap", "half"], ["--window_overlap", "1.5"], ["--window_overlap"]):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(base + bad + ["in.y4m", "out.y4m"])
        assert e.value.code == 2
    capsys.readouterr()
    # judged by main() before any file is opened: the files named here do not exist
    missing = ["/nonexistent/in.y4m", "/nonexistent/out.y4m"]
    for bad, word in ((["--window_overlap", "-1"], ">= 0"), (["--one_len", "4", "--window_overlap", "3"], "half of one_len"),
                      (["--window_overlap", "9"], "half of one_len"), (["--one_len", "5", "--window_overlap", "3"], "half of one_len")):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(base + bad + missing)
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "--window_overlap" in err and word in err, (bad, err)


def test_header_build_list_and_library_have_the_new_symbol_and_the_abi_version_stays_20():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_time.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_time.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^int sn_time_crossfade\(const float\* prev, float\* cur, const float\* w_prev, const float\* w_cur,\s+"
                     r"unsigned long long\* sq(?:\s*/\*[^*]*\*/)?,\s+int V, int C, int Hp, int Wp, int h, int w, void\* stream\);", header, flags=re.M)
    assert hasattr(lib, "sn_time_crossfade") and "sn_time_crossfade" in L.SYMBOLS
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    assert len(lib.sn_time_crossfade.argtypes) == 12
    # the argument checks are host side and need no GPU: host memory is refused before anything would read it
    arr = np.zeros(4096, np.float32)
    buf = arr.ctypes.data
    p, c, a, b, sq = buf, buf + 4096, buf + 8192, buf + 8448, buf + 12288

    def call(pp=p, cp=c, ap=a, bp=b, sp=sq, V=2, C=3, Hp=8, Wp=8, h=8, w=8):
        return lib.sn_time_crossfade(pp, cp, ap, bp, sp, V, C, Hp, Wp, h, w, None)
    for kw in ({"pp": None}, {"cp": None}, {"ap": None}, {"bp": None},                                       # a null pointer (sq may be null)
               {"pp": p + 2}, {"cp": c + 1}, {"ap": a + 3}, {"bp": b + 2}, {"sp": sq + 4}, {"sp": sq + 1},        # 4-byte alignment; 8 for sq
               {"V": 0}, {"C": 0}, {"Hp": 0}, {"Wp": 0}, {"V": -1}, {"Wp": -8},                                # a size below 1
               {"h": 0}, {"w": 0}, {"h": 9}, {"w": 9}, {"h": -1},                                              # a picture outside the plane
               {"V": 21846, "C": 3}, {"V": 65536, "C": 1}, {"V": 2 ** 16, "C": 2 ** 16},                       # V * C > 65535 (the last: a product past 2^31)
               {"Hp": 8192, "Wp": 4097, "h": 8192, "w": 4097}, {"Hp": 2 ** 16, "Wp": 2 ** 16, "h": 2 ** 16, "w": 2 ** 16},      # with sq: h * w > 2^25
               {"sp": None, "pp": None}, {"sp": None, "h": 9}):
        assert call(**kw) == -22, kw
