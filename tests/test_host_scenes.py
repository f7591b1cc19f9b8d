"""CPU: the scene-cut rule (shiftnet_amd/scenes.py), the scene-aware window planner and frame source of the video restorer, the cut-list
format and the command line; and that the library exports ``sn_yuv_thumb`` without an ABI bump.  No tolerance anywhere: integers and lists."""
import importlib.util
import itertools
import os

import numpy as np
import pytest

import scene_ref as S
import yuv_ref as R
from shiftnet_amd import restore, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(90, 130), (144, 176), (270, 480)]                  # 90 x 130: partial blocks on both edges


def measure_of(rgb, h, w):
    """m of a clip, with the luma taken from the Y plane that yuv_ref.egress_emu writes (BT.601 limited, 4:2:0)."""
    return scenes.cut_measure(S.thumb_ref(S.payloads_of(rgb, h, w), S.FMT420, h, w), h, w, 8)


# ---- 1. the library ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_sn_yuv_thumb_and_keeps_the_abi_version():
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()                                              # hipcc cross-compiles gfx950 without a GPU
    from shiftnet_amd import lib as L
    lib = L.load()
    assert hasattr(lib, "sn_yuv_thumb") and "sn_yuv_thumb" in L.SYMBOLS
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20
    with open(os.path.join(ROOT, "include", "shiftnet_hip.h")) as fh:
        assert "int sn_yuv_thumb(const uint8_t* src, const sn_yuv_fmt* fmt, uint16_t* dst, int T, int H, int W, void* stream);" in fh.read()


def test_scenes_module_does_not_import_torch():
    import subprocess
    import sys
    code = "import sys; import shiftnet_amd.scenes; sys.exit(1 if 'torch' in sys.modules else 0)"
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "shift-net_amd"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- 2. the rule on the clip it was checked on ------------------------------------------------------------------------------------------
def test_thumbnail_and_measure_restatements_agree_on_small_cases():
    rng = np.random.default_rng(0)
    for bits, (h, w) in itertools.product((8, 10), ((1, 1), (8, 8), (9, 17), (67, 101))):
        fmt = R.Fmt(bits, R.C420_LEFT, R.BT709, R.FULL)
        n = R.frame_bytes(fmt, h, w) // (1 if bits == 8 else 2)
        p = rng.integers(0, 1 << bits, (3, n))
        p = p.astype(np.uint8) if bits == 8 else p.astype("<u2").view(np.uint8).reshape(3, -1)
        th = S.thumb_ref(p, fmt, h, w)
        assert th.shape == (3, (h + 7) // 8, (w + 7) // 8) and th.dtype == np.uint16
        Y = [R.split_planes(q, fmt, h, w)[0] for q in p]
        assert all(int(th[t].astype(np.int64).sum()) == int(Y[t].sum()) for t in range(3))          # every pixel counted once, nothing else
        assert int(th[1, -1, -1]) == int(Y[1][(h - 1) // 8 * 8:, (w - 1) // 8 * 8:].sum())           # the partial corner block
        m = scenes.cut_measure(th, h, w, bits)
        assert m == S.measure_ref(th, h, w, bits) and m[0] == 0.0 and len(m) == 3
    full = np.full((2, 8, 8), 1023, np.int64)
    full[1] = 0
    p = np.concatenate([full.reshape(2, -1), np.zeros((2, 32), np.int64)], axis=1).astype("<u2").view(np.uint8).reshape(2, -1)
    th = S.thumb_ref(p, R.Fmt(10, R.C420_CENTER, 0, 0), 8, 8)
    assert th[0, 0, 0] == 65472 and scenes.cut_measure(th, 8, 8, 10) == [0.0, 1023 / 4]            # the largest sum fits; 10 bit is in 8-bit units


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_detect_cuts_finds_exactly_the_five_scene_starts_with_the_margin_it_relies_on(hw, kind):
    h, w = hw
    m = measure_of(S.clip26(kind, h, w), h, w)
    assert len(m) == 26
    ratios = {t: m[t] / S.reference_level(m, t) for t in range(1, 26)}
    inside = max(r for t, r in ratios.items() if t not in S.CUTS26)
    at_cut = min(ratios[t] for t in S.CUTS26)
    print(f"{kind} {h}x{w}: largest m/ref inside a scene {inside:.3f}, smallest at a cut {at_cut:.3f} (ratio {scenes.RATIO}); "
          f"largest m inside a scene {max(m[t] for t in range(1, 26) if t not in S.CUTS26):.2f}, smallest at a cut {min(m[t] for t in S.CUTS26):.2f} "
          f"(threshold {scenes.THRESHOLD})")
    assert scenes.detect_cuts(m, 4.0, 2.5) == [7, 12, 18, 22, 23]
    assert scenes.detect_cuts(m) == [7, 12, 18, 22, 23]                       # the defaults are those
    assert inside < scenes.RATIO < at_cut, (inside, at_cut)
    assert min(m[t] for t in S.CUTS26) >= scenes.THRESHOLD


def test_the_sizes_of_the_gpu_tests_give_the_same_cuts():
    """tests/test_gpu_scenes.py runs the blurred clip at 70 x 98 and 72 x 104 and a 13-frame clip without cuts."""
    for h, w in ((70, 98), (72, 104)):
        assert scenes.detect_cuts(measure_of(S.clip26("blurred", h, w), h, w)) == S.CUTS26
    assert scenes.detect_cuts(measure_of(S._mk("blurred", 13, 70, 98, 7), 70, 98)) == []


def test_rule_details():
    assert scenes.detect_cuts([]) == [] and scenes.detect_cuts([0.0]) == []
    assert scenes.detect_cuts([0.0, 30.0]) == [1]                             # two frames: no neighbour, ref = 0
    assert scenes.detect_cuts([0.0, 3.9]) == []                               # below the threshold
    assert scenes.detect_cuts([0.0, 5, 5, 5, 12.4, 5, 5, 5]) == [] and scenes.detect_cuts([0.0, 5, 5, 5, 12.5, 5, 5, 5]) == [4]      # >= ratio * median
    assert scenes.detect_cuts([0.0, 5, 5, 30, 30, 5, 5, 5]) == [3, 4]         # a scene of one frame
    assert scenes.detect_cuts([0.0, 1, 1, 30, 1, 1], threshold=31.0) == [] and scenes.detect_cuts([0.0, 1, 1, 30, 1, 1], ratio=31.0) == []
    assert scenes.cut_reference([0.0, 1, 2, 3, 4, 5, 6, 7, 8], 4) == 4.0      # median of 1, 2, 3, 5, 6, 7
    assert scenes.cut_reference([0.0, 1, 2, 3], 1) == 2.5                     # m[0] never votes


# ---- 3. the incremental detector --------------------------------------------------------------------------------------------------------
def _streams():
    h, w = 90, 130
    th26 = S.thumb_ref(S.payloads_of(S.clip26("blurred", h, w), h, w), S.FMT420, h, w)
    plain = S.thumb_ref(S.payloads_of(S._mk("blurred", 13, h, w, 7), h, w), S.FMT420, h, w)
    return h, w, {"clip26": th26, "no cuts": plain, "1 frame": th26[6:7], "2 frames": th26[6:8], "4 frames": th26[5:9], "4 frames, none": th26[:4]}


def test_cut_detector_in_chunks_equals_detect_cuts_and_never_decides_early():
    h, w, streams = _streams()
    for name, th in streams.items():
        n = len(th)
        want = scenes.detect_cuts(scenes.cut_measure(th, h, w, 8))
        if name == "clip26":
            assert want == S.CUTS26
        if name == "2 frames" or name == "4 frames":
            assert want, name                                                   # the short streams with a cut in them do have one
        for chunk in (1, 2, 5, n):
            det = scenes.CutDetector(h, w, 8)
            seen, released = 0, []
            for o in range(0, n, chunk):
                out = det.feed(th[o:o + chunk])
                seen = min(o + chunk, n)
                assert all(t + 3 <= seen - 1 for t, _ in out), (name, chunk, out, seen)      # frame t + 3 has been seen
                assert det.decided == max(0, seen - 3)
                released += out
            with pytest.raises(ValueError):
                det.is_cut(det.decided)
            released += det.finish()
            assert [t for t, _ in released] == list(range(n)), (name, chunk)                 # every frame once, in order
            assert [t for t, c in released if c] == want == det.cuts, (name, chunk)
            assert det.m == scenes.cut_measure(th, h, w, 8)
            assert all(det.is_cut(t) == (t in want) for t in range(n))
            with pytest.raises(ValueError):
                det.feed(th[:1])
    with pytest.raises(ValueError):
        scenes.CutDetector(h, w).feed(np.zeros((1, 3, 3), np.uint16))


# ---- 4. windows -------------------------------------------------------------------------------------------------------------------------
def _scene_of(t, starts, n):
    a = max(s for s in starts if s <= t)
    b = min([s for s in starts if s > t] + [n])
    return a, b


CUT_SETS = [[], [1], [4], [5], [8], [1, 2], [4, 6], [3, 4, 5], [7, 12, 18, 22, 23], [8, 16], [25], [24, 25], [2, 40]]


def test_plan_scene_windows_restores_every_frame_once_inside_its_scene_and_equals_the_per_scene_plans():
    for n, L, cuts in itertools.product((1, 2, 3, 8, 9, 26), (1, 4, 5, 16), CUT_SETS):
        plan = restore.plan_scene_windows(n, L, cuts)
        starts = [0] + [c for c in cuts if c < n]
        done = []
        for lo, cnt, idx in plan:
            a, b = _scene_of(lo, starts, n)
            assert 1 <= cnt <= L and len(idx) == 2 + cnt + 2 and idx[2:2 + cnt] == list(range(lo, lo + cnt))
            assert all(a <= i < b for i in idx), (n, L, cuts, lo, idx)            # no input frame of another scene
            assert (lo - a) % L == 0                                                # windows restart at the scene start
            done += idx[2:2 + cnt]
        assert done == list(range(n)), (n, L, cuts)
        want = []
        for a, b in zip(starts, starts[1:] + [n]):
            want += [(a + lo, cnt, [a + i for i in idx]) for lo, cnt, idx in restore.plan_windows(b - a, L)]
        assert plan == want
        if not starts[1:]:
            assert plan == restore.plan_windows(n, L)
    assert restore.plan_scene_windows(11, 4, []) == restore.plan_windows(11, 4)
    # a cut at a multiple of one_len and one that is not; scenes of 1 and 2 frames clamp as clips of that length do
    assert restore.plan_scene_windows(10, 4, [4])[:2] == [(0, 4, [2, 1, 0, 1, 2, 3, 2, 1]), (4, 4, [6, 5, 4, 5, 6, 7, 8, 9])]
    assert restore.plan_scene_windows(10, 4, [5])[:3] == [(0, 4, [2, 1, 0, 1, 2, 3, 4, 3]), (4, 1, [2, 3, 4, 3, 2]), (5, 4, [7, 6, 5, 6, 7, 8, 9, 8])]
    assert restore.plan_scene_windows(6, 4, [3, 4]) == [(0, 3, [2, 1, 0, 1, 2, 1, 0]), (3, 1, [3, 3, 3, 3, 3]), (4, 2, [4, 4, 4, 5, 5, 5])]
    for bad in ([0], [-1], [3, 3], [5, 4], [2.5]):
        with pytest.raises(ValueError):
            restore.plan_scene_windows(10, 4, bad)


class _LateCuts:
    """A decider that knows the cuts but, like the detector, releases the decision for frame t only once frame t + 3 has been fed or the
    stream has ended; it records what it was fed."""
    lookahead = 3

    def __init__(self, cuts):
        self.cuts, self.fed, self.ended, self.asked = set(cuts), [], False, []

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


def _drain(src, L):
    got, k = [], 0
    while True:
        w = src.window(k, L)
        if w is None:
            return got
        got.append((w[0], w[1], [int(f[0]) for f in w[2]]))
        assert len(src.buf) <= L + restore.PAST + restore.FUTURE + 3 + 1, len(src.buf)       # only what a future window can still need
        k += 1


def test_streaming_source_with_late_decisions_hands_out_the_planned_windows():
    for n, L, cuts in itertools.product((1, 2, 3, 5, 8, 9, 26, 33), (1, 4, 5, 16), CUT_SETS):
        frames = [np.array([i]) for i in range(n)]
        late = _LateCuts(cuts)
        src = restore._SceneFrames(iter(frames), late)
        assert _drain(src, L) == restore.plan_scene_windows(n, L, cuts), (n, L, cuts)
        assert late.fed == list(range(n)) and late.ended                                     # every frame once, in order
        assert src.cuts == [c for c in cuts if c < n]
        listed = restore._SceneFrames(iter(frames), scenes.ListedCuts(cuts))
        assert _drain(listed, L) == restore.plan_scene_windows(n, L, cuts), (n, L, cuts)
        assert listed.cuts == [c for c in cuts if c < n]
    assert restore._SceneFrames(iter([]), scenes.ListedCuts([3])).window(0, 4) is None


def test_streaming_source_driven_by_the_real_detector_reads_no_further_than_three_frames_beyond_the_window():
    h, w, L = 90, 130, 4
    th = S.thumb_ref(S.payloads_of(S.clip26("blurred", h, w), h, w), S.FMT420, h, w)

    class Host:                                                                               # the detector behind host thumbnails
        lookahead = 3

        def __init__(self):
            self.det = scenes.CutDetector(h, w, 8)

        def feed(self, frames):
            self.det.feed([th[int(f[0])] for f in frames])

        finish = lambda self: self.det.finish()                                              # noqa: E731
        is_cut = lambda self, t: self.det.is_cut(t)                                          # noqa: E731

    read = []

    def frames():
        for i in range(26):
            read.append(i)
            yield np.array([i])
    src = restore._SceneFrames(frames(), Host())
    k, got = 0, []
    while True:
        win = src.window(k, L)
        if win is None:
            break
        got.append((win[0], win[1], [int(f[0]) for f in win[2]]))
        assert read[-1] <= min(25, win[0] + L + restore.FUTURE - 1 + 3)                       # the window's last possible input frame + 3
        k += 1
    assert got == restore.plan_scene_windows(26, L, S.CUTS26) and src.cuts == S.CUTS26


# ---- 5. the cut list and the command line -----------------------------------------------------------------------------------------------
def test_parse_cuts_accepts_and_refuses_what_the_format_says():
    assert scenes.parse_cuts("") == [] and scenes.parse_cuts("# nothing\n\n   \n") == []
    assert scenes.parse_cuts("7\n12 # second scene\n\n# c\n  18\n22\n23") == [7, 12, 18, 22, 23]
    assert scenes.parse_cuts("1\r\n2\r\n") == [1, 2]
    assert scenes.parse_cuts(scenes.format_cuts([7, 12, 18])) == [7, 12, 18] and scenes.parse_cuts(scenes.format_cuts([])) == []
    for text, line in (("0\n", 1), ("3\n3\n", 2), ("5\n# c\n4\n", 3), ("7\n-1\n", 2), ("1.5\n", 1), ("1 2\n", 1), ("x\n", 1), ("2\n\n+3\n", 3)):
        with pytest.raises(ValueError, match=f"line {line}:"):
            scenes.parse_cuts(text)


def test_parser_defaults_and_scene_options():
    ap = restore.make_parser()
    a = ap.parse_args(["--variant", "deblur_small", "--checkpoint", "synthetic", "-", "-"])
    assert (a.scene_cuts, a.cut_threshold, a.cut_ratio, a.cuts_out) == ("off", 4.0, 2.5, None)
    assert (a.dtype, a.one_len, a.matrix, a.range, a.no_pipeline, a.input, a.output) == ("bf16", 16, None, None, False, "-", "-")
    a = ap.parse_args(["--variant", "deblur_small", "--checkpoint", "synthetic", "--scene_cuts", "auto", "--cut_threshold", "6", "--cut_ratio", "3",
                       "--cuts_out", "c.txt", "-", "-"])
    assert (a.scene_cuts, a.cut_threshold, a.cut_ratio, a.cuts_out) == ("auto", 6.0, 3.0, "c.txt")
    assert ap.parse_args(["--variant", "deblur", "--checkpoint", "synthetic", "--scene_cuts", "cuts.txt", "-", "-"]).scene_cuts == "cuts.txt"


def test_restore_video_refuses_a_bad_cut_file_before_it_touches_the_device(tmp_path):
    import subprocess
    import sys
    bad = tmp_path / "cuts.txt"
    bad.write_text("4\n4\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--variant", "deblur_small", "--checkpoint", "synthetic",
                        "--scene_cuts", str(bad), "-", "-"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "line 2" in r.stderr
