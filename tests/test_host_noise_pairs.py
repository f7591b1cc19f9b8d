"""CPU: the temporal noise estimate of the video restorer (shiftnet_amd/noise.py): that the library exports the two pair
histograms without an ABI bump, the pair histogram -> sigma function on hand-made histograms, the restatement of tests/noise_pairs_ref.py on
hand-made frames, the rule that combines the two estimates, the curves, the restorer's and the command line's forms, and the accuracy of the
estimate against the INJECTED sigma on synthetic clips (never against a second run of the estimator)."""
import importlib.util
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import noise_pairs_ref as NP
import noise_ref as N
import yuv_ref as R
from shiftnet_amd import noise, restore, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = R.Fmt(8, R.C444, R.BT709, R.LIMITED)


# ---- 1. the library ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_pair_histograms_and_keeps_the_abi_version():
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()                                              # hipcc cross-compiles gfx950 without a GPU
    from shiftnet_amd import lib as L
    lib = L.load()
    for name in ("sn_yuv_noise_hist_pairs", "sn_yuv_noise_hist_pairs_bands"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20
    with open(os.path.join(ROOT, "include", "shiftnet_hip.h")) as fh:
        header = fh.read()
    assert "#define SN_ABI_VERSION 20 " in header
    for name in ("sn_yuv_noise_hist_pairs", "sn_yuv_noise_hist_pairs_bands"):
        assert (f"int {name}(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, uint32_t* dst, int lo, int hi,"
                in header)


def test_noise_module_still_imports_no_torch():
    code = ("import sys; import shiftnet_amd.noise as n; n.combine_sigma(3.0, 2.0, 'min'); n.pair_sigma([0, 4, 4], 8, 0, 0); "
            "sys.exit(1 if 'torch' in sys.modules else 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "shift-net_amd"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- 2. pair histogram -> sigma on hand-made histograms -----------------------------------------------------------------------------------
def test_pair_hist_to_sigma_on_hand_made_histograms():
    assert noise.pair_bins(8) == 1021 == NP.nbp(8) and noise.pair_bins(10) == 4093 == NP.nbp(10)
    empty = np.zeros(1021, np.uint32)
    assert noise.pair_sigma(empty, 8, noise.BT709, noise.LIMITED) is None and noise.pair_sigma_luma(empty) is None      # no block counted
    zero = empty.copy()
    zero[0] = 1234                                           # every block in bin 0: the same frame twice
    assert noise.pair_sigma(zero, 8, noise.BT709, noise.LIMITED) is None and noise.pair_is_repeat(zero) and noise.pair_is_repeat(empty)
    assert noise.pair_sigma_luma(zero) == 0.0                # the arithmetic alone would say "no noise"; the repeat rule is pair_sigma's
    zero[1] = 1                                              # one block outside bin 0: an estimate again (the median stays in bin 0: 0)
    assert not noise.pair_is_repeat(zero) and noise.pair_sigma(zero, 8, noise.BT709, noise.LIMITED) == 0.0
    # the worked example of the spatial test: counts 10, 20, 40, 20, 10 in bins 0 .. 4 -> med = 2.0 (hist_median, the same bin geometry)
    h = empty.copy()
    h[:5] = [10, 20, 40, 20, 10]
    assert noise.hist_median(h) == 2.0
    var = (2.0 / 0.6744897501960817) ** 2 - 2.0 / 3.0        # 8.79237... - 0.66667... = 8.125704...
    assert abs(var - 8.1257) < 1e-4
    assert noise.pair_sigma_luma(h) == math.sqrt(var / 8.0) and abs(noise.pair_sigma_luma(h) - 1.00783) < 1e-4         # the 2/3 and the / 8
    g = (0.2126 ** 2 + 0.7152 ** 2 + 0.0722 ** 2) ** 0.5
    assert abs(noise.pair_sigma(h, 8, noise.BT709, noise.LIMITED) - math.sqrt(var / 8.0) / (g * 219.0 / 255.0)) < 1e-12
    assert abs(noise.pair_sigma(h, 10, noise.BT709, noise.LIMITED) * 4.0 - noise.pair_sigma(h, 8, noise.BT709, noise.LIMITED)) < 1e-12
    # a median whose square falls below 2/3 is clamped to zero noise: counts 60, 40 -> med = 0.5 * 50 / 60 = 0.41667, (med / 0.6745)^2 = 0.3816
    h0 = empty.copy()
    h0[:2] = [60, 40]
    assert noise.pair_sigma(h0, 8, noise.BT601, noise.FULL) == 0.0
    # white noise of sigma s on the codes: var(v) = 8 s^2 + 2/3.  A histogram drawn from that model reads s (the constants, end to end)
    rng = np.random.default_rng(5)
    for s in (1.0, 4.0):
        codes = np.rint(100.0 + rng.normal(0.0, s, (8, 400000))).astype(np.int64)
        v = np.abs((codes[4] - codes[5] - codes[6] + codes[7]) - (codes[0] - codes[1] - codes[2] + codes[3]))
        assert abs(v.astype(np.float64).var() + v.mean() ** 2 - (8 * s * s + 2.0 / 3.0)) < 0.02 * (8 * s * s + 2.0 / 3.0)
        assert abs(noise.pair_sigma_luma(np.bincount(v, minlength=1021)) - s) < 0.02 * s
    # the function and the plain-loop restatement of the tests agree on random histograms
    for name, fmt in N.FORMATS.items():
        for _ in range(20):
            hh = np.zeros(NP.nbp(fmt.bits), np.uint32)
            k = int(rng.integers(1, 300))
            hh[:k] = rng.integers(0, 5000, k)
            a, b = noise.pair_sigma(hh, fmt.bits, fmt.matrix, fmt.range), NP.pair_sigma_ref(hh, fmt)
            assert (a is None and b is None) or abs(a - b) <= 1e-12 * max(1.0, b), (name, a, b)


def test_window_sigma_temporal_is_the_median_over_the_pairs_that_have_an_estimate():
    assert noise.window_sigma_temporal([None, 4.0, None, 10.0, 6.0]) == 6.0
    assert noise.window_sigma_temporal([None, 4.0, 10.0]) == 7.0
    assert noise.window_sigma_temporal([None, None]) is None and noise.window_sigma_temporal([]) is None
    assert noise.window_sigma_temporal([3.0, 3.5, 90.0, 3.25]) == 3.375                     # a cut inside a window is one outlier pair
    assert noise.window_sigma_temporal([70.0]) == 70.0                                       # no clamp here


# ---- 3. the restatement on hand-made frames ---------------------------------------------------------------------------------------------
def _frames(*Ys):
    return np.stack([R.join_planes(np.asarray(Y), np.full(np.shape(Y), 128), np.full(np.shape(Y), 128), F8) for Y in Ys])


def test_pair_restatement_counts_a_block_only_if_all_eight_codes_are_unclipped():
    Y0 = [[20, 30, 16, 40, 99], [25, 50, 60, 70, 99], [200, 234, 100, 90, 99]]                # 3 x 5: the last row and column are in no block
    Y1 = [[21, 33, 40, 40, 99], [25, 50, 60, 70, 99], [200, 235, 100, 90, 99]]
    p = _frames(Y0, Y1)
    h = NP.hist_pairs_ref(p, F8, 3, 5, 16, 235)
    assert h.shape == (1, 1021) and h.dtype == np.uint32
    v = abs((21 - 33 - 25 + 50) - (20 - 30 - 25 + 50))
    assert int(h.sum()) == 1 and h[0, v] == 1                # the second block holds a 16 in the FIRST frame only: it does not count
    assert int(NP.hist_pairs_ref(p[::-1], F8, 3, 5, 16, 235).sum()) == 1                       # ... nor with the 16 in the second frame
    both = NP.hist_pairs_ref(p, F8, 3, 5, 0, 255)
    assert int(both.sum()) == 2 and both[0, abs((40 - 40 - 60 + 70) - (16 - 40 - 60 + 70))] == 1
    assert int(NP.hist_pairs_ref(p, F8, 3, 5, 16, 50).sum()) == 0                              # 50 is not strictly below hi
    assert int(NP.hist_pairs_ref(p, F8, 3, 5, 20, 255).sum()) == 0                             # 20 is not strictly above lo
    assert NP.hist_pairs_ref(p[:, :15], F8, 1, 5, 0, 255).sum() == 0 and NP.hist_pairs_ref(p[:, :9], F8, 3, 1, 0, 255).sum() == 0     # H < 2, W < 2
    same = NP.hist_pairs_ref(_frames(Y0, Y0, Y1), F8, 3, 5, 0, 255)                            # three payloads are two pairs; a repeated frame: bin 0
    assert same.shape == (2, 1021) and same[0, 0] == 2 and int(same[0].sum()) == 2 and np.array_equal(same[1], both[0])
    rect = (1, 0, 4, 2)                                                                        # the grid is anchored at the rectangle's origin
    hr = NP.hist_pairs_ref(p, F8, 3, 5, 0, 255, rect)
    assert int(hr.sum()) == 2 and hr[0, abs((33 - 40 - 50 + 60) - (30 - 16 - 50 + 60))] >= 1
    bands = NP.hist_pairs_bands_ref(p, F8, 3, 5, 0, 255)                                       # the same blocks, split by band and saturated
    assert bands.shape == (1, 16, 128) and np.array_equal(bands.sum(axis=1)[:, :127], both[:, :127])
    assert bands[0, (2 * (20 + 30 + 25 + 50 + 21 + 33 + 25 + 50)) // 255, v] == 1


def test_band_indices_0_and_15_are_reached_and_16_never_is():
    for bits in (8, 10):
        for rng_ in (R.LIMITED, R.FULL):
            lo, hi = N.clip_codes(R.Fmt(bits, R.C444, R.BT709, rng_))
            assert NP.band_of(8 * (lo + 1), lo, hi) == 0 and NP.band_of(8 * (hi - 1), lo, hi) == 15
            S = np.arange(8 * (lo + 1), 8 * (hi - 1) + 1)                                      # every sum a counting block can have
            b = NP.band_of(S, lo, hi)
            assert b.min() == 0 and b.max() == 15 and set(np.unique(b)) == set(range(16)) and (np.diff(b) >= 0).all()
    for span in (2, 3):                                                                         # hi - lo small: the only codes are lo + 1 .. hi - 1
        for lo in (0, 7, -5):
            S = np.arange(8 * (lo + 1), 8 * (lo + span - 1) + 1)
            b = NP.band_of(S, lo, lo + span)
            assert 0 <= b.min() and b.max() <= 15, (span, lo, b)
    assert NP.band_of(8, 0, 2) == 8 and list(NP.band_of([8, 16], 0, 3)) == [5, 10]
    # through the histogram: a block of lo + 1 everywhere lands in band 0, one of hi - 1 in band 15
    fmt = R.Fmt(8, R.C444, R.BT709, R.LIMITED)
    Y = np.full((2, 4), 17)
    Y[:, 2:] = 234
    h = NP.hist_pairs_bands_ref(_frames(Y, Y), fmt, 2, 4, 16, 235)
    assert h[0, 0, 0] == 1 and h[0, 15, 0] == 1 and int(h.sum()) == 2


# ---- 4. the rule ---------------------------------------------------------------------------------------------------------------------------
def test_combine_sigma_in_all_three_modes_with_none_and_the_clamp_applied_once():
    c = noise.combine_sigma
    assert c(12.0, 5.0, "spatial") == 12.0 and c(12.0, 5.0, "temporal") == 5.0 and c(12.0, 5.0, "min") == 5.0
    assert c(5.0, 12.0, "spatial") == 5.0 and c(5.0, 12.0, "temporal") == 12.0 and c(5.0, 12.0, "min") == 5.0
    for est in noise.ESTIMATORS:
        assert c(12.0, None, est) == 12.0                                                      # no pair has an estimate: the spatial one
    assert c(0.0, None, "min") == 0.0 and c(0.0, 3.0, "min") == 0.0
    assert c(70.0, 60.0, "temporal") == 50.0 and c(70.0, 60.0, "min") == 50.0                  # the default clamp (0, 50), last
    # once and last: the rule sees the unclamped estimates, the clamp sees the rule's result
    assert c(1.0, 3.0, "min", (2.0, 30.0)) == 2.0 and c(40.0, 35.0, "min", (2.0, 30.0)) == 30.0 and c(1.0, 40.0, "temporal", (2.0, 30.0)) == 30.0
    assert c(1.0, None, "temporal", (2.0, 30.0)) == 2.0
    # "spatial" is today's window_sigma, which is factored through the same median
    for per in ([None, 4.0, None, 10.0, 6.0], [None, 4.0, 10.0], [None, None], [], [70.0, 80.0, None]):
        for clamp in ((0.0, 50.0), (5.0, 7.5)):
            assert noise.window_sigma(per, clamp) == c(noise.frames_median(per), 123.0, "spatial", clamp) == c(noise.frames_median(per), None, "min", clamp)
    assert noise.frames_median([None]) == 0.0 and noise.frames_median([90.0, None, 70.0]) == 80.0      # unclamped
    for bad in ("Spatial", "max", "", None, 1):
        with pytest.raises(ValueError, match="sigma_estimator"):
            c(1.0, 2.0, bad)
    with pytest.raises(ValueError, match="sigma_clamp"):
        c(1.0, 2.0, "min", (5.0, 1.0))


# ---- 5. curves -----------------------------------------------------------------------------------------------------------------------------
def _band_hists(levels, n=4096, bins=128):
    """[16, NBV] with n blocks per listed band, all in the bin whose median reads about that v; bands not listed stay empty."""
    h = np.zeros((16, bins), np.int64)
    for b, v in levels.items():
        h[b, v] = n
    return h


def test_curves_min_per_band_repeats_left_out_and_filling_after_combining():
    args = (8, noise.BT709, noise.LIMITED)
    sp = lambda v: noise.band_sigma(_band_hists({0: v})[0], *args)                              # noqa: E731 -- what a bin reads, spatially ...
    te = lambda v: noise.pair_band_sigma(_band_hists({0: v})[0], *args)                         # noqa: E731 -- ... and temporally
    assert abs(te(8) * math.sqrt(2.0) - sp(8)) < 0.02 * sp(8)                                   # the same v is sqrt(2) times less noise between two frames
    spatial = _band_hists({2: 20, 5: 20, 9: 6, 12: 6})[None]
    pairs = _band_hists({2: 8, 5: 40, 9: 8})[None]                                              # band 12 has no temporal estimate, band 5's is higher
    curve = noise.window_curve_pairs(spatial, pairs, *args, "min")
    assert curve[2] == te(8) < sp(20) and curve[5] == sp(20) < te(40) and curve[9] == min(sp(6), te(8)) and curve[12] == sp(6)
    # filling happens after combining: band 3 and 4 lie on the line between the COMBINED knots 2 and 5, not between the spatial ones
    assert curve[3] == te(8) + (sp(20) - te(8)) * 1 / 3 and curve[4] == te(8) + (sp(20) - te(8)) * 2 / 3
    assert curve[0] == curve[1] == curve[2] and curve[15] == curve[12]
    assert noise.window_curve_pairs(spatial, pairs, *args, "spatial") == noise.window_curve(spatial, *args)
    t = noise.window_curve_pairs(spatial, pairs, *args, "temporal")
    assert t[2] == te(8) and t[5] == te(40) and t[9] == te(8) and t[12] == sp(6)                # the spatial knot where there is no temporal one
    # a band that only the pairs can estimate: spatial None, temporal there -> the temporal knot (None where neither exists: filled)
    only = noise.window_curve_pairs(_band_hists({2: 20})[None], _band_hists({7: 8})[None], *args, "min")
    assert only[7] == te(8) and only[2] == sp(20) and only[4] == sp(20) + (te(8) - sp(20)) * 2 / 5
    assert noise.window_curve_pairs(np.zeros((1, 16, 128)), np.zeros((2, 16, 128)), *args, "min") == [0.0] * 16
    # a repeat pair is left out of the sum: its bin-0 mass would halve the median's position in every band
    repeat = _band_hists({2: 0, 5: 0, 9: 0})
    with_repeat = np.stack([pairs[0], repeat, pairs[0]])
    assert noise.pair_is_repeat(repeat) and not noise.pair_is_repeat(pairs[0])
    assert np.array_equal(noise.sum_pair_bands(with_repeat), 2 * pairs[0])
    assert noise.window_curve_pairs(spatial, with_repeat, *args, "min") == curve
    summed_anyway = with_repeat.sum(axis=0)[None]
    assert noise.window_curve_pairs(spatial, summed_anyway, *args, "temporal")[2] != te(8)      # what leaving it in would do
    assert np.array_equal(noise.sum_pair_bands(np.stack([repeat, repeat])), np.zeros((16, 128)))
    # the rules of band_sigma: fewer than NLF_MIN_BLOCKS blocks, or the median in the saturating bin -> no temporal estimate
    assert noise.pair_band_sigma(_band_hists({0: 8}, n=1023)[0], *args) is None and noise.pair_band_sigma(_band_hists({0: 127})[0], *args) is None
    # the clamp comes last
    assert noise.window_curve_pairs(spatial, pairs, *args, "min", (3.0, 4.0)) == [min(max(k, 3.0), 4.0) for k in curve]


# ---- 6. accuracy against the injected sigma -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    """(spatial, temporal, min) per clip and injected sigma: 180 x 320, five frames, BT.709 limited 8 bit, seed 0.  Computed once, left unchanged."""
    out = {(clip, s): NP.clip_estimates(clip, s) for clip in NP.CLIPS for s in NP.ACC["sigmas"]}
    for clip in NP.CLIPS:
        print(f"{clip}: " + ", ".join(f"{s}: spatial {out[clip, s][0]:.2f} temporal {out[clip, s][1]:.2f}" for s in NP.ACC["sigmas"]))
    return out


def test_flat_clip_temporal_and_min_read_the_injected_sigma(table):
    for s in NP.ACC["sigmas"]:
        sp, te, mn = table["flat 0.5", s]
        assert abs(te - s) <= N.margin(s) and abs(mn - s) <= N.margin(s), (s, sp, te, mn)


def test_static_texture_temporal_and_min_read_the_injected_sigma_where_spatial_does_not(table):
    for s in NP.ACC["sigmas"]:
        sp, te, mn = table["static texture", s]
        assert abs(te - s) <= N.margin(s) and abs(mn - s) <= N.margin(s), (s, sp, te, mn)
        assert sp - s > N.margin(s), (s, sp)                                                    # the defect the estimator exists for


def test_moving_texture_min_is_no_worse_than_spatial_and_both_stay_upper_bounds(table):
    for s in NP.ACC["sigmas"]:
        sp, te, mn = table["texture moving 1 px per frame", s]
        assert mn <= sp and mn >= s - N.margin(s) and sp >= s - N.margin(s), (s, sp, te, mn)


def test_identical_frames_have_no_temporal_estimate_and_fall_back_to_spatial():
    pay = N.noisy_payloads(NP.texture_clip(1, 36, 44), 0.0, NP.ACC_FMT)                        # a clip of one frame: the window is that frame five times
    est = NP.window_estimates(list(pay), NP.ACC_FMT, 36, 44, 5, "min")
    assert est["pair_sigma"] == [[None] * 4] and est["temporal"] == [None] and est["sigma"] == [min(est["spatial"][0], 50.0)] and est["spatial"][0] > 5.0


# ---- 7. the restorer's and the command line's forms ---------------------------------------------------------------------------------------
class _Net:
    """As much of a GShiftNet as VideoRestorer looks at before it asks for the device."""

    def __init__(self, denoise):
        self.V = types.SimpleNamespace(denoise=denoise, topo="s")

    def parameters(self):
        import torch
        return iter([torch.zeros(1)])


def test_sigma_estimator_form_and_the_restorer_argument():
    for word in noise.ESTIMATORS:
        assert windows.sigma_estimator_form(word, "auto") == word == restore.sigma_estimator_form(word)
    assert windows.sigma_estimator_form("spatial", "fixed") == "spatial" and windows.sigma_estimator_form("spatial", "list") == "spatial"
    for bad in ("Min", "median", "", None, 3, ["min"]):
        with pytest.raises(ValueError, match="sigma_estimator"):
            windows.sigma_estimator_form(bad, "auto")
        with pytest.raises(ValueError, match="sigma_estimator"):
            restore.VideoRestorer(_Net(True), 4, sigma="auto", sigma_estimator=bad)
    for word in ("temporal", "min"):
        for mode in ("fixed", "list"):
            with pytest.raises(ValueError, match=r"sigma_estimator.*sigma='auto'"):             # the message names both options
                windows.sigma_estimator_form(word, mode)
        for sigma in (10.0, [10.0, 12.0]):
            with pytest.raises(ValueError, match=r"sigma_estimator.*sigma='auto'"):
                restore.VideoRestorer(_Net(True), 4, sigma=sigma, sigma_estimator=word)
        with pytest.raises(ValueError, match="HIP device"):                                     # accepted: the device check is what refuses
            restore.VideoRestorer(_Net(True), 4, sigma="auto", sigma_estimator=word)
        with pytest.raises(ValueError, match="HIP device"):
            restore.VideoRestorer(_Net(True), 4, sigma="auto", sigma_estimator=word, noise_model="level")
        with pytest.raises(ValueError):                                                         # a deblur variant has no sigma to estimate
            restore.VideoRestorer(_Net(False), 4, sigma_estimator=word)
    with pytest.raises(ValueError, match="HIP device"):
        restore.VideoRestorer(_Net(True), 4, sigma=10.0, sigma_estimator="spatial")
    with pytest.raises(ValueError, match="HIP device"):
        restore.VideoRestorer(_Net(False), 4, sigma_estimator="spatial")


def test_parser_takes_the_three_estimators():
    ap = restore.make_parser()
    base = ["--variant", "denoise_small", "--checkpoint", "synthetic", "--sigma", "auto"]
    assert ap.parse_args(base + ["-", "-"]).sigma_estimator == "spatial"
    for word in noise.ESTIMATORS:
        assert ap.parse_args(base + ["--sigma_estimator", word, "-", "-"]).sigma_estimator == word
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--sigma_estimator", "median", "-", "-"])


def test_restore_video_refuses_an_estimator_without_sigma_auto_before_it_touches_the_device(tmp_path):
    exe = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--checkpoint", "synthetic", "--variant", "denoise_small"]
    run = lambda args: subprocess.run(exe + args + ["-", "-"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)   # noqa: E731
    r = run(["--sigma", "10", "--sigma_estimator", "min"])
    assert r.returncode == 2 and "--sigma_estimator min needs --sigma auto" in r.stderr
    r = run(["--sigma", str(tmp_path / "missing.txt"), "--sigma_estimator", "temporal"])          # refused before the file is looked for
    assert r.returncode == 2 and "--sigma_estimator temporal needs --sigma auto" in r.stderr
    r = run(["--sigma", "auto", "--sigma_estimator", "median"])
    assert r.returncode == 2 and "--sigma_estimator" in r.stderr
    r = run(["--sigma", "10", "--sigma_estimator", "spatial", "--sigma_clamp", "9", "3"])        # spatial with a number is today's call: the next check speaks
    assert r.returncode == 2 and "sigma_clamp" in r.stderr
