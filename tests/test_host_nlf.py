"""The noise-level function on the host (no GPU): shiftnet_amd/noise.py against the plain-loop restatement of tests/nlf_ref.py and against the
INJECTED function of a synthetic clip, the hole-filling rules on hand-made histograms with exact floats, the file format, and every argument error of
``VideoRestorer(noise_model=...)`` and of the command line that is reachable before the device is."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import nlf_ref as F
import noise_ref as N
import yuv_ref as R
from shiftnet_amd import noise, restore, restore_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The worst |knot - injected| and |knot - flat estimate| that the numpy reference (F.curve_ref on F.hist_bands_ref) reaches on the seeded clips below,
# recorded in DESIGN.md 3.17; the bounds are these times 1.5, to allow for seed-to-seed scatter.
MEASURED_CURVE_ERROR = 1.2331
MEASURED_FLAT_ERROR = 0.4297


def test_constants_and_knot_positions():
    assert noise.NLF_BANDS == F.BANDS == 16 and noise.NLF_MIN_BLOCKS == F.MIN_BLOCKS == 1024
    assert (noise.nlf_bins(8), noise.nlf_bins(10)) == (F.nbv(8), F.nbv(10)) == (128, 512)
    assert noise.knot_codes(16, 235) == F.knot_codes(16, 235) == [16 + (b + 0.5) * 219 / 16 for b in range(16)]
    assert noise.knot_codes(0, 1023)[0] == 0.5 * 1023 / 16 and noise.knot_codes(0, 1023)[15] == 15.5 * 1023 / 16


def test_band_histograms_summed_over_the_bands_are_the_flat_histogram():
    """The restatement the GPU test holds the kernel to, against the restatement of the flat statistic: the same blocks, only split."""
    for fmt, (H, W) in ((F.FMT, (38, 52)), (R.Fmt(10, R.C444, R.BT709, R.FULL), (34, 70))):
        rng = np.random.default_rng(3)
        top = (1 << fmt.bits) - 1
        n = R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)
        p = rng.integers(0, top + 1, (2, n))
        p = p.astype(np.uint8) if fmt.bits == 8 else p.astype("<u2").view(np.uint8).reshape(2, -1)
        lo, hi = N.clip_codes(fmt)
        nb = F.nbv(fmt.bits)
        bands = F.hist_bands_ref(p, fmt, H, W, lo, hi).astype(np.int64)
        flat = N.hist_ref(p, fmt, H, W, lo, hi).astype(np.int64)
        assert bands.shape == (2, 16, nb) and bands.sum() == flat.sum() > 0
        assert np.array_equal(bands.sum(axis=1)[:, :nb - 1], flat[:, :nb - 1])
        assert np.array_equal(bands.sum(axis=1)[:, nb - 1], flat[:, nb - 1:].sum(axis=1)) and bands[:, :, nb - 1].sum() > 0


def test_curve_of_a_ramp_with_signal_dependent_noise_is_the_injected_function():
    """96 x 256, T = 6, seed 7: a luma ramp over all bands, sigma of the luma codes affine from 6 at black to 2 at white.  Judged against the INJECTED
    function at the knots' codes.  Reference (F.curve_ref): worst |knot - injected| 1.2331 at knot 0 (9.13 injected, 7.89 estimated: blocks that the
    noise pushes below black do not count, which truncates the distribution in the outer bands), 0.31 over knots 1 .. 14.  Bound: 1.5 x 1.2331."""
    c, fmt = F.RAMP, F.FMT
    lo, hi = N.clip_codes(fmt)
    hb = F.hist_bands_ref(F.ramp_payloads(), fmt, c["h"], c["w"], lo, hi)
    assert int(hb.sum(axis=(0, 2)).min()) >= noise.NLF_MIN_BLOCKS                           # every band has an estimate of its own
    ref = F.curve_ref(hb, fmt)
    got = noise.window_curve(hb, fmt.bits, fmt.matrix, fmt.range)
    inj = F.injected_sigma(F.knot_codes(lo, hi))
    err_ref, err = np.abs(np.array(ref) - inj), np.abs(np.array(got) - inj)
    print("injected", np.round(inj, 3).tolist())
    print("curve   ", np.round(got, 3).tolist())
    print(f"worst |knot - injected|: reference {err_ref.max():.4f} (knot {int(err_ref.argmax())}), knots 1 .. 14 {err_ref[1:15].max():.4f}; "
          f"noise.window_curve {err.max():.4f}")
    assert inj[0] > 2.5 * inj[15]                                                           # the shadows carry several times the highlights' noise
    assert got == ref                                                                       # the same integers through the same definition
    assert err.max() <= 1.5 * MEASURED_CURVE_ERROR, (err.max(), int(err.argmax()))
    flat = noise.frame_sigma(N.hist_ref(F.ramp_payloads(), fmt, c["h"], c["w"], lo, hi).sum(axis=0), fmt.bits, fmt.matrix, fmt.range)
    assert inj[15] < flat < inj[0]                                                          # what one level per window makes of it: too little, too much


def test_flat_noise_gives_a_flat_curve_at_the_flat_estimate():
    """The same ramp with sigma 4 of the luma codes everywhere: every estimated knot against ``frame_sigma`` of the summed flat histogram.  Reference:
    worst |knot - flat| 0.4297 (knot 0, the truncation again; the flat estimate itself reads 6.183 for 6.213 injected).  Bound: 1.5 x 0.4297."""
    c, fmt = F.RAMP, F.FMT
    lo, hi = N.clip_codes(fmt)
    p = F.ramp_payloads(s_black=4.0, s_white=4.0)
    hb = F.hist_bands_ref(p, fmt, c["h"], c["w"], lo, hi)
    flat = noise.frame_sigma(N.hist_ref(p, fmt, c["h"], c["w"], lo, hi).sum(axis=0), fmt.bits, fmt.matrix, fmt.range)
    got = noise.window_curve(hb, fmt.bits, fmt.matrix, fmt.range)
    assert got == F.curve_ref(hb, fmt)
    err = np.abs(np.array(got) - flat)
    print(f"flat estimate {flat:.4f} (injected {F.luma_to_rgb_sigma(4.0, fmt):.4f}); worst |knot - flat| {err.max():.4f} (knot {int(err.argmax())})")
    assert abs(flat - F.luma_to_rgb_sigma(4.0, fmt)) <= N.margin(F.luma_to_rgb_sigma(4.0, fmt))
    assert err.max() <= 1.5 * MEASURED_FLAT_ERROR, (err.max(), int(err.argmax()))


def _hand_made():
    """[16][128]: band 0 empty; 1 below NLF_MIN_BLOCKS; 2 and 5 estimated; 3, 4 holes between them; 6 estimated; 7 saturated (median in the last bin);
    8 with exactly NLF_MIN_BLOCKS blocks; 9 .. 15 empty."""
    h = np.zeros((16, 128), np.uint32)
    h[1, 2] = 1023
    h[2, 2], h[2, 3], h[2, 4] = 500, 1200, 500
    h[5, 8], h[5, 9] = 3000, 3001
    h[6, 1] = 4000
    h[7, 5], h[7, 127] = 1000, 1001
    h[8, 6], h[8, 7] = 512, 512
    return h


def test_holes_are_filled_exactly_as_specified():
    fmt = F.FMT
    h = _hand_made()
    s = lambda b: N.sigma_ref(h[b], fmt)                                                      # noqa: E731 -- the flat definition, plain loops
    k2, k5, k6, k8 = s(2), s(5), s(6), s(8)
    assert 0.0 < k6 < k2 < k8 < k5 < 50.0
    want = [k2, k2, k2, k2 + (k5 - k2) * 1 / 3, k2 + (k5 - k2) * 2 / 3, k5, k6, k6 + (k8 - k6) * 1 / 2, k8] + [k8] * 7
    assert noise.window_curve(h, 8, fmt.matrix, fmt.range) == want == F.curve_ref(h, fmt)    # exact floats
    assert [noise.band_sigma(h[b], 8, fmt.matrix, fmt.range) for b in (0, 1, 7, 9)] == [None] * 4
    assert noise.band_sigma(h[8], 8, fmt.matrix, fmt.range) == k8                            # exactly NLF_MIN_BLOCKS blocks do count
    # the window's frames are summed before anything is judged: two frames of 512 blocks make a band that neither is
    two = np.zeros((2, 16, 128), np.uint32)
    two[:, 4, 3] = 512
    one = np.zeros((16, 128), np.uint32)
    one[4, 3] = 1024
    assert noise.window_curve(two, 8, fmt.matrix, fmt.range) == noise.window_curve(one, 8, fmt.matrix, fmt.range) == [N.sigma_ref(one[4], fmt)] * 16
    assert noise.window_curve(two[:1], 8, fmt.matrix, fmt.range) == [0.0] * 16
    # clamped last: the filled values as well
    got = noise.window_curve(h, 8, fmt.matrix, fmt.range, clamp=(k2 + 0.01, k8))
    assert got == [min(max(k, k2 + 0.01), k8) for k in want] and got[0] == k2 + 0.01 and got[5] == k8
    assert noise.fill_curve([None, 1.0, None, None, 4.0, None]) == [1.0, 1.0, 2.0, 3.0, 4.0, 4.0]


def test_no_band_with_an_estimate_gives_zeros_which_are_then_clamped():
    z = np.zeros((3, 16, 512), np.uint32)
    assert noise.window_curve(z, 10, R.BT709, R.LIMITED) == [0.0] * 16 == F.curve_ref(z, R.Fmt(10, 0, R.BT709, R.LIMITED))
    assert noise.window_curve(z, 10, R.BT709, R.LIMITED, clamp=(2.5, 50.0)) == [2.5] * 16
    z[:, :, 511] = 5000                                                                     # every band saturated: the same
    assert noise.window_curve(z, 10, R.BT709, R.LIMITED, clamp=(2.5, 50.0)) == [2.5] * 16
    with pytest.raises(ValueError, match="sigma_clamp"):
        noise.window_curve(z, 10, R.BT709, R.LIMITED, clamp=(3.0, 1.0))


def test_curve_file_round_trip_and_refusals():
    rng = np.random.default_rng(0)
    curves = [[float(x) for x in rng.uniform(0.0, 50.0, 16)], [0.0] * 16, [1 / 3] * 15 + [49.99999999999999], [float(b) for b in range(16)]]
    text = noise.format_curves(curves, "level")
    assert text.startswith("#") and "level" in text.splitlines()[0] and len(text.splitlines()) == 5
    assert noise.parse_curves(text) == curves                                               # the same float64s, not nearly the same
    assert noise.format_curves(noise.parse_curves(text), "level") == text                   # and the same bytes
    assert noise.parse_curves(noise.format_curves([])) == [] and noise.parse_curves("") == []
    line = " ".join(["2"] * 16)
    assert noise.parse_curves(f"# c\n{line}\n\n  {line} # second window\r\n") == [[2.0] * 16] * 2
    for text, no in ((f"{line} 3\n", 1), (f"{line}\n1 2 3\n", 2), (f"{line}\n# c\n" + " ".join(["x"] * 16) + "\n", 3),
                     (" ".join(["-1"] * 16) + "\n", 1), (" ".join(["nan"] * 16) + "\n", 1), (f"{line}\n{line}\n" + " ".join(["inf"] * 16), 3), ("level\n", 1)):
        with pytest.raises(ValueError, match=f"line {no}:"):
            noise.parse_curves(text)
    assert noise.check_curves([range(16), np.arange(16.0)]) == [[float(b) for b in range(16)]] * 2
    for bad in ([[1.0] * 15], [[1.0] * 17], [1.0] * 16, ["level"], [[1.0] * 15 + [-1.0]], [[1.0] * 15 + [float("nan")]], [[1.0] * 15 + ["auto"]], [None]):
        with pytest.raises(ValueError):
            noise.check_curves(bad)


class _Net:
    """As much of a GShiftNet as VideoRestorer looks at before it asks for the device."""

    def __init__(self, denoise):
        self.V = types.SimpleNamespace(denoise=denoise, topo="s")

    def parameters(self):
        import torch
        return iter([torch.zeros(1)])


def test_restorer_noise_model_forms():
    curve = [5.0] * 16
    for nm in ("level", [curve]):                                                           # any noise model with a deblur variant
        with pytest.raises(ValueError, match="noise_model is for the denoise variants"):
            restore.VideoRestorer(_Net(False), 4, sigma=10.0, noise_model=nm)
    for sigma in (10.0, [10.0, 12.0]):                                                      # "level" rides on the flat estimate
        with pytest.raises(ValueError, match="needs sigma='auto'"):
            restore.VideoRestorer(_Net(True), 4, sigma=sigma, noise_model="level")
    for bad in ("Level", "flat", "auto", 5.0, [[1.0] * 15], [curve, [1.0] * 15 + [-2.0]], [[1.0] * 15 + [float("inf")]], [1.0] * 16):
        with pytest.raises(ValueError, match="noise"):
            restore.VideoRestorer(_Net(True), 4, sigma="auto", noise_model=bad)
    for sigma, good in (("auto", "level"), ("auto", [curve]), (10.0, [curve, curve]), ([10.0], (tuple(curve),)), ("auto", np.full((3, 16), 2.0)), (10.0, None)):
        with pytest.raises(ValueError, match="HIP device"):                                 # accepted: the device check is what refuses
            restore.VideoRestorer(_Net(True), 4, sigma=sigma, noise_model=good)


def test_per_window_list_of_curves_running_short_names_the_window():
    a, b = [1.0] * 16, [float(i) for i in range(16)]
    mode, nlf = restore.noise_model_form([a, b])
    assert mode == "list" and isinstance(nlf, restore.PerWindow) and nlf.at(0) == a and nlf.at(1) == b
    with pytest.raises(ValueError, match="noise_model lists 2 windows, window 2 has no entry"):
        nlf.at(2)
    part, run = restore_parts.NoiseLevel(*restore.sigma_form(10.0), nlf_mode=mode, nlf=nlf), restore._Run()      # the restorer's record of what every window used
    assert part.level(None, 9, run) == (10.0, a) and part.level(None, 9, run) == (10.0, b)
    with pytest.raises(ValueError, match="window 2"):
        part.level(None, 9, run)
    assert run.window_nlf == [a, b]


def test_parser_takes_flat_level_or_a_file():
    ap = restore.make_parser()
    base = ["--variant", "denoise_small", "--checkpoint", "synthetic", "--sigma", "auto"]
    a = ap.parse_args(base + ["-", "-"])
    assert a.noise_model == "flat" and a.noise_model_out is None
    for word in ("flat", "level", "nlf.txt"):
        assert ap.parse_args(base + ["--noise_model", word, "-", "-"]).noise_model == word
    a = ap.parse_args(base + ["--noise_model", "level", "--noise_model_out", "n.txt", "-", "-"])
    assert (a.noise_model, a.noise_model_out) == ("level", "n.txt")


def test_restore_video_refuses_bad_noise_model_arguments_before_it_touches_the_device(tmp_path):
    exe = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--checkpoint", "synthetic"]
    run = lambda args: subprocess.run(exe + args + ["-", "-"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)   # noqa: E731
    bad = tmp_path / "nlf.txt"
    bad.write_text(" ".join(["3"] * 16) + "\n" + " ".join(["3"] * 15) + "\n")
    r = run(["--variant", "denoise_small", "--sigma", "10", "--noise_model", str(bad)])
    assert r.returncode == 2 and "line 2" in r.stderr
    r = run(["--variant", "denoise_small", "--sigma", "10", "--noise_model", str(tmp_path / "missing.txt")])
    assert r.returncode == 2 and "--noise_model" in r.stderr
    r = run(["--variant", "denoise_small", "--sigma", "10", "--noise_model", "level"])
    assert r.returncode == 2 and "--sigma auto" in r.stderr
    r = run(["--variant", "deblur_small", "--noise_model", "level"])
    assert r.returncode == 2 and "denoise" in r.stderr
