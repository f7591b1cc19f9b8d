"""CPU: the noise-level estimate of the video restorer (shiftnet_amd/noise.py): that the library exports ``sn_yuv_noise_hist`` without an
ABI bump, the histogram -> sigma function on hand-made histograms, the restorer's and the command line's sigma forms, and the accuracy of
the estimate against the INJECTED sigma on synthetic clips (never against a second run of the estimator)."""
import importlib.util
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import noise_ref as N
import yuv_ref as R
from shiftnet_amd import noise, restore, restore_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the library ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_sn_yuv_noise_hist_and_keeps_the_abi_version():
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()                                              # hipcc cross-compiles gfx950 without a GPU
    from shiftnet_amd import lib as L
    lib = L.load()
    assert hasattr(lib, "sn_yuv_noise_hist") and "sn_yuv_noise_hist" in L.SYMBOLS
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20
    with open(os.path.join(ROOT, "include", "shiftnet_hip.h")) as fh:
        header = fh.read()
    assert "#define SN_ABI_VERSION 20 " in header
    assert ("int sn_yuv_noise_hist(const uint8_t* src, const sn_yuv_fmt* fmt, uint32_t* dst, int lo, int hi, int T, int H, int W, void* stream);"
            in header)


def test_noise_module_does_not_import_torch():
    code = "import sys; import shiftnet_amd.noise; sys.exit(1 if 'torch' in sys.modules else 0)"
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "shift-net_amd"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- 2. histogram -> sigma on hand-made histograms --------------------------------------------------------------------------------------
def test_hist_to_sigma_on_hand_made_histograms():
    assert noise.nbins(8) == 511 and noise.nbins(10) == 2047
    assert noise.clip_codes(8, noise.LIMITED) == (16, 235) and noise.clip_codes(10, noise.LIMITED) == (64, 940)
    assert noise.clip_codes(8, noise.FULL) == (0, 255) and noise.clip_codes(10, noise.FULL) == (0, 1023)
    empty = np.zeros(511, np.uint32)
    assert noise.hist_median(empty) is None and noise.sigma_luma(empty) is None and noise.frame_sigma(empty, 8, noise.BT709, noise.LIMITED) is None
    zero = empty.copy()
    zero[0] = 1234                                           # med = 0 + 0.5 * 617 / 1234 = 0.25; (0.25 / 0.6745)^2 = 0.137 < 1/3: clamped
    assert noise.hist_median(zero) == 0.25
    assert noise.sigma_luma(zero) == 0.0 and noise.frame_sigma(zero, 8, noise.BT601, noise.FULL) == 0.0
    # the worked example: counts 10, 20, 40, 20, 10 in bins 0 .. 4.  N = 100, N / 2 = 50; cumulative 10, 30, 70: bin 2 is the first to reach 50.
    # Bin 2 covers [1.5, 2.5): med = 1.5 + 1 * (50 - 30) / 40 = 2.0.
    # var = (2 / 0.6744897501960817)^2 - 1/3 = 8.79237... - 0.33333... = 8.459037...; sigma_Y = sqrt(var) / 2 = 1.454221...
    h = empty.copy()
    h[:5] = [10, 20, 40, 20, 10]
    assert noise.hist_median(h) == 2.0
    var = (2.0 / 0.6744897501960817) ** 2 - 1.0 / 3.0
    assert noise.sigma_luma(h) == np.sqrt(var) / 2.0 and abs(noise.sigma_luma(h) - 1.4542) < 1e-4
    # BT.709 limited, 8 bit: g = sqrt(0.2126^2 + 0.7152^2 + 0.0722^2) = 0.74961..., s = 219 / 255
    g = (0.2126 ** 2 + 0.7152 ** 2 + 0.0722 ** 2) ** 0.5
    assert abs(g - 0.7496) < 1e-4 and abs(noise.luma_gain(noise.BT709) - g) < 1e-15
    assert abs(noise.frame_sigma(h, 8, noise.BT709, noise.LIMITED) - noise.sigma_luma(h) / (g * 219.0 / 255.0)) < 1e-12
    # 10 bit: the same histogram is a quarter of the noise; full range: s = 1023 / 255
    assert abs(noise.frame_sigma(h, 10, noise.BT709, noise.LIMITED) * 4.0 - noise.frame_sigma(h, 8, noise.BT709, noise.LIMITED)) < 1e-12
    assert noise.code_scale(10, noise.FULL) == 1023 / 255.0 and noise.code_scale(8, noise.FULL) == 1.0
    # the median falls into bin 0: counts 60, 40 -> N / 2 = 50 is reached in bin 0: med = 0.5 * 50 / 60
    h0 = empty.copy()
    h0[:2] = [60, 40]
    assert noise.hist_median(h0) == 0.5 * 50 / 60
    # the function and the plain-loop restatement of the tests agree on random histograms
    rng = np.random.default_rng(3)
    for name, fmt in N.FORMATS.items():
        for _ in range(20):
            hh = np.zeros(N.nbins(fmt.bits), np.uint32)
            k = int(rng.integers(1, 200))
            hh[:k] = rng.integers(0, 5000, k)
            a, b = noise.frame_sigma(hh, fmt.bits, fmt.matrix, fmt.range), N.sigma_ref(hh, fmt)
            assert (a is None and b is None) or abs(a - b) <= 1e-12 * max(1.0, b), (name, a, b)


def test_histogram_restatement_counts_whole_unclipped_blocks_only():
    fmt = R.Fmt(8, R.C444, R.BT709, R.LIMITED)
    Y = np.array([[20, 30, 16, 40, 99], [25, 50, 60, 70, 99], [200, 235, 100, 90, 99]])          # 3 x 5: the last row and column are in no block
    p = R.join_planes(Y, np.full((3, 5), 128), np.full((3, 5), 128), fmt)[None]
    h = N.hist_ref(p, fmt, 3, 5, 16, 235)
    assert h.shape == (1, 511) and h.dtype == np.uint32
    assert int(h.sum()) == 1 and h[0, abs(20 - 30 - 25 + 50)] == 1                                # the second block holds a 16: not strictly above lo
    assert int(N.hist_ref(p, fmt, 3, 5, 0, 255).sum()) == 2
    assert int(N.hist_ref(p[:, :], fmt, 3, 5, 16, 50).sum()) == 0                                 # 50 is not strictly below hi
    assert N.hist_ref(p[:, :15], fmt, 1, 5, 0, 255).sum() == 0 and N.hist_ref(p[:, :9], fmt, 3, 1, 0, 255).sum() == 0    # H < 2, W < 2: no block


# ---- 3. the restorer's and the command line's logic -------------------------------------------------------------------------------------
def test_window_sigma_leaves_out_none_and_clamps():
    assert noise.window_sigma([None, 4.0, None, 10.0, 6.0]) == 6.0
    assert noise.window_sigma([None, 4.0, 10.0]) == 7.0                                           # numpy's median of two
    assert noise.window_sigma([None, None]) == 0.0 and noise.window_sigma([]) == 0.0
    assert noise.window_sigma([70.0, 80.0, None]) == 50.0                                         # the default clamp: (0, 50)
    assert noise.window_sigma([1.0], (2.0, 30.0)) == 2.0 and noise.window_sigma([40.0], (2.0, 30.0)) == 30.0
    assert noise.window_sigma([None], (2.0, 30.0)) == 2.0                                         # 0 is clamped as well
    for bad in ((-1.0, 5.0), (6.0, 5.0), (float("nan"), 5.0), (1.0,)):
        with pytest.raises(ValueError):
            noise.window_sigma([1.0], bad)


class _Net:
    """As much of a GShiftNet as VideoRestorer looks at before it asks for the device."""

    def __init__(self, denoise):
        self.V = types.SimpleNamespace(denoise=denoise, topo="s")

    def parameters(self):
        import torch
        return iter([torch.zeros(1)])


def test_restorer_sigma_forms():
    with pytest.raises(ValueError, match="denoise variants"):
        restore.VideoRestorer(_Net(False), 4, sigma="auto")
    with pytest.raises(ValueError, match="denoise variants"):
        restore.VideoRestorer(_Net(False), 4, sigma=[10.0, 12.0])
    with pytest.raises(ValueError, match="HIP device"):                                           # a number is ignored there: the next check speaks
        restore.VideoRestorer(_Net(False), 4, sigma=10.0)
    with pytest.raises(ValueError, match="sigma is required"):
        restore.VideoRestorer(_Net(True), 4)
    for good in ("auto", [10.0, 12.5], (3,), 10, 10.5, np.float32(3.0), np.array([1.0, 2.0])):    # accepted: the device check is what refuses
        with pytest.raises(ValueError, match="HIP device"):
            restore.VideoRestorer(_Net(True), 4, sigma=good)
    for bad in ("Auto", "10", [1.0, -2.0], [float("nan")], [1.0, "auto"]):
        with pytest.raises(ValueError, match="sigma"):
            restore.VideoRestorer(_Net(True), 4, sigma=bad)
    with pytest.raises(ValueError, match="sigma_clamp"):
        restore.VideoRestorer(_Net(True), 4, sigma="auto", sigma_clamp=(5.0, 1.0))


def test_per_window_list_running_short_names_the_window():
    mode, sigma = restore.sigma_form([10.0, 12.5])
    assert mode == "list" and isinstance(sigma, restore.PerWindow) and sigma.at(0) == 10.0 and sigma.at(1) == 12.5
    with pytest.raises(ValueError, match="sigma lists 2 windows, window 2 has no entry"):
        sigma.at(2)
    assert restore.sigma_form(10)[1].at(0) == restore.sigma_form(10)[1].at(99) == 10.0            # one value for the stream never runs out
    part, run = restore_parts.NoiseLevel(mode, sigma), restore._Run()                             # the restorer's record of what every window used
    assert part.level(None, 9, run) == (10.0, None) and part.level(None, 9, run) == (12.5, None)
    with pytest.raises(ValueError, match="window 2"):
        part.level(None, 9, run)
    assert run.window_sigma == [10.0, 12.5]


def test_sigma_list_format_round_trip_and_refusals():
    vals = [0.0, 10.0, 12.345678901234567, 1 / 3, 49.99999999999999]
    text = noise.format_sigmas(vals, "auto")
    assert text.startswith("#") and noise.parse_sigmas(text) == vals                              # the same float64s, not nearly the same
    assert noise.parse_sigmas(noise.format_sigmas([])) == [] and noise.parse_sigmas("") == []
    assert noise.parse_sigmas("# c\n10\n\n 12.5 # second window\r\n3e1\n") == [10.0, 12.5, 30.0]
    for text, line in (("x\n", 1), ("10\n-1\n", 2), ("1 2\n", 1), ("5\n# c\nnan\n", 3), ("inf\n", 1), ("auto\n", 1)):
        with pytest.raises(ValueError, match=f"line {line}:"):
            noise.parse_sigmas(text)


def test_parser_takes_a_number_auto_or_a_file():
    ap = restore.make_parser()
    base = ["--variant", "denoise_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["-", "-"])
    assert a.sigma is None and tuple(a.sigma_clamp) == (0.0, 50.0) and a.sigma_out is None
    for word, want in (("10", 10.0), ("10.5", 10.5), ("auto", "auto"), ("sig.txt", "sig.txt")):
        got = ap.parse_args(base + ["--sigma", word, "-", "-"]).sigma
        assert got == want and type(got) is type(want), word
    a = ap.parse_args(base + ["--sigma", "auto", "--sigma_clamp", "2", "30", "--sigma_out", "s.txt", "-", "-"])
    assert (a.sigma, list(a.sigma_clamp), a.sigma_out) == ("auto", [2.0, 30.0], "s.txt")


def test_restore_video_refuses_bad_sigma_arguments_before_it_touches_the_device(tmp_path):
    exe = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--checkpoint", "synthetic"]
    run = lambda args: subprocess.run(exe + args + ["-", "-"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)   # noqa: E731
    bad = tmp_path / "sig.txt"
    bad.write_text("10\nten\n")
    r = run(["--variant", "denoise_small", "--sigma", str(bad)])
    assert r.returncode == 2 and "line 2" in r.stderr
    r = run(["--variant", "denoise_small", "--sigma", str(tmp_path / "missing.txt")])
    assert r.returncode == 2 and "--sigma" in r.stderr
    r = run(["--variant", "deblur_small", "--sigma", "auto"])
    assert r.returncode == 2 and "denoise" in r.stderr
    r = run(["--variant", "denoise_small", "--sigma", "auto", "--sigma_clamp", "9", "3"])
    assert r.returncode == 2 and "sigma_clamp" in r.stderr
    r = run(["--variant", "denoise_small"])                                                        # still required
    assert r.returncode == 2 and "--sigma" in r.stderr


# ---- 4. accuracy against the injected sigma -----------------------------------------------------------------------------------------------
def _estimate(clip: str, s: float, fmt: R.Fmt, h: int = 720, w: int = 1280) -> float:
    p = N.noisy_payloads(N.CLIPS[clip](h, w)[None], s, fmt, seed=0)
    lo, hi = N.clip_codes(fmt)
    assert (lo, hi) == noise.clip_codes(fmt.bits, fmt.range)
    return noise.frame_sigma(N.hist_ref(p, fmt, h, w, lo, hi)[0], fmt.bits, fmt.matrix, fmt.range)


@pytest.mark.parametrize("name", list(N.FORMATS))
@pytest.mark.parametrize("clip", ["smooth", "checkerboard"])
def test_estimate_is_the_injected_sigma_within_the_margin(clip, name):
    """1280 x 720, seed 0.  |estimate - s| <= max(0.25, 0.03 s) for s <= 30; at 40 and 50 only 0.90 s <= estimate <= 1.02 s: the clipping of
    R'G'B' to [0, 1] removes noise before the estimator sees it, so it reads low by construction."""
    fmt = N.FORMATS[name]
    got = {s: _estimate(clip, float(s), fmt) for s in (0, 2, 5, 10, 20, 30, 40, 50)}
    print(f"{clip}, {name}: " + ", ".join(f"{s}: {v:.2f}" for s, v in got.items()))
    for s in (0, 2, 5, 10, 20, 30):
        assert abs(got[s] - s) <= N.margin(s), (clip, name, s, got[s])
    for s in (40, 50):
        assert 0.90 * s <= got[s] <= 1.02 * s, (clip, name, s, got[s])


def test_the_two_level_clip_of_the_gpu_test_reads_near_each_level_on_the_host():
    """tests/test_gpu_noise.py restores this clip with sigma="auto" and asserts these window sigmas exactly; here: that they are near 5 and 30."""
    c = N.TWO_LEVEL
    pay = N.two_level_payloads()
    lo, hi = N.clip_codes(N.FMT420)
    hist = N.hist_ref(pay, N.FMT420, c["h"], c["w"], lo, hi)
    per = [noise.frame_sigma(x, 8, N.FMT420.matrix, N.FMT420.range) for x in hist]
    ws = [noise.window_sigma([per[i] for i in idx]) for idx in N.window_inputs(c["n"], c["one_len"])]
    print("two-level clip, window sigmas:", [round(x, 3) for x in ws])
    assert len(ws) == 6
    for k in (0, 1):                                        # input frames 0 .. 11: all sigma 5
        assert abs(ws[k] - 5.0) <= N.margin(5.0), (k, ws[k])
    for k in (3, 4, 5):                                     # input frames 13 .. 25: all sigma 30
        assert abs(ws[k] - 30.0) <= N.margin(30.0), (k, ws[k])
    assert 5.0 - N.margin(5.0) <= ws[2] <= 30.0 + N.margin(30.0)      # frames 8 .. 16: five of one level, four of the other
