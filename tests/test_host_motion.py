"""CPU: the motion-compensated temporal noise estimate (shiftnet_amd/noise.py): that the library exports the three entry points
without an ABI bump, the numpy restatement of tests/motion_ref.py on hand-made frames with known answers, the accuracy of the scheme against the
INJECTED sigma on synthetic clips (never against a second run of the estimator), the bias that the checkerboard split removes, and the forms of the
restorer's and the command line's new option."""
import importlib.util
import inspect
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import motion_ref as M
import noise_pairs_ref as NP
import noise_ref as N
import yuv_ref as R
from shiftnet_amd import noise, restore, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = R.Fmt(8, R.C444, R.BT709, R.LIMITED)


# ---- 1. the library and the module ----------------------------------------------------------------------------------------------------------
def test_library_exports_the_three_entry_points_and_keeps_the_abi_version():
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()                                              # hipcc cross-compiles gfx950 without a GPU
    from shiftnet_amd import lib as L
    lib = L.load()
    for name in ("sn_yuv_block_motion", "sn_yuv_noise_hist_pairs_mv", "sn_yuv_noise_hist_pairs_bands_mv"):
        assert hasattr(lib, name) and name in L.SYMBOLS
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20
    with open(os.path.join(ROOT, "include", "shiftnet_hip.h")) as fh:
        header = fh.read()
    assert "#define SN_ABI_VERSION 20 " in header
    assert "int sn_yuv_block_motion(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, int8_t* mv, uint32_t* sad," in header
    for name in ("sn_yuv_noise_hist_pairs_mv", "sn_yuv_noise_hist_pairs_bands_mv"):
        assert f"int {name}(const uint8_t* src, const sn_yuv_fmt* fmt, const sn_yuv_rect* rect /* NULL: whole frame */, const int8_t* mv," in header
    assert noise.ESTIMATORS == ("spatial", "temporal", "min")      # the option is no fourth estimator


def test_motion_grid_and_summary():
    assert noise.MOTION_BLOCK == 16 == 2 * M.BLOCK and noise.MOTION_RANGE == 7 == M.RANGE and len(M.CANDIDATES) == 225
    assert M.CANDIDATES[:5] == [(0, 0), (-1, 0), (0, -1), (0, 1), (1, 0)] and M.CANDIDATES[-1] == (7, 7)
    for h, w in ((2, 2), (1, 5), (5, 1), (16, 16), (17, 16), (18, 34), (37, 70), (64, 96), (32, 288), (720, 1280), (0, 0)):
        assert noise.motion_grid(h, w) == M.grid(h, w), (h, w)
    assert noise.motion_grid(16, 16) == (1, 1) and noise.motion_grid(18, 34) == (2, 3) and noise.motion_grid(720, 1280) == (45, 80)
    assert noise.motion_grid(1, 5) == (0, 0) == noise.motion_grid(5, 1)
    assert 19 * 45 * 80 * 2 == 136800                              # the vectors of a 720p window of 20 frames: 137 KB
    rng = np.random.default_rng(3)
    mv = rng.integers(-7, 8, (3, 4, 5, 2)).astype(np.int8)
    mv[1] = 0
    mv[2, :, :, 1] = 0
    got = noise.motion_summary(mv)
    assert got == M.summary_ref(mv) and got[1] == (0.0, 0.0, 0.0) and got[2][2] == 0.0 and 0.0 < got[0][0] <= 1.0
    assert all(isinstance(x, float) for t in got for x in t)
    assert noise.motion_summary(np.zeros((2, 0, 0, 2), np.int8)) == [(0.0, 0.0, 0.0)] * 2 == M.summary_ref(np.zeros((2, 0, 0, 2), np.int8))
    one = np.zeros((1, 1, 2, 2), np.int8)
    one[0, 0, 0] = (3, -2)
    assert noise.motion_summary(one) == [(0.5, 1.5, -1.0)] == M.summary_ref(one)


# ---- 2. known answers of the restatement ------------------------------------------------------------------------------------------------------
def _canvas(seed=1, n=96):
    return np.random.default_rng(seed).integers(20, 230, (n, n)).astype(np.int64)


def test_a_shifted_frame_gives_its_vector_in_every_interior_block_and_sad_zero():
    C, h, w, m = _canvas(), 64, 64, 8
    Y0 = C[m:m + h, m:m + w]
    for dy, dx in ((0, 0), (7, 7), (-7, -7), (7, -7), (-7, 7), (3, -2), (0, 5), (-1, 0)):
        Y1 = C[m - dy:m - dy + h, m - dx:m - dx + w]                # Y1(y + dy, x + dx) = Y0(y, x)
        mv, sad = M.motion_pair(Y0, Y1)
        assert mv.shape == (4, 4, 2) and mv.dtype == np.int8 and sad.shape == (4, 4) and sad.dtype == np.uint32
        assert (mv[1:3, 1:3] == (dy, dx)).all() and (sad[1:3, 1:3] == 0).all(), (dy, dx)
        if (dy, dx) == (7, 7):                                      # the last block cannot follow: (7, 7) is not admissible there
            assert tuple(mv[3, 3]) != (7, 7) and sad[3, 3] > 0 and tuple(mv[0, 0]) == (7, 7)


def test_constant_frames_and_stripes_follow_the_tie_rule():
    Y = np.full((40, 72), 100, np.int64)
    mv, sad = M.motion_pair(Y, Y)
    assert not mv.any() and not sad.any()                           # 225 candidates with SAD 0: (0, 0) is the first in the order
    x = np.arange(72)
    S0 = np.repeat((60 + 30 * (x % 4))[None], 40, axis=0)
    mv, sad = M.motion_pair(S0, S0)
    assert not mv.any() and not sad.any()                           # dx = -4, 0, 4 and every dy fit: (0, 0)
    S1 = np.repeat((60 + 30 * ((x - 6) % 4))[None], 40, axis=0)      # moved 6 to the right: dx = -6, -2, 2, 6 fit, with every admissible dy
    mv, sad = M.motion_pair(S0, S1)
    assert not sad.any() and (mv[:, 1:] == (0, -2)).all()           # the nearest alias, and of (0, -2), (0, 2) the one that comes first
    assert (mv[:, 0] == (0, 2)).all()                               # the left column cannot look to the left


def test_a_16_x_16_picture_is_one_block_for_which_only_the_zero_vector_is_admissible():
    rng = np.random.default_rng(2)
    Y0, Y1 = rng.integers(0, 65536, (16, 16)).astype(np.int64), rng.integers(0, 65536, (16, 16)).astype(np.int64)      # words as a 16-bit payload may hold
    mv, sad = M.motion_pair(Y0, Y1)
    want = sum(abs(int(Y0[y, x]) - int(Y1[y, x])) for y in range(16) for x in range(16) if (y // 2 + x // 2) % 2 == 0)
    assert mv.shape == (1, 1, 2) and not mv.any() and int(sad[0, 0]) == want
    assert want * 256 + 224 < 2 ** 32                               # the key of the device's reduction fits
    mv17, sad17 = M.motion_pair(np.pad(Y0, ((0, 1), (0, 0))), np.pad(Y1, ((0, 1), (0, 0))))      # 17 rows: (1, 0) is admissible as well
    assert int(sad17[0, 0]) <= want


def test_pictures_without_a_whole_block_have_empty_grids():
    for h, w in ((1, 5), (5, 1), (1, 1)):
        p = np.zeros((3, R.frame_bytes(F8, h, w)), np.uint8)
        mv, sad = M.block_motion_ref(p, F8, h, w)
        assert mv.shape == (2, 0, 0, 2) and sad.shape == (2, 0, 0)
        assert M.hist_pairs_mv_ref(p, mv, F8, h, w, 0, 255).sum() == 0 and M.hist_pairs_bands_mv_ref(p, mv, F8, h, w, 0, 255).sum() == 0


def _frames(*Ys):
    return np.stack([R.join_planes(np.asarray(Y), np.full(np.shape(Y), 128), np.full(np.shape(Y), 128), F8) for Y in Ys])


def test_only_measuring_blocks_count_and_one_displaced_outside_the_picture_does_not():
    rng = np.random.default_rng(4)
    Y0, Y1 = rng.integers(30, 200, (16, 16)), rng.integers(30, 200, (16, 16))
    p = _frames(Y0, Y1)
    zero = np.zeros((1, 1, 1, 2), np.int8)
    h0 = M.hist_pairs_mv_ref(p, zero, F8, 16, 16, 16, 235)
    assert int(h0.sum()) == 32                                      # half of the 64 blocks
    every = NP.hist_pairs_ref(p, F8, 16, 16, 16, 235)
    both = M.hist_pairs_mv_ref(p, zero, F8, 16, 16, 16, 235, split=False)
    assert np.array_equal(both, every) and int(every.sum()) == 64   # the zero vector on every block is the plain pair histogram
    i, j = 0, 1                                                     # a measuring block by hand
    v = abs(int(Y1[0, 2]) - int(Y1[0, 3]) - int(Y1[1, 2]) + int(Y1[1, 3]) - (int(Y0[0, 2]) - int(Y0[0, 3]) - int(Y0[1, 2]) + int(Y0[1, 3])))
    assert h0[0, v] >= 1 and (i + j) % 2 == 1
    up = zero.copy()
    up[..., 0] = -1                                                 # one row up: the four measuring blocks of block row 0 leave the picture
    assert int(M.hist_pairs_mv_ref(p, up, F8, 16, 16, 16, 235).sum()) == 28
    left = zero.copy()
    left[..., 1] = -2                                               # block column 0 leaves it
    assert int(M.hist_pairs_mv_ref(p, left, F8, 16, 16, 16, 235).sum()) == 28
    for far in ((127, 0), (-128, 5), (0, 127), (15, 0), (0, -16)):
        m = zero.copy()
        m[0, 0, 0] = far
        assert int(M.hist_pairs_mv_ref(p, m, F8, 16, 16, 16, 235).sum()) == 0 == int(M.hist_pairs_bands_mv_ref(p, m, F8, 16, 16, 16, 235).sum())
    down = zero.copy()
    down[..., 0] = 14                                               # only block row 0 stays inside, and reads rows 14, 15 of the second frame
    h = M.hist_pairs_mv_ref(p, down, F8, 16, 16, 16, 235)
    v = abs(int(Y1[14, 2]) - int(Y1[14, 3]) - int(Y1[15, 2]) + int(Y1[15, 3]) - (int(Y0[0, 2]) - int(Y0[0, 3]) - int(Y0[1, 2]) + int(Y0[1, 3])))
    assert int(h.sum()) == 4 and h[0, v] >= 1
    bands = M.hist_pairs_bands_mv_ref(p, zero, F8, 16, 16, 16, 235)  # the same blocks, split by band and saturated
    assert bands.shape == (1, 16, 128) and np.array_equal(bands.sum(axis=1)[:, :127], h0[:, :127])


def test_the_restatement_of_a_rectangle_is_that_of_the_cropped_payloads():
    import picture_ref as P
    rng = np.random.default_rng(6)
    H, W, rect = 37, 70, (16, 2, 40, 30)
    p = _frames(*[rng.integers(16, 236, (H, W)) for _ in range(3)])
    mv, sad = M.block_motion_ref(p, F8, H, W, rect)
    crop = P.crop_payloads(p, F8, H, W, rect)
    cmv, csad = M.block_motion_ref(crop, F8, rect[3], rect[2])
    assert mv.shape == (2, 2, 3, 2) and np.array_equal(mv, cmv) and np.array_equal(sad, csad)
    assert np.array_equal(M.hist_pairs_mv_ref(p, mv, F8, H, W, 16, 235, rect), M.hist_pairs_mv_ref(crop, cmv, F8, rect[3], rect[2], 16, 235))


# ---- 3. accuracy against the injected sigma -------------------------------------------------------------------------------------------------
# Measured with tests/motion_ref.py (its __main__ prints the table of DESIGN.md 3.23): over the six whole-pel clips, sigma 2, 5, 10, 20, 30 and seeds
# 0 .. 2 the compensated estimate deviates from the injected sigma by at most 3.16 % (texture moving 1 px down and 2 px right, sigma 30, seed 2).  Twice
# that is 6.3 %; the bound may not exceed 5 %, so 5 % it is, with 0.1 absolute at sigma 2 (which is the same number there).
BOUND, BOUND_ABS = 0.05, 0.1


@pytest.fixture(scope="module")
def table():
    """(plain temporal, compensated) per whole-pel clip, injected sigma and seed: 180 x 320, five frames, BT.709 limited 8 bit.  Computed once, left unchanged."""
    out = {(clip, s, seed): M.clip_estimates(clip, s, seed) for clip in M.WHOLE for s in M.SIGMAS for seed in M.SEEDS}
    for clip in M.WHOLE:
        print(f"{clip}: " + "; ".join(f"{s}: plain {out[clip, s, 0][0]:.2f} compensated " + " / ".join(f"{out[clip, s, k][1]:.2f}" for k in M.SEEDS)
                                      for s in M.SIGMAS))
    print("largest relative deviation: %.2f %%" % (100 * max(abs(v[1] - k[1]) / k[1] for k, v in out.items())))
    return out


def test_compensated_estimate_reads_the_injected_sigma_on_every_whole_pel_clip(table):
    for (clip, s, seed), (plain, comp) in table.items():
        assert abs(comp - s) <= max(BOUND * s, BOUND_ABS if s == 2 else 0.0), (clip, s, seed, plain, comp)


def test_compensated_estimate_is_closer_than_the_plain_one_where_the_texture_moves(table):
    for clip in ("texture, 1 px per frame", "texture, 3 px per frame"):
        for s in M.SIGMAS:
            for seed in M.SEEDS:
                plain, comp = table[clip, s, seed]
                assert abs(comp - s) < abs(plain - s), (clip, s, seed, plain, comp)
    for s in (2, 5, 10):                                            # the defect the option exists for: the plain estimate reads the motion
        assert table["texture, 1 px per frame", s, 0][0] > 1.2 * s and table["texture, 3 px per frame", s, 0][0] > 1.9 * s


def test_measuring_where_the_vector_was_chosen_reads_low_on_flat_content():
    """The reason for the split, kept visible: with split=False the vector with the smallest SAD among 225 also fits the noise of the pixels the
    statistic is then taken from."""
    plain, every = M.clip_estimates("flat 0.5", 10, 0, split=False)
    assert every < 0.95 * 10 and abs(plain - 10) <= N.margin(10), (plain, every)


def test_sub_pixel_motion_is_a_stated_limit_that_still_beats_the_plain_estimate():
    """0.5 px per frame reads 5.22 at an injected 5 (4.5 % high, 22 % at sigma 2): no vector fits a half-pel shift.  Reported, not bounded."""
    for clip in M.FRACTIONAL:
        plain, comp = M.clip_estimates(clip, 5, 0)
        print(f"{clip}: sigma 5: plain {plain:.2f} compensated {comp:.2f}")
        assert 5.0 < comp < plain


# ---- 4. the restorer's and the command line's forms ---------------------------------------------------------------------------------------
class _Net:
    """As much of a GShiftNet as VideoRestorer looks at before it asks for the device."""

    def __init__(self, denoise):
        self.V = types.SimpleNamespace(denoise=denoise, topo="s")

    def parameters(self):
        import torch
        return iter([torch.zeros(1)])


def test_sigma_motion_form_and_the_restorer_argument():
    for est in ("temporal", "min"):
        assert windows.sigma_motion_form("blocks", est) == "blocks" == restore.sigma_motion_form("blocks", est)
    for est in noise.ESTIMATORS:
        assert windows.sigma_motion_form(None, est) is None
    for bad in ("Blocks", "none", "", "auto", 1, True, ["blocks"], ("blocks",)):
        with pytest.raises(ValueError, match="sigma_motion"):
            windows.sigma_motion_form(bad, "min")
        with pytest.raises(ValueError, match="sigma_motion"):
            restore.VideoRestorer(_Net(True), 4, sigma="auto", sigma_estimator="min", sigma_motion=bad)
    with pytest.raises(ValueError, match=r"sigma_motion.*sigma_estimator"):                     # the message names both options
        windows.sigma_motion_form("blocks", "spatial")
    with pytest.raises(ValueError, match=r"sigma_motion.*sigma_estimator"):
        restore.VideoRestorer(_Net(True), 4, sigma="auto", sigma_motion="blocks")
    with pytest.raises(ValueError, match=r"sigma_motion.*sigma_estimator"):
        restore.VideoRestorer(_Net(True), 4, sigma=10.0, sigma_motion="blocks")
    with pytest.raises(ValueError):                                                             # a deblur variant has no sigma to estimate
        restore.VideoRestorer(_Net(False), 4, sigma_motion="blocks")
    for est in ("temporal", "min"):
        with pytest.raises(ValueError, match=r"sigma_estimator.*sigma='auto'"):                 # the estimator's own check speaks first
            restore.VideoRestorer(_Net(True), 4, sigma=10.0, sigma_estimator=est, sigma_motion="blocks")
        with pytest.raises(ValueError, match="HIP device"):                                     # accepted: the device check is what refuses
            restore.VideoRestorer(_Net(True), 4, sigma="auto", sigma_estimator=est, sigma_motion="blocks")
        with pytest.raises(ValueError, match="HIP device"):
            restore.VideoRestorer(_Net(True), 4, sigma="auto", sigma_estimator=est, sigma_motion="blocks", noise_model="level")
        with pytest.raises(ValueError, match="HIP device"):
            restore.VideoRestorer(_Net(True), 4, sigma="auto", sigma_estimator=est, sigma_motion=None)


def test_the_option_is_off_by_default_and_a_run_starts_without_motion_records():
    """That the slots of a restorer without the option hold no motion buffers needs a device: tests/test_gpu_motion.py looks at them."""
    assert inspect.signature(restore.VideoRestorer.__init__).parameters["sigma_motion"].default is None
    assert restore._Run().launches["motion"] == 0 and restore._Run().window_pair_motion == []


def test_parser_takes_the_option_and_restore_video_refuses_it_without_a_temporal_estimator(tmp_path):
    ap = restore.make_parser()
    base = ["--variant", "denoise_small", "--checkpoint", "synthetic", "--sigma", "auto"]
    assert ap.parse_args(base + ["-", "-"]).sigma_motion == "none"
    assert ap.parse_args(base + ["--sigma_estimator", "min", "--sigma_motion", "blocks", "-", "-"]).sigma_motion == "blocks"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--sigma_motion", "pixels", "-", "-"])
    exe = [sys.executable, os.path.join(ROOT, "inference", "restore_video.py"), "--checkpoint", "synthetic", "--variant", "denoise_small"]
    run = lambda args: subprocess.run(exe + args, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=300)   # noqa: E731
    missing = str(tmp_path / "missing.y4m")                                                      # refused before the input is looked for
    r = run(["--sigma", "auto", "--sigma_motion", "blocks", missing, "-"])
    assert r.returncode == 2 and "--sigma_motion blocks needs --sigma_estimator temporal or min" in r.stderr
    r = run(["--sigma", "auto", "--sigma_estimator", "spatial", "--sigma_motion", "blocks", missing, "-"])
    assert r.returncode == 2 and "--sigma_motion blocks needs --sigma_estimator temporal or min" in r.stderr
    r = run(["--sigma", "10", "--sigma_estimator", "min", "--sigma_motion", "blocks", missing, "-"])      # the neighbouring check speaks first
    assert r.returncode == 2 and "--sigma_estimator min needs --sigma auto" in r.stderr
    r = run(["--sigma", "auto", "--sigma_estimator", "min", "--sigma_motion", "pixels", missing, "-"])
    assert r.returncode == 2 and "--sigma_motion" in r.stderr
