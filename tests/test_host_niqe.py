"""CPU tests of the host part of the NIQE score (shiftnet_amd/niqe.py) against what the reference implementation recorded
(tests/golden/niqe_cases.npz, made by tools/make_niqe_golden.py from the generators of tests/niqe_cases.py): the fit of a block from its five sums per
map, the score of a frame from the float64 restatement of the device sums (tests/niqe_ref.py), the NaN rule, the shape lookup, the model file, and the
refusals of the C entry point, of ``quality_form`` and of the command line.

Tolerances, measured here against the fixtures (DESIGN.md 3.33 has the list):
  * features other than the shapes: the reference fits the float32 blocks of the fixture in float32 (numpy's mean of a float32 array), the sums here are
    float64 -- largest relative difference 1.5e-5 (laplace96), asserted at 5e-5;
  * scores: restatement and reference are both float64 and differ by the order of their sums -- largest relative difference 2.0e-14, and 6.2e-10 on
    the full-range case, where the restatement scales the codes by the kernel's float32 constant (219 / 255 rounded once: 3e-8 relative) -- asserted
    at 2e-9.  On the near-flat, mixed and clipped cases and the 10-bit rectangle: 7.1e-12 at limited range, where the reference's own float64
    m2 - mu mu has lost digits the restatement keeps, and 1.6e-9 / 4.9e-9 on the 8-bit / 10-bit full-range levels (the float32 constant again, on
    variances of a code) -- asserted at 10 times the largest, 5e-8;
  * the restatement against the plain long-double reference, both with the model's float64 taps: every count equal, largest relative difference
    of a sum 2.7e-12 (10-bit full range at level 1000; 1.7e-12 at level 230, 5e-13 at 128, 1e-14 at 20, 2e-15 on the textured cases: it grows with
    the square of the level, as the cancellation in the long-double reference's own m2 - mu mu does -- the restatement filters deviations and does
    not see the level) -- asserted at 10 times that, 3e-11."""
import os
import re
import warnings

import numpy as np
import pytest

import niqe_cases as K
import niqe_ref as NR
from shiftnet_amd import niqe as N
from shiftnet_amd import restore_cli, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FEATURE_RTOL = 5e-5
SCORE_RTOL = 2e-9                                              # the ten textured cases
NEW_SCORE_RTOL = 5e-8                                          # the near-flat, mixed and clipped cases and the 10-bit rectangle
PLAIN_RTOL = 3e-11
SHAPES = [0, 2, 6, 10, 14]                                     # the alphas among a block's 18 features
OTHERS = [i for i in range(18) if i not in SHAPES]


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(GOLDEN, "niqe_cases.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def model():
    return N.load_params(N.default_params_path())


@pytest.fixture(scope="module")
def restated(model):
    """case name -> per frame the float64 restatement's sums [2, nbh, nbw, 5, 5], with the model's float64 taps: computed once, read by every test."""
    win7 = model[2]
    return {c.name: [NR.sums_of_luma(K.picture(c, Y), c.fmt, win7) for Y in K.frames(c)] for c in K.CASES + K.PARTLY_FLAT}


def test_the_default_model_is_the_fixture_and_its_window_is_separable_and_symmetric(model):
    mu, cov, win7 = model
    assert N.default_params_path() == os.path.join(GOLDEN, "niqe_pris_params.npz")
    assert mu.shape == (36,) and cov.shape == (36, 36) and win7.shape == (7,) and all(a.dtype == np.float64 for a in model)
    assert abs(win7.sum() - 1.0) < 1e-15 and np.array_equal(win7, win7[::-1])
    assert os.path.getsize(N.default_params_path()) < 16384 and os.path.getsize(os.path.join(GOLDEN, "niqe_cases.npz")) < 16384


def test_load_params_refuses_a_window_that_is_not_separable_and_a_file_that_is_no_model(tmp_path, model):
    with np.load(N.default_params_path()) as z:
        good = {k: z[k] for k in z.files}
    win = good["gaussian_window"].copy()
    win[0, 1] += 1e-9                                           # no longer the outer product of anything, to 1e-12
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, **{**good, "gaussian_window": win})
    with pytest.raises(ValueError, match="outer product"):
        N.load_params(bad)
    win = good["gaussian_window"].copy()
    win[0, 0] += 5e-13                                          # inside the tolerance
    ok = str(tmp_path / "ok.npz")
    np.savez(ok, **{**good, "gaussian_window": win})
    assert N.load_params(ok)[2].shape == (7,)
    short = str(tmp_path / "short.npz")
    np.savez(short, **{**good, "mu_pris_param": good["mu_pris_param"][:, :18]})
    with pytest.raises(ValueError, match="36"):
        N.load_params(short)


def test_the_table_is_the_grid_and_increases_and_bisection_is_the_argmin():
    a, rho = N.gamma_table()
    assert len(a) == 9801 and a[0] == 0.2 and abs(a[-1] - 10.0) < 1e-9 and (np.diff(rho) > 0).all()
    rng = np.random.default_rng(7)
    # inside the table, beyond both ends, on grid points and on midpoints between them
    xs = np.concatenate([rng.uniform(rho[0], rho[-1], 9000), rng.uniform(-0.1, rho[0], 300), rng.uniform(rho[-1], 1.2, 300),
                         rho[rng.integers(0, len(rho), 200)], (rho[:-1] + rho[1:])[rng.integers(0, len(rho) - 1, 200)] / 2])
    assert len(xs) == 10 ** 4
    for x in xs:
        assert N.nearest_shape(float(x)) == int(np.argmin((rho - x) ** 2)), x
    assert N.nearest_shape(float("nan")) == 0                   # what an argmin over an all-NaN array returns


def test_block_features_of_the_restated_sums_are_the_references_features(recorded):
    worst = 0.0
    for name, block in K.feature_blocks():
        want = recorded["feature/" + name]
        got = N.block_features(NR.map_sums(block), block.shape[0])
        assert got.shape == (18,) and np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.nanmax(np.abs(got[SHAPES] - want[SHAPES])) <= 0.001 + 1e-12, (name, got[SHAPES], want[SHAPES])      # one step of the grid
        fin = [i for i in OTHERS if not np.isnan(want[i])]
        rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
        worst = max(worst, float(rel.max()))
        assert rel.max() <= FEATURE_RTOL, (name, rel)
    print(f"largest relative difference of a feature: {worst:.3g}")
    # the block that is positive everywhere: every map has an empty side, the shape falls to the first grid point and the fitted side stays finite
    got = N.block_features(NR.map_sums(dict(K.feature_blocks())["positive96"]), 96)
    assert (got[SHAPES] == 0.2).all() and np.isnan(got[1]) and np.isnan(got[[3, 4]]).all() and got[5] > 0


def test_the_score_of_the_restated_sums_is_the_references_score(recorded, restated, model):
    mu, cov, _ = model
    assert sorted(k[6:] for k in recorded if k.startswith("score/")) == sorted(c.name for c in K.CASES)
    for cases, tol in ((K.TEXTURED, SCORE_RTOL), (K.NEAR_FLAT + K.NEW_FORMATS, NEW_SCORE_RTOL)):
        worst = 0.0
        for c in cases:
            want = recorded["score/" + c.name]
            assert want.shape == (len(c.seeds),) and np.isfinite(want).all()
            for t, sums in enumerate(restated[c.name]):
                rel = abs(N.frame_score(sums, mu, cov) - want[t]) / want[t]
                print(f"{c.name}[{t}]: reference {want[t]:.6f}, relative difference {rel:.3g}")
                worst = max(worst, rel)
                assert rel <= tol, (c.name, t, rel)
        print(f"largest relative difference of a score: {worst:.3g} (asserted at {tol:g})")


def test_the_near_flat_mixed_and_clipped_cases_have_no_constant_window_and_no_map_value_near_zero(model):
    """What the comparisons of counts rest on (tests/niqe_cases.py: NEAR_FLAT).  A constant window is an exact zero with a pivot and a residue without:
    the flat case, tested on its own.  A map value below 1e-9 could lie on the other side of zero in another precision."""
    from numpy.lib.stride_tricks import sliding_window_view
    smallest = np.inf
    for c in K.NEAR_FLAT:
        for Y in K.frames(c):
            lo, hi = K.legal(c.fmt)
            assert lo <= Y.min() and Y.max() <= hi and Y.min() < Y.max(), c.name
            I = NR.values(Y, c.fmt)
            for s in range(2):
                I = NR.halve(I) if s else I
                w = sliding_window_view(np.pad(I, 3, mode="edge"), (7, 7))
                assert (w.max(axis=(2, 3)) > w.min(axis=(2, 3))).all(), (c.name, s)
            for g in (model[2], NR.kernel_taps(model[2])):
                for s, by, bx, n in NR.coefficient_blocks(Y, c.fmt, g):
                    low = min(float(np.abs(m).min()) for m in NR.block_maps(n))
                    assert low >= 1e-9, (c.name, s, by, bx, low)
                    smallest = min(smallest, low)
    print(f"smallest magnitude of a map value: {smallest:.3g}")
    mixed, clipped = K.frames(K.BY_NAME["mixed-40-228"])[0], K.frames(K.BY_NAME["clipped-225-sigma3"])[0]
    assert mixed[:, :48].mean() < 60 and mixed[:, :48].std() > 8 and abs(mixed[:, 48:96].mean() - 228) < 0.1 and mixed[:, 48:96].std() < 1
    assert 0.005 < (clipped == 235).mean() < 0.1                # a share of the samples sits on the legal limit


def test_the_restatement_equals_the_plain_long_double_reference(restated, model):
    """The kernel's arithmetic -- float64, deviations from the block's first sample -- against the formula written down plainly in long double, both
    with the model's float64 taps, on every case that is not flat everywhere.  A flat area is an exact zero in the one and a residue of 1e-17 in the
    other; in the two partly flat cases only the blocks no window of which touches the flat square are compared."""
    assert np.finfo(np.longdouble).nmant >= 63
    worst = 0.0
    for c in K.CASES + K.PARTLY_FLAT:
        for t, Y in enumerate(K.frames(c)):
            got, want = restated[c.name][t], NR.plain_sums_of_luma(K.picture(c, Y), c.fmt, model[2])
            assert got.shape == want.shape
            if c.flat:
                assert (got[:, 0, 0] == 0).all()
                got, want = got[:, :, 2:], want[:, :, 2:]          # FLAT_SIDE reaches into block columns 0 and 1
            assert np.array_equal(got[..., [0, 2]], want[..., [0, 2]]), c.name
            g, w = got[..., [1, 3, 4]], want[..., [1, 3, 4]]
            assert (w > 0).all()
            rel = float((np.abs(g - w) / w).max())
            print(f"{c.name}[{t}]: largest relative difference of a sum {rel:.3g}")
            worst = max(worst, rel)
    print(f"largest relative difference of a sum: {worst:.3g} (asserted at {PLAIN_RTOL:g})")
    assert worst <= PLAIN_RTOL <= 1e-9


def test_a_flat_picture_gives_25_zeros_per_block_and_scale_at_every_code_and_no_score(model):
    mu, cov, win7 = model
    for c in K.FLAT_CASES:
        (Y,) = K.frames(c)
        assert Y.min() == Y.max() == c.level
        for g in (win7, NR.kernel_taps(win7)):
            sums = NR.sums_of_luma(Y, c.fmt, g)
            assert sums.shape == (2, 1, 2, 5, 5) and (sums == 0).all(), c.name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            assert np.isnan(N.frame_score(sums, mu, cov)), c.name
    c = K.BY_NAME["192x288-flat-block-196"]                       # a flat block in a textured frame: block (0, 0) alone is all zeros
    (Y,) = K.frames(c)
    sums = NR.sums_of_luma(Y, c.fmt, NR.kernel_taps(win7))
    assert (Y[:K.FLAT_SIDE, :K.FLAT_SIDE] == 196).all() and (sums[:, 0, 0] == 0).all() and (sums[:, 1:, :, :, [0, 2]].sum(axis=-1) > 9000 / 4).all()


def test_a_block_that_cannot_be_fitted_is_dropped_from_the_covariance_and_the_others_count(restated, model):
    mu, cov, _ = model
    sums = restated["192x288-flat-block"][0]
    assert (sums[:, 0, 0] == 0).all()                           # coefficients of exactly zero at both scales: nothing on either side of any map
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        feat = N.frame_features(sums)
    assert feat.shape == (6, 36)
    bad = np.isnan(feat).any(axis=1)
    assert bad.tolist() == [True] + [False] * 5                 # block (0, 0) comes first in column order too
    assert np.isnan(feat[0][[i + 18 * s for s in range(2) for i in OTHERS]]).all() and (feat[0][[i + 18 * s for s in range(2) for i in SHAPES]] == 0.2).all()
    whole = N.score(feat, mu, cov)
    # the covariance is that of the five other rows; the mean ignores the NaN entries only -- the flat block's shapes of 0.2 still count in it
    clean = feat[1:]
    d = mu - np.nanmean(feat, axis=0)
    assert whole == pytest.approx(float(np.sqrt(d @ np.linalg.pinv((cov + np.cov(clean, rowvar=False)) / 2) @ d)), rel=1e-12)
    assert whole != pytest.approx(N.score(clean, mu, cov), rel=1e-6)
    assert np.isfinite(whole)


def test_fewer_than_two_blocks_that_can_be_fitted_give_nan(restated, model):
    mu, cov, _ = model
    sums = restated["96x192"][0]                                # two blocks
    assert np.isfinite(N.frame_score(sums, mu, cov))
    assert np.isnan(N.frame_score(sums[:, :, :1], mu, cov))     # one
    feat = N.frame_features(sums)
    feat[1, 7] = np.nan                                         # two, one of them with a NaN
    assert np.isnan(N.score(feat, mu, cov)) and np.isnan(N.score(feat[:0], mu, cov))
    with pytest.raises(ValueError):
        N.block_features(np.zeros((5, 4)), 96)


def test_header_build_list_and_library_have_the_new_symbol_and_the_entry_point_refuses_on_the_host():
    import ctypes as C
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_niqe.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_niqe.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    from shiftnet_amd.io_edges import yuv_fmt
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^int sn_yuv_niqe_sums\(const uint8_t\* src, const sn_yuv_fmt\* fmt, const sn_yuv_rect\* rect /\* NULL: whole frame \*/,\s+"
                     r"const float\* win7 /\* device, 7 taps \*/, double\* dst /\* \[T\]\[2\]\[nbh\]\[nbw\]\[5\]\[5\] \*/,\s+"
                     r"int T, int H, int W, void\* stream\);", header, flags=re.M)
    for name, v in (("SN_NIQE_BLOCK", 96), ("SN_NIQE_MAPS", 5), ("SN_NIQE_SUMS", 5)):
        assert re.search(rf"#define {name} {v}\b", header) and getattr(L, name) == v
    assert hasattr(lib, "sn_yuv_niqe_sums") and "sn_yuv_niqe_sums" in L.SYMBOLS and len(lib.sn_yuv_niqe_sums.argtypes) == 9
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    # the argument checks are host side and need no GPU: host memory is refused before anything would read it
    arr = np.zeros(1 << 16, np.uint8)
    buf = arr.ctypes.data + (-arr.ctypes.data) % 16
    src, win, dst = buf, buf + 32768, buf + 49152
    f8, f10 = yuv_fmt(8, L.SN_YUV_444, L.SN_YUV_BT709, L.SN_YUV_LIMITED), yuv_fmt(10, L.SN_YUV_420_CENTER, L.SN_YUV_BT709, L.SN_YUV_LIMITED)
    call = lib.sn_yuv_niqe_sums
    R = L.YuvRect
    refused = [
        (None, f8, None, win, dst, 1, 96, 192), (src, None, None, win, dst, 1, 96, 192), (src, f8, None, None, dst, 1, 96, 192),
        (src, f8, None, win, None, 1, 96, 192),                                                                  # null pointers
        (src, yuv_fmt(12, 0, 0, 0), None, win, dst, 1, 96, 192), (src, yuv_fmt(8, 3, 0, 0), None, win, dst, 1, 96, 192),      # bits, chroma code
        (src, f8, R(0, 0, 0, 96), win, dst, 1, 96, 192), (src, f8, R(100, 0, 96, 96), win, dst, 1, 96, 192),     # an empty rectangle, one past the frame
        (src, f10, R(1, 0, 96, 96), win, dst, 1, 96, 192),                                                       # 4:2:0: an odd origin shares chroma samples
        (src, f8, None, win, dst, 0, 96, 192), (src, f8, None, win, dst, 65536, 96, 192),                        # T
        (src, f8, None, win, dst, 1, 95, 192), (src, f8, None, win, dst, 1, 192, 95), (src, f8, R(0, 0, 192, 95), win, dst, 1, 96, 192),      # no whole block
        (src, f8, None, win, dst + 4, 1, 96, 192), (src, f8, None, win + 2, dst, 1, 96, 192),                    # alignment of dst and of win7
        (src + 1, f10, None, win, dst, 1, 96, 192),                                                              # 10 bit: an odd address
    ]
    for args in refused:
        rect = args[2]
        assert call(args[0], args[1], None if rect is None else C.byref(rect), *args[3:], None) == -22, args


def test_quality_form_and_the_command_line_refuse_what_they_say_they_refuse(tmp_path, capsys, model):
    assert windows.quality_form() is None and windows.quality_form(None, None, True) is None
    got = windows.quality_form("niqe", None, True)
    assert all(np.array_equal(a, b) for a, b in zip(got, model))
    assert np.array_equal(windows.quality_form("niqe", N.default_params_path(), True)[0], model[0])
    for args, word in ((("niqe", None, False), "report=True"), (("brisque", None, True), "report_quality"), ((True, None, True), "report_quality"),
                       ((None, "x.npz", True), "needs that option"), (("niqe", str(tmp_path / "missing.npz"), True), "niqe_params")):
        with pytest.raises(ValueError, match=word):
            windows.quality_form(*args)
    junk = tmp_path / "junk.npz"
    junk.write_bytes(b"not a model")
    with pytest.raises(ValueError, match="niqe_params"):
        windows.quality_form("niqe", str(junk), True)
    ap = restore_cli.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["in.y4m", "out.y4m"])
    assert a.report_quality == "none" and a.niqe_params is None
    a = ap.parse_args(base + ["--report", "r.txt", "--report_quality", "niqe", "--niqe_params", "m.npz", "in.y4m", "out.y4m"])
    assert a.report_quality == "niqe" and a.niqe_params == "m.npz"
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--report_quality", "brisque", "in.y4m", "out.y4m"])
    # judged by main() before any file is opened: the files named here do not exist
    missing = ["/nonexistent/in.y4m", "/nonexistent/out.y4m"]
    for bad, word in ((["--report_quality", "niqe"], "needs --report"),
                      (["--report", "r.txt", "--report_quality", "niqe", "--niqe_params", "/nonexistent/model.npz"], "--niqe_params"),
                      (["--report", "r.txt", "--niqe_params", "m.npz"], "needs that option")):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(base + bad + missing)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, (bad, word)


def test_the_report_file_gains_two_columns_and_reads_back():
    from shiftnet_amd import report as rep
    sums = [1000, 10, 5000, 990, 100, 980, 90, 50, 200, 1500, 250, 1, 300, -2, 280, 0]
    frames = rep.frames_report([sums, sums, sums], [0, 0, 1], [None] * 3, 8, 1, 0)
    pairs = [(5.25, 4.5), (float("nan"), 6.0), (7.75, float("nan"))]
    plain, text = rep.format_report(frames, "edge 16"), rep.format_report(frames, "edge 16", None, pairs)
    lines = text.splitlines()
    cols = [ln for ln in lines if ln.startswith("# frame ")]
    assert len(cols) == 1 and cols[0].split()[-2:] == ["niqe_in", "niqe_out"]
    assert lines[-1].startswith("# median ") and lines[-1].split()[-2:] == [repr(6.5), repr(5.25)]      # medians ignore nan
    body = [ln for ln in lines if not ln.startswith("#")]
    assert [ln.split()[-2:] for ln in body] == [[repr(5.25), repr(4.5)], ["nan", repr(6.0)], [repr(7.75), "nan"]]
    assert [ln.split()[:-2] for ln in body] == [ln.split() for ln in plain.splitlines() if not ln.startswith("#")]
    got = rep.parse_report_quality(text)
    assert got[0] == (5.25, 4.5) and np.isnan(got[1][0]) and got[1][1] == 6.0 and rep.parse_report_quality(plain) == [None] * 3
    assert [f.frame for f in rep.parse_report(text)] == [f.frame for f in frames]
    assert all(np.isnan(v) for v in rep.summarize_quality([]).values())       # the medians of nothing
    with pytest.raises(ValueError):
        rep.format_report(frames, "", None, pairs[:2])
