"""CPU tests of the restoration amount and the removed view: the numpy restatement of ``sn_egress_yuv_mix`` (tests/mix_ref.py) against the same
formulas in float64, its two identities, and the argument forms of the restorer and of the command line.  No GPU."""
import os
import re

import numpy as np
import pytest

import mix_ref as M
import yuv_ref as R
from shiftnet_amd import lib as L
from shiftnet_amd import restore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = [R.Fmt(b, c, m, r) for b in (8, 10) for c in (R.C444, R.C420_CENTER, R.C420_LEFT) for m, r in ((R.BT601, R.LIMITED), (R.BT709, R.FULL))]
IDS = [f"{f.bits}bit-{('444', '420c', '420l')[f.chroma]}-{'709' if f.matrix else '601'}-{'full' if f.range else 'lim'}" for f in FORMATS]
MIXES = [("amount", 0.5, 0.5), ("amount", 0.25, 1.0), ("amount", 1.0, 0.0), ("amount", 0.7, 0.3), ("removed", 1.0, 1.0), ("removed", 4.0, 2.0)]


def tensor(rng, T, Hp, Wp):
    return (rng.random((T, 3, Hp, Wp), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_the_restatement_differs_from_float64_by_at_most_one_code_and_only_next_to_a_tie(fmt):
    """The criterion of tests/test_host_yuv.py for the egress: a code may differ only where the float64 value before the rounding lies within 1e-3
    of a tie between two codes."""
    rng = np.random.default_rng(100 + fmt.bits + 3 * fmt.chroma + fmt.matrix)
    T, H, W = 2, 203, 301
    x = tensor(rng, T, H + 1, W + 3)
    inp = M.random_payloads(fmt, T, H, W, seed=7)
    ch, cw = R.chroma_shape(fmt, H, W)
    for mix in MIXES:
        for dither in (None, (3, 5)):
            got = M.codes(M.egress(x, fmt, H, W, mix, inp, dither), fmt)
            raw, pay = M.egress_f64(x, fmt, H, W, mix, inp, dither)
            want = M.codes(pay, fmt)
            assert got.shape == want.shape == raw.shape == (T, H * W + 2 * ch * cw)
            diff = got != want
            assert np.abs(got - want).max() <= 1, (mix, dither)
            frac = np.abs(raw - np.floor(raw) - 0.5)
            worst = float(frac[diff].max()) if diff.any() else 0.0
            print(f"{fmt} {mix} dither {dither}: {int(diff.sum())} of {diff.size} codes differ, farthest from a tie {worst:.2e}")
            assert worst <= 1e-3, (mix, dither, worst)


@pytest.mark.parametrize("fmt", FORMATS, ids=IDS)
def test_amount_zero_returns_the_input_whatever_its_codes_and_whatever_the_dither(fmt):
    rng = np.random.default_rng(5)
    T, H, W = 2, 35, 67
    x = tensor(rng, T, H + 1, W + 5)
    inp = M.random_payloads(fmt, T, H, W, seed=11)                 # the whole code range: illegal codes included
    c = R.constants(fmt)
    Y = R.split_planes(inp[0], fmt, H, W)[0]
    if fmt.range == R.LIMITED:
        assert (Y < c["ylo"]).any() and (Y > c["yhi"]).any()
    for dither in (None, (1, 0), (0xDEADBEEF, 7)):
        assert np.array_equal(M.egress(x, fmt, H, W, ("amount", 0.0, 0.0), inp, dither), inp)
        assert np.array_equal(M.egress_f64(x, fmt, H, W, ("amount", 0.0, 0.0), inp, dither)[1], inp)
    # one plane kind at zero: that kind is the input's, the other is not
    half = M.egress(x, fmt, H, W, ("amount", 1.0, 0.0), inp)
    assert np.array_equal(M.codes(half, fmt)[:, H * W:], M.codes(inp, fmt)[:, H * W:]) and not np.array_equal(half, inp)


def test_amounts_never_leave_the_legal_range_unless_the_input_already_had():
    fmt = R.Fmt(8, R.C444, R.BT601, R.LIMITED)
    rng = np.random.default_rng(6)
    T, H, W = 1, 64, 64
    x = tensor(rng, T, H, W)
    inp = M.random_payloads(fmt, T, H, W, seed=12)
    c = R.constants(fmt)
    for a in (0.25, 0.5, 1.0):
        for dither in (None, (2, 0)):
            got, cin = M.codes(M.egress(x, fmt, H, W, ("amount", a, a), inp, dither), fmt)[0], M.codes(inp, fmt)[0]
            lo = np.where(np.arange(got.size) < H * W, c["ylo"], c["clo"])
            hi = np.where(np.arange(got.size) < H * W, c["yhi"], c["chi"])
            assert (got >= np.minimum(lo, cin)).all() and (got <= np.maximum(hi, cin)).all()
            legal = (cin >= lo) & (cin <= hi)
            assert (got[legal] >= lo[legal]).all() and (got[legal] <= hi[legal]).all()


@pytest.mark.parametrize("bits", [8, 10])
def test_removed_of_the_inputs_own_float_image_is_mid_grey_everywhere(bits):
    """4:4:4 full range, in-gamut input: the egress of the ingested input is the input (tests/test_host_yuv.py: the round trip, every value within
    1e-3 of its code before the rounding), so input minus result is 0 and every sample of all three planes is co = 128 s."""
    fmt = R.Fmt(bits, R.C444, R.BT709, R.FULL)
    rng = np.random.default_rng(8)
    top = (1 << bits) - 1
    Y, U, V = (rng.integers(0, top + 1, 400_000) for _ in range(3))
    rgb64 = R.yuv_to_rgb_f64(Y, U, V, fmt)
    ok = (rgb64.min(0) >= 0.0) & (rgb64.max(0) <= 1.0)
    T, H, W = 2, 48, 80
    assert ok.sum() >= T * H * W
    Y, U, V = (a[ok][:T * H * W].reshape(T, H * W) for a in (Y, U, V))
    inp = np.stack([R.join_planes(Y[t], U[t], V[t], fmt) for t in range(T)])
    x = R.ingest_emu(inp, fmt, H, W, H, W, "fp32")
    assert np.array_equal(R.egress_emu(x, fmt, H, W), inp)
    co = 128 << (bits - 8)
    for gain in (1.0, 4.0):                                        # |e - v| <= 1e-3: still nothing at gain 4
        got = M.codes(M.egress(x, fmt, H, W, ("removed", gain, gain), inp), fmt)
        assert (got == co).all(), gain
    other = M.codes(M.egress(x, fmt, H, W, ("removed", 1.0, 1.0), np.roll(inp, 1, axis=1)), fmt)
    assert not (other == co).all()                                 # another input: the difference shows


def test_removed_shows_the_difference_times_the_gain_around_mid_grey():
    fmt = R.Fmt(8, R.C444, R.BT601, R.FULL)
    H, W = 4, 8
    x = np.full((1, 3, H, W), 0.5, np.float32)                     # grey: Y' = 0.5 -> v = 127.5, Cb = Cr = 0 -> v = 128
    inp = R.join_planes(np.full((H, W), 130), np.full((H, W), 125), np.full((H, W), 128), fmt)[None]
    Y, U, V = R.split_planes(M.egress(x, fmt, H, W, ("removed", 2.0, 3.0), inp)[0], fmt, H, W)
    assert (Y == 133).all() and (U == 128 - 9).all() and (V == 128).all()        # 128 + 2 * 2.5, 128 + 3 * (-3), 128
    Y, _, _ = R.split_planes(M.egress(x, fmt, H, W, ("removed", 100.0, 1.0), inp)[0], fmt, H, W)
    assert (Y == 255).all()                                        # clamped to the legal codes


# ---- argument forms -----------------------------------------------------------------------------------------------------------------------
def test_amount_form_takes_a_number_or_a_pair_and_refuses_the_rest():
    f = restore.amount_form
    assert f(None) == (None, None, None)
    assert f(1.0) == (None, (1.0, 1.0), None) and f(1) == (None, (1.0, 1.0), None) and f((1.0, 1.0)) == (None, (1.0, 1.0), None)
    assert f(0.7) == (("amount", 0.7, 0.7), (0.7, 0.7), None)
    assert f((0.7, 1.0)) == (("amount", 0.7, 1.0), (0.7, 1.0), None) and f([0, 1]) == (("amount", 0.0, 1.0), (0.0, 1.0), None)
    assert f(0.0) == (("amount", 0.0, 0.0), (0.0, 0.0), None)
    assert f(np.float32(0.5)) == (("amount", 0.5, 0.5), (0.5, 0.5), None)
    assert f(None, "removed") == (("removed", 1.0, 1.0), None, "removed")
    assert f(1.0, "removed", 4) == (("removed", 4.0, 4.0), (1.0, 1.0), "removed")
    assert f((1.0, 1.0), "removed", 0.0) == (("removed", 0.0, 0.0), (1.0, 1.0), "removed")
    for bad in (-0.1, 1.5, float("nan"), float("inf"), (0.5,), (0.5, 0.5, 0.5), (0.5, 1.1), (float("nan"), 1.0), "0.5", "auto", (None, 1.0), ()):
        with pytest.raises(ValueError, match="amount"):
            f(bad)
    for bad in ("restored", "added", "", 1, True):
        with pytest.raises(ValueError, match="view"):
            f(None, bad)
    for bad in (0.5, (1.0, 0.5), 0.0):
        with pytest.raises(ValueError, match="view='removed'"):
            f(bad, "removed")
    for bad in (-1.0, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError, match="removed_gain"):
            f(None, "removed", bad)


def test_the_command_line_flags_and_their_errors(capsys):
    ap = restore.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["in", "out"])
    assert (a.amount, a.view, a.removed_gain) == (None, "restored", 1.0)
    a = ap.parse_args(base + ["--amount", "0.5", "in", "out"])
    assert a.amount == 0.5
    a = ap.parse_args(base + ["--amount", "0.5,1", "--view", "restored", "in", "out"])
    assert a.amount == (0.5, 1.0)
    a = ap.parse_args(base + ["--view", "removed", "--removed_gain", "4", "in", "out"])
    assert (a.amount, a.view, a.removed_gain) == (None, "removed", 4.0)
    assert restore.amount_arg("0.25") == 0.25 and restore.amount_arg("1,0") == (1.0, 0.0)
    for bad in (["--amount", "x"], ["--amount", "0.5,x"], ["--amount", "0.1,0.2,0.3"], ["--amount", ""], ["--view", "added"], ["--removed_gain", "x"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + bad + ["in", "out"])
    # judged by main() before any file is opened and before the device is touched
    for bad, word in ((["--amount", "1.5"], "amount"), (["--amount", "0.5,-1"], "amount"), (["--amount", "nan"], "amount"),
                      (["--amount", "0.5", "--view", "removed"], "view='removed'"), (["--view", "removed", "--removed_gain", "-1"], "removed_gain"),
                      (["--view", "removed", "--removed_gain", "inf"], "removed_gain")):
        with pytest.raises(SystemExit):
            restore.main(base + bad + ["/nonexistent/in.y4m", "/nonexistent/out.y4m"])
        assert word in capsys.readouterr().err


def test_the_symbol_the_struct_and_the_formulas_are_declared():
    assert "sn_egress_yuv_mix" in L.SYMBOLS and (L.SN_MIX_AMOUNT, L.SN_MIX_REMOVED) == (0, 1)
    with open(os.path.join(ROOT, "include", "shiftnet_hip.h")) as fh:
        header = fh.read()
    assert re.search(r"#define SN_ABI_VERSION 20\b", header)
    assert "typedef struct sn_yuv_mix { int mode; float ay, ac; } sn_yuv_mix;" in header
    assert re.search(r"#define SN_MIX_AMOUNT\s+0\b", header) and re.search(r"#define SN_MIX_REMOVED\s+1\b", header)
    for line in ("m = e + a * (v - e)", "m = co + a * (e - v)", "min(lo, code_in), max(hi, code_in)"):
        assert line in header
    import ctypes
    assert ctypes.sizeof(L.YuvMix) == 12
    lib = L.load()
    assert hasattr(lib, "sn_egress_yuv_mix") and lib.sn_abi_version() == 20
