"""CPU tests of the self-ensemble's pure parts: the index map of tests/geo_ref.py (round trip, inverses), ensemble.members, windows.ensemble_form, the
command line, the new symbols in header, build list and library, and the argument checks of the two kernels, which are host side."""
import ctypes
import os
import re

import numpy as np
import pytest

import geo_ref as G
from shiftnet_amd import ensemble, restore, restore_cli, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2, 5, 7), (2, 3, 8, 8)]


def ramp(shape, dtype=np.float32):
    return np.arange(1, int(np.prod(shape)) + 1).reshape(shape).astype(dtype)      # distinct values: a misplaced element cannot pass


@pytest.mark.parametrize("shape", SHAPES)
def test_accumulating_the_transform_gives_the_tensor_back_for_all_16_ops(shape):
    a = ramp(shape)
    for op in range(16):
        moved = G.transform(a, op)
        assert moved.shape == G.out_shape(shape, op)
        back = G.accumulate(np.full(shape, np.nan, np.float32), moved, op, init=1, scale=1.0)
        assert np.array_equal(back, a), op
        assert sorted(moved.reshape(-1)) == sorted(a.reshape(-1)), op              # a permutation


@pytest.mark.parametrize("shape", SHAPES)
def test_the_map_is_what_numpy_calls_flip_and_transpose_and_its_inverse_swaps_the_flips_under_the_transpose(shape):
    a = ramp(shape)
    for op in range(16):
        want = a
        if op & G.TRANSPOSE:
            want = want.transpose(0, 1, 3, 2)
        if op & G.FLIP_Y:
            want = want[:, :, ::-1]
        if op & G.FLIP_X:
            want = want[:, :, :, ::-1]
        if op & G.REVERSE_T:
            want = want[::-1]
        assert np.array_equal(G.transform(a, op), want), op
        inv = op if not op & G.TRANSPOSE else (op & 12) | ((op & 1) << 1) | ((op & 2) >> 1)
        assert np.array_equal(G.transform(G.transform(a, op), inv), a), (op, inv)
    assert [(op & 12) | ((op & 1) << 1) | ((op & 2) >> 1) for op in (4, 5, 6, 7)] == [4, 6, 5, 7]


def test_accumulate_rounds_the_sum_and_the_product_separately():
    canvas = np.array([1.0, 1.0, -0.0], np.float32).reshape(1, 1, 1, 3)
    member = np.array([2.0 ** -24, 3 * 2.0 ** -24, -0.0], np.float32).reshape(1, 1, 1, 3)
    got = G.accumulate(canvas.copy(), member, 0, init=0, scale=3.0)
    # 1 + 2^-24 rounds to 1 (a tie, to even), 1 + 3 * 2^-24 to 1 + 2^-22 (a tie again); a fused multiply-add would give 3 + 2^-22 and 3 + 2^-21
    assert got.reshape(-1).tolist() == [3.0, np.float32(np.float32(1 + 2.0 ** -22) * np.float32(3)), 0.0]
    assert np.signbit(G.accumulate(canvas.copy(), member, 0, init=0, scale=1.0).reshape(-1)[2])     # -0 + -0 = -0
    assert np.signbit(G.accumulate(canvas.copy(), member, 1, init=1, scale=0.125).reshape(-1)[0])   # mirrored: -0 lands first


def test_members():
    assert ensemble.members(None) == ensemble.members(1) == [0]
    assert ensemble.members(2) == [0, 1] and ensemble.members(4) == [0, 1, 2, 3] and ensemble.members(8) == list(range(8))
    assert ensemble.members() == list(range(8))
    assert ensemble.members(1, True) == [0, 8] and ensemble.members(None, time=True) == [0, 8]
    assert ensemble.members(4, True) == [0, 1, 2, 3, 8, 9, 10, 11] and ensemble.members(8, True) == list(range(16))
    for e in (None, 1, 2, 4, 8):
        for t in (False, True):
            m = ensemble.members(e, t)
            assert m[0] == 0 and len(m) & (len(m) - 1) == 0 and len(set(m)) == len(m)
    for bad in (0, 3, 16, "8", 8.0, True, -2, (8,)):
        with pytest.raises(ValueError, match="ensemble"):
            ensemble.members(bad)


def test_ensemble_form():
    assert windows.ensemble_form() is None and windows.ensemble_form(None, False) is None and windows.ensemble_form(1, False, (16, 16, 4)) is None
    assert windows.ensemble_form(4) == (4, False, [0, 1, 2, 3]) and windows.ensemble_form(np.int64(2), np.bool_(False)) == (2, False, [0, 1])
    assert windows.ensemble_form(None, True) == (1, True, [0, 8]) and windows.ensemble_form(8, True) == (8, True, list(range(16)))
    for bad in (0, 3, 16, "8"):
        with pytest.raises(ValueError, match="ensemble"):
            windows.ensemble_form(bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="ensemble_time"):
            windows.ensemble_form(4, bad)
    for e, t in ((4, False), (None, True), (8, True)):
        with pytest.raises(ValueError, match="tile"):
            windows.ensemble_form(e, t, (16, 16, 4))


def test_the_restorer_refuses_before_the_device_is_touched():
    """The module is on the CPU, which the restorer refuses last: the ensemble's errors come first."""
    net = restore.load_net("deblur_small", "synthetic", "fp32", device="cpu")
    for kw, word in (({"ensemble": 3}, "ensemble must be"), ({"ensemble": "8"}, "ensemble must be"), ({"ensemble": 0}, "ensemble must be"),
                     ({"ensemble": 16}, "ensemble must be"), ({"ensemble": 4, "ensemble_time": 1}, "ensemble_time"),
                     ({"ensemble": 4, "tile": 16}, "tile"), ({"ensemble_time": True, "tile": 16}, "tile")):
        with pytest.raises(ValueError, match=word):
            restore.VideoRestorer(net, 4, **kw)
    with pytest.raises(ValueError, match="HIP device"):
        restore.VideoRestorer(net, 4, ensemble=4)


def test_the_command_line_takes_the_options_and_refuses_what_the_restorer_refuses(capsys):
    ap = restore_cli.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["in.y4m", "out.y4m"])
    assert a.ensemble == 1 and a.ensemble_time is False
    a = ap.parse_args(base + ["--ensemble", "8", "--ensemble_time", "in.y4m", "out.y4m"])
    assert a.ensemble == 8 and a.ensemble_time is True
    missing = ["/nonexistent/in.y4m", "/nonexistent/out.y4m"]      # judged by main() before any file is opened
    for bad, word in ((["--ensemble", "3"], "--ensemble"), (["--ensemble", "4", "--tile", "64"], "tile"),
                      (["--ensemble_time", "--tile", "64"], "tile")):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(base + bad + missing)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, (bad, word)


def test_header_build_list_and_library_have_the_new_symbols_and_the_abi_version_stays_20():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_geo.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_geo.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^int sn_geo_transform\(const void\* src, void\* dst, int esz, int op, int T, int C, int H, int W, void\* stream\);", header, flags=re.M)
    assert re.search(r"^int sn_geo_accumulate\(const float\* member, float\* canvas, int op, int init, float scale, int T, int C, int H, int W, "
                     r"void\* stream\);", header, flags=re.M)
    for name, value in (("FLIP_X", 1), ("FLIP_Y", 2), ("TRANSPOSE", 4), ("REVERSE_T", 8)):
        assert re.search(rf"^#define SN_GEO_{name} {value}\b", header, flags=re.M) and getattr(L, "SN_GEO_" + name) == value == getattr(G, name)
    assert ensemble.REVERSE_T == L.SN_GEO_REVERSE_T
    for sym in ("sn_geo_transform", "sn_geo_accumulate"):
        assert hasattr(lib, sym) and sym in L.SYMBOLS
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    assert len(lib.sn_geo_transform.argtypes) == 9 and len(lib.sn_geo_accumulate.argtypes) == 10
    assert lib.sn_geo_accumulate.argtypes[4] is ctypes.c_float


def test_the_argument_checks_need_no_gpu():
    """Host memory: everything here is refused before anything would read it or be launched."""
    from shiftnet_amd import lib as L
    lib = L.load()
    arr = np.zeros(8192, np.float32)
    a, b = arr.ctypes.data, arr.ctypes.data + 4096 * 4
    # T, C, H, W = 2, 3, 8, 8: 384 elements, so the two halves of arr do not overlap

    def tr(src=a, dst=b, esz=4, op=0, T=2, C=3, H=8, W=8):
        return lib.sn_geo_transform(src, dst, esz, op, T, C, H, W, None)

    def ac(member=a, canvas=b, op=0, init=1, scale=1.0, T=2, C=3, H=8, W=8):
        return lib.sn_geo_accumulate(member, canvas, op, init, scale, T, C, H, W, None)
    for kw in ({"src": None}, {"dst": None}, {"esz": 3}, {"esz": 0}, {"esz": 8}, {"esz": 1}, {"op": 16}, {"op": -1}, {"H": 0}, {"W": 0}, {"T": 0},
               {"C": 0}, {"H": -8}, {"src": a + 2}, {"dst": b + 1}, {"esz": 2, "dst": b + 1},      # a pointer that is not esz-byte aligned
               {"dst": a}, {"dst": a + 4 * 383}, {"src": a + 4 * 383, "dst": a}, {"esz": 2, "dst": a + 2 * 383},      # overlapping by one element
               {"T": 2 ** 31 - 1, "C": 2 ** 31 - 1, "H": 2 ** 31 - 1, "W": 2 ** 31 - 1}, {"T": 2 ** 30, "C": 2 ** 30, "H": 2, "W": 1}):      # the count
        assert tr(**kw) == -22, kw
    for kw in ({"member": None}, {"canvas": None}, {"op": 16}, {"op": -1}, {"H": 0}, {"W": 0}, {"T": 0}, {"C": 0}, {"member": a + 2}, {"canvas": b + 2},
               {"canvas": a}, {"canvas": a + 4 * 383}, {"member": a + 4 * 383, "canvas": a},
               {"scale": float("inf")}, {"scale": float("-inf")}, {"scale": float("nan")},
               {"T": 2 ** 31 - 1, "C": 2 ** 31 - 1, "H": 2 ** 31 - 1, "W": 2 ** 31 - 1}):
        assert ac(**kw) == -22, kw
    assert not arr.any()
