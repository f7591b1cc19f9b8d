"""CPU tests of the tiled restorer's pure parts: windows.plan_tiles and its weights against the position-by-position restatement of tests/tile_ref.py,
the accepted forms of ``tile`` / ``tile_overlap`` in Python and on the command line, and the new symbol in header, build list and library."""
import math
import os
import re

import numpy as np
import pytest

import tile_ref as T
from shiftnet_amd import restore_cli, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = (8, 16, 24, 40)
LENGTHS = range(1, 201)


def cases():
    for S in SIDES:
        for V in range(0, S // 2 + 1):
            for L in LENGTHS:
                yield L, S, V


def test_origins_start_at_zero_end_at_the_far_edge_ascend_and_overlap_by_at_least_v():
    for L, S, V in cases():
        o, w = windows.tile_axis(L, S, V)
        assert o == T.origins(L, S, V), (L, S, V)
        if S >= L:
            assert o == [0] and w.shape == (1, L) and (w == 1.0).all(), (L, S, V)
            continue
        n = math.ceil((L - S) / (S - V)) + 1
        assert len(o) == n and n >= 2, (L, S, V)
        assert o[0] == 0 and o[-1] == L - S, (L, S, V)
        assert all(b > a for a, b in zip(o, o[1:])), (L, S, V)                       # ascending, no tile twice
        assert all(a + S - b >= V for a, b in zip(o, o[1:])), (L, S, V)              # consecutive tiles overlap by at least V
        assert all(a + S >= b for a, b in zip(o, o[1:])), (L, S, V)                  # and every position is covered
        assert w.shape == (n, S)


def test_weights_sum_to_one_are_one_where_one_tile_covers_and_have_no_ramp_at_the_pictures_edges():
    ulp = 2.0 ** -23
    for L, S, V in cases():
        o, w64 = windows.tile_axis(L, S, V)
        side = min(S, L)
        assert np.array_equal(w64, T.weights64(L, S, V)), (L, S, V)                  # the vectorised plan equals the restatement exactly
        w32 = w64.astype(np.float32)
        assert np.isfinite(w64).all() and (w64 > 0).all() and (w64 <= 1).all(), (L, S, V)
        sum64, sum32 = np.zeros(L), np.zeros(L)
        for k, ok in enumerate(o):
            sum64[ok:ok + side] += w64[k]
            sum32[ok:ok + side] += w32[k].astype(np.float64)
        assert np.abs(sum64 - 1.0).max() <= 1e-12, (L, S, V)
        assert np.abs(sum32 - 1.0).max() <= 4 * ulp, (L, S, V)
        for p, ks in enumerate(T.cover(L, S, V)):
            assert ks, (L, S, V, p)
            if len(ks) == 1:
                assert w32[ks[0], p - o[ks[0]]] == np.float32(1.0) and w64[ks[0], p - o[ks[0]]] == 1.0, (L, S, V, p)
        # the picture's own edges: the first tile does not ramp up from position 0, the last does not ramp down to position L - 1
        assert w64[0, 0] == 1.0 and w64[-1, -1] == 1.0, (L, S, V)
        if len(o) > 1:
            first_shared, last_shared = o[1], o[-2] + S - 1
            assert (w64[0, :first_shared] == 1.0).all() and (w64[-1, last_shared - o[-1] + 1:] == 1.0).all(), (L, S, V)


def test_two_facing_tiles_cross_fade_linearly():
    """Where exactly tiles k and k + 1 cover a position and both are on the ramp that faces the other -- always so when they overlap by m <= S / 2
    samples, which the regular overlap V <= S / 2 is, and always for two tiles -- tile k's weight is (o_k + S - p) / (m + 1): m, m - 1, ..., 1 over
    m + 1.  The shifted last tile may overlap its neighbour by more than S / 2; with three or more tiles the neighbour's other ramp can then be the
    shorter one, the cross-fade is no longer a straight line, and the weights are checked to be positive and to sum to 1 (the test above)."""
    seen_wide = 0
    for L, S, V in cases():
        o, w64 = windows.tile_axis(L, S, V)
        if len(o) < 2:
            continue
        cover = T.cover(L, S, V)
        for k in range(len(o) - 1):
            m = o[k] + S - o[k + 1]
            straight = 2 * m <= S or len(o) == 2
            seen_wide += (not straight)
            for p in range(o[k + 1], o[k] + S):
                if cover[p] != [k, k + 1] or not straight:
                    continue
                assert w64[k, p - o[k]] == (o[k] + S - p) / (m + 1), (L, S, V, k, p)
                assert w64[k + 1, p - o[k + 1]] == (p - o[k + 1] + 1) / (m + 1), (L, S, V, k, p)
    assert seen_wide > 0                                                            # the wide last overlap occurs among the cases


def test_plan_tiles_is_the_two_axes_in_row_major_order_with_float32_tables():
    plan = windows.plan_tiles(40, 56, 24, 32, 8)
    assert (plan.th, plan.tw) == (24, 32) and plan.ys == [0, 16] and plan.xs == [0, 24]
    assert plan.tiles == [(0, 0, 24, 32), (0, 24, 24, 32), (16, 0, 24, 32), (16, 24, 24, 32)] and not plan.single
    assert plan.wy.dtype == plan.wx.dtype == np.float32 and plan.wy.shape == (2, 24) and plan.wx.shape == (2, 32)
    assert np.array_equal(plan.wy, T.weights64(40, 24, 8).astype(np.float32)) and np.array_equal(plan.wx, T.weights64(56, 32, 8).astype(np.float32))
    one = windows.plan_tiles(40, 56, 40, 64, 8)                                      # a tile that is not smaller than the picture: clipped to it
    assert one.single and one.tiles == [(0, 0, 40, 56)] and (one.wy == 1).all() and (one.wx == 1).all()
    row = windows.plan_tiles(40, 56, 48, 32, 0)                                      # one axis tiled, no overlap: abutting tiles of weight 1
    assert row.tiles == [(0, 0, 40, 32), (0, 24, 40, 32)] and not row.single
    blend = T.blend([np.full((1, 3, 40, 32), 2.0, np.float32)] * 2, row, (1, 3, 40, 56))
    assert np.array_equal(blend[..., :24], np.full((1, 3, 40, 24), 2.0, np.float32)) and np.array_equal(blend[..., 32:], blend[..., :24])
    assert np.abs(blend[..., 24:32].astype(np.float64) - 2.0).max() <= 2.0 * 16 * 2.0 ** -23      # 32 + 32 - 56 = 8 columns shared, cross-faded back to 2.0


def test_the_reference_blend_of_a_constant_is_the_constant_to_rounding():
    plan = windows.plan_tiles(40, 56, 16, 24, 4)
    got = T.blend([np.full((2, 3, 16, 24), 0.75, np.float32)] * len(plan.tiles), plan, (2, 3, 40, 56))
    # the weights of an axis sum to 1 within 4 ulp, so their products within 8; up to four terms of three roundings of half an ulp each add 6
    assert np.abs(got.astype(np.float64) - 0.75).max() <= 0.75 * 16 * 2.0 ** -23


ILLEGAL = [((24, 30), 8, "small"), ((22, 32), 8, "small"), ((4, 32), 0, "small"), ((24, 32), 13, "small"), ((24, 32), -1, "small"), ((24, 32), 8.0, "small"),
           ((24, 32), None, "small"), ((24, 32), True, "small"), ((24.0, 32), 8, "small"), ((24, 32, 8), 8, "small"), ((24,), 8, "small"), ("24x32", 8, "small"),
           (0, 0, "small"), (-16, 0, "small"), (True, 0, "small"), (12, 4, "plus"), ((8, 64), 4, "plus"), ((24, 36), 4, "plus"), (None, -1, "small"),
           (None, "32", "small"), (6, 0, "small"), (2.5, 0, "small")]


@pytest.mark.parametrize("tile,overlap,topo", ILLEGAL)
def test_illegal_tiles_and_overlaps_are_value_errors(tile, overlap, topo):
    with pytest.raises(ValueError, match="tile"):
        windows.tile_form(tile, overlap, topo)


def test_legal_tiles_and_overlaps():
    assert windows.tile_form(None) is None and windows.tile_form(None, 0, "plus") is None
    assert windows.tile_form(512) == (512, 512, 32) and windows.tile_form((544, 960), 32, "plus") == (544, 960, 32)
    assert windows.tile_form((24, 32), 12) == (24, 32, 12) and windows.tile_form([8, 8], 4) == (8, 8, 4) and windows.tile_form(np.int64(16), 0) == (16, 16, 0)
    assert windows.tile_form(12, 6, "small") == (12, 12, 6) and windows.tile_form(16, 8, "plus") == (16, 16, 8)
    assert windows.DEFAULT_TILE_OVERLAP == 32


def test_the_command_line_parses_both_forms_and_refuses_what_the_restorer_refuses(capsys):
    assert restore_cli.tile_arg("544x960") == (544, 960) and restore_cli.tile_arg("512") == 512 and restore_cli.tile_arg("64X48") == (64, 48)
    ap = restore_cli.make_parser()
    base = ["--variant", "deblur_small", "--checkpoint", "synthetic"]
    a = ap.parse_args(base + ["--tile", "544x960", "--tile_overlap", "32", "in.y4m", "out.y4m"])
    assert a.tile == (544, 960) and a.tile_overlap == 32
    a = ap.parse_args(base + ["--tile", "512", "in.y4m", "out.y4m"])
    assert a.tile == 512 and a.tile_overlap is None
    assert ap.parse_args(base + ["in.y4m", "out.y4m"]).tile is None
    for bad in (["--tile", "544x"], ["--tile", "x960"], ["--tile", "5x4x4"], ["--tile", "-64"], ["--tile", "64.5"], ["--tile", "big"],
                ["--tile", "64", "--tile_overlap", "half"]):
        with pytest.raises(SystemExit):
            ap.parse_args(base + bad + ["in.y4m", "out.y4m"])
    # judged by main() before any file is opened: the files named here do not exist
    missing = ["/nonexistent/in.y4m", "/nonexistent/out.y4m"]
    for variant, bad, word in (("deblur_small", ["--tile", "30"], "multiples of 4"), ("deblur_small", ["--tile", "4"], "at least 8"),
                               ("deblur", ["--tile", "20x32"], "multiples of 8"), ("deblur_small", ["--tile", "24x32", "--tile_overlap", "13"], "half"),
                               ("deblur_small", ["--tile", "24x32", "--tile_overlap", "-1"], "tile_overlap"),
                               ("deblur_small", ["--tile_overlap", "8"], "needs --tile")):
        with pytest.raises(SystemExit) as e:
            restore_cli.main(["--variant", variant, "--checkpoint", "synthetic"] + bad + missing)
        assert e.value.code == 2
        assert word in capsys.readouterr().err, (bad, word)


def test_header_build_list_and_library_have_the_new_symbol_and_the_abi_version_stays_20():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert "sn_tile.hip" in mod.SOURCES and os.path.exists(os.path.join(ROOT, "shift-net_amd", "csrc", "sn_tile.hip"))
    mod.build()
    from shiftnet_amd import lib as L
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "shiftnet_hip.h")).read()
    assert re.search(r"^int sn_tile_accumulate\(const float\* tile, float\* canvas, const float\* wy, const float\* wx, int T, int C, int th, int tw, "
                     r"int Hc, int Wc,\s+int y0, int x0, void\* stream\);", header, flags=re.M)
    assert hasattr(lib, "sn_tile_accumulate") and "sn_tile_accumulate" in L.SYMBOLS
    assert L.ABI_VERSION == 20 and lib.sn_abi_version() == 20 and re.search(r"#define SN_ABI_VERSION 20\b", header)
    assert len(lib.sn_tile_accumulate.argtypes) == 13
    # the argument checks are host side and need no GPU
    assert lib.sn_tile_accumulate(None, None, None, None, 1, 3, 8, 8, 8, 8, 0, 0, None) == -22
    arr = np.zeros(4096, np.float32)                                                 # host memory: refused before anything would read it
    buf = arr.ctypes.data
    assert lib.sn_tile_accumulate(buf, buf + 1024, buf + 2048, buf + 3072, 1, 3, 8, 8, 8, 8, 1, 0, None) == -22
    assert lib.sn_tile_accumulate(buf + 2, buf + 1024, buf + 2048, buf + 3072, 1, 3, 8, 8, 8, 8, 0, 0, None) == -22
