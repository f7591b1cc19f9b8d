"""CPU checks behind tests/test_gpu_gsts_edges.py: the float64 references of tests/gsts_edge_cases.py against the oracle's own chain, the K0 plan
(sn_gsts_shiftconv_mfma_plan at ncu = 256) and that every plan's item loops produce each tile exactly once, the walking kernel's ring-row
arithmetic, and negative controls that prove the operands exercise what the rows claim."""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gsts_edge_cases as GE
from oracle import shiftnet_oracle as O
from shiftnet_amd import lib as L
from shiftnet_amd.spec import shift_table

D = torch.float64


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    return L.load()


def src_of(c, x=0x10000000, halo=0x20000000):
    return L.UnitSrc(x, c.T, c.h, c.w, c.C, c.mode, c.wrap, halo if c.wrap == 2 else None, c.t0, c.nt, c.clip)


# ---- the references are the oracle's chain ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [64, 80])
@pytest.mark.parametrize("mode,wrap", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_references_equal_the_oracle_chain(C, mode, wrap):
    """K0: O.temporal_roll -> O.spatial_shift -> depthwise conv2d, in float64, on the same bf16 operands; K4's shortcut: O.gsts_gather(...)[:, :C]"""
    assert O.shift_offsets(C) == shift_table(C)
    k0 = GE.K0Case("oracle", C, 3, 21, 19, mode, wrap, (4,), seed=11 + C + mode)
    ops = GE.k0_operands(k0)
    ref, _, _ = GE.k0_reference(k0, ops)
    x = ops["x"].to(D).permute(0, 3, 1, 2).contiguous()
    _, hw = O.temporal_roll(x, mode == 2, bool(wrap))
    w = ops["w"].to(torch.bfloat16).to(D).view(C // 2, 1, 3, 3)
    want = F.conv2d(O.spatial_shift(hw.contiguous()), w, padding=1, groups=C // 2).permute(0, 2, 3, 1)
    assert (ref - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
    k4 = GE.K4Case("oracle", C, 3, 5, 7, mode, wrap, True, seed=13 + C + mode)
    ops4 = GE.k4_operands(k4)
    x4 = ops4["x"].to(D).permute(0, 3, 1, 2).contiguous()
    u = O.gsts_gather(x4, mode == 2, bool(wrap))[:, :C].permute(0, 2, 3, 1)
    got = torch.stack([GE.k4_shortcut(k4, ops4, t) for t in range(k4.T)])
    assert torch.equal(got, u)
    assert torch.equal(GE.k4_shortcut(GE.K4Case("cab1", C, 3, 5, 7, 0, 0, True), ops4, 1), ops4["x"][1].to(D))


def test_halo_and_clips_follow_the_long_window():
    """wrap 2: a rank's slabs with the halo equal those of the long window it was cut from; clips: each clip's slabs equal the clip alone"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((6, 3, 4, 64), generator=g).to(torch.bfloat16)
    for mode in (1, 2):
        lo, hi = (x[3:], x[2][..., 32:]) if mode == 1 else (x[:3], x[3][..., :32])
        off = 3 if mode == 1 else 0
        for t in range(3):
            for a, b in zip(GE.unit_slabs(lo, hi.contiguous(), mode, 2, 0, t), GE.unit_slabs(x, None, mode, 0, 0, t + off)):
                assert torch.equal(a, b), (mode, t)
        for wrap in (0, 1):
            for t in range(6):
                for a, b in zip(GE.unit_slabs(x, None, mode, wrap, 3, t), GE.unit_slabs(x[t // 3 * 3: t // 3 * 3 + 3], None, mode, wrap, 0, t % 3)):
                    assert torch.equal(a, b), (mode, wrap, t)


def test_k4_operands_are_what_pack_out_gemm_packs():
    """the reference's W' and bias' are the values inside prep.pack_out_gemm's fragments (rows in natural order: lane (g, p) of M-tile mt = row
    mt 16 + p, k-slot 8 g + j) and its bias"""
    for C in (64, 80):
        c = GE.K4Case("pack", C, 1, 2, 2, 0, 0, True, seed=3 + C)
        ops = GE.k4_operands(c)
        wp, bias = GE.k4_folded(ops)
        pk = GE.k4_packed(ops)
        mt, ks = C // 16, (C + 31) // 32
        frag = pk["wfrag"].to(D).view(mt, ks, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(16 * mt, 32 * ks)      # [row][k]
        from shiftnet_amd.prep import rows_natural
        assert torch.equal(frag[torch.from_numpy(rows_natural(C, mt))][:, :C], wp) and (frag[:, C:] == 0).all()
        assert torch.equal(pk["bias"].to(D), bias)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(GE.K0_PLAN_ROWS), ids=lambda k: "c%d_%dx%dx%d" % k)
def test_plan_table_at_256_compute_units(key, lib):
    C, T, h, w = key
    form, S = GE.K0_PLAN_ROWS[key]
    p = L.k0_plan(lib, L.UnitSrc(0x10000000, T, h, w, C, 1, 0), 256)
    assert (p["form"], p["S"]) == (form, S), p
    assert p["ntx"] == (w + 15) // 16 and p["nty"] == (h + 15) // 16 and p["nt"] == T and p["grid"] == 8 * p["wgs"]
    assert p["nseg"] == -(-p["nty"] // p["S"])
    if form == GE.WALK:                     # at least four items per workgroup slot
        assert p["nseg"] * p["ntx"] * T >= 4 * (2 if C == 64 else 1) * 256 and p["wgs"] == (64 if C == 64 else 32) and not p["per_tile"]


def test_plan_per_tile_flag(lib):
    """C = 64 with 1500 tiles or more per XCD in the tile form: one workgroup per tile; so is a launch with fewer tiles than workgroup slots"""
    assert L.k0_plan(lib, L.UnitSrc(0x10000000, 8, 360, 640, 64, 1, 0), 256)["per_tile"] == 0
    big = L.k0_plan(lib, L.UnitSrc(0x10000000, 20, 360, 640, 64, 1, 0), 256, L.K0Opts(GE.TILE, 0, 0))
    assert big["form"] == GE.TILE and big["per_tile"] == 1 and big["wgs"] == big["per_x"] * big["ntx"] >= 1500
    big80 = L.k0_plan(lib, L.UnitSrc(0x10000000, 20, 360, 640, 80, 1, 0), 256, L.K0Opts(GE.TILE, 0, 0))
    assert big80["per_tile"] == 0 and big80["wgs"] == 32
    small = L.k0_plan(lib, L.UnitSrc(0x10000000, 5, 90, 160, 64, 1, 0), 256)
    assert small["per_tile"] == 1 and small["wgs"] == small["per_x"] * small["ntx"] == 40


def test_plan_refuses_what_the_launch_refuses(lib):
    ok = L.UnitSrc(0x10000000, 4, 37, 50, 64, 1, 0)
    plan = (ctypes.c_int * len(L.K0_PLAN_FIELDS))()
    assert lib.sn_gsts_shiftconv_mfma_plan(ctypes.byref(ok), 256, plan) == 0
    assert lib.sn_gsts_shiftconv_mfma_plan(ctypes.byref(ok), 256, None) == GE.EINVAL
    assert lib.sn_gsts_shiftconv_mfma_plan(ctypes.byref(ok), 7, plan) == GE.EINVAL
    for bad in (L.UnitSrc(0x10000000, 4, 37, 50, 64, 0, 0), L.UnitSrc(0x10000000, 4, 37, 50, 48, 1, 0), L.UnitSrc(None, 4, 37, 50, 64, 1, 0),
                L.UnitSrc(0x10000000, 4, 37, 50, 64, 1, 2), L.UnitSrc(0x10000000, 4, 37, 50, 64, 1, 0, None, 3, 2),
                L.UnitSrc(0x10000000, 4, 37, 50, 64, 1, 0, None, 0, 0, 3)):
        assert lib.sn_gsts_shiftconv_mfma_plan(ctypes.byref(bad), 256, plan) == GE.EINVAL
    for opt in (L.K0Opts(3, 0, 0), L.K0Opts(-1, 0, 0), L.K0Opts(GE.WALK, 9, 0), L.K0Opts(GE.WALK, -1, 0), L.K0Opts(GE.TILE, 4, 0), L.K0Opts(0, 4, 0),
                L.K0Opts(GE.TILE, 0, -1)):
        assert lib.sn_gsts_shiftconv_mfma_plan_opt(ctypes.byref(ok), 256, ctypes.byref(opt), plan) == GE.EINVAL, (opt.form, opt.seg, opt.wgs)
    # all zeros = NULL = the plan
    assert L.k0_plan(lib, ok, 256, L.K0Opts(0, 0, 0)) == L.k0_plan(lib, ok, 256)


def _covers(plan, tag):
    items = GE.k0_items(plan)
    want = {(t, ty, tx) for t in range(plan["nt"]) for ty in range(plan["nty"]) for tx in range(plan["ntx"])}
    assert len(items) == len(want) and set(items) == want, (tag, plan, len(items), len(want))


def _replay_every_form(lib, tag, s, ncu, seen):
    _covers(L.k0_plan(lib, s, ncu), (tag, ncu, "auto"))
    for wgs in (0, 1, 1 << 20):
        p = L.k0_plan(lib, s, ncu, L.K0Opts(GE.TILE, 0, wgs))
        assert p["form"] == GE.TILE and (wgs != 1 or p["wgs"] == 1) and (wgs != 1 << 20 or p["per_tile"] == 1)
        _covers(p, (tag, ncu, "tile", wgs))
    for seg in range(0, 9):
        for wgs in (0, 1):
            p = L.k0_plan(lib, s, ncu, L.K0Opts(GE.WALK, seg, wgs))
            assert p["form"] == GE.WALK and (seg == 0 or p["S"] == min(seg, p["nty"])) and (wgs != 1 or p["wgs"] == 1)
            _covers(p, (tag, ncu, "walk", seg, wgs))
            seen.add(p["S"])


@pytest.mark.parametrize("key", sorted(GE.K0_PLAN_ROWS), ids=lambda k: "c%d_%dx%dx%d" % k)
def test_every_plan_of_the_table_covers_every_tile_once(key, lib):
    """every row of the plan table, at the table's 256 compute units: the library's choice and every forced form -- tile with wgs auto / 1 / one
    per tile, walk with S = 1 .. 8 and wgs auto / 1 -- in the spirit of test_phase1_work_plan_covers_every_row_once"""
    seen = set()
    _replay_every_form(lib, key, L.UnitSrc(0x10000000, key[1], key[2], key[3], key[0], 1, 0), 256, seen)
    assert seen == set(range(1, min(8, -(-key[2] // 16)) + 1))                  # a segment is no longer than the map has tile rows


def test_every_plan_of_the_gpu_rows_covers_every_tile_once(lib):
    """the same replay for every K0 row of the GPU test (frame ranges, clips and halos included), at 256, 8 and 304 compute units"""
    seen = set()
    for c in GE.K0_CASES:
        for ncu in (256, 8, 304):
            _replay_every_form(lib, c.id, src_of(c), ncu, seen)
    assert seen == set(range(1, 9))


def _walk_slacks(lib, c, S):
    """(block slack, tile, position in its segment) of every staging block a walk launch of row c at segment length S issues, from the plan"""
    p = L.k0_plan(lib, src_of(c), 256, L.K0Opts(GE.WALK, S, 0))
    out = []
    for sg in range(p["nseg"]):
        for jj in range(min(p["S"], p["nty"] - sg * p["S"])):
            for tx in range(p["ntx"]):
                out += [(b, (sg * p["S"] + jj, tx), jj) for b in GE.walk_block_slacks(c.h, c.w, sg * p["S"] + jj, tx, jj)]
    return out


def test_rows_reach_the_edges_they_name(lib):
    """what the K0 rows claim, read off the plans and the loaders' `full` predicates as tests/gsts_edge_cases.py restates them (tile_window_slack,
    walk_block_slacks: slack 0 = met with equality, -1 = missed by one): tile counts, the early break, items per workgroup; and the K4 rows' item
    counts"""
    by = {c.id: c for c in GE.K0_CASES}
    for C in (64, 80):
        c, m = by[f"c{C}_ragged_3x137x41_m1"], by[f"c{C}_full_misses_by_one_3x136x40"]
        p = L.k0_plan(lib, src_of(c), 256, L.K0Opts(GE.WALK, 4, 0))
        assert (p["nty"], p["ntx"], p["nseg"]) == (9, 3, 3) and c.h % 16 and c.w % 16
        assert p["nt"] * p["nseg"] == 9 and p["per_x"] == 2 and 8 * p["per_x"] > 9                   # XCD 4's second row does not exist: break
        assert sorted(i for i in GE.k0_items(p) if i[0] == 0 and i[2] == 0) == [(0, ty, 0) for ty in range(9)]
        seg_len = lambda S: [min(S, 9 - s * S) for s in range(-(-9 // S))]
        assert c.walk == (4, 6, 8, 5, 7) and [seg_len(S) for S in c.walk] == [[4, 4, 1], [6, 3], [8, 1], [5, 4], [7, 2]]
        # tile form: the window of tile (7, 1) ends on the image's last row and last column, and is the only one that does
        tiles = {(ty, tx): GE.tile_window_slack(c.h, c.w, ty, tx) for ty in range(9) for tx in range(3)}
        assert [k for k, v in tiles.items() if v == (0, 0)] == [(7, 1)] and not any(v and min(v) > 0 for v in tiles.values())
        assert any(v and v[0] > 0 and v[1] == 0 for v in tiles.values()) and any(v is None for v in tiles.values())
        # walking form: a later block of a segment meets `full` with equality at every S the row lists but 7, where tile 7 starts a segment and
        # its second 17-row block does
        for S in c.walk:
            eq = [(t, jj) for b, t, jj in _walk_slacks(lib, c, S) if b == (0, 0)]
            assert eq == [((7, 1), 0 if S == 7 else 7 % S)], (S, eq)
        # one row and one column fewer: no loader of either form runs without tests, tile (7, 1) misses by exactly one both ways
        assert m.walk and (m.h, m.w) == (c.h - 1, c.w - 1)
        mt = {(ty, tx): GE.tile_window_slack(m.h, m.w, ty, tx) for ty in range(9) for tx in range(3)}
        assert mt[(7, 1)] == (-1, -1) and not any(v and min(v) >= 0 for v in mt.values())
        for S in m.walk:
            sl = _walk_slacks(lib, m, S)
            assert not any(b and min(b) >= 0 for b, _, _ in sl) and [(t, jj) for b, t, jj in sl if b == (-1, -1)] == [((7, 1), 7 % S)], S
    # S = 8 visits the eight ring offsets
    assert [GE.ring_row_read(jj, 0) for jj in range(8)] == [0, 16, 32, 14, 30, 12, 28, 10] and 8 in by["c64_ragged_3x137x41_m1"].walk
    w = by["c64_items_per_workgroup_2x70x200"]
    for form, seg in ((GE.WALK, 4), (GE.WALK, 2), (GE.TILE, 0)):
        p = L.k0_plan(lib, src_of(w), 256, L.K0Opts(form, seg, 1))
        assert p["wgs"] == 1 and p["per_x"] * p["ntx"] >= 13
    assert sorted({c.items for c in GE.K4_CASES if "15_items" in c.id or "6_items" in c.id}) == [6, 15]
    assert {c.h * c.w for c in GE.K4_CASES} == {1, 256, 259, 513}
    for C in (64, 80):
        rows = [c for c in GE.K4_CASES if c.C == C]
        assert {c.mode for c in rows} == {0, 1, 2} and {c.wrap for c in rows} == {0, 1, 2} and {c.bias for c in rows} == {True, False}
        assert any(c.clip for c in rows) and any(c.nt for c in rows)
        rows = [c for c in GE.K0_CASES if c.C == C]
        assert {(c.mode, c.wrap) for c in rows} >= {(1, 2), (2, 2), (1, 0), (2, 0), (1, 1), (2, 1)} and any(c.clip for c in rows) and any(c.nt for c in rows)


# ---- the ring ----------------------------------------------------------------------------------------------------------------------------

def test_ring_rows_written_are_the_ring_rows_read():
    """For every tile jj of a segment and every window row: the ring row `stage` wrote it to -- when this tile, or an earlier one of the segment,
    staged it -- is the ring row the MFMA loop reads at r0 + s, and no later staging has overwritten it."""
    ring = {}                                                       # ring row -> (tile, window row) it holds
    for jj in range(8):
        for wr, rr in GE.ring_rows_written(jj).items():
            assert 0 <= rr < GE.RW
            ring[rr] = (jj, wr)
        assert len(ring) == GE.RW
        for wr in range(GE.RW):                                     # n + 8 + sy + s spans 0 .. 33
            tile, row = ring[GE.ring_row_read(jj, wr)]
            assert 16 * tile + row == 16 * jj + wr, (jj, wr, tile, row)      # the same image row, whichever tile staged it
    for jj in range(1, 8):
        assert sorted(GE.ring_rows_written(jj)) == list(range(18, 34))


# ---- negative controls ------------------------------------------------------------------------------------------------------------------

def _ratio(ref, other, tol):
    return ((other - ref).abs() / tol).max().item()


@pytest.mark.parametrize("case", GE.K0_CASES, ids=[c.id for c in GE.K0_CASES])
def test_k0_controls_break_the_bound(case):
    ops = GE.k0_operands(case)
    ref, tol, m = GE.k0_reference(case, ops)
    assert torch.isfinite(ref).all() and (tol > 0).all()
    nopad, _, _ = GE.k0_reference(case, ops, control="no_conv_padding")
    d = (nopad - ref).abs() / tol
    assert d.max().item() >= 8.0, case.id
    inner = d[:, 1:-1, 1:-1] if case.h > 2 and case.w > 2 else d[:, :0]
    assert inner.numel() == 0 or inner.max().item() == 0.0                     # ... and only on the border
    drop, _, _ = GE.k0_reference(case, ops, control="tap_dropped")
    assert _ratio(ref, drop, tol) >= 8.0, case.id


@pytest.mark.parametrize("case", GE.K4_CASES, ids=[c.id for c in GE.K4_CASES])
def test_k4_controls_break_the_bound(case):
    ops = GE.k4_operands(case)
    ref, tol, m = GE.k4_reference(case, ops)
    assert torch.isfinite(ref).all() and (tol > 0).all()
    noca, _, _ = GE.k4_reference(case, ops, control="no_ca")
    assert _ratio(ref, noca, tol) >= 8.0, case.id
    if case.mode:
        unrolled, _, _ = GE.k4_reference(case, ops, control="unrolled_shortcut")
        per_frame = ((unrolled - ref).abs() / tol).flatten(1).max(1).values
        kept = [i for i, t in enumerate(case.frames)
                if torch.equal(GE.k4_shortcut(case, ops, t), GE.k4_shortcut(case, ops, t, rolled=False))]
        assert len(kept) <= 1 + (case.T // case.clip - 1 if case.clip else 0)      # only kept boundary frames are their own shortcut
        assert all(per_frame[i].item() >= 8.0 for i in range(len(per_frame)) if i not in kept), (case.id, per_frame.tolist())
