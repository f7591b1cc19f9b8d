"""CPU tests of sn_conv2d_route (include/shiftnet_hip.h): the kernel instance sn_conv2d / sn_cab_stats launch, computed on the host from the
descriptor, and the streaming kernel's work plan on a 256-CU device.

The GPU kernel table (tests/bf16_conv_cases.py, run by tests/test_gpu_bf16_conv_kernels.py) declares a route per row and, for streaming rows, the
plan; here every declared route and plan fact must be what the library selects, and the rows together must reach every instance the selector
can return, so an instance that appears in the dispatch without a row of its own fails this test."""
import ctypes
import dataclasses

import pytest
import torch

import bf16_conv_cases as BC

NCU = 256


@pytest.fixture(scope="module")
def lib():
    from shiftnet_amd import lib as L
    return L.load(), L


def _route(lb, c, ncu=NCU, flags=None):
    d = BC.fill_desc(c, BC.pointer_model(c), flags)
    plan = (ctypes.c_int * 8)(*([-7] * 8))
    return lb.sn_conv2d_route(ctypes.byref(d), c.lines_len, ncu, plan), list(plan)


@pytest.mark.parametrize("case", BC.CASES, ids=[c.id for c in BC.CASES])
def test_declared_route_and_plan_are_the_selected_ones(case, lib):
    lb, L = lib
    r, plan = _route(lb, case)
    assert r == case.route, (case.id, L.conv_route_name(r), L.conv_route_name(case.route))
    if BC.is_stream(r):
        got = dict(zip(L.CONV_PLAN_FIELDS, plan))
        assert case.plan == got, (case.id, case.plan, got)
        for e in case.edges:
            assert BC.EDGE_CHECKS[e](got), (case.id, e, got)
    else:
        assert not case.plan and not case.edges, case.id
        assert plan == [-7] * 8, (case.id, plan)                 # the plan is written for streaming routes only
    # the measurement bits 12..14 and the workgroups-per-CU bits 4..7 never change the instance
    for extra in (1 << 12, 2 << 12, 4 << 12, 7 << 12, 3 << 4):
        assert _route(lb, case, flags=case.flags | extra)[0] == r, (case.id, extra)


def test_cases_cover_every_instance_of_the_selector():
    declared = {c.route for c in BC.CASES}
    from shiftnet_amd import lib as L
    missing = [L.conv_route_name(r) for r in BC.ALL_ROUTES if r not in declared]
    unknown = [L.conv_route_name(r) for r in declared if r not in BC.ALL_ROUTES and r != BC.EINVAL]
    assert not missing and not unknown, (missing, unknown)
    assert len(BC.ALL_ROUTES) == len(set(BC.ALL_ROUTES)) == 50
    # every instance runs on the GPU, every streaming MODE through its own entry point
    gpu = {c.route for c in BC.CASES if c.gpu}
    assert all(r in gpu for r in BC.ALL_ROUTES)
    for c in BC.CASES:
        stats = (c.route >> 24) == BC.KS or (BC.is_stream(c.route) and BC.stream_mode(c.route) == 3)
        assert c.lines == stats, c.id
    for e in BC.EDGE_CHECKS:
        assert any(e in c.edges for c in BC.CASES), e


def test_route_codes_are_injective():
    from shiftnet_amd import lib as L
    names = {L.conv_route_name(r) for r in BC.ALL_ROUTES}
    assert len(names) == len(BC.ALL_ROUTES)
    for r in BC.ALL_ROUTES:
        k, mt, a, d, mode, rl = r >> 24, (r >> 20) & 15, (r >> 12) & 255, (r >> 8) & 15, (r >> 4) & 15, r & 15
        assert L.conv_route(k, mt, a, d, mode, rl) == r and r > 0


def test_selector_only_returns_listed_instances(lib):
    """Sweep the selector's inputs on the host (kernel size, stride, widths, inputs, modes, operands, flags; both entry points): every answer is
    SN_EINVAL or an instance of ALL_ROUTES -- never one of the 16 x 32-tile generic instances, which no longer exist."""
    lb, L = lib
    seen = set()
    base = BC.Case(id="sweep", route=0, cs_in=16, cins=(16,), c_out=16)
    for k in (1, 2, 3, 5):
        for stride in (1, 2):
            for cs, n_in in ((8, 1), (16, 1), (24, 1), (40, 1), (48, 1), (64, 1), (80, 1), (16, 2), (32, 3)):
                for c_out in (3, 16, 24, 40, 48, 64, 80, 96):
                    for ep in ("plain", "prelu_pool", "osc_res", "res2", "neg_slope"):
                        for flags in (0, BC.TILE, BC.STREAM_ALL, BC.STREAM_ALL | BC.RES_REGS, BC.DEPTH3, BC.DEPTH4, 3 << 10, BC.S2_SMALL):
                            kw = dict(prelu=0.25, pool=True) if ep == "prelu_pool" else dict(oscale=True, res=True) if ep == "osc_res" else \
                                dict(res=True, res2=True) if ep == "res2" else dict(prelu=-0.5, pool=True) if ep == "neg_slope" else {}
                            c = dataclasses.replace(base, cs_in=cs, cins=(cs,) * n_in, c_out=c_out, k=k, stride=stride, h_in=20, w_in=70, flags=flags, **kw)
                            for lines in (False, True) if ep == "prelu_pool" else (False,):
                                c2 = dataclasses.replace(c, lines=lines)
                                r, _ = _route(lb, c2)
                                assert r == BC.EINVAL or r in BC.ALL_ROUTES, (c2, L.conv_route_name(r))
                                assert not (r > 0 and (r >> 24) == BC.KG and ((r >> 12) & 255) == 16), c2
                                seen.add(r)
    for out_mode in (1, 2):
        for in_mode in (0, 1):
            c = dataclasses.replace(base, out_mode=out_mode, in_mode=in_mode, c_out=3 if out_mode == 2 else 64, h_in=10, w_in=18)
            r, _ = _route(lb, c)
            assert r in BC.ALL_ROUTES, (c, L.conv_route_name(r))
            seen.add(r)
    assert len(seen - {BC.EINVAL}) >= 40, sorted(L.conv_route_name(r) for r in seen)


def _fail_mutations(c0: "BC.Case", lines: bool):
    """descriptors the entry point refuses in its argument checks (before any launch), as (label, mutate(d))"""
    def m(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f
    common = [("no wfrag", m(wfrag=None)), ("no out", m(out=None)), ("remap set", m(clip_n=1, clip_T=1, clip_lo=0))]
    if lines:
        return common + [("no pool", m(pool=None)), ("res", m(res=0x1234)), ("res2", m(res2=0x1234)), ("oscale", m(oscale=0x1234, oscale_stride=64)),
                         ("cs_in != cs_out", m(cs_out=24)), ("h < 2", m(h_out=1, h_in=1)), ("generic shape", m(k=5, pad=2, ks=25, flags=1))]
    return common + [("n_in 0", m(n_in=0)), ("n_in 4", m(n_in=4)), ("cs_in % 8", m(cs_in=12)), ("cs_out % 8", m(cs_out=20)), ("k 6", m(k=6)),
                     ("stride 3", m(stride=3)), ("mt 0", m(mt=0)), ("mt 7", m(mt=7)), ("ks 0", m(ks=0)), ("ks short", m(ks=4)),
                     ("odd in_mode 1", m(in_mode=1, h_in=9)), ("nchw without sc", m(out_mode=2, sc=None, c_out=3)),
                     ("nchw dtype", m(out_mode=2, sc=0x1234, c_out=3, nchw_dtype=3)), ("nchw c_out", m(out_mode=2, sc=0x1234, c_out=4 * c0.mt + 1)),
                     ("oscale stride", m(oscale=0x1234, oscale_stride=15)), ("res with shuffle", m(res=0x1234, out_mode=1, cs_out=4)),
                     ("shuffle cs_out", m(out_mode=1, cs_out=8)), ("remap on the 3x3 path", m(clip_n=1, clip_T=1, clip_lo=0, T=1)),
                     ("remap T", m(clip_n=2, clip_T=3, clip_lo=0, T=3))]


@pytest.mark.parametrize("row", ["st1016_d2_m1", "s1016_tile_2x2_T3", "g8_mt3_cat3_clip_remap", "f3040_plain"])
def test_route_query_refuses_what_the_entry_points_refuse(row, lib):
    """The argument checks run before any launch, so both the query and the entry point answer on the host; the entry points are called with
    fake pointers only where they refuse."""
    lb, L = lib
    c = BC.by_id(row)
    for label, mut in _fail_mutations(c, c.lines):
        if label.startswith("remap") and label != "remap T" and (c.route >> 24) == BC.KG:
            continue                                             # the generic kernel implements the remap
        d = BC.fill_desc(c, BC.pointer_model(c))
        mut(d)
        assert lb.sn_conv2d_route(ctypes.byref(d), c.lines_len, NCU, None) == BC.EINVAL, (row, label)
        assert lb.sn_conv2d_route(ctypes.byref(d), c.lines_len, -1, None) == BC.EINVAL, (row, label)
        got = lb.sn_cab_stats(ctypes.byref(d), c.lines_len, None) if c.lines else lb.sn_conv2d(ctypes.byref(d), None)
        assert got == BC.EINVAL, (row, label, got)
    assert lb.sn_conv2d_route(None, 0, NCU, None) == BC.EINVAL
    assert lb.sn_cab_stats(None, 10, None) == BC.EINVAL
    d = BC.fill_desc(c, BC.pointer_model(c))
    if c.lines:
        assert lb.sn_cab_stats(ctypes.byref(d), 0, None) == BC.EINVAL
    # the generic kernel's 160 KB LDS limit: query and entry point refuse the same descriptor
    big = BC.by_id("refuse_generic_lds_160k")
    d = BC.fill_desc(big, BC.pointer_model(big))
    assert lb.sn_conv2d_route(ctypes.byref(d), 0, NCU, None) == BC.EINVAL and lb.sn_conv2d(ctypes.byref(d), None) == BC.EINVAL


def test_streaming_falls_back_to_the_tile_kernel_without_a_device(lib):
    """ncu < 0 (no device): every streaming row takes the tile kernel the entry point falls back to; a frame of 2^31 bytes does so on any device."""
    lb, L = lib
    for c in BC.CASES:
        if not BC.is_stream(c.route):
            continue
        r, plan = _route(lb, c, ncu=-1)
        mt, cs = (c.route >> 20) & 15, (c.route >> 12) & 255
        want = BC.FAST(mt, cs)
        if c.lines:                                              # the tile kernel has statistics instances for 16 and 24 channels only
            want = BC.STATS(mt, cs) if cs in (16, 24) else BC.EINVAL
        assert r == want, (c.id, L.conv_route_name(r), L.conv_route_name(want))
        if not torch.cuda.is_available():                       # ncu = 0 asks the current device: none here
            assert _route(lb, c, ncu=0)[0] == want, c.id
    big = BC.by_id("frame_2g_bytes_tile")
    assert _route(lb, big)[0] == BC.FAST(1, 16) and _route(lb, dataclasses.replace(big, h_in=8191))[0] == BC.ST(1, 16, 2, 0)
