"""CPU tests of sn32_conv2d_route (include/shiftnet_hip.h): the kernel instance sn32_conv2d launches, computed on the host from the descriptor.

The GPU kernel table (tests/fp32_cases.py, run by tests/test_gpu_fp32_kernels.py) declares a route per row and arithmetic; here every declared
route must be the one the library selects, and the rows together must reach every instance the selector can return, so an instance that
appears in the dispatch without a row of its own fails this test."""
import ctypes

import pytest

import fp32_cases as FC


@pytest.fixture(scope="module")
def lib():
    from shiftnet_amd import lib as L
    return L.load(), L


@pytest.mark.parametrize("case", FC.CASES, ids=[c.id for c in FC.CASES])
def test_declared_route_is_the_selected_route(case, lib):
    lb, L = lib
    for mode, want in case.routes.items():
        c = FC.for_mode(case, mode)
        d = FC.fill_desc(L, c, mode, FC.pointer_model(c), FC.fake_strides(c))
        got = lb.sn32_conv2d_route(ctypes.byref(d))
        assert got == want, (case.id, mode, FC.route_name(got), FC.route_name(want))


def test_cases_cover_every_instance_of_the_selector():
    declared = {r for c in FC.CASES for r in c.routes.values()}
    missing = [FC.route_name(r) for r in FC.ALL_ROUTES if r not in declared]
    unknown = [FC.route_name(r) for r in declared if r not in FC.ALL_ROUTES]
    assert not missing and not unknown, (missing, unknown)
    # every instance is run in each arithmetic it exists in: split instances by split rows, the others by exact rows
    for r in FC.ALL_ROUTES:
        modes = {m for c in FC.CASES for m, rr in c.routes.items() if rr == r}
        assert ("split" in modes) if FC.is_split(r) else ("exact" in modes), (FC.route_name(r), modes)


def test_route_query_refuses_what_sn32_conv2d_refuses(lib):
    lb, L = lib
    case = FC.CASES[0]
    d = FC.fill_desc(L, case, "split", FC.pointer_model(case), FC.fake_strides(case))
    d.k = 3
    d.ln_w = d.ln_b = FC.pointer_model(case)["ln_w"]             # LayerNorm on load exists for the flat 1x1 kernel only
    assert lb.sn32_conv2d_route(ctypes.byref(d)) == -22
    assert lb.sn32_conv2d(ctypes.byref(d), None) == -22
    assert lb.sn32_conv2d_route(None) == -22


def test_selector_only_returns_listed_instances(lib):
    """Sweep the selector's inputs (kernel size, stride, groups, widths, alignment, optional operands) on the host: every answer is SN_EINVAL
    or an instance of fp32_cases.ALL_ROUTES."""
    lb, L = lib
    seen = set()
    base = FC.Case(id="sweep", routes={}, cins=(32,), c_out=32)
    for k in (1, 2, 3, 5):
        for stride in (1, 2):
            for cin, cout, groups in ((32, 48, 1), (160, 80, 1), (8, 12, 1), (16, 16, 2), (48, 48, 6), (80, 80, 10), (40, 40, 40), (6, 6, 6), (16, 16, 4)):
                for hw in ((1, 1), (8, 8), (4, 33)):
                    for off in (0, 2):
                        for mode in ("split", "exact"):
                            for in_mode in (0, 1):
                                c = FC.Case(id="sweep", routes={}, cins=(cin,), c_out=cout, k=k, stride=stride, groups=groups, h_in=2 * hw[0],
                                            w_in=2 * hw[1], in_mode=in_mode, in_off=(off,), cs_extra=(off,))
                                d = FC.fill_desc(L, c, mode, FC.pointer_model(c), FC.fake_strides(c))
                                r = lb.sn32_conv2d_route(ctypes.byref(d))
                                assert r == -22 or r in FC.ALL_ROUTES, (k, stride, cin, cout, groups, hw, off, mode, in_mode, FC.route_name(r))
                                seen.add(r)
    assert base.c_out == 32 and len(seen - {-22}) >= 15
