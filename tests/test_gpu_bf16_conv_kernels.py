"""-m gpu: every instance of the bf16-storage conv (csrc/sn_conv.hip, csrc/sn_conv3p.hip) through the C ABI against float64 on the CPU, element by
element.

tests/test_gpu_parity.py::test_conv bounds whole tensors at max-abs <= 8e-3 of the tensor's peak, and the streaming kernels are otherwise only
compared with the tile kernel bit for bit.  Here each row of tests/bf16_conv_cases.py names the instance sn_conv2d / sn_cab_stats must launch
(sn_conv2d_route on the device; tests/test_host_bf16_routes.py checks the same table on the CPU), and every output element gets its own bound,
u_out |ref| + (1 + u_out) (eps M + extra) (the cases file states it).  Also per row: the pad channels are exactly 0, nothing outside the output,
the pool rows or the line buffer changes (sentinel guards), every pool row is written and each frame's rows sum to the float64 channel sums,
and a negative control -- the same op without the last 32-wide K block (one input channel where all products sit in one block) -- must break
the bound by >= 8x somewhere.  Statistics rows (sn_cab_stats) must reproduce the border rows / columns and the pool of the matching sn_conv2d
bit for bit.  Measured max |err| / M, |err| / tol and the control ratios go to parity_report_bf16_conv.json in $SN_PARITY_REPORT_DIR (default:
parity_out/ at the repository root).
"""
import ctypes
import json
import os

import pytest
import torch

import bf16_conv_cases as BC
from shiftnet_amd import prep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = BC.U
REPORT = []
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096                        # sentinel elements before and after every output buffer
SENT = 7.0


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    d = os.environ.get("SN_PARITY_REPORT_DIR") or os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report_bf16_conv.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    from shiftnet_amd import lib as L
    return L.load(), L


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape, dtype, fill):
    """(buffer, view): a view of `shape` inside a buffer with GUARD sentinel elements on both sides (16-byte aligned)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, fill):
    b = buf.float()
    g = torch.cat([b[:GUARD], b[-GUARD:]])
    return bool((g == fill).all()) if fill == fill else bool(torch.isnan(g).all())


def bound_check(name, got, ref, tol, m):
    got = got.double().cpu()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs()
    bad = err > tol
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.numel()} elements out of bound, max err/tol {(err / tol).max().item():.3g}; first at "
                             f"flat index {i} of {tuple(got.shape)}: got {got.flatten()[i].item():.9g} ref {ref.flatten()[i].item():.9g} "
                             f"tol {tol.flatten()[i].item():.3g}")
    return (err / tol).max().item(), (err / (m + 1e-30)).max().item()


class Run:
    """one row's device operands, descriptor and output buffers"""

    def __init__(self, case, ops, L):
        c = case
        dv = lambda t: t.contiguous().to(DEV)      # noqa: E731
        self.xs = [dv(x) for x in ops["xs"]]
        pk = prep.pack_conv(ops["w"], ops["bias"], list(c.cins), c.cs_in, shuffle=c.out_mode == 1)
        assert pk["mt"] == c.mt and pk["ks"] == c.ks - c.ks_extra, (c.id, pk["mt"], pk["ks"])
        wf = pk["wfrag"]
        if c.ks_extra:
            wf = torch.cat([wf, torch.zeros((c.mt, c.ks_extra, 64, 8), dtype=wf.dtype)], 1)
        self.wfrag, self.bias = dv(wf), dv(pk["bias"])
        self.keep = {k: dv(ops[k]) for k in ("oscale", "res", "res2", "sc") if k in ops}
        if c.out_mode == 2:
            dt = {BC.F32: torch.float32, BC.F16: torch.float16, BC.BF16: torch.bfloat16}[c.nchw_dtype]
            self.out_buf, self.out = guarded((c.T, c.c_out, c.h_out, c.w_out), dt, SENT)
        else:
            f = 2 if c.out_mode == 1 else 1
            self.out_buf, self.out = guarded((c.T, f * c.h_out, f * c.w_out, c.cs_out), torch.bfloat16, SENT)
        self.lines_buf = self.lines = None
        if c.lines:
            self.lines_buf, self.lines = guarded((c.T, 4, c.lines_len, c.cs_out), torch.bfloat16, SENT)
        self.ptr = {"in": [x.data_ptr() for x in self.xs], "w": self.wfrag.data_ptr(), "bias": self.bias.data_ptr(), "pool": None,
                    "out": (self.lines if c.lines else self.out).data_ptr()}
        for k in ("oscale", "res", "res2", "sc"):
            self.ptr[k] = self.keep[k].data_ptr() if k in self.keep else None
        self.pool_buf = self.pool = None
        self.rows = 0
        if c.pool:
            d = BC.fill_desc(c, dict(self.ptr, pool=None))
            d.pool = None
            self.rows = L.load().sn_conv_pool_blocks(ctypes.byref(d))      # asked before the buffer exists, as the engine does
            assert self.rows > 0, c.id
            self.pool_buf, self.pool = guarded((c.T, self.rows, 16 * c.mt), torch.float32, float("nan"))
            self.ptr["pool"] = self.pool.data_ptr()

    def desc(self, case, **over):
        p = dict(self.ptr, **over)
        return BC.fill_desc(case, p)


CONV_ROWS = [c for c in BC.CASES if c.gpu]


@pytest.mark.parametrize("case", CONV_ROWS, ids=[c.id for c in CONV_ROWS])
def test_conv_route_against_float64(case, lib):
    lb, L = lib
    c = case
    ops = BC.make_operands(c)
    run = Run(c, ops, L)
    d = run.desc(c)
    plan = (ctypes.c_int * 8)()
    r = lb.sn_conv2d_route(ctypes.byref(d), c.lines_len, 0, plan)
    assert r == c.route, (c.id, L.conv_route_name(r), L.conv_route_name(c.route))      # checked BEFORE anything is launched
    if r == BC.EINVAL:                                          # a refusal: nothing is launched, nothing written
        rc = lb.sn_cab_stats(ctypes.byref(d), c.lines_len, stream()) if c.lines else lb.sn_conv2d(ctypes.byref(d), stream())
        torch.cuda.synchronize()
        assert rc == BC.EINVAL and (run.out_buf.float() == SENT).all(), (c.id, rc)
        record(test="refusal", id=c.id, route=L.conv_route_name(r))
        return
    plan = dict(zip(L.CONV_PLAN_FIELDS, plan)) if BC.is_stream(r) else None
    if plan is not None and c.pool:
        assert run.rows == plan["pool_rows"], (c.id, run.rows, plan)       # sn_conv_pool_blocks = the rows the launch writes
    rc = lb.sn_cab_stats(ctypes.byref(d), c.lines_len, stream()) if c.lines else lb.sn_conv2d(ctypes.byref(d), stream())
    assert rc == 0, (c.id, rc)
    torch.cuda.synchronize()
    name = c.id
    ref, tol, m, e = BC.reference(c, ops)
    rec = dict(test="conv", id=c.id, route=L.conv_route_name(r), shape=[c.T, c.h_in, c.w_in, list(c.cins), c.cs_in, c.c_out, c.k, c.stride],
               eps=BC.eps_of(c), n_products=c.n_products, plan=plan)

    if c.lines:
        # the conv itself through sn_conv2d on the matching route; the line buffer / pool must be its border / pool bit for bit
        conv = Run(c, ops, L)
        dc = conv.desc(c, out=conv.out.data_ptr())
        rc2 = lb.sn_conv2d_route(ctypes.byref(dc), 0, 0, None)
        assert rc2 == BC.stats_partner(r), (c.id, L.conv_route_name(rc2))
        assert lb.sn_conv2d(ctypes.byref(dc), stream()) == 0
        torch.cuda.synchronize()
        assert guards_intact(run.lines_buf, SENT) and guards_intact(conv.out_buf, SENT), f"{name}: wrote outside its buffers"
        o = conv.out
        h, w = c.h_out, c.w_out
        bits = lambda t: t.contiguous().view(torch.int16)      # noqa: E731
        for q, want in enumerate((o[:, 0], o[:, h - 1], o[:, :, 0], o[:, :, w - 1])):
            n = w if q < 2 else h
            assert torch.equal(bits(run.lines[:, q, :n]), bits(want)), f"{name}: line {q} differs from the conv output"
            assert (run.lines[:, q, n:].float() == SENT).all(), f"{name}: line {q} written beyond its length"
        assert torch.equal(run.pool, conv.pool), f"{name}: statistics pool differs from the conv's"
        got = o
    else:
        assert guards_intact(run.out_buf, SENT), f"{name}: wrote outside its output"
        got = run.out
    if c.out_mode != 2:
        assert (got[..., c.c_log:].float() == 0).all(), f"{name}: pad channels [c_out, cs_out) not zero"
        got = got[..., :c.c_log]
    r_tol, r_m = bound_check(name, got, ref, tol, m)
    rec.update(max_err_over_M=r_m, max_err_over_tol=r_tol)
    lo, hi = BC.rounding_interval(c, ref, e)
    g64 = got.double().cpu()
    outside = (g64 < lo) | (g64 > hi)
    assert not outside.any(), (f"{name}: {int(outside.sum())} stored values are no rounding of a value within eps M + extra of ref; first: got "
                               f"{g64[outside][0].item():.9g} interval [{lo[outside][0].item():.9g}, {hi[outside][0].item():.9g}]")

    if c.pool:
        assert guards_intact(run.pool_buf, float("nan")), f"{name}: wrote past the pool rows"
        pg = run.pool.double().cpu()
        assert not torch.isnan(pg).any(), f"{name}: pool rows left unwritten ({int(torch.isnan(pg).any(2).sum())} of {c.T * run.rows})"
        assert (pg[..., c.c_out:] == 0).all(), f"{name}: pool pad channels"
        depth = BC.pool_depth(r, None if plan is None else list(plan.values()))
        s_got = pg.sum(1)[:, :c.c_out]
        s_ref = ref.sum((1, 2))
        s_tol = e.sum((1, 2)) + (depth + 8) * U * ref.abs().sum((1, 2)) + 1e-30
        rs, _ = bound_check(name + ":pool", s_got, s_ref, s_tol, s_tol)
        rec["pool_err_over_tol"] = rs

    nc, _, _, _ = BC.reference(c, ops, control=True)
    ratio = ((nc - ref).abs() / tol).max().item()
    rec["negative_control_ratio"] = ratio
    if c.nc_waiver:
        rec["negative_control_waived"] = c.nc_waiver
    else:
        assert ratio >= 8.0, f"{name}: the control without the last K block stays within {ratio:.3g}x of the bound"
    record(**rec)


def record(**kw):
    REPORT.append(kw)


# ---- the network's own descriptors ---------------------------------------------------------------------------------------------------

def test_network_convs_take_tabled_routes(monkeypatch, lib):
    """Every sn_conv2d / sn_cab_stats descriptor the engine issues takes an instance that has rows of its own in tests/bf16_conv_cases.py: whole-net
    forwards of all four variants (bf16 modules) at 5 x 48 x 64 and at 5 x 720 x 1280 -- where the 16-channel CABs run the streaming fused form
    and its statistics pass -- and one forward_clips call (2 clips of 5 x 48 x 64; rconcat's per-clip remap).  The report lists what was taken
    (route_census).  The network never takes, and only the table runs: the tile kernel's conv3_fast<3,40>, <3,48>, <4,64> and both statistics
    instances (the engine streams those convs); conv3p<1,16,*,MODE 2> (the library keeps 16-channel scale + residual on the tile kernel), every
    D3 / D4 instance (measurement flags), conv3p<2,24,D2,MODE2> (register residual, a measurement flag), the MODE 0 and MODE 3 instances of
    2024 / 3040 / 3048 / 4064 (conv_trans and the fused-CAB statistics pass are 16-channel convs); conv_mfma<1,4,16>, <2,4,16> and <6,4,16>."""
    from shiftnet_amd import synth
    from shiftnet_amd.arch import CLASSES
    from shiftnet_amd.engine import Engine
    from shiftnet_amd.spec import VARIANTS
    from shiftnet_amd.weights import synth_state_dict
    lb, L = lib
    seen = {}
    orig = Engine._call

    def spy(self, fn, label, *args):
        if fn in ("sn_conv2d", "sn_cab_stats"):
            r = lb.sn_conv2d_route(args[0], args[1] if fn == "sn_cab_stats" else 0, 0, None)
            seen.setdefault(r, label)
        return orig(self, fn, label, *args)
    monkeypatch.setattr(Engine, "_call", spy)
    for name in VARIANTS:
        net = CLASSES[name](past_frames=2, future_frames=2)
        net.load_state_dict(synth_state_dict(name), strict=True)
        net = net.to(torch.bfloat16).to(DEV).eval()
        V = VARIANTS[name]
        for (T, h, w, B) in ((5, 48, 64, 0), (5, 720, 1280, 0), (5, 48, 64, 2)):
            x = torch.stack([torch.from_numpy(synth.unit_noise((T, 3, h, w), seed=7 + b)).abs().clamp(0, 1) for b in range(max(B, 1))])
            x = x.to(torch.bfloat16).to(DEV)
            nm = torch.full((max(B, 1), T, 1, h, w), 30.0 / 255.0, dtype=torch.bfloat16, device=DEV) if V.denoise else None
            with torch.no_grad():
                args = (x,) if nm is None else (x, nm)
                out = net.forward_clips(*args) if B else net(*args)
            torch.cuda.synchronize()
            assert torch.isfinite(out.float()).all(), (name, T, h, w, B)
        del net
        torch.cuda.empty_cache()
    assert seen, "no sn_conv2d / sn_cab_stats call recorded"
    tabled = {c.route for c in BC.CASES}
    record(test="route_census", id="all_variants", taken=sorted(L.conv_route_name(r) for r in seen),
           never_taken=sorted(L.conv_route_name(r) for r in BC.ALL_ROUTES if r not in seen))
    missing = {L.conv_route_name(r): lbl for r, lbl in seen.items() if r not in tabled or r < 0}
    assert not missing, missing
