"""-m gpu: every kernel of the fp32 engine (csrc/sn_f32.hip) through the C ABI against float64 on the CPU, element by element.

tests/test_gpu_fp32.py compares whole blocks at max-abs <= 1e-4 of the tensor's maximum; an element 100x below the maximum can be wrong by all
of itself there.  Here each output element has its own bound, eps * M with M = conv(|x|, |w|) + |bias| carried through the epilogue
(tests/fp32_cases.py states eps per route), and each conv row of the kernel table names the instance sn32_conv2d must launch for it
(sn32_conv2d_route; tests/test_host_fp32_routes.py checks the same table on the CPU).  Split rows also run a negative control: the same op with
bf16-only products must exceed the bound by >= 8x somewhere, so a kernel that lost its lo terms would fail.  Every measured max |err| / M goes
to parity_report_fp32.json in $SN_PARITY_REPORT_DIR (default: parity_out/ at the repository root).

Reductions (channel sums, LayerNorm) are bounded the same way: (n + 8) 2^-24 * sum |terms| for n fp32 additions.  Claims of bit identity the
header makes (sn32_dw_gate, sn32_gate_sum, sn32_gsts_shiftconv) are asserted with torch.equal.
"""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp32_cases as FC
from oracle import shiftnet_oracle as O
from shiftnet_amd import prep, synth
from shiftnet_amd.spec import VARIANTS, shift_table
from shiftnet_amd.weights import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = FC.U
REPORT = []
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    d = os.environ.get("SN_PARITY_REPORT_DIR") or os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report_fp32.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    from shiftnet_amd import lib as L
    return L.load(), L


def stream():
    return torch.cuda.current_stream().cuda_stream


def check_rc(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def record(**kw):
    REPORT.append(kw)


def bound_check(name, got, ref, tol, m=None):
    """|got - ref| <= tol element-wise (float64); returns max |err| / tol and max |err| / m."""
    got = got.double().cpu()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs()
    r_tol = (err / tol).max().item()
    r_m = (err / (m + 1e-30)).max().item() if m is not None else None
    bad = err > tol
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {err.numel()} elements out of bound, max err/tol {r_tol:.3g}; first at flat index {i}: "
                             f"got {got.flatten()[i].item():.9g} ref {ref.flatten()[i].item():.9g} tol {tol.flatten()[i].item():.3g}")
    return r_tol, r_m


# ---- the conv kernel table ---------------------------------------------------------------------------------------------------------------

CONV_RUNS = [(c, m) for c in FC.CASES for m in ("exact", "split") if m in c.routes]


@pytest.mark.parametrize("case,mode", CONV_RUNS, ids=[f"{c.id}-{m}" for c, m in CONV_RUNS])
def test_conv_route_against_float64(case, mode, lib):
    lb, L = lib
    c = FC.for_mode(case, mode)
    r = case.routes[mode]
    ops = FC.make_operands(c)
    T, ho, wo = c.T, c.h_out, c.w_out
    dv = lambda t: t.contiguous().to(DEV)      # noqa: E731  (one allocation per operand: the alignment tests/fp32_cases.py models)
    xs = [dv(x) for x in ops["xs"]]
    keep = {"xs": xs}
    ptr = {"in": [x.data_ptr() + 4 * c.in_off_(i) for i, x in enumerate(xs)]}
    keep["w"] = dv(ops["w"].permute(2, 3, 1, 0))
    ptr["w"] = keep["w"].data_ptr()
    strides = {"oscale": 0, "iscale": 0, "rscale": 0}
    for name in ("bias", "oscale", "iscale", "rscale", "res", "ln_w", "ln_b", "sc"):
        if ops.get(name) is not None:
            keep[name] = dv(ops[name])
            ptr[name] = keep[name].data_ptr()
        else:
            ptr[name] = None
    if c.oscale is not None:
        strides["oscale"] = ops["oscale_st"]
    if c.iscale:
        strides["iscale"] = keep["iscale"].stride(0)
    if c.rscale:
        strides["rscale"] = keep["rscale"].stride(0)
    packable = c.groups == 1 or (sum(c.cins) // c.groups == 8 and c.c_out // c.groups == 8 and c.c_out % 16 == 0 and c.k in (3, 5))
    keep["wsplit"] = None
    if mode == "split":          # depthwise / direct rows: the descriptor carries fragments, which those kernels never read
        keep["wsplit"] = prep.pack_conv32_split(ops["w"], c.groups).to(DEV) if packable else torch.zeros(64, device=DEV)
    ptr["wsplit"] = keep["wsplit"].data_ptr() if keep["wsplit"] is not None else None
    SENT = 7.0
    if c.out_mode == 0:
        out = torch.full((T, ho, wo, c.cs_out), SENT, device=DEV)
        ptr["out"] = out.data_ptr() + 4 * c.out_off
    elif c.out_mode == 1:
        out = torch.full((T, 2 * ho, 2 * wo, c.c_out // 4), SENT, device=DEV)
        ptr["out"] = out.data_ptr()
    else:
        dt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[c.nchw_dtype]
        out = torch.full((T, c.c_out, ho, wo), SENT, dtype=dt, device=DEV)
        ptr["out"] = out.data_ptr()
    csum = None
    if c.csum is not None:
        tiles = lb.sn32_conv_csum_tiles(ho, wo)
        csum = torch.full((T, tiles, c.csum), SENT, device=DEV)
        ptr["csum"] = csum.data_ptr()
    d = FC.fill_desc(L, c, mode, ptr, strides)
    assert lb.sn32_conv2d_route(ctypes.byref(d)) == r, (case.id, mode, FC.route_name(lb.sn32_conv2d_route(ctypes.byref(d))), FC.route_name(r))
    check_rc(lb.sn32_conv2d(ctypes.byref(d), stream()), f"sn32_conv2d[{case.id}]")
    torch.cuda.synchronize()
    ref, tol, m = FC.reference(c, ops, r)
    name = f"{case.id}-{mode}"
    if c.out_mode == 0:
        got = out[..., c.out_off: c.out_off + c.c_out]
        rest = torch.cat([out[..., :c.out_off], out[..., c.out_off + c.c_out:]], -1)
        assert (rest == SENT).all(), f"{name}: wrote outside its channel slice"
    else:
        got = out
    r_tol, r_m = bound_check(name, got, ref, tol, m)
    rec = dict(test="conv", id=case.id, mode=mode, route=FC.route_name(r), shape=[T, c.h_in, c.w_in, list(c.cins), c.c_out, c.k, c.stride],
               max_err_over_M=r_m, max_err_over_tol=r_tol, eps_start=FC.eps_of(c, r))
    if csum is not None:
        # per-workgroup channel sums of the stored output: tiles of SN_C32S_TH3 = 4 rows x 32 columns, row-major over the frame
        th, tw = 4, 32
        ty, tx = -(-ho // th), -(-wo // tw)
        assert csum.shape[1] == ty * tx
        pad = lambda t: F.pad(t, (0, 0, 0, tx * tw - wo, 0, ty * th - ho))      # noqa: E731
        ts = lambda t: pad(t).reshape(T, ty, th, tx, tw, -1).sum((2, 4)).reshape(T, ty * tx, -1)      # noqa: E731
        ref_s = ts(ref)
        tol_s = ts(tol) + (th * tw + 8) * U * ts(ref.abs())
        got_s = csum.double().cpu()
        assert (got_s[..., c.c_out:] == 0).all(), f"{name}: csum pad channels"
        rs, _ = bound_check(name + ":csum", got_s[..., :c.c_out], ref_s, tol_s)
        rec["csum_err_over_tol"] = rs
    if FC.is_split(r):
        nc, _, _ = FC.reference(c, ops, r, bf16_products=True)
        ratio = ((nc - ref).abs() / tol).max().item()
        rec["negative_control_ratio"] = ratio
        if c.nc:
            assert ratio >= 8.0, f"{name}: bf16-only products stay within {ratio:.3g}x of the bound: the bound cannot see lost lo terms"
        else:
            rec["negative_control_waived"] = FC.NC_WAIVED
    record(**rec)


# ---- sn32_conv1x1_gate2 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,C,T,hw", [(32, 16, 1, 64), (60, 32, 3, 64), (96, 48, 2, 192), (128, 80, 3, 128), (16, 64, 1, 320)])
def test_conv1x1_gate2_against_float64(cin, C, T, hw, lib):
    lb, L = lib
    g = torch.Generator().manual_seed(cin * 7 + C)
    cs = cin + 4
    x = torch.randn((T, hw, cs), generator=g)
    w = (torch.randn((2 * C, cin, 1, 1), generator=g) / math.sqrt(cin)).float()
    cpad = C + 8
    xd, ws = x.to(DEV), prep.pack_conv32_split(w, 1).to(DEV)
    out = torch.full((T, hw, C), 7.0, device=DEV)
    nblk = hw // 64
    part = torch.full((T * nblk, cpad), 7.0, device=DEV)
    check_rc(lb.sn32_conv1x1_gate2(xd.data_ptr(), cs, cin, ws.data_ptr(), C, cpad, out.data_ptr(), T, hw, part.data_ptr(), stream()), "gate2")
    torch.cuda.synchronize()
    x64, w64 = x[..., :cin].double(), w[:, :, 0, 0].double()
    eps = 3e-5 + (3 * math.ceil(cin / 32) + 8) * U

    def gated(xx, ww):
        a = xx @ ww.t()
        return a[..., :C] * torch.sigmoid(a[..., C:]), a
    ref, a = gated(x64, w64)
    m = x64.abs() @ w64.abs().t()
    s = torch.sigmoid(a[..., C:])
    tol = eps * (m[..., :C] * s + a[..., :C].abs() * s * (1 - s) * m[..., C:]) + 16 * U * ref.abs() + 1e-30
    r_tol, r_m = bound_check(f"gate2_{cin}_{C}_{T}_{hw}", out, ref, tol, m[..., :C])
    ref_p = ref.reshape(T * nblk, 64, C).sum(1)
    tol_p = tol.reshape(T * nblk, 64, C).sum(1) + 72 * U * ref.abs().reshape(T * nblk, 64, C).sum(1)
    pg = part.double().cpu()
    assert (pg[:, C:] == 0).all()
    rp, _ = bound_check(f"gate2_partial_{cin}_{C}", pg[:, :C], ref_p, tol_p)
    nc, _ = gated(x64.float().bfloat16().double(), w64.float().bfloat16().double())
    ratio = ((nc - ref).abs() / tol).max().item()
    record(test="conv1x1_gate2", id=f"cin{cin}_C{C}_T{T}_hw{hw}", mode="split", route=f"conv32s_1x1<{(cin + 31) // 32},gate>", shape=[T, hw, cin, C],
           max_err_over_M=r_m, max_err_over_tol=r_tol, partial_err_over_tol=rp, eps_start=eps, negative_control_ratio=ratio)
    assert ratio >= 8.0, ratio


# ---- elementwise kernels and reductions -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,mean", [(1, 0.0), (15, 0.0), (16, 0.0), (17, 0.0), (128, 0.0), (64, 100.0), (64, 1000.0), (17, 1000.0)])
def test_layernorm_against_float64(K, mean, lib):
    lb, L = lib
    g = torch.Generator().manual_seed(K + int(mean))
    npix, cs_x, cs_o = 111, K + 3, K + 5
    x = (torch.randn((npix, cs_x), generator=g) + mean * (1 + 0.1 * torch.rand((npix, 1), generator=g))).float()
    w = (1 + 0.5 * torch.randn(K, generator=g)).float()
    b = (0.3 * torch.randn(K, generator=g)).float()
    out = torch.full((npix, cs_o), 7.0, device=DEV)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    check_rc(lb.sn32_layernorm(xd.data_ptr(), cs_x, K, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), cs_o, npix, stream()), "layernorm")
    torch.cuda.synchronize()
    x64 = x[:, :K].double()
    mu = x64.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt((x64 - mu).pow(2).mean(1, keepdim=True) + 1e-6)
    ref = (x64 - mu) * rstd * w.double() + b.double()
    tol = 16 * U * (x64.abs().mean(1, keepdim=True) + (x64 - mu).abs()) * rstd * w.double().abs() + 4 * U * (b.double().abs() + ref.abs()) + 1e-30
    r_tol, _ = bound_check(f"layernorm_{K}_{mean}", out[:, :K], ref, tol)
    assert (out[:, K:] == 7.0).all()
    record(test="layernorm", id=f"K{K}_mean{mean}", mode="-", route="layernorm32", shape=[npix, K], max_err_over_tol=r_tol)


def _gate_ref(a64, C, mode):
    x1, x2 = a64[..., :C], a64[..., C:]
    return x1 * torch.sigmoid(x2) if mode else x1 * x2


def _gate_input(T, hw, C, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((T, hw, 2 * C), generator=g)
    a[..., C::7] = 30.0                                   # SimpleGate2's sigmoid at +-30
    a[..., C + 3::7] = -30.0
    return a.float()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("T,hw,C,cpad,nblk", [(1, 5, 16, 16, 8), (3, 111, 72, 80, 8), (2, 64, 40, 48, 64), (2, 37, 250, 256, 3)])
def test_gate_gate_sum_chan_sum(mode, T, hw, C, cpad, nblk, lib):
    """sn32_gate / sn32_gate_sum against float64, their outputs bit-identical; the sums of sn32_gate_sum bit-identical to sn32_chan_sum of the
    sn32_gate output (header); each block's sum against float64 of the pixels that block owns (h w below nblk, ragged blocks)."""
    lb, L = lib
    a = _gate_input(T, hw, C, seed=hw + C + mode)
    ad = a.to(DEV)
    o1 = torch.full((T, hw, C), 7.0, device=DEV)
    o2 = torch.full((T, hw, C), 7.0, device=DEV)
    p2 = torch.full((T, nblk, cpad), 7.0, device=DEV)
    p3 = torch.full((T, nblk, cpad), 7.0, device=DEV)
    check_rc(lb.sn32_gate(ad.data_ptr(), C, mode, o1.data_ptr(), T * hw, stream()), "gate")
    check_rc(lb.sn32_gate_sum(ad.data_ptr(), C, cpad, mode, o2.data_ptr(), T, hw, nblk, p2.data_ptr(), stream()), "gate_sum")
    check_rc(lb.sn32_chan_sum(o1.data_ptr(), C, C, cpad, T, hw, nblk, p3.data_ptr(), stream()), "chan_sum")
    torch.cuda.synchronize()
    ref = _gate_ref(a.double(), C, mode)
    tol = 16 * U * ref.abs() + 1e-30
    r_tol, _ = bound_check(f"gate_{mode}", o1, ref, tol)
    assert torch.equal(o1, o2), "sn32_gate_sum output != sn32_gate output"
    assert torch.equal(p2, p3), "sn32_gate_sum sums != sn32_chan_sum of the sn32_gate output"
    # chan_sum32_kernel: pixel i of a frame belongs to block (i // nsplit) % nblk, nsplit = 256 // cpad
    nsplit = 256 // cpad
    owner = (torch.arange(hw) // nsplit) % nblk
    g64 = o1.double().cpu()
    ref_p = torch.zeros((T, nblk, C), dtype=torch.float64)
    abs_p = torch.zeros((T, nblk, C), dtype=torch.float64)
    cnt = torch.zeros(nblk)
    ref_p.index_add_(1, owner, g64)
    abs_p.index_add_(1, owner, g64.abs())
    cnt.index_add_(0, owner, torch.ones(hw))
    tol_p = (cnt.view(1, -1, 1).double() + 8) * U * abs_p + 1e-30
    pg = p3.double().cpu()
    assert (pg[..., C:] == 0).all()
    rp, _ = bound_check("chan_sum", pg[..., :C], ref_p, tol_p)
    record(test="gate_sum", id=f"mode{mode}_T{T}_hw{hw}_C{C}_cpad{cpad}_nblk{nblk}", mode="-", route="gate32/gate_sum32/chan_sum32",
           shape=[T, hw, C], max_err_over_tol=r_tol, partial_err_over_tol=rp)


@pytest.mark.parametrize("with_x", [False, True])
def test_scale_residual_against_float64(with_x, lib):
    lb, L = lib
    g = torch.Generator().manual_seed(3 + with_x)
    T, hw, C, st = 3, 37, 20, 28
    r = torch.randn((T, hw, C), generator=g)
    x = torch.randn((T, hw, C), generator=g)
    ca = (torch.rand((T, st), generator=g) + torch.arange(T).view(-1, 1)).float()
    out = torch.empty((T, hw, C), device=DEV)
    rd, xd, cad = r.to(DEV), x.to(DEV), ca.to(DEV)
    check_rc(lb.sn32_scale_residual(rd.data_ptr(), xd.data_ptr() if with_x else None, cad.data_ptr(), st, out.data_ptr(), T, hw, C, stream()), "scale_res")
    torch.cuda.synchronize()
    ref = r.double() * ca[:, :C].double().view(T, 1, C) + (x.double() if with_x else 0)
    tol = 2 * U * (r.double().abs() * ca[:, :C].double().view(T, 1, C) + (x.double().abs() if with_x else 0)) + 1e-30
    r_tol, _ = bound_check("scale_residual", out, ref, tol)
    record(test="scale_residual", id=f"x{int(with_x)}", mode="-", route="scale_res32", shape=[T, hw, C], max_err_over_tol=r_tol)


@pytest.mark.parametrize("dt", [0, 1, 2])
@pytest.mark.parametrize("noise", [False, True])
def test_ingest_is_exact(dt, noise, lib):
    lb, L = lib
    tdt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dt]
    g = torch.Generator().manual_seed(dt)
    T, Cc, H, W = 3, 3, 17, 19
    src = torch.rand((T, Cc, H, W), generator=g).to(tdt)
    nm = torch.rand((T, 1, H, W), generator=g).to(tdt)
    CD = Cc + (1 if noise else 0)
    dst = torch.full((T, H, W, CD), 7.0, device=DEV)
    sd, nd = src.to(DEV), nm.to(DEV)
    check_rc(lb.sn32_ingest(sd.data_ptr(), dt, nd.data_ptr() if noise else None, dst.data_ptr(), T, Cc, H, W, stream()), "ingest")
    torch.cuda.synchronize()
    ref = torch.cat([src, nm], 1) if noise else src
    assert torch.equal(dst.cpu(), ref.float().permute(0, 2, 3, 1))


# ---- sn32_dw_gate == depthwise sn32_conv2d (res = a) + sn32_gate ----------------------------------------------------------------------------

@pytest.mark.parametrize("T,h,w,C,nblk", [(2, 2, 3, 16, 8), (3, 5, 7, 80, 4), (1, 9, 13, 64, 5), (2, 1, 1, 32, 2), (1, 16, 48, 64, 64)])
def test_dw_gate_is_depthwise_conv_plus_gate(T, h, w, C, nblk, lib):
    lb, L = lib
    g = torch.Generator().manual_seed(h * w + C)
    cs = 2 * C + 8
    a = torch.randn((T, h, w, cs), generator=g)
    wt = (torch.randn((9, 2 * C), generator=g) / 3).float()
    ad, wd = a.to(DEV), wt.to(DEV)
    cpad = C + 8 if C + 8 <= 256 else C
    out = torch.full((T, h, w, C), 7.0, device=DEV)
    part = torch.full((T, nblk, cpad), 7.0, device=DEV)
    check_rc(lb.sn32_dw_gate(ad.data_ptr(), cs, wd.data_ptr(), C, cpad, out.data_ptr(), T, h, w, nblk, part.data_ptr(), stream()), "dw_gate")
    # the unfused pair: depthwise conv (dw32_kernel) with the input as its residual, then SimpleGate
    mid = torch.empty((T, h, w, 2 * C), device=DEV)
    d = L.Conv32Desc()
    d.inp[0], d.c_in[0], d.cs_in[0], d.n_in = ad.data_ptr(), 2 * C, cs, 1
    d.T, d.h_in, d.w_in, d.h_out, d.w_out = T, h, w, h, w
    d.k, d.stride, d.pad, d.groups, d.c_out = 3, 1, 1, 2 * C, 2 * C
    d.w, d.res, d.cs_res, d.out, d.cs_out = wd.data_ptr(), ad.data_ptr(), cs, mid.data_ptr(), 2 * C
    assert lb.sn32_conv2d_route(ctypes.byref(d)) == FC.route(FC.K_DW)
    check_rc(lb.sn32_conv2d(ctypes.byref(d), stream()), "dw conv")
    o2 = torch.empty((T, h, w, C), device=DEV)
    check_rc(lb.sn32_gate(mid.data_ptr(), C, 0, o2.data_ptr(), T * h * w, stream()), "gate")
    torch.cuda.synchronize()
    assert torch.equal(out, o2), "sn32_dw_gate != sn32_conv2d(depthwise, res = a) + sn32_gate"
    # against float64, and each block's sums: block b owns the pixels [b chunk, (b + 1) chunk) of its frame
    a64 = a[..., :2 * C].double().permute(0, 3, 1, 2)
    w64 = wt.double().t().reshape(2 * C, 1, 3, 3)
    ap = F.conv2d(a64, w64, padding=1, groups=2 * C) + a64
    mp = F.conv2d(a64.abs(), w64.abs(), padding=1, groups=2 * C) + a64.abs()
    ref = (ap[:, :C] * ap[:, C:]).permute(0, 2, 3, 1)
    tol = (13 * U * (mp[:, :C] * ap[:, C:].abs() + ap[:, :C].abs() * mp[:, C:]) + 1e-30).permute(0, 2, 3, 1)
    r_tol, _ = bound_check("dw_gate", out, ref, tol)
    chunk = -(-h * w // nblk)
    g64 = out.double().cpu().reshape(T, h * w, C)
    owner = torch.clamp(torch.arange(h * w) // chunk, max=nblk - 1)
    ref_p = torch.zeros((T, nblk, C), dtype=torch.float64).index_add_(1, owner, g64)
    abs_p = torch.zeros((T, nblk, C), dtype=torch.float64).index_add_(1, owner, g64.abs())
    pg = part.double().cpu()
    assert (pg[..., C:] == 0).all()
    rp, _ = bound_check("dw_gate_partial", pg[..., :C], ref_p, (chunk + 8) * U * abs_p + 1e-30)
    record(test="dw_gate", id=f"T{T}_{h}x{w}_C{C}_nblk{nblk}", mode="-", route="dwgate32", shape=[T, h, w, C], max_err_over_tol=r_tol,
           partial_err_over_tol=rp)


# ---- sn32_gsts_gather / sn32_gsts_shiftconv: index work, bit-exact ------------------------------------------------------------------------

def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("name", list(VARIANTS))
@pytest.mark.parametrize("hw", [(24, 24), (6, 10), (3, 5), (1, 1)])
def test_gsts_gather_and_shiftconv_bit_exact(name, hw, lib):
    """sn32_gsts_gather (with and without the spatial shift, u2) against O.gsts_gather / O.temporal_roll, whole clip and a frame range; and
    sn32_gsts_shiftconv (both forms) against gather + the depthwise conv1 it replaces."""
    lb, L = lib
    V = O.VARIANTS[name]
    C, T = V.c1, 5
    h, w = hw
    x = torch.from_numpy(synth.unit_noise((T, C, h, w), seed=h * 31 + w))
    xd = _nhwc(x).to(DEV)
    offs = prep.shift_offsets_i8(shift_table(C)).to(DEV)
    for mode, rev in ((1, False), (2, True)):
        wrap = 1 if V.wrap else 0
        ref_u = _nhwc(O.gsts_gather(x, rev, V.wrap))
        ref_y = _nhwc(O.temporal_roll(x, rev, V.wrap)[0])
        for (t0, nt) in ((0, 0), (1, 3)):
            s = L.UnitSrc(xd.data_ptr(), T, h, w, C, mode, wrap, None, t0, nt)
            u = torch.full((T, h, w, C + C // 2), 7.0, device=DEV)
            u2 = torch.full((T, h, w, C + C // 2), 7.0, device=DEV)
            y = torch.full((T, h, w, C), 7.0, device=DEV)
            check_rc(lb.sn32_gsts_gather(ctypes.byref(s), offs.data_ptr(), u.data_ptr(), u2.data_ptr(), stream()), "gather")
            check_rc(lb.sn32_gsts_gather(ctypes.byref(s), None, y.data_ptr(), None, stream()), "roll")
            torch.cuda.synchronize()
            fr = slice(t0, t0 + nt) if nt else slice(0, T)
            assert torch.equal(u[fr].cpu(), ref_u[fr]), (name, hw, mode, t0, nt)
            assert torch.equal(u2[fr, ..., :C].cpu(), ref_u[fr, ..., :C]), (name, hw, mode, t0, nt)
            assert torch.equal(y[fr].cpu(), ref_y[fr]), (name, hw, mode, t0, nt)
            if nt:
                assert (u[:t0] == 7.0).all() and (u[t0 + nt:] == 7.0).all()         # frames outside the range untouched
            # shiftconv: vin[:, :C] = roll(x); u = shifted half (separate conv1), or vin[:, C:] = conv1(shifted half) in the kernel
            wk = (torch.randn((9, C // 2), generator=torch.Generator().manual_seed(C)) / 3).float().to(DEV)
            vin_a = torch.full((T, h, w, C + C // 2), 7.0, device=DEV)
            vin_b = torch.full((T, h, w, C + C // 2), 7.0, device=DEV)
            us = torch.full((T, h, w, C // 2), 7.0, device=DEV)
            check_rc(lb.sn32_gsts_shiftconv(ctypes.addressof(s), offs.data_ptr(), None, vin_a.data_ptr(), us.data_ptr(), stream()), "shiftconv u")
            check_rc(lb.sn32_gsts_shiftconv(ctypes.addressof(s), offs.data_ptr(), wk.data_ptr(), vin_b.data_ptr(), None, stream()), "shiftconv w")
            torch.cuda.synchronize()
            assert torch.equal(vin_a[fr, ..., :C].cpu(), ref_u[fr, ..., :C]) and torch.equal(vin_b[fr, ..., :C].cpu(), ref_u[fr, ..., :C])
            assert torch.equal(us[fr].cpu(), ref_u[fr, ..., C:])
            # conv1 of the gather output through the depthwise sn32_conv2d: the same taps in the same order
            conv = torch.empty((T, h, w, C // 2), device=DEV)
            ushift = u[..., C:]
            d = L.Conv32Desc()
            d.inp[0], d.c_in[0], d.cs_in[0], d.n_in = ushift.data_ptr(), C // 2, C + C // 2, 1
            d.T, d.h_in, d.w_in, d.h_out, d.w_out = T, h, w, h, w
            d.k, d.stride, d.pad, d.groups, d.c_out = 3, 1, 1, C // 2, C // 2
            d.w, d.out, d.cs_out = wk.data_ptr(), conv.data_ptr(), C // 2
            check_rc(lb.sn32_conv2d(ctypes.byref(d), stream()), "conv1")
            torch.cuda.synchronize()
            assert torch.equal(vin_b[fr, ..., C:], conv[fr]), (name, hw, mode, t0, nt, "shiftconv(w) != gather + conv1")


@pytest.mark.parametrize("hw", [(6, 10), (3, 5), (1, 1)])
def test_gsts_gather_halo_wrap2(hw, lib):
    """wrap = 2: the unit's boundary frames read their neighbour from the halo tensor (a temporally split window): the result equals the
    gather of the clip extended by the halo frame, cut back to the window, for both directions and a frame range."""
    lb, L = lib
    V = O.VARIANTS["gshift_deblur1"]
    C, T = V.c1, 4
    h, w = hw
    x = torch.from_numpy(synth.unit_noise((T + 2, C, h, w), seed=7 + h))
    offs = prep.shift_offsets_i8(shift_table(C)).to(DEV)
    for mode, rev in ((1, False), (2, True)):
        win = x[1:T + 1]
        halo = _nhwc(x[0:1])[..., C // 2:] if not rev else _nhwc(x[T + 1:T + 2])[..., :C // 2]       # the neighbour's borrowed half
        ext = x[0:T + 1] if not rev else x[1:T + 2]
        full = _nhwc(O.gsts_gather(ext, rev, False))
        ref = full[1:] if not rev else full[:T]
        xd, hd = _nhwc(win).to(DEV), halo.contiguous().to(DEV)
        for (t0, nt) in ((0, 0), (1, 2)):
            s = L.UnitSrc(xd.data_ptr(), T, h, w, C, mode, 2, hd.data_ptr(), t0, nt)
            u = torch.full((T, h, w, C + C // 2), 7.0, device=DEV)
            check_rc(lb.sn32_gsts_gather(ctypes.byref(s), offs.data_ptr(), u.data_ptr(), None, stream()), "gather halo")
            vin = torch.full((T, h, w, C + C // 2), 7.0, device=DEV)
            us = torch.full((T, h, w, C // 2), 7.0, device=DEV)
            check_rc(lb.sn32_gsts_shiftconv(ctypes.addressof(s), offs.data_ptr(), None, vin.data_ptr(), us.data_ptr(), stream()), "shiftconv halo")
            torch.cuda.synchronize()
            fr = slice(t0, t0 + nt) if nt else slice(0, T)
            assert torch.equal(u[fr].cpu(), ref[fr]), (hw, mode, t0, nt)
            assert torch.equal(vin[fr, ..., :C].cpu(), ref[fr, ..., :C]) and torch.equal(us[fr].cpu(), ref[fr, ..., C:]), (hw, mode, t0, nt)


# ---- through the engine: the closed-form CALayer (sn32_cab_ca), odd-size whole nets, the routes the network takes ------------------------

def _close(name, got, ref, tol=1e-4):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = max(1.0, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    assert np.isfinite(err) and err <= tol * scale, f"{name}: max-abs {err:.3g} > {tol} * {scale:.3g}"
    return err / scale


class _Mode:
    """Engine32's arithmetic (split_bf16) and operator chain (fuse_ops) for the duration of a block."""

    def __init__(self, split, fuse=None):
        self.split, self.fuse = split, fuse

    def __enter__(self):
        from shiftnet_amd.engine32 import Engine32
        self.old = (Engine32.split_bf16, Engine32.fuse_ops)
        Engine32.split_bf16 = self.split
        if self.fuse is not None:
            Engine32.fuse_ops = self.fuse

    def __exit__(self, *a):
        from shiftnet_amd.engine32 import Engine32
        Engine32.split_bf16, Engine32.fuse_ops = self.old


@pytest.mark.parametrize("mode", ["exact", "split"])
def test_cab_closed_form_at_small_sizes(mode):
    """Engine32.cab: the CALayer scale in closed form (sn32_cab_ca: border / corner corrections of the pooled conv2 output, which overlap at
    h or w = 2) against O.cab, both operator chains; h or w = 1 takes the engine's fallback."""
    from shiftnet_amd.engine import Act, make_engine
    name = "gshift_deblur1"
    sd = synth_state_dict(name)
    V = O.VARIANTS[name]
    eng = make_engine(VARIANTS[name], sd, DEV, torch.float32)
    for (h, w) in ((2, 2), (2, 9), (9, 2), (3, 3), (23, 41), (1, 7), (5, 1)):
        x0 = torch.from_numpy(synth.unit_noise((3, V.c0, h, w), seed=h * 50 + w))
        ref = O.cab(sd, "stage1.concat.", x0)
        for fuse in (True, False):
            with _Mode(mode == "split", fuse), torch.no_grad():
                got = eng.cab("stage1.concat.", Act(_nhwc(x0).to(DEV), V.c0)).t
            e = _close(f"cab_{mode}_fuse{int(fuse)}_{h}x{w}", got.float().cpu().permute(0, 3, 1, 2), ref)
            record(test="cab", id=f"{h}x{w}_fuse{int(fuse)}", mode=mode, route="sn32_cab_ca", shape=[3, V.c0, h, w], max_err_over_scale=e)


def _net_run(name, T, h, w, sd=None, seed=3):
    import importlib
    mod = importlib.import_module(f"basicsr.models.archs.{name}")
    V = O.VARIANTS[name]
    sd = synth_state_dict(name) if sd is None else sd
    blur, _ = synth.blurred_clip(T, h, w, seed=seed)
    x = O.frames_to_tensor(list(blur))
    nm = torch.full((1, T, 1, h, w), 30.0 / 255.0) if V.denoise else None
    net = mod.GShiftNet(future_frames=2, past_frames=2)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    with torch.no_grad():
        out = net(x.to(DEV), nm.to(DEV)) if V.denoise else net(x.to(DEV))
    return net, out, (V, sd, x, nm)


@pytest.mark.parametrize("mode", ["exact", "split"])
@pytest.mark.parametrize("name,h,w", [("gshift_deblur2", 68, 100), ("gshift_denoise1", 40, 56)])
def test_whole_net_fp32_odd_sizes(name, h, w, mode):
    """Odd frame sizes against a live fp32 O.forward at the fp32 file's 1e-4: 68 x 100 (the bf16 odd-size test's shape) and 40 x 56 (the "+"
    model needs multiples of 8), whose second and third levels have h w % 64 != 0 (20 x 28 = 560, 10 x 14 = 140), so sn32_conv1x1_gate2 falls
    back to the unfused chain there."""
    with _Mode(mode == "split"):
        _, out, (V, sd, x, nm) = _net_run(name, 5, h, w)
    ref = O.forward(V, sd, x, nm, 2, 2)
    e = _close(f"net32_{name}_{h}x{w}_{mode}", out, ref)
    record(test="whole_net", id=f"{name}_{h}x{w}", mode=mode, route="-", shape=[5, h, w], max_err_over_scale=e)


@pytest.mark.parametrize("mode", ["exact", "split"])
def test_network_convs_take_tabled_routes(mode, monkeypatch):
    """Every sn32_conv2d the engine issues in the 48 x 64 whole-net runs of all four variants takes an instance that has rows of its own in the
    kernel table (tests/fp32_cases.py) in this arithmetic."""
    from shiftnet_amd import lib as L
    from shiftnet_amd.engine32 import Engine32
    lb = L.load()
    seen = {}
    orig = Engine32._call

    def spy(self, fn, label, *args, **kw):
        if fn == "sn32_conv2d":
            r = lb.sn32_conv2d_route(args[0])
            seen.setdefault(r, label)
        return orig(self, fn, label, *args, **kw)
    monkeypatch.setattr(Engine32, "_call", spy)
    tabled = {c.routes[mode] for c in FC.CASES if mode in c.routes}
    for name in VARIANTS:
        with _Mode(mode == "split"):
            _net_run(name, 7, 48, 64)
    assert seen, "no sn32_conv2d call recorded"
    record(test="route_census", id="48x64_all_variants", mode=mode, route=sorted(FC.route_name(r) for r in seen), shape=[7, 48, 64])
    missing = {FC.route_name(r): lbl for r, lbl in seen.items() if r not in tabled}
    assert not missing, missing
