"""-m gpu: the first and the last launch of a GSTS unit (csrc/sn_gsts.hip) through the C ABI against float64 on the CPU, element by element.

K0: sn_gsts_shiftconv (VALU) and sn_gsts_shiftconv_mfma in every form -- the tile form with the library's workgroup count, one workgroup per XCD
and one per tile, and the walking form at every segment length a row lists (sn_gsts_shiftconv_mfma_opt).  K4: sn_gsts_cab2_phase2 /
sn_cab1_phase2.  tests/test_gpu_parity.py bounds these kernels at max-abs <= 8e-3 of the tensor's peak, which a wrong padding mask on a border
column, a stale ring row on a low-magnitude channel or a clamped pixel leaking into a store can all stay inside; here every row of
tests/gsts_edge_cases.py gets a per-element bound u |ref| + (1 + u) eps M (the cases file states it), outputs live in guarded buffers (NaN
prefill, sentinel margins), frames outside the launch's range must stay NaN, every matrix-core form must be bit-identical to the tile form and the
VALU kernel within one bf16 step of it.  One device-only row per C checks that the production dispatch takes the walking form where the plan
says so and equals the forced tile form bit for bit.  Measured max |err| / tol, |err| / M and the control ratios go to
parity_report_gsts_edges.json in $SN_PARITY_REPORT_DIR (default: parity_out/ at the repository root).
"""
import ctypes
import json
import os

import pytest
import torch

import gsts_edge_cases as GE
from test_gpu_bf16_conv_kernels import bound_check, guarded, guards_intact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPORT = []
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    d = os.environ.get("SN_PARITY_REPORT_DIR") or os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report_gsts_edges.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    from shiftnet_amd import lib as L
    return L.load(), L


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int16)


def unit_src(L, c, x, halo):
    return L.UnitSrc(x.data_ptr(), c.T, c.h, c.w, c.C, c.mode, c.wrap, halo.data_ptr() if halo is not None else None, c.t0, c.nt, c.clip)


def outside_frames_untouched(out, c):
    o = out.float()
    return bool(torch.isnan(o[:c.frames.start]).all()) and bool(torch.isnan(o[c.frames.stop:]).all())


@pytest.mark.parametrize("case", GE.K0_CASES, ids=[c.id for c in GE.K0_CASES])
def test_k0_every_form_against_float64(case, lib):
    lb, L = lib
    c = case
    ops = GE.k0_operands(c)
    ref, tol, m = GE.k0_reference(c, ops)
    x = ops["x"].to(DEV)
    halo = ops["halo"].to(DEV) if ops["halo"] is not None else None
    w1, offs = GE.k0_words(ops["w"]).to(DEV), ops["offs"].to(DEV)
    src = unit_src(L, c, x, halo)
    ntiles = -(-c.h // 16) * -(-c.w // 16) * len(c.frames)
    launches = [("valu", None), ("tile_auto", L.K0Opts(GE.TILE, 0, 0)), ("tile_wgs1", L.K0Opts(GE.TILE, 0, 1)), ("tile_per_tile", L.K0Opts(GE.TILE, 0, ntiles))]
    for S in c.walk:
        launches.append((f"walk_S{S}", L.K0Opts(GE.WALK, S, 0)))
        if c.wgs1:
            launches.append((f"walk_S{S}_wgs1", L.K0Opts(GE.WALK, S, 1)))
    rec = dict(test="k0", id=c.id, shape=[c.T, c.h, c.w, c.C], mode=c.mode, wrap=c.wrap, clip=c.clip, frames=[c.frames.start, c.frames.stop], forms={})
    outs = {}
    for name, opt in launches:
        buf, out = guarded((c.T, c.h, c.w, c.C // 2), torch.bfloat16, NAN)
        if opt is None:
            rc = lb.sn_gsts_shiftconv(ctypes.byref(src), offs.data_ptr(), w1.data_ptr(), out.data_ptr(), stream())
        else:
            rc = lb.sn_gsts_shiftconv_mfma_opt(ctypes.byref(src), offs.data_ptr(), w1.data_ptr(), out.data_ptr(), ctypes.byref(opt), stream())
        assert rc == 0, (c.id, name, rc)
        torch.cuda.synchronize()
        tag = f"{c.id}:{name}"
        assert guards_intact(buf, NAN), f"{tag}: wrote outside its output"
        assert outside_frames_untouched(out, c), f"{tag}: wrote a frame outside [{c.frames.start}, {c.frames.stop})"
        r_tol, r_m = bound_check(tag, out[c.frames.start:c.frames.stop], ref, tol, m)
        rec["forms"][name] = dict(max_err_over_tol=r_tol, max_err_over_M=r_m)
        if opt is not None:
            pl = L.k0_plan(lb, src, torch.cuda.get_device_properties(0).multi_processor_count, opt)
            assert pl["form"] == opt.form and (not opt.seg or pl["S"] == min(opt.seg, pl["nty"])), (tag, pl)
            assert name != "tile_per_tile" or pl["per_tile"] == 1, (tag, pl)      # one workgroup per tile is what ran
            assert not name.endswith("wgs1") or pl["wgs"] == 1, (tag, pl)
            rec["forms"][name]["plan"] = pl
        outs[name] = out[c.frames.start:c.frames.stop]
    tile = outs["tile_auto"]
    for name, o in outs.items():
        if name == "valu":      # the two kernels round the same fp32 sums (up to the order of nine additions) to bf16: at most one bf16 step apart
            d = (o.float() - tile.float()).abs()
            assert (d <= 2.0 ** -7 * tile.float().abs().clamp_min(2.0 ** -10)).all(), (c.id, d.max().item())
        else:
            assert torch.equal(bits(o), bits(tile)), f"{c.id}: {name} is not bit-identical to the tile form"
    # the default entry point is the opt == NULL launch
    buf, out = guarded((c.T, c.h, c.w, c.C // 2), torch.bfloat16, NAN)
    assert lb.sn_gsts_shiftconv_mfma(ctypes.byref(src), offs.data_ptr(), w1.data_ptr(), out.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert guards_intact(buf, NAN) and outside_frames_untouched(out, c) and torch.equal(bits(out[c.frames.start:c.frames.stop]), bits(tile)), c.id
    for ctl in ("no_conv_padding", "tap_dropped"):
        other, _, _ = GE.k0_reference(c, ops, control=ctl)
        rec[f"control_{ctl}"] = ((other - ref).abs() / tol).max().item()
        assert rec[f"control_{ctl}"] >= 8.0, (c.id, ctl)
    REPORT.append(rec)


def test_k0_opt_refusals_launch_nothing(lib):
    lb, L = lib
    c = next(k for k in GE.K0_CASES if k.id == "c64_one_tile_2x16x16")
    assert c.wrap != 2 and c.mode                 # nothing but the options is wrong with this launch
    ops = GE.k0_operands(c)
    x, w1, offs = ops["x"].to(DEV), GE.k0_words(ops["w"]).to(DEV), ops["offs"].to(DEV)
    src = unit_src(L, c, x, None)
    buf, out = guarded((c.T, c.h, c.w, c.C // 2), torch.bfloat16, NAN)
    for opt in (L.K0Opts(3, 0, 0), L.K0Opts(GE.WALK, 9, 0), L.K0Opts(GE.TILE, 2, 0), L.K0Opts(0, 0, -1), L.K0Opts(-1, 0, 0)):
        rc = lb.sn_gsts_shiftconv_mfma_opt(ctypes.byref(src), offs.data_ptr(), w1.data_ptr(), out.data_ptr(), ctypes.byref(opt), stream())
        assert rc == GE.EINVAL, (opt.form, opt.seg, opt.wgs, rc)
    ok = L.K0Opts(0, 0, 0)
    for args in ((None, w1.data_ptr(), out.data_ptr()), (offs.data_ptr(), None, out.data_ptr()), (offs.data_ptr(), w1.data_ptr(), None)):
        assert lb.sn_gsts_shiftconv_mfma_opt(ctypes.byref(src), *args, ctypes.byref(ok), stream()) == GE.EINVAL
    bad = L.UnitSrc(x.data_ptr(), c.T, c.h, c.w, c.C, 0, c.wrap)          # the descriptor's refusals are the plan's: mode 0 has no K0
    assert lb.sn_gsts_shiftconv_mfma_opt(ctypes.byref(bad), offs.data_ptr(), w1.data_ptr(), out.data_ptr(), ctypes.byref(ok), stream()) == GE.EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(buf.float()).all()


@pytest.mark.parametrize("C", [64, 80])
def test_k0_production_dispatch_walks_and_equals_the_tile_form(C, lib):
    """360 x 640 with the smallest T for which the plan, asked with the device's own CU count, walks: the auto launch against the forced tile form"""
    lb, L = lib
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    h, w = 360, 640
    T = next(t for t in range(1, 41) if L.k0_plan(lb, L.UnitSrc(1, t, h, w, C, 1, 0), ncu)["form"] == GE.WALK)
    g = torch.Generator().manual_seed(77 + C)
    gd = torch.Generator(device=DEV).manual_seed(78 + C)          # the operands of this row never reach the CPU: made on the device
    x = torch.randn((T, h, w, C), device=DEV, generator=gd) * torch.exp2(torch.rand((T, h, w, C), device=DEV, generator=gd) * 12.0 - 6.0)
    x = x.to(torch.bfloat16)
    wt = (torch.randn((C // 2, 9), generator=g) / 3.0).float()
    w1, offs = GE.k0_words(wt).to(DEV), GE.k0_operands(GE.K0Case("offs", C, 1, 1, 1, 1, 0, ()))["offs"].to(DEV)
    src = L.UnitSrc(x.data_ptr(), T, h, w, C, 1, GE.VARIANT_WRAP[C])
    plan = L.k0_plan(lb, src, ncu)
    assert plan["form"] == GE.WALK and plan["S"] >= 4, plan
    buf_a, auto = guarded((T, h, w, C // 2), torch.bfloat16, NAN)
    buf_t, tile = guarded((T, h, w, C // 2), torch.bfloat16, NAN)
    assert lb.sn_gsts_shiftconv_mfma(ctypes.byref(src), offs.data_ptr(), w1.data_ptr(), auto.data_ptr(), stream()) == 0
    opt = L.K0Opts(GE.TILE, 0, 0)
    assert lb.sn_gsts_shiftconv_mfma_opt(ctypes.byref(src), offs.data_ptr(), w1.data_ptr(), tile.data_ptr(), ctypes.byref(opt), stream()) == 0
    torch.cuda.synchronize()
    assert guards_intact(buf_a, NAN) and guards_intact(buf_t, NAN)
    assert torch.isfinite(tile.float()).all()
    assert torch.equal(bits(auto), bits(tile))
    REPORT.append(dict(test="k0_dispatch", id=f"c{C}_{T}x{h}x{w}", ncu=ncu, plan=plan))


@pytest.mark.parametrize("case", GE.K4_CASES, ids=[c.id for c in GE.K4_CASES])
def test_k4_against_float64(case, lib):
    lb, L = lib
    c = case
    ops = GE.k4_operands(c)
    ref, tol, m = GE.k4_reference(c, ops)
    pk = GE.k4_packed(ops)
    x, g2, ca = ops["x"].to(DEV), ops["g2"].to(DEV), ops["ca"].to(DEV)
    halo = ops["halo"].to(DEV) if ops["halo"] is not None else None
    wfrag = pk["wfrag"].contiguous().to(DEV)
    bias = pk["bias"].to(DEV) if pk["bias"] is not None else None
    assert (bias is not None) == c.bias
    bptr = bias.data_ptr() if bias is not None else None
    src = unit_src(L, c, x, halo)
    fn, other = (lb.sn_gsts_cab2_phase2, lb.sn_cab1_phase2) if c.mode else (lb.sn_cab1_phase2, lb.sn_gsts_cab2_phase2)
    buf, y = guarded((c.T, c.h, c.w, c.C), torch.bfloat16, NAN)
    # refusals first, nothing written: the other block's entry point, and y == x
    x_before = x.clone()
    assert other(ctypes.byref(src), g2.data_ptr(), ca.data_ptr(), wfrag.data_ptr(), bptr, y.data_ptr(), stream()) == GE.EINVAL
    assert fn(ctypes.byref(src), g2.data_ptr(), ca.data_ptr(), wfrag.data_ptr(), bptr, x.data_ptr(), stream()) == GE.EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(buf.float()).all() and torch.equal(bits(x), bits(x_before)), c.id
    assert fn(ctypes.byref(src), g2.data_ptr(), ca.data_ptr(), wfrag.data_ptr(), bptr, y.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert guards_intact(buf, NAN), f"{c.id}: wrote outside its output"
    assert outside_frames_untouched(y, c), f"{c.id}: wrote a frame outside [{c.frames.start}, {c.frames.stop})"
    r_tol, r_m = bound_check(c.id, y[c.frames.start:c.frames.stop], ref, tol, m)
    rec = dict(test="k4", id=c.id, shape=[c.T, c.h, c.w, c.C], mode=c.mode, wrap=c.wrap, clip=c.clip, frames=[c.frames.start, c.frames.stop],
               bias=c.bias, items=c.items, max_err_over_tol=r_tol, max_err_over_M=r_m)
    ctls = ("no_ca", "unrolled_shortcut") if c.mode else ("no_ca",)
    for ctl in ctls:
        o, _, _ = GE.k4_reference(c, ops, control=ctl)
        rec[f"control_{ctl}"] = ((o - ref).abs() / tol).max().item()
        assert rec[f"control_{ctl}"] >= 8.0, (c.id, ctl)
    REPORT.append(rec)
