"""-m gpu: phase 1 as two kernels -- sn_ln_gemm_gate (K12), then sn_dw5m_gemm_gate (K3m, C = 64) or sn_grp5_gemm_gate (K3g, C = 80), g1 in bf16
through HBM: the chain Engine._recover falls back to -- and sn_nhwc_to_planar, through the C ABI inside the float64 INTERVALS of
tests/chain_cases.py, element by element.

tests/test_gpu_parity.py sees this chain through Engine.naf at 8e-3 .. 1.2e-2 of the tensor's peak on unit-variance noise.  Here every row of the
case tables gets, per element, the interval of a contract that models each rounding of the kernel it belongs to (tests/test_host_chain_ref.py holds
the contracts against the oracle, the packed weights, point emulations and one-fault controls): every g1 / g2 element of the frame range is written
(NaN prefill) and inside, every pool row is inside its interval sum, the planar g1 carries +0 in its pad columns and the same bits as the NHWC one,
frames outside a frame range keep their NaN, sentinels before and after every output are intact, an impulse's g2 is +0 bit for bit outside its
5 x 5 footprint, a persistent workgroup walks across frame boundaries with a ca_in that differs per frame, and the hot rows run at the magnitude the
fallback exists for.  The chain check runs K12 -> sn_ca_mlp -> K3 on the device's own g1, pool and ca1 (Engine._phase1's non-fused branch restated
with raw pointers, bit-identical to a sibling engine with phase1 = "0") and holds K3's output against K3's contract evaluated on those device
tensors.  Per row the share of elements AT an interval end goes to parity_report_chain_edges.json in $SN_PARITY_REPORT_DIR (default: parity_out/).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import chain_cases as CC
from oracle import shiftnet_oracle as O
from test_gpu_bf16_conv_kernels import guarded, guards_intact
from test_gpu_parity import _sibling_engine, act, engines, to_dev      # noqa: F401  (engines: the module fixture of the parity tests)

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
    with open(os.path.join(d, "parity_report_chain_edges.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    from shiftnet_amd import lib as L
    return L.load(), L


def stream():
    return torch.cuda.current_stream().cuda_stream


def dv(t):
    return t.contiguous().to(DEV) if t is not None else None


def bits(t):
    return t.contiguous().view(torch.int16)


def inside(rec, tag, what, got, lo, hi):
    """every element written and inside its interval; the record gets the share at an interval end, or the worst element"""
    got = got.double().cpu().numpy()
    assert got.shape == lo.shape, (rec["id"], tag, what, got.shape, lo.shape)
    out = CC.outside(got, lo, hi)
    r = rec.setdefault(tag, {})
    r[what] = dict(at_an_end=float(((got == lo) | (got == hi)).mean()), zero_width=float((lo == hi).mean()), outside=int(out.sum()), elements=int(out.size),
                   unwritten=int(np.isnan(got).sum()))
    if out.any():
        peak = max(np.abs(lo).max(), np.abs(hi).max(), 1e-300)
        ex = np.where(out, np.maximum(lo - got, got - hi), 0.0)
        ex[np.isnan(got)] = np.inf
        i = np.unravel_index(int(np.argmax(ex)), ex.shape)
        r[what]["worst"] = dict(index=[int(k) for k in i], got=float(got[i]), lo=float(lo[i]), hi=float(hi[i]), excess_over_peak=float(ex[i] / peak))
        REPORT.append(dict(rec))
        raise AssertionError(f"{rec['id']}:{tag}: {int(out.sum())} of {out.size} {what} elements outside their interval ({int(np.isnan(got).sum())} not written); "
                             f"worst {r[what]['worst']['index']}: got {got[i]:.9g}, interval [{lo[i]:.9g}, {hi[i]:.9g}]")


def untouched(c, tag, fr, *views):
    for v in views:
        if v is not None:
            assert bool(torch.isnan(v[:fr.start].float()).all()) and bool(torch.isnan(v[fr.stop:].float()).all()), f"{c.id}:{tag}: wrote a frame outside [{fr.start}, {fr.stop})"


# ---- K12 ------------------------------------------------------------------------------------------------------------------------------------

def k12_launch(lb, L, c, d, pk, layout, pool, tag):
    """-> (g1 as NHWC view, the planar view or None, pool view or None): guarded NaN buffers, guards and the frames outside the range checked"""
    wr = CC.planar_pitch(c.w)
    gb, gv = guarded((c.T, c.h, c.C, wr) if layout == 2 else (c.T, c.h, c.w, c.C), torch.bfloat16, NAN)
    nblk = lb.sn_lngate_blocks(c.h, c.w)
    pb, pv = guarded((c.T, nblk, c.C), torch.float32, NAN) if pool else (None, None)
    src = L.UnitSrc(d["x"].data_ptr(), c.T, c.h, c.w, c.C, c.mode, c.wrap, d["halo"].data_ptr() if d["halo"] is not None else None, c.t0, c.nt, c.clip)
    rc = lb.sn_ln_gemm_gate(ctypes.byref(src), d["hw"].data_ptr() if d["hw"] is not None else None, pk["w_ln"].data_ptr(), pk["b_ln"].data_ptr(),
                            pk["w_dw3_h2"].data_ptr(), gv.data_ptr(), pv.data_ptr() if pool else None, layout, stream())
    assert rc == 0, (c.id, tag, rc)
    torch.cuda.synchronize()
    assert guards_intact(gb, NAN) and (pb is None or guards_intact(pb, NAN)), f"{c.id}:{tag}: wrote outside its output"
    fr = slice(c.frames.start, c.frames.stop)
    untouched(c, tag, fr, gv, pv)
    if layout == 2:
        pad = gv[fr][..., c.w:]
        assert pad.numel() == 0 or not bool(bits(pad).any()), f"{c.id}:{tag}: planar pad columns are not +0"
        return gv[..., :c.w].permute(0, 1, 3, 2), gv, pv
    return gv, None, pv


def k3_launch(lb, c, T, g1_dev, ca_dev, pk, pool, tag):
    """K3m on a planar g1 (C = 64) or K3g on an NHWC one -> (g2 view, pool view or None)"""
    fn, wk, nblk = (lb.sn_dw5m_gemm_gate, "w_toep5", lb.sn_dw5m_blocks(c.h, c.w)) if c.C == 64 else (lb.sn_grp5_gemm_gate, "w_grp", lb.sn_grp5_blocks(c.h, c.w))
    gb, gv = guarded((T, c.h, c.w, c.C), torch.bfloat16, NAN)
    pb, pv = guarded((T, nblk, c.C), torch.float32, NAN) if pool else (None, None)
    rc = fn(g1_dev.data_ptr(), ca_dev.data_ptr() if ca_dev is not None else None, pk[wk].data_ptr(), pk["w_gate"].data_ptr(), gv.data_ptr(),
            pv.data_ptr() if pool else None, T, c.h, c.w, c.C, stream())
    assert rc == 0, (c.id, tag, rc)
    torch.cuda.synchronize()
    assert guards_intact(gb, NAN) and (pb is None or guards_intact(pb, NAN)), f"{c.id}:{tag}: wrote outside its output"
    return gv, pv


@pytest.mark.parametrize("case", CC.K12_CASES, ids=[c.id for c in CC.K12_CASES])
def test_k12_inside_the_intervals(case, lib):
    lb, L = lib
    c = case
    ops = CC.k12_operands(c)
    ref = CC.k12_reference(c, ops)
    fr = slice(c.frames.start, c.frames.stop)
    rec = dict(test="k12", id=c.id, shape=[c.T, c.h, c.w, c.C], mode=c.mode, wrap=c.wrap, clip=c.clip, frames=[fr.start, fr.stop], family=c.family,
               widths=CC.width_stats(*ref["g1"]))
    d = {k: dv(ops[k]) for k in ("x", "halo", "hw")}
    pk = {k: dv(v) for k, v in CC.packed(ops).items()}
    first = None
    for layout in c.layouts:
        tag = f"layout{layout}"
        g1, planar, pool = k12_launch(lb, L, c, d, pk, layout, c.pool, tag)
        inside(rec, tag, "g1", g1[fr], *ref["g1"])
        if c.pool:
            inside(rec, tag, "pool", pool[fr], *ref["pool"])
            g1n, _, _ = k12_launch(lb, L, c, d, pk, layout, False, tag + "_no_pool")      # pool == NULL is accepted and changes nothing
            assert torch.equal(bits(g1n[fr]), bits(g1[fr])), (c.id, tag, "pool changes g1")
        if first is None:
            first = (g1, pool)
        else:
            assert torch.equal(bits(g1[fr]), bits(first[0][fr])), (c.id, "the two layouts differ")
            assert not c.pool or torch.equal(pool[fr], first[1][fr]), (c.id, "the pool rows of the two layouts differ")
    if c.family == "hot":                   # K12, then K3 on the device's g1, at the magnitude the fallback exists for
        g1c = first[0][fr].contiguous()
        assert bool(torch.isfinite(g1c.float()).all())
        ca = CC._scale(torch.Generator().manual_seed(c.seed + 3), len(c.frames), c.C)
        k3 = CC.k3_reference(c.C, g1c.cpu(), ca, ops)
        g1k = dv(CC.planar(g1c.cpu())) if c.C == 64 else g1c
        g2, pool2 = k3_launch(lb, c, len(c.frames), g1k, dv(ca), pk, True, "hot_k3")
        assert bool(torch.isfinite(g2.float()).all()) and bool(torch.isfinite(pool2).all())
        inside(rec, "hot_k3", "g2", g2, *k3["g2"])
        inside(rec, "hot_k3", "pool", pool2, *k3["pool"])
        rec["hot_k3"]["peak_g1"] = float(g1c.float().abs().max())
    REPORT.append(rec)


# ---- K3m / K3g ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CC.K3_CASES, ids=[c.id for c in CC.K3_CASES])
def test_k3_inside_the_intervals(case, lib):
    lb, _ = lib
    c = case
    rec = dict(test="k3", id=c.id, family=c.family)
    if c.walk:                              # tiles > CUs on THIS device: rebuilt, never skipped
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        T = CC.walk_frames(c, ncu)
        if T != c.T:
            c = c.with_frames(T)
        wgs = CC.walk(c.T * c.tiles_per_frame, min(c.T * c.tiles_per_frame, ncu))
        tpf = c.tiles_per_frame
        rec["walk"] = dict(ncu=ncu, frames=c.T, tiles=c.T * tpf, two_tiles=sum(len(w) >= 2 for w in wgs), starts_past_its_end=sum(not w for w in wgs),
                           frame_crossings=sum(a // tpf != b // tpf for w in wgs for a, b in zip(w, w[1:])))
        assert rec["walk"]["two_tiles"] > 0 and rec["walk"]["frame_crossings"] > 0, rec["walk"]
    rec["shape"] = [c.T, c.h, c.w, c.C]
    ops = CC.k3_operands(c)
    pk = {k: dv(v) for k, v in CC.packed(ops).items()}
    g1_dev = dv(CC.planar(ops["g1"])) if c.C == 64 else dv(ops["g1"])
    ca_dev = dv(ops["ca"])
    for scaled in (True, False):
        ref = CC.k3_reference(c.C, ops["g1"], ops["ca"] if scaled else None, ops)
        tag = "ca" if scaled else "no_ca"
        rec.setdefault("widths", {})[tag] = CC.width_stats(*ref["g2"])
        g2, pool = k3_launch(lb, c, c.T, g1_dev, ca_dev if scaled else None, pk, True, tag)
        inside(rec, tag, "g2", g2, *ref["g2"])
        inside(rec, tag, "pool", pool, *ref["pool"])
        g2n, _ = k3_launch(lb, c, c.T, g1_dev, ca_dev if scaled else None, pk, False, tag + "_no_pool")      # pool == NULL is accepted and changes nothing
        assert torch.equal(bits(g2n), bits(g2)), (c.id, tag, "pool changes g2")
        if c.family == "impulse":
            away = torch.from_numpy(~CC.footprint(c, ops["impulse"])).to(DEV)
            assert not bool(bits(g2)[away].any()), f"{c.id}:{tag}: g2 is not +0 bit for bit outside an impulse's 5 x 5 footprint"
    REPORT.append(rec)


# ---- the chain on the device's own tensors --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_denoise2", "gshift_deblur1", "gshift_denoise1"])
def test_chain_on_the_devices_own_tensors(name, engines, lib):
    """K12 (pool on for the denoisers) -> sn_ca_mlp -> K3 with raw pointers on 2 x 17 x 70: the same bits as Engine.naf of a sibling engine with
    phase1 = "0" leaves in its buffers, K12's g1 and pool rows inside K12's contract on the device's x and hw, K3's g2 and pool rows inside K3's
    contract evaluated on the device's own g1 and ca1"""
    from shiftnet_amd import synth
    lb, L = lib
    eng, sd = engines(name)
    chain = _sibling_engine(eng, phase1="0")
    V = O.VARIANTS[name]
    C, (T, h, w), mode = V.c1, CC.CHAIN_SHAPE, 1
    assert not chain._fused_phase1(T)
    x = torch.from_numpy(synth.unit_noise((T, C, h, w), seed=87)).to(torch.bfloat16).float()
    xa = act(to_dev(x), C)
    pre = "stage1.decoder_level1.encoder_level1.0."
    B = chain.naf_buffers(T, h, w, C, mode)
    chain.naf(pre, xa, mode, bufs=B)
    torch.cuda.synchronize()
    u, r = chain.P.units[pre], chain.route(T, C)
    assert not r.fused and r.mstencil == (C == 64)
    src = chain._unit_src(xa, mode)
    rec = dict(test="chain", id=name, shape=[T, h, w, C], denoise=bool(V.denoise))
    wr = CC.planar_pitch(w)
    gb, g1 = guarded((T, h, C, wr) if r.mstencil else (T, h, w, C), torch.bfloat16, NAN)
    p1b, pool1 = guarded((T, lb.sn_lngate_blocks(h, w), C), torch.float32, NAN) if V.denoise else (None, None)
    assert lb.sn_ln_gemm_gate(ctypes.byref(src), B["hwb"].data_ptr(), u["w_ln"].data_ptr(), u["b_ln"].data_ptr(), u["w_dw3_h2"].data_ptr(), g1.data_ptr(),
                              pool1.data_ptr() if V.denoise else None, 2 if r.mstencil else 0, stream()) == 0
    ca1 = None
    if V.denoise:
        q = chain.P.cas[pre + "ca1"]
        cb, ca1 = guarded((T, C), torch.float32, NAN)
        assert lb.sn_ca_mlp(pool1.data_ptr(), pool1.shape[1], C, q["c"], q["cr"], 1.0 / (h * w), q["wa"].data_ptr(), q["wb"].data_ptr(), ca1.data_ptr(), T, None, stream()) == 0
    pku = {"w_toep5": u.get("w_toep5"), "w_grp": u.get("w_grp"), "w_gate": u["w_gate"]}
    kc = CC.K3Case("chain_" + name, C, T, h, w)
    g2, pool2 = k3_launch(lb, kc, T, g1, ca1, pku, True, "k3")
    assert guards_intact(gb, NAN) and (p1b is None or guards_intact(p1b, NAN)) and (ca1 is None or guards_intact(cb, NAN))
    assert torch.equal(bits(g1), bits(B["g1"])) and torch.equal(bits(g2), bits(B["g2"])) and torch.equal(pool2, B["pool2"]), (name, "Engine.naf's chain differs")
    if V.denoise:
        assert torch.equal(pool1, B["pool1"]) and torch.equal(ca1, B["ca1"])
    g1n = g1[..., :w].permute(0, 1, 3, 2).contiguous() if r.mstencil else g1
    assert not r.mstencil or not bool(bits(g1[..., w:]).any())
    i = 4 if V.denoise else 3
    ops = {"x": xa.t.cpu(), "halo": None, "hw": B["hwb"].cpu(), "w1": sd[pre + "body.0.weight"], "ln_w": sd[pre + "norm.weight"], "ln_b": sd[pre + "norm.bias"],
           "w_dw3": sd[pre + "body.1.conv_2.weight"], "w_rep5": sd[f"{pre}body.{i}.conv_1.weight"], "w_rep3": sd[f"{pre}body.{i}.conv_2.weight"],
           "w2": sd[f"{pre}body.{i + 1}.weight"]}
    k12 = CC.K12Case("chain_" + name, C, T, h, w, mode, src.wrap, pool=bool(V.denoise))
    ref1 = CC.k12_reference(k12, ops)
    inside(rec, "k12", "g1", g1n, *ref1["g1"])
    if V.denoise:
        inside(rec, "k12", "pool", pool1, *ref1["pool"])
    ref = CC.k3_reference(C, g1n.cpu(), ca1.cpu() if ca1 is not None else None, ops)
    inside(rec, "k3", "g2", g2, *ref["g2"])
    inside(rec, "k3", "pool", pool2, *ref["pool"])
    REPORT.append(rec)


# ---- sn_nhwc_to_planar ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", CC.PLANAR_C)
def test_nhwc_to_planar_bit_for_bit(C, lib):
    lb, _ = lib
    T, h = 2, 3
    g = torch.Generator().manual_seed(400 + C)
    for w in CC.PLANAR_W:
        x = CC.GE._act(g, (T, h, w, C))
        xb, xp = guarded((T, h, C, CC.planar_pitch(w)), torch.bfloat16, NAN)
        assert lb.sn_nhwc_to_planar(dv(x).data_ptr(), xp.data_ptr(), T, h, w, C, stream()) == 0
        torch.cuda.synchronize()
        assert guards_intact(xb, NAN), (C, w)
        assert torch.equal(bits(xp.cpu()), bits(CC.planar(x))), (C, w)
