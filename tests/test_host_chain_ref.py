"""CPU checks behind tests/test_gpu_chain_edges.py: the interval contracts of tests/chain_cases.py (K12 sn_ln_gemm_gate, K3m sn_dw5m_gemm_gate,
K3g sn_grp5_gemm_gate) on their own.  With every rounding off and the weights folded in float64, K12 -> K3 is the oracle's chain; the folded
matrices are bit for bit what the packers of Plan.add_naf pack; the kernels' data flow as tests/emu.py addresses the packed operands agrees with
the contract run on the same rounded weights; point emulations (accumulations moved by up to their whole term, fp16 subnormals kept or flushed)
stay inside every interval and every pool row; point emulations with exactly ONE fault each leave them on the row named for the fault; the
intervals are narrow; the hot gains are what the table says; the persistent walk of K3m / K3g visits every tile once; every SN_EINVAL of the four
entry points comes back before a launch.  Width statistics and control counts go to parity_report_chain_ref.json in $SN_PARITY_REPORT_DIR
(default: parity_out/ at the repository root); DESIGN.md section 3.27 quotes them.

tests/emu.py rounds nothing (its header says so), and 82 .. 98 % of the g1 intervals have zero width: an un-rounded fp32 emulation cannot be
INSIDE them.  What it can prove -- that the packed operands, decoded the way the kernels address them, are the contract's natural-order matrices
-- it proves against the contract's "exact" run on the rounded weights, to the fp32 accumulation bound.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import chain_cases as CC
import emu
import phase1_cases as PC
from oracle import shiftnet_oracle as O
from shiftnet_amd import lib as L
from shiftnet_amd import prep

D = torch.float64
REPORT = []
WIDTH_CAP = {64: 3e-3, 80: 6e-3}            # the limits the fused reference is held to (tests/test_host_phase1_ref.py)
Arith = CC.Arith


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    d = os.environ.get("SN_PARITY_REPORT_DIR") or os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report_chain_ref.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    return L.load()


_K12, _K3 = {}, {}


def k12_ref(c):
    if c.id not in _K12:
        ops = CC.k12_operands(c)
        _K12[c.id] = (ops, CC.k12_reference(c, ops))
    return _K12[c.id]


def k3_ref(c, scaled=True):
    key = (c.id, scaled)
    if key not in _K3:
        ops = CC.k3_operands(c)
        _K3[key] = (ops, CC.k3_reference(c.C, ops["g1"], ops["ca"] if scaled else None, ops))
    return _K3[key]


# ---- the contracts without roundings are the oracle's chain ---------------------------------------------------------------------------------

ORACLE_ROWS = [c for c in CC.K12_CASES if c.oracle]


@pytest.mark.parametrize("scaled", [False, True], ids=["deblur", "denoise"])
@pytest.mark.parametrize("case", ORACLE_ROWS, ids=[c.id for c in ORACLE_ROWS])
def test_contracts_without_roundings_are_the_oracle_chain(case, scaled):
    """K12's contract, then K3's on its g1 (scaled: times a per-frame scale in between, the denoisers' ca1), every rounding and widening off,
    weights folded in float64, against O.layer_norm_2d -> O._conv -> dw3x3 + id -> gate [-> ca1] -> O._rep_conv -> O._conv -> gate2: 1e-10"""
    c = case
    C = c.C
    ops = CC.k12_operands(c)
    ar = Arith("exact")
    g1 = CC.k12_reference(c, ops, ar, want=("g1",))["g1"]
    assert np.array_equal(g1[0], g1[1])
    ca = CC._scale(torch.Generator().manual_seed(c.seed + 3), c.T, C) if scaled else None
    got = CC.k3_reference(C, torch.from_numpy(g1[0]), ca, ops, ar, want=("v",))["v"][0]
    sd = {"norm.weight": ops["ln_w"].to(D), "norm.bias": ops["ln_b"].to(D), "body.0.weight": ops["w1"].to(D), "body.1.conv_2.weight": ops["w_dw3"].to(D),
          "body.3.conv_1.weight": ops["w_rep5"].to(D), "body.3.conv_2.weight": ops["w_rep3"].to(D), "body.4.weight": ops["w2"].to(D)}
    x = ops["x"].to(D).permute(0, 3, 1, 2).contiguous()
    if c.mode:
        u = O.gsts_gather(x, c.mode == 2, bool(c.wrap))[:, :C]
        u = torch.cat((u, ops["hw"].to(D).permute(0, 3, 1, 2)), 1)
    else:
        u = x
    a = O._conv(sd, "body.0.", O.layer_norm_2d(u, sd["norm.weight"], sd["norm.bias"]))
    a = O._conv(sd, "body.1.conv_2.", a, groups=a.shape[1]) + a
    a1, a2 = a.chunk(2, dim=1)
    g = a1 * a2
    assert np.abs(g1[0] - g.permute(0, 2, 3, 1).numpy()).max() <= 1e-10 * max(1.0, float(g.abs().max()))
    if scaled:
        g = g * ca.to(D)[:, :, None, None]
    b1, b2 = O._conv(sd, "body.4.", O._rep_conv(sd, "body.3.", g, groups=C // 8 if C == 80 else C)).chunk(2, dim=1)
    want = (b1 * torch.sigmoid(b2)).permute(0, 2, 3, 1).numpy()
    assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())


def _unfrag(f):
    return f.reshape(f.shape[0], f.shape[1], 4, 16, 8).transpose(0, 3, 1, 2, 4).reshape(16 * f.shape[0], 32 * f.shape[1])


@pytest.mark.parametrize("C", [64, 80])
@pytest.mark.parametrize("mode", [0, 1])
def test_folded_matrices_are_what_the_packers_pack(C, mode):
    """w_ln / b_ln, w_dw3_h2, w_toep5 / w_grp and w_gate unpacked as the kernels address them against chain_cases.folded, bit for bit; the
    slots a kernel multiplies by padding are zero"""
    c = CC.K12Case("pack", C, 1, 2, 2, mode, 0, seed=77 + C + mode)
    ops = CC.k12_operands(c)
    fw, pk = CC.folded(ops), CC.packed(ops)
    K, mt = c.K, C // 8
    rg, pg = prep.rows_gate(C), prep.pos_gate(C)
    w1 = _unfrag(emu.frag_to_np(pk["w_ln"]).astype(np.float64))
    assert w1.shape == (2 * C, 32 * ((K + 31) // 32)) and np.array_equal(w1[rg][:, :K], fw["W1"]) and not w1[:, K:].any()
    assert np.array_equal(pk["b_ln"].numpy().astype(np.float64)[pg], fw["b"])
    words = pk["w_dw3_h2"].numpy().view(np.uint32)                              # [9][C] words: positions (2k, 2k + 1)
    assert words.shape == (9, C)
    d3p = np.zeros((9, 2 * C))
    d3p[:, 0::2], d3p[:, 1::2] = emu._h2(words)
    assert np.array_equal(d3p[:, pg].T, fw["d3"])
    # the kernel's own addressing of the gate pair: lane slot gs, chunk q, word k -> positions gs 4 mt + q 8 + 2k (+1): channel pairs (c, C + c)
    for gs in range(4):
        for q in range(mt // 2):
            for k in range(4):
                pos = gs * 4 * mt + q * 8 + 2 * k
                ch = [int(np.where(pg == pos + i)[0][0]) for i in range(2)]
                assert (ch[0] < C) == (k < 2) and ch[1] == ch[0] + 1
    w2 = _unfrag(emu.frag_to_np(pk["w_gate"]).astype(np.float64))
    assert np.array_equal(w2[rg][:, :C], fw["W2"]) and not w2[:, C:].any()
    if C == 64:
        tab = pk["w_toep5"].to(torch.float64).numpy()                           # [C][5][2][20]
        assert np.array_equal(tab[:, :, 0, 7:12], fw["k5"]) and np.array_equal(tab[:, :, 1, 6:11], fw["k5"])
        assert not tab[:, :, 0, :7].any() and not tab[:, :, 0, 12:].any() and not tab[:, :, 1, :6].any() and not tab[:, :, 1, 11:].any()
    else:
        wg = _unfrag(emu.frag_to_np(pk["w_grp"]).astype(np.float64))            # [C][13 * 32]
        want = np.zeros_like(wg)
        for o in range(C):
            for s in range(13):
                for g in range(4):
                    tap = 2 * s + (g >> 1)
                    if tap < 25 and (g & 1) == ((o % 16) >> 3):
                        want[o, s * 32 + g * 8: s * 32 + g * 8 + 8] = fw["dg"][o // 8, o % 8, :, tap // 5, tap % 5]
        assert np.array_equal(wg, want)


EMU_ROWS = [c for c in CC.K12_CASES if c.id.endswith(("one_pixel_1x1x1_m0", "small_2x5x9_m1"))]


def _emu_grp5(g1, wgrp):
    """K3g's grouped conv as grp5p_gemm_gate_kernel addresses it, through emu.mfma_tiles: k-step s, lane group g -> tap 2 s + (g >> 1), input
    channels 16 m + 8 (g & 1) ..; D register r of lane (g, p) -> output channel 16 m + 4 g + r of pixel p.  g1 [h][w][C] -> r [h][w][C], fp32"""
    h, w, C = g1.shape
    wf = emu.frag_to_np(wgrp)
    gp = np.zeros((h + 4, w + 4, C), np.float32)
    gp[2:-2, 2:-2] = g1
    px = [(y, x) for y in range(h) for x in range(w)]
    r = np.zeros((h, w, C), np.float32)
    for i0 in range(0, len(px), 16):
        for m in range(C // 16):
            b = np.zeros((13, 64, 8), np.float32)
            for lane in range(64):
                g, p = lane >> 4, lane & 15
                y, x = px[min(i0 + p, len(px) - 1)]
                for s in range(13):
                    tap = 2 * s + (g >> 1)
                    tap = tap if tap < 25 else 0
                    b[s, lane] = gp[y + tap // 5, x + tap % 5, 16 * m + 8 * (g & 1): 16 * m + 8 * (g & 1) + 8]
            regs = emu.mfma_tiles(wf[m:m + 1], b)[0]
            for lane in range(64):
                g, p = lane >> 4, lane & 15
                if i0 + p < len(px):
                    y, x = px[i0 + p]
                    r[y, x, 16 * m + 4 * g: 16 * m + 4 * g + 4] = regs[lane]
    return r


@pytest.mark.parametrize("case", EMU_ROWS, ids=[c.id for c in EMU_ROWS])
def test_emulated_data_flow_is_the_contract(case):
    """emu.ln_gemm -> emu.dw_gate -> emu.dw5m_gemm_gate (C = 64) or the grouped path through emu.mfma_tiles (C = 80) on the PACKED operands
    against the contract run "exact" on the same rounded weights.  Both round no activation; the emulation accumulates in fp32: per stage
    (terms + 8) 2^-24 M, through three GEMMs and the stencils: 1e-4 of the tensor's peak holds with two decades to spare (a misplaced row,
    tap or channel is an error of order one)."""
    c = case
    C = c.C
    ops = CC.k12_operands(c)
    pk, fw = CC.packed(ops), CC.folded(ops)
    ar = Arith("exact")
    ref = CC.k12_reference(c, ops, ar, fw=fw, want=("g1",))["g1"][0]
    ca = CC._scale(torch.Generator().manual_seed(c.seed + 3), c.T, C)
    ref2 = CC.k3_reference(C, torch.from_numpy(ref), ca, ops, ar, fw=fw, want=("v",))["v"][0]
    x = ops["x"].float().numpy()
    hwb = ops["hw"].float().numpy() if c.mode else None
    a = emu.ln_gemm(x, hwb, pk["w_ln"], pk["b_ln"].numpy(), c.mode, bool(c.wrap))
    d3p = np.zeros((9, 2 * C), np.float32)
    d3p[:, 0::2], d3p[:, 1::2] = emu._h2(pk["w_dw3_h2"].numpy().view(np.uint32))
    g1 = emu.dw_gate(a, d3p)
    assert np.abs(g1 - ref).max() <= 1e-4 * np.abs(ref).max()
    if C == 64:
        g2, _ = emu.dw5m_gemm_gate(ref.astype(np.float32), pk["w_toep5"], pk["w_gate"], ca.numpy())
    else:
        r = np.stack([_emu_grp5((ref[t] * ca[t].double().numpy()).astype(np.float32), pk["w_grp"]) for t in range(c.T)])
        w2 = _unfrag(emu.frag_to_np(pk["w_gate"]))[prep.rows_gate(C)][:, :C]
        b = r @ w2.T
        g2 = b[..., :C] / (1.0 + np.exp(-b[..., C:]))
    assert np.abs(g2 - ref2).max() <= 1e-4 * max(np.abs(ref2).max(), 1e-30)


# ---- containment ----------------------------------------------------------------------------------------------------------------------------

RUNS = [(1.0, False, 0), (-1.0, True, 0), (None, False, 1), (None, True, 2), (None, False, 3)]


@pytest.mark.parametrize("case", CC.K12_CASES, ids=[c.id for c in CC.K12_CASES])
def test_k12_point_emulations_stay_inside(case):
    """K12's arithmetic as a point emulation -- LayerNorm in float32 in the kernel's order, every rounding, the matrix-core accumulation moved by a
    share of its term (+1, -1, random per element), fp16 subnormals kept or flushed -- is inside every g1 interval and every pool row"""
    c = case
    ops, ref = k12_ref(c)
    for share, flush, seed in RUNS:
        ar = Arith("point", np.random.default_rng(seed), share, flush)
        pt = CC.k12_reference(c, ops, ar)
        out = CC.outside(pt["g1"][0], *ref["g1"])
        assert not out.any(), (c.id, share, flush, seed, int(out.sum()), np.argwhere(out)[0].tolist())
        if c.pool:
            assert not CC.outside(pt["pool"][0], *ref["pool"]).any(), (c.id, share, flush, seed)


@pytest.mark.parametrize("scaled", [False, True], ids=["no_ca", "ca"])
@pytest.mark.parametrize("case", CC.K3_CASES, ids=[c.id for c in CC.K3_CASES])
def test_k3_point_emulations_stay_inside(case, scaled):
    """the same for K3m / K3g from their stored g1, with and without ca_in (a walk row's 3 M elements: one random run over all frames, the other
    four over its first three)"""
    c = case
    ops, ref = k3_ref(c, scaled)
    for share, flush, seed in RUNS:
        n = 3 if c.walk and seed != 1 else c.T
        ar = Arith("point", np.random.default_rng(seed), share, flush)
        pt = CC.k3_reference(c.C, ops["g1"][:n], ops["ca"][:n] if scaled else None, ops, ar)
        out = CC.outside(pt["g2"][0], ref["g2"][0][:n], ref["g2"][1][:n])
        assert not out.any(), (c.id, share, flush, seed, int(out.sum()), np.argwhere(out)[0].tolist())
        assert not CC.outside(pt["pool"][0], ref["pool"][0][:n], ref["pool"][1][:n]).any(), (c.id, share, flush, seed)
    if c.family == "impulse":                                                   # outside the footprint the contract itself says 0, of zero width
        away = ~CC.footprint(c, ops["impulse"])
        assert not ref["g2"][0][away].any() and not ref["g2"][1][away].any()


# ---- controls: one fault each ---------------------------------------------------------------------------------------------------------------

def _check(rec, C, name, out, reach=None, at=None):
    """out [n][h][w][C] (or rows): reach [h][w] where the fault can show (None: everywhere), at: where it must (default: reach)"""
    if reach is None:
        n_at = int(out.sum())
    else:
        must = reach if at is None else at
        n_at = int(out[:, must].sum())
        assert not out[:, ~reach].any(), (C, name, "outside where the fault cannot reach")
    assert n_at > 0, (C, name, "not detected")
    rec["outside"][name] = dict(total=int(out.sum()), where_it_must=n_at, elements=int(out.size))


@pytest.mark.parametrize("C", [64, 80])
def test_every_k12_control_leaves_the_intervals(C):
    """point emulations (accumulation shares random) with exactly one fault each, on 2 x 17 x 70 (mode 2, pool on); g1 in fp16 on the hot row"""
    c = CC.K12_BY_ID[f"c{C}_3x3_tiles_2x17x70_m2"]
    ops, ref = k12_ref(c)
    lo, hi = ref["g1"]
    cls = ops["cls"].numpy()
    h, w = c.h, c.w
    yy, xx = np.mgrid[0:h, 0:w]
    rec = dict(test="k12_controls", id=c.id, elements=int(lo.size), outside={})
    run = lambda fault: CC.outside(CC.k12_reference(c, ops, Arith("point", np.random.default_rng(11)), fault=fault)["g1"][0], lo, hi)      # noqa: E731
    border = (yy < 1) | (yy >= h - 1) | (xx < 1) | (xx >= w - 1)
    _check(rec, C, "bias_outside", run("bias_outside"), border)
    everywhere = np.ones((h, w), bool)
    _check(rec, C, "no_eps", run("no_eps"), everywhere, at=cls == 2)
    if C == 80:
        _check(rec, C, "mean_ks", run("mean_ks"))
    for name in ("taps_transposed", "no_identity", "gate_partner", "same_frame"):
        _check(rec, C, name, run(name))
    ar = Arith("point", np.random.default_rng(11))
    pt = CC.k12_reference(c, ops, ar)
    assert not CC.outside(pt["pool"][0], *ref["pool"]).any()
    out = CC.outside(CC.k12_pool_rows(ar, pt["p"], h, w, edge=True)[0], *ref["pool"])
    ntx = -(-w // CC.K12_TW)
    partial = np.array([(4 * (b // 4 // ntx * 2) + 2 * (b % 4) + 2 > h) or ((b // 4) % ntx == ntx - 1 and w % CC.K12_TW) for b in range(out.shape[1])], bool)
    assert out[:, partial].sum() > 0 and not out[:, ~partial].any(), (C, "pool_counts_outside")
    rec["outside"]["pool_counts_outside"] = dict(total=int(out.sum()), where_it_must=int(out[:, partial].sum()), elements=int(out[:, partial].size))
    ch = CC.K12_BY_ID[f"c{C}_hot_2x9x33_m1"]
    oph, refh = k12_ref(ch)
    with np.errstate(over="ignore", invalid="ignore"):
        bad = CC.k12_reference(ch, oph, Arith("point", np.random.default_rng(11)), fault="g1_fp16")["g1"][0]
    _check(rec, C, "g1_fp16_on_the_hot_row", CC.outside(bad, *refh["g1"]))
    REPORT.append(rec)


@pytest.mark.parametrize("C", [64, 80])
def test_every_k3_control_leaves_the_intervals(C):
    """the same for K3m (C = 64) / K3g (C = 80): the dense 3 x 3 tiles row, the impulse row for the seams, w = 70 for the planar pad column, the
    walk row for the scale of the next frame"""
    th, tw = CC.K3_TILE[C]
    c = CC.K3_BY_ID["c64_3x3_tiles_2x17x130" if C == 64 else "c80_3x3_tiles_2x9x70"]
    ops, ref = k3_ref(c)
    lo, hi = ref["g2"]
    fw = CC.folded(ops)
    rec = dict(test="k3_controls", id=c.id, elements=int(lo.size), outside={})
    pt_ar = lambda: Arith("point", np.random.default_rng(11))      # noqa: E731
    run = lambda fault, f=None: CC.outside(CC.k3_reference(C, ops["g1"], ops["ca"], ops, pt_ar(), fw=f or fw, fault=fault)["g2"][0], lo, hi)      # noqa: E731
    _check(rec, C, "k5_transposed", run("k5_transposed"))
    off = CC.folded({k: (v if k != "w_rep3" else torch.zeros_like(v)) for k, v in ops.items() if k.startswith("w")})      # the 3x3 folded one tap to the left
    key = "k5" if C == 64 else "dg"
    a3 = ops["w_rep3"].double().numpy()
    mis = off[key].copy()
    if C == 64:
        mis[:, 1:4, 0:3] += a3[:, 0]
    else:
        mis.reshape(C, 8, 5, 5)[:, :, 1:4, 0:3] += a3
    off[key] = CC._tb(mis)
    _check(rec, C, "k3_one_tap_off", run("k3_one_tap_off", off))
    _check(rec, C, "gate_swapped", run("gate_swapped"))
    if C == 80:
        out = run("scale_after")
        rec["outside"]["scale_after"] = dict(total=int(out.sum()), elements=int(out.size), note="reported, not asserted: the two orders differ by one bf16 rounding of the operand")
    # the pool: a row that counts its tile's outside pixels; a row written at rem + 1
    ar = pt_ar()
    pt = CC.k3_reference(C, ops["g1"], ops["ca"], ops, ar, fw=fw)
    assert not CC.outside(pt["pool"][0], *ref["pool"]).any()
    ntx = -(-c.w // tw)
    nrows = ref["pool"][0].shape[1]
    partial = np.array([(b // ntx == nrows // ntx - 1 and c.h % th) or (b % ntx == ntx - 1 and c.w % tw) for b in range(nrows)], bool)
    out = CC.outside(CC.k3_pool_rows(ar, C, pt["v"], c.h, c.w, edge=True)[0], *ref["pool"])
    assert out[:, partial].sum() > 0 and not out[:, ~partial].any(), (C, "pool_counts_outside")
    rec["outside"]["pool_counts_outside"] = dict(total=int(out.sum()), where_it_must=int(out[:, partial].sum()), elements=int(out[:, partial].size))
    out = CC.outside(CC.k3_pool_rows(ar, C, pt["v"], c.h, c.w, shift=1)[0], *ref["pool"])
    assert out.sum() > 0
    rec["outside"]["pool_row_at_rem_plus_1"] = dict(total=int(out.sum()), elements=int(out.size))
    # the seams, on the impulse row: every frame whose impulse sits within two pixels left of / above the seam must show it
    ci = CC.K3_BY_ID["c64_impulse_13x17x130" if C == 64 else "c80_impulse_13x9x70"]
    opi, refi = k3_ref(ci)
    for name, hit in (("seam_x", lambda y, x: tw - 2 <= x < tw), ("seam_y", lambda y, x: th - 2 <= y < th)):
        bad = CC.k3_reference(C, opi["g1"], opi["ca"], opi, pt_ar(), fault=name, seam=(th, tw))["g2"][0]
        out = CC.outside(bad, *refi["g2"])
        frames = [t for t, (y, x) in enumerate(opi["impulse"]) if hit(y, x)]
        assert len(frames) >= 3 and all(out[t].any() for t in frames), (C, name, [int(out[t].sum()) for t in frames])
        line = out[:, :, tw] if name == "seam_x" else out[:, th]
        assert int(out.sum()) == int(line.sum()), (C, name, "outside off the seam")
        rec["outside"][name] = dict(total=int(out.sum()), frames=frames, per_frame=[int(out[t].sum()) for t in frames])
    if C == 64:                                                                 # a nonzero planar pad column reaches the last two image columns
        cp = CC.K3_BY_ID["c64_2x2_tiles_2x12x70"]
        opp, refp = k3_ref(cp)
        out = CC.outside(CC.k3_reference(C, opp["g1"], opp["ca"], opp, pt_ar(), fault="pad_column")["g2"][0], *refp["g2"])
        xx = np.mgrid[0:cp.h, 0:cp.w][1]
        _check(rec, C, "pad_column_w70", out, xx >= cp.w - 2)
    cw = CC.K3_BY_ID["c64_walk_44x17x65" if C == 64 else "c80_walk_66x5x33"]
    opw, refw = k3_ref(cw)
    out = CC.outside(CC.k3_reference(C, opw["g1"], opw["ca"], opw, pt_ar(), ca_shift=1, want=("g2",))["g2"][0], *refw["g2"])
    assert all(out[t].any() for t in range(cw.T)), (C, "ca_of_next_frame")
    rec["outside"]["ca_of_next_frame_walk_row"] = dict(total=int(out.sum()), elements=int(out.size))
    REPORT.append(rec)


# ---- widths, gains --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CC.K12_CASES, ids=[c.id for c in CC.K12_CASES])
def test_k12_interval_widths(case):
    ops, ref = k12_ref(case)
    st = CC.width_stats(*ref["g1"])
    rec = dict(test="k12_widths", id=case.id, C=case.C, K=case.K, **st)
    if case.pool:
        rec["pool"] = CC.width_stats(*ref["pool"])
    REPORT.append(rec)
    print(case.id, st)
    assert st["median"] <= WIDTH_CAP[case.C], (case.id, st)


@pytest.mark.parametrize("scaled", [False, True], ids=["no_ca", "ca"])
@pytest.mark.parametrize("case", CC.K3_CASES, ids=[c.id for c in CC.K3_CASES])
def test_k3_interval_widths(case, scaled):
    ops, ref = k3_ref(case, scaled)
    lo, hi = ref["g2"]
    if case.family == "impulse":                                                # the footprints only: everything else is 0 of zero width
        m = CC.footprint(case, ops["impulse"])
        lo, hi = lo[m], hi[m]
    st = CC.width_stats(lo, hi)
    REPORT.append(dict(test="k3_widths", id=case.id, C=case.C, scaled=scaled, pool=CC.width_stats(*ref["pool"]), **st))
    print(case.id, scaled, st)
    assert st["median"] <= WIDTH_CAP[case.C], (case.id, st)


def _max16(c, ops, gain):
    o = dict(ops)
    o["w1"] = ops["w1"] * gain
    ar, fw = Arith("interval"), CC.folded(o)
    with np.errstate(all="ignore"):
        for t in c.frames:
            CC.k12_frame(c, o, fw, ar, t)
    return ar.max16


@pytest.mark.parametrize("C", [64, 80])
def test_hot_gain_is_the_smallest_that_leaves_the_fused_range(C):
    """family (c): HOT_GAIN[C] is the smallest power of two at which phase1_cases.reference (the fused kernel's model) trips its own
    max16 <= 2^15 assertion while this chain's largest fp16 value -- `a` and every partial of the nine-tap sum -- stays below 2^15.  Also
    recorded: the gain at which the chain's own `a` passes 2^15 and the one at which it is no longer finite in fp16 (CPU model only)."""
    c = CC.K12_BY_ID[f"c{C}_hot_2x9x33_m1"]
    base = PC.operands(c)

    def fused_trips(gain):
        o = dict(base)
        o["w1"] = base["w1"] * gain
        ar = Arith("interval")
        try:
            with np.errstate(all="ignore"):
                PC.reference(c, o, ar, want=("g2",))
        except AssertionError:
            assert not ar.max16 <= PC.MAX16
            return True
        return False
    gains = [2.0 ** k for k in range(0, 16)]
    first = next(g for g in gains if fused_trips(g) and _max16(c, base, g) < PC.MAX16)
    assert first == CC.HOT_GAIN[C] == c.gain and not any(fused_trips(g) for g in gains if g < first)
    leaves = next(g for g in gains if _max16(c, base, g) > PC.MAX16)
    inf = next(g for g in gains if not np.isfinite(_max16(c, base, g)))
    REPORT.append(dict(test="hot_gain", C=C, gain=first, chain_max16_at_gain=_max16(c, base, first), chain_passes_2_15_at=leaves, chain_not_finite_at=inf))
    print(C, first, leaves, inf)
    assert leaves > first


# ---- the tables -----------------------------------------------------------------------------------------------------------------------------

NCUS = (8, 64, 104, 256, 304)


def test_the_persistent_walk_visits_every_tile_once():
    """the seg / seg0 / seg1 / wpx arithmetic of K3m and K3g (chain_cases.walk) for grids min(ntiles, ncu)"""
    for ncu in NCUS:
        for ntiles in range(1, 701):
            seen = sorted(t for wg in CC.walk(ntiles, min(ntiles, ncu)) for t in wg)
            assert seen == list(range(ntiles)), (ncu, ntiles)


def test_rows_reach_the_edges_they_name():
    for c in CC.K3_CASES:
        if not c.walk:
            continue
        tpf = c.tiles_per_frame
        assert tpf == (6 if c.C == 64 else 4) and CC.walk_frames(c, 256) == c.T and c.T * tpf > 256
        wgs = CC.walk(c.T * tpf, 256)
        multi = [wg for wg in wgs if len(wg) >= 2]
        assert multi and any(wg[0] // tpf != wg[1] // tpf for wg in multi), c.id      # two tiles or more, and a frame crossing
        if "short_last_segment" in c.id:
            assert any(not wg for wg in wgs), c.id                              # a workgroup that starts past its segment's end
        for ncu in (8, 64, 104, 304):                                           # on another device the row is rebuilt, never skipped
            T = CC.walk_frames(c, ncu)
            assert T * tpf > ncu and any(len(wg) >= 2 for wg in CC.walk(T * tpf, min(T * tpf, ncu)))
    by = CC.K3_BY_ID
    assert [len(w) for w in CC.walk(by["c64_8_tiles_4x8x128"].T * by["c64_8_tiles_4x8x128"].tiles_per_frame, 8)] == [1] * 8
    assert by["c64_8_tiles_4x8x128"].T * by["c64_8_tiles_4x8x128"].tiles_per_frame == 8 == by["c80_8_tiles_2x8x64"].T * by["c80_8_tiles_2x8x64"].tiles_per_frame
    assert by["c64_slivers_1x9x65"].tiles_per_frame == 4 == by["c80_slivers_1x5x33"].tiles_per_frame      # 4 tiles: nxcd = 1 (2 x 12 x 70 is 2 x 4 tiles: nxcd = 8, wpx = 1)
    assert by["c64_2x2_tiles_2x12x70"].T * by["c64_2x2_tiles_2x12x70"].tiles_per_frame == 8 and CC.planar_pitch(70) == 72
    assert by["c64_3x3_tiles_2x17x130"].tiles_per_frame == 9 == by["c80_3x3_tiles_2x9x70"].tiles_per_frame
    for C in (64, 80):
        rows = [c for c in CC.K12_CASES if c.C == C]
        assert {c.mode for c in rows} == {0, 1, 2} and {c.wrap for c in rows} == {0, 1, 2} and any(c.clip for c in rows) and any(c.nt for c in rows)
        assert any(c.wrap == 1 - CC.VARIANT_WRAP[C] and c.mode == 1 and (c.h, c.w) == (16, 16) for c in rows)
        t = CC.K12_BY_ID[f"c{C}_3x3_tiles_2x17x70_m2"]
        nrf = -(-t.h // CC.K12_TH) * t.T
        assert -(-t.w // CC.K12_TW) * nrf > 8 and nrf % 8                       # more than 8 tiles, tile rows x frames no multiple of 8
        cls = CC.k12_operands(t)["cls"]
        assert all(int((cls == k).sum()) >= 4 for k in (1, 2, 3))
    assert {CC.planar_pitch(c.w) for c in CC.K12_CASES if c.C == 64} >= {16, 40, 64, 72}
    for C in (64, 80):
        th, tw = CC.K3_TILE[C]
        ci = CC.K3_BY_ID["c64_impulse_13x17x130" if C == 64 else "c80_impulse_13x9x70"]
        pos = CC.impulse_positions(ci.h, ci.w, th, tw)
        assert {(0, 0), (0, ci.w - 1), (ci.h - 1, 0), (ci.h - 1, ci.w - 1)} <= set(pos)
        assert {x for _, x in pos} >= {tw - 1, tw} and {y for y, _ in pos} >= {th - 1, th}


# ---- refusals: every SN_EINVAL comes back before a launch -----------------------------------------------------------------------------------

def test_refusals(lib):
    E = CC.EINVAL
    p = ctypes.c_void_p(4096)                                                   # never dereferenced: every call below returns before a launch
    src = lambda **kw: L.UnitSrc(**{**dict(x=4096, T=4, h=12, w=70, C=64, mode=1, wrap=1, halo=None, t0=0, nt=0, clip=0), **kw})      # noqa: E731
    k12 = lambda s, hw=p, wf=p, b=p, wd=p, g1=p, pool=None, blocked=0: lib.sn_ln_gemm_gate(ctypes.byref(s) if s is not None else None, hw, wf, b, wd, g1, pool, blocked, None)      # noqa: E731
    assert k12(None) == E and k12(src(x=None)) == E
    assert k12(src(), wf=None) == E and k12(src(), b=None) == E and k12(src(), wd=None) == E and k12(src(), g1=None) == E
    for C in (0, 32, 72, 96, 128):
        assert k12(src(C=C)) == E, C
    assert k12(src(mode=-1)) == E and k12(src(mode=3)) == E
    assert k12(src(mode=1), hw=None) == E and k12(src(mode=2), hw=None) == E
    assert k12(src(), blocked=1) == E and k12(src(), blocked=3) == E and k12(src(), blocked=-1) == E and k12(src(C=80), blocked=2) == E
    assert k12(src(wrap=2, halo=None)) == E and k12(src(mode=2, wrap=2, halo=None)) == E
    assert k12(src(t0=-1, nt=2)) == E and k12(src(t0=0, nt=5)) == E and k12(src(t0=3, nt=2)) == E and k12(src(t0=4, nt=1)) == E
    assert k12(src(clip=3)) == E and k12(src(clip=-1)) == E and k12(src(clip=2, wrap=2, halo=4096)) == E
    for kw in (dict(T=0), dict(T=-1), dict(h=0), dict(h=-3), dict(w=0), dict(w=-1)):
        assert k12(src(**kw)) == E, kw
    for fn, C in ((lib.sn_dw5m_gemm_gate, 64), (lib.sn_grp5_gemm_gate, 80)):
        k3 = lambda g1=p, ca=None, w5=p, wf=p, g2=p, pool=None, T=2, h=9, w=33, C=C: fn(g1, ca, w5, wf, g2, pool, T, h, w, C, None)      # noqa: E731
        assert k3(g1=None) == E and k3(w5=None) == E and k3(wf=None) == E and k3(g2=None) == E
        assert k3(C=144 - C) == E and k3(C=0) == E and k3(C=C + 8) == E
        assert k3(T=0) == E and k3(h=0) == E and k3(w=0) == E and k3(T=-1) == E and k3(h=-1) == E and k3(w=-1) == E
    pl = lambda x=p, xp=p, T=2, h=3, w=9, C=64: lib.sn_nhwc_to_planar(x, xp, T, h, w, C, None)      # noqa: E731
    assert pl(x=None) == E and pl(xp=None) == E
    for C in (0, 4, 12, 136, 7):
        assert pl(C=C) == E, C
    assert pl(T=0) == E and pl(h=0) == E and pl(w=0) == E
    assert lib.sn_lngate_blocks(17, 70) == 4 * 3 * 3 and lib.sn_dw5m_blocks(17, 130) == 9 and lib.sn_grp5_blocks(9, 70) == 9
    assert all(lib.sn_planar_pitch(w) == CC.planar_pitch(w) for w in range(1, 140))
