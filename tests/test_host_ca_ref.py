"""CPU: the float64 contracts of tests/ca_cases.py are what they claim, and their bounds can tell a right kernel from a wrong one.

  - the table's (c, cs, cpad, cr) are what Engine's Plan.add_cab makes of the named modules;
  - an fp32 point emulation in the kernels' reduction order (tap products as multiply-then-add and as one FMA) stays inside the bound on every
    case and family, and every frame of every family meets the condition (two positive hidden units, |o| <= 8);
  - the same emulation with ONE fault leaves its bound by >= 8x in at least one family of every channel configuration, and the seam faults
    (a partial row skipped / doubled, a border pixel skipped) are caught by their impulse family in every case;
  - with every rounding off the contract is conv2d(mid, w2, padding=1).mean((2, 3)) into the MLP (torch, float64) to 1e-10;
  - the bilinear reference is torch's, its four faults leave the rounding interval, and the impulse footprints are exact in bf16;
  - the ingest specials round as their comment says.
SN_CA_PRINT=1 prints the measured ratios (DESIGN 3.24 quotes them).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import ca_cases as CA

PRINT = os.environ.get("SN_CA_PRINT", "0") == "1"
_cache = {}


def families(case):
    """{family: (partial, mid, reference, frames that must meet the condition)} of a CAB case, computed once"""
    if case.id not in _cache:
        wts = CA.cab_weights(case.variant, case.pre)
        fam = {}
        p, m, tries = CA.dense_operands(case)
        fam["dense"] = (p, m, None)
        p8, m8, tries8 = CA.dense_operands(case, offset=8.0)
        fam["dense+8"] = (p8, m8, None)
        p, m, rows = CA.impulse_row_operands(case)
        fam["rows"] = (p, m, None)
        p, m, px = CA.impulse_pixel_operands(case)
        fam["pixels"] = (p, m, np.array([k != "interior" for (_, _, k) in px]))
        out = {k: (p, m, CA.cab_ca_reference(case, wts, p, m), sel) for k, (p, m, sel) in fam.items()}
        _cache[case.id] = (out, max(tries, tries8), rows, px)
    return _cache[case.id]


def test_table_matches_the_plan():
    seen = set()
    for case in CA.CAB_CASES:
        w = CA.cab_weights(case.variant, case.pre)
        sd = CA._state_dict(case.variant)
        assert (w["c"], w["cs"], w["cpad"]) == (case.c, case.cs, case.cpad), case.id
        assert w["cr"] == sd[case.pre + "CA.conv_du.0.weight"].shape[0] and w["wa"].shape == (w["cr"], case.c) and w["wb"].shape == (case.c, w["cr"])
        assert w["w2"].shape == (case.c, 9, case.cpad) and (w["w2"][:, :, case.c:] == 0).all()
        assert np.array_equal(CA.bf16(w["w2"]), w["w2"]), "w2 is bf16-rounded like the MFMA operand"
        seen.add((case.c, case.cs, case.cpad))
    assert seen == {(14, 16, 16), (18, 24, 32), (22, 24, 32), (24, 24, 32), (36, 40, 48), (48, 48, 48), (64, 64, 64), (80, 80, 80)}
    assert len(CA.CAB_CASES) == 8 * 9 and len(CA.MLP_CASES) == 6 * 2 * 5
    big = CA.cab_by_id("cab14_37x33_b257")
    assert big.nblk == 16 * big.nsplit + 1 and CA.cab_by_id("cab80_13x70_b40").nblk == 40


@pytest.mark.parametrize("case", CA.CAB_CASES, ids=[c.id for c in CA.CAB_CASES])
def test_cab_ca_emulation_within_the_bound(case):
    wts = CA.cab_weights(case.variant, case.pre)
    fam, tries, rows, px = families(case)
    assert tries <= 4, (case.id, tries)
    assert rows == CA.seam_rows(case.nblk, case.nsplit) and {0, case.nblk - 1} <= set(rows)
    kinds = [k for (_, _, k) in px]
    assert kinds.count("corner") == min(4, case.h * case.w) and (("interior" in kinds) == (case.h > 2 and case.w > 2))
    for name, (p, m, ref, sel) in fam.items():
        ok = ((ref["hid_pre"] > 0).sum(-1) >= 2) & (np.abs(ref["o"]) <= 8.0).all(-1)
        assert ok[sel].all() if sel is not None else ok.all(), (case.id, name, "a frame whose scale says nothing")
        assert (ref["ca"][..., case.c:] == 0).all() and (ref["tol"][..., :case.c] > 0).all()
        for fma in (False, True):
            r = CA.ratio(CA.emulate_cab_ca(case, wts, p, m, fma=fma), ref)
            if PRINT:
                print(f"EMU {case.id} {name} fma={int(fma)} err/tol {r:.3g}")
            assert r <= 1.0, (case.id, name, fma, r)
    if "interior" in kinds:                                    # an interior pixel is invisible to the contract: the zero-input value, 0.5
        ref = fam["pixels"][2]
        f = kinds.index("interior")
        assert (ref["ca"][f, :case.c] == 0.5).all() and (ref["tol"][f, :case.c] == 3 * 2.0 ** -23).all()


@pytest.mark.parametrize("config", range(len(CA.CONFIGS)), ids=[f"c{c[2]}" for c in CA.CONFIGS])
def test_cab_ca_controls_leave_the_bound(config):
    variant, pre, c, cs, cpad = CA.CONFIGS[config]
    wts = CA.cab_weights(variant, pre)
    best = {f: 0.0 for f in CA.CAB_FAULTS}
    for case in CA.CAB_CASES:
        if (case.variant, case.pre) != (variant, pre):
            continue
        fam = families(case)[0]
        for fault in CA.CAB_FAULTS:
            for name, (p, m, ref, _) in fam.items():
                r = CA.ratio(CA.emulate_cab_ca(case, wts, p, m, fault=fault), ref)
                best[fault] = max(best[fault], r)
                if PRINT:
                    print(f"CTL {case.id} {fault} {name} {r:.3g}")
                if CA.SEAM_FAULTS.get(fault) == name:
                    assert r >= CA.CONTROL_RATIO, (case.id, fault, name, r)
    for fault, r in best.items():
        assert r >= CA.CONTROL_RATIO, (c, fault, r)


@pytest.mark.parametrize("case", CA.CAB_CASES, ids=[c.id for c in CA.CAB_CASES])
def test_cab_ca_contract_is_the_calayer_of_conv2(case):
    wts = CA.cab_weights(case.variant, case.pre)
    for offset in (0.0, 8.0):
        _, mid, _ = CA.dense_operands(case, offset=offset)
        ref = CA.cab_ca_reference(case, wts, CA.block_sums(case, mid, dtype=np.float64), mid)
        want = CA.torch_calayer(case, wts, mid)
        assert np.abs(ref["ca"][:, :case.c] - want).max() <= 1e-10, case.id


@pytest.mark.parametrize("case", CA.MLP_CASES, ids=[c.id for c in CA.MLP_CASES])
def test_ca_mlp_emulation_and_controls(case):
    wts = CA.mlp_weights(case)
    p, inv, tries = CA.mlp_operands(case)
    assert tries <= CA.MAX_SEED_TRIES, (case.id, tries)
    pi, inv_i, rows = CA.mlp_impulse_operands(case)
    assert {0, case.nblk - 1} <= set(rows) and inv == inv_i
    best = {f: 0.0 for f in CA.MLP_FAULTS}
    for name, part in (("dense", p), ("rows", pi)):
        ref = CA.ca_mlp_reference(case, wts, part, inv)
        assert CA.condition(ref), (case.id, name)
        for fma in (False, True):
            r = CA.ratio(CA.emulate_ca_mlp(case, wts, part, inv, fma=fma), ref)
            if PRINT:
                print(f"EMU {case.id} {name} fma={int(fma)} err/tol {r:.3g}")
            assert r <= 1.0, (case.id, name, fma, r)
        for fault in CA.MLP_FAULTS:
            r = CA.ratio(CA.emulate_ca_mlp(case, wts, part, inv, fault=fault), ref)
            best[fault] = max(best[fault], r)
            if name == "rows" and fault != "no_relu":
                assert r >= CA.CONTROL_RATIO, (case.id, fault, r)
    if PRINT:
        print(f"CTL {case.id} {best}")
    assert best["no_relu"] >= CA.CONTROL_RATIO, (case.id, best)
    # the float64 tail is torch's
    t = torch.from_numpy(np.asarray(p, np.float64)[..., :case.c]).sum(1) * float(inv)
    want = torch.sigmoid(torch.relu(t @ torch.from_numpy(wts["wa"]).double().T) @ torch.from_numpy(wts["wb"]).double().T).numpy()
    assert np.abs(CA.ca_mlp_reference(case, wts, p, inv)["ca"][:, :case.c] - want).max() <= 1e-10


# ---- sn_upsample2_add ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", CA.UP_MAPS, ids=[f"{h}x{w}" for h, w in CA.UP_MAPS])
def test_upsample_reference_is_torchs_and_the_controls_leave_the_interval(hw):
    hs, ws = hw
    lo, res = CA.upsample_operands(hs, ws, 24, seed=900 + 10 * hs + ws)
    ref, tol = CA.upsample_add_reference(lo.float().numpy(), res.float().numpy())
    want = Fn.interpolate(lo.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False).permute(0, 2, 3, 1) + res.double()
    assert np.abs(ref - want.numpy()).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    a, b = CA.upsample_interval(ref, tol)
    # an fp32 evaluation in the kernel's order lies inside
    emu = emulate_upsample(lo.float().numpy(), res.float().numpy())
    assert ((emu >= a) & (emu <= b)).all()
    for fault in CA.UP_FAULTS:
        bad, _ = CA.upsample_add_reference(lo.float().numpy(), res.float().numpy(), fault=fault)
        stored = CA.round_bf16_f64(bad)
        out = int(((stored < a) | (stored > b)).sum())
        differs = {"align_corners": hs * ws > 1, "weights_exchanged": hs * ws > 1, "no_clamp_low": True, "no_clamp_high": True}[fault]
        if PRINT:
            print(f"UP {hs}x{ws} {fault}: {out} of {stored.size} outside")
        assert (out > 0) == differs, (hw, fault, out)


def emulate_upsample(lo, res):
    """upsample2_add_kernel in fp32, operation by operation: va = hx a0 + lx a1 per source row, (hy va + ly vb) + res, bf16"""
    f = np.float32
    T, hs, ws, cs = lo.shape
    out = np.zeros((T, 2 * hs, 2 * ws, cs), f)
    for x in range(2 * ws):
        sx = max(f(x) * f(0.5) - f(0.25), f(0))
        x0 = int(sx)
        x1 = min(x0 + 1, ws - 1)
        lx = f(sx - x0)
        hx = f(1) - lx
        col = hx * lo[:, :, x0] + lx * lo[:, :, x1]               # [T][hs][cs], one value per source row
        for i in range(hs):
            ra, rc = max(i - 1, 0), min(i + 1, hs - 1)
            ly0 = f(0.75) if i > 0 else f(0)
            hy0 = f(1) - ly0
            out[:, 2 * i, x] = (hy0 * col[:, ra] + ly0 * col[:, i]) + res[:, 2 * i, x]
            out[:, 2 * i + 1, x] = (f(0.75) * col[:, i] + f(0.25) * col[:, rc]) + res[:, 2 * i + 1, x]
    return CA.bf16(out).astype(np.float64)


def test_upsample_impulse_footprints_are_exact_in_bf16():
    for (hs, ws) in CA.UP_MAPS:
        for (y, x) in CA.upsample_impulses(hs, ws):
            lo = np.zeros((1, hs, ws, 8))
            lo[0, y, x] = 2.0 ** np.arange(-3, 5)
            ref, tol = CA.upsample_add_reference(lo, np.zeros((1, 2 * hs, 2 * ws, 8)))
            assert np.array_equal(CA.round_bf16_f64(ref), ref), (hs, ws, y, x)
            assert np.allclose(ref.sum((1, 2)), 4 * lo.sum((1, 2)), rtol=0, atol=0), "the weights of a source pixel sum to 4"
            q = np.unique(ref[0, :, :, 3])                        # amplitude 1
            assert set(q) <= {0.0, 1 / 16, 3 / 16, 9 / 16, 4 / 16, 12 / 16, 1.0}, q


def test_round_bf16_is_torchs():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4096, generator=g, dtype=torch.float64) * torch.exp2(torch.rand(4096, generator=g, dtype=torch.float64) * 40 - 20)
    x = x.float().double()
    assert np.array_equal(CA.round_bf16_f64(x.numpy()), x.float().to(torch.bfloat16).double().numpy())


# ---- sn_ingest -----------------------------------------------------------------------------------------------------------------------------

def test_ingest_specials_round_as_stated():
    sp = torch.tensor(CA.INGEST_SPECIALS, dtype=torch.float32)
    got = sp.to(torch.bfloat16).float().tolist()
    assert got[:4] == [1.0, 1.0 + 2.0 ** -6, -1.0, -(1.0 + 2.0 ** -6)]
    assert got[6:10] == [1.0, 1.0 + 2.0 ** -7, 2.0, -2.0] and got[10] == float("inf") and got[11] == float("-inf")
    assert got[12] == 3.3895313892515355e38 and got[13] == 1.0
    assert str(got[4]) == "0.0" and str(got[5]) == "-0.0"
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        src, nz = CA.ingest_operands(dt, 3, 257, True, seed=1)
        ref = CA.ingest_reference(src, nz)
        assert ref.shape == (CA.INGEST_T, 257, 8) and (ref[..., 4:].float() == 0).all()
        assert torch.equal(ref[..., 3].float(), nz.to(torch.bfloat16).float()[:, 0])
        tiny = (src.float().abs() < 2.0 ** -14) & (src.float() != 0)
        assert not tiny.any(), "no subnormal of any source format"
