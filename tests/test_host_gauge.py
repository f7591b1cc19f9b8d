"""CPU checks of the gate's rescaling symmetry (tests/gauge.py) and of what it needs from the interval reference of tests/phase1_cases.py.

  * the helper is right: on all four variants a regauged synth_state_dict gives the oracle's CAB1, CAB2 and whole forward bit for bit, and the drop-in
    module loads it strict=True;
  * phase1_cases.reference with every rounding off is bit for bit the base on every rung of the ladder;
  * containment: point emulations that KEEP fp16 subnormals are inside the "keep16" intervals, kept and flushed ones inside the "either" intervals;
  * the control: a point emulation that FLUSHES leaves the keep16 intervals at k = -4 and k = -6 on every row -- the test of the kernel
    (tests/test_gpu_phase1_gauge.py) can tell the two apart;
  * a rung the interval reference refuses would be dropped for that row and listed; the uniform and lopsided rungs are accepted on every row;
  * packing: at k = -7 the fused kernel's second 1x1 is not finite in fp16; Plan.add_naf notices and Engine acts on it (three branches).
Per row and rung the shares and widths go to parity_report_gauge_ref.json in $SN_PARITY_REPORT_DIR (default: parity_out/ at the repository root).
"""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gauge as G
import phase1_cases as PC
from oracle import shiftnet_oracle as O
from shiftnet_amd import lib as L
from shiftnet_amd import prep
from shiftnet_amd.spec import VARIANTS
from shiftnet_amd.weights import synth_state_dict

REPORT = []
ROWS = G.phase1_rows()
CONTROL_RUNGS = ("k-4", "k-6")               # a third / over 95 % of g1 is below 2^-14 there; at k = -2 (5 %) a flushed run may still be inside: not asserted


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    d = os.environ.get("SN_PARITY_REPORT_DIR") or os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report_gauge_ref.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "shift-net_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    return L.load()


# ---- the helper is right ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(O.VARIANTS))
def test_regauged_checkpoint_is_the_same_function_bit_for_bit(name):
    """per block and channel random exponents in +-6: CAB2 (both directions), CAB1, a unit and the whole forward on the smallest clip the topology
    allows (three levels of stride 2: 8 x 8) are torch.equal to the base; keys, shapes and the drop-in module's strict load are unchanged"""
    import importlib
    V = O.VARIANTS[name]
    sd = synth_state_dict(name)
    rg = G.regauge_state_dict(name, sd, *G.seeded_exponents(6, 5))
    assert list(rg) == list(sd) and all(rg[k].shape == sd[k].shape and rg[k].dtype == sd[k].dtype for k in sd)
    pres = G.naf_prefixes(sd)
    assert len(pres) == 2 * V.units * (12 if V.topo == "small" else 7)
    changed = [k for k in sd if not torch.equal(rg[k], sd[k])]
    assert len(changed) == len(pres) * (2 + int(V.denoise) + 2 * int(V.grouped_rep)), len(changed)      # body.0, the second 1x1; conv_du.0; conv_1, conv_2
    assert all(rg[k] is sd[k] for k in sd if k not in changed)                  # untouched keys, the aliased PReLU slopes among them, keep their tensors
    g = torch.Generator().manual_seed(11)
    C = V.c1
    x = torch.randn((3, C, 12, 20), generator=g)
    blk = "stage1.decoder_level1."
    with torch.no_grad():
        for rev, unit in ((False, "encoder_level1."), (True, "encoder_level1_1.")):
            u = O.gsts_gather(x, rev, V.wrap)
            assert torch.equal(O.cab2(rg, blk + unit + "0.", u, V), O.cab2(sd, blk + unit + "0.", u, V)), (name, unit)
            assert torch.equal(O.cab1(rg, blk + unit + "1.", x, V), O.cab1(sd, blk + unit + "1.", x, V)), (name, unit)
            assert torch.equal(O.gsts_unit(rg, blk + unit, x, rev, V), O.gsts_unit(sd, blk + unit, x, rev, V)), (name, unit)
        T, H, W = V.past + V.future + 1, 8, 8
        clip = torch.rand((1, T, 3, H, W), generator=g)
        nm = torch.full((1, T, 1, H, W), 30.0 / 255.0) if V.denoise else None
        assert torch.equal(O.forward(V, rg, clip, nm), O.forward(V, sd, clip, nm)), name
    mod = importlib.import_module(f"basicsr.models.archs.{name}")
    mod.GShiftNet().load_state_dict(rg, strict=True)


@pytest.mark.parametrize("C", [64, 80])
def test_regauge_ops_scales_what_the_docstring_says(C):
    c = PC.P1Case("ops", C, 1, 2, 2, 1, 0, seed=5 + C)
    ops = PC.operands(c)
    ks, kt = G.random_exponents(C, 6, 9)
    rg = G.regauge_ops(ops, ks, kt)
    u = ks + kt
    assert all(rg[k] is ops[k] for k in ops if k not in ("w1", "w2", "w_rep5", "w_rep3"))
    w1, r1 = ops["w1"].double().numpy(), rg["w1"].double().numpy()
    assert np.array_equal(r1[:C], w1[:C] * 2.0 ** ks[:, None, None, None]) and np.array_equal(r1[C:], w1[C:] * 2.0 ** kt[:, None, None, None])
    assert np.array_equal(rg["w2"].double().numpy(), ops["w2"].double().numpy() * 2.0 ** -u[None, :, None, None])
    for k in ("w_rep5", "w_rep3"):
        if C == 64:
            assert rg[k] is ops[k]
        else:
            w, r = ops[k].double().numpy(), rg[k].double().numpy()
            for oc in (0, 7, 8, 41, 79):
                for j in range(8):
                    assert np.array_equal(r[oc, j], w[oc, j] * 2.0 ** (u[oc] - u[8 * (oc // 8) + j]))


# ---- the ladder on the rows of the GPU test ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ROWS, ids=[c.id for c in ROWS])
def test_ladder_exact_containment_and_control(case, lib):
    c = case
    ops = PC.operands(c)
    bounds = PC.strip_bounds(lib, c.w)
    want = ("g2", "v", "g1")
    base = PC.reference(c, ops, PC.Arith("exact"), want=want)
    dropped = []
    for tag, ks, kt in G.ladder(c.C):
        o = G.regauge_ops(ops, ks, kt)
        ex = PC.reference(c, o, PC.Arith("exact"), want=want)
        # g1 is the one stage that moves: by 2^u per channel, exactly; everything behind the second 1x1 is bit for bit the base
        assert np.array_equal(ex["v"][0], base["v"][0]) and np.array_equal(ex["g2"][0], base["g2"][0]), (c.id, tag)
        assert np.array_equal(ex["g1"][0], base["g1"][0] * 2.0 ** (ks + kt)), (c.id, tag)
        refs = {}
        for kind, keep in (("either", False), ("keep16", True)):
            refs[kind], why = G.try_reference(c, o, PC.Arith("interval", keep16=keep), want)
            if refs[kind] is None:
                dropped.append(dict(rung=tag, interval=kind, reason=why))
        if len(refs) != 2 or any(v is None for v in refs.values()):
            REPORT.append(dict(id=c.id, rung=tag, dropped=True, reason=dropped[-1]["reason"]))
            continue
        rec = dict(id=c.id, rung=tag, dropped=False, g1_below_2e14=float((np.abs(ex["g1"][0]) < PC.SUB16).mean()))
        # what the kernel writes on this row: g2 and its pool rows, or (sums pass) the pool rows of 16 g1
        def outputs(r, ar):
            if c.kind == "sums":
                return {"g1_pool": PC.pool_rows(ar, (16.0 * r["g1"][0], 16.0 * r["g1"][1]), bounds)}
            return {"g2": r["g2"], "pool": PC.pool_rows(ar, r["v"], bounds)}
        iv = {kind: outputs(r, PC.Arith("interval", keep16=kind == "keep16")) for kind, r in refs.items()}
        for kind in iv:
            for what, (lo, hi) in iv[kind].items():
                assert (lo <= hi).all()
                rec[f"width_{kind}_{what}"] = PC.width_stats(lo, hi)
        for what in iv["either"]:                                             # keep16 only drops an extension: it is inside "either"
            assert (iv["keep16"][what][0] >= iv["either"][what][0]).all() and (iv["keep16"][what][1] <= iv["either"][what][1]).all(), (c.id, tag, what)
        runs = [(1.0, False, 0), (-1.0, False, 0), (None, False, 1), (None, True, 2)]
        flushed_outside = 0
        for share, flush, seed in runs:
            ar = PC.Arith("point", np.random.default_rng(seed), share, flush)
            pt = outputs(PC.reference(c, o, ar, want=want), ar)
            for what, (p, _) in pt.items():
                assert not PC.outside(p, *iv["either"][what]).any(), (c.id, tag, what, share, flush)
                out_keep = int(PC.outside(p, *iv["keep16"][what]).sum())
                if not flush:
                    assert out_keep == 0, (c.id, tag, what, share, out_keep)
                else:
                    flushed_outside += out_keep
                    rec[f"flushed_outside_keep16_{what}"] = out_keep / p.size
        if tag in CONTROL_RUNGS:
            assert flushed_outside >= 1, (c.id, tag)
        REPORT.append(rec)
    # the uniform and the lopsided rungs are inside the reference's range on every row of the table (a row that refused one would get another seed)
    assert not [d for d in dropped if not d["rung"].startswith("random")], (c.id, dropped)


# ---- packing ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [64, 80])
def test_packing_beyond_the_ladder_is_not_finite_and_says_nothing(C):
    """uniform k = -7: the compensated second 1x1, times 1 / P1_G1_SCALE, passes 65504 and prep.pack_phase1r writes inf; the reference refuses the rung.
    The chain's own operands stay finite there (its second 1x1 and RepConv are bf16, its stencil is untouched by the symmetry); pk_f16_words and
    _h2_words round beyond-range values to inf just as silently."""
    c = PC.P1Case("pack", C, 1, 2, 2, 0, 0, seed=17 + C)
    ops = PC.operands(c)
    k = np.full(C, G.PACK_OVERFLOW_K)
    cold = G.regauge_ops(ops, k, k)
    pk = PC.packed(cold)
    assert not torch.isfinite(pk["wfrag2"]).all()
    assert torch.isfinite(pk["wgrp"]).all() and torch.isfinite(pk["w3"].view(torch.float16)).all() and torch.isfinite(pk["wfrag1"].float()).all()
    assert torch.isfinite(PC.packed(ops)["wfrag2"]).all()
    assert G.try_reference(c, cold, PC.Arith("interval"), ("g2",))[0] is None
    assert torch.isfinite(prep.pack_gate_gemm(cold["w2"], C).float()).all()
    big = torch.tensor([[1.0, 7.0e4], [-7.0e4, 2.0]])
    assert not torch.isfinite(prep.pk_f16_words(big).view(torch.float16)).all()
    with np.errstate(over="ignore"):
        assert not np.isfinite(prep._h2_words(big.numpy()[0], big.numpy()[1]).view(np.float16)).all()
    if C == 80:                                                                 # lopsided per channel inside a group: the grouped RepConv's ratios overflow fp16 too
        ks = np.where(np.arange(C) % 8 == 0, 10, -10)
        assert not torch.isfinite(PC.packed(G.regauge_ops(ops, ks, np.zeros(C, np.int64)))["wgrp"]).all()


def _naf_plan(name: str, pre: str, sd):
    """a Plan that holds one CAB1 / CAB2, built by Plan.add_naf on the CPU"""
    from shiftnet_amd.engine import Plan, host_f32_copy
    P = Plan.__new__(Plan)
    P.V, P.device = VARIANTS[name], torch.device("cpu")
    P.sd = host_f32_copy({k: v for k, v in sd.items() if k.startswith(pre)})
    P.convs, P.cas, P.units = {}, {}, {}
    P.add_naf(pre, sd[pre + "beta"].shape[1], pre + "conv1.weight" in sd)
    return P


@pytest.mark.parametrize("name", ["gshift_deblur2", "gshift_denoise1"])
def test_plan_and_engine_act_on_a_packing_that_is_not_finite(name, lib, monkeypatch):
    from shiftnet_amd.engine import Engine
    pre = "stage1.decoder_level1.encoder_level1.0."
    sd = synth_state_dict(name)
    base = _naf_plan(name, pre, sd)
    assert base.p1r_not_finite is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert Engine(base).phase1 == Engine.phase1                            # nothing to say about a checkpoint that packs
    cold = _naf_plan(name, pre, G.regauge_state_dict(name, sd, G.PACK_OVERFLOW_K, G.PACK_OVERFLOW_K))
    assert cold.p1r_not_finite == pre + "wfrag2"
    # fused operand not finite, SN_PHASE1=auto: one warning that names it, and the module starts on the chain
    monkeypatch.setattr(Engine, "phase1", "auto")
    with pytest.warns(UserWarning, match="wfrag2") as rec:
        eng = Engine(cold)
    assert len(rec) == 1 and pre in str(rec[0].message)
    assert eng.phase1 == "0" and not eng._fused_phase1(4) and eng.fallbacks == 0
    # ... SN_PHASE1=r: the explicit request cannot be honoured
    monkeypatch.setattr(Engine, "phase1", "r")
    with pytest.raises(ValueError, match="wfrag2"):
        Engine(cold)
    # ... SN_PHASE1=0: the chain was asked for, nothing to report
    monkeypatch.setattr(Engine, "phase1", "0")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert Engine(cold).phase1 == "0"
    # chain operand not finite: no half-precision path is left
    hot = dict(sd)
    w = sd[pre + "body.1.conv_2.weight"].clone()
    w[3, 0, 0, 2] = 7.0e4
    hot[pre + "body.1.conv_2.weight"] = w
    with pytest.raises(ValueError, match=r"body\.1\.conv_2\.weight.*float32"):
        _naf_plan(name, pre, hot)


# ---- the chain's K12 ----------------------------------------------------------------------------------------------------------------------------------

CHAIN_ROWS = G.chain_rows()


@pytest.mark.parametrize("case", CHAIN_ROWS, ids=[c.id for c in CHAIN_ROWS])
def test_chain_k12_ladder_containment(case):
    """chain_cases.k12_reference shares Arith: the un-rounded gate product moves by 2^u exactly on every rung, every rung is accepted, point
    emulations that keep fp16 subnormals are inside the keep16 intervals, kept and flushed ones inside the "either" intervals.  The share of
    flushed elements outside keep16 is recorded, not asserted: the chain's `a` is 2^k of the base (its g1 is bf16), so even at k = -6 few are."""
    import chain_cases as CC
    c = case
    ops = CC.k12_operands(c)
    base = CC.k12_reference(c, ops, CC.Arith("exact"), want=("p",))["p"][0]
    for tag, ks, kt in G.ladder(c.C):
        o = G.regauge_ops(ops, ks, kt)
        assert np.array_equal(CC.k12_reference(c, o, CC.Arith("exact"), want=("p",))["p"][0], base * 2.0 ** (ks + kt)), (c.id, tag)
        iv = {kind: CC.k12_reference(c, o, CC.Arith("interval", keep16=kind == "keep16")) for kind in ("either", "keep16")}
        rec = dict(id=c.id, rung=tag, dropped=False)
        for share, flush, seed in [(1.0, False, 0), (-1.0, False, 0), (None, False, 1), (None, True, 2)]:
            pt = CC.k12_reference(c, o, CC.Arith("point", np.random.default_rng(seed), share, flush))
            for what in ("g1", "pool") if c.pool else ("g1",):
                assert not CC.outside(pt[what][0], *iv["either"][what]).any(), (c.id, tag, what, share, flush)
                n = int(CC.outside(pt[what][0], *iv["keep16"][what]).sum())
                if flush:
                    rec[f"flushed_outside_keep16_{what}"] = n / pt[what][0].size
                else:
                    assert n == 0, (c.id, tag, what, share, n)
        REPORT.append(rec)
