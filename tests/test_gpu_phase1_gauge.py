"""-m gpu: the fused phase 1 (csrc/sn_phase1r.hip) along the gate's rescaling orbit (tests/gauge.py), through the C ABI as tests/test_gpu_phase1_edges.py
runs it: does every fp16 stage of the kernel keep subnormals?

The kernel carries `a`, g1 = a1 a2 2^-4 and r in fp16.  A checkpoint whose body.0 rows are 2^k times the synthetic ones (the second 1x1 compensates,
the network function is the same bit for bit in fp32) puts g1 at 4^k: at k = -4 a third of it is below 2^-14.  The interval reference that pins the
kernel accepts a consumer that flushes there (the "either" interval of tests/phase1_cases.py); a flushing kernel would lose one to two decimal
digits in every GSTS block without any test noticing.  Per row (the smallest shapes with every mechanism, C = 64 and C = 80) and rung (uniform
k = -6 .. +6, two lopsided, one per-channel random draw), with the operands packed by prep.pack_phase1r from the regauged weights:
  1. every g2 element is written and inside the "either" interval, every pool row inside its interval sum, guards intact -- whatever the hardware
     does with subnormals;
  2. every g2 element and pool row is inside the "keep16" interval, which holds only if NO stage flushes (tests/test_host_gauge.py: a point emulation
     that flushes leaves it at k = -4 and k = -6 on every row); a failing element names the stage it left;
  3. team sizes 1 and 2 and the denoisers' g1 store give the bits of the library's own plan.
Each row and rung adds a record to parity_report_phase1_gauge.json in $SN_PARITY_REPORT_DIR (default: parity_out/ at the repository root): the share
of g1 below 2^-14, inside / outside counts and width statistics of both intervals, and the rms error of the kernel's output against the exact float64
function over the tensor's rms, next to the same figure at the base rung (measured, not asserted).  A rung the interval reference refuses is listed
as dropped with the reason and not run.

Measured on MI355X: see the docstring of test_phase1_along_the_orbit.
"""
import json
import os

import numpy as np
import pytest
import torch

import chain_cases as CC
import gauge as G
import phase1_cases as PC
from test_gpu_chain_edges import dv, k12_launch, k3_launch
from test_gpu_chain_edges import inside as chain_inside
from test_gpu_phase1_edges import Dev, inside

pytestmark = pytest.mark.gpu
REPORT = []
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = G.phase1_rows()
RUNGS = {C: G.ladder(C) for C in (64, 80)}
CASES = [(c, i) for c in ROWS for i in range(len(RUNGS[c.C]))]


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    d = os.environ.get("SN_PARITY_REPORT_DIR") or os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report_phase1_gauge.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    from shiftnet_amd import lib as L
    return L.load(), L


class Run:
    """one row at one rung on the device: the launches of its kind and the row's outputs as {name: tensor}"""

    def __init__(self, c, ops, lb, L):
        self.c, self.d = c, Dev(c, ops, lb, L)
        self.fr = slice(c.frames.start, c.frames.stop)

    def outputs(self):
        c, d, fr = self.c, self.d, self.fr
        if c.kind == "sums":
            _, pool = d.launch("sums", g2=False, sums=True)
            _, pool_s = d.launch("sums_store", g2=False, sums=True, store=d.g1_store())
            assert torch.equal(pool_s[fr], pool[fr]), c.id
            return {"g1_pool": pool[fr]}
        if c.kind == "scale":
            g2, pool = d.launch("scale", scale=True)
            store = d.g1_store()
            d.launch("sums_store", g2=False, sums=True, store=store)
            g2_s, pool_s = d.launch("scale_store", scale=True, store=store)
            assert torch.equal(g2_s[fr].view(torch.int16), g2[fr].view(torch.int16)) and torch.equal(pool_s[fr], pool[fr]), c.id
            return {"g2": g2[fr], "pool": pool[fr]}
        g2, pool = d.launch("team0")
        for team in (1, 2):
            g2_t, pool_t = d.launch(f"team{team}", team=team)
            assert torch.equal(g2_t[fr].view(torch.int16), g2[fr].view(torch.int16)) and torch.equal(pool_t[fr], pool[fr]), (c.id, team)
        return {"g2": g2[fr], "pool": pool[fr]}


def intervals(c, ref, bounds, keep16):
    ar = PC.Arith("interval", keep16=keep16)
    if c.kind == "sums":
        return {"g1_pool": PC.pool_rows(ar, (16.0 * ref["g1"][0], 16.0 * ref["g1"][1]), bounds)}
    return {"g2": ref["g2"], "pool": PC.pool_rows(ar, ref["v"], bounds)}


_BASE = {}


def base_of(c, lb, L, bounds):
    """(operands, the exact float64 outputs, the kernel's error against them) of a row at the base rung, once per row"""
    if c.id not in _BASE:
        ops = PC.operands(c)
        ex = PC.reference(c, ops, PC.Arith("exact"), want=("v", "g1"))
        _BASE[c.id] = (ops, ex, errors(c, Run(c, ops, lb, L).outputs(), exact_outputs(c, ex, bounds, 0)))
    return _BASE[c.id]


def exact_outputs(c, ex, bounds, u):
    """the exact function's outputs at a rung: g2 and its pool rows do not move along the orbit, g1 moves by 2^u per channel"""
    ar = PC.Arith("exact")
    if c.kind == "sums":
        g1 = 16.0 * ex["g1"][0] * 2.0 ** np.asarray(u, np.float64)
        return {"g1_pool": PC.pool_rows(ar, (g1, g1), bounds)[0]}
    return {"g2": ex["v"][0], "pool": PC.pool_rows(ar, ex["v"], bounds)[0]}


def errors(c, got, exact):
    return {k: G.rel_rms_error(got[k].double().cpu().numpy(), exact[k]) for k in got}


@pytest.mark.parametrize("case,rung", CASES, ids=[f"{c.id}-{RUNGS[c.C][i][0]}" for c, i in CASES])
def test_phase1_along_the_orbit(case, rung, lib):
    """Measured on MI355X (gfx950): every row and rung is inside BOTH intervals -- the kernel keeps fp16 subnormals in every stage (the conversion,
    the packed FMAs, the gate product, the fp16 MFMA operands) -- and the error against the exact function at k = -6 (98 % of g1 subnormal) is
    at most 10 % above the base rung's on every row (k = -4: 0.3 %; g2 of 2 x 9 x 65, C = 80, second pass: 4.17e-3 base, 4.17e-3 at k = -4, 4.34e-3
    at k = -6): the cold range ends at k = -7, where the packing overflows, not at the arithmetic.  parity_report_phase1_gauge.json has the figures."""
    lb, L = lib
    c = case
    tag, ks, kt = RUNGS[c.C][rung]
    bounds = PC.strip_bounds(lb, c.w)
    ops0, ex, base_err = base_of(c, lb, L, bounds)
    ops = G.regauge_ops(ops0, ks, kt)
    rec = dict(test="phase1_gauge", id=c.id, rung=tag, shape=[c.T, c.h, c.w, c.C], mode=c.mode, kind=c.kind, strips=bounds, dropped=False)
    want = ("g2", "v", "g1")
    refs = {}
    for kind, keep in (("either", False), ("keep16", True)):
        refs[kind], why = G.try_reference(c, ops, PC.Arith("interval", keep16=keep), want)
        if refs[kind] is None:
            rec.update(dropped=True, reason=why)
            REPORT.append(rec)
            assert tag.startswith("random"), (c.id, tag, why)                    # tests/test_host_gauge.py: only the random draw may be refused
            return
    rec["g1_below_2e14"] = float((np.abs(refs["keep16"]["g1"][0]) < PC.SUB16).mean())
    got = Run(c, ops, lb, L).outputs()
    failed = []
    for kind in ("either", "keep16"):
        iv = intervals(c, refs[kind], bounds, kind == "keep16")
        rec[f"widths_{kind}"] = {what: PC.width_stats(*iv[what]) for what in iv}
        for what in iv:
            try:
                inside(c, ops, rec, kind, what, got[what], *iv[what], keep16=kind == "keep16")
            except AssertionError as e:
                failed.append(f"{kind}: {e}")
    err = errors(c, got, exact_outputs(c, ex, bounds, ks + kt))
    rec["rel_rms_error_vs_exact"] = err
    rec["rel_rms_error_vs_exact_base_rung"] = base_err
    rec["verdict"] = {kind: not any(f.startswith(kind) for f in failed) for kind in ("either", "keep16")}
    REPORT.append(rec)
    print(f"{c.id} {tag}: g1 below 2^-14 {rec['g1_below_2e14']:.3f}, error vs exact {err} (base {base_err}), verdict {rec['verdict']}")
    assert not failed, failed


# ---- the two-kernel chain (what the engine falls back to) -----------------------------------------------------------------------------------------

CHAIN_ROWS = G.chain_rows()
CHAIN_CASES = [(c, i) for c in CHAIN_ROWS for i in range(len(RUNGS[c.C]))]


@pytest.mark.parametrize("case,rung", CHAIN_CASES, ids=[f"{c.id}-{RUNGS[c.C][i][0]}" for c, i in CHAIN_CASES])
def test_chain_along_the_orbit(case, rung, lib):
    """K12 (sn_ln_gemm_gate: `a` and the nine-tap sum are fp16, g1 is bf16) on the regauged operands inside the "either" and the "keep16" interval
    of chain_cases.k12_reference, then K3m / K3g (no fp16 stage: one interval) on the g1 the device wrote, as the hot rows of
    tests/test_gpu_chain_edges.py chain them.  The chain's `a` is 2^k of the base, not 4^k: at k = -6 under 1 % of it is subnormal.
    Measured on MI355X: every row and rung inside both intervals."""
    lb, L = lib
    c = case
    tag, ks, kt = RUNGS[c.C][rung]
    ops = G.regauge_ops(CC.k12_operands(c), ks, kt)
    fr = slice(c.frames.start, c.frames.stop)
    rec = dict(test="chain_gauge", id=c.id, rung=tag, shape=[c.T, c.h, c.w, c.C], mode=c.mode, dropped=False)
    refs = {}
    for kind, keep in (("either", False), ("keep16", True)):
        try:
            refs[kind] = CC.k12_reference(c, ops, CC.Arith("interval", keep16=keep), want=("g1", "p", "a"))
        except AssertionError as e:
            rec.update(dropped=True, reason=f"the interval reference refuses: {str(e)[:80]}")
            REPORT.append(rec)
            assert tag.startswith("random"), (c.id, tag, str(e))
            return
    rec["a_below_2e14"] = float((np.abs(refs["keep16"]["a"][0]) < PC.SUB16).mean())
    d = {k: dv(ops[k]) for k in ("x", "halo", "hw")}
    pk = {k: dv(v) for k, v in CC.packed(ops).items()}
    g1, _, pool = k12_launch(lb, L, c, d, pk, 0, c.pool, tag)
    failed = []
    for kind in ("either", "keep16"):
        rec[f"widths_{kind}"] = CC.width_stats(*refs[kind]["g1"])
        for what, got in (("g1", g1[fr]),) + ((("pool", pool[fr]),) if c.pool else ()):
            try:
                chain_inside(rec, kind, what, got, *refs[kind][what])
            except AssertionError as e:
                failed.append(f"{kind}: {e}")
    rec["verdict"] = {kind: not any(f.startswith(kind) for f in failed) for kind in ("either", "keep16")}
    g1c = g1[fr].contiguous()
    assert bool(torch.isfinite(g1c.float()).all())
    ca = CC._scale(torch.Generator().manual_seed(c.seed + 3), len(c.frames), c.C)
    k3 = CC.k3_reference(c.C, g1c.cpu(), ca, ops)
    g2, pool2 = k3_launch(lb, c, len(c.frames), dv(CC.planar(g1c.cpu())) if c.C == 64 else g1c, dv(ca), pk, True, tag + "_k3")
    try:
        chain_inside(rec, "k3", "g2", g2, *k3["g2"])
        chain_inside(rec, "k3", "pool", pool2, *k3["pool"])
    except AssertionError as e:
        failed.append(f"k3: {e}")
    REPORT.append(rec)
    assert not failed, failed
