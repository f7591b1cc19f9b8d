"""-m gpu: the fused phase 1 (csrc/sn_phase1r.hip: sn_gsts_cab2_phase1, sn_cab1_phase1) through the C ABI inside the float64 INTERVALS of
tests/phase1_cases.py, element by element.

tests/test_gpu_parity.py::test_cab_phase1_fused_kernel bounds this kernel at 1.2e-2 of the tensor's peak against an fp32 oracle that rounds nothing
where the kernel rounds, on unit-variance noise, and sees the pool only as the sum of its rows: a wrong halo column at a strip seam, one dropped
RepConv corner tap or a pool row that counts a seam pixel twice all stay inside.  Here every row of the case table gets, per element, the interval
[lo, hi] of a reference that models each of the kernel's roundings (tests/test_host_phase1_ref.py holds that reference against the oracle, the
packed weights, point emulations and one-fault controls): every g2 element is written and lo <= got <= hi, every pool row is inside its interval
sum, row by row; outputs live in guarded buffers (NaN prefill), frames outside a frame range keep their NaN, every team size a row lists is
bit-identical to the library's own, the denoisers' two passes run without and with the g1 store, and the squeeze-excite fold is held against
sigmoid(wb relu(wa mean)) in float64 of the pool rows the kernel itself wrote.  Per case the share of elements at an interval end, the width
statistics and -- if an element is outside -- its position and the interval of every stage there (phase1_cases.stage_intervals) go to
parity_report_phase1_edges.json in $SN_PARITY_REPORT_DIR (default: parity_out/ at the repository root).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import phase1_cases as PC
from test_gpu_bf16_conv_kernels import guarded, guards_intact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REPORT = []
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
U = PC.U


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    d = os.environ.get("SN_PARITY_REPORT_DIR") or os.path.join(ROOT, "parity_out")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "parity_report_phase1_edges.json"), "w") as f:
        json.dump(REPORT, f, indent=1)


@pytest.fixture(scope="module")
def lib():
    from shiftnet_amd import lib as L
    return L.load(), L


def stream():
    return torch.cuda.current_stream().cuda_stream


class Dev:
    """one row's operands on the device and its launches"""

    def __init__(self, c, ops, lb, L):
        self.c, self.lb, self.L = c, lb, L
        dv = lambda t: t.contiguous().to(DEV) if t is not None else None      # noqa: E731
        self.x, self.halo, self.hw, self.scale = dv(ops["x"]), dv(ops["halo"]), dv(ops["hw"]), dv(ops["g1_scale"])
        self.pk = {k: dv(v) for k, v in PC.packed(ops).items()}
        self.wt = L.Phase1Weights(*(self.pk[k].data_ptr() for k in ("wfrag1", "w3", "wgrp", "wfrag2")))
        self.src = L.UnitSrc(self.x.data_ptr(), c.T, c.h, c.w, c.C, c.mode, c.wrap, self.halo.data_ptr() if self.halo is not None else None, c.t0, c.nt, c.clip)
        self.nblk = lb.sn_phase1_pool_blocks(c.T, c.h, c.w)
        assert self.nblk >= 1

    def launch(self, tag, team=0, g2=True, sums=False, scale=False, store=None, se=None):
        """-> (g2 view or None, pool view): guarded NaN buffers, guards checked"""
        c, L = self.c, self.L
        gb, gv = guarded((c.T, c.h, c.w, c.C), torch.bfloat16, NAN) if g2 else (None, None)
        pb, pv = guarded((c.T, self.nblk, c.C), torch.float32, NAN)
        opt = L.Phase1Opts(self.scale.data_ptr() if scale else None, 1 if sums else 0, team, store.data_ptr() if store is not None else None)
        rc = L.cab_phase1(self.lb, self.src, self.hw.data_ptr() if self.hw is not None else None, self.wt, gv.data_ptr() if g2 else None, pv.data_ptr(), stream(), se, opt)
        assert rc == 0, (c.id, tag, rc)
        torch.cuda.synchronize()
        assert guards_intact(pb, NAN) and (gb is None or guards_intact(gb, NAN)), f"{c.id}:{tag}: wrote outside its output"
        f = c.frames
        for v in (gv, pv):
            if v is not None:
                assert bool(torch.isnan(v[:f.start].float()).all()) and bool(torch.isnan(v[f.stop:].float()).all()), f"{c.id}:{tag}: wrote a frame outside [{f.start}, {f.stop})"
        return gv, pv

    def g1_store(self):
        n = ctypes.c_longlong(0)
        assert self.lb.sn_phase1_g1_store_bytes(self.c.T, self.c.h, self.c.w, self.c.C, ctypes.byref(n)) == 0 and n.value > 0
        return torch.full((n.value // 2,), NAN, dtype=torch.float16, device=DEV)      # NaN: a row the second pass reads but the first did not write would show


def inside(c, ops, rec, tag, what, got, lo, hi, keep16=False):
    """every element written and inside its interval; the record gets the share at an interval end, or the worst element and its stages (keep16: the
    stages' intervals that take fp16 subnormals as kept, for tests/test_gpu_phase1_gauge.py)"""
    got = got.double().cpu().numpy()
    assert got.shape == lo.shape, (c.id, tag, what, got.shape, lo.shape)
    out = PC.outside(got, lo, hi)
    r = rec.setdefault(tag, {})
    r[what] = dict(at_an_end=float(((got == lo) | (got == hi)).mean()), outside=int(out.sum()), elements=int(out.size), unwritten=int(np.isnan(got).sum()))
    if out.any():
        peak = max(np.abs(lo).max(), np.abs(hi).max())
        ex = np.where(out, np.maximum(lo - got, got - hi), 0.0)
        ex[np.isnan(got)] = np.inf
        i = np.unravel_index(int(np.argmax(ex)), ex.shape)
        r[what]["worst"] = dict(index=[int(k) for k in i], got=float(got[i]), lo=float(lo[i]), hi=float(hi[i]), excess_over_peak=float(ex[i] / peak))
        if what == "g2":
            t, y, x = c.frames.start + i[0], i[1], i[2]
            r[what]["worst"]["stages"] = {k: [v[0].tolist(), v[1].tolist()] for k, v in PC.stage_intervals(c, t, y, x, ops, keep16).items()}
        REPORT.append(dict(rec))
        raise AssertionError(f"{c.id}:{tag}: {int(out.sum())} of {out.size} {what} elements outside their interval ({int(np.isnan(got).sum())} not written); "
                             f"worst {r[what]['worst']['index']}: got {got[i]:.9g}, interval [{lo[i]:.9g}, {hi[i]:.9g}]")


def se_check(c, rec, pool, ca, wa, wb):
    """ca[t] = sigmoid(wb relu(wa mean)), mean = (sum of the frame's pool rows) / (h w), in float64 from the rows the kernel wrote.  Bound: the
    three fp32 sums (nrows rows, c and cr products) against the chain of absolute values M, through the sigmoid's slope <= 1/4, plus exp (1 ulp,
    and its argument's scaling: |o| ulps), the addition and rcp (1 ulp)."""
    p = pool.double().cpu().numpy()
    got = ca.double().cpu().numpy()
    A, B = wa.double().cpu().numpy(), wb.double().cpu().numpy()
    inv = float(np.float32(1.0) / (np.float32(c.h) * np.float32(c.w)))
    nrows, cr = p.shape[1], A.shape[0]
    worst = 0.0
    for t in c.frames:
        mean, mabs = p[t].sum(0) * inv, np.abs(p[t]).sum(0) * inv
        hid = np.maximum(A @ mean, 0.0)
        o = B @ hid
        M = np.abs(B) @ (np.abs(A) @ mabs)
        ref = 1.0 / (1.0 + np.exp(-o))
        tol = 0.25 * (nrows + c.C + cr + 8) * U * M + ref * (3.0 + np.abs(o)) * 2.0 ** -23
        err = np.abs(got[t] - ref)
        assert np.isfinite(got[t]).all() and (err <= tol).all(), (c.id, t, float((err / tol).max()))
        worst = max(worst, float((err / tol).max()))
    rec["se_fold_max_err_over_tol"] = worst


@pytest.mark.parametrize("case", PC.CASES, ids=[c.id for c in PC.CASES])
def test_phase1_inside_the_intervals(case, lib):
    lb, L = lib
    c = case
    ops = PC.operands(c)
    ref = PC.reference(c, ops, want=("g2", "v", "g1") if c.kind != "plan" else ("g2", "v"))
    bounds = PC.strip_bounds(lb, c.w)
    fr = slice(c.frames.start, c.frames.stop)
    ar = PC.Arith("interval")
    rec = dict(test="phase1", id=c.id, shape=[c.T, c.h, c.w, c.C], mode=c.mode, wrap=c.wrap, clip=c.clip, frames=[fr.start, fr.stop], kind=c.kind,
               strips=bounds, widths=PC.width_stats(*ref["g2"]))
    d = Dev(c, ops, lb, L)
    assert d.nblk == (len(bounds) - 1) * -(-c.h // PC.P1R_RB)
    if c.kind == "sums":
        slo, shi = PC.pool_rows(ar, (16.0 * ref["g1"][0], 16.0 * ref["g1"][1]), bounds)
        _, pool = d.launch("sums", g2=False, sums=True)
        inside(c, ops, rec, "sums", "g1_pool", pool[fr], slo, shi)
        _, pool_s = d.launch("sums_store", g2=False, sums=True, store=d.g1_store())
        assert torch.equal(pool_s[fr], pool[fr]), c.id
        REPORT.append(rec)
        return
    plo, phi = PC.pool_rows(ar, ref["v"], bounds)
    if c.kind == "scale":
        g2, pool = d.launch("scale", scale=True)
        inside(c, ops, rec, "scale", "g2", g2[fr], *ref["g2"])
        inside(c, ops, rec, "scale", "pool", pool[fr], plo, phi)
        store = d.g1_store()
        d.launch("sums_store", g2=False, sums=True, store=store)
        g2_s, pool_s = d.launch("scale_store", scale=True, store=store)
        assert torch.equal(g2_s[fr].view(torch.int16), g2[fr].view(torch.int16)) and torch.equal(pool_s[fr], pool[fr]), c.id
        REPORT.append(rec)
        return
    teams = (0,) + c.teams
    if c.kind == "plan":                    # the row exists for a chunk that crosses a strip end with at least two row blocks per team: on THIS device?
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        o = (ctypes.c_int * 7)()
        assert lb.sn_p1r_plan(len(c.frames), c.h, c.w, ncu, 0, o) == 0
        nbh = -(-c.h // PC.P1R_RB)
        blocks = o[0] * o[4] * nbh
        cross = any((t * o[5]) // nbh != (min(t * o[5] + o[5], blocks) - 1) // nbh for t in range(o[6]))
        rec["plan"] = dict(ncu=ncu, plan=list(o), two_row_blocks=o[5] >= 2, crosses=cross)
        if not (o[5] >= 2 and cross):
            rec["plan"]["note"] = "this device's plan has no chunk that crosses a strip end: team 1 run as well"
            teams = (0, 1)
    se = tickets = ca = None
    if c.se:
        g = torch.Generator().manual_seed(c.seed + 1)
        cr = c.C // 8
        wa = (torch.randn((cr, c.C), generator=g) / c.C ** 0.5).float().to(DEV)
        wb = (torch.randn((c.C, cr), generator=g) / cr ** 0.5 * 4.0).float().to(DEV)
        tickets = torch.zeros((c.T,), dtype=torch.int32, device=DEV)
        cab, ca = guarded((c.T, c.C), torch.float32, NAN)
        se = L.SeFold(wa.data_ptr(), wb.data_ptr(), c.C, cr, tickets.data_ptr(), ca.data_ptr(), None)
    first = None
    for team in teams:
        tag = f"team{team}"
        g2, pool = d.launch(tag, team=team, se=se if team == 0 else None)
        inside(c, ops, rec, tag, "g2", g2[fr], *ref["g2"])
        inside(c, ops, rec, tag, "pool", pool[fr], plo, phi)
        if team == 0 and c.se:
            assert guards_intact(cab, NAN) and int(tickets.abs().sum()) == 0, c.id
            se_check(c, rec, pool, ca, wa, wb)
        if first is None:
            first = (g2, pool)
        else:
            assert torch.equal(g2[fr].view(torch.int16), first[0][fr].view(torch.int16)) and torch.equal(pool[fr], first[1][fr]), (c.id, tag)
    REPORT.append(rec)
