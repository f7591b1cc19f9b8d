#!/usr/bin/env python3
"""Kernel-level A/B of the K4 fusion: sn_gsts_cab2_phase2 + sn_cab1_phase1 (two launches) against sn_cab2_phase2_cab1_phase1
(one), on the level-1 and level-2 shapes of config 2, both unit directions.  The two forms ALTERNATE over the rounds on one device (back-to-back
timings on this part differ by 10-15 % with their order); per form the minimum and the median over all rounds are printed.

    python tools/k4_fuse_ab.py [--rounds 6] [--reps 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from shiftnet_amd import lib as L, synth                    # noqa: E402
from shiftnet_amd.engine import Engine, Plan                # noqa: E402
from shiftnet_amd.spec import VARIANTS                      # noqa: E402
from shiftnet_amd.weights import synth_state_dict           # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = Engine(Plan(VARIANTS["gshift_deblur2"], synth_state_dict("gshift_deblur2"), dev))
    lib, st = eng.lib, torch.cuda.current_stream().cuda_stream
    blk, Cc = "stage1.decoder_level1.", 64
    lines = []
    for T, h, w in ((20, 360, 640), (20, 180, 320)):
        x = torch.from_numpy(synth.unit_noise((T, h, w, Cc), seed=1)).to(torch.bfloat16).to(dev)
        g2_in = torch.from_numpy(synth.unit_noise((T, h, w, Cc), seed=2)).to(torch.bfloat16).to(dev)
        ca = (0.5 + torch.rand((T, Cc), device=dev)).float()
        y, g2 = torch.empty_like(x), torch.empty_like(x)
        nblk = lib.sn_phase1_pool_blocks(T, h, w)
        pool = torch.empty((T, nblk, Cc), dtype=torch.float32, device=dev)
        ca_o = torch.empty((T, Cc), dtype=torch.float32, device=dev)
        tick = torch.zeros((T,), dtype=torch.int32, device=dev)
        for mode, unit in ((1, "encoder_level1."), (2, "encoder_level1_1.")):
            u2, u1, q = eng.P.units[blk + unit + "0."], eng.P.units[blk + unit + "1."], eng.P.cas[blk + unit + "1.ca2"]
            bias = u2["b_out"].data_ptr() if u2["b_out"] is not None else None
            src2 = L.UnitSrc(x.data_ptr(), T, h, w, Cc, mode, 1)
            src1 = L.UnitSrc(y.data_ptr(), T, h, w, Cc, 0, 0)
            se = L.SeFold(q["wa"].data_ptr(), q["wb"].data_ptr(), q["c"], q["cr"], tick.data_ptr(), ca_o.data_ptr(), None)
            wt = C.byref(u1["p1r"]["desc"])

            def two():
                L.check(lib.sn_gsts_cab2_phase2(C.byref(src2), g2_in.data_ptr(), ca.data_ptr(), u2["w_out"].data_ptr(), bias, y.data_ptr(), st), "K4")
                L.check(lib.sn_cab1_phase1(C.byref(src1), wt, g2.data_ptr(), pool.data_ptr(), C.byref(se), None, st), "phase 1")

            def one():
                L.check(lib.sn_cab2_phase2_cab1_phase1(C.byref(src2), g2_in.data_ptr(), ca.data_ptr(), u2["w_out"].data_ptr(), bias, y.data_ptr(), wt, g2.data_ptr(),
                                                       pool.data_ptr(), C.byref(se), None, st), "fused")
            t = {"two": [], "one": []}
            for f in (two, one):
                f()
            torch.cuda.synchronize()
            for r in range(a.rounds):
                for name, f in ((("two", two), ("one", one)) if r % 2 == 0 else (("one", one), ("two", two))):
                    for _ in range(a.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(); f(); e1.record()
                        torch.cuda.synchronize()
                        t[name].append(e0.elapsed_time(e1) * 1e3)
            ln = (f"{T}x{h}x{w} mode {mode}: K4 + phase 1 min {min(t['two']):.1f} median {statistics.median(t['two']):.1f} us | fused min {min(t['one']):.1f} "
                  f"median {statistics.median(t['one']):.1f} us | saved (medians) {statistics.median(t['two']) - statistics.median(t['one']):.1f} us  "
                  f"({a.rounds} alternating rounds x {a.reps})")
            print(ln, flush=True)
            lines.append(ln)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
