#!/usr/bin/env python3
"""Sequential vs batched forward (GShiftNet.forward_clips), A/B in one process on one device.

  (a) config 4's window: Shift-Net+ denoiser, 852 x 480, 36 input frames, the CLI's four overlapping quadrants (cli.quadrant_forward) as four
      forwards against one batched forward, bf16 and fp32 modules;
  (b) a small-clip serving case: Shift-Net-s deblur, 256 x 256, 20 input frames, B = 8 clips as eight forwards against one batched forward;
  (c) the peak device memory of each form (torch.cuda.max_memory_allocated above what was allocated before the call).

The two forms alternate repeat by repeat, each timed with device events around the whole form and a synchronisation after it; the line per
case gives median, min and max over the repeats.  Weights are synthetic (timing does not depend on their values).

    python tools/batch_ab.py [--repeats 7] [--cases a,b] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "shift-net_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from shiftnet_amd import cli  # noqa: E402
from shiftnet_amd.arch import CLASSES  # noqa: E402
from shiftnet_amd.weights import synth_state_dict  # noqa: E402

DEV = "cuda:0"


def make_net(name, dtype):
    net = CLASSES[name](future_frames=2, past_frames=2)          # as the CLIs build it
    net.load_state_dict(synth_state_dict(name), strict=True)
    return net.to(dtype).to(DEV).eval()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def peak_mib(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def ab(label, seq, bat, repeats, frames):
    for f in (seq, bat):               # warm-up: plans, allocator pools, captured graphs where the engine takes them
        f()
        f()
    ts, tb = [], []
    for _ in range(repeats):
        ts.append(timed(seq))
        tb.append(timed(bat))
    ms, mb = peak_mib(seq), peak_mib(bat)
    r = {"case": label, "restored_frames": frames, "repeats": repeats,
         "sequential_ms": {"median": statistics.median(ts), "min": min(ts), "max": max(ts)},
         "batched_ms": {"median": statistics.median(tb), "min": min(tb), "max": max(tb)},
         "speedup_median": statistics.median(ts) / statistics.median(tb),
         "peak_mib": {"sequential": ms, "batched": mb}}
    print(f"{label}: sequential {r['sequential_ms']['median']:.2f} ms [{min(ts):.2f}, {max(ts):.2f}]  batched {r['batched_ms']['median']:.2f} ms "
          f"[{min(tb):.2f}, {max(tb):.2f}]  -> x{r['speedup_median']:.3f}   peak memory {ms:.0f} / {mb:.0f} MiB", flush=True)
    return r


def case_a(dtype, repeats):
    net = make_net("gshift_denoise1", dtype)
    N, H, W, sigma = 36, 480, 852, 30 / 255.0
    g = torch.Generator().manual_seed(0)
    x32 = (torch.rand((1, N, 3, H, W), generator=g) + torch.randn((1, N, 3, H, W), generator=g) * sigma).to(DEV)
    x = x32.to(dtype)

    def seq():
        return cli.quadrant_forward(net, x, sigma, on_device=True, x32=x32)

    def bat():
        return cli.quadrant_forward(net, x, sigma, on_device=True, x32=x32, batch=True)
    assert torch.equal(seq(), bat())
    return ab(f"(a) config-4 window, 4 quadrants, {str(dtype).split('.')[-1]}", seq, bat, repeats, N - 4)


def case_b(repeats):
    net = make_net("gshift_deblur2", torch.bfloat16)
    B, T, H, W = 8, 20, 256, 256
    x = torch.rand((B, T, 3, H, W), generator=torch.Generator().manual_seed(1)).to(torch.bfloat16).to(DEV)

    def seq():
        return [net(x[b:b + 1]) for b in range(B)]

    def bat():
        return net.forward_clips(x)
    assert torch.equal(torch.stack(seq()), bat())
    return ab(f"(b) Shift-Net-s {H}x{W} T_in {T}, B = {B}, bf16", seq, bat, repeats, B * (T - 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = []
    with torch.no_grad():
        if "a" in a.cases.split(","):
            res.append(case_a(torch.bfloat16, a.repeats))
            res.append(case_a(torch.float32, a.repeats))
        if "b" in a.cases.split(","):
            res.append(case_b(a.repeats))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
