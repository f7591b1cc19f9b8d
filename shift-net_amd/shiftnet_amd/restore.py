"""Restore a whole video: N frames in, N restored frames of the same size and pixel format out (single GPU).

Not part of the upstream API.  The programs under ``inference/test_*.py`` are upstream's evaluation harnesses (ground truth, dropped border
frames, crops); this is the path for footage.  Frames are planar Y'CbCr payloads as a Y4M stream carries them (shiftnet_amd/y4m.py); the
colour conversion, the padding to a legal size and the crop run on the device (csrc/sn_yuv.hip), so 1.5 bytes per pixel cross PCIe for
8-bit 4:2:0 and no float frame touches the host.

Windows: window k restores frames [k L, min((k + 1) L, N)) and feeds the network those plus 2 frames before and 2 after; frames before
0 and after N - 1 are reflected without repeating the edge (-1 -> 1, -2 -> 2, N -> N - 2), or clamped where N <= 2.
"""
from __future__ import annotations

import argparse
import queue
import sys
import threading
import time
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

PAST, FUTURE = 2, 2
VARIANTS = {"deblur": "gshift_deblur1", "deblur_small": "gshift_deblur2", "denoise": "gshift_denoise1", "denoise_small": "gshift_denoise2"}


# ---- the window planner (pure) ----------------------------------------------------------------------------------------------------
def reflect_index(i: int, n: int) -> int:
    """Frame index i of a clip of n frames: reflection about the first / last frame without repeating it; clamped where n <= 2."""
    if n <= 2:
        return min(max(i, 0), n - 1)
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    return min(max(i, 0), n - 1)


def window_indices(k: int, one_len: int, n: int, past: int = PAST, future: int = FUTURE) -> Tuple[int, int, List[int]]:
    """(first restored frame, number restored, the past + number + future input frame indices) of window k of a clip of n frames."""
    lo = k * one_len
    hi = min(lo + one_len, n)
    return lo, hi - lo, [reflect_index(i, n) for i in range(lo - past, hi + future)]


def plan_windows(n: int, one_len: int, past: int = PAST, future: int = FUTURE) -> List[Tuple[int, int, List[int]]]:
    if n < 1 or one_len < 1:
        raise ValueError(f"plan_windows: need n >= 1 and one_len >= 1, got {n}, {one_len}")
    return [window_indices(k, one_len, n, past, future) for k in range((n + one_len - 1) // one_len)]


def pad_multiple(topo: str) -> int:
    return 8 if topo == "plus" else 4


def padded_size(h: int, w: int, topo: str) -> Tuple[int, int]:
    m = pad_multiple(topo)
    return (h + m - 1) // m * m, (w + m - 1) // m * m


# ---- frame source: look-ahead over an iterator whose length is unknown until it ends ----------------------------------------------
class _Frames:
    def __init__(self, it: Iterable[np.ndarray]) -> None:
        self.it = iter(it)
        self.base = 0                     # index of buf[0]
        self.buf: List[np.ndarray] = []
        self.n: Optional[int] = None      # known once the iterator ends

    def _fill(self, upto: int) -> None:
        while self.n is None and self.base + len(self.buf) <= upto:
            try:
                self.buf.append(next(self.it))
            except StopIteration:
                self.n = self.base + len(self.buf)

    def window(self, k: int, one_len: int) -> Optional[Tuple[int, int, List[np.ndarray]]]:
        """The frames of window k, or None past the end.  Reads ahead as far as the window reaches."""
        self._fill((k + 1) * one_len + FUTURE - 1)
        n = self.n if self.n is not None else self.base + len(self.buf)      # not at the end: every index of the window is < frames read
        if n == 0 and k == 0:
            return None
        if k * one_len >= n:
            return None
        lo, cnt, idx = window_indices(k, one_len, n)
        frames = [self.buf[i - self.base] for i in idx]
        drop = max(0, (k + 1) * one_len - PAST - self.base)                  # the next window reaches back to (k + 1) L - PAST
        if drop > 0:
            del self.buf[:drop]
            self.base += drop
        return lo, cnt, frames


class _Thread(threading.Thread):
    """A producer thread: runs fn(put) and forwards its exception to the consumer of the queue."""
    END = object()

    def __init__(self, fn, depth: int) -> None:
        super().__init__(daemon=True)
        self.q: "queue.Queue" = queue.Queue(maxsize=depth)
        self.fn, self.stop = fn, threading.Event()

    def put(self, item) -> bool:
        while not self.stop.is_set():
            try:
                self.q.put(item, timeout=0.1)
                return True
            except queue.Full:
                pass
        return False

    def run(self) -> None:
        try:
            self.fn(self.put)
            self.put(self.END)
        except BaseException as e:      # noqa: BLE001 -- handed to the consumer, which raises it
            self.put(e)

    def __iter__(self):
        while True:
            item = self.q.get()
            if item is self.END:
                return
            if isinstance(item, BaseException):
                raise item
            yield item

    def close(self) -> None:
        self.stop.set()
        while self.is_alive():
            try:
                self.q.get_nowait()
            except queue.Empty:
                pass
            self.join(timeout=0.05)


# ---- the restorer -----------------------------------------------------------------------------------------------------------------
class VideoRestorer:
    """``VideoRestorer(net, one_len, sigma=None).restore(frames, fmt, height, width)`` -> iterator of restored payloads, one per input frame.

    net: a GShiftNet of shiftnet_amd.arch on a HIP device (eval mode, any dtype).  sigma: the noise level in 8-bit code values for the
    denoise variants (noise_map = sigma / 255 everywhere; no noise is added and the frame is not cut into quadrants).
    pipeline: read / copy / ingest window k + 1 on a side stream and copy back / hand out window k - 1 while window k runs; False runs
    the same steps one after the other.  Both give identical bytes."""

    def __init__(self, net, one_len: int, sigma: Optional[float] = None, pipeline: bool = True) -> None:
        import torch
        self.torch = torch
        self.net, self.one_len, self.pipeline = net, int(one_len), bool(pipeline)
        if self.one_len < 1:
            raise ValueError("one_len must be >= 1")
        self.V = net.V
        if self.V.denoise and sigma is None:
            raise ValueError("sigma is required by the denoise variants (the noise level of the footage, in 8-bit code values)")
        self.sigma = None if sigma is None else float(sigma)
        p = next(net.parameters())
        self.dev, self.dtype = p.device, p.dtype
        if self.dev.type != "cuda":
            raise ValueError("VideoRestorer needs the module on a HIP device")
        self.stats = {"frames": 0, "windows": 0, "forward_s": 0.0, "window_forward_ms": []}
        self._shape = None

    # -- per-shape state: two slots of staging and device buffers, sized for the largest window -------------------------------------
    def _prepare(self, fmt, h: int, w: int) -> None:
        torch = self.torch
        key = (fmt.bits, fmt.chroma, fmt.matrix, fmt.range, h, w)
        if self._shape == key:
            return
        self._shape = key
        self.fmt, self.h, self.w = fmt, h, w
        self.hp, self.wp = padded_size(h, w, self.V.topo)
        self.fb = fmt.frame_bytes(h, w)
        tin, tout = self.one_len + PAST + FUTURE, self.one_len
        dev = self.dev
        self.pin_in = [torch.empty((tin, self.fb), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.pin_out = [torch.empty((tout, self.fb), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev_in = [torch.empty((tin, self.fb), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.dev_out = [torch.empty((tout, self.fb), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.x = [torch.empty((1, tin, 3, self.hp, self.wp), dtype=self.dtype, device=dev) for _ in range(2)]
        half = self.dtype != torch.float32
        self.x32 = [torch.empty((1, tin, 3, self.hp, self.wp), dtype=torch.float32, device=dev) if half else None for _ in range(2)]
        self.s_in, self.s_out = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        ev = lambda: [torch.cuda.Event() for _ in range(2)]      # noqa: E731
        self.ev_h2d, self.ev_ready, self.ev_done, self.ev_d2h = ev(), ev(), ev(), ev()
        self.used = [False, False]

    # -- the steps of one window; slot = k % 2 -------------------------------------------------------------------------------------
    def _stage(self, slot: int, frames: Sequence[np.ndarray]) -> int:
        """Host frames -> pinned slot -> device -> RGB tensors, on the side stream."""
        from .io_edges import ingest_yuv
        torch = self.torch
        t = len(frames)
        if self.used[slot]:
            self.ev_h2d[slot].synchronize()                      # the copy that last read this pinned slot has finished
        pin = self.pin_in[slot].numpy()
        for i, f in enumerate(frames):
            pin[i] = f
        with torch.cuda.stream(self.s_in):
            if self.used[slot]:
                self.s_in.wait_event(self.ev_done[slot])         # the forward that last read this slot's tensors has finished
            self.dev_in[slot][:t].copy_(self.pin_in[slot][:t], non_blocking=True)
            self.ev_h2d[slot].record(self.s_in)
            ingest_yuv(self.dev_in[slot][:t], self.fmt, self.h, self.w, self.hp, self.wp, self.dtype, out=self.x[slot][:, :t])
            if self.x32[slot] is not None:
                ingest_yuv(self.dev_in[slot][:t], self.fmt, self.h, self.w, self.hp, self.wp, torch.float32, out=self.x32[slot][:, :t])
            self.ev_ready[slot].record(self.s_in)
        return t

    def _run(self, slot: int, t: int, main) -> int:
        """Forward + egress on the main stream, copy back on the output stream."""
        from .io_edges import egress_yuv
        torch = self.torch
        n = t - PAST - FUTURE
        with torch.cuda.stream(main), torch.no_grad():
            main.wait_event(self.ev_ready[slot])
            if self.used[slot]:
                main.wait_event(self.ev_d2h[slot])               # the copy that last read this slot's device payloads has finished
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(main)
            x = self.x[slot][:, :t]
            kw = {}
            if self.x32[slot] is not None:
                kw["shortcut"] = self.x32[slot][:, :t]
            if self.V.denoise:
                nm = torch.full((1, 1, 1, 1, 1), self.sigma / 255.0, dtype=self.dtype, device=self.dev).expand(1, t, 1, self.hp, self.wp)
                out = self.net.forward_fp32_out(x, nm, **kw)
            else:
                out = self.net.forward_fp32_out(x, **kw)
            e1.record(main)
            self._timers.append((e0, e1))
            egress_yuv(out, self.fmt, self.h, self.w, dst=self.dev_out[slot][:n])
            self.ev_done[slot].record(main)
        with torch.cuda.stream(self.s_out):
            self.s_out.wait_event(self.ev_done[slot])
            self.pin_out[slot][:n].copy_(self.dev_out[slot][:n], non_blocking=True)
            self.ev_d2h[slot].record(self.s_out)
        self.used[slot] = True
        return n

    def _collect(self, slot: int, n: int) -> List[np.ndarray]:
        self.ev_d2h[slot].synchronize()
        return list(self.pin_out[slot][:n].numpy().copy())

    def _finish_stats(self) -> None:
        ms = [a.elapsed_time(b) for a, b in self._timers]        # every event has completed: the last copy back has been waited for
        self.stats["window_forward_ms"] = ms
        self.stats["forward_s"] = sum(ms) / 1e3
        self.stats["windows"] = len(ms)

    # -- drivers -------------------------------------------------------------------------------------------------------------------
    def restore(self, frames: Iterable[np.ndarray], fmt, height: int, width: int) -> Iterator[np.ndarray]:
        """frames: iterable of uint8 payloads (``fmt.frame_bytes(height, width)`` each) -> the restored payloads, in order."""
        torch = self.torch
        self._prepare(fmt, height, width)
        self._timers: List = []
        self.used = [False, False]
        self.stats = {"frames": 0, "windows": 0, "forward_s": 0.0, "window_forward_ms": []}
        main = torch.cuda.current_stream(self.dev)

        def checked(it):
            for f in it:
                f = np.asarray(f, dtype=np.uint8).reshape(-1)
                if f.size != self.fb:
                    raise ValueError(f"frame payload of {f.size} bytes, the format and size say {self.fb}")
                yield f

        if not self.pipeline:
            src = _Frames(checked(frames))
            k = 0
            with torch.cuda.device(self.dev):
                while True:
                    win = src.window(k, self.one_len)
                    if win is None:
                        break
                    t = self._stage(k % 2, win[2])
                    n = self._run(k % 2, t, main)
                    for p in self._collect(k % 2, n):
                        self.stats["frames"] += 1
                        yield p
                    k += 1
                self._finish_stats()
            return

        # Three threads besides the kernels: the stager reads frames and brings window k + 1 onto the device (side stream), the forward
        # thread runs window k (its range-guard check waits for the device, so nothing else may depend on this thread), and the caller's
        # thread takes window k - 1 out of the pinned buffer.  Streams order the device work with events; the semaphores only say that
        # the event a stream is about to wait for HAS been recorded (in slots) and that a pinned output slot has been emptied (out slots).
        in_free = [threading.Semaphore(1), threading.Semaphore(1)]
        out_free = [threading.Semaphore(1), threading.Semaphore(1)]
        halt = threading.Event()

        def acquire(sem) -> bool:
            while not halt.is_set():
                if sem.acquire(timeout=0.1):
                    return True
            return False

        def stage_loop(put):
            src = _Frames(checked(frames))
            k = 0
            with torch.cuda.device(self.dev):
                while True:
                    win = src.window(k, self.one_len)
                    if win is None or not acquire(in_free[k % 2]):
                        return
                    if not put((k % 2, self._stage(k % 2, win[2]))):
                        return
                    k += 1

        stager = _Thread(stage_loop, depth=1)

        def forward_loop(put):
            with torch.cuda.device(self.dev):
                for slot, t in stager:
                    if not acquire(out_free[slot]):
                        return
                    n = self._run(slot, t, main)
                    in_free[slot].release()
                    if not put((slot, n)):
                        return

        worker = _Thread(forward_loop, depth=1)
        stager.start()
        worker.start()
        try:
            for slot, n in worker:
                payloads = self._collect(slot, n)
                out_free[slot].release()
                for p in payloads:
                    self.stats["frames"] += 1
                    yield p
            self._finish_stats()
        finally:
            halt.set()
            worker.close()
            stager.close()


# ---- command line -------------------------------------------------------------------------------------------------------------------
def make_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Restore a Y4M video with Shift-Net on the MI355X: same frames, size and pixel format out")
    ap.add_argument("--variant", choices=list(VARIANTS), required=True)
    ap.add_argument("--checkpoint", required=True, help="checkpoint path, or 'synthetic' for the deterministic synthetic weights")
    ap.add_argument("--dtype", choices=["fp32", "fp16", "bf16"], default="bf16")
    ap.add_argument("--one_len", type=int, default=16, help="frames restored per window")
    ap.add_argument("--sigma", type=float, default=None, help="noise level (8-bit code values), required by the denoise variants")
    ap.add_argument("--matrix", choices=["bt601", "bt709"], default=None, help="default: bt709 when H >= 720, else bt601")
    ap.add_argument("--range", choices=["limited", "full"], default=None, help="default: the stream's XCOLORRANGE, else limited")
    ap.add_argument("--no_pipeline", action="store_true", help="run read / copy / forward / write one after the other")
    ap.add_argument("input", metavar="IN", help="Y4M file, or - for stdin")
    ap.add_argument("output", metavar="OUT", help="Y4M file, or - for stdout")
    return ap


def load_net(variant: str, checkpoint: str, dtype: str, device="cuda"):
    import torch
    from .arch import CLASSES
    from .weights import synth_state_dict
    name = VARIANTS[variant]
    net = CLASSES[name](future_frames=FUTURE, past_frames=PAST)
    if checkpoint == "synthetic":
        net.load_state_dict(synth_state_dict(name), strict=True)
    else:
        net.load_state_dict(torch.load(checkpoint, map_location="cpu")["params"])
    dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[dtype]
    return net.to(dt).to(device).eval()


def main(argv: Optional[Sequence[str]] = None) -> int:
    from . import lib as L
    from .io_edges import yuv_fmt
    from .y4m import Y4MReader, Y4MWriter
    ap = make_parser()
    a = ap.parse_args(argv)
    if "denoise" in a.variant and a.sigma is None:
        ap.error("--sigma is required by the denoise variants")
    log = lambda s: (sys.stderr.write(s + "\n"), sys.stderr.flush())      # noqa: E731
    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    fout = sys.stdout.buffer if a.output == "-" else open(a.output, "wb")
    try:
        rd = Y4MReader(fin)
        hd = rd.header
        matrix = a.matrix or ("bt709" if hd.height >= 720 else "bt601")
        rng = a.range or (hd.color_range if hd.color_range in ("full", "limited") else "limited")
        log(f"input: {hd.width}x{hd.height} C{hd.chroma} F{hd.fps}; matrix {matrix}{'' if a.matrix else ' (default)'}, range {rng}"
            f"{'' if a.range else (' (stream)' if hd.color_range else ' (default)')}")
        fmt = yuv_fmt(hd.bits, hd.chroma_code, L.SN_YUV_BT709 if matrix == "bt709" else L.SN_YUV_BT601,
                      L.SN_YUV_FULL if rng == "full" else L.SN_YUV_LIMITED)
        net = load_net(a.variant, a.checkpoint, a.dtype)
        vr = VideoRestorer(net, a.one_len, sigma=a.sigma, pipeline=not a.no_pipeline)
        wr = Y4MWriter(fout, hd)
        t0 = time.perf_counter()
        n = 0
        for p in vr.restore(rd, fmt, hd.height, hd.width):
            wr.write(p)
            n += 1
            if n % max(a.one_len, 1) == 0:
                log(f"  {n} frames, {time.perf_counter() - t0:.1f} s")
        fout.flush()
        dt = time.perf_counter() - t0
        fwd = vr.stats["forward_s"]
        log(f"done: {n} frames in {dt:.2f} s, {n / dt if dt > 0 else 0.0:.2f} frames/s end to end, "
            f"{n / fwd if fwd > 0 else 0.0:.2f} frames/s forward only")
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
        if fout is not sys.stdout.buffer:
            fout.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
