"""GShiftNet.forward as a straight-line sequence of operator calls on torch's current HIP stream (one process = one GPU = one clip window):
the control flow that ``engine.Engine`` (bf16 storage) and ``engine32.Engine32`` (fp32) share.  It mirrors the reference forward of each variant
(file:line cited per method) so parity can be audited line by line against ``oracle/shiftnet_oracle.py``, and it names no kernel but the
squeeze-excite MLP, which is fp32 in both engines: each engine brings every other operator itself and inherits nothing from the other one.
"""
from __future__ import annotations

import contextlib
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from . import lib as L
from .spec import UNIT_NAMES


@dataclass
class Act:
    """NHWC activation (bf16, or fp32 in Engine32): t [T,H,W,Cs] with c logical channels (pad channels are zero)."""
    t: torch.Tensor
    c: int

    @property
    def dims(self) -> Tuple[int, int, int, int]:
        return tuple(self.t.shape)  # type: ignore[return-value]


def _dtype_code(dt: torch.dtype) -> int:
    return {torch.float32: L.SN_F32, torch.float16: L.SN_F16, torch.bfloat16: L.SN_BF16}[dt]


class Network:
    """The forward pass over operators a subclass supplies: conv, cab, temporal_roll, naf, _ingest and act_dtype.  gsts_unit, _shift_chain and
    skip_up below are the reference's form of the operators that the bf16 engine specialises."""
    # bench.py assigns and reads these on the engine of either dtype; only the bf16 Engine reads the environment and acts on them
    schedule, frame_group, stream_groups = "unit", 4, 2

    def __init__(self, plan, dtype: Optional[torch.dtype] = None, graph_auto: bool = False) -> None:
        self.P = plan
        self.dtype = dtype or self.act_dtype
        self.V = plan.V
        self.lib = L.load()
        self.dev = plan.device
        self.prof: Optional[list] = None      # bench.py attaches a list to collect (fn, label, meta, ev0, ev1)
        self._meta: Tuple = ()
        self._unit: Optional[Tuple] = None    # (T, h, w, c, mode) while the launches of a CAB2 / CAB1 of a GSTS unit are being issued
        self.split = None                     # temporal_split.TemporalSplit: this engine holds a frame range of a longer window
        self._side = None                     # side stream of the halo exchanges (created on first use)
        self._clip = 0                        # frames per clip while a batch of clips is being issued (forward_clips); 0: one clip
        # hipGraph replay of the whole forward (~1400 launches per window): the first call with a given input signature runs eagerly, the second
        # one is captured, later ones replay, so the Python / ctypes / allocator work per launch disappears.  Measured on MI355X: neutral at
        # 1280x720 (126.4 vs 126.0 ms per window: the GPU is never starved there, kernels average 90 us), 1.39x on a 64x96 clip where the ~10 us
        # squeeze-excite kernels dominate the launch stream.  SN_GRAPH=1: always, 0: never, default: windows below GRAPH_AUTO_PXF pixel-frames.
        g = os.environ.get("SN_GRAPH", "auto")
        self.use_graph = g == "1"
        self.graph_auto = graph_auto and g not in ("0", "1")         # replay by size is the bf16 engine's choice: measured there only
        self._graphs: "OrderedDict[Tuple, object]" = OrderedDict()   # LRU over input signatures, at most GRAPH_SLOTS captured graphs alive

    # ---- low level wrappers --------------------------------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _call(self, fn: str, label: str, *args) -> None:
        """One C-ABI launch on the current stream; with a profiler attached, bracketed by stream events."""
        f = getattr(self.lib, fn)
        if self.prof is None:
            L.check(f(*args), label)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(f(*args), label)
        e1.record()
        meta = self._meta
        if self._unit is not None and not (meta and meta[0] == "naf"):       # a kernel of the unit with its own meta (the fp32 engine's operators)
            meta = tuple(meta) + ("unit",) + self._unit
        self.prof.append((fn, label, meta, e0, e1))

    def _new(self, T: int, h: int, w: int, cs: int) -> torch.Tensor:
        return torch.empty((T, h, w, cs), dtype=self.act_dtype, device=self.dev)

    def ca_mlp(self, name: str, pool: torch.Tensor, npix: int, *, out: Optional[torch.Tensor] = None, frames: Optional[Tuple[int, int]] = None, guard: Optional[int] = None) -> torch.Tensor:
        """Squeeze-excite MLP: partial channel sums pool [T][nblk][cpad] -> scales [T][cpad] in `out` (or a new tensor), of `frames` = (f0, n) only if given."""
        p = self.P.cas[name]
        T, nblk, cpad = pool.shape
        ca = out if out is not None else torch.empty((T, cpad), dtype=torch.float32, device=self.dev)
        f0, n = frames if frames is not None else (0, T)
        self._call("sn_ca_mlp", f"sn_ca_mlp[{name}]", pool.data_ptr() + f0 * nblk * cpad * 4, nblk, cpad, p["c"], p["cr"], 1.0 / npix, p["wa"].data_ptr(),
                   p["wb"].data_ptr(), ca.data_ptr() + f0 * cpad * 4, n, guard, self._stream())
        return ca

    def _wrap_flag(self, mode: int, circular: bool) -> int:
        """sn_unit_src.wrap: 0 keep the window's boundary frame, 1 circular, 2 the neighbour frame's half arrives from the adjacent rank."""
        if self.split is not None and mode:
            return self.split.wrap_flag(mode, circular)
        return 1 if circular else 0

    def _unit_src(self, x: Act, mode: int, *, wrap: Optional[int] = None, halo: Optional[torch.Tensor] = None, t0: int = 0, nt: int = 0) -> L.UnitSrc:
        T, h, w, cs = x.dims
        assert cs == x.c
        wrap = self._wrap_flag(mode, self.V.wrap) if wrap is None else wrap
        return L.UnitSrc(x.t.data_ptr(), T, h, w, x.c, mode, wrap, halo.data_ptr() if halo is not None else None, t0, nt, self._clip)

    def _split_pieces(self, x: Act, mode: int, circular: bool):
        """Launch plan of a shifted operator on a temporally split window (temporal_split.py): [(wrap, halo, t0, nt), ...].

        Without a split (or where this rank has no neighbour on the borrowing side): one piece, all frames.  Otherwise the frames that
        need no halo are launched FIRST, on the compute stream; the halo exchange runs meanwhile on the engine's side stream (it waits
        only for the producer of x), and the boundary frame -- the only one that reads the neighbour's half -- follows once it arrived."""
        T = x.dims[0]
        flag = self._wrap_flag(mode, circular)
        if self.split is None:
            yield (flag, None, 0, 0)
            return
        main = torch.cuda.current_stream(self.dev)
        ready = main.record_event()                       # x is complete here (stream order)
        recv = flag == 2                                  # this rank's boundary frame borrows from a neighbour rank
        bt = 0 if mode == 1 else T - 1
        if recv and T > 1:
            yield (0, None, 1 if mode == 1 else 0, T - 1)  # the boundary frame is outside the range, so its rule does not matter
        if self._side is None:
            self._side = torch.cuda.Stream(self.dev)
        with torch.cuda.stream(self._side):               # every rank takes part: one that receives nothing may still have to send
            self._side.wait_event(ready)
            x.t.record_stream(self._side)
            halo = self.split.exchange(x.t, mode, circular)
        if recv:
            main.wait_stream(self._side)
            halo.record_stream(main)
            yield (2, halo, bt, 1)
        else:
            yield (flag, None, 0, 0)

    def shift_cab(self, pre: str, x: Act, reverse: bool) -> Act:
        """Shift_CAB (gshift_denoise1.py:157-186)."""
        return self.cab(pre, self.temporal_roll(x, reverse))

    def gsts_unit(self, pre: str, x: Act, reverse: bool) -> Act:
        """CAB2 (pre + "0.", on the GSTS gather of x) then CAB1 (pre + "1.")."""
        return self.naf(pre + "1.", self.naf(pre + "0.", x, 2 if reverse else 1), 0)

    def shift_block(self, pre: str, x: Act) -> Act:
        """Encoder_shift_block.forward (gshift_deblur1.py:530-547 / gshift_deblur2.py:521-530)."""
        for i in range(self.V.units):
            x = self.gsts_unit(f"{pre}{UNIT_NAMES[i]}.", x, reverse=(i % 2 == 1))
        return x

    def shift_chain(self, pres: Sequence[str], x: Act) -> Act:
        """Consecutive Encoder_shift_blocks at one level (Encoder2.forward, gshift_deblur1.py:623-637 / gshift_deblur2.py:594-609)."""
        ev = None
        if self.prof is not None:             # wall time of the whole chain on the launching stream (bench.py: GSTS time of the window under any schedule)
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        y = self._shift_chain(pres, x)
        if ev is not None:
            ev[1].record()
            self.prof.append(("gsts_chain", "gsts_chain", ("chain",) + tuple(x.dims) + (len(pres) * self.V.units,), ev[0], ev[1]))
        return y

    def _shift_chain(self, pres: Sequence[str], x: Act) -> Act:
        for pre in pres:
            x = self.shift_block(pre, x)
        return x

    def down(self, pre: str, x: Act) -> Act:
        """DownSample (gshift_deblur1.py:330-340 / gshift_denoise1.py:356-365)."""
        if self.V.denoise:
            return self.conv(pre + "down", [x], stride=2, prelu=self.P.scalar(pre + "down.1.weight"))
        return self.conv(pre + "down", [x], stride=2)

    def skip_up(self, name: str, x: Act, y: Act) -> Act:
        """SkipUpSample: bilinear x2 -> 1x1 -> + y (gshift_deblur1.py:341-350)."""
        return self.conv(name, [x], in_mode=1, res=y)

    def tfr_unet(self, pre: str, x: Act, extra: Optional[Act] = None) -> Act:
        """TFR_UNet.forward (gshift_deblur1.py:709-722).  `extra` is added to the result in the epilogue of the last CAB's
        second conv: the "+ shortcut" that follows the last orb / rorb (:769,779) costs no pass of its own."""
        def seq(nm: str, n: int, t: Act, ex: Optional[Act] = None) -> Act:
            for i in range(n):
                t = self.cab(f"{pre}{nm}.{i}.", t, ex if i == n - 1 else None)
            return t
        enc1 = seq("encoder_level1", 1, x)
        enc2 = seq("encoder_level2", 3, self.down(pre + "down12.", enc1))
        enc3 = seq("encoder_level3", 3, self.down(pre + "down23.", enc2))
        dec3 = seq("decoder_level3", 3, enc3)
        t = self.skip_up(pre + "up32", dec3, self.cab(pre + "skip_attn2.", enc2))
        dec2 = seq("decoder_level2", 3, t)
        t = self.skip_up(pre + "up21", dec2, self.cab(pre + "skip_attn1.", enc1))
        return seq("decoder_level1", 1, t, extra)

    def stage1(self, x: Act) -> Act:
        """Encoder2.forward (gshift_deblur1.py:613-642, gshift_deblur2.py:587-613, gshift_denoise1.py:640-670)."""
        V, p = self.V, "stage1."
        x = self.cab(p + "concat.", x)
        shortcut = x
        if V.shift_cab:
            x = self.shift_cab(p + "encoder_level0.", x, False)
            x = self.shift_cab(p + "encoder_level0_1.", x, True)
        x = self.conv(p + "down01", [x], stride=2, pad=0, prelu=self.P.scalar(p + "down01.1.weight"))
        if V.topo == "small":
            enc11 = self.shift_chain([p + "encoder_level1.", p + "encoder_level1_1.", p + "encoder_level1_2."], x)
            e = self.down(p + "down12.", enc11)
            e = self.shift_chain([f"{p}{n}." for n in ("encoder_level2", "encoder_level2_1", "encoder_level2_2",
                                                       "decoder_level2", "decoder_level2_1", "decoder_level2_2")], e)
            x = self.skip_up(p + "up21", e, self.cab(p + "skip_attn1.", enc11))
        else:
            if V.shift_cab:
                e = self.shift_cab(p + "encoder_level1.", x, False)
                enc11 = self.shift_cab(p + "encoder_level1_1.", e, True)
            else:
                enc11 = self.cab(p + "encoder_level1_1.", self.cab(p + "encoder_level1.", x))
            e = self.down(p + "down12.", enc11)
            enc22 = self.cab(p + "encoder_level2_1.", self.cab(p + "encoder_level2.", e))
            e = self.down(p + "down23.", enc22)
            enc33 = self.cab(p + "encoder_level3_1.", self.cab(p + "encoder_level3.", e))
            d = self.shift_chain([p + "decoder_level3.", p + "decoder_level3_1."], enc33)
            x = self.skip_up(p + "up32", d, self.cab(p + "skip_attn2.", enc22))
            d = self.shift_chain([p + "decoder_level2.", p + "decoder_level2_1."], x)
            x = self.skip_up(p + "up21", d, self.cab(p + "skip_attn1.", enc11))
        dec11 = self.shift_chain([p + "decoder_level1.", p + "decoder_level1_1.", p + "decoder_level1_2."], x)
        skip = self.cab(p + "skip_conv.", shortcut)
        if V.hr_cat:
            up = self.conv(p + "upsample0", [dec11], out_mode=1)
            out = self.conv(p + "conv_hr0", [up, skip])
        else:   # conv_hr0(act(upsample0(x))) + skip: the PReLU commutes with pixel_shuffle, so it is the conv epilogue
            up = self.conv(p + "upsample0", [dec11], out_mode=1, prelu=self.P.scalar(p + "act.weight"))
            out = self.conv(p + "conv_hr0", [up], res=skip)
        return self.cab(p + "out_conv.", out)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, noise_map: Optional[torch.Tensor], past: int, future: int,
                out_dtype: Optional[torch.dtype] = None, shortcut: Optional[torch.Tensor] = None) -> torch.Tensor:
        """GShiftNet.forward; x:[T,C,H,W] (already x[0]) on this engine's device, any of fp32/fp16/bf16.  out_dtype (default: x.dtype, the
        module contract) = torch.float32 returns the restored frames from conv_last's fp32 accumulators without the rounding to a
        half-precision image tensor: the CLIs' metrics / PNG path (inference/test_deblur.py:137-143 converts with .float() anyway).
        shortcut: optional [T,3,H,W] tensor added instead of x in "return output_features + shortcut[...]" (gshift_deblur1.py:791): the
        un-rounded float32 frames when x had to be rounded to a half-precision module dtype."""
        with torch.cuda.device(self.dev):      # launches, events and allocations all belong to the engine's device
            graphed = self.use_graph or (self.graph_auto and x.shape[0] * x.shape[2] * x.shape[3] <= self.GRAPH_AUTO_PXF)
            eager = (not graphed or self.split is not None or self.prof is not None or out_dtype is not None or shortcut is not None
                     or torch.cuda.is_current_stream_capturing())
            rerun = lambda: self._forward(x, noise_map, past, future, out_dtype, shortcut)      # noqa: E731
            return self._checked(rerun if eager else lambda: self._forward_graphed(x, noise_map, past, future), rerun, int(x.shape[0]))

    @torch.no_grad()
    def forward_clips(self, x: torch.Tensor, noise_map: Optional[torch.Tensor], past: int, future: int,
                      out_dtype: Optional[torch.dtype] = None, shortcut: Optional[torch.Tensor] = None) -> torch.Tensor:
        """B independent clips of the same shape in one set of launches: x:[B,T,C,H,W] -> [B, T-past-future, 3, H, W], clip b bit-identical
        to forward(x[b], ...).  The batch runs as B*T frames: the shift units apply their neighbour rule inside each clip (sn_unit_src.clip),
        rconcat reads each clip's kept frames [past, T-future) in place (the conv remap), every other operator is per frame.
        noise_map: [B,T,1,H,W] or broadcastable to it; shortcut: [B,T,3,H,W] as in forward.  One range-guard check (and at most one recovery)
        covers the whole batch.  Not combinable with a temporal split (ValueError); SN_SCHEDULE=frame / streams run the plain unit schedule here."""
        if self.split is not None:
            raise ValueError("forward_clips cannot be combined with a temporal split (set_temporal_split)")
        if x.dim() != 5:
            raise ValueError(f"forward_clips expects x:[B,T,C,H,W], got {tuple(x.shape)}")
        B, T, cin, H, W = x.shape
        xf = x.reshape(B * T, cin, H, W)
        nm = noise_map.expand(B, T, 1, H, W).reshape(B * T, 1, H, W) if noise_map is not None else None
        sc = None
        if shortcut is not None:
            assert shortcut.dim() == 5 and tuple(shortcut.shape[:2]) == (B, T), tuple(shortcut.shape)
            sc = shortcut.reshape(B * T, *shortcut.shape[2:])
        n_out = max(T - past - future, 0)
        with torch.cuda.device(self.dev):
            graphed = self.use_graph or (self.graph_auto and B * T * H * W <= self.GRAPH_AUTO_PXF)
            eager = (not graphed or self.prof is not None or out_dtype is not None or shortcut is not None
                     or torch.cuda.is_current_stream_capturing())
            rerun = lambda: self._forward(xf, nm, past, future, out_dtype, sc, clip=T)      # noqa: E731
            out = self._checked(rerun if eager else lambda: self._forward_graphed(xf, nm, past, future, clip=T), rerun, T)
            return out.reshape(B, n_out, *out.shape[1:])

    def _checked(self, first, rerun, frames: int) -> torch.Tensor:
        """Every forward runs through here: first() issues the window (eagerly or as a replay), rerun() would issue it again eagerly, frames is
        the window's length.  Nothing to check here; Engine wraps its range guard around it."""
        return first()

    class GuardScope:
        """Result of guard_scope(): `tripped` is set when the scope closes."""
        tripped = False
        frames = 1

    @contextlib.contextmanager
    def guard_scope(self):
        """Several forwards under ONE range-guard check at the scope's exit (Engine.guard_scope).  Without a guard the scope never trips."""
        yield Network.GuardScope()

    def _forward_graphed(self, x, noise_map, past, future, clip: int = 0):
        # clip: frames per clip of a batch (forward_clips; x holds B * clip frames), 0 for forward -- part of the key, so is B
        key = (tuple(x.shape), x.dtype, None if noise_map is None else (tuple(noise_map.shape), noise_map.dtype), past, future, clip)

        def run(xx, nn):
            return self._forward(xx, nn, past, future, clip=clip) if clip else self._forward(xx, nn, past, future)
        ent = self._graphs.get(key)
        if ent is None:                         # first sight of this signature: eager (also the warm-up the capture needs)
            self._graphs[key] = "seen"
            self._evict_graphs()
            return run(x, noise_map)
        self._graphs.move_to_end(key)
        if ent == "eager":
            return run(x, noise_map)
        if ent == "seen":
            try:
                sx = x.clone()
                sn = noise_map.clone() if noise_map is not None else None
                g = torch.cuda.CUDAGraph()
                # thread_local: an allocation or a sync on ANOTHER host thread (pin-memory workers, a second engine) must neither fail nor
                # invalidate this capture; __exit__ ends the capture on an exception too: the stream is never left capturing
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    so = run(sx, sn)
                ent = self._graphs[key] = (g, sx, sn, so)
                self._evict_graphs()
            except Exception as e:                                  # noqa: BLE001  (capture unsupported here: stay eager, say so once)
                import warnings
                if torch.cuda.is_current_stream_capturing():        # belt and braces: a capture that __exit__ could not end
                    try:
                        g.capture_end()
                    except Exception:                               # noqa: BLE001
                        pass
                warnings.warn(f"shiftnet_amd: hipGraph capture failed ({type(e).__name__}: {e}); running eagerly")
                self._graphs[key] = "eager"
                torch.cuda.synchronize(self.dev)
                return run(x, noise_map)
        g, sx, sn, so = ent
        sx.copy_(x)
        if sn is not None:
            sn.copy_(noise_map)
        g.replay()
        return so.clone()                       # the graph owns `so`: hand out a copy, like the fresh tensor upstream returns

    GRAPH_AUTO_PXF = 500_000   # T x H x W below which the launch stream, not the GPU, paces a forward (a 20 x 144 x 256 window: 0.74 M is GPU-bound)
    GRAPH_SLOTS = 2          # captured graphs kept per engine: each pins its whole activation pool (GBs at 720p), so a client that varies
    #                          the window shape must not accumulate them

    def _evict_graphs(self) -> None:
        live = [k for k, v in self._graphs.items() if isinstance(v, tuple)]
        while len(live) > self.GRAPH_SLOTS:
            k = live.pop(0)                     # least recently used
            g = self._graphs.pop(k)[0]
            g.reset()                           # frees the graph's private memory pool
        while len(self._graphs) > 16:           # the "seen" / "eager" markers are bounded too
            k = next(iter(self._graphs))
            v = self._graphs.pop(k)
            if isinstance(v, tuple):
                v[0].reset()

    def _forward(self, x: torch.Tensor, noise_map: Optional[torch.Tensor], past: int, future: int,
                 out_dtype: Optional[torch.dtype] = None, shortcut: Optional[torch.Tensor] = None, clip: int = 0) -> torch.Tensor:
        """clip > 0: x holds x.shape[0] / clip clips of `clip` frames (forward_clips); the result is their trimmed frames, clip after clip."""
        assert not clip or (self.split is None and x.shape[0] % clip == 0)
        self._clip = clip
        try:
            return self._forward_frames(x, noise_map, past, future, out_dtype, shortcut)
        finally:
            self._clip = 0

    def _forward_frames(self, x: torch.Tensor, noise_map: Optional[torch.Tensor], past: int, future: int,
                        out_dtype: Optional[torch.dtype], shortcut: Optional[torch.Tensor]) -> torch.Tensor:
        V = self.V
        x = x.contiguous()
        T, cin, H, W = x.shape
        div = 8 if V.topo == "plus" else 4
        if H % div or W % div:
            raise ValueError(f"{V.name}: H and W must be multiples of {div} (got {H}x{W})")
        sp = self.split
        Tc = self._clip or T                # frames per clip
        B = T // Tc
        lo = past if (sp is None or sp.rank == 0) else 0                         # a split window trims on its outer ranks only
        hi = Tc - (future if (sp is None or sp.rank == sp.world - 1) else 0)
        n_out = max(hi - lo, 0)
        out = torch.empty((B * n_out, 3, H, W), dtype=out_dtype or x.dtype, device=x.device)
        if sp is not None:
            sp.validate(n_out)              # collective: all ranks raise together, none is left waiting in an exchange
        if n_out == 0:
            return out                      # T <= past+future yields an empty tensor upstream as well
        x0 = self.cab("feat_extract.1.", self.conv("feat_extract.0", [self._ingest(x, noise_map)]))
        t = x0
        for i in range(1, V.n_orb + 1):     # deblur: res0 = orbN(..) + shortcut (gshift_deblur1.py:769), folded into the last CAB
            t = self.tfr_unet(f"orb{i}.", t, x0 if (i == V.n_orb and not V.denoise) else None)
        res0 = t
        sam = self.conv("conv_trans", [res0])
        dec = self.stage1(sam)
        feats = sam if V.denoise else res0

        def cut(a: Act) -> Act:
            return Act(a.t[lo:hi], a.c)
        prelu = self.P.scalar("lrelu.weight") if V.denoise else None
        if self._clip:                      # a batch of clips: every clip's [lo, hi) read in place by the conv's frame remap
            y = self.conv("rconcat", [x0, feats, dec], prelu=prelu, remap=(n_out, Tc, lo))
        else:
            y = self.conv("rconcat", [cut(x0), cut(feats), cut(dec)], prelu=prelu)
        sc = y
        for i in range(1, V.n_orb + 1):     # deblur: "+ shortcut" after the last rorb (:779), same folding
            y = self.tfr_unet(f"rorb{i}.", y, sc if (i == V.n_orb and not V.denoise) else None)
        sc = x if shortcut is None else shortcut
        assert sc.shape[0] == T and tuple(sc.shape[2:]) == (H, W) and sc.shape[1] >= 3 and sc.device == x.device
        if self._clip:                      # the per-clip [lo, hi) frames of the 3-channel shortcut, gathered
            sc_out = sc.reshape(B, Tc, *sc.shape[1:])[:, lo:hi, :3].reshape(B * n_out, 3, H, W).contiguous()
        else:
            sc_out = sc[lo:hi, :3].contiguous() if sc.shape[1] > 3 else sc[lo:hi].contiguous()
        self.conv("conv_last", [y], out_mode=2, nchw_out=out, nchw_sc=sc_out)
        return out
