"""The bf16-storage engine: ``network.Network``'s forward on the bf16 / fp16 HIP kernels.  ``Engine`` holds every operator of that path, its
switches (SN_*), the GSTS routes, the frame and streams schedules and the fp16 range guard; ``Plan`` (plan.py) the weights in kernel layouts.

Activations are NHWC bf16 torch tensors ``[T, H, W, Cs]`` (PyTorch is only the allocator / stream owner here); no op below has a torch/ATen
compute fallback.  fp32 modules run on ``engine32.Engine32``, a sibling under ``Network`` that inherits nothing from this file.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import lib as L
from . import prep
from .network import Act, Network, _dtype_code
from .plan import Plan, host_f32_copy          # noqa: F401  (host_f32_copy: imported from here by tests and tools)
from .schedule import stream_plan, wavefront_order
from .spec import UNIT_NAMES, Variant


class Route(NamedTuple):
    """How the GSTS units of a tensor run (Engine.route): decided once per unit, read by naf_buffers and by every step that issues a launch."""
    fused: bool       # phase 1 is ONE kernel (sn_gsts_cab2_phase1 / sn_cab1_phase1), not the two-kernel bf16 chain
    fold: bool        # ... and its squeeze-excite tail finishes CALayer2: no sn_ca_mlp launch
    k4: bool          # the CAB2's phase 2 runs inside the CAB1's phase 1: four launches per unit (k4_fused)
    mstencil: bool    # chain: the depthwise RepConv (C = 64) as a Toeplitz-MFMA 5x5 on a channel-planar g1
    g1_store: bool    # fused denoisers: the sums pass stores its g1 rows and the main pass reads them back


class Engine(Network):
    """bf16-storage engine (fp16 / bf16 modules).  fp32 modules run on engine32.Engine32 (same control flow, fp32 kernels)."""

    def __init__(self, plan: Plan, dtype: torch.dtype = torch.bfloat16) -> None:
        super().__init__(plan, dtype, graph_auto=True)
        self._tickets = None                  # sn_se_fold frame counters: zero between launches (the kernels re-arm them)
        self._old_tickets: List[torch.Tensor] = []
        self._bad = None                      # the range guard's device flag (one u32), created on first use
        self.fallbacks = 0                    # how often the guard moved this engine from the fused phase 1 to the bf16 chain (0 or 1)
        if self.phase1 not in ("auto", "r", "0"):
            raise ValueError(f"SN_PHASE1={self.phase1!r}: expected auto, r (fused kernel) or 0 (two-kernel bf16 chain)")
        if self.k4_fuse not in ("0", "1"):
            raise ValueError(f"SN_K4_FUSE={self.k4_fuse!r}: expected 1 (CAB2's phase 2 inside CAB1's phase 1, four launches per unit) or 0 (five launches)")
        if self.cab_fused not in ("0", "p", "p16", "8", "16", "s8", "s16"):
            raise ValueError(f"SN_CAB_FUSED={self.cab_fused!r}: expected 0 (two launches), p / p16 (streaming form) or 8 / 16 / s8 / s16 (tile form)")
        bad = getattr(plan, "p1r_not_finite", None)
        if bad is not None and self.phase1 != "0":      # known at pack time: no window is wasted on the range guard, and the message names the weight
            msg = (f"shiftnet_amd: {bad}: an fp16 operand of the fused phase-1 kernel is not finite for this checkpoint (body.0 rows small against the "
                   "second 1x1, which the kernel takes times 16 in fp16)")
            if self.phase1 == "r":
                raise ValueError(msg + ".  SN_PHASE1=r was asked for explicitly; SN_PHASE1=auto starts the module on the two-kernel chain, float32 has no fp16 operands.")
            import warnings
            warnings.warn(msg + ": this module runs phase 1 as the two-kernel chain (SN_PHASE1=0), whose second 1x1 is bf16.")
            self.phase1 = "0"

    act_dtype = torch.bfloat16

    # single-input 3x3 stride-1 convs: the persistent streaming kernel (csrc/sn_conv3p.hip) or, SN_CONV_TILES=1, the one-workgroup-per-tile kernel
    conv_tiles = os.environ.get("SN_CONV_TILES", "0") == "1"
    conv_stream_all = os.environ.get("SN_CONV_STREAM_ALL", "0") == "1"      # measurements / tests: the streaming kernel also where the library prefers the tile kernel
    conv_res_regs = os.environ.get("SN_CONV_RES_REGS", "0") == "1"          # measurements: the residual operand of the streaming kernel through registers, not LDS
    conv_dbg = int(os.environ.get("SN_CONV_DBG", "0"))                      # measurements (wrong results): 1 no DMA, 2 no B reads / MFMAs, 4 no stores
    conv_depth = int(os.environ.get("SN_CONV_DEPTH", "0"))                  # measurements: 1 / 2 = three / four tiles of prefetch (16 channels)
    conv_wgs = int(os.environ.get("SN_CONV_WGS", "0"))            # measurements: persistent workgroups per CU of the streaming kernel (0: the library's choice)
    conv_s2_small = os.environ.get("SN_CONV_S2_SMALL", "0") == "1"  # measurements: stride-2 convs on 4 x 16 tiles whatever their width (round 5's choice)

    def conv(self, name: str, ins: Sequence[Act], *, stride: int = 1, pad: Optional[int] = None, prelu: Optional[float] = None,
             res: Optional[Act] = None, out_mode: int = 0, pool: bool = False, in_mode: int = 0, oscale: Optional[torch.Tensor] = None,
             nchw_out: Optional[torch.Tensor] = None, nchw_sc: Optional[torch.Tensor] = None, res2: Optional[Act] = None,
             remap: Optional[Tuple[int, int, int]] = None):
        """remap = (clip_n, clip_T, clip_lo): the inputs hold clips of clip_T frames and output frame j reads frame
        (j / clip_n) * clip_T + clip_lo + j % clip_n of them (sn_conv_desc; the trim of a batch of clips read in place)."""
        p = self.P.convs[name]
        k, cout = int(p["k"]), int(p["cout"])
        T, hs, ws, cs_in = ins[0].dims
        if remap is not None:
            T = T // remap[1] * remap[0]
        assert cs_in == p["cs_in"] and len(ins) == p["n_in"], (name, cs_in, p["cs_in"])
        h_in, w_in = (2 * hs, 2 * ws) if in_mode == 1 else (hs, ws)
        if pad is None:
            pad = k // 2
        h_out = (h_in + 2 * pad - k) // stride + 1
        w_out = (w_in + 2 * pad - k) // stride + 1
        d = L.ConvDesc()
        for i in range(3):
            d.inp[i] = ins[i].t.data_ptr() if i < len(ins) else None
        d.n_in, d.cs_in, d.T, d.h_in, d.w_in, d.in_mode = len(ins), cs_in, T, h_in, w_in, in_mode
        d.k, d.stride, d.pad, d.h_out, d.w_out = k, stride, pad, h_out, w_out
        d.wfrag, d.mt, d.ks = p["wfrag"].data_ptr(), int(p["mt"]), int(p["ks"])
        d.bias = p["bias"].data_ptr() if p["bias"] is not None else None
        d.act, d.prelu = (1, prelu) if prelu is not None else (0, 0.0)
        pool_buf = None
        out_act: Optional[Act] = None
        if out_mode == 2:
            assert nchw_out is not None and nchw_sc is not None
            d.out, d.sc, d.cs_out = nchw_out.data_ptr(), nchw_sc.data_ptr(), 8
            d.c_out, d.nchw_dtype, d.sc_dtype = cout, _dtype_code(nchw_out.dtype), _dtype_code(nchw_sc.dtype)
        else:
            c_log = cout // 4 if out_mode == 1 else cout
            cs_out = prep.ceil8(c_log)
            o = self._new(T, 2 * h_out, 2 * w_out, cs_out) if out_mode == 1 else self._new(T, h_out, w_out, cs_out)
            out_act = Act(o, c_log)
            d.out, d.cs_out, d.c_out = o.data_ptr(), cs_out, cout
        d.out_mode = out_mode
        d.flags = (L.SN_CONV_TILE_KERNEL | L.conv_flags(s2_small=self.conv_s2_small) if self.conv_tiles else
                   L.conv_flags(self.conv_wgs, self.conv_stream_all, self.conv_res_regs, self.conv_depth, self.conv_dbg, self.conv_s2_small))
        if res is not None:
            assert out_mode == 0 and res.dims == out_act.dims
            d.res = res.t.data_ptr()
        if res2 is not None:
            assert out_mode == 0 and res2.dims == out_act.dims
            d.res2 = res2.t.data_ptr()
        if oscale is not None:
            d.oscale, d.oscale_stride = oscale.data_ptr(), oscale.shape[1]
        if remap is not None:
            d.clip_n, d.clip_T, d.clip_lo = remap
        if pool:
            nblk = self.lib.sn_conv_pool_blocks(C.byref(d))
            pool_buf = torch.empty((T, nblk, 16 * d.mt), dtype=torch.float32, device=self.dev)
            d.pool = pool_buf.data_ptr()
        self._meta = ("conv", T, h_out, w_out, len(ins) * cs_in, int(d.cs_out), k, stride, in_mode, out_mode)
        self._call("sn_conv2d", f"sn_conv2d[{name}]", C.byref(d), self._stream())
        if pool:
            return out_act, pool_buf, h_out * w_out
        return out_act

    # ---- blocks (oracle/shiftnet_oracle.py has the same names) ----------------------------------------------
    # K0 = CAB2.conv1(spatial_shift2(borrowed half)): "1" the depthwise 3x3 as a banded GEMM on the matrix cores over a channel-planar LDS window
    # (sn_gsts_shiftconv_mfma, round 6); "0" the VALU kernel of rounds 1-5 (nine 2-byte LDS reads + nine v_dot2c per pixel and channel)
    k0_mfma = os.environ.get("SN_K0_MFMA", "1") != "0"
    # Denoisers (inner CALayer2 on g1): the sums pass of the fused phase 1 stores its g1 rows (fp16, kernel order) and the second pass reads them back
    # instead of running LayerNorm -> 1x1 -> 3x3 -> gate again (sn_phase1_opts.g1_store; bit-identical).  SN_G1_STORE=0: both passes from the input.
    g1_store = os.environ.get("SN_G1_STORE", "1") != "0"
    fold_se = True             # fused phase 1: CALayer2's MLP is finished by the frame's last workgroup (sn_se_fold) instead of an sn_ca_mlp launch
    # Phase 1 of CAB2 / CAB1.  "r": the role-split fused kernel (csrc/sn_phase1r.hip, every variant; `a`, g1 = a1 a2 2^-4 and r are fp16 inside it);
    # "0": the two-kernel chain sn_ln_gemm_gate + sn_dw5m_gemm_gate / sn_grp5_gemm_gate (g1 in bf16 through HBM: a product of two activations
    # cannot leave ITS range).  SN_PHASE1 picks one; "auto" starts fused and lets the range guard decide.
    # C = 64, 20 x 360 x 640, CAB1 / CAB2: "r" 565 / 696 us (round 4), chain 837 / 950 us
    phase1 = os.environ.get("SN_PHASE1", "auto")
    # A GSTS unit is K0 -> phase 1 (CAB2) -> K4 (CAB2) -> phase 1 (CAB1) -> K4 (CAB1).  "1": the CAB2's K4 runs inside the stager waves of the CAB1's
    # phase 1 (sn_cab2_phase2_cab1_phase1: one launch and one read of y per unit less, bit-identical); "0": five launches.  See k4_fused().
    k4_fuse = os.environ.get("SN_K4_FUSE", "1")
    # Range guard of the half-precision intermediates: every squeeze-excite reduction of the GSTS path (the sn_se_fold tail, sn_ca_mlp)
    # raises a device flag when a channel sum is not finite -- what an overflowed fp16 `a`, g1 or r upstream turns into.  forward() reads the flag
    # once per call; a raised flag on the fused path switches THIS engine to the chain for good, warns, and recomputes the window.
    range_guard = os.environ.get("SN_RANGE_GUARD", "1") != "0"
    # "1": forward() reads the flag before it hands the window out (one blocking 4-byte copy: the window can be recomputed).  "async": the flag goes
    # to pinned host memory behind the forward and is looked at when the NEXT forward starts (or by check_range_guard()): no device sync at the end
    # of a window, host preparation of the next one overlaps the GPU -- but a tripped window has already been handed out: it is reported, the
    # engine moves to the chain for the windows that follow, and nothing is recomputed.
    range_guard_async = os.environ.get("SN_RANGE_GUARD", "1") == "async"

    def cab(self, pre: str, x: Act, extra: Optional[Act] = None) -> Act:
        """CAB: 3x3 -> PReLU -> 3x3 -> CALayer -> +x (gshift_deblur1.py:141-156).

        The CALayer scale is known BEFORE the second conv (its pooled input is linear in `mid`, sn_cab_ca), so scale and residual
        (and the optional second residual `extra`) are applied in conv2's epilogue: two sn_conv2d launches, 5 tensor passes.
        Large 16-channel CABs run the streaming fused form instead (3 passes, `mid` in LDS, bit-identical: `cab_fused` below)."""
        p = self.P.cas[pre + "CA"]
        T, h, w, cs = x.dims
        slope = self.P.scalar(pre + "body.1.weight")
        if self.cab_fused in ("8", "16", "s8", "s16") or (self.cab_fused[0] == "p" and extra is None and not self.conv_tiles and
                                                          (self.cab_fused == "p" or (cs == 16 and T * h * w >= self.CAB_FUSED_MIN_PX))):
            out = self._cab_fused(pre, x, extra, slope)
            if out is not None:
                return out
        scratch = torch.empty((self.lib.sn_cab_ca_scratch_floats(T),), dtype=torch.float32, device=self.dev)
        mid, pool, _ = self.conv(pre + "body.0", [x], prelu=slope, pool=True)
        _, nblk, cpad = pool.shape
        ca = torch.empty((T, cpad), dtype=torch.float32, device=self.dev)
        self._call("sn_cab_ca", f"sn_cab_ca[{pre}]", pool.data_ptr(), nblk, cpad, mid.t.data_ptr(), cs, p["c"], p["cr"], h, w,
                   p["w2"].data_ptr(), p["wa"].data_ptr(), p["wb"].data_ptr(), scratch.data_ptr(), ca.data_ptr(), T, self._stream())
        return self.conv(pre + "body.2", [mid], res=x, oscale=ca, res2=extra)

    # Fused dense CAB: statistics pass + one kernel with `mid` in LDS, three tensor passes instead of five, bit-identical to the two-launch form.
    # SN_CAB_FUSED: "0" two sn_conv2d launches; "p" the streaming form (csrc/sn_conv3p.hip: cabp_kernel; 16 / 24 channels) wherever it exists;
    # "p16" (default) the streaming form for 16-channel CABs of at least CAB_FUSED_MIN_PX pixel-frames -- the one case it wins: 504 against 606 us
    # per CAB at 20 x 720 x 1280 alone, 496 against 534 inside a config-2 window (-0.75 ms of 101); 24 channels lose (one workgroup per CU);
    # "8" / "16" / "s8" / "s16": the one-workgroup-per-tile form of csrc/sn_cabf.hip with that many tile rows ("s": statistics on the streaming conv).
    cab_fused = os.environ.get("SN_CAB_FUSED", "p16")
    CAB_FUSED_MIN_PX = 4 << 20

    def _conv_desc(self, name: str, x: Act, *, prelu: Optional[float] = None) -> L.ConvDesc:
        """sn_conv_desc of a single-input 3x3 stride-1 conv of a CAB on x (no output, residual or pool operands yet)."""
        p = self.P.convs[name]
        T, h, w, cs = x.dims
        assert cs == p["cs_in"] and p["n_in"] == 1 and int(p["k"]) == 3
        d = L.ConvDesc()
        d.inp[0] = x.t.data_ptr()
        d.n_in, d.cs_in, d.T, d.h_in, d.w_in, d.in_mode = 1, cs, T, h, w, 0
        d.k, d.stride, d.pad, d.h_out, d.w_out = 3, 1, 1, h, w
        d.wfrag, d.mt, d.ks = p["wfrag"].data_ptr(), int(p["mt"]), int(p["ks"])
        d.bias = p["bias"].data_ptr() if p["bias"] is not None else None
        d.act, d.prelu = (1, prelu) if prelu is not None else (0, 0.0)
        d.cs_out, d.c_out, d.out_mode = prep.ceil8(int(p["cout"])), int(p["cout"]), 0
        d.flags = L.SN_CONV_TILE_KERNEL          # the statistics pass and the fused kernel are tile kernels: their pool rows are per tile
        return d

    def _cab_fused(self, pre: str, x: Act, extra: Optional[Act], slope: float) -> Optional[Act]:
        """CAB as sn_cab_stats -> sn_cab_ca_lines -> sn_cab_fused; None when the library has no fused instance for this width or slope."""
        lib = self.lib
        T, h, w, cs = x.dims
        if h < 2 or w < 2:
            return None
        if self.cab_fused[0] == "p" and not 0.0 <= slope <= 1.0:
            # the streaming form implements PReLU as max(v, a v), right for a slope in [0, 1] only (sn_cab_fused answers SN_EINVAL for any
            # other), and sn_cab_fused_supported looks at geometry alone: decide before anything is launched -- the two-launch form is general
            return None
        d1 = self._conv_desc(pre + "body.0", x, prelu=slope)
        d2 = self._conv_desc(pre + "body.2", x)
        if self.cab_fused[0] in "sp" and not self.conv_tiles:
            # statistics pass on the streaming kernel (its own pool rows: sn_conv_pool_blocks); the streaming fused kernel reads its plan from conv1's flags
            d1.flags = L.conv_flags(wgs=self.conv_wgs, depth=self.conv_depth, dbg=0 if self.cab_fused[0] == "p" else self.conv_dbg)
            if self.cab_fused[0] == "p":
                d2.flags = L.conv_flags(dbg=self.conv_dbg & 1)        # measurements: conv2's weights in LDS, not registers (16 channels)
        if d1.cs_out != cs or d2.cs_out != cs or not lib.sn_cab_fused_supported(C.byref(d1), C.byref(d2)):
            return None
        p = self.P.cas[pre + "CA"]
        ll = max(h, w)
        lines = torch.empty((T, 4, ll, cs), dtype=self.act_dtype, device=self.dev)
        nblk = lib.sn_conv_pool_blocks(C.byref(d1))
        pool = torch.empty((T, nblk, 16 * d1.mt), dtype=torch.float32, device=self.dev)
        scratch = torch.empty((lib.sn_cab_ca_scratch_floats(T),), dtype=torch.float32, device=self.dev)
        ca = torch.empty((T, 16 * d1.mt), dtype=torch.float32, device=self.dev)
        out = self._new(T, h, w, cs)
        d1.out, d1.pool = lines.data_ptr(), pool.data_ptr()
        d2.out, d2.res, d2.oscale, d2.oscale_stride = out.data_ptr(), x.t.data_ptr(), ca.data_ptr(), ca.shape[1]
        if extra is not None:
            assert extra.dims == x.dims
            d2.res2 = extra.t.data_ptr()
        rows = 0 if self.cab_fused[0] == "p" else 16 if self.cab_fused.endswith("16") else 8      # 0: the streaming form (csrc/sn_conv3p.hip: cabp_kernel)
        st = self._stream()
        self._meta = ("cabf", T, h, w, cs, 1)                   # statistics pass: reads x
        self._call("sn_cab_stats", f"sn_cab_stats[{pre}]", C.byref(d1), ll, st)
        self._meta = ()
        self._call("sn_cab_ca_lines", f"sn_cab_ca[{pre}]", pool.data_ptr(), nblk, 16 * d1.mt, lines.data_ptr(), ll, cs, p["c"], p["cr"], h, w,
                   p["w2"].data_ptr(), p["wa"].data_ptr(), p["wb"].data_ptr(), scratch.data_ptr(), ca.data_ptr(), T, st)
        self._meta = ("cabf", T, h, w, cs, 3 if extra is not None else 2)      # fused pass: reads x (+ extra), writes out
        self._call("sn_cab_fused", f"sn_cab_fused[{pre}]", C.byref(d1), C.byref(d2), rows, st)
        return Act(out, x.c)

    def temporal_roll(self, x: Act, reverse: bool) -> Act:
        T, h, w, cs = x.dims
        assert cs == x.c, "Shift_CAB widths (24, 80) are stored unpadded"
        y = self._new(T, h, w, cs)
        mode = 2 if reverse else 1
        self._meta = ("roll", T, h, w, cs)              # (not a kernel of a GSTS unit: bench.py's unit figure must not inherit the previous launch's record)
        for wrap, halo, t0, nt in self._split_pieces(x, mode, False):
            s = self._unit_src(x, mode, wrap=wrap, halo=halo, t0=t0, nt=nt)
            self._call("sn_temporal_roll", "sn_temporal_roll", C.byref(s), y.data_ptr(), self._stream())
        return Act(y, x.c)

    def _guard_ptr(self) -> Optional[int]:
        if not self.range_guard:
            return None
        if self._bad is None:
            self._bad = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        return self._bad.data_ptr()

    def _fold_ok(self, T: int) -> bool:
        """Can the squeeze-excite tail of phase 1 finish the CALayer2 of a tensor of T frames?  Decided on the CLIP length, so that a batch of
        clips (forward_clips) takes the path each of its clips would take alone; the counters then cover the whole batch (_ticket_ptr)."""
        return self.fold_se and (self._clip or T) <= self.MAX_TICKETS

    def _ticket_ptr(self, T: int) -> int:
        """sn_se_fold frame counters for T frames (zero between launches: the kernels re-arm them).  A buffer outgrown by a larger batch stays
        referenced: a captured graph may still use it."""
        if self._tickets is None or self._tickets.numel() < T:
            if self._tickets is not None:
                self._old_tickets.append(self._tickets)
            self._tickets = torch.zeros((max(self.MAX_TICKETS, T),), dtype=torch.int32, device=self.dev)
        return self._tickets.data_ptr()

    def _fused_phase1(self, T: int) -> bool:
        """Does phase 1 of this engine's CAB2 / CAB1 run as the fused kernel?  (The denoisers' two passes rely on the squeeze-excite tail for
        the inner scale, whose frame counters cover MAX_TICKETS frames per clip.)"""
        if self.phase1 == "0":
            return False
        return not (self.V.denoise and not self._fold_ok(T))

    def k4_fused(self, T: int, c: int) -> bool:
        """Route.k4: does gsts_unit run the CAB2's phase 2 inside the CAB1's phase 1?  The fused launch exists for C = 64 without the denoisers'
        inner CALayer2 (C = 80 and the denoisers' two passes keep the five launches), it needs the CAB2's squeeze-excite scale on the device before
        it starts (the fold: the tail of the CAB2's phase 1 wrote it) and takes whole tensors only: no temporal split, no batch of clips, and the unit
        schedule (frame / streams launch frame ranges through naf).  The range guard's move to the bf16 chain (phase1 "0") switches it off too."""
        return (self.k4_fuse == "1" and self._fused_phase1(T) and self._fold_ok(T) and c == 64 and not self.V.denoise and self.split is None
                and not self._clip and self.schedule == "unit")

    def route(self, T: int, c: int) -> Route:
        """The route of the GSTS units of a [T, h, w, c] tensor under this engine's switches and state: the one place that decides it."""
        fused = self._fused_phase1(T)                    # phase 1 in ONE kernel: neither a, g1 nor r leave the CU
        return Route(fused, fused and self._fold_ok(T), self.k4_fused(T, c), not self.V.grouped_rep, fused and self.V.denoise and self.g1_store)

    # ---- one stage of a CAB2 / CAB1 each, for one piece (src; f0, n: its frames for the operators that take plain pointers) on the tensors B of naf_buffers
    def _k0(self, pre: str, src: L.UnitSrc, B: Dict[str, torch.Tensor], st: int) -> None:
        """K0 (CAB2): conv1 of the spatially shifted borrowed half -> hwb."""
        fn = "sn_gsts_shiftconv_mfma" if self.k0_mfma and self.P.k0_mfma_ok else "sn_gsts_shiftconv"
        self._call(fn, "sn_gsts_shiftconv", C.byref(src), self.P.offs.data_ptr(), self.P.units[pre]["w1"].data_ptr(), B["hwb"].data_ptr(), st)

    def _se_fold(self, name: str, T: int, ca: torch.Tensor):
        """sn_se_fold operand: the last workgroup of each frame of a fused phase 1 finishes the squeeze-excite MLP `name` into ca."""
        q = self.P.cas[name]
        return C.byref(L.SeFold(q["wa"].data_ptr(), q["wb"].data_ptr(), q["c"], q["cr"], self._ticket_ptr(T), ca.data_ptr(), self._guard_ptr()))

    def _phase1(self, pre: str, r: Route, src: L.UnitSrc, f0: int, n: int, B: Dict[str, torch.Tensor], st: int) -> bool:
        """Phase 1: g2 and the partial channel sums of CALayer2 (pool2).  True if the fold has also finished its scale ca2."""
        V, u = self.V, self.P.units[pre]
        if r.fused:
            fn = "sn_gsts_cab2_phase1" if src.mode else "sn_cab1_phase1"
            def args(g2_ptr, se, opt):     # the two entry points differ by K0's output, which only the CAB2 reads
                return (C.byref(src),) + ((B["hwb"].data_ptr(),) if src.mode else ()) + (C.byref(u["p1r"]["desc"]), g2_ptr, B["pool2"].data_ptr(), se, opt, st)
            opt = None
            if V.denoise:      # inner CALayer2 on g1 (gshift_denoise1.py:224,257): pass 1 = the channel sums of g1 and, by the tail, its scale ca1
                g1s = B["g1s"].data_ptr() if r.g1_store else None
                self._call(fn, fn + "[g1 sums]", *args(None, self._se_fold(pre + "ca1", src.T, B["ca1"]), C.byref(L.Phase1Opts(None, 1, 0, g1s))))
                opt = C.byref(L.Phase1Opts(B["ca1"].data_ptr(), 0, 0, g1s))
            self._call(fn, fn, *args(B["g2"].data_ptr(), self._se_fold(pre + "ca2", src.T, B["ca2"]) if r.fold else None, opt))
            return r.fold
        g1, g2, pool1, pool2, h, w, c, es = B["g1"], B["g2"], B.get("pool1"), B["pool2"], src.h, src.w, src.C, 2      # es: bytes per activation element
        self._call("sn_ln_gemm_gate", "sn_ln_gemm_gate", C.byref(src), B["hwb"].data_ptr() if src.mode else None, u["w_ln"].data_ptr(), u["b_ln"].data_ptr(),
                   u["w_dw3_h2"].data_ptr(), g1.data_ptr(), pool1.data_ptr() if pool1 is not None else None, 2 if r.mstencil else 0, st)
        ca1_ptr = self.ca_mlp(pre + "ca1", pool1, h * w, out=B["ca1"], frames=(f0, n), guard=self._guard_ptr()).data_ptr() + f0 * c * 4 if V.denoise else None
        k3 = "sn_dw5m_gemm_gate" if r.mstencil else "sn_grp5_gemm_gate"
        self._call(k3, k3, g1.data_ptr() + g1.stride(0) * es * f0, ca1_ptr, u["w_toep5" if r.mstencil else "w_grp"].data_ptr(), u["w_gate"].data_ptr(),
                   g2.data_ptr() + g2.stride(0) * es * f0, pool2.data_ptr() + f0 * pool2.stride(0) * 4, n, h, w, c, st)
        return False

    def _phase2_args(self, pre: str, src: L.UnitSrc, B: Dict[str, torch.Tensor]) -> Tuple:
        u = self.P.units[pre]
        return C.byref(src), B["g2"].data_ptr(), B["ca2"].data_ptr(), u["w_out"].data_ptr(), u["b_out"].data_ptr() if u["b_out"] is not None else None, B["y"].data_ptr()

    def _phase2(self, pre: str, src: L.UnitSrc, B: Dict[str, torch.Tensor], st: int) -> None:
        """Phase 2 (K4): y = shortcut + beta * (1x1 of ca2 * g2)."""
        fn = "sn_gsts_cab2_phase2" if src.mode else "sn_cab1_phase2"
        self._call(fn, fn, *self._phase2_args(pre, src, B), st)

    def _cab2_phase2_cab1_phase1(self, pre2: str, src2: L.UnitSrc, B2: Dict[str, torch.Tensor], meta2: Tuple, pre1: str, B1: Dict[str, torch.Tensor], st: int) -> None:
        """The CAB2's phase 2 inside the stager waves of the CAB1's phase 1 (Route.k4): writes the CAB2's y and the CAB1's g2, pool2 and ca2."""
        fn = "sn_cab2_phase2_cab1_phase1"
        self._call(fn, fn, *self._phase2_args(pre2, src2, B2), C.byref(self.P.units[pre1]["p1r"]["desc"]), B1["g2"].data_ptr(), B1["pool2"].data_ptr(),
                   self._se_fold(pre1 + "ca2", src2.T, B1["ca2"]), None, st)
        if self.prof is not None:
            # The fused launch IS the CAB1's phase 1 (plus the CAB2's phase 2 in its stagers): its time is recorded as sn_cab1_phase1.  The consumers of these
            # records count a finished CAB -- and so the window's units and their bytes -- by its phase-2 record: the CAB2 gets one of zero length (one event twice).
            _, label, meta, e0, e1 = self.prof.pop()
            self.prof += [("sn_gsts_cab2_phase2", "sn_gsts_cab2_phase2 [in sn_cab1_phase1]", meta2, e0, e0), ("sn_cab1_phase1", label, meta, e0, e1)]

    def naf(self, pre: str, x: Act, mode: int, *, frames: Optional[Tuple[int, int]] = None, bufs: Optional[Dict[str, torch.Tensor]] = None) -> Act:
        """CAB2 (mode 1/2, fed by the GSTS gather of x) or CAB1 (mode 0) (gshift_deblur1.py:183-255).

        [K0 (CAB2 only)] -> phase 1 up to g2 (ONE kernel, which the denoisers run twice, or -- phase1 "0" -- the bf16 chain K12 -> K3) -> the squeeze-excite
        MLP (folded into phase 1's last workgroup per frame, or sn_ca_mlp) -> phase 2, K4.  The global average pool of CALayer2 sits between the phases
        and forbids a single pass.  Every frame is independent inside a CAB (the pool is per frame), so a temporally split window runs
        the steps for two pieces: all frames but the boundary one while the halo exchange is in flight, then the boundary frame.  frames = (t0, nt) /
        bufs: one frame range of a block whose tensors the caller owns (the frame-wavefront and streams schedules)."""
        T, h, w, c = x.dims
        r = self.route(T, c)
        self._meta = ("naf", frames[1] if frames is not None else T, h, w, c, mode, T)      # (frames of this launch group, ..., frames of the tensor)
        B = bufs if bufs is not None else self.naf_buffers(T, h, w, c, mode)
        assert frames is None or self.split is None
        pieces = ([(self._wrap_flag(mode, self.V.wrap) if mode else 0, None, frames[0], frames[1])] if frames is not None
                  else self._split_pieces(x, mode, self.V.wrap) if mode else [(0, None, 0, 0)])
        for wrap, halo, t0, nt in pieces:
            st = self._stream()
            src = self._unit_src(x, mode, wrap=wrap, halo=halo, t0=t0, nt=nt)
            f0, n = (t0, nt) if nt else (0, T)
            if mode:
                self._k0(pre, src, B, st)
            if not self._phase1(pre, r, src, f0, n, B, st):
                self.ca_mlp(pre + "ca2", B["pool2"], h * w, out=B["ca2"], frames=(f0, n), guard=self._guard_ptr())
            self._phase2(pre, src, B, st)
        return Act(B["y"], c)

    def naf_buffers(self, T: int, h: int, w: int, c: int, mode: int) -> Dict[str, torch.Tensor]:
        """The tensors one CAB2 / CAB1 writes: hwb (conv1 of the shifted half, CAB2), g2, y, the partial channel sums and the squeeze-excite
        scales; chain only: g1 (bf16, channel-planar for the depthwise RepConv) and the inner pool of the denoisers.  All of them stay
        referenced by the caller until the block's launches are issued: a temporary would go back to the caching allocator at once and a
        tensor K3 WRITES could be carved out of the block K3 still READS its scale from (intermittent wrong frames at the small pyramid
        levels; found by the full-size determinism check of config 4)."""
        lib, V, r = self.lib, self.V, self.route(T, c)
        B: Dict[str, torch.Tensor] = {}
        if mode:
            B["hwb"] = self._new(T, h, w, c // 2)
        B["g2"] = self._new(T, h, w, c)
        B["y"] = self._new(T, h, w, c)
        if r.fused:
            nb2 = lib.sn_phase1_pool_blocks(T, h, w)
            if nb2 < 1:
                raise L.ShiftNetLibError(f"sn_phase1_pool_blocks failed with code {nb2}")
            if r.g1_store:
                nbytes = C.c_longlong(0)
                L.check(lib.sn_phase1_g1_store_bytes(T, h, w, c, C.byref(nbytes)), "sn_phase1_g1_store_bytes")
                B["g1s"] = torch.empty((nbytes.value,), dtype=torch.uint8, device=self.dev)
        else:
            B["g1"] = (torch.empty((T, h, c, lib.sn_planar_pitch(w)), dtype=torch.bfloat16, device=self.dev) if r.mstencil else self._new(T, h, w, c))
            nb2 = lib.sn_dw5m_blocks(h, w) if r.mstencil else lib.sn_grp5_blocks(h, w)
            if V.denoise:
                B["pool1"] = torch.empty((T, lib.sn_lngate_blocks(h, w), c), dtype=torch.float32, device=self.dev)
        if V.denoise:
            B["ca1"] = torch.empty((T, c), dtype=torch.float32, device=self.dev)
        B["pool2"] = torch.empty((T, nb2, c), dtype=torch.float32, device=self.dev)
        B["ca2"] = torch.empty((T, c), dtype=torch.float32, device=self.dev)
        return B

    def gsts_unit(self, pre: str, x: Act, reverse: bool) -> Act:
        """CAB2 (pre + "0.", on the GSTS gather of x) then CAB1 (pre + "1.").  Both CABs' tensors are locals here until the last launch is issued."""
        mode, (T, h, w, c) = 2 if reverse else 1, x.dims
        r = self.route(T, c)
        if not r.k4:
            return super().gsts_unit(pre, x, reverse)
        B2, B1 = self.naf_buffers(T, h, w, c, mode), self.naf_buffers(T, h, w, c, 0)
        src2, src1, st = self._unit_src(x, mode), self._unit_src(Act(B2["y"], c), 0, wrap=0), self._stream()
        self._meta = meta2 = ("naf", T, h, w, c, mode, T)
        self._k0(pre + "0.", src2, B2, st)
        self._phase1(pre + "0.", r, src2, 0, T, B2, st)          # (r.k4 implies r.fold: the CAB2's ca2 is on the device)
        self._meta = ("naf", T, h, w, c, 0, T)
        self._cab2_phase2_cab1_phase1(pre + "0.", src2, B2, meta2, pre + "1.", B1, st)
        self._phase2(pre + "1.", src1, B1, st)
        return Act(B1["y"], c)

    # layer-frame wavefront.  "unit" (default): every unit runs over all T frames before the next one starts (the reference's
    # order, gshift_deblur1.py:530-547).  "frame": the units of consecutive Encoder_shift_blocks of one pyramid level are issued per FRAME GROUP in
    # dependency order -- unit k needs frames {t, t -/+ 1} of unit k - 1 (forward / reverse shift, :504-518), so a group of unit k can start as
    # soon as its own and one neighbouring group of unit k - 1 are done and a frame's working set moves through many units while it is still in
    # the Infinity Cache.  Results are bit-identical (every kernel honours frame ranges and the pool rows do not depend on them).  Measured:
    # DESIGN.md section 3.3 -- no gain while phase 1 is not bandwidth-bound; SN_SCHEDULE=frame / bench.py --schedule frame keep it one flag away.
    # "streams" (round 6): the window's frames are cut into stream_groups contiguous frame groups and every group runs ITS chain of launches
    # (K0 -> phase 1 -> K4 -> phase 1 -> K4, unit after unit) on its own HIP stream; the only cross-stream edges are the one boundary frame a
    # shifted unit borrows from the neighbouring group (events).  The groups drift out of phase by themselves -- two phase-1 launches cannot
    # share a CU (131 / 149 KB of LDS each), so the second one waits and from then on its memory-bound K4 runs UNDER the other group's
    # issue-bound phase 1 (K4 has no LDS and 76 VGPRs: it fits beside phase 1's 12 waves).  Bit-identical to unit-major by construction.
    schedule = os.environ.get("SN_SCHEDULE", "unit")
    frame_group = int(os.environ.get("SN_FRAME_GROUP", "4"))
    stream_groups = int(os.environ.get("SN_STREAM_GROUPS", "2"))
    STREAMS_MIN_PXF = 400_000     # frames x pixels of a GROUP below which the streams schedule is not used (launches too small to overlap usefully)

    def _shift_chain(self, pres: Sequence[str], x: Act) -> Act:
        T = x.dims[0]
        if self.schedule not in ("unit", "frame", "streams") or self.frame_group < 1 or self.stream_groups < 1:
            raise ValueError(f"SN_SCHEDULE={self.schedule!r} / SN_FRAME_GROUP={self.frame_group} / SN_STREAM_GROUPS={self.stream_groups}: "
                             "expected unit, frame or streams, and groups of >= 1 frames")
        if self.schedule == "streams" and self.split is None and not self._clip and not torch.cuda.is_current_stream_capturing():
            ng = min(self.stream_groups, T // 2)
            if ng >= 2 and (T // ng) * x.dims[1] * x.dims[2] >= self.STREAMS_MIN_PXF:
                return self._shift_chain_streams(pres, x, ng)
        if self.schedule != "frame" or self.split is not None or self._clip or T <= self.frame_group:
            return super()._shift_chain(pres, x)
        _, h, w, c = x.dims
        units = [(f"{pre}{UNIT_NAMES[i]}.", i % 2 == 1) for pre in pres for i in range(self.V.units)]
        G = self.frame_group
        groups = [(t0, min(G, T - t0)) for t0 in range(0, T, G)]
        # every unit owns its tensors for the whole chain (no reuse games: 12 units x 3 GB at level 1 of config 2, out of 288 GB)
        bufs = [(self.naf_buffers(T, h, w, c, 2 if rev else 1), self.naf_buffers(T, h, w, c, 0)) for _, rev in units]
        ins = [x] + [Act(b1["y"], c) for _, b1 in bufs]           # ins[u]: input of unit u; ins[u + 1]: its output
        for u, j in wavefront_order([rev for _, rev in units], T, G, self.V.wrap):
            pre, rev = units[u]
            y2 = self.naf(pre + "0.", ins[u], 2 if rev else 1, frames=groups[j], bufs=bufs[u][0])
            self.naf(pre + "1.", y2, 0, frames=groups[j], bufs=bufs[u][1])
        return ins[-1]

    STREAM_RING = 3            # buffer sets of the streams schedule: unit u writes set u % STREAM_RING

    def _shift_chain_streams(self, pres: Sequence[str], x: Act, ng: int) -> Act:
        """The chain with one HIP stream per frame group (see `schedule`).  Group g's stream runs, unit after unit, CAB2 then CAB1 on ITS frames
        (frame-range launches: every GSTS kernel honours sn_unit_src.t0 / nt and their results do not depend on the range).  stream_plan gives
        the cross-stream edges: before CAB2 of unit u a group waits for the group that owns the ONE frame its boundary frame borrows from to
        have finished unit u - 1 (gshift_deblur1.py:504-518), and before it overwrites the ring slot of unit u - STREAM_RING for the groups
        that borrowed from it there."""
        T, h, w, c = x.dims
        units = [(f"{pre}{UNIT_NAMES[i]}.", i % 2 == 1) for pre in pres for i in range(self.V.units)]
        R = min(self.STREAM_RING, max(len(units), 2))
        groups, plan = stream_plan([rev for _, rev in units], T, ng, self.V.wrap, R)
        if getattr(self, "_gstreams", None) is None or len(self._gstreams) < ng:
            self._gstreams = [torch.cuda.Stream(self.dev) for _ in range(ng)]
        streams = self._gstreams[:ng]
        main = torch.cuda.current_stream(self.dev)
        sets = [(self.naf_buffers(T, h, w, c, 1), self.naf_buffers(T, h, w, c, 0)) for _ in range(R)]
        if self.route(T, c).fold:                           # allocated on the launching stream, not on a group's
            self._ticket_ptr(T)
        self._guard_ptr()
        ready = main.record_event()
        done: List[List[Optional[torch.cuda.Event]]] = [[None] * ng for _ in units]      # unit u's output frames of group g are written
        cab2: List[List[Optional[torch.cuda.Event]]] = [[None] * ng for _ in units]      # group g no longer reads unit u's input
        cur = x
        for u, (pre, rev) in enumerate(units):
            b2, b1 = sets[u % R]
            for g, fr in enumerate(groups):
                raw, war = plan[u][g]
                with torch.cuda.stream(streams[g]):
                    s = streams[g]
                    if u == 0:
                        s.wait_event(ready)
                    for uu, gg in raw:
                        s.wait_event(done[uu][gg])
                    for uu, gg in war:
                        s.wait_event(cab2[uu][gg])
                    y2 = self.naf(pre + "0.", cur, 2 if rev else 1, frames=fr, bufs=b2)
                    cab2[u][g] = s.record_event()
                    self.naf(pre + "1.", y2, 0, frames=fr, bufs=b1)
                    done[u][g] = s.record_event()
            cur = Act(b1["y"], c)
        for g in range(ng):
            main.wait_event(done[-1][g])
        return cur

    # SkipUpSample: "1" (default) the 1x1 at LOW resolution, then one streaming pass bilinear x2 + skip (sn_upsample2_add: conv and interpolation
    # commute); "0" round 2's form, the interpolation in the loader of a full-resolution conv (1.3-1.8 TB/s of its bytes)
    skip_up_lowres = os.environ.get("SN_SKIPUP_LOWRES", "1") != "0"

    def skip_up(self, name: str, x: Act, y: Act) -> Act:
        """SkipUpSample: bilinear x2 -> 1x1 -> + y (gshift_deblur1.py:341-350)."""
        if not self.skip_up_lowres:
            return super().skip_up(name, x, y)
        lo = self.conv(name, [x])                             # [T][hs][ws][cs_out]
        T, hs, ws, cs = lo.dims
        assert y.dims == (T, 2 * hs, 2 * ws, cs), (y.dims, lo.dims)
        out = self._new(T, 2 * hs, 2 * ws, cs)
        self._meta = ("up2add", T, hs, ws, cs)
        self._call("sn_upsample2_add", f"sn_upsample2_add[{name}]", lo.t.data_ptr(), y.t.data_ptr(), out.data_ptr(), T, hs, ws, cs, self._stream())
        return Act(out, lo.c)

    def _ingest(self, x: torch.Tensor, noise_map: Optional[torch.Tensor]) -> Act:
        """x = x[0]; cat((x, noise_map), 1) into the kernel layout (gshift_deblur1.py:784-787, gshift_denoise1.py:828-831)."""
        T, cin, H, W = x.shape
        nm_ptr = None
        if self.V.denoise:
            noise_map = noise_map.to(x.dtype).expand(T, 1, H, W).contiguous()
            nm_ptr = noise_map.data_ptr()
        x8 = self._new(T, H, W, 8)
        self._call("sn_ingest", "sn_ingest", x.data_ptr(), _dtype_code(x.dtype), nm_ptr, x8.data_ptr(), T, cin, H, W, self._stream())
        return Act(x8, self.V.in_ch)

    def _checked(self, first, rerun, frames: int) -> torch.Tensor:
        """The range guard around a forward (Network._checked): one flag read per call, and a tripped flag recomputes the window on the chain."""
        if self.range_guard_async:
            self.check_range_guard()               # the PREVIOUS window's flag (its copy has long landed: no wait in the steady state)
        out = first()
        if self._scope is not None:                # guard_scope(): one check when the scope closes
            self._scope.frames = max(self._scope.frames, frames)
        elif self.range_guard_async:
            self._post_guard_copy()
        elif self._guard_tripped():
            out = self._recover(rerun, out, frames)
        return out

    _scope = None

    @contextlib.contextmanager
    def guard_scope(self):
        """Several forwards whose results are consumed TOGETHER (the denoise CLIs' four quadrants of a window, inference/test_denoise.py:153-173) under
        ONE range-guard check: inside the scope no forward reads the flag -- no device sync between them, the launches of the next one queue up
        behind the previous one's kernels -- and the scope's exit reads it once.  If it tripped, the engine has moved to the two-kernel chain and
        `scope.tripped` tells the caller to run the scope's forwards again (cli.quadrant_forward does).  Measured on config 4 (bf16, 4 quadrants x ~2900
        launches per window): 111-114 frames/s with a check per forward (round 5), 118 without any (round 4's library) -- VERDICT r05 item 3."""
        sc = Engine.GuardScope()
        outer, self._scope = self._scope, sc
        try:
            yield sc
        finally:
            self._scope = outer
            if outer is None and not self.range_guard_async:
                sc.tripped = self._guard_tripped()
                if sc.tripped:
                    self._recover(None, None, sc.frames)
            elif outer is not None:
                outer.frames = max(outer.frames, sc.frames)
            else:
                self._post_guard_copy()

    def _post_guard_copy(self) -> None:
        """async guard: flag -> pinned host word behind this forward's launches, then re-arm on the device (stream order)."""
        if self._bad is None or torch.cuda.is_current_stream_capturing():
            return
        if getattr(self, "_bad_host", None) is None:
            self._bad_host = torch.zeros((1,), dtype=torch.int32).pin_memory()
            self._bad_event = torch.cuda.Event()
        self._bad_host.copy_(self._bad, non_blocking=True)
        self._bad.zero_()
        self._bad_event.record()
        self._bad_pending = True

    def check_range_guard(self) -> bool:
        """async guard: has a window since the last check tripped the guard?  Waits for the pending flag copy only (a finished forward: no wait).
        A tripped flag warns and moves the engine to the two-kernel chain for the windows that follow (unless SN_PHASE1=r was asked for)."""
        if not getattr(self, "_bad_pending", False):
            return False
        self._bad_event.synchronize()
        self._bad_pending = False
        v = int(self._bad_host.item())
        if self.split is not None:
            v = self.split.any_rank(v)
        if v:
            self._recover(None, None, 1)
        return bool(v)

    def _guard_tripped(self) -> bool:
        """Reads (and re-arms) the range guard's flag: one 4-byte device-to-host copy per forward.  On a temporally split window the ranks
        agree first -- a rank that recomputed on its own would leave the others alone in the halo exchanges."""
        if self._bad is None or torch.cuda.is_current_stream_capturing():
            return False
        v = int(self._bad.item())
        if self.split is not None:
            v = self.split.any_rank(v)
        if v:
            self._bad.zero_()
        return bool(v)

    def _recover(self, rerun, out, T: int = 1):
        """A tripped range guard.  T: frames of the window that tripped it (did THAT forward run the fused kernel?  The denoisers' long windows
        already run the chain).  rerun None (async guard): report and switch only -- the window has been handed out."""
        import warnings
        if self._fused_phase1(T) and self.phase1 == "r":           # an explicit SN_PHASE1=r is honoured: warn, do not switch
            warnings.warn(f"shiftnet_amd: {self.V.name}: a channel sum of the GSTS path is not finite -- an activation left the fp16 range of the fused "
                          "phase-1 kernel (`a`, g1, r).  SN_PHASE1=r was asked for explicitly, so the module stays on it: the result of this window is "
                          "not reliable (SN_PHASE1=auto would have moved to the two-kernel chain).")
            return out
        if self._fused_phase1(T) and self.phase1 != "0":
            warnings.warn(f"shiftnet_amd: {self.V.name}: a channel sum of the GSTS path is not finite -- an activation left the fp16 range of the fused "
                          "phase-1 kernel (`a`, g1, r).  This module now runs phase 1 as the two-kernel chain with g1 in bf16 (SN_PHASE1=0)"
                          + (" and the window is recomputed." if rerun is not None else "; the results since the previous check (a guard_scope, or the "
                             "window already handed out under SN_RANGE_GUARD=async) are NOT reliable: run them again."))
            self.phase1 = "0"
            self.fallbacks += 1
            for v in self._graphs.values():
                if isinstance(v, tuple):
                    v[0].reset()
            self._graphs.clear()
            if rerun is None:
                return out
            out = rerun()
            if not self._guard_tripped():
                return out
        warnings.warn(f"shiftnet_amd: {self.V.name}: non-finite channel sums on the bf16 chain as well (its `a` is fp16): the result of this window is "
                      "not reliable -- run the module in float32 (net.float(): the fp32 engine has no half-precision intermediates).")
        return out

    MAX_TICKETS = 4096       # frames per tensor the squeeze-excite fold has counters for (longer windows fall back to sn_ca_mlp)


def make_engine(V: Variant, sd: Dict[str, torch.Tensor], device: torch.device, dtype: torch.dtype):
    """Engine for a module of `dtype`: fp32 modules compute in fp32 end to end (what upstream's denoise CLI does for the
    "+" model, inference/test_denoise.py:83-85); fp16 / bf16 modules run the bf16-storage MFMA kernels."""
    if dtype == torch.float32:
        from .engine32 import Engine32, Plan32
        return Engine32(Plan32(V, sd, device))
    return Engine(Plan(V, sd, device), dtype)
