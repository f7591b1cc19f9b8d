"""ctypes binding of libshiftnet_hip.so (the C ABI in include/shiftnet_hip.h).

There is deliberately NO fallback: if the shared object is missing or a symbol
is absent, importing the product path fails loudly (the HIP kernels ARE the
product; the CPU oracle under ``oracle/`` is test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libshiftnet_hip.so")

SN_F32, SN_F16, SN_BF16 = 0, 1, 2

ABI_VERSION = 20    # == SN_ABI_VERSION of include/shiftnet_hip.h; a stale .so from before a struct / signature change fails the check in load()

SYMBOLS = [          # include/shiftnet_hip.h, production ABI
    "sn_abi_version", "sn_selftest_mfma", "sn_ingest", "sn_conv2d", "sn_conv_pool_blocks", "sn_conv2d_route","sn_upsample2_add", "sn_ca_mlp",
    "sn_cab_ca", "sn_cab_ca_scratch_floats", "sn_cab_fused_supported", "sn_cab_stats", "sn_cab_ca_lines", "sn_cab_fused", "sn_planar_pitch", "sn_nhwc_to_planar", "sn_dw5m_blocks",
    "sn_dw5m_gemm_gate", "sn_gsts_gather", "sn_temporal_roll", "sn_gsts_shiftconv", "sn_gsts_shiftconv_mfma", "sn_gsts_shiftconv_mfma_plan", "sn_gsts_shiftconv_mfma_plan_opt", "sn_gsts_shiftconv_mfma_opt", "sn_gsts_cab2_phase2", "sn_cab1_phase2",
    "sn_ingest_u8", "sn_egress_blocks", "sn_egress_u8", "sn_ssim_blocks", "sn_ssim_u8",
    "sn_ingest_yuv", "sn_egress_yuv", "sn_yuv_thumb", "sn_yuv_noise_hist",
    "sn_ingest_yuv_rect", "sn_egress_yuv_rect", "sn_yuv_noise_hist_rect", "sn_yuv_rowcol_sums", "sn_egress_yuv_dither",
    "sn_yuv_noise_hist_bands", "sn_noise_map_level", "sn_egress_yuv_mix", "sn_yuv_noise_hist_pairs", "sn_yuv_noise_hist_pairs_bands",
    "sn_yuv_diff_stats", "sn_yuv_diff_stats_mv", "sn_yuv_block_motion", "sn_yuv_noise_hist_pairs_mv", "sn_yuv_noise_hist_pairs_bands_mv",
    "sn_tile_accumulate", "sn_geo_transform", "sn_geo_accumulate", "sn_time_crossfade", "sn_yuv_niqe_sums", "sn_yuv_ssim_sums", "sn_yuv_degrade", "sn_yuv_blur", "sn_yuv_grain",
    "sn_yuv_code_hist", "sn_yuv_apply_lut", "sn_yuv_despot",
    "sn32_conv2d", "sn32_conv2d_route", "sn32_gsts_gather", "sn32_layernorm", "sn32_gate", "sn32_gate_sum", "sn32_chan_sum", "sn32_scale_residual", "sn32_ingest", "sn32_cab_ca", "sn32_dw_gate", "sn32_conv1x1_gate2", "sn32_gsts_shiftconv", "sn32_conv_csum_tiles",
    "sn_ln_gemm_gate", "sn_lngate_blocks", "sn_grp5_gemm_gate", "sn_grp5_blocks", "sn_gsts_cab2_phase1", "sn_cab1_phase1", "sn_phase1_pool_blocks", "sn_phase1_g1_store_bytes", "sn_p1r_plan", "sn_p1r_strip_begin",
    "sn_cab2_phase2_cab1_phase1", "sn_cab2_phase2_cab1_phase1_supported",
]


class Phase1Weights(C.Structure):
    """sn_phase1_weights (device pointers): prep.pack_phase1r (csrc/sn_phase1r.hip)."""
    _fields_ = [("wfrag1", C.c_void_p), ("w3", C.c_void_p), ("wgrp", C.c_void_p), ("wfrag2", C.c_void_p)]


class SeFold(C.Structure):
    """sn_se_fold: CALayer2's MLP finished by the last workgroup of each frame of the phase-1 launch."""
    _fields_ = [("wa", C.c_void_p), ("wb", C.c_void_p), ("c", C.c_int), ("cr", C.c_int), ("ticket", C.c_void_p), ("ca", C.c_void_p), ("bad", C.c_void_p)]


class Phase1Opts(C.Structure):
    """sn_phase1_opts: the denoisers' inner CALayer2 (pass 1: g1_sums = 1; pass 2: g1_scale = its scale [T][C] f32); team: 0 = the library's
    choice of how many workgroups walk consecutive frames in lock step (measurement knob)."""
    _fields_ = [("g1_scale", C.c_void_p), ("g1_sums", C.c_int), ("team", C.c_int), ("g1_store", C.c_void_p)]


def cab_phase1(lib, src: "UnitSrc", hw_ptr, wt: "Phase1Weights", g2_ptr, pool_ptr, stream, se: "SeFold" = None, opt: "Phase1Opts" = None) -> int:
    """sn_gsts_cab2_phase1 (src.mode 1 / 2) or sn_cab1_phase1 (mode 0)."""
    sep = C.byref(se) if se is not None else None
    op = C.byref(opt) if opt is not None else None
    if src.mode:
        return lib.sn_gsts_cab2_phase1(C.byref(src), hw_ptr, C.byref(wt), g2_ptr, pool_ptr, sep, op, stream)
    return lib.sn_cab1_phase1(C.byref(src), C.byref(wt), g2_ptr, pool_ptr, sep, op, stream)


class ConvDesc(C.Structure):
    _fields_ = [
        ("inp", C.c_void_p * 3), ("n_in", C.c_int), ("cs_in", C.c_int),
        ("T", C.c_int), ("h_in", C.c_int), ("w_in", C.c_int), ("in_mode", C.c_int),
        ("k", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("h_out", C.c_int), ("w_out", C.c_int),
        ("wfrag", C.c_void_p), ("mt", C.c_int), ("ks", C.c_int), ("bias", C.c_void_p),
        ("act", C.c_int), ("prelu", C.c_float), ("res", C.c_void_p), ("out", C.c_void_p),
        ("cs_out", C.c_int), ("out_mode", C.c_int), ("c_out", C.c_int), ("nchw_dtype", C.c_int),
        ("sc", C.c_void_p), ("sc_dtype", C.c_int), ("pool", C.c_void_p), ("oscale", C.c_void_p), ("oscale_stride", C.c_int), ("res2", C.c_void_p),
        ("flags", C.c_int), ("clip_n", C.c_int), ("clip_T", C.c_int), ("clip_lo", C.c_int),
    ]


SN_CONV_TILE_KERNEL = 1


def conv_flags(wgs: int = 0, stream_all: bool = False, res_regs: bool = False, depth: int = 0, dbg: int = 0, s2_small: bool = False) -> int:
    """The measurement fields of sn_conv_desc.flags, above bit 0 (SN_CONV_TILE_KERNEL).  Bits 4-7 wgs: persistent workgroups per CU of the streaming
    kernel (0: the library's choice); 8 stream_all: the streaming kernel also where the library prefers the tile kernel; 9 res_regs: its residual
    operand through registers, not LDS; 10-11 depth: 1 / 2 = three / four tiles of prefetch (16 channels); 12-14 dbg (wrong results): 1 no DMA,
    2 no B reads / MFMAs, 4 no stores; 15 s2_small: stride-2 convs on 4 x 16 tiles whatever their width.  A value that does not fit its field would
    overwrite the neighbouring ones: ValueError."""
    if not (0 <= wgs < 16 and 0 <= depth < 4 and 0 <= dbg < 8):
        raise ValueError(f"sn_conv_desc.flags: wgs={wgs} (0..15), depth={depth} (0..3) or dbg={dbg} (0..7) does not fit its field")
    return (wgs << 4) | (bool(stream_all) << 8) | (bool(res_regs) << 9) | (depth << 10) | (dbg << 12) | (bool(s2_small) << 15)


# sn_conv2d_route: SN_CONV_ROUTE(kernel, mt, a, d, mode, rl) of include/shiftnet_hip.h
SN_CONV_K_GENERIC, SN_CONV_K_FAST, SN_CONV_K_STATS, SN_CONV_K_STREAM = 1, 2, 3, 4
CONV_KERNEL_NAMES = {SN_CONV_K_GENERIC: "conv_mfma", SN_CONV_K_FAST: "conv3_fast", SN_CONV_K_STATS: "conv3_fast_stats", SN_CONV_K_STREAM: "conv3p"}
CONV_PLAN_FIELDS = ("ntx", "nty", "S", "nseg", "nsg", "qs", "grid", "pool_rows")      # the plan argument of sn_conv2d_route


def conv_route(kernel: int, mt: int, a: int, d: int = 0, mode: int = 0, rl: int = 0) -> int:
    return (kernel << 24) | (mt << 20) | (a << 12) | (d << 8) | (mode << 4) | rl


def conv_route_name(r: int) -> str:
    """conv_mfma<MT,TH,TW> / conv3_fast<MT,CS> / conv3_fast_stats<MT,CS> / conv3p<MT,CS,D,MODE,RL>, or EINVAL(code)"""
    if r < 0:
        return f"EINVAL({r})"
    k, mt, a, d, mode, rl = r >> 24, (r >> 20) & 15, (r >> 12) & 255, (r >> 8) & 15, (r >> 4) & 15, r & 15
    name = CONV_KERNEL_NAMES.get(k, str(k))
    if k == SN_CONV_K_GENERIC:
        return f"{name}<{mt},{a},{4 * a}>"
    if k == SN_CONV_K_STREAM:
        return f"{name}<{mt},{a},D{d},MODE{mode},RL{rl}>"
    return f"{name}<{mt},{a}>"


class Conv32Desc(C.Structure):
    _fields_ = [
        ("inp", C.c_void_p * 3), ("c_in", C.c_int * 3), ("cs_in", C.c_int * 3), ("n_in", C.c_int),
        ("T", C.c_int), ("h_in", C.c_int), ("w_in", C.c_int), ("in_mode", C.c_int),
        ("k", C.c_int), ("stride", C.c_int), ("pad", C.c_int), ("groups", C.c_int),
        ("h_out", C.c_int), ("w_out", C.c_int), ("c_out", C.c_int),
        ("w", C.c_void_p), ("bias", C.c_void_p), ("act", C.c_int), ("prelu", C.c_float),
        ("oscale", C.c_void_p), ("oscale_stride", C.c_int), ("res", C.c_void_p), ("cs_res", C.c_int),
        ("out", C.c_void_p), ("cs_out", C.c_int), ("out_mode", C.c_int), ("nchw_dtype", C.c_int), ("sc", C.c_void_p),
        ("wsplit", C.c_void_p), ("iscale", C.c_void_p), ("iscale_stride", C.c_int), ("rscale", C.c_void_p), ("rscale_stride", C.c_int),
        ("ln_w", C.c_void_p), ("ln_b", C.c_void_p), ("csum", C.c_void_p), ("csum_cpad", C.c_int),
        ("clip_n", C.c_int), ("clip_T", C.c_int), ("clip_lo", C.c_int),
    ]


class UnitSrc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("T", C.c_int), ("h", C.c_int), ("w", C.c_int), ("C", C.c_int),
                ("mode", C.c_int), ("wrap", C.c_int), ("halo", C.c_void_p), ("t0", C.c_int), ("nt", C.c_int),
                ("clip", C.c_int)]


# sn_gsts_shiftconv_mfma_plan / sn_gsts_shiftconv_mfma_opt: the two forms of K0 on the matrix cores
SN_K0_TILE, SN_K0_WALK = 1, 2
K0_PLAN_FIELDS = ("form", "S", "nseg", "wgs", "per_x", "per_tile", "ntx", "nty", "nt", "grid")      # the plan argument of sn_gsts_shiftconv_mfma_plan


class K0Opts(C.Structure):
    """sn_k0_opts: form 0 = the plan's, SN_K0_TILE, SN_K0_WALK; seg: segment length 1..8 of the walking form; wgs: workgroups per XCD; 0 = the plan's."""
    _fields_ = [("form", C.c_int), ("seg", C.c_int), ("wgs", C.c_int)]


def k0_plan(lib, src: "UnitSrc", ncu: int, opt: "K0Opts" = None) -> dict:
    """sn_gsts_shiftconv_mfma_plan (opt: sn_gsts_shiftconv_mfma_plan_opt) as a dict of K0_PLAN_FIELDS; raises on SN_EINVAL."""
    plan = (C.c_int * len(K0_PLAN_FIELDS))()
    if opt is None:
        check(lib.sn_gsts_shiftconv_mfma_plan(C.byref(src), ncu, plan), "sn_gsts_shiftconv_mfma_plan")
    else:
        check(lib.sn_gsts_shiftconv_mfma_plan_opt(C.byref(src), ncu, C.byref(opt), plan), "sn_gsts_shiftconv_mfma_plan_opt")
    return dict(zip(K0_PLAN_FIELDS, plan))


# sn_yuv_fmt (csrc/sn_yuv.hip, csrc/sn_yuv_stats.hip)
SN_YUV_444, SN_YUV_420_CENTER, SN_YUV_420_LEFT = 0, 1, 2
SN_YUV_BT601, SN_YUV_BT709 = 0, 1
SN_YUV_LIMITED, SN_YUV_FULL = 0, 1


class YuvFmt(C.Structure):
    """sn_yuv_fmt: sample format of the planar Y'CbCr payloads of sn_ingest_yuv / sn_egress_yuv / sn_yuv_thumb / sn_yuv_noise_hist."""
    _fields_ = [("bits", C.c_int), ("chroma", C.c_int), ("matrix", C.c_int), ("range", C.c_int)]

    def frame_bytes(self, H: int, W: int) -> int:
        c = H * W if self.chroma == SN_YUV_444 else ((H + 1) // 2) * ((W + 1) // 2)
        return (H * W + 2 * c) * (1 if self.bits == 8 else 2)


class YuvRect(C.Structure):
    """sn_yuv_rect: a picture rectangle in luma samples of the stream (sn_ingest_yuv_rect / sn_egress_yuv_rect / sn_yuv_noise_hist_rect)."""
    _fields_ = [("x0", C.c_int), ("y0", C.c_int), ("w", C.c_int), ("h", C.c_int)]


SN_DITHER_NONE, SN_DITHER_TPDF = 0, 1
SN_BLUR_MAX_TAPS = 15 # the longest window of sn_yuv_blur
SN_NLF_BANDS = 16    # knots of a noise-level function (sn_yuv_noise_hist_bands / sn_noise_map_level)
SN_DIFF_STATS = 16   # int64 words per payload of sn_yuv_diff_stats
SN_DIFF_STATS_MV = 8  # int64 words per pair of payloads of sn_yuv_diff_stats_mv
SN_NIQE_BLOCK, SN_NIQE_MAPS, SN_NIQE_SUMS = 96, 5, 5      # sn_yuv_niqe_sums: the block's side in luma samples, maps per block and scale, doubles per map
SN_SSIM_TILE = 32    # sn_yuv_ssim_sums: the side of a tile of the SSIM map in luma samples, one double per tile


class YuvDither(C.Structure):
    """sn_yuv_dither: the dither of sn_egress_yuv_dither; t0 is the frame number of the launch's first payload."""
    _fields_ = [("mode", C.c_int), ("seed", C.c_uint32), ("t0", C.c_int)]


SN_MIX_AMOUNT, SN_MIX_REMOVED = 0, 1
SN_GEO_FLIP_X, SN_GEO_FLIP_Y, SN_GEO_TRANSPOSE, SN_GEO_REVERSE_T = 1, 2, 4, 8      # the op bits of sn_geo_transform / sn_geo_accumulate


class YuvMix(C.Structure):
    """sn_yuv_mix: the mix of sn_egress_yuv_mix; ay, ac are the amounts (SN_MIX_AMOUNT) or the gains (SN_MIX_REMOVED) of Y and of Cb / Cr."""
    _fields_ = [("mode", C.c_int), ("ay", C.c_float), ("ac", C.c_float)]


class YuvDegradeNoise(C.Structure):
    """sn_yuv_degrade_noise: the noise of sn_yuv_degrade; t0 is the stream's frame number of the launch's first payload, knots the sigma curve in 8-bit
    R'G'B' code units."""
    _fields_ = [("seed", C.c_uint32), ("t0", C.c_int), ("knots", C.c_float * SN_NLF_BANDS)]


class YuvBlurWindow(C.Structure):
    """sn_yuv_blur_window: output t of sn_yuv_blur is the mean of the n source payloads clamp(c0 + t + j, lo, hi), j = -(n / 2) .. n / 2."""
    _fields_ = [("n", C.c_int), ("c0", C.c_int), ("lo", C.c_int), ("hi", C.c_int)]


class YuvGrainNoise(C.Structure):
    """sn_yuv_grain_noise: the grain of sn_yuv_grain; t0 is the frame number, in its clip, of the launch's first payload, knots the level curve in LUMA
    code units of the format, chroma the share of it the chroma planes get, taps (w0, w1, w2) of the separable filter (w2, w1, w0, w1, w2)."""
    _fields_ = [("seed", C.c_uint32), ("t0", C.c_int), ("knots", C.c_float * SN_NLF_BANDS), ("chroma", C.c_float), ("taps", C.c_float * 3)]


class ShiftNetLibError(RuntimeError):
    pass


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the library once; raise (never degrade) if it or any declared symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own libamdhip64; it must be mapped BEFORE our library so that both bind to the same HIP
    # runtime (a second runtime in the process owns different streams/contexts and every launch fails).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise ShiftNetLibError(
            f"{LIB_PATH} not found: build it with `python shift-net_amd/build.py` (hipcc, gfx950). "
            "There is no CPU fallback for the Shift-Net HIP path.")
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise ShiftNetLibError(f"{LIB_PATH} lacks symbols {missing}")
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    lib.sn_abi_version.restype = ci
    lib.sn_selftest_mfma.argtypes = [vp, vp, vp, vp]
    lib.sn_ingest.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci, vp]
    lib.sn_conv2d.argtypes = [C.POINTER(ConvDesc), vp]
    lib.sn_conv_pool_blocks.argtypes = [C.POINTER(ConvDesc)]
    lib.sn_conv2d_route.argtypes = [C.POINTER(ConvDesc), ci, ci, C.POINTER(ci * 8)]
    lib.sn_upsample2_add.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp]
    lib.sn_ca_mlp.argtypes = [vp, ci, ci, ci, ci, cf, vp, vp, vp, ci, vp, vp]
    lib.sn_planar_pitch.argtypes = [ci]
    lib.sn_nhwc_to_planar.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    lib.sn_dw5m_blocks.argtypes = [ci, ci]
    lib.sn_dw5m_gemm_gate.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.sn_cab_ca.argtypes = [vp, ci, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp]
    lib.sn_cab_ca_scratch_floats.argtypes = [ci]
    lib.sn_cab_fused_supported.argtypes = [C.POINTER(ConvDesc), C.POINTER(ConvDesc)]
    lib.sn_cab_stats.argtypes = [C.POINTER(ConvDesc), ci, vp]
    lib.sn_cab_ca_lines.argtypes = [vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp]
    lib.sn_cab_fused.argtypes = [C.POINTER(ConvDesc), C.POINTER(ConvDesc), ci, vp]
    lib.sn32_cab_ca.argtypes = [vp, ci, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp]
    lib.sn_gsts_gather.argtypes = [C.POINTER(UnitSrc), vp, vp, vp]
    lib.sn_temporal_roll.argtypes = [C.POINTER(UnitSrc), vp, vp]
    lib.sn_gsts_shiftconv.argtypes = [C.POINTER(UnitSrc), vp, vp, vp, vp]
    lib.sn_gsts_shiftconv_mfma.argtypes = [C.POINTER(UnitSrc), vp, vp, vp, vp]
    lib.sn_gsts_shiftconv_mfma_plan.argtypes = [C.POINTER(UnitSrc), ci, C.POINTER(ci * len(K0_PLAN_FIELDS))]
    lib.sn_gsts_shiftconv_mfma_plan_opt.argtypes = [C.POINTER(UnitSrc), ci, C.POINTER(K0Opts), C.POINTER(ci * len(K0_PLAN_FIELDS))]
    lib.sn_gsts_shiftconv_mfma_opt.argtypes = [C.POINTER(UnitSrc), vp, vp, vp, C.POINTER(K0Opts), vp]
    lib.sn_ln_gemm_gate.argtypes = [C.POINTER(UnitSrc), vp, vp, vp, vp, vp, vp, ci, vp]
    lib.sn_lngate_blocks.argtypes = [ci, ci]
    lib.sn_grp5_gemm_gate.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    lib.sn_grp5_blocks.argtypes = [ci, ci]
    lib.sn_phase1_pool_blocks.argtypes = [ci, ci, ci]
    lib.sn_phase1_g1_store_bytes.argtypes = [ci, ci, ci, ci, C.POINTER(C.c_longlong)]
    lib.sn_p1r_plan.argtypes = [ci, ci, ci, ci, ci, C.POINTER(ci * 7)]
    lib.sn_p1r_strip_begin.argtypes = [C.POINTER(ci * 7), ci, ci]
    lib.sn_gsts_cab2_phase1.argtypes = [C.POINTER(UnitSrc), vp, C.POINTER(Phase1Weights), vp, vp, C.POINTER(SeFold), C.POINTER(Phase1Opts), vp]
    lib.sn_cab1_phase1.argtypes = [C.POINTER(UnitSrc), C.POINTER(Phase1Weights), vp, vp, C.POINTER(SeFold), C.POINTER(Phase1Opts), vp]
    lib.sn_gsts_cab2_phase2.argtypes = [C.POINTER(UnitSrc), vp, vp, vp, vp, vp, vp]
    lib.sn_cab1_phase2.argtypes = [C.POINTER(UnitSrc), vp, vp, vp, vp, vp, vp]
    lib.sn_cab2_phase2_cab1_phase1_supported.argtypes = [C.POINTER(UnitSrc)]
    lib.sn_cab2_phase2_cab1_phase1.argtypes = [C.POINTER(UnitSrc), vp, vp, vp, vp, vp, C.POINTER(Phase1Weights), vp, vp, C.POINTER(SeFold), C.POINTER(Phase1Opts), vp]
    lib.sn_ingest_u8.argtypes = [vp, vp, ci, ci, ci, ci, vp]
    lib.sn_egress_blocks.argtypes = []
    lib.sn_egress_u8.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, vp]
    lib.sn_ssim_blocks.argtypes = []
    lib.sn_ssim_u8.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, vp]
    lib.sn_ingest_yuv.argtypes = [vp, C.POINTER(YuvFmt), vp, ci, ci, ci, ci, ci, ci, vp]
    lib.sn_egress_yuv.argtypes = [vp, ci, C.POINTER(YuvFmt), vp, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_thumb.argtypes = [vp, C.POINTER(YuvFmt), vp, ci, ci, ci, vp]
    lib.sn_yuv_noise_hist.argtypes = [vp, C.POINTER(YuvFmt), vp, ci, ci, ci, ci, ci, vp]
    lib.sn_ingest_yuv_rect.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, ci, ci, ci, ci, ci, ci, vp]
    lib.sn_egress_yuv_rect.argtypes = [vp, ci, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_noise_hist_rect.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_rowcol_sums.argtypes = [vp, C.POINTER(YuvFmt), vp, vp, ci, ci, ci, vp]
    lib.sn_egress_yuv_dither.argtypes = [vp, ci, C.POINTER(YuvFmt), C.POINTER(YuvRect), C.POINTER(YuvDither), vp, ci, ci, ci, ci, ci, vp]
    lib.sn_egress_yuv_mix.argtypes = [vp, ci, C.POINTER(YuvFmt), C.POINTER(YuvRect), C.POINTER(YuvDither), C.POINTER(YuvMix), vp, vp, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_noise_hist_bands.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_noise_hist_pairs.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_noise_hist_pairs_bands.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_block_motion.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, vp, ci, ci, ci, vp]
    lib.sn_yuv_noise_hist_pairs_mv.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, vp, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_noise_hist_pairs_bands_mv.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, vp, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_diff_stats.argtypes = [vp, vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), ci, vp, ci, ci, ci, vp]
    lib.sn_yuv_diff_stats_mv.argtypes = [vp, vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, vp, ci, ci, ci, vp]
    lib.sn_noise_map_level.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), C.POINTER(cf * SN_NLF_BANDS), ci, ci, vp, ci, ci, ci, ci, ci, ci, vp]
    lib.sn_tile_accumulate.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]
    lib.sn_geo_transform.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp]
    lib.sn_geo_accumulate.argtypes = [vp, vp, ci, ci, cf, ci, ci, ci, ci, vp]
    lib.sn_time_crossfade.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
    lib.sn_yuv_niqe_sums.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, vp, ci, ci, ci, vp]
    lib.sn_yuv_ssim_sums.argtypes = [vp, vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, ci, ci, ci, vp]
    lib.sn_yuv_degrade.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvDegradeNoise), vp, vp, ci, ci, ci, vp]
    lib.sn_yuv_blur.argtypes = [vp, ci, C.POINTER(YuvFmt), C.POINTER(YuvBlurWindow), vp, vp, vp, ci, ci, ci, vp]
    lib.sn_yuv_grain.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), C.POINTER(YuvGrainNoise), vp, vp, ci, ci, ci, vp]
    lib.sn_yuv_code_hist.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, ci, ci, ci, vp]
    lib.sn_yuv_apply_lut.argtypes = [vp, C.POINTER(YuvFmt), C.POINTER(YuvRect), vp, vp, ci, ci, ci, vp]
    lib.sn_yuv_despot.argtypes = [vp, C.POINTER(YuvFmt), vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp]
    ll = C.c_longlong
    lib.sn32_conv2d.argtypes = [C.POINTER(Conv32Desc), vp]
    lib.sn32_conv2d_route.argtypes = [C.POINTER(Conv32Desc)]
    lib.sn32_gsts_gather.argtypes = [C.POINTER(UnitSrc), vp, vp, vp, vp]
    lib.sn32_layernorm.argtypes = [vp, ci, ci, vp, vp, vp, ci, ll, vp]
    lib.sn32_gate.argtypes = [vp, ci, ci, vp, ll, vp]
    lib.sn32_gate_sum.argtypes = [vp, ci, ci, ci, vp, ci, ci, ci, vp, vp]
    lib.sn32_dw_gate.argtypes = [vp, ci, vp, ci, ci, vp, ci, ci, ci, ci, vp, vp]
    lib.sn32_conv_csum_tiles.argtypes = [ci, ci]
    lib.sn32_gsts_shiftconv.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.sn32_conv1x1_gate2.argtypes = [vp, ci, ci, vp, ci, ci, vp, ci, ci, vp, vp]
    lib.sn32_chan_sum.argtypes = [vp, ci, ci, ci, ci, ci, ci, vp, vp]
    lib.sn32_scale_residual.argtypes = [vp, vp, vp, ci, vp, ci, ci, ci, vp]
    lib.sn32_ingest.argtypes = [vp, ci, vp, vp, ci, ci, ci, ci, vp]
    for s in SYMBOLS:
        getattr(lib, s).restype = ci
    if lib.sn_abi_version() != ABI_VERSION:
        raise ShiftNetLibError(f"ABI version mismatch: {LIB_PATH} reports {lib.sn_abi_version()}, shiftnet_amd/lib.py expects {ABI_VERSION} "
                               "(stale build: run `python shift-net_amd/build.py`)")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise ShiftNetLibError(f"{what} failed with code {rc}")
