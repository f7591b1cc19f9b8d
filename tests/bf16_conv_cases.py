"""The kernel table of the bf16-storage conv (csrc/sn_conv.hip: sn_conv2d, sn_cab_stats) and its float64 reference, shared by the CPU route test
(tests/test_host_bf16_routes.py) and the GPU test (tests/test_gpu_bf16_conv_kernels.py).

Every row names the instance -- SN_CONV_ROUTE(kernel, mt, a, d, mode, rl) of include/shiftnet_hip.h, shiftnet_amd.lib.conv_route -- that
sn_conv2d_route must return for it on a 256-CU device, and streaming rows also the facts of the work plan they must get there (`plan`, literal
values) and the plan shapes they stand for (`edges`, checked as properties of the plan).

Operands: inputs and residuals are bf16 values of a wide exponent range (unit normal noise x 2^U(-6, 6)) with 1 in 16 exact zeros and zero pad
channels; weights are rounded to bf16 exactly as prep.pack_conv rounds them and the reference uses the rounded values; bias and oscale are
nonzero fp32.

Per-element bound (the GPU test): |got - ref| <= u_out |ref| + (1 + u_out) (eps M + extra) with
  M     = conv(|x_eff|, |w|) + |bias|, through max(1, |slope|), |oscale|, + |res| + |res2| (+ |sc| for NCHW outputs); x_eff = the input, or its
          bilinear x2 upsampling for in_mode 1 (of |x|);
  eps   = (n + 8) 2^-24, n = k k sum(cin) products per output, on every route: bf16 x bf16 products are exact in fp32, so this is Higham's gamma_n
          for the fp32 sums in any order plus the epilogue's few operations (bias, PReLU, scale, residuals, the NCHW shortcut);
  extra = in_mode 1 only: conv(2^-8 |up(x)|, |w|) -- the loader (ld_bilinear) rounds the interpolated value to bf16 before the MFMA;
  u_out = the rounding of the stored value: 2^-8 for bf16 (RNE to 8 significant bits: half an ulp is at most 2^-8 of the value, reached just
          above a power of two -- 2^-9 would be the bound of a 9-bit format), 2^-11 (+ 2^-25 absolute, subnormals) for fp16, 0 for fp32 NCHW.
The (1 + u_out) factor: the stored value is the rounding of the fp32 result, which is itself within eps M + extra of ref.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from shiftnet_amd import lib as L

U = 2.0 ** -24
U_BF16 = 2.0 ** -8
R = L.conv_route
KG, KF, KS, KP = L.SN_CONV_K_GENERIC, L.SN_CONV_K_FAST, L.SN_CONV_K_STATS, L.SN_CONV_K_STREAM
EINVAL = -22
TILE, STREAM_ALL, RES_REGS, DEPTH3, DEPTH4, S2_SMALL = 1, 1 << 8, 1 << 9, 1 << 10, 2 << 10, 1 << 15
F32, F16, BF16 = L.SN_F32, L.SN_F16, L.SN_BF16
FAST_KEYS = ((1, 16), (2, 24), (3, 40), (3, 48), (4, 64), (5, 80))
STREAM_KEYS = ((1, 16), (2, 24), (3, 40), (3, 48), (4, 64))


def G8(mt):
    return R(KG, mt, 8)


def G4(mt):
    return R(KG, mt, 4)


def FAST(mt, cs):
    return R(KF, mt, cs)


def STATS(mt, cs):
    return R(KS, mt, cs)


def ST(mt, cs, d, mode, rl=0):
    return R(KP, mt, cs, d, mode, rl)


def WGS(n):
    return n << 4


# every instance sn_conv2d / sn_cab_stats can launch (csrc/sn_conv.hip: conv_route, csrc/sn_conv3p.hip: sn_conv3p_route)
ALL_ROUTES = sorted(
    [G8(mt) for mt in range(1, 7)] + [G4(mt) for mt in range(1, 7)]
    + [FAST(*k) for k in FAST_KEYS] + [STATS(1, 16), STATS(2, 24)]
    + [ST(1, 16, d, m) for d in (2, 3, 4) for m in range(4)] + [ST(1, 16, 2, 2, 1)]
    + [ST(2, 24, 2, m) for m in range(4)] + [ST(2, 24, 1, 2, 1)]
    + [ST(mt, cs, 1 if cs == 64 else 2, m) for (mt, cs) in STREAM_KEYS[2:] for m in range(4)])


def is_stream(r):
    return r >= 0 and (r >> 24) == KP


def stream_mode(r):
    return (r >> 4) & 15


@dataclass
class Case:
    id: str
    route: int                             # at ncu = 256 (and on the MI355X)
    cs_in: int
    cins: Tuple[int, ...]                  # logical channels of each input (n_in = len), the rest of cs_in is zero padding
    c_out: int                             # logical output channels of the conv (out_mode 1: 4 x the shuffled channels)
    T: int = 1
    h_in: int = 8                          # spatial size the conv sees (in_mode 1: twice the stored size)
    w_in: int = 8
    k: int = 3
    stride: int = 1
    pad: Optional[int] = None
    in_mode: int = 0
    out_mode: int = 0
    nchw_dtype: int = F32
    sc_dtype: int = F32
    prelu: Optional[float] = None
    res: bool = False
    res2: bool = False
    oscale: bool = False
    pool: bool = False
    flags: int = 0
    ks_extra: int = 0                      # zero k-steps beyond the minimum
    clip: Optional[Tuple[int, int, int]] = None     # (clip_n, clip_T, clip_lo)
    lines: bool = False                    # an sn_cab_stats row
    plan: Dict[str, int] = field(default_factory=dict)
    edges: Tuple[str, ...] = ()
    gpu: bool = True                       # False: host only (a frame of 2^31 bytes is never allocated)
    nc_waiver: Optional[str] = None
    seed: int = 0

    @property
    def p(self):
        return self.k // 2 if self.pad is None else self.pad

    @property
    def n_in(self):
        return len(self.cins)

    @property
    def hs(self):
        return self.h_in // 2 if self.in_mode == 1 else self.h_in

    @property
    def ws(self):
        return self.w_in // 2 if self.in_mode == 1 else self.w_in

    @property
    def h_out(self):
        return (self.h_in + 2 * self.p - self.k) // self.stride + 1

    @property
    def w_out(self):
        return (self.w_in + 2 * self.p - self.k) // self.stride + 1

    @property
    def c_log(self):                       # channels of the stored output
        return self.c_out // 4 if self.out_mode == 1 else self.c_out

    @property
    def cs_out(self):
        return 8 if self.out_mode == 2 else (self.c_log + 7) // 8 * 8

    @property
    def mt(self):
        return self.cs_out // 4 if self.out_mode == 1 else (self.c_out + 15) // 16

    @property
    def ks(self):
        return (self.k * self.k * self.n_in * self.cs_in + 31) // 32 + self.ks_extra

    @property
    def T_in(self):
        return self.T if self.clip is None else self.T // self.clip[0] * self.clip[1]

    @property
    def n_products(self):
        return self.k * self.k * sum(self.cins)

    @property
    def lines_len(self):
        return max(self.h_out, self.w_out) + 3 if self.lines else 0

    @property
    def oscale_stride(self):
        return 16 * self.mt + 4


def _c(id, route, cs_in, cins, c_out, **kw):
    return Case(id=id, route=route, cs_in=cs_in, cins=tuple(cins), c_out=c_out, **kw)


def _stream_rows(mt, cs, d, flags, modes=(0, 1, 2, 3), rl2=0, flags2=0, tag=""):
    """one row per MODE of a streaming instance; MODE 2 rows add flags2 (16 channels: the streaming kernel only where asked for)"""
    shapes = {0: dict(T=3, h_in=40, w_in=70), 1: dict(T=2, h_in=21, w_in=33, prelu=0.25, pool=True),
              2: dict(T=2, h_in=17, w_in=64, oscale=True, res=True), 3: dict(T=3, h_in=12, w_in=37, prelu=0.6, pool=True, lines=True)}
    out = []
    for m in modes:
        kw = dict(shapes[m])
        out.append(_c(f"st{mt}0{cs}_d{d}_m{m}{tag}", ST(mt, cs, d, m, rl2 if m == 2 else 0), cs, [cs], cs,
                      flags=flags | (flags2 if m == 2 else 0), **kw))
    return out


PN, PB = -0.25, 1.25                       # PReLU slopes outside [0, 1]

CASES: List[Case] = [
    # ---- generic MFMA kernel, 8 x 32 tiles: MT 1..6, 2-3 inputs, k 1 / 2 / 3 / 5, bilinear loader, pixel shuffle, NCHW, padded ks, remap ----
    _c("g8_mt1_cat2_res_pool_T3", G8(1), 8, [8, 6], 16, T=3, h_in=9, w_in=33, prelu=PN, res=True, pool=True),
    _c("g8_mt2_k2s2_pool", G8(2), 16, [14], 32, h_in=17, w_in=65, k=2, stride=2, pad=0, pool=True),
    _c("g8_mt1_k5_nchw_f32_sc_f16", G8(1), 16, [14], 3, T=2, h_in=9, w_in=35, k=5, out_mode=2, nchw_dtype=F32, sc_dtype=F16),
    _c("g8_mt1_k5_nchw_f16_sc_bf16", G8(1), 16, [14], 3, h_in=7, w_in=33, k=5, out_mode=2, nchw_dtype=F16, sc_dtype=BF16),
    _c("g8_mt1_k5_nchw_bf16_sc_f32", G8(1), 16, [14], 3, T=2, h_in=11, w_in=31, k=5, out_mode=2, nchw_dtype=BF16, sc_dtype=F32),
    _c("g8_mt2_up_k1_res_odd", G8(2), 24, [18], 24, T=2, in_mode=1, h_in=10, w_in=18, k=1, res=True, pool=True),
    _c("g8_mt4_up_k3_cat2_odd", G8(4), 16, [16, 12], 56, in_mode=1, h_in=14, w_in=6, prelu=PB, oscale=True),
    _c("g8_mt4_pixshuffle", G8(4), 32, [30], 56, out_mode=1, h_in=9, w_in=33, prelu=PN),
    _c("g8_mt6_pixshuffle_T2", G8(6), 16, [16], 80, T=2, out_mode=1, h_in=5, w_in=17),
    _c("g8_mt2_pixshuffle_k1", G8(2), 8, [8], 24, out_mode=1, h_in=3, w_in=40, k=1),
    _c("g8_mt1_ks_padded", G8(1), 16, [16], 16, h_in=12, w_in=40, ks_extra=2, prelu=0.25, pool=True),
    _c("g8_mt2_cs32_osc_res", G8(2), 32, [32], 32, h_in=10, w_in=40, oscale=True, res=True),
    _c("g8_mt5_cs56_res_res2_pool", G8(5), 56, [52], 80, T=2, h_in=9, w_in=31, prelu=PN, res=True, res2=True, pool=True),
    _c("g8_mt3_cat2_osc_res_res2", G8(3), 24, [24, 20], 48, h_in=8, w_in=32, oscale=True, res=True, res2=True),
    _c("g8_mt3_cat3_clip_remap", G8(3), 8, [8, 8, 6], 40, T=4, clip=(2, 5, 2), h_in=9, w_in=33, prelu=PN, res=True),
    _c("g8_mt6_cat2_lds92k_pool", G8(6), 64, [64, 60], 96, h_in=10, w_in=35, pool=True),
    _c("g8_mt5_k5_cat2_osc", G8(5), 16, [16, 16], 72, h_in=8, w_in=32, k=5, oscale=True),
    # ---- generic MFMA kernel, 4 x 16 tiles: stride 2 over more than 24 input channels, bit 15 of flags on a narrow one ----
    _c("g4_mt1_s2_cs32_pool", G4(1), 32, [32], 16, stride=2, h_in=17, w_in=33, prelu=PB, pool=True),
    _c("g4_mt2_k2s2_res", G4(2), 32, [28], 32, k=2, stride=2, pad=0, h_in=16, w_in=62, res=True),
    _c("g4_mt3_s2_cat2_res_res2", G4(3), 16, [16, 14], 48, T=3, stride=2, h_in=9, w_in=35, res=True, res2=True),
    _c("g4_mt4_k5s2", G4(4), 40, [40], 64, k=5, stride=2, h_in=11, w_in=19),
    _c("g4_mt5_s2_pool", G4(5), 64, [64], 80, stride=2, h_in=15, w_in=40, prelu=PN, pool=True),
    _c("g4_mt6_s2_1x1_T2", G4(6), 48, [48], 96, T=2, stride=2, h_in=1, w_in=1, oscale=True),
    _c("g4_mt2_bit15_narrow", G4(2), 16, [14], 18, stride=2, h_in=33, w_in=65, flags=S2_SMALL),
    # ---- specialised 3x3 tile kernel, all six keys (SN_CONV_TILE_KERNEL): plain, PReLU + pool, oscale + res ----
    _c("f1016_plain_T5_1x1", FAST(1, 16), 16, [16], 16, T=5, h_in=1, w_in=1, flags=TILE),
    _c("f1016_prelu_pool", FAST(1, 16), 16, [16], 16, T=2, h_in=13, w_in=70, prelu=0.25, pool=True, flags=TILE),
    _c("f1016_osc_res_1xW", FAST(1, 16), 16, [16], 16, h_in=1, w_in=97, oscale=True, res=True, flags=TILE),
    _c("f2024_plain_Hx1", FAST(2, 24), 24, [24], 18, h_in=45, w_in=1, flags=TILE),
    _c("f2024_prelu_pool_T3", FAST(2, 24), 24, [22], 24, T=3, h_in=17, w_in=33, prelu=0.6, pool=True, flags=TILE),
    _c("f2024_osc_res_8x32", FAST(2, 24), 24, [24], 24, T=2, h_in=8, w_in=32, oscale=True, res=True, flags=TILE),
    _c("f3040_plain", FAST(3, 40), 40, [40], 36, h_in=9, w_in=31, flags=TILE),
    _c("f3040_prelu_pool", FAST(3, 40), 40, [40], 40, h_in=20, w_in=70, prelu=PB, pool=True, flags=TILE),
    _c("f3040_osc_res_T3", FAST(3, 40), 40, [36], 40, T=3, h_in=7, w_in=40, oscale=True, res=True, flags=TILE),
    _c("f3048_plain_T2", FAST(3, 48), 48, [48], 48, T=2, h_in=16, w_in=33, flags=TILE),
    _c("f3048_prelu_pool", FAST(3, 48), 48, [48], 48, h_in=9, w_in=64, prelu=PN, pool=True, flags=TILE),
    _c("f3048_osc_res", FAST(3, 48), 48, [48], 48, h_in=3, w_in=5, oscale=True, res=True, flags=TILE),
    _c("f4064_plain", FAST(4, 64), 64, [64], 64, h_in=10, w_in=30, flags=TILE),
    _c("f4064_prelu_pool_T2", FAST(4, 64), 64, [64], 64, T=2, h_in=8, w_in=65, prelu=0.25, pool=True, flags=TILE),
    _c("f4064_osc_res", FAST(4, 64), 64, [60], 64, h_in=17, w_in=17, oscale=True, res=True, flags=TILE),
    _c("f5080_plain_default", FAST(5, 80), 80, [80], 80, h_in=9, w_in=33),
    _c("f5080_prelu_pool", FAST(5, 80), 80, [80], 80, T=2, h_in=11, w_in=40, prelu=PB, pool=True, flags=TILE),
    _c("f5080_osc_res", FAST(5, 80), 80, [80], 80, h_in=8, w_in=64, oscale=True, res=True, flags=TILE),
    # ... and what the selector moves off the streaming kernel without the flag
    _c("f1016_res_res2_default", FAST(1, 16), 16, [16], 16, T=2, h_in=12, w_in=40, res=True, res2=True),
    _c("f1016_osc_res_default", FAST(1, 16), 16, [16], 16, T=2, h_in=17, w_in=64, oscale=True, res=True),
    _c("f2024_prelu_neg_mode1_default", FAST(2, 24), 24, [24], 24, h_in=21, w_in=33, prelu=PN, pool=True),
    _c("f1016_prelu_1p25_mode1_default", FAST(1, 16), 16, [16], 16, T=2, h_in=21, w_in=33, prelu=PB, pool=True),
    # ---- sn_cab_stats on the tile kernel ----
    _c("s1016_tile_2x2_T3", STATS(1, 16), 16, [16], 16, T=3, h_in=2, w_in=2, prelu=0.25, pool=True, lines=True, flags=TILE),
    _c("s2024_tile", STATS(2, 24), 24, [24], 24, T=2, h_in=19, w_in=45, prelu=0.6, pool=True, lines=True, flags=TILE),
    _c("s1016_tile_neg_slope_default", STATS(1, 16), 16, [16], 16, h_in=9, w_in=33, prelu=PN, pool=True, lines=True),
]
# ---- streaming kernel, every instance: MODE 0 bias, 1 PReLU + pool, 2 oscale + res, 3 sn_cab_stats ----
CASES += _stream_rows(1, 16, 2, 0, modes=(0, 1, 3)) + _stream_rows(1, 16, 2, 0, modes=(2,), rl2=1, flags2=STREAM_ALL)
CASES += _stream_rows(1, 16, 2, 0, modes=(2,), flags2=STREAM_ALL | RES_REGS, tag="_regs")
CASES += _stream_rows(1, 16, 3, DEPTH3, flags2=STREAM_ALL) + _stream_rows(1, 16, 4, DEPTH4, flags2=STREAM_ALL)
CASES += _stream_rows(2, 24, 2, 0, modes=(0, 1, 3)) + _stream_rows(2, 24, 1, 0, modes=(2,), rl2=1)
CASES += _stream_rows(2, 24, 2, 0, modes=(2,), flags2=RES_REGS, tag="_regs")
CASES += _stream_rows(3, 40, 2, 0) + _stream_rows(3, 48, 2, 0) + _stream_rows(4, 64, 1, 0)
CASES += [
    # ---- streaming plans: edge images and work splits ----
    _c("st1016_m1_one_tile_T5", ST(1, 16, 2, 1), 16, [16], 16, T=5, h_in=8, w_in=32, prelu=0.25, pool=True),
    _c("st1016_m0_1x1_T3", ST(1, 16, 2, 0), 16, [16], 16, T=3, h_in=1, w_in=1),
    _c("st2024_m1_1xW", ST(2, 24, 2, 1), 24, [24], 24, T=2, h_in=1, w_in=100, prelu=0.25, pool=True),
    _c("st1016_m2_Hx1", ST(1, 16, 2, 2, 1), 16, [16], 16, T=2, h_in=50, w_in=1, oscale=True, res=True, flags=STREAM_ALL),
    _c("st1016_m1_wgs1", ST(1, 16, 2, 1), 16, [16], 16, T=4, h_in=60, w_in=100, prelu=0.25, pool=True, flags=WGS(1)),
    _c("st2024_m3_wgs5", ST(2, 24, 2, 3), 24, [24], 24, T=5, h_in=44, w_in=70, prelu=0.25, pool=True, lines=True, flags=WGS(5)),
    _c("st3048_m0_tall_T4", ST(3, 48, 2, 0), 48, [48], 48, T=4, h_in=100, w_in=40),
    _c("st1016_m1_short_segment", ST(1, 16, 2, 1), 16, [16], 16, T=2, h_in=83, w_in=100, prelu=0.25, pool=True),
    _c("st1016_m3_short_segment", ST(1, 16, 2, 3), 16, [16], 16, T=2, h_in=81, w_in=40, prelu=0.6, pool=True, lines=True),
    # ---- refusals and fallbacks checked on the host ----
    _c("refuse_generic_lds_160k", EINVAL, 64, [64, 64, 64], 16, k=5, h_in=8, w_in=32),
    _c("frame_2g_bytes_tile", FAST(1, 16), 16, [16], 16, h_in=8192, w_in=8192, gpu=False),
]
for _i, _cs in enumerate(CASES):
    _cs.seed = 2000 + 31 * _i

# ---- plan facts at ncu = 256: {ntx, nty, S, nseg, nsg, qs, grid, pool_rows} of every streaming row ----
PLANS = {
    "st1016_d2_m0": (3, 5, 1, 5, 45, 8, 8, 60), "st1016_d2_m1": (2, 3, 3, 1, 4, 2, 8, 8), "st1016_d2_m3": (2, 2, 2, 1, 6, 3, 8, 8),
    "st1016_d2_m2": (2, 3, 3, 1, 4, 2, 8, 8), "st1016_d2_m2_regs": (2, 3, 3, 1, 4, 2, 8, 8),
    "st1016_d3_m0": (3, 5, 1, 5, 45, 8, 8, 60), "st1016_d3_m1": (2, 3, 3, 1, 4, 2, 8, 8), "st1016_d3_m2": (2, 3, 3, 1, 4, 2, 8, 8),
    "st1016_d3_m3": (2, 2, 2, 1, 6, 3, 8, 8),
    "st1016_d4_m0": (3, 5, 1, 5, 45, 8, 8, 60), "st1016_d4_m1": (2, 3, 3, 1, 4, 2, 8, 8), "st1016_d4_m2": (2, 3, 3, 1, 4, 2, 8, 8),
    "st1016_d4_m3": (2, 2, 2, 1, 6, 3, 8, 8),
    "st2024_d2_m0": (3, 5, 1, 5, 45, 8, 8, 60), "st2024_d2_m1": (2, 3, 3, 1, 4, 2, 8, 8), "st2024_d2_m3": (2, 2, 2, 1, 6, 3, 8, 8),
    "st2024_d1_m2": (2, 3, 3, 1, 4, 2, 8, 8), "st2024_d2_m2_regs": (2, 3, 3, 1, 4, 2, 8, 8),
    "st3040_d2_m0": (3, 5, 1, 5, 45, 8, 8, 60), "st3040_d2_m1": (2, 3, 3, 1, 4, 2, 8, 8), "st3040_d2_m2": (2, 3, 3, 1, 4, 2, 8, 8),
    "st3040_d2_m3": (2, 2, 2, 1, 6, 3, 8, 8),
    "st3048_d2_m0": (3, 5, 1, 5, 45, 8, 8, 60), "st3048_d2_m1": (2, 3, 3, 1, 4, 2, 8, 8), "st3048_d2_m2": (2, 3, 3, 1, 4, 2, 8, 8),
    "st3048_d2_m3": (2, 2, 2, 1, 6, 3, 8, 8),
    "st4064_d1_m0": (3, 5, 1, 5, 45, 8, 8, 60), "st4064_d1_m1": (2, 3, 3, 1, 4, 2, 8, 8), "st4064_d1_m2": (2, 3, 3, 1, 4, 2, 8, 8),
    "st4064_d1_m3": (2, 2, 2, 1, 6, 3, 8, 8),
    "st1016_m1_one_tile_T5": (1, 1, 1, 1, 5, 5, 8, 4), "st1016_m0_1x1_T3": (1, 1, 1, 1, 3, 3, 8, 4), "st2024_m1_1xW": (4, 1, 1, 1, 8, 8, 8, 16),
    "st1016_m2_Hx1": (1, 7, 1, 7, 14, 7, 8, 28), "st1016_m1_wgs1": (4, 8, 8, 1, 16, 1, 16, 16), "st2024_m3_wgs5": (3, 6, 2, 3, 45, 4, 16, 36),
    "st3048_m0_tall_T4": (2, 13, 1, 13, 104, 8, 16, 104),
    "st1016_m1_short_segment": (4, 11, 3, 4, 32, 3, 16, 64), "st1016_m3_short_segment": (2, 11, 3, 4, 16, 3, 8, 32),
}
# the work splits a row stands for (EDGE_CHECKS): a short last segment of a column, a workgroup's chunk that runs into the next frame, a grid
# padded to a multiple of 8 past the last chunk, a frame of one tile; st1016_m1_wgs1 / st2024_m3_wgs5 override the workgroups per CU
EDGES = {
    "st1016_m1_short_segment": ("short_last_segment", "chunk_crosses_frame", "idle_workgroups"),
    "st1016_m3_short_segment": ("short_last_segment", "chunk_crosses_frame", "idle_workgroups"),
    "st1016_d2_m0": ("chunk_crosses_frame", "idle_workgroups"),
    "st2024_m3_wgs5": ("chunk_crosses_frame", "idle_workgroups"),
    "st1016_m1_one_tile_T5": ("one_tile_per_frame", "chunk_crosses_frame", "idle_workgroups"),
    "st1016_m0_1x1_T3": ("one_tile_per_frame",),
    "st1016_m2_Hx1": ("idle_workgroups",),
}
EDGE_CHECKS = {
    "short_last_segment": lambda p: p["nseg"] * p["S"] > p["nty"],
    "chunk_crosses_frame": lambda p: (p["nseg"] * p["ntx"]) % p["qs"] != 0 and p["nsg"] > p["nseg"] * p["ntx"],
    "idle_workgroups": lambda p: p["grid"] > -(-p["nsg"] // p["qs"]),
    "one_tile_per_frame": lambda p: p["ntx"] == 1 and p["nty"] == 1,
}
for _cs in CASES:
    if _cs.id in PLANS:
        _cs.plan = dict(zip(L.CONV_PLAN_FIELDS, PLANS[_cs.id]))
    _cs.edges = EDGES.get(_cs.id, ())


def by_id(i: str) -> Case:
    return next(c for c in CASES if c.id == i)


def stats_partner(route: int) -> int:
    """the sn_conv2d route of the conv a statistics route computes (its lines and pool must be bit-identical to that conv's)"""
    if (route >> 24) == KS:
        return R(KF, (route >> 20) & 15, (route >> 12) & 255)
    return R(KP, (route >> 20) & 15, (route >> 12) & 255, (route >> 8) & 15, 1, 0)


# ---- descriptors ----------------------------------------------------------------------------------------------------------------------

def pointer_model(case: Case) -> Dict[str, object]:
    """fake device addresses (sn_conv2d_route tests them for NULL only)"""
    base = [0x10000000 * (i + 1) for i in range(12)]
    return {"in": base[0:3], "w": base[3], "bias": base[4], "oscale": base[5], "res": base[6], "res2": base[7], "out": base[8],
            "sc": base[9], "pool": base[10]}


def fill_desc(case: Case, ptr: Dict[str, object], flags: Optional[int] = None):
    d = L.ConvDesc()
    for i in range(case.n_in):
        d.inp[i] = ptr["in"][i]
    d.n_in, d.cs_in, d.T, d.h_in, d.w_in, d.in_mode = case.n_in, case.cs_in, case.T, case.h_in, case.w_in, case.in_mode
    d.k, d.stride, d.pad, d.h_out, d.w_out = case.k, case.stride, case.p, case.h_out, case.w_out
    d.wfrag, d.mt, d.ks = ptr["w"], case.mt, case.ks
    d.bias = ptr["bias"]
    d.act, d.prelu = (1, case.prelu) if case.prelu is not None else (0, 0.0)
    d.out, d.cs_out, d.out_mode, d.c_out = ptr["out"], case.cs_out, case.out_mode, case.c_out
    if case.out_mode == 2:
        d.sc, d.nchw_dtype, d.sc_dtype = ptr["sc"], case.nchw_dtype, case.sc_dtype
    if case.res:
        d.res = ptr["res"]
    if case.res2:
        d.res2 = ptr["res2"]
    if case.oscale:
        d.oscale, d.oscale_stride = ptr["oscale"], case.oscale_stride
    if case.pool:
        d.pool = ptr["pool"]
    if case.clip is not None:
        d.clip_n, d.clip_T, d.clip_lo = case.clip
    d.flags = case.flags if flags is None else flags
    return d


# ---- operands and the float64 reference ------------------------------------------------------------------------------------------------

def _act(g, shape, c):
    x = torch.randn(shape, generator=g) * torch.exp2(torch.rand(shape, generator=g) * 12.0 - 6.0)
    x[torch.rand(shape, generator=g) < 1.0 / 16] = 0.0
    x[..., c:] = 0.0
    return x.to(torch.bfloat16)


def make_operands(case: Case) -> Dict[str, object]:
    """CPU operands of a case (deterministic per case): xs bf16 NHWC [T_in][hs][ws][cs_in], w fp32 [c_out][sum cins][k][k] (rounded to bf16 by
    the packing), bias fp32 [c_out], oscale fp32 [T][oscale_stride], res / res2 bf16 NHWC, sc [T][c_log][h][w] (out_mode 2)."""
    g = torch.Generator().manual_seed(case.seed)
    ops: Dict[str, object] = {"xs": [_act(g, (case.T_in, case.hs, case.ws, case.cs_in), c) for c in case.cins]}
    fan = sum(case.cins) * case.k * case.k
    ops["w"] = (torch.randn((case.c_out, sum(case.cins), case.k, case.k), generator=g) / math.sqrt(fan)).float()
    sgn = lambda n: torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)      # noqa: E731
    ops["bias"] = ((0.05 + 0.5 * torch.rand(case.c_out, generator=g)) * sgn(case.c_out)).float()
    shp = (case.T, case.h_out, case.w_out, case.cs_out)
    if case.oscale:
        n = case.T * case.oscale_stride
        ops["oscale"] = ((0.25 + torch.rand(n, generator=g)) * sgn(n)).float().view(case.T, case.oscale_stride)
    if case.res:
        ops["res"] = _act(g, shp, case.c_log)
    if case.res2:
        ops["res2"] = _act(g, shp, case.c_log)
    if case.out_mode == 2:
        dt = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}[case.sc_dtype]
        ops["sc"] = torch.rand((case.T, case.c_out, case.h_out, case.w_out), generator=g).to(dt)
    return ops


def frame_map(case: Case) -> List[int]:
    if case.clip is None:
        return list(range(case.T))
    n, cT, lo = case.clip
    return [(j // n) * cT + lo + j % n for j in range(case.T)]


def eps_of(case: Case) -> float:
    return (case.n_products + 8) * U


def nc_mask(case: Case) -> torch.Tensor:
    """Negative control: the weights with the LAST 32-wide block of the kernel's K order (k = tap * n_in cs_in + input * cs_in + channel) that holds
    a real channel of a tap the image reaches zeroed -- or, where all those products sit in one block, the last input channel dropped.  (A 1 x W
    image never reads the taps of the rows above and below it: a block of those alone changes nothing.)"""
    cv = case.n_in * case.cs_in

    def reach(n_in, n_out):
        return [any(0 <= y * case.stride - case.p + dy < n_in for y in range(n_out)) for dy in range(case.k)]
    ry, rx = reach(case.h_in, case.h_out), reach(case.w_in, case.w_out)
    kidx = torch.full((sum(case.cins), case.k * case.k), -1, dtype=torch.long)
    base = 0
    for i, c in enumerate(case.cins):
        for tap in range(case.k * case.k):
            if ry[tap // case.k] and rx[tap % case.k]:
                kidx[base:base + c, tap] = tap * cv + i * case.cs_in + torch.arange(c)
        base += c
    blocks = torch.where(kidx >= 0, kidx // 32, kidx)
    blocks = torch.where(blocks >= 0, blocks, blocks.max())        # unreachable taps join the last block (zeroing them changes nothing)
    if int(blocks.min()) < 0:
        blocks = blocks.clamp(min=0)
    mask = torch.ones((case.c_out, sum(case.cins), case.k, case.k), dtype=torch.float64)
    if int(blocks.max()) == int(blocks.min()):
        mask[:, -1] = 0.0
    else:
        mask[:, (blocks == blocks.max()).view(sum(case.cins), case.k, case.k)] = 0.0
    return mask


def reference(case: Case, ops: Dict[str, object], control: bool = False):
    """(ref, tol, M, e) in float64: NHWC [T][h][w][c_log] (out_mode 0 / 1) or NCHW [T][c_out][h][w] (out_mode 2); e = eps M + extra, the bound of
    the fp32 value before the store rounds it (what `pool` sums).  control: the negative-control weights (nc_mask)."""
    d = torch.float64
    idx = frame_map(case)
    x = torch.cat([xx[idx][..., :c].permute(0, 3, 1, 2).to(d) for xx, c in zip(ops["xs"], case.cins)], 1)
    w = ops["w"].to(torch.bfloat16).to(d)                 # the rounding prep.pack_conv applies
    if control:
        w = w * nc_mask(case)
    ax = x.abs()
    ex_in = None
    if case.in_mode == 1:
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        ax = F.interpolate(ax, scale_factor=2, mode="bilinear", align_corners=False)
        ex_in = U_BF16 * x.abs()
    a = F.conv2d(x, w, stride=case.stride, padding=case.p)
    m = F.conv2d(ax, w.abs(), stride=case.stride, padding=case.p)
    ex = F.conv2d(ex_in, w.abs(), stride=case.stride, padding=case.p) if ex_in is not None else torch.zeros_like(m)
    b = ops["bias"].to(d).view(1, -1, 1, 1)
    a, m = a + b, m + b.abs()
    if case.prelu is not None:
        a = torch.where(a >= 0, a, a * case.prelu)
        sl = max(1.0, abs(case.prelu))
        m, ex = m * sl, ex * sl
    if case.oscale:
        os_ = ops["oscale"][:, :case.c_out].to(d).view(case.T, -1, 1, 1)
        a, m, ex = a * os_, m * os_.abs(), ex * os_.abs()
    for name in ("res", "res2"):
        if name in ops:
            r = ops[name][..., :case.c_out].permute(0, 3, 1, 2).to(d)
            a, m = a + r, m + r.abs()
    u_abs = 0.0
    if case.out_mode == 2:
        sc = ops["sc"].to(d)
        a, m = a + sc, m + sc.abs()
        u_out = {F32: 0.0, F16: 2.0 ** -11, BF16: U_BF16}[case.nchw_dtype]
        u_abs = 2.0 ** -25 if case.nchw_dtype == F16 else 0.0
    else:
        u_out = U_BF16
    e = eps_of(case) * m + ex
    tol = u_out * a.abs() + (1.0 + u_out) * e + u_abs + 1e-30
    if case.out_mode == 2:
        return a, tol, m, e
    if case.out_mode == 1:
        a, tol, m, e = (F.pixel_shuffle(t, 2) for t in (a, tol, m, e))
    return tuple(t.permute(0, 2, 3, 1) for t in (a, tol, m, e))


def round_to(x: torch.Tensor, dtype: int) -> torch.Tensor:
    """float64 x rounded to nearest even in the stored format (bf16: 8 significant bits; fp16: 11, subnormal below 2^-14), exactly, in float64"""
    if dtype == F32:
        return x.float().double()
    bits, emin = (8, -125) if dtype == BF16 else (11, -13)
    m, ex = torch.frexp(x)                                      # x = m 2^ex, 0.5 <= |m| < 1
    ex = ex.clamp(min=emin)
    return torch.round(torch.ldexp(x, bits - ex)) * torch.exp2((ex - bits).double())


def rounding_interval(case: Case, ref: torch.Tensor, e: torch.Tensor):
    """[lo, hi]: every value the store can produce from an fp32 result within e of ref (rounding is monotone).  A tighter test than the bound
    above, which has to allow a whole rounding step around ref: here the stored value must be the rounding of SOME value within eps M + extra."""
    dt = case.nchw_dtype if case.out_mode == 2 else BF16
    return round_to(ref - e, dt), round_to(ref + e, dt)


def pool_depth(route: int, plan: Optional[List[int]]) -> int:
    """most output values one pool row sums: a tile (generic / tile kernels) or a wave's two rows of 32 pixels over a segment of S tiles"""
    if is_stream(route):
        return 64 * plan[2]
    if (route >> 24) == KG:
        th = (route >> 12) & 255
        return th * 4 * th
    return 256
