"""The kernel table of the fp32 conv (csrc/sn_f32.hip: sn32_conv2d) and its float64 reference, shared by the CPU route test
(tests/test_host_fp32_routes.py) and the GPU test (tests/test_gpu_fp32_kernels.py).

Every row names the route -- SN32_ROUTE(kernel, a, b) of include/shiftnet_hip.h -- that sn32_conv2d_route must return for it in each arithmetic
("split": the descriptor carries the bf16 hi / lo weight fragments; "exact": it does not).  The route depends on the pointers' 16-byte
alignment, so the CPU test gives every tensor a fake base address with the alignment torch's allocator gives it on the GPU (every allocation is
at least 256-byte aligned) plus the same element offset.

Per-element tolerance (the GPU test): |got - ref| <= tol with tol = eps * M + extra + 1e-30 and
  M     = conv(|x_eff|, |w|) + |bias|, through the same PReLU slope (x max(1, |slope|)), |oscale| and + |res * rscale| as the output;
          x_eff = the operand the kernel multiplies (input x iscale, LayerNorm2d of it, or its bilinear x2 upsampling: of |x|);
  eps   = exact routes: (n + 8) 2^-24, n = cin / groups * k * k products per output: fp32 products and sums in any order (Higham's
          gamma_n) plus the four epilogue operations;
          split routes: 3e-5 + (3 ceil(n / 32) + 8) 2^-24: the two-term bf16 split of both operands keeps every product within 3e-5 of
          |w x| (tests/test_host_packing.py::test_split_precision_product_error_bound), plus one fp32 rounding of the accumulator per
          bf16 MFMA (three per 32 products) and the epilogue;
  extra = LayerNorm on load: conv(delta, |w|) with delta = 16 u (mean|x| + |x - mu|) rstd |g| + 2 u |b| per input value (the fp32 mean and
          variance of the kernel: a few roundings of values of size mean|x|); NCHW half-precision outputs: one rounding of the stored
          value (2^-8 |ref| for bf16, 2^-11 |ref| + 2^-25 for fp16).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

# include/shiftnet_hip.h
K_1X1, K_SPLIT, K_SPLIT_G8, K_EXACT, K_DW, K_DIRECT = 1, 2, 3, 4, 5, 6
KNAME = {K_1X1: "conv32s_1x1", K_SPLIT: "conv32s_dense", K_SPLIT_G8: "conv32s_grouped", K_EXACT: "conv32m", K_DW: "dw32", K_DIRECT: "conv32"}
U = 2.0 ** -24


def route(kern: int, a: int = 0, b: int = 0) -> int:
    return (kern << 16) | (a << 8) | b


def route_name(r: int) -> str:
    if r < 0:
        return f"EINVAL({r})"
    return f"{KNAME.get(r >> 16, r >> 16)}<{(r >> 8) & 255},{r & 255}>"


# every instance sn32_conv2d can launch: the selector's enum x template arguments (csrc/sn_f32.hip: conv32_route)
ALL_ROUTES = sorted(
    [route(K_1X1, ncb, load) for ncb in (1, 2, 3, 4) for load in (0, 1, 2)]
    + [route(K_SPLIT, mtc, ksz) for mtc in (1, 3, 4) for ksz in (1, 3)]
    + [route(K_SPLIT_G8, mtc, ksz) for mtc in (3, 4) for ksz in (3, 5)]
    + [route(K_EXACT, mtc, th) for (mtc, th) in ((1, 8), (3, 8), (5, 8), (2, 4), (5, 4))]
    + [route(K_DW), route(K_DIRECT, 1), route(K_DIRECT, 4)])


def exact_mt(c_out: int, stride: int = 1) -> int:
    """route of the exact matrix-core kernel sn32_conv2d picks for c_out output channels"""
    mt = (c_out + 15) // 16
    if stride == 2:
        return route(K_EXACT, 2 if mt <= 2 else 5, 4)
    return route(K_EXACT, 1 if mt == 1 else (3 if mt <= 3 else 5), 8)


@dataclass
class Case:
    id: str
    routes: Dict[str, int]                 # "split" / "exact" -> declared route
    cins: Tuple[int, ...]                  # logical channels of each input
    c_out: int
    T: int = 1
    h_in: int = 8                          # spatial size the conv sees (in_mode 1: twice the stored size)
    w_in: int = 8
    k: int = 3
    stride: int = 1
    pad: Optional[int] = None
    groups: int = 1
    in_mode: int = 0
    cs_extra: Tuple[int, ...] = ()         # per input: storage channels beyond the slice
    in_off: Tuple[int, ...] = ()           # per input: element offset of the slice inside its pixel
    bias: bool = True
    prelu: Optional[float] = None
    oscale: Optional[int] = None           # None, 0 (one row for all frames) or a row stride >= c_out
    iscale: bool = False
    rscale: bool = False
    res: Optional[int] = None              # None or the residual's pixel stride (>= c_out)
    ln: Optional[float] = None             # LayerNorm on load: None, or the inputs' mean / std (0: zero-mean)
    csum: Optional[int] = None             # channel sums: cpad
    out_mode: int = 0
    nchw_dtype: int = 0                    # SN_F32 / SN_F16 / SN_BF16 (out_mode 2)
    out_cs: Optional[int] = None           # out_mode 0: output pixel stride (default c_out)
    out_off: int = 0                       # out_mode 0: element offset of the output slice
    nc: bool = True                        # split rows: assert the bf16-products negative control (see NC_WAIVED)
    seed: int = 0

    @property
    def p(self) -> int:
        return self.k // 2 if self.pad is None else self.pad

    @property
    def hs(self) -> int:
        return self.h_in // 2 if self.in_mode == 1 else self.h_in

    @property
    def ws(self) -> int:
        return self.w_in // 2 if self.in_mode == 1 else self.w_in

    @property
    def h_out(self) -> int:
        return (self.h_in + 2 * self.p - self.k) // self.stride + 1

    @property
    def w_out(self) -> int:
        return (self.w_in + 2 * self.p - self.k) // self.stride + 1

    def cs_in(self, i: int) -> int:
        return self.in_off_(i) + self.cins[i] + (self.cs_extra[i] if i < len(self.cs_extra) else 0)

    def in_off_(self, i: int) -> int:
        return self.in_off[i] if i < len(self.in_off) else 0

    @property
    def cs_out(self) -> int:
        if self.out_mode == 1:
            return self.c_out // 4
        return self.out_cs if self.out_cs is not None else self.c_out

    @property
    def n_products(self) -> int:
        return sum(self.cins) // self.groups * self.k * self.k


def _c(id, routes, cins, c_out, **kw):
    return Case(id=id, routes=routes, cins=tuple(cins), c_out=c_out, **kw)


S, E = "split", "exact"
PR = -0.3                                  # PReLU slopes outside [0, 1]
PR2 = 1.7

CASES: List[Case] = [
    # ---- flat split 1x1 (conv32s_1x1_kernel), LOAD 0: npix % 64 in {0, 1, 63}, frames shared by a workgroup, NCB 1..4 ----
    _c("1x1_ncb1_8x8", {S: route(K_1X1, 1, 0), E: exact_mt(48)}, [32], 48, h_in=8, w_in=8, k=1, prelu=PR),
    _c("1x1_ncb2_13x5_tail1", {S: route(K_1X1, 2, 0), E: exact_mt(36)}, [60], 36, h_in=13, w_in=5, k=1, oscale=0, res=36),
    _c("1x1_ncb3_1x127_tail63", {S: route(K_1X1, 3, 0), E: exact_mt(20)}, [96], 20, h_in=1, w_in=127, k=1, prelu=PR2, iscale=True),
    _c("1x1_ncb4_T3_hw64", {S: route(K_1X1, 4, 0), E: exact_mt(80)}, [128], 80, T=3, h_in=8, w_in=8, k=1, iscale=True, oscale=84, res=88),
    _c("1x1_ncb1_T3_hw65", {S: route(K_1X1, 1, 0), E: exact_mt(32)}, [16], 32, T=3, h_in=5, w_in=13, k=1, iscale=True, oscale=36, res=40, prelu=PR),
    _c("1x1_ncb2_T3_hw127_slices", {S: route(K_1X1, 2, 0), E: exact_mt(40)}, [40], 40, T=3, h_in=1, w_in=127, k=1, cs_extra=(12,), in_off=(8,),
       iscale=True, oscale=40, res=44, out_cs=48, out_off=4),
    # LOAD 1: LayerNorm2d on load, NCB 1..4, large means
    _c("1x1_ln_ncb1", {S: route(K_1X1, 1, 1)}, [16], 32, T=2, h_in=8, w_in=9, k=1, ln=0.0, prelu=PR),
    _c("1x1_ln_ncb2_T3_hw65", {S: route(K_1X1, 2, 1)}, [64], 128, T=3, h_in=5, w_in=13, k=1, ln=0.0, oscale=128, res=132),
    _c("1x1_ln_ncb3", {S: route(K_1X1, 3, 1)}, [80], 160, h_in=9, w_in=15, k=1, ln=0.0, bias=True, cs_extra=(16,)),
    _c("1x1_ln_ncb4", {S: route(K_1X1, 4, 1)}, [128], 48, h_in=4, w_in=33, k=1, ln=0.0, res=48),
    _c("1x1_ln_mean100", {S: route(K_1X1, 1, 1)}, [32], 64, T=2, h_in=8, w_in=8, k=1, ln=100.0),
    _c("1x1_ln_mean1000", {S: route(K_1X1, 1, 1)}, [32], 64, T=2, h_in=8, w_in=8, k=1, ln=1000.0, nc=False),
    # LOAD 2: bilinear x2 on load (SkipUpSample), NCB 1..4; the exact kernel takes the same shapes without fragments
    _c("1x1_up_ncb1", {S: route(K_1X1, 1, 2), E: exact_mt(32)}, [32], 32, h_in=10, w_in=14, k=1, in_mode=1, res=32),
    _c("1x1_up_ncb2_T3", {S: route(K_1X1, 2, 2), E: exact_mt(48)}, [64], 48, T=3, h_in=6, w_in=22, k=1, in_mode=1, res=52, prelu=PR),
    _c("1x1_up_ncb3", {S: route(K_1X1, 3, 2), E: exact_mt(80)}, [80], 80, h_in=16, w_in=8, k=1, in_mode=1, oscale=0),
    _c("1x1_up_ncb4", {S: route(K_1X1, 4, 2), E: exact_mt(64)}, [128], 64, h_in=8, w_in=16, k=1, in_mode=1, cs_extra=(4,), res=64),
    # ---- split tiles, dense 1x1 (conv32s_kernel<MTC, 1>): one M-tile, concatenated inputs, > 128 channels, images below 64 pixels ----
    _c("s1_mtc1_9x40", {S: route(K_SPLIT, 1, 1), E: exact_mt(12)}, [32], 12, h_in=9, w_in=40, k=1, prelu=PR, res=12),
    _c("s1_mtc3_cat2_9x33", {S: route(K_SPLIT, 3, 1), E: exact_mt(48)}, [24, 40], 48, h_in=9, w_in=33, k=1, oscale=0, res=52),
    _c("s1_mtc4_ncb5_7x31", {S: route(K_SPLIT, 4, 1), E: exact_mt(80)}, [160], 80, h_in=7, w_in=31, k=1, iscale=True, prelu=PR2),
    _c("s1_mtc3_3x5_small", {S: route(K_SPLIT, 3, 1), E: exact_mt(36)}, [36], 36, T=3, h_in=3, w_in=5, k=1, iscale=True, oscale=40, res=36),
    _c("s1_mtc4_1x1_img", {S: route(K_SPLIT, 4, 1), E: exact_mt(64)}, [64], 64, T=3, h_in=1, w_in=1, k=1, res=64),
    # ---- split tiles, dense 3x3 (conv32s_kernel<MTC, 3>, TH 4, TW 32): tile remainders 0 / 1 / TH-1, TW-1, csum, three inputs ----
    _c("s3_mtc1_T3_4x32_csum", {S: route(K_SPLIT, 1, 3), E: exact_mt(16)}, [24], 16, T=3, h_in=4, w_in=32, csum=16, prelu=PR),
    _c("s3_mtc3_cat3_5x33", {S: route(K_SPLIT, 3, 3), E: exact_mt(40)}, [16, 24, 8], 40, h_in=5, w_in=33, oscale=44, res=40, prelu=PR2),
    _c("s3_mtc4_7x63_all", {S: route(K_SPLIT, 4, 3), E: exact_mt(80)}, [64], 80, T=2, h_in=7, w_in=63, iscale=True, oscale=80, res=84,
       csum=80, prelu=PR),
    _c("s3_mtc3_T3_9x31_csum", {S: route(K_SPLIT, 3, 3), E: exact_mt(48)}, [40], 48, T=3, h_in=9, w_in=31, csum=48, oscale=0, res=48),
    _c("s3_mtc4_2x3_small", {S: route(K_SPLIT, 4, 3), E: exact_mt(64)}, [32], 64, T=3, h_in=2, w_in=3, iscale=True, res=64, csum=64),
    _c("s3_mtc1_1x1_img", {S: route(K_SPLIT, 1, 3), E: exact_mt(8)}, [12], 8, T=3, h_in=1, w_in=1, prelu=PR),
    _c("s3_slice_off8", {S: route(K_SPLIT, 3, 3), E: exact_mt(32)}, [24], 32, h_in=6, w_in=20, cs_extra=(8,), in_off=(8,), out_cs=40, out_off=8),
    _c("s3_pixshuffle", {S: route(K_SPLIT, 4, 3), E: exact_mt(64)}, [32], 64, h_in=5, w_in=9, out_mode=1, prelu=PR),
    # unaligned operands leave the split kernels for the exact one
    _c("s3_slice_off2_unaligned", {S: exact_mt(32), E: exact_mt(32)}, [24], 32, h_in=6, w_in=20, cs_extra=(6,), in_off=(2,)),
    _c("s3_cin_odd", {S: exact_mt(24), E: exact_mt(24)}, [22], 24, h_in=9, w_in=17, res=24),
    # ---- split tiles, grouped by 8 (conv32s_kernel<MTC, KSZ, grouped>, TH 8): the "+" RepConv, iscale / rscale / res ----
    _c("g5_mtc3_T3_9x33_rep", {S: route(K_SPLIT_G8, 3, 5), E: exact_mt(48)}, [48], 48, groups=6, T=3, h_in=9, w_in=33, k=5,
       iscale=True, rscale=True, res=48, prelu=PR),
    _c("g5_mtc4_15x31", {S: route(K_SPLIT_G8, 4, 5), E: exact_mt(80)}, [80], 80, groups=10, h_in=15, w_in=31, k=5, oscale=0, res=84),
    _c("g5_mtc4_T3_3x5_rep", {S: route(K_SPLIT_G8, 4, 5), E: exact_mt(64)}, [64], 64, groups=8, T=3, h_in=3, w_in=5, k=5,
       iscale=True, rscale=True, res=64),
    _c("g3_mtc3_8x32", {S: route(K_SPLIT_G8, 3, 3), E: exact_mt(32)}, [32], 32, groups=4, h_in=8, w_in=32, k=3, prelu=PR2, oscale=32),
    _c("g3_mtc4_T3_1x1_img", {S: route(K_SPLIT_G8, 4, 3), E: exact_mt(64)}, [64], 64, groups=8, T=3, h_in=1, w_in=1, k=3, iscale=True,
       rscale=True, res=64),
    _c("g3_mtc4_17x33", {S: route(K_SPLIT_G8, 4, 3), E: exact_mt(80)}, [80], 80, groups=10, h_in=17, w_in=33, k=3, res=80),
    # ---- exact kernel only (conv32m_kernel): k = 2 / 5 dense, bilinear 3x3, NCHW outputs, stride 2 ----
    _c("m1_nchw_f32", {E: exact_mt(3)}, [20], 3, T=2, h_in=9, w_in=33, out_mode=2, nchw_dtype=0),
    _c("m1_nchw_f16", {E: exact_mt(3)}, [20], 3, h_in=8, w_in=31, out_mode=2, nchw_dtype=1),
    _c("m1_nchw_bf16", {E: exact_mt(3)}, [20], 3, h_in=7, w_in=32, out_mode=2, nchw_dtype=2),
    _c("m1_pixshuffle_k3", {S: exact_mt(16), E: exact_mt(16)}, [12], 16, h_in=18, w_in=14, out_mode=1, in_mode=1, prelu=PR),
    _c("m3_k2_pad0_odd", {S: exact_mt(48), E: exact_mt(48)}, [32], 48, T=3, h_in=9, w_in=33, k=2, pad=0, prelu=PR, oscale=48),
    _c("m5_k5_dense_cat2", {S: exact_mt(80), E: exact_mt(80)}, [12, 12], 80, h_in=9, w_in=31, k=5, res=84),
    _c("m5_up3x3_cat2", {S: exact_mt(96), E: exact_mt(96)}, [32, 16], 96, h_in=18, w_in=34, in_mode=1, prelu=PR2, res=96),
    _c("m3_iscale_k5_dense", {S: exact_mt(40), E: exact_mt(40)}, [24], 40, T=2, h_in=8, w_in=33, k=5, iscale=True, oscale=0),
    _c("m2_s2_k3_17x33", {S: exact_mt(32, 2), E: exact_mt(32, 2)}, [16], 32, T=3, h_in=17, w_in=33, stride=2, prelu=PR, res=32),
    _c("m5_s2_k2_15x31", {S: exact_mt(80, 2), E: exact_mt(80, 2)}, [40], 80, h_in=15, w_in=31, k=2, pad=0, stride=2, oscale=80),
    _c("m5_s2_k3_7x29_iscale", {S: exact_mt(64, 2), E: exact_mt(64, 2)}, [64], 64, T=2, h_in=7, w_in=29, stride=2, iscale=True, res=68),
    _c("m2_s2_k5_1x1_img", {S: exact_mt(24, 2), E: exact_mt(24, 2)}, [8], 24, T=3, h_in=1, w_in=1, k=5, stride=2),
    # ---- depthwise (dw32_kernel) and the direct kernels (conv32_kernel<4> grouped by 4, conv32_kernel<1>) ----
    _c("dw3_T3_9x33", {S: route(K_DW), E: route(K_DW)}, [40], 40, groups=40, T=3, h_in=9, w_in=33, prelu=PR, oscale=40, res=44),
    _c("dw5_7x6", {S: route(K_DW), E: route(K_DW)}, [16], 16, groups=16, h_in=7, w_in=6, k=5, oscale=0, cs_extra=(4,)),
    _c("dw3_1x1_img", {S: route(K_DW), E: route(K_DW)}, [24], 24, groups=24, T=3, h_in=1, w_in=1, res=24),
    _c("direct4_g4_5x7", {S: route(K_DIRECT, 4), E: route(K_DIRECT, 4)}, [16], 16, groups=4, T=3, h_in=5, w_in=7, prelu=PR, oscale=16, res=20),
    _c("direct4_g2_k5", {S: route(K_DIRECT, 4), E: route(K_DIRECT, 4)}, [12], 8, groups=2, h_in=6, w_in=9, k=5),
    _c("direct1_dw_c6", {S: route(K_DIRECT, 1), E: route(K_DIRECT, 1)}, [6], 6, groups=6, T=3, h_in=5, w_in=9, prelu=PR2, oscale=0, res=6),
    _c("direct1_dw_unaligned", {S: route(K_DIRECT, 1), E: route(K_DIRECT, 1)}, [8], 8, groups=8, h_in=4, w_in=5, cs_extra=(1,), in_off=(1,)),
    _c("direct1_g3_c9", {S: route(K_DIRECT, 1), E: route(K_DIRECT, 1)}, [9], 9, groups=3, h_in=3, w_in=4, oscale=9, res=9),
]
for _i, _cs in enumerate(CASES):
    _cs.seed = 1000 + 17 * _i

NC_WAIVED = "LayerNorm on load at mean / std = 1000: the kernel's own fp32 mean (16 u * 1000 relative) is within 8x of a bf16 product's error"


def for_mode(case: Case, mode: str) -> Case:
    """The row as run in one arithmetic: the operands that exist in the split kernels only (csum, rscale) are dropped from exact runs."""
    return case if mode == "split" else replace(case, csum=None, rscale=False)


def pointer_model(case: Case):
    """Fake device addresses with the alignment the GPU test's tensors have: every tensor its own 256-byte aligned allocation, views offset
    by their element offset.  Only sn32_conv2d_route reads them (never dereferenced)."""
    base = [0x10000000 * (i + 1) for i in range(16)]
    return {
        "in": [base[i] + 4 * case.in_off_(i) for i in range(len(case.cins))],
        "w": base[4], "bias": base[5], "oscale": base[6], "res": base[7], "out": base[8] + 4 * case.out_off, "wsplit": base[9],
        "iscale": base[10], "rscale": base[11], "ln_w": base[12], "ln_b": base[13], "csum": base[14], "sc": base[15],
    }


def fill_desc(L, case: Case, mode: str, ptr: Dict[str, object], strides: Dict[str, int]):
    """sn32_conv_desc of a case; ptr: addresses (ints), strides: oscale / iscale / rscale row strides."""
    d = L.Conv32Desc()
    for i, c in enumerate(case.cins):
        d.inp[i], d.c_in[i], d.cs_in[i] = ptr["in"][i], c, case.cs_in(i)
    d.n_in, d.T, d.h_in, d.w_in, d.in_mode = len(case.cins), case.T, case.h_in, case.w_in, case.in_mode
    d.k, d.stride, d.pad, d.groups, d.h_out, d.w_out, d.c_out = case.k, case.stride, case.p, case.groups, case.h_out, case.w_out, case.c_out
    d.w = ptr["w"]
    d.bias = ptr["bias"] if case.bias else None
    d.act, d.prelu = (1, case.prelu) if case.prelu is not None else (0, 0.0)
    if case.oscale is not None:
        d.oscale, d.oscale_stride = ptr["oscale"], strides["oscale"]
    if case.res is not None:
        d.res, d.cs_res = ptr["res"], case.res
    d.out, d.cs_out, d.out_mode = ptr["out"], case.cs_out if case.out_mode != 2 else 0, case.out_mode
    if case.out_mode == 2:
        d.nchw_dtype, d.sc = case.nchw_dtype, ptr["sc"]
    if mode == "split":
        d.wsplit = ptr["wsplit"]
    if case.iscale:
        d.iscale, d.iscale_stride = ptr["iscale"], strides["iscale"]
    if case.rscale:
        d.rscale, d.rscale_stride = ptr["rscale"], strides["rscale"]
    if case.ln is not None:
        d.ln_w, d.ln_b = ptr["ln_w"], ptr["ln_b"]
    if case.csum is not None:
        d.csum, d.csum_cpad = ptr["csum"], case.csum
    return d


def row_stride(c: int) -> int:
    return (c + 3) // 4 * 4 + 4


def fake_strides(case: Case) -> Dict[str, int]:
    return {"oscale": 0 if case.oscale == 0 else (case.oscale or 0), "iscale": row_stride(sum(case.cins)), "rscale": row_stride(case.c_out)}


# ---- operands and the float64 reference ------------------------------------------------------------------------------------------------

def make_operands(case: Case) -> Dict[str, object]:
    """fp32 CPU operands of a case (deterministic per case)."""
    g = torch.Generator().manual_seed(case.seed)
    cin = sum(case.cins)
    T, hs, ws = case.T, case.hs, case.ws
    ops: Dict[str, object] = {}
    xs = []
    for i, c in enumerate(case.cins):
        x = torch.randn((T, hs, ws, case.cs_in(i)), generator=g)
        if case.ln:                                          # large-mean LayerNorm input: mean / std = case.ln per pixel
            x = x + case.ln * (1.0 + 0.1 * torch.rand((T, hs, ws, 1), generator=g))
        xs.append(x.float())
    ops["xs"] = xs
    fan = cin // case.groups * case.k * case.k
    ops["w"] = (torch.randn((case.c_out, cin // case.groups, case.k, case.k), generator=g) / math.sqrt(fan)).float()
    ops["bias"] = (0.5 * torch.randn(case.c_out, generator=g)).float() if case.bias else None
    if case.oscale is not None:
        rows = 1 if case.oscale == 0 else T
        ops["oscale_st"] = 0 if case.oscale == 0 else case.oscale
        ops["oscale"] = (0.5 + torch.rand((rows, max(case.oscale, case.c_out)), generator=g) + torch.arange(rows).view(-1, 1)).float()
    if case.iscale:
        ops["iscale"] = (0.25 + torch.rand((T, row_stride(cin)), generator=g) + 0.75 * torch.arange(T).view(-1, 1)).float()
    if case.rscale:
        ops["rscale"] = (0.25 + torch.rand((T, row_stride(case.c_out)), generator=g) + 0.5 * torch.arange(T).view(-1, 1)).float()
    if case.res is not None:
        r = torch.randn((T, case.h_out, case.w_out, case.res), generator=g)
        ops["res"] = (r + 3.0 * torch.arange(T).view(-1, 1, 1, 1)).float()     # per-frame offset: a wrong frame index shows
    if case.ln is not None:
        ops["ln_w"] = (1.0 + 0.5 * torch.randn(cin, generator=g)).float()
        ops["ln_b"] = (0.3 * torch.randn(cin, generator=g)).float()
    if case.out_mode == 2:
        dt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[case.nchw_dtype]
        ops["sc"] = torch.rand((T, case.c_out, case.h_out, case.w_out), generator=g).to(dt)
    return ops


def _ln64(x, w, b):
    mu = x.mean(1, keepdim=True)
    var = (x - mu).pow(2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-6) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1), mu, var


def is_split(r: int) -> bool:
    return (r >> 16) in (K_1X1, K_SPLIT, K_SPLIT_G8)


def eps_of(case: Case, r: int) -> float:
    """the analytic start of the per-element bound (module docstring)"""
    n = case.n_products
    return (3e-5 + (3 * math.ceil(n / 32) + 8) * U) if is_split(r) else (n + 8) * U


def reference(case: Case, ops: Dict[str, object], r: int, bf16_products: bool = False):
    """(ref, tol, M): float64 reference of the case on route r (NHWC for out_mode 0 / 1, NCHW for 2), its per-element tolerance and M.  bf16_products: the same op
    with bf16(x_eff) * bf16(w) products (the negative control of the split routes)."""
    d = torch.float64
    T = case.T
    xs = [x[..., case.in_off_(i): case.in_off_(i) + c].permute(0, 3, 1, 2).to(d) for i, (x, c) in enumerate(zip(ops["xs"], case.cins))]
    x = torch.cat(xs, 1)
    if case.iscale:
        x = x * ops["iscale"][:, :x.shape[1]].to(d).view(T, -1, 1, 1)
    ax = x.abs()
    delta = None
    if case.ln is not None:
        lw, lb = ops["ln_w"].to(d), ops["ln_b"].to(d)
        x0 = x
        x, mu, var = _ln64(x, lw, lb)
        rstd = 1.0 / torch.sqrt(var + 1e-6)
        delta = 16 * U * (ax.mean(1, keepdim=True) + (x0 - mu).abs()) * rstd * lw.abs().view(1, -1, 1, 1) + 2 * U * lb.abs().view(1, -1, 1, 1)
        ax = x.abs()
    if case.in_mode == 1:
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        ax = F.interpolate(ax, scale_factor=2, mode="bilinear", align_corners=False)
    w = ops["w"].to(d)
    if bf16_products:
        x = x.float().to(torch.bfloat16).to(d)
        w = ops["w"].to(torch.bfloat16).to(d)
    a = F.conv2d(x, w, stride=case.stride, padding=case.p, groups=case.groups)
    m = F.conv2d(ax, w.abs(), stride=case.stride, padding=case.p, groups=case.groups)
    extra = F.conv2d(delta, w.abs(), stride=case.stride, padding=case.p, groups=case.groups) if delta is not None else torch.zeros_like(m)
    if ops.get("bias") is not None:
        b = ops["bias"].to(d).view(1, -1, 1, 1)
        a, m = a + b, m + b.abs()
    if case.prelu is not None:
        a = torch.where(a >= 0, a, a * case.prelu)
        sl = max(1.0, abs(case.prelu))
        m, extra = m * sl, extra * sl
    if case.oscale is not None:
        os_ = ops["oscale"][:, :case.c_out].to(d)
        os_ = os_.expand(T, -1) if os_.shape[0] == 1 else os_
        os_ = os_.view(T, -1, 1, 1)
        a, m, extra = a * os_, m * os_.abs(), extra * os_.abs()
    eps = eps_of(case, r)
    if case.res is not None:
        r = ops["res"][..., :case.c_out].permute(0, 3, 1, 2).to(d)
        if case.rscale:
            r = r * ops["rscale"][:, :case.c_out].to(d).view(T, -1, 1, 1)
        a, m = a + r, m + r.abs()
    tol = eps * m + extra + 1e-30
    if case.out_mode == 1:
        a, tol, m = F.pixel_shuffle(a, 2), F.pixel_shuffle(tol, 2), F.pixel_shuffle(m, 2)
    if case.out_mode == 2:
        a = a + ops["sc"].to(d)
        tol = tol + {0: 0.0, 1: 2.0 ** -11, 2: 2.0 ** -8}[case.nchw_dtype] * a.abs() + (2.0 ** -25 if case.nchw_dtype == 1 else 0.0)
        return a, tol, m
    return a.permute(0, 2, 3, 1), tol.permute(0, 2, 3, 1), m.permute(0, 2, 3, 1)
