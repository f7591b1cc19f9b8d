"""The case tables of phase 1 as TWO kernels -- the chain the engine falls back to (Engine._recover, windows longer than Engine.MAX_TICKETS,
SN_PHASE1=0) -- their operands and one float64 INTERVAL contract per entry point, shared by the CPU test (tests/test_host_chain_ref.py) and the
GPU test (tests/test_gpu_chain_edges.py).  No GPU import.

  K12  sn_ln_gemm_gate    (csrc/sn_gsts2.hip, ln_gemm_gate_kernel<64|80, hw>):   g1 = bf16(F1 F2), F = dw3x3+id(a), a = fp16(W1' xn + b),
                                                                                 xn = bf16((u - mean) rstd)
  K3m  sn_dw5m_gemm_gate  (csrc/sn_gsts3.hip, dw5m_gemm_gate_kernel<8>, C = 64): g2 = bf16(b1 sigmoid(b2)), b = W2 r, r = bf16(fl32(dw5x5(g1p) ca))
  K3g  sn_grp5_gemm_gate  (csrc/sn_gsts2.hip, grp5p_gemm_gate_kernel<80, 2>):    the same with r = bf16(grp5x5(bf16(fl32(g1 ca))))
  sn_nhwc_to_planar: a layout change, held bit for bit.

Every contract takes its input AS STORED: K3's g1 is an independent bf16 operand, not a K12 output, so an interval passes through three (K12)
or two (K3) modelled roundings and not the six stages of the fused reference.  The method is phase1_cases.py's (Arith: "interval" / "point" /
"exact"); what differs per stage, read off the kernels:
  K12
  1 LayerNorm in fp32, two passes over the registers.  A lane sums its 8 KS values as packed pairs (4 KS adds per half, the first onto 0), adds the
    halves, sum_rows4 adds twice more: no path through the reduction is longer than DEPTH = 4 KS + 3 additions, and an error bound of a summation is
    (longest path) u sum |.| whatever the order.  With u = 2^-24, A = mean |v|, z = var + 1e-6 the half-width of xn is that of phase1_cases with K - 1
    replaced by DEPTH:
        mean~ = fl(S~ fl(1/K))                     em = DEPTH u A + 2 u |mean|
        d~ = fl(v - mean~)                         ed = em + u (|d| + em)
        q~ = sum of FMAs, all terms >= 0           |q~ - q| <= eq + (DEPTH + 1) u q,  eq = sum (2 |d| ed + ed^2)
        z~ = fl(fl(q~ fl(1/K)) + 1e-6f)            relative ez = eq / (K z) + (DEPTH + 4) u
        rstd~ = 1.0f / sqrtf(z~)                   a square root and a division, correctly rounded or 1 ulp each: er = (1 - ez)^-1/2 - 1 + 2^-22
        xn~ = fl(d~ rstd~)                         |xn~ - xn| <= rstd (ed (1 + er) + |d| (er + u))
    and where the fp32 sum is provably exact (the offset and the constant pixels) mean~ and d~ are modelled operation by operation, plain and
    contracted, as there.  Both ends to bf16.  The padding k-slots of the 80-channel variants are zero in both passes: they add nothing.
  2 1x1 on the bf16 MFMA with the fp32 bias as the accumulator's initial value: widened by (K + 8) u M, M = sum |W| |xn| + |b| (the convention of
    tests/bf16_conv_cases.py); ends to fp16 (pack_h2).  `a` is ZERO outside the image: the 3x3's zero padding applies to `a`, the ring carries no bias.
  3 3x3 + identity: nine v_pk_fma_f16 from 0, taps row-major (ty outer), fp16 weights, no 2^-4 on this path.  An FMA onto 0 is a rounded product,
    so phase1_cases.stencil3 is this stage as it stands.  No widening.
  4 gate: the fp32 product of two fp16 values is exact; g1 is the bf16 rounding of the interval product.  Pool rows (pool != NULL; the denoisers'
    inner CALayer2): the fp32 sum of the UN-ROUNDED products of a 64-pixel group (two tile rows of 32), inside pixels only (outside ones enter as
    0): row_sum16 and two shuffles are 6 additions on every path; n = 7 (one more for the second-order terms).  Row 4 (tyi ntx + txi) + pg of
    sn_lngate_blocks(h, w) rows per frame.
  5 layout: g1_blocked 0 NHWC; 2 (C = 64) [T][h][C][sn_planar_pitch(w)] with +0 in the columns w .. wr - 1; the same bits in both.
  K3m
  1 acc = Toeplitz bf16 MFMA over the 25 real taps of bf16(5x5 + 3x3 + id) (prep.pack_dw5 -> prep.pack_toeplitz; the band's zero slots add nothing):
    widened by (25 + 8) u M; r = bf16(fl32(acc ca_in[t][c])): the scale meets the accumulator BEFORE the rounding; ca_in == NULL is 1.
  2 second 1x1, bf16 MFMA: (C + 8) u M; v = b1 rcp(1 + __expf(-b2)): widened relatively by (3 + |b2|) 2^-23 (exp 1 ulp and the scaling of its
    argument, the addition, rcp) plus the product's 2^-24, the convention of sections 3.22 / 3.24; g2 = bf16(v).  A gate product's dynamic range
    puts b2 near -90 at a few elements: an fp32 result below 2^-100 extends its interval to 0 (Arith.rel), a g2 end inside (0, 2^-126) moves out to
    2^-126 (the bf16 store rounds to a subnormal or flushes), and a pool row gets n 2^-126 of absolute slack for subnormal partial sums.
  3 pool row of tile `rem`: the sum of the un-rounded v over the tile's inside pixels: 4 per-lane adds, row_sum16 (4), eight partials (8): n = 17.
  K3g
  the operand is bf16(fl32(g1 ca_in)), formed at staging: here the scale comes BEFORE the conv.  Grouped MFMA over 25 taps x 8 input channels:
  (200 + 8) u M, r to bf16; the tail is K3m's; pool row per 32 x 4 tile: 4 per-lane adds, row_sum16 (4), red[tid] + red[C + tid] (1): n = 10.
Weights: the fp32 expressions of prep.pack_ln_gemm, pack_dw3_gate -> pk_f16_words, pack_dw5 -> pack_toeplitz, pack_grouped_frag, pack_gate_gemm
folded and rounded here (folded), handed to the kernels through those packers (packed); tests/test_host_chain_ref.py compares the two bit for bit.

Operand families: (a) dense -- phase1_cases._special for x, hw, halo; K3's g1 = bf16(a1 a2) of two such tensors; ca_in per frame and channel with
both signs and 1 in 8 exact zeros.  (b) impulses -- g1 zero but one pixel per frame (power-of-two amplitudes) at the corners, on both sides of
every tile seam and inside: every g2 element outside the pixel's 5 x 5 footprint is +0 bit for bit; K12: one non-constant pixel per frame in a
constant image.  (c) hot -- w1 times HOT_GAIN[C], the smallest power of two at which phase1_cases.reference trips its fp16 range assertion while
this chain's `a` and stencil partials stay below 2^15.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import gsts_edge_cases as GE
import phase1_cases as PC
from phase1_cases import Arith, F32, F64, U, r16, rbf      # noqa: F401  (re-exported for the two tests)
from shiftnet_amd import prep

EINVAL = GE.EINVAL
VARIANT_WRAP = GE.VARIANT_WRAP
K12_TH, K12_TW = 8, 32
K3_TILE = {64: (8, 64), 80: (4, 32)}        # (rows, columns) of a K3m / K3g tile
N_POOL_K12 = 7
N_POOL_K3 = {64: 17, 80: 10}
TINY = 2.0 ** -126                          # the smallest normal fp32 / bf16 magnitude
HOT_GAIN = {64: 256.0, 80: 256.0}            # asserted to be the smallest such power of two by tests/test_host_chain_ref.py


def planar_pitch(w: int) -> int:
    return (w + 7) & ~7


# ---- the tables -------------------------------------------------------------------------------------------------------------------------

@dataclass
class K12Case(PC.P1Case):
    pool: bool = False
    family: str = "dense"                   # "dense" | "impulse" | "hot"

    @property
    def gain(self):
        return HOT_GAIN[self.C] if self.family == "hot" else 1.0

    @property
    def layouts(self):
        return (0, 2) if self.C == 64 else (0,)


def _k12_rows(C: int) -> List[K12Case]:
    v = VARIANT_WRAP[C]
    k = lambda *a, **kw: K12Case(f"c{C}_{a[0]}", C, *a[1:], **kw)      # noqa: E731
    rows = [
        k("one_pixel_1x1x1_m0", 1, 1, 1, 0, 0, oracle=True, pool=True),                     # smaller than the ring
        k("small_2x5x9_m1", 2, 5, 9, 1, v, oracle=True),
        k("exact_tile_1x8x32_m0", 1, 8, 32, 0, 0, oracle=True),
        k("slivers_1x9x33_m0", 1, 9, 33, 0, 0, oracle=True, pool=True),                     # four tiles with one-pixel slivers
        k("3x3_tiles_2x17x70_m2", 2, 17, 70, 2, v, pool=True),                              # 18 tile rows x frames: the XCD walk of sn_xcd_tiles
        k("frame_range_4x12x70_m1", 4, 12, 70, 1, v, t0=1, nt=2, pool=True),
        k("clips_of_2_4x12x70_m1", 4, 12, 70, 1, v, clip=2),
        k("clips_of_2_4x12x70_m2", 4, 12, 70, 2, 1 - v, clip=2, pool=True),
        k("halo_3x12x70_m1", 3, 12, 70, 1, 2),
        k("halo_3x12x70_m2", 3, 12, 70, 2, 2, pool=True),
        k("other_wrap_2x16x16_m1", 2, 16, 16, 1, 1 - v),
        k("hot_2x9x33_m1", 2, 9, 33, 1, v, family="hot", pool=True),
        k("impulse_13x17x70_m0", 13, 17, 70, 0, 0, family="impulse"),
    ]
    if C == 64:                             # the planar layout's pitches: wr = 16, 40, 64, 72 (70 is in the rows above)
        rows += [k("pitch_1x3x9_m0", 1, 3, 9, 0, 0), k("pitch_1x3x64_m0", 1, 3, 64, 0, 0, pool=True)]
    return rows


@dataclass
class K3Case:
    id: str
    C: int
    T: int
    h: int
    w: int
    family: str = "dense"                   # "dense" | "impulse"
    walk: bool = False                      # tiles > CUs: a workgroup walks from frame to frame
    seed: int = 0

    def with_frames(self, T: int) -> "K3Case":
        return K3Case(self.id, self.C, T, self.h, self.w, self.family, self.walk, self.seed)

    @property
    def tiles_per_frame(self):
        th, tw = K3_TILE[self.C]
        return -(-self.h // th) * -(-self.w // tw)


K3M_ROWS = [
    K3Case("c64_one_pixel_1x1x1", 64, 1, 1, 1),                             # smaller than the halo
    K3Case("c64_exact_tile_1x8x64", 64, 1, 8, 64),
    K3Case("c64_slivers_1x9x65", 64, 1, 9, 65),
    K3Case("c64_3x3_tiles_2x17x130", 64, 2, 17, 130),
    K3Case("c64_8_tiles_4x8x128", 64, 4, 8, 128),                           # nxcd = 8, wpx = 1
    K3Case("c64_2x2_tiles_2x12x70", 64, 2, 12, 70),                           # 2 x 4 tiles (nxcd = 1 is the 4 and 18 tiles of the rows above); w = 70: the planar pad columns 70, 71
    K3Case("c64_walk_44x17x65", 64, 44, 17, 65, walk=True),                 # 264 tiles > 256 CUs
    K3Case("c64_walk_short_last_segment_46x17x65", 64, 46, 17, 65, walk=True),      # 276 = 7 x 35 + 31: one workgroup of the last XCD starts past its end
    K3Case("c64_impulse_13x17x130", 64, 13, 17, 130, family="impulse"),
]
K3G_ROWS = [
    K3Case("c80_one_pixel_1x1x1", 80, 1, 1, 1),
    K3Case("c80_exact_tile_1x4x32", 80, 1, 4, 32),
    K3Case("c80_slivers_1x5x33", 80, 1, 5, 33),
    K3Case("c80_3x3_tiles_2x9x70", 80, 2, 9, 70),
    K3Case("c80_8_tiles_2x8x64", 80, 2, 8, 64),
    K3Case("c80_walk_66x5x33", 80, 66, 5, 33, walk=True),                   # 264 tiles
    K3Case("c80_walk_short_last_segment_67x5x33", 80, 67, 5, 33, walk=True),        # 268 = 7 x 34 + 30
    K3Case("c80_impulse_13x9x70", 80, 13, 9, 70, family="impulse"),
]
K12_CASES: List[K12Case] = _k12_rows(64) + _k12_rows(80)
K3_CASES: List[K3Case] = K3M_ROWS + K3G_ROWS
for _i, _c in enumerate(K12_CASES):
    _c.seed = 12000 + 47 * _i
for _i, _c in enumerate(K3_CASES):
    _c.seed = 14000 + 53 * _i
K12_BY_ID = {c.id: c for c in K12_CASES}
K3_BY_ID = {c.id: c for c in K3_CASES}
CHAIN_SHAPE = (2, 17, 70)                   # the chain check: K12 -> sn_ca_mlp -> K3 on the device's own tensors
PLANAR_W = (1, 7, 8, 9, 63, 64, 65, 129)
PLANAR_C = (8, 64, 80, 128)


def walk_frames(c: K3Case, ncu: int) -> int:
    """frames of a walk row on a device with ncu CUs: the table's where that already gives more tiles than CUs, else ncu // tiles + 2"""
    return c.T if c.T * c.tiles_per_frame > ncu else ncu // c.tiles_per_frame + 2


def impulse_positions(h: int, w: int, th: int, tw: int) -> List[Tuple[int, int]]:
    """(y, x) of the 13 impulse frames: the corners, both sides of the first tile seam in x and in y (alone and together), one interior pixel"""
    ym, xm = th // 2, tw // 2
    pos = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    pos += [(ym, tw - 1), (ym, tw), (th - 1, xm), (th, xm)]
    pos += [(th - 1, tw - 1), (th - 1, tw), (th, tw - 1), (th, tw)]
    pos += [(th + 3, tw + 5)]
    assert all(0 <= y < h and 0 <= x < w for y, x in pos)
    return pos


# ---- operands ---------------------------------------------------------------------------------------------------------------------------

def _scale(g, T: int, C: int) -> torch.Tensor:
    s = (0.25 + 1.5 * torch.rand((T, C), generator=g)) * GE._sgn(g, (T, C))
    s[torch.rand((T, C), generator=g) < 1.0 / 8] = 0.0
    return s.float()


def k12_operands(c: K12Case) -> Dict[str, object]:
    """phase1_cases.operands (x, halo, hw, the raw fp32 weights, cls); family "hot": w1 times the gain; "impulse": every pixel constant over its
    channels but one per frame, which keeps its dense values"""
    ops = PC.operands(c)
    ops["w1"] = ops["w1"] * c.gain
    if c.family == "impulse":
        assert c.mode == 0
        g = torch.Generator().manual_seed(c.seed + 7)
        const = (torch.randn((c.T, c.h, c.w, 1), generator=g) * torch.exp2(torch.rand((c.T, c.h, c.w, 1), generator=g) * 6.0 - 3.0)).to(torch.bfloat16)
        x = const.expand(c.T, c.h, c.w, c.C).clone()
        for t, (py, px) in enumerate(impulse_positions(c.h, c.w, K12_TH, K12_TW)):
            x[t, py, px] = GE._act(g, (c.C,))
        ops["x"] = x
        ops["impulse"] = impulse_positions(c.h, c.w, K12_TH, K12_TW)
    return ops


def k3_operands(c: K3Case) -> Dict[str, object]:
    """g1 bf16 [T][h][w][C] (dense: bf16(a1 a2) of two phase1_cases._special tensors, a gate product's dynamic range; impulse: one pixel per
    frame), ca fp32 [T][C], the raw fp32 weights w_rep5, w_rep3, w2"""
    g = torch.Generator().manual_seed(c.seed)
    C = c.C
    ops: Dict[str, object] = {}
    if c.family == "impulse":
        th, tw = K3_TILE[C]
        pos = impulse_positions(c.h, c.w, th, tw)
        assert c.T == len(pos)
        g1 = torch.zeros((c.T, c.h, c.w, C))
        for t, (py, px) in enumerate(pos):
            g1[t, py, px] = GE._sgn(g, C) * torch.exp2(torch.randint(-6, 7, (C,), generator=g).float())
        ops["g1"], ops["impulse"] = g1.to(torch.bfloat16), pos
    else:
        pos = PC._positions(g, c.h, c.w)
        a1, a2 = PC._special(g, (c.T, c.h, c.w, C), pos), PC._special(g, (c.T, c.h, c.w, C), pos)
        ops["g1"] = (a1.float() * a2.float()).to(torch.bfloat16)
    ops["ca"] = _scale(g, c.T, C)
    cig = 1 if C == 64 else 8
    ops["w_rep5"] = (torch.randn((C, cig, 5, 5), generator=g) / math.sqrt(25.0 * cig)).float()
    ops["w_rep3"] = (torch.randn((C, cig, 3, 3), generator=g) / math.sqrt(9.0 * cig)).float()
    ops["w2"] = (torch.randn((2 * C, C, 1, 1), generator=g) / math.sqrt(C)).float()
    return ops


def planar(g1: torch.Tensor) -> torch.Tensor:
    """NHWC [T][h][w][C] -> [T][h][C][planar_pitch(w)], pad columns zero: what K3m reads (built on the host: no dependence on sn_nhwc_to_planar)"""
    T, h, w, C = g1.shape
    out = torch.zeros((T, h, C, planar_pitch(w)), dtype=g1.dtype)
    out[..., :w] = g1.permute(0, 1, 3, 2)
    return out


def packed(ops: Dict[str, object]) -> Dict[str, torch.Tensor]:
    """what the kernels get, through the packers Plan.add_naf uses"""
    C = ops["w2"].shape[0] // 2
    pk: Dict[str, torch.Tensor] = {}
    if "w1" in ops:
        g = prep.pack_ln_gemm(ops["w1"], ops["ln_w"], ops["ln_b"], C)
        pk["w_ln"], pk["b_ln"] = g["wfrag"], g["bias"]
        pk["w_dw3_h2"] = prep.pk_f16_words(prep.pack_dw3_gate(ops["w_dw3"], C))
    if ops["w_rep5"].shape[1] == 8:
        pk["w_grp"] = prep.pack_grouped_frag(ops["w_rep5"], ops["w_rep3"])
    else:
        pk["w_toep5"] = prep.pack_toeplitz(prep.pack_dw5(ops["w_rep5"], ops["w_rep3"]), 5)
    pk["w_gate"] = prep.pack_gate_gemm(ops["w2"], C)
    return pk


def _tb(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def folded(ops: Dict[str, object], rounded: bool = True) -> Dict[str, np.ndarray]:
    """The matrices the kernels multiply by, float64, channels in natural order: the packers' expressions in float32 as there, rounded as they round.
    rounded False: the same foldings in float64, nothing rounded ("exact" runs).
      W1 [2C][K] bf16, b [2C] fp32;  d3 [2C][9] fp16 (identity in the centre);
      k5 [C][5][5] bf16 (C = 64) or dg [C/8][8 oc][8 ic][5][5] bf16 (C = 80), 3x3 and identity folded;  W2 [2C][C] bf16"""
    c = ops["w2"].shape[0] // 2
    fw: Dict[str, np.ndarray] = {}
    np_ = (lambda t: t.detach().float().cpu().numpy()) if rounded else (lambda t: t.detach().double().cpu().numpy())
    if "w1" in ops:
        w = np_(ops["w1"]).reshape(2 * c, -1)
        wf, b = w * np_(ops["ln_w"])[None, :], w @ np_(ops["ln_b"])
        d3 = np_(ops["w_dw3"]).reshape(2 * c, 9).copy()
        d3[:, 4] += 1.0
        fw["W1"], fw["b"] = (_tb(wf), b.astype(F64)) if rounded else (wf, b)
        fw["d3"] = torch.from_numpy(d3).to(torch.float16).to(torch.float64).numpy() if rounded else d3
    a5, a3 = np_(ops["w_rep5"]).copy(), np_(ops["w_rep3"])
    if a5.shape[1] == 8:
        a5[:, :, 1:4, 1:4] += a3
        for o in range(c):
            a5[o, o % 8, 2, 2] += 1.0
        dg = a5.reshape(c // 8, 8, 8, 5, 5)
        fw["dg"] = _tb(dg) if rounded else dg
    else:
        k = a5[:, 0]
        k[:, 1:4, 1:4] += a3[:, 0]
        k[:, 2, 2] += 1.0
        fw["k5"] = _tb(k) if rounded else k
    w2 = np_(ops["w2"]).reshape(2 * c, c)
    fw["W2"] = _tb(w2) if rounded else w2
    return fw


# ---- K12 --------------------------------------------------------------------------------------------------------------------------------

def _tree32(v: np.ndarray) -> np.ndarray:
    """fp32 butterfly sum over the last axis (a power of two): row_sum16 / sum_rows4 / the shuffles, every lane ends with the same value"""
    v = v.astype(F32)
    n = v.shape[-1]
    idx = np.arange(n)
    s = 1
    while s < n:
        v = v + v[..., idx ^ s]
        s *= 2
    return v[..., 0]


def _ln_lane_sum(v: np.ndarray, KS: int) -> np.ndarray:
    """the kernel's order: v [..., 32 KS] fp32 -> per lane group g the packed-pair sum over (s, j), the two halves added, then sum_rows4"""
    q = v.reshape(v.shape[:-1] + (KS, 4, 4, 2))                                # [s][g][j][half]
    acc = np.zeros(v.shape[:-1] + (4, 2), F32)
    for s in range(KS):
        for j in range(4):
            acc = acc + q[..., s, :, j, :]
    return _tree32(acc[..., 0] + acc[..., 1])


def layer_norm(ar: Arith, u: np.ndarray, fault: Optional[str] = None):
    """stage 1 of K12 on u [..., K] -> (lo, hi) of xn.  Point runs follow the kernel operation by operation in float32 (faults "no_eps"; "mean_ks":
    the mean over the 32 KS slots instead of K); the other runs in float64 with the half-width of the module docstring."""
    K = u.shape[-1]
    KS = (K + 31) // 32
    depth = 4 * KS + 3
    if ar.kind == "point":
        v = np.zeros(u.shape[:-1] + (32 * KS,), F32)
        v[..., :K] = u
        ck = F32(1.0) / F32(K)
        mean = (_ln_lane_sum(v, KS) * (F32(1.0) / F32(32 * KS) if fault == "mean_ks" else ck))[..., None]
        d = v - mean
        d[..., K:] = 0.0
        var = _ln_lane_sum(d * d, KS) * ck                                      # (the FMA chain's single rounding per term: inside the same bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = var if fault == "no_eps" else var + F32(1e-6)
            rstd = (F32(1.0) / np.sqrt(z.astype(F32))).astype(F32)
            y = rbf((d[..., :K] * rstd[..., None]).astype(F64))
        return y, y
    eps = float(F32(1e-6)) if ar.kind == "interval" else 1e-6
    m = u.mean(-1, keepdims=True)
    d = u - m
    z = (d * d).mean(-1, keepdims=True) + eps
    rstd = 1.0 / np.sqrt(z)
    y = d * rstd
    if ar.kind == "exact":
        return y, y
    asum = np.abs(u).sum(-1, keepdims=True)
    em = (depth * U * asum / K + 2.01 * U * np.abs(m)) * (1.0 + 2.0 ** -20)
    ed = em + U * (np.abs(d) + em)
    eq = (2.0 * np.abs(d) * ed + ed * ed).sum(-1, keepdims=True)
    ez = np.minimum(eq / (K * z) + (depth + 4) * U, 0.75)
    er = 1.0 / np.sqrt(1.0 - ez) - 1.0 + 2.0 ** -22
    hw = rstd * (ed * (1.0 + er) + np.abs(d) * (er + U)) * (1.0 + 2.0 ** -20)
    lo, hi = y - hw, y + hw
    fr, ex = np.frexp(u)                                                        # pixels whose fp32 sum is provably exact: d~ itself is modelled
    n8 = np.abs(fr * 256.0).astype(np.int64)
    quantum = np.where(n8 > 0, np.ldexp((n8 & -n8).astype(F64), ex - 8), np.inf).min(-1, keepdims=True)
    exact = (asum < 2.0 ** 24 * quantum)[..., 0]
    if exact.any():
        ue = u[exact]
        s = ue.sum(-1, keepdims=True)
        ck = F32(1.0) / F32(K)
        d_two = (ue.astype(F32) - s.astype(F32) * ck).astype(F64)
        d_fma = (ue - s * F64(ck)).astype(F32).astype(F64)
        ends = []
        for de in (d_two, d_fma):
            ye = de / np.sqrt((de * de).mean(-1, keepdims=True) + eps)
            he = np.abs(ye) * (1.0 / math.sqrt(1.0 - (depth + 4) * U) - 1.0 + 2.0 ** -22 + 2.0 * U) * (1.0 + 2.0 ** -20)
            ends += [ye - he, ye + he]
        elo, ehi = np.minimum.reduce(ends), np.maximum.reduce(ends)
        lo[exact], hi[exact] = np.maximum(lo[exact], elo), np.minimum(hi[exact], ehi)      # both statements hold: their intersection
    assert (ez < 0.5)[~exact].all(), ez.max()
    return ar.bf(lo, hi)


def k12_pool_rows(ar: Arith, p, h: int, w: int, edge: bool = False):
    """p (lo, hi) [n][h][w][C], the un-rounded gate products -> pool rows (lo, hi) [n][sn_lngate_blocks][C].  edge (negative control): a pixel
    outside the image contributes what the nearest inside pixel does instead of 0."""
    n, C = p[0].shape[0], p[0].shape[-1]
    nty, ntx = -(-h // K12_TH), -(-w // K12_TW)
    pad = ((0, 0), (0, nty * K12_TH - h), (0, ntx * K12_TW - w), (0, 0))
    lo, hi = (np.pad(q, pad, mode="edge" if edge else "constant") for q in p)
    sh = (n, nty, 4, 2, ntx, K12_TW, C)                                         # [n][tyi][pg][row of the group][txi][ox][C]
    perm = (0, 1, 4, 2, 3, 5, 6)
    lo, hi = lo.reshape(sh).transpose(perm).reshape(n, nty * ntx * 4, 64, C), hi.reshape(sh).transpose(perm).reshape(n, nty * ntx * 4, 64, C)
    if ar.kind == "point":
        q = _tree32(np.moveaxis(lo, 2, -1)).astype(F64)
        return q, q
    return ar.acc(lo.sum(2), hi.sum(2), N_POOL_K12, np.maximum(np.abs(lo), np.abs(hi)).sum(2))


def k12_frame(c: K12Case, ops, fw, ar: Arith, t: int, fault: Optional[str] = None) -> Dict[str, tuple]:
    """xn, a, F, p (the un-rounded gate product), g1 of absolute frame t, each (lo, hi) on the image.  Faults (point runs, one each): "bias_outside",
    "no_eps", "mean_ks", "same_frame", "taps_transposed", "no_identity", "gate_partner" (the partner one chunk of 4 channels on), "g1_fp16"."""
    C = c.C
    u = PC.gather(c, ops, t, fault)
    xn = layer_norm(ar, u, fault)
    lo, hi, M = PC._imatmul(xn[0], xn[1], fw["W1"])
    a = ar.h16(*ar.acc(lo + fw["b"], hi + fw["b"], c.K + 8, M + np.abs(fw["b"])))
    d3 = fw["d3"]
    if fault == "taps_transposed":
        d3 = d3.reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9)
    if fault == "no_identity":
        d3 = d3.copy()
        d3[:, 4] = r16(d3[:, 4] - 1.0)
    outside = ar.h16(fw["b"], fw["b"])[0] if fault == "bias_outside" else None
    Fe = PC.stencil3(ar, a, d3, outside)
    Fl, Fh = Fe[0][1:-1, 1:-1], Fe[1][1:-1, 1:-1]
    F2l, F2h = Fl[..., C:], Fh[..., C:]
    if fault == "gate_partner":
        F2l, F2h = np.roll(F2l, -4, -1), np.roll(F2h, -4, -1)
    p = PC._imul(Fl[..., :C], Fh[..., :C], F2l, F2h)
    g1 = ar.h16(*p) if fault == "g1_fp16" else ar.bf(*p)
    return {"xn": xn, "a": a, "F": (Fl, Fh), "p": p, "g1": g1}


def k12_reference(c: K12Case, ops, ar: Optional[Arith] = None, fw=None, fault: Optional[str] = None, want=("g1", "p")) -> Dict[str, tuple]:
    """stage -> (lo, hi) [nt][h][w][...] over c.frames; "pool" (lo, hi) [nt][rows][C] is added for rows with the pool on.  The interval run asserts
    that no modelled fp16 value (a, every partial of the nine-tap sum) exceeds 2^15: ar.max16."""
    ar = ar or Arith("interval")
    fw = fw or folded(ops, rounded=ar.kind != "exact")
    acc: Dict[str, list] = {k: [[], []] for k in want}
    for t in c.frames:
        st = k12_frame(c, ops, fw, ar, t, fault)
        for k in want:
            acc[k][0].append(st[k][0])
            acc[k][1].append(st[k][1])
    out = {k: (np.stack(v[0]), np.stack(v[1])) for k, v in acc.items()}
    if c.pool and "p" in out:
        out["pool"] = k12_pool_rows(ar, out["p"], c.h, c.w)
    if ar.kind == "interval":
        assert ar.max16 <= PC.MAX16, (c.id, ar.max16)
        assert all(np.isfinite(v[0]).all() and np.isfinite(v[1]).all() for v in out.values()), c.id
    return out


# ---- K3m / K3g --------------------------------------------------------------------------------------------------------------------------

def _r32(ar: Arith, lo, hi):
    return (lo, hi) if ar.kind == "exact" else (lo.astype(F32).astype(F64), hi.astype(F32).astype(F64))


def dw5(ar: Arith, g, k5):
    """K3m stage 1 before the scale: g (lo, hi) [h][w][C] (zero outside the image) -> acc (lo, hi), widened by (25 + 8) u M"""
    h, w, _ = g[0].shape
    if g[0] is g[1]:                                                            # a stored operand: one value, no interval product
        pl = np.pad(g[0], ((2, 2), (2, 2), (0, 0)))
        a, M = np.zeros_like(g[0]), np.zeros_like(g[0])
        for dy in range(5):
            for dx in range(5):
                t = pl[dy:dy + h, dx:dx + w] * k5[:, dy, dx]
                a += t
                M += np.abs(t)
        return ar.acc(a, a, 25 + 8, M)
    pl, ph = np.pad(g[0], ((2, 2), (2, 2), (0, 0))), np.pad(g[1], ((2, 2), (2, 2), (0, 0)))
    pa = np.maximum(np.abs(pl), np.abs(ph))
    lo, hi, M = np.zeros_like(g[0]), np.zeros_like(g[0]), np.zeros_like(g[0])
    for dy in range(5):
        for dx in range(5):
            sl, sh = PC._iscale(pl[dy:dy + h, dx:dx + w], ph[dy:dy + h, dx:dx + w], k5[:, dy, dx])
            lo, hi, M = lo + sl, hi + sh, M + pa[dy:dy + h, dx:dx + w] * np.abs(k5[:, dy, dx])
    return ar.acc(lo, hi, 25 + 8, M)


def grp5(ar: Arith, g, dg):
    """K3g's grouped conv: g (lo, hi) [h][w][C] -> r (lo, hi) bf16, widened by (200 + 8) u M"""
    h, w, C = g[0].shape
    ng = dg.shape[0]
    pl, ph = np.pad(g[0], ((2, 2), (2, 2), (0, 0))), np.pad(g[1], ((2, 2), (2, 2), (0, 0)))
    kp, kn, ka = np.maximum(dg, 0.0), np.minimum(dg, 0.0), np.abs(dg)
    sh = (h, w, ng, 8)
    lo, hi, M = np.zeros(sh), np.zeros(sh), np.zeros(sh)
    if g[0] is g[1]:                                                            # a stored operand: one value, no interval product
        for dy in range(5):
            for dx in range(5):
                sl = pl[dy:dy + h, dx:dx + w].reshape(sh)
                lo += np.einsum("hwgi,goi->hwgo", sl, dg[:, :, :, dy, dx])
                M += np.einsum("hwgi,goi->hwgo", np.abs(sl), ka[:, :, :, dy, dx])
        return ar.bf(*ar.acc(lo.reshape(h, w, C), lo.reshape(h, w, C), 200 + 8, M.reshape(h, w, C)))
    for dy in range(5):
        for dx in range(5):
            sl, su = pl[dy:dy + h, dx:dx + w].reshape(sh), ph[dy:dy + h, dx:dx + w].reshape(sh)
            e = lambda v, k: np.einsum("hwgi,goi->hwgo", v, k[:, :, :, dy, dx])      # noqa: E731
            lo += e(sl, kp) + e(su, kn)
            hi += e(su, kp) + e(sl, kn)
            M += e(np.maximum(np.abs(sl), np.abs(su)), ka)
    return ar.bf(*ar.acc(lo.reshape(h, w, C), hi.reshape(h, w, C), 200 + 8, M.reshape(h, w, C)))


def gate2(ar: Arith, r, W2, C: int, swapped: bool = False):
    """second 1x1 and SimpleGate2 -> ((lo, hi) of the un-rounded v, (lo, hi) of g2).  swapped (negative control): b2 sigmoid(b1)"""
    lo, hi, M = PC._imatmul(r[0], r[1], W2)
    lo, hi = ar.acc(lo, hi, C + 8, M)
    b1, b2 = (lo[..., :C], hi[..., :C]), (lo[..., C:], hi[..., C:])
    if swapped:
        b1, b2 = b2, b1
    with np.errstate(over="ignore"):
        s_lo, s_hi = 1.0 / (1.0 + np.exp(-b2[0])), 1.0 / (1.0 + np.exp(-b2[1]))
    v = PC._imul(b1[0], b1[1], s_lo, s_hi)
    rho = (3.0 + np.maximum(np.abs(b2[0]), np.abs(b2[1]))) * 2.0 ** -23 + 2.0 ** -24
    v = ar.rel(v[0], v[1], rho)
    g2 = ar.bf(*v)
    if ar.kind == "interval":                                                   # below bf16's normal range the store rounds to a subnormal or flushes
        g2 = (np.where((g2[0] < 0) & (g2[0] > -TINY), -TINY, g2[0]), np.where((g2[1] > 0) & (g2[1] < TINY), TINY, g2[1]))
    return v, g2


def _k3_order_sum(C: int, tile: np.ndarray) -> np.ndarray:
    """the kernels' order of a pool row in fp32: tile [th tw][C] (outside pixels 0; an addition of 0 is exact) -> [C]"""
    npart = 8 if C == 64 else 2
    q = tile.astype(F32).reshape(npart, 4, 16, C)                               # tp = 64 part + 16 n + p
    lane = np.zeros((npart, 16, C), F32)
    for n in range(4):
        lane = lane + q[:, n]
    part = _tree32(np.moveaxis(lane, 1, -1))                                     # [part][C]
    out = np.zeros(C, F32)
    for k in range(npart):
        out = out + part[k]
    return out


def k3_pool_rows(ar: Arith, C: int, v, h: int, w: int, edge: bool = False, shift: int = 0):
    """v (lo, hi) [n][h][w][C] un-rounded -> pool rows (lo, hi) [n][tiles per frame][C]: per tile the sum over its inside pixels, widened by
    n u sum |.|.  Negative controls: edge (an outside pixel contributes what the nearest inside pixel does), shift (the row is written at rem + shift)."""
    n = v[0].shape[0]
    th, tw = K3_TILE[C]
    nty, ntx = -(-h // th), -(-w // tw)
    pad = ((0, 0), (0, nty * th - h), (0, ntx * tw - w), (0, 0))
    lo, hi = (np.pad(q, pad, mode="edge" if edge else "constant") for q in v)
    sh, perm = (n, nty, th, ntx, tw, C), (0, 1, 3, 2, 4, 5)
    lo, hi = lo.reshape(sh).transpose(perm).reshape(n, nty * ntx, th * tw, C), hi.reshape(sh).transpose(perm).reshape(n, nty * ntx, th * tw, C)
    if ar.kind == "point":
        q = np.stack([np.stack([_k3_order_sum(C, lo[i, r]) for r in range(nty * ntx)]) for i in range(n)]).astype(F64)
        q = np.roll(q, shift, 1)
        return q, q
    lo, hi = ar.acc(lo.sum(2), hi.sum(2), N_POOL_K3[C], np.maximum(np.abs(lo), np.abs(hi)).sum(2))
    return (lo - N_POOL_K3[C] * TINY, hi + N_POOL_K3[C] * TINY) if ar.kind == "interval" else (lo, hi)      # fp32 subnormal partial sums


def k3_frame(C: int, g1: np.ndarray, ca: Optional[np.ndarray], fw, ar: Arith, fault: Optional[str] = None, seam: Optional[Tuple[int, int]] = None):
    """one frame: g1 [h][w][C] float64 (bf16 values as stored), ca [C] or None -> r, v, g2 as (lo, hi).  Faults (point runs, one each):
    "k5_transposed", "k3_one_tap_off" (fw already holds the misfolded stencil), "pad_column" (C = 64: the planar pad column w holds g1's column
    w - 1), "seam_x" / "seam_y" (seam = (row, column) of the second tile: its first column / row sees zeros left of / above it),
    "scale_after" (C = 80: the scale meets the conv's result instead of its operand), "gate_swapped"."""
    h, w, _ = g1.shape
    one = np.ones(C) if ca is None else ca
    g = (g1, g1)
    if C == 64:
        k5 = fw["k5"].transpose(0, 2, 1) if fault == "k5_transposed" else fw["k5"]
        src = g
        if fault == "pad_column":
            ext = np.concatenate((g1, g1[:, -1:]), 1)                           # the stencil of the last two columns reaches it
            acc = dw5(ar, (ext, ext), k5)
            acc = (acc[0][:, :w], acc[1][:, :w])
        else:
            acc = dw5(ar, src, k5)
        if fault in ("seam_x", "seam_y"):
            y0, x0 = seam
            cut = g1.copy()
            if fault == "seam_x":
                cut[:, :x0] = 0.0
            else:
                cut[:y0] = 0.0
            ac = dw5(ar, (cut, cut), k5)
            sel = np.zeros((h, w, 1), bool)
            if fault == "seam_x":
                sel[:, x0] = True
            else:
                sel[y0] = True
            acc = (np.where(sel, ac[0], acc[0]), np.where(sel, ac[1], acc[1]))
        r = ar.bf(*_r32(ar, *PC._iscale(acc[0], acc[1], one)))
    else:
        dg = fw["dg"].transpose(0, 1, 2, 4, 3) if fault == "k5_transposed" else fw["dg"]
        if fault == "scale_after":
            acc = grp5(Arith("exact") if ar.kind == "exact" else _NoBf(ar), g, dg)
            r = ar.bf(*_r32(ar, *PC._iscale(acc[0], acc[1], one)))
        else:
            sp = g1 if ca is None else g1 * one                                 # the scaled operand is a point: one fp32 product, one bf16 rounding
            sp = sp if ca is None or ar.kind == "exact" else rbf(sp.astype(F32).astype(F64))
            s = (sp, sp)
            r = grp5(ar, s, dg)
            if fault in ("seam_x", "seam_y"):
                y0, x0 = seam
                cl, ch = s[0].copy(), s[1].copy()
                sel = np.zeros((h, w, 1), bool)
                if fault == "seam_x":
                    cl[:, :x0], ch[:, :x0] = 0.0, 0.0
                    sel[:, x0] = True
                else:
                    cl[:y0], ch[:y0] = 0.0, 0.0
                    sel[y0] = True
                rc = grp5(ar, (cl, ch), dg)
                r = (np.where(sel, rc[0], r[0]), np.where(sel, rc[1], r[1]))
    v, g2 = gate2(ar, r, fw["W2"], C, swapped=fault == "gate_swapped")
    return {"r": r, "v": v, "g2": g2}


class _NoBf:
    """an Arith whose bf16 rounding is the identity (the "scale_after" control rounds after its scale)"""

    def __init__(self, ar: Arith):
        self.ar, self.kind = ar, ar.kind

    def bf(self, lo, hi):
        return lo, hi

    def acc(self, *a):
        return self.ar.acc(*a)


def k3_reference(C: int, g1: torch.Tensor, ca: Optional[torch.Tensor], ops=None, ar: Optional[Arith] = None, fw=None, fault: Optional[str] = None,
                 seam=None, want=("g2", "v"), ca_shift: int = 0) -> Dict[str, tuple]:
    """stage -> (lo, hi) [T][h][w][C] from the stored operands g1 bf16 NHWC [T][h][w][C] and ca fp32 [T][C] (None: no scale); "pool" [T][tiles][C]
    from "v".  ca_shift (negative control): frame t is scaled by ca[t + ca_shift]."""
    ar = ar or Arith("interval")
    fw = fw or folded(ops, rounded=ar.kind != "exact")
    T = g1.shape[0]
    g = g1.to(torch.float64).numpy()
    s = None if ca is None else ca.to(torch.float64).numpy()
    acc: Dict[str, list] = {k: [[], []] for k in want}
    for t in range(T):
        st = k3_frame(C, g[t], None if s is None else s[(t + ca_shift) % T], fw, ar, fault, seam)
        for k in want:
            acc[k][0].append(st[k][0])
            acc[k][1].append(st[k][1])
    out = {k: (np.stack(v[0]), np.stack(v[1])) for k, v in acc.items()}
    if "v" in out:
        out["pool"] = k3_pool_rows(ar, C, out["v"], g1.shape[1], g1.shape[2])
    if ar.kind == "interval":
        assert all(np.isfinite(v[0]).all() and np.isfinite(v[1]).all() for v in out.values())
    return out


def footprint(c: K3Case, pos) -> np.ndarray:
    """[T][h][w] bool: inside the 5 x 5 footprint of frame t's impulse"""
    yy, xx = np.mgrid[0:c.h, 0:c.w]
    return np.stack([(np.abs(yy - py) <= 2) & (np.abs(xx - px) <= 2) for py, px in pos])


# ---- the persistent walk of K3m / K3g, restated ---------------------------------------------------------------------------------------------

def walk(ntiles: int, grid: int) -> List[List[int]]:
    """tiles of every workgroup of a launch of `grid` workgroups, in its order: nxcd / wpx / seg / seg0 / seg1 of dw5m_gemm_gate_kernel and
    grp5p_gemm_gate_kernel"""
    nxcd = 8 if grid % 8 == 0 else 1
    wpx, seg = grid // nxcd, -(-ntiles // nxcd)
    out = []
    for b in range(grid):
        seg0 = (b % nxcd) * seg
        seg1 = min(seg0 + seg, ntiles)
        out.append(list(range(seg0 + b // nxcd, seg1, wpx)))
    return out


outside = PC.outside
width_stats = PC.width_stats
