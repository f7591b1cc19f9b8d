"""The case table of a GSTS unit's first and last launch (csrc/sn_gsts.hip) and their float64 references, shared by the CPU test
(tests/test_host_gsts_edges.py) and the GPU test (tests/test_gpu_gsts_edges.py).  No GPU import.

K0 (sn_gsts_shiftconv, sn_gsts_shiftconv_mfma in its tile and walking forms): hw = dw3x3(spatial_shift(borrowed half)).
K4 (sn_gsts_cab2_phase2, sn_cab1_phase2): y = shortcut + W' . bf16(ca * g2) + bias'.

Operands, as bf16_conv_cases.make_operands builds them: bf16 values of a wide exponent range (unit normal noise x 2^U(-6, 6)) with 1 in 16 exact
zeros; K0's weights rounded to bf16 exactly as the engine packs w1 (k0_words); K4's matrix and bias are the expressions of prep.pack_out_gemm (beta
folded in float32, the matrix then rounded to bf16), recomputed here (k4_folded) and handed to the kernel through prep.pack_out_gemm itself; ca is
fp32 with both signs and 1 in 8 exact zeros.

Where a frame's half-channel slabs come from (unit_slabs) restates sn_unit_slabs of csrc/sn_common.h: wrap 0 / 1 / 2 (halo), clips, modes 0 / 1 / 2.
tests/test_host_gsts_edges.py holds it against the oracle's own chain (temporal_roll -> spatial_shift -> conv2d; gsts_gather) to 1e-12.

Per-element bounds, the convention of bf16_conv_cases.py: |got - ref| <= u |ref| + (1 + u) eps M, u = 2^-8 (the bf16 store),
  K0: eps = (9 + 8) 2^-24, M = sum |w| |S| over the nine taps;
  K4: eps = (C + 8) 2^-24, M = sum |W'| |bf16(ca g2)| + |bias'| + |shortcut|.
K4 rounds the scaled operand ca * g2 to bf16 before the MFMA (pack8(v) in scale_gemm_res_kernel).  The reference MODELS that rounding explicitly --
the fp32 product of the fp32 scale and the bf16 value, rounded to nearest even to bf16, which is what the kernel computes bit for bit -- instead of
covering it with an extra term sum |W'| 2^-8 |ca g2| in the bound: the bound stays ~C/2 times tighter.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from shiftnet_amd import prep
from shiftnet_amd.spec import shift_table

U = 2.0 ** -24
U_BF16 = 2.0 ** -8
EINVAL = -22
TILE, WALK = 1, 2                           # sn_k0_opts.form
VARIANT_WRAP = {64: 1, 80: 0}               # gshift_deblur2 (C = 64) rolls circularly, gshift_deblur1 (C = 80) keeps the boundary frame
D = torch.float64


@dataclass
class K0Case:
    id: str
    C: int
    T: int
    h: int
    w: int
    mode: int
    wrap: int
    walk: Tuple[int, ...]                   # segment lengths of the walking-form launches
    clip: int = 0
    t0: int = 0
    nt: int = 0
    wgs1: bool = False                      # the walking form also with one workgroup per XCD
    seed: int = 0

    @property
    def frames(self):
        return range(self.t0, self.t0 + self.nt) if self.nt else range(self.T)


@dataclass
class K4Case:
    id: str
    C: int
    T: int
    h: int
    w: int
    mode: int
    wrap: int
    bias: bool
    clip: int = 0
    t0: int = 0
    nt: int = 0
    seed: int = 0

    @property
    def frames(self):
        return range(self.t0, self.t0 + self.nt) if self.nt else range(self.T)

    @property
    def items(self):                        # (pixel chunk, frame) workgroups of the launch: 64 SN_K4_NT = 256 pixels per chunk
        return -(-self.h * self.w // 256) * len(self.frames)


def _k0_rows(C: int) -> List[K0Case]:
    v = VARIANT_WRAP[C]
    return [
        # nty = 9, ntx = 3, ragged bottom and right tiles; tile column 1 meets the loaders' `full` test with equality (7 + 34 = 41), a segment's
        # later block too (112 + 25 = 137); S = 8 visits all eight ring offsets; 9 (frame, segment) rows over 8 XCDs: the early break
        K0Case(f"c{C}_ragged_3x137x41_m1", C, 3, 137, 41, 1, v, (4, 6, 8, 5, 7)),
        K0Case(f"c{C}_ragged_3x137x41_m2", C, 3, 137, 41, 2, v, (4, 8)),
        K0Case(f"c{C}_full_misses_by_one_3x136x40", C, 3, 136, 40, 2, v, (4, 8)),
        K0Case(f"c{C}_one_tile_2x16x16", C, 2, 16, 16, 1, 1 - v, (1, 4)),
        K0Case(f"c{C}_smaller_than_the_shifts_1x5x3", C, 1, 5, 3, 2, v, (4,)),
        K0Case(f"c{C}_items_per_workgroup_2x70x200", C, 2, 70, 200, 1, v, (4, 2), wgs1=True),
        K0Case(f"c{C}_frame_range_4x37x50", C, 4, 37, 50, 1, v, (2, 3), t0=1, nt=2),
        K0Case(f"c{C}_frame_range_4x37x50_m2", C, 4, 37, 50, 2, 1 - v, (3,), t0=2, nt=2),
        K0Case(f"c{C}_clips_of_2_4x37x50_m1", C, 4, 37, 50, 1, v, (3,), clip=2),
        K0Case(f"c{C}_clips_of_2_4x37x50_m2", C, 4, 37, 50, 2, 1 - v, (2,), clip=2),
        K0Case(f"c{C}_halo_3x37x50_m1", C, 3, 37, 50, 1, 2, (3,)),
        K0Case(f"c{C}_halo_3x37x50_m2", C, 3, 37, 50, 2, 2, (2,)),
    ]


def _k4_rows(C: int) -> List[K4Case]:
    v = VARIANT_WRAP[C]
    return [
        K4Case(f"c{C}_px1_cab1", C, 2, 1, 1, 0, 0, True),
        K4Case(f"c{C}_px256_one_chunk_m1", C, 2, 16, 16, 1, 1 - v, False),
        K4Case(f"c{C}_px259_3_frames_6_items_m2", C, 3, 7, 37, 2, v, True),                 # two of the eight XCD slots stay empty
        K4Case(f"c{C}_px513_5_frames_15_items_m1", C, 5, 19, 27, 1, v, True),               # not a multiple of 8
        K4Case(f"c{C}_px513_cab1_no_bias", C, 1, 19, 27, 0, 0, False),
        K4Case(f"c{C}_px259_cab1_frame_range", C, 4, 7, 37, 0, 0, True, t0=2, nt=1),
        K4Case(f"c{C}_halo_3x7x37_m1", C, 3, 7, 37, 1, 2, True),
        K4Case(f"c{C}_halo_2x19x27_m2", C, 2, 19, 27, 2, 2, False),
        K4Case(f"c{C}_clips_of_2_4x7x37_m2", C, 4, 7, 37, 2, v, False, clip=2),
        K4Case(f"c{C}_clips_of_2_4x16x16_m1", C, 4, 16, 16, 1, 1 - v, True, clip=2),
        K4Case(f"c{C}_frame_range_4x16x16_m1", C, 4, 16, 16, 1, v, True, t0=1, nt=2),
        K4Case(f"c{C}_frame_range_4x7x37_m2", C, 4, 7, 37, 2, 1 - v, False, t0=0, nt=3),
    ]


K0_CASES: List[K0Case] = _k0_rows(64) + _k0_rows(80)
K4_CASES: List[K4Case] = _k4_rows(64) + _k4_rows(80)
for _i, _c in enumerate(K0_CASES):
    _c.seed = 5000 + 37 * _i
for _i, _c in enumerate(K4_CASES):
    _c.seed = 7000 + 41 * _i

# ---- the plan of sn_gsts_shiftconv_mfma at ncu = 256 (sn_gsts_shiftconv_mfma_plan): (C, T, h, w) -> (form, S) -----------------------------
# The walking form needs a segment length S >= 4 with at least 4 * (workgroups per CU) * ncu items: 2048 at C = 64, 1024 at C = 80.  360 x 640 is
# 23 x 40 tiles, so nseg * 40 * T items: S = 8 (nseg 3) from T = 18 / 9, S = 6 (nseg 4) from T = 13 / 7, S = 4 (nseg 6) from T = 9 / 5.
K0_PLAN_ROWS: Dict[Tuple[int, int, int, int], Tuple[int, int]] = {
    (64, 20, 360, 640): (WALK, 8), (64, 20, 180, 320): (TILE, 2), (64, 5, 90, 160): (TILE, 2), (80, 5, 90, 160): (TILE, 2),
    (64, 8, 360, 640): (TILE, 3), (64, 9, 360, 640): (WALK, 4), (64, 12, 360, 640): (WALK, 4), (64, 13, 360, 640): (WALK, 6),
    (64, 17, 360, 640): (WALK, 6), (64, 18, 360, 640): (WALK, 8), (64, 3, 184, 328): (TILE, 2),
    (80, 20, 360, 640): (WALK, 8), (80, 20, 180, 320): (WALK, 4), (80, 4, 360, 640): (TILE, 3), (80, 5, 360, 640): (WALK, 4),
    (80, 6, 360, 640): (WALK, 4), (80, 7, 360, 640): (WALK, 6), (80, 8, 360, 640): (WALK, 6), (80, 9, 360, 640): (WALK, 8),
    (80, 3, 184, 328): (TILE, 2),
}


# ---- operands --------------------------------------------------------------------------------------------------------------------------

def _act(g, shape):
    x = torch.randn(shape, generator=g) * torch.exp2(torch.rand(shape, generator=g) * 12.0 - 6.0)
    x[torch.rand(shape, generator=g) < 1.0 / 16] = 0.0
    return x.to(torch.bfloat16)


def _sgn(g, n):
    return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def k0_words(w: torch.Tensor) -> torch.Tensor:
    """fp32 [C/2][9] -> int32 words with the bf16 weight in the low half: Plan.add_unit's expression for u["w1"]"""
    return (w.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF).contiguous()


def k0_operands(c: K0Case) -> Dict[str, object]:
    """x bf16 [T][h][w][C], halo bf16 [h][w][C/2] (wrap 2), w fp32 [C/2][9] (rounded to bf16 by the packing), offs int8 [C/2][2]"""
    g = torch.Generator().manual_seed(c.seed)
    ops: Dict[str, object] = {"x": _act(g, (c.T, c.h, c.w, c.C))}
    ops["halo"] = _act(g, (c.h, c.w, c.C // 2)) if c.wrap == 2 else None
    ops["w"] = (torch.randn((c.C // 2, 9), generator=g) / 3.0).float()
    ops["offs"] = prep.shift_offsets_i8(shift_table(c.C))
    return ops


def k4_operands(c: K4Case) -> Dict[str, object]:
    """x, g2 bf16 [T][h][w][C], halo bf16 [h][w][C/2] (wrap 2), ca fp32 [T][C], w3 fp32 [C][C][1][1], beta fp32 [1][C][1][1], bias3 fp32 [C] or None"""
    g = torch.Generator().manual_seed(c.seed)
    ops: Dict[str, object] = {"x": _act(g, (c.T, c.h, c.w, c.C)), "g2": _act(g, (c.T, c.h, c.w, c.C))}
    ops["halo"] = _act(g, (c.h, c.w, c.C // 2)) if c.wrap == 2 else None
    ca = (0.25 + 1.5 * torch.rand((c.T, c.C), generator=g)) * _sgn(g, (c.T, c.C))
    ca[torch.rand((c.T, c.C), generator=g) < 1.0 / 8] = 0.0
    ops["ca"] = ca.float()
    ops["w3"] = (torch.randn((c.C, c.C, 1, 1), generator=g) / math.sqrt(c.C)).float()
    ops["beta"] = ((0.25 + torch.rand((1, c.C, 1, 1), generator=g)) * _sgn(g, (1, c.C, 1, 1))).float()
    ops["bias3"] = ((0.05 + 0.5 * torch.rand(c.C, generator=g)) * _sgn(g, c.C)).float() if c.bias else None
    return ops


def k4_folded(ops: Dict[str, object]) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(W' [C][C] float64 = bf16(w3 * beta), bias' [C] float64 = fp32(bias3 * beta) or None): prep.pack_out_gemm's expressions, in float32 as there"""
    C = ops["w3"].shape[0]
    w = ops["w3"].numpy().reshape(C, C)
    b = ops["beta"].numpy().reshape(C)
    wp = torch.from_numpy(w * b[:, None]).to(torch.bfloat16).to(D)
    bias = None if ops["bias3"] is None else torch.from_numpy(ops["bias3"].numpy() * b).to(D)
    return wp, bias


def k4_packed(ops: Dict[str, object]) -> Dict[str, object]:
    """what the kernel gets: prep.pack_out_gemm's fragments and bias"""
    return prep.pack_out_gemm(ops["w3"], ops["beta"], ops["bias3"], ops["w3"].shape[0])


# ---- float64 references ----------------------------------------------------------------------------------------------------------------

def unit_slabs(x: torch.Tensor, halo: Optional[torch.Tensor], mode: int, wrap: int, clip: int, t: int):
    """(u[:, :C/2], u[:, C/2:C], borrowed half) of absolute frame t, each [h][w][C/2]: sn_unit_slabs (csrc/sn_common.h) on an NHWC tensor x [T][h][w][C].
    mode 0: u = x[t], nothing borrowed."""
    T, Ch = x.shape[0], x.shape[-1] // 2
    n = clip if clip > 0 else T
    base = t // n * n
    tl = t - base
    lo = lambda f: x[base + f][..., :Ch]      # noqa: E731
    hi = lambda f: x[base + f][..., Ch:]      # noqa: E731
    if mode == 0:
        return lo(tl), hi(tl), None
    if mode == 1:                             # forward: borrows the upper half of frame t - 1
        if tl > 0 or wrap == 1:
            b = hi((tl - 1) % n)
            return b, lo(tl), b
        if wrap == 2:
            return halo, lo(tl), halo
        return lo(tl), hi(tl), lo(tl)         # kept boundary frame: its own lower half
    if tl < n - 1 or wrap == 1:               # reverse: borrows the lower half of frame t + 1
        b = lo((tl + 1) % n)
        return hi(tl), b, b
    if wrap == 2:
        return hi(tl), halo, halo
    return lo(tl), hi(tl), hi(tl)


def shifted(b: torch.Tensor, C: int, conv_padding: bool = True) -> torch.Tensor:
    """b [Ch][h][w] -> S [Ch][h + 2][w + 2] on the image and its one-pixel ring (S[:, 1 + y, 1 + x] is pixel (y, x)): S[p] = b[p + d_k] where
    p + d_k is inside the image, 0 elsewhere -- and 0 on the ring, where p itself is outside: the 3x3's zero padding.  conv_padding False (negative
    control): the ring too reads b[p + d_k] wherever that is inside."""
    Ch, h, w = b.shape
    pad = F.pad(b, (9, 9, 9, 9))
    out = torch.zeros((Ch, h + 2, w + 2), dtype=b.dtype)
    for k, (dy, dx) in enumerate(shift_table(C)):
        out[k] = pad[k, 8 + dy: 8 + dy + h + 2, 8 + dx: 8 + dx + w + 2]
    if conv_padding:
        out[:, 0] = 0
        out[:, -1] = 0
        out[:, :, 0] = 0
        out[:, :, -1] = 0
    return out


def k0_reference(c: K0Case, ops: Dict[str, object], control: Optional[str] = None):
    """(ref, tol, M) float64 [nt][h][w][C/2] of the frames c.frames.  control: "no_conv_padding" (S is read wherever p + d is inside the image,
    even where p is not) or "tap_dropped" (tap k % 9 of channel k is zero)."""
    Ch = c.C // 2
    w = ops["w"].to(torch.bfloat16).to(D).view(Ch, 1, 3, 3).clone()
    if control == "tap_dropped":
        for k in range(Ch):
            w[k, 0].view(9)[k % 9] = 0.0
    refs, ms = [], []
    for t in c.frames:
        b = unit_slabs(ops["x"], ops["halo"], c.mode, c.wrap, c.clip, t)[2].to(D).permute(2, 0, 1)
        s = shifted(b, c.C, conv_padding=control != "no_conv_padding")[None]
        refs.append(F.conv2d(s, w, groups=Ch)[0])
        ms.append(F.conv2d(s.abs(), w.abs(), groups=Ch)[0])
    ref, m = torch.stack(refs).permute(0, 2, 3, 1), torch.stack(ms).permute(0, 2, 3, 1)
    tol = U_BF16 * ref.abs() + (1.0 + U_BF16) * (9 + 8) * U * m + 1e-30
    return ref, tol, m


def k4_shortcut(c: K4Case, ops: Dict[str, object], t: int, rolled: bool = True) -> torch.Tensor:
    """[h][w][C] float64: x[t] for CAB1, the rolled u[:, :C] for CAB2 (rolled False, negative control: x[t] there too)"""
    p0, p1, _ = unit_slabs(ops["x"], ops["halo"], c.mode if rolled else 0, c.wrap, c.clip, t)
    return torch.cat((p0, p1), -1).to(D)


def k4_reference(c: K4Case, ops: Dict[str, object], control: Optional[str] = None):
    """(ref, tol, M) float64 [nt][h][w][C] of the frames c.frames.  control: "no_ca" (g2 unscaled) or "unrolled_shortcut"."""
    wp, bias = k4_folded(ops)
    refs, ms = [], []
    for t in c.frames:
        g2 = ops["g2"][t]
        if control == "no_ca":
            v = g2.to(D)
        else:
            v = (g2.float() * ops["ca"][t].view(1, 1, -1)).to(torch.bfloat16).to(D)      # fp32 product, rounded to bf16: the kernel's own operand
        sc = k4_shortcut(c, ops, t, rolled=control != "unrolled_shortcut")
        a, m = v @ wp.T + sc, v.abs() @ wp.abs().T + sc.abs()
        if bias is not None:
            a, m = a + bias, m + bias.abs()
        refs.append(a)
        ms.append(m)
    ref, m = torch.stack(refs), torch.stack(ms)
    tol = U_BF16 * ref.abs() + (1.0 + U_BF16) * (c.C + 8) * U * m + 1e-30
    return ref, tol, m


# ---- the kernels' item loops and ring arithmetic, restated ---------------------------------------------------------------------------------

def k0_items(plan: Dict[str, int]) -> List[Tuple[int, int, int]]:
    """every (frame, tile row, tile column) a launch with this plan computes, in workgroup order: the item loops of shiftconv_mfma_walk_kernel
    (xcd, j0, i += nwg, row = xcd per_x + rl, break, ntile = min(S, nty - ty0)) and of shiftconv_mfma_kernel"""
    out = []
    ntx, nty, nt, per_x, nwg = plan["ntx"], plan["nty"], plan["nt"], plan["per_x"], plan["grid"] >> 3
    for b in range(plan["grid"]):
        xcd, j0 = b & 7, b >> 3
        for i in range(j0, per_x * ntx, nwg):
            rl, tx = divmod(i, ntx)
            row = xcd * per_x + rl
            if plan["form"] == WALK:
                if row >= nt * plan["nseg"]:
                    break
                tc, sg = divmod(row, plan["nseg"])
                ty0 = sg * plan["S"]
                for jj in range(min(plan["S"], nty - ty0)):
                    out.append((tc, ty0 + jj, tx))
            else:
                if row >= nty * nt:
                    break
                tc, ty = divmod(row, nty)
                out.append((tc, ty, tx))
    return out


RW = 34                                     # rows of a window = rows of the ring
BR = 17                                     # rows of one of the two staging blocks of a segment's first window


def tile_window_slack(h: int, w: int, ty: int, tx: int) -> Optional[Tuple[int, int]]:
    """shiftconv_mfma_kernel's `wfull` (yc >= 9 && xc >= 9 && yc + 25 <= h && xc + 25 <= w) for tile (ty, tx): None where the window starts
    outside the image, else (h - (yc + 25), w - (xc + 25)) -- the loader runs without any test iff both are >= 0, with equality at 0"""
    yc, xc = 16 * ty, 16 * tx
    return (h - (yc + 25), w - (xc + 25)) if yc >= 9 and xc >= 9 else None


def walk_block_slacks(h: int, w: int, ty: int, tx: int, jj: int) -> List[Optional[Tuple[int, int]]]:
    """`full` of the walking kernel's `stage` calls for tile (ty, tx), the jj-th of its segment (gy0 = yc - 9 + wr0, gx0 = xc - 9; gy0 >= 0 &&
    gy0 + nrows <= h && gx0 >= 0 && gx0 + 34 <= w): two blocks (wr0, nrows) = (0, 17), (17, 17) for jj = 0, one block (18, 16) afterwards.  Per
    block: None where it starts outside the image, else (h - (gy0 + nrows), w - (gx0 + 34))"""
    out = []
    for wr0, nrows in ([(0, BR), (BR, BR)] if jj == 0 else [(RW - 16, 16)]):
        gy0, gx0 = 16 * ty - 9 + wr0, 16 * tx - 9
        out.append((h - (gy0 + nrows), w - (gx0 + RW)) if gy0 >= 0 and gx0 >= 0 else None)
    return out


def ring_rows_written(jj: int) -> Dict[int, int]:
    """window row -> ring row the walking kernel's `stage` calls of a segment's tile jj write: two blocks of 17 rows at ring base 0 for jj = 0, window
    rows 18 .. 33 at rbase = 16 jj % 34 afterwards (rr = rbase + wr0 + lr, two conditional subtractions)"""
    out = {}
    rbase = (16 * jj) % RW
    calls = [(0, 17, 0), (17, 17, 0)] if jj == 0 else [(RW - 16, 16, rbase)]
    for wr0, nrows, rb in calls:
        for lr in range(nrows):
            rr = rb + wr0 + lr
            rr -= RW if rr >= RW else 0
            rr -= RW if rr >= RW else 0
            out[wr0 + lr] = rr
    return out


def ring_row_read(jj: int, wr: int) -> int:
    """ring row the MFMA loop reads for window row wr = n + 8 + sy + s of tile jj (rr = rbase + wr, one conditional subtraction)"""
    rr = (16 * jj) % RW + wr
    rr -= RW if rr >= RW else 0
    return rr
