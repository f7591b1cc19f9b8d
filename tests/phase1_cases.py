"""The case table of the fused phase 1 (csrc/sn_phase1r.hip: sn_gsts_cab2_phase1, sn_cab1_phase1), its operands and a float64 INTERVAL reference,
shared by the CPU test (tests/test_host_phase1_ref.py) and the GPU test (tests/test_gpu_phase1_edges.py).  No GPU import.

    g2 = SimpleGate2(1x1(RepConv(SimpleGate(dw3x3 + id(1x1(LayerNorm(u)))))))

Why an interval and not a bound around one value.  The kernel rounds five times on the way (xn to bf16, `a` to fp16, nine fp16 FMAs, the fp16 gate
product, r to fp16).  A first-order worst-case bound u |v| + eps M carried through the six stages ends at a tolerance of tens of per cent of the
tensor's peak.  Here every rounding the kernel performs is MODELLED and each element carries [lo, hi]:
  * a VALU stage is a fixed sequence of correctly rounded operations; both ends go through the same sequence in the kernel's order (rounding is
    monotone, so the kernel's value stays between the ends);
  * a matrix-core stage takes the exact float64 interval product (weights split by sign), widens it by the accumulation term n 2^-24 M of
    tests/bf16_conv_cases.py (M = sum |W| max(|lo|, |hi|) + |bias|) and rounds both ends.
The interval has zero width wherever no rounding boundary falls inside it: error does not accumulate, it only appears where a value sits next to
a tie.

Stages (Arith: the roundings; reference(): the chain; the kernel's header comment names each of them):
  1 LayerNorm, fp32 two-pass statistics in the stagers, xn = bf16(d rstd).  The point value is float64; its half-width, with u = 2^-24, K channels,
    A = mean |v|, z = var + 1e-6:
        mean   K - 1 additions, the rounded 1/K, one product:           |mean~ - mean| <= em = (K - 1) u A + 2 u |mean|
        d = v - mean~, one subtraction, relative to its RESULT:          |d~ - d| <= ed = em + u (|d| + em)
        q = sum d~^2, K FMAs and the lane reductions, all terms >= 0:    |q~ - q| <= eq + (K + 2) u q,   eq = sum (2 |d| ed + ed^2)
        z~ = q~ (1/K)~ + 1e-6f, three more roundings:                    relative ez = eq / (K z) + (K + 5) u
        rstd~ = v_rsq_f32(z~), 1 ulp:                                    relative er = (1 - ez)^-1/2 - 1 + 2^-23
        xn~ = d~ rstd~, one product:                                     |xn~ - xn| <= rstd (ed (1 + er) + |d| (er + u))
    (The centring term is u (|v| + |mean|) rstd at most: 2 u |mean| sits in em, and the subtraction's own rounding is relative to d.)
    Where the fp32 sum is provably EXACT -- every addend a multiple of a quantum q0 and sum |v| < 2^24 q0, which holds for the offset and the
    constant pixels: all values in one or two binades -- mean~ and d~ are not bounded but modelled: mean~ = fl(S (1/K)~), d~ = fl(v - mean~), or
    d~ = fl(v - S (1/K)~) should a compiler contract the two into one FMA (today's does not; both are inside), and only the statistics' relative
    error (er + 2 u) |xn| is left.  This is what keeps the special pixels from widening their 7 x 7 neighbourhoods.
    Both ends are then rounded to bf16.  Pixels outside the image are exact zeros, the constant-one slots included.
  2 first 1x1 (bf16 MFMA, K + 2 slots: the bias is bf16 hi + lo against a constant 1): widened by (K + 2 + 8) u M, ends to fp16 (v_cvt_pk_f16_f32).
  3 3x3 + identity, packed fp16: taps 0..8 row-major, tx = 0 the left neighbour; a rounded product, then eight FMAs, each rounding once to fp16.
  4 gate: g1 = fp16(F1 F2) (the 2^-4 sits in F1's taps); second pass of the denoisers: fp16(g1 fp16(scale)).  Zero outside the image.
  5 RepConv on the dense per-group kernels (fp16 MFMA, 240 slots): widened by (240 + 8) u M, ends to fp16.
  6 second 1x1 (fp16 MFMA): widened by (C + 8) u M; g2 = b1 rcp(1 + exp2(b2')): e = exp2(b2') (1 + d1), |d1| <= 2^-23 (1 ulp), weighs at most d1 in
    1 + e; the addition 2^-24; v_rcp_f32 2^-23; the product 2^-24: 3 2^-23 to first order, the reference widens by RHO_GATE2 = 2^-21 relative.  The
    pool sums this value; g2 stores it rounded to bf16.
fp16 subnormals: wherever an fp16 end is below 2^-14 in magnitude the interval is extended to contain 0, so a consumer that flushes and one that
does not are both inside.  fp32 results below 2^-100 likewise (exp2 / rcp saturate there).  No modelled fp16 value may exceed 2^15 (asserted).

Two intervals, and which means what.  Arith("interval"), the default and the one every assertion above is about, is the "EITHER" interval: it holds
for a kernel that keeps fp16 subnormals, for one that flushes them, and for any mixture per stage.  That makes it blind exactly where a checkpoint
is cold (tests/gauge.py: body.0 rows a few powers of two smaller than the synthetic ones): once a fifth of g1 lies below 2^-14 the extension to 0
is most of the width, and a kernel that loses two decimal digits by flushing is still inside.  Arith("interval", keep16=True) is the "KEEP16"
interval: h16 rounds both ends as numpy's fp16 does (gradual underflow, nearest even) and extends nothing, everything else is the same code.  It
holds only for a kernel EVERY fp16 stage of which keeps subnormals (v_cvt_pk_f16_f32, the packed FMAs, the gate product, the fp16 MFMA operands),
and stays as narrow at a cold rung as at the base one.  A point emulation that flushes leaves it (the control of tests/test_host_gauge.py); the
kernel is held inside it by tests/test_gpu_phase1_gauge.py.

Pool rows are per (frame, strip, block of 8 image rows): the interval sum of the un-rounded g2 (sums pass: 16 g1) over the row's own pixels,
widened by n u sum |.| for the fp32 summation of n terms.

The same code run as a POINT emulation (Arith "point": LayerNorm in numpy float32, every accumulation term replaced by a share of it) gives the
containment check and the one-fault controls of tests/test_host_phase1_ref.py; run "exact" (no rounding, un-rounded float64 weights) it is the
oracle's chain.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

import gsts_edge_cases as GE
from shiftnet_amd import prep

U = 2.0 ** -24
SUB16 = 2.0 ** -14
SUB32 = 2.0 ** -100
MAX16 = 2.0 ** 15
RHO_GATE2 = 2.0 ** -21
P1R_RB = 8
VARIANT_WRAP = GE.VARIANT_WRAP
F32 = np.float32
F64 = np.float64


@dataclass
class P1Case:
    id: str
    C: int
    T: int
    h: int
    w: int
    mode: int
    wrap: int
    clip: int = 0
    t0: int = 0
    nt: int = 0
    teams: Tuple[int, ...] = ()             # team sizes run besides the library's own (0)
    kind: str = "g2"                        # "g2" | "sums" (denoisers' first pass) | "scale" (their second pass) | "plan" (a chunk crosses a strip end)
    se: bool = False                        # squeeze-excite fold checked on this row
    oracle: bool = False                    # held against the oracle's chain on the CPU
    seed: int = 0

    @property
    def frames(self):
        return range(self.t0, self.t0 + self.nt) if self.nt else range(self.T)

    @property
    def K(self):
        return self.C + self.C // 2 if self.mode else self.C


def _rows(C: int) -> List[P1Case]:
    v = VARIANT_WRAP[C]
    return [
        P1Case(f"c{C}_one_pixel_1x1x1_m0", C, 1, 1, 1, 0, 0, oracle=True),                         # smaller than every halo and warm-up
        P1Case(f"c{C}_fewer_rows_than_warmup_2x5x9_m1", C, 2, 5, 9, 1, v, oracle=True),
        P1Case(f"c{C}_one_strip_full_block_1x8x64_m0", C, 1, 8, 64, 0, 0, oracle=True),              # the region touches both edges; row block exactly full
        P1Case(f"c{C}_two_strips_1x9x65_m0", C, 1, 9, 65, 0, 0, oracle=True),                        # two strips (the plan spreads the slack: 32 + 33 columns); one row over the block
        P1Case(f"c{C}_61_61_2x9x122_m2", C, 2, 9, 122, 2, v, oracle=True),
        P1Case(f"c{C}_three_strips_2x9x123_m1", C, 2, 9, 123, 1, v, se=True, oracle=True),
        P1Case(f"c{C}_four_strips_3x17x181_m1", C, 3, 17, 181, 1, v, se=True, oracle=True),          # capacity slack spread (sd, sr); three row blocks
        P1Case(f"c{C}_ragged_frame_block_5x17x70_m2", C, 5, 17, 70, 2, v, teams=(1, 2, 4)),
        P1Case(f"c{C}_frame_range_4x12x70_m1", C, 4, 12, 70, 1, v, t0=1, nt=2),
        P1Case(f"c{C}_clips_of_2_4x12x70_m1", C, 4, 12, 70, 1, v, clip=2),
        P1Case(f"c{C}_clips_of_2_4x12x70_m2", C, 4, 12, 70, 2, 1 - v, clip=2),
        P1Case(f"c{C}_halo_3x12x70_m1", C, 3, 12, 70, 1, 2),
        P1Case(f"c{C}_halo_3x12x70_m2", C, 3, 12, 70, 2, 2),
        P1Case(f"c{C}_other_wrap_2x16x16_m1", C, 2, 16, 16, 1, 1 - v),
        P1Case(f"c{C}_denoise_sums_2x17x123_m1", C, 2, 17, 123, 1, 0, kind="sums"),
        P1Case(f"c{C}_denoise_scale_2x17x123_m0", C, 2, 17, 123, 0, 0, kind="scale"),
        P1Case(f"c{C}_chunk_crosses_strip_4x97x250_m1", C, 4, 97, 250, 1, v, kind="plan"),
    ]


CASES: List[P1Case] = _rows(64) + _rows(80)
for _i, _c in enumerate(CASES):
    _c.seed = 9000 + 43 * _i
BY_ID = {c.id: c for c in CASES}


# ---- number formats ---------------------------------------------------------------------------------------------------------------------

def r16(x):
    """float64 -> nearest-even fp16, as float64 (numpy converts double to half in one rounding)"""
    with np.errstate(over="ignore"):
        return np.asarray(x, F64).astype(np.float16).astype(F64)


def rbf(x):
    """float64 -> nearest-even bf16 (8 significant bits), as float64; bf16 subnormals do not occur at these magnitudes"""
    m, e = np.frexp(np.asarray(x, F64))
    return np.ldexp(np.rint(m * 256.0), e - 8)


class Arith:
    """The roundings and widenings of one run.  kind "interval": both ends rounded, accumulation terms widen; "point": lo == hi throughout, every
    accumulation term n u M is replaced by share * n u M (share in [-1, 1]: a number, or None for random per element), fp16 subnormals kept or
    flushed to zero (flush); "exact": nothing is rounded or widened.  keep16 (interval): fp16 subnormals are taken as KEPT -- the ends are rounded and
    not extended to 0 (module docstring: the two intervals)."""

    def __init__(self, kind: str = "interval", rng: Optional[np.random.Generator] = None, share: Optional[float] = None, flush: bool = False,
                 keep16: bool = False):
        assert kind in ("interval", "point", "exact")
        assert not keep16 or kind == "interval"
        self.kind, self.rng, self.share, self.flush, self.keep16 = kind, rng, share, flush, keep16
        self.max16 = 0.0

    def bf(self, lo, hi):
        return (lo, hi) if self.kind == "exact" else (rbf(lo), rbf(hi))

    def h16(self, lo, hi):
        if self.kind == "exact":
            return lo, hi
        lo, hi = r16(lo), r16(hi)
        if self.kind == "interval":
            if lo.size:
                self.max16 = max(self.max16, float(np.abs(lo).max()), float(np.abs(hi).max()))      # inf and NaN fail reference()'s assertion too
            if not self.keep16:
                lo = np.where(np.abs(lo) < SUB16, np.minimum(lo, 0.0), lo)
                hi = np.where(np.abs(hi) < SUB16, np.maximum(hi, 0.0), hi)
        elif self.flush:
            lo = np.where(np.abs(lo) < SUB16, 0.0, lo)
            hi = lo
        return lo, hi

    def acc(self, lo, hi, n: int, M):
        """a matrix-core (or fp32 summation) result of n terms with magnitude sum M"""
        if self.kind == "exact":
            return lo, hi
        e = n * U * M
        if self.kind == "interval":
            return lo - e, hi + e
        s = self.share if self.share is not None else self.rng.uniform(-1.0, 1.0, np.shape(lo))
        return lo + s * e, hi + s * e

    def rel(self, lo, hi, rho: float):
        if self.kind == "exact":
            return lo, hi
        if self.kind == "interval":
            lo, hi = lo - rho * np.abs(lo), hi + rho * np.abs(hi)
            return np.where(np.abs(lo) < SUB32, np.minimum(lo, 0.0), lo), np.where(np.abs(hi) < SUB32, np.maximum(hi, 0.0), hi)
        s = self.share if self.share is not None else self.rng.uniform(-1.0, 1.0, np.shape(lo))
        return lo + s * rho * np.abs(lo), hi + s * rho * np.abs(hi)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------

def _positions(g, h: int, w: int):
    """per image position: class (0 plain, 1 offset, 2 tiny, 3 constant), scale, offset / constant value.  The class is a property of the POSITION:
    every frame, the halo and hw share it, so a pixel of the virtual input u (halves of two frames and hw) is special in all its K channels."""
    r = torch.rand((h, w), generator=g)
    cls = torch.zeros((h, w), dtype=torch.int64)
    cls[r < 1 / 16] = 1
    cls[(r >= 1 / 16) & (r < 1 / 16 + 1 / 32)] = 2
    cls[(r >= 1 / 16 + 1 / 32) & (r < 1 / 16 + 1 / 32 + 1 / 64)] = 3
    scale = torch.exp2(torch.rand((h, w), generator=g) * 6.0 - 4.0)
    value = GE._sgn(g, (h, w)) * scale * (90.0 + 20.0 * torch.rand((h, w), generator=g))
    const = torch.randn((h, w), generator=g) * torch.exp2(torch.rand((h, w), generator=g) * 8.0 - 6.0)
    noise = torch.exp2(torch.rand((h, w), generator=g) * 1.5 - 1.5)              # the offset is 100 .. 280 standard deviations: bf16's 8 bits end at 256
    return cls, scale, value, const, noise


def _special(g, shape, pos):
    """gsts_edge_cases._act, and at the special positions: a common offset of 100 .. 280 standard deviations (the cancellation case of two-pass
    statistics; bf16's 8 bits end at 256), amplitudes within +-2^-10 (variance near the 1e-6 epsilon), an exactly constant pixel (d = 0, xn = 0)"""
    cls, scale, value, const, noise = pos
    x = GE._act(g, shape).float()
    lead = (None,) * (len(shape) - 3)
    c, s, v, k, n = (t[lead + (slice(None), slice(None), None)].expand(shape) for t in (cls, scale, value, const, noise))
    off = v + s * n * torch.randn(shape, generator=g)
    tiny = (torch.rand(shape, generator=g) * 2.0 - 1.0) * 2.0 ** -10
    x = torch.where(c == 1, off, x)
    x = torch.where(c == 2, tiny, x)
    x = torch.where(c == 3, k, x)
    return x.to(torch.bfloat16)


def operands(c: P1Case) -> Dict[str, object]:
    """x bf16 [T][h][w][C], halo bf16 [h][w][C/2] (wrap 2), hw bf16 [T][h][w][C/2] (modes 1 / 2: an independent operand, not a K0 output), the raw
    fp32 weights of the block as prep.pack_phase1r takes them, g1_scale fp32 [T][C] (kind "scale"), "cls" int64 [h][w]"""
    g = torch.Generator().manual_seed(c.seed)
    C, K = c.C, c.K
    pos = _positions(g, c.h, c.w)
    ops: Dict[str, object] = {"cls": pos[0], "x": _special(g, (c.T, c.h, c.w, C), pos)}
    ops["halo"] = _special(g, (c.h, c.w, C // 2), pos) if c.wrap == 2 else None
    ops["hw"] = _special(g, (c.T, c.h, c.w, C // 2), pos) if c.mode else None
    cig = 1 if C == 64 else 8                                                   # depthwise RepConv at C = 64, grouped 8 -> 8 at C = 80
    ops["w1"] = (torch.randn((2 * C, K, 1, 1), generator=g) / math.sqrt(K)).float()
    ops["ln_w"] = ((0.25 + torch.rand(K, generator=g)) * GE._sgn(g, K)).float()
    ops["ln_b"] = ((0.05 + 0.5 * torch.rand(K, generator=g)) * GE._sgn(g, K)).float()
    ops["w_dw3"] = (torch.randn((2 * C, 1, 3, 3), generator=g) / 3.0).float()
    ops["w_rep5"] = (torch.randn((C, cig, 5, 5), generator=g) / math.sqrt(25.0 * cig)).float()
    ops["w_rep3"] = (torch.randn((C, cig, 3, 3), generator=g) / math.sqrt(9.0 * cig)).float()
    ops["w2"] = (torch.randn((2 * C, C, 1, 1), generator=g) / math.sqrt(C)).float()
    ops["g1_scale"] = None
    if c.kind == "scale":
        s = (0.25 + 1.5 * torch.rand((c.T, C), generator=g)) * GE._sgn(g, (c.T, C))
        s[torch.rand((c.T, C), generator=g) < 1.0 / 8] = 0.0
        ops["g1_scale"] = s.float()
    return ops


def packed(ops: Dict[str, object]) -> Dict[str, torch.Tensor]:
    """what the kernel gets: prep.pack_phase1r's four operands"""
    return prep.pack_phase1r(ops["w1"], ops["ln_w"], ops["ln_b"], ops["w_dw3"], ops["w_rep5"], ops["w_rep3"], ops["w2"], ops["w1"].shape[0] // 2)


def folded(ops: Dict[str, object], rounded: bool = True) -> Dict[str, np.ndarray]:
    """The matrices the kernel multiplies by, float64, channels in natural order: prep.pack_phase1r's expressions in float32 as there, rounded as it
    rounds them.  rounded False: the same foldings in float64, nothing rounded ("exact" runs).
      W1 [2C][K] bf16, b_hi / b_lo [2C] bf16;  d3 [2C][9] fp16 (identity in the centre, rows < C times P1_G1_SCALE);
      dg [C/8][8 oc][8 ic][5][5] fp16 (prep.rep_dense_group);  W2 [2C][C] fp16 (/ P1_G1_SCALE, gate rows times -log2 e)"""
    c = ops["w1"].shape[0] // 2
    if rounded:
        w = ops["w1"].detach().float().cpu().numpy().reshape(2 * c, -1)
        wf = w * ops["ln_w"].detach().float().cpu().numpy()[None, :]
        b = w @ ops["ln_b"].detach().float().cpu().numpy()
        b_hi = torch.from_numpy(b.astype(np.float32)).to(torch.bfloat16).float().numpy()
        b_lo = b - b_hi
        d3 = ops["w_dw3"].detach().float().cpu().numpy().reshape(2 * c, 9).copy()
        d3[:, 4] += 1.0
        d3[:c] *= prep.P1_G1_SCALE
        dg = prep.rep_dense_group(ops["w_rep5"], ops["w_rep3"], c)
        w2n = ops["w2"].detach().float().cpu().numpy().reshape(2 * c, c) / prep.P1_G1_SCALE
        w2n[c:] *= -np.log2(np.e)
        tb = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()      # noqa: E731
        th = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.float16).to(torch.float64).numpy()       # noqa: E731
        return {"W1": tb(wf), "b_hi": tb(b_hi), "b_lo": tb(b_lo), "d3": d3.astype(np.float16).astype(F64), "dg": th(dg), "W2": th(w2n)}
    w = ops["w1"].double().numpy().reshape(2 * c, -1)
    d3 = ops["w_dw3"].double().numpy().reshape(2 * c, 9).copy()
    d3[:, 4] += 1.0
    d3[:c] *= prep.P1_G1_SCALE
    a5, a3 = ops["w_rep5"].double().numpy(), ops["w_rep3"].double().numpy()
    ng = c // 8
    dg = np.zeros((ng, 8, 8, 5, 5), F64)
    if a5.shape[1] == 8:
        k = a5.copy()
        k[:, :, 1:4, 1:4] += a3
        dg[:] = k.reshape(ng, 8, 8, 5, 5)
        for o in range(8):
            dg[:, o, o, 2, 2] += 1.0
    else:
        k = a5[:, 0].copy()
        k[:, 1:4, 1:4] += a3[:, 0]
        k[:, 2, 2] += 1.0
        k = k.reshape(ng, 8, 5, 5)
        for o in range(8):
            dg[:, o, o] = k[:, o]
    w2n = ops["w2"].double().numpy().reshape(2 * c, c) / prep.P1_G1_SCALE
    w2n[c:] *= -math.log2(math.e)
    return {"W1": w * ops["ln_w"].double().numpy()[None, :], "b_hi": w @ ops["ln_b"].double().numpy(), "b_lo": np.zeros(2 * c), "d3": d3, "dg": dg, "W2": w2n}


# ---- the stages -------------------------------------------------------------------------------------------------------------------------

def gather(c: P1Case, ops: Dict[str, object], t: int, fault: Optional[str] = None) -> np.ndarray:
    """the virtual input u [h][w][K] of absolute frame t, float64: gsts_edge_cases.unit_slabs, then hw[t].  fault "same_frame": the borrowed half is
    taken from frame t itself instead of its neighbour"""
    x = ops["x"]
    Ch = c.C // 2
    if fault == "same_frame" and c.mode:
        p0, p1 = x[t][..., Ch:], x[t][..., :Ch]
    else:
        p0, p1, _ = GE.unit_slabs(x, ops["halo"], c.mode, c.wrap, c.clip, t)
    parts = [p0, p1] + ([ops["hw"][t]] if c.mode else [])
    return torch.cat(parts, -1).to(torch.float64).numpy()


def layer_norm(ar: Arith, u: np.ndarray, fault: Optional[str] = None):
    """stage 1 on u [..., K] -> (lo, hi) of xn.  Point runs compute it in float32 as the stagers do (two passes; fault "one_pass": E[x^2] - mean^2;
    fault "no_eps": the epsilon left out); the other runs in float64 with the half-width of the module docstring."""
    K = u.shape[-1]
    if ar.kind == "point":
        v = u.astype(F32)
        ck = F32(1.0) / F32(K)
        mean = (v.sum(-1, dtype=F32) * ck)[..., None]
        d = v - mean
        if fault == "one_pass":
            var = (v * v).sum(-1, dtype=F32) * ck - mean[..., 0] * mean[..., 0]
        else:
            var = (d * d).sum(-1, dtype=F32) * ck
        with np.errstate(divide="ignore", invalid="ignore"):
            rstd = (F32(1.0) / np.sqrt((var if fault == "no_eps" else var + F32(1e-6)).astype(F64))).astype(F32)
            y = (d * rstd[..., None]).astype(F64)
        y = rbf(y)                                                              # (a NaN or inf of a faulty run stays one)
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
    em = ((K - 1) * U * asum / K + 2.01 * U * np.abs(m)) * (1.0 + 2.0 ** -20)
    ed = em + U * (np.abs(d) + em)
    eq = (2.0 * np.abs(d) * ed + ed * ed).sum(-1, keepdims=True)
    ez = np.minimum(eq / (K * z) + (K + 5) * U, 0.75)
    er = 1.0 / np.sqrt(1.0 - ez) - 1.0 + 2.0 ** -23
    hw = rstd * (ed * (1.0 + er) + np.abs(d) * (er + U)) * (1.0 + 2.0 ** -20)
    lo, hi = y - hw, y + hw
    # pixels whose fp32 sum is provably exact: d~ itself is modelled, only the statistics' relative error is left
    fr, ex = np.frexp(u)
    n8 = np.abs(fr * 256.0).astype(np.int64)                                    # bf16: 8 significant bits
    quantum = np.where(n8 > 0, np.ldexp((n8 & -n8).astype(F64), ex - 8), np.inf).min(-1, keepdims=True)
    exact = (asum < 2.0 ** 24 * quantum)[..., 0]
    if exact.any():
        ue = u[exact]
        s = ue.sum(-1, keepdims=True)
        ck = F32(1.0) / F32(K)
        d_two = (ue.astype(F32) - s.astype(F32) * ck).astype(F64)               # mean rounded, then the subtraction
        d_fma = (ue - s * F64(ck)).astype(F32).astype(F64)                       # contracted: v - sum (1/K)~ rounded once
        ends = []
        for de in (d_two, d_fma):
            ye = de / np.sqrt((de * de).mean(-1, keepdims=True) + eps)
            he = np.abs(ye) * (1.0 / math.sqrt(1.0 - (K + 5) * U) - 1.0 + 2.0 ** -23 + 2.0 * U) * (1.0 + 2.0 ** -20)
            ends += [ye - he, ye + he]
        elo, ehi = np.minimum.reduce(ends), np.maximum.reduce(ends)
        assert (elo >= lo[exact]).all() and (ehi <= hi[exact]).all()             # the modelled d~ lies inside the general bound
        lo[exact], hi[exact] = elo, ehi
    assert (ez < 0.5)[~exact].all(), ez.max()
    return ar.bf(lo, hi)


def _imatmul(lo, hi, W):
    """[..., k] intervals times W [m][k] -> (lo, hi, M) [..., m]"""
    Wp, Wn = np.maximum(W, 0.0).T, np.minimum(W, 0.0).T
    return lo @ Wp + hi @ Wn, hi @ Wp + lo @ Wn, np.maximum(np.abs(lo), np.abs(hi)) @ np.abs(W).T


def _imul(alo, ahi, blo, bhi):
    p = (alo * blo, alo * bhi, ahi * blo, ahi * bhi)
    return np.minimum(np.minimum(p[0], p[1]), np.minimum(p[2], p[3])), np.maximum(np.maximum(p[0], p[1]), np.maximum(p[2], p[3]))


def _iscale(lo, hi, w):
    """interval times the exact factor w (broadcast): the end of v w is picked by the sign of w"""
    return np.where(w >= 0, lo * w, hi * w), np.where(w >= 0, hi * w, lo * w)


def _pad(a, n, value=None):
    out = np.pad(a, ((n, n), (n, n), (0, 0)))
    if value is not None:
        out[:] = value
        out[n:-n, n:-n] = a
    return out


def first_1x1(ar: Arith, xn, fw, K: int):
    lo, hi, M = _imatmul(xn[0], xn[1], fw["W1"])
    bias = fw["b_hi"] + fw["b_lo"]
    lo, hi = ar.acc(lo + bias, hi + bias, K + 2 + 8, M + np.abs(fw["b_hi"]) + np.abs(fw["b_lo"]))
    return ar.h16(lo, hi)


def stencil3(ar: Arith, a, d3, outside=None):
    """stage 3 on `a` (lo, hi) [h][w][2C] -> F on the image and its one-pixel ring [h + 2][w + 2][2C] (F[1 + y][1 + x] is pixel (y, x)); `a` is zero
    outside the image (outside: the value it takes there instead, a negative control)"""
    h, w, _ = a[0].shape
    plo, phi = _pad(a[0], 2, outside), _pad(a[1], 2, outside)
    lo = hi = None
    for k in range(9):
        ty, tx = divmod(k, 3)
        slo, shi = _iscale(plo[ty:ty + h + 2, tx:tx + w + 2], phi[ty:ty + h + 2, tx:tx + w + 2], d3[:, k])
        lo, hi = ar.h16(slo, shi) if k == 0 else ar.h16(slo + lo, shi + hi)
    return lo, hi


def gate(ar: Arith, F, C: int, scale=None, keep_row_above: bool = False):
    """stage 4 on F [h + 2][w + 2][2C] -> (unscaled g1, g1 as the RepConv reads it), each (lo, hi) [h + 4][w + 4][C], zero outside the image
    (keep_row_above: the row above the image keeps its values, a negative control).  scale [C]: the denoisers' second pass."""
    lo, hi = ar.h16(*_imul(F[0][..., :C], F[1][..., :C], F[0][..., C:], F[1][..., C:]))
    mask = np.zeros(lo.shape[:2] + (1,))
    mask[1:-1, 1:-1] = 1.0
    if keep_row_above:
        mask[0, 1:-1] = 1.0
    lo, hi = lo * mask, hi * mask
    raw = (np.pad(lo, ((1, 1), (1, 1), (0, 0))), np.pad(hi, ((1, 1), (1, 1), (0, 0))))
    if scale is None:
        return raw, raw
    s = r16(scale) if ar.kind != "exact" else np.asarray(scale, F64)
    slo, shi = ar.h16(*_iscale(lo, hi, s))
    return raw, (np.pad(slo, ((1, 1), (1, 1), (0, 0))), np.pad(shi, ((1, 1), (1, 1), (0, 0))))


def rep_conv(ar: Arith, g1p, dg, cols: Optional[Tuple[int, int]] = None):
    """stage 5 on the padded g1 (lo, hi) [h + 4][w + 4][C] -> r (lo, hi) [h][w or the column range][C]"""
    h, w = g1p[0].shape[0] - 4, g1p[0].shape[1] - 4
    x0, x1 = cols if cols else (0, w)
    ng = dg.shape[0]
    kp, kn, ka = np.maximum(dg, 0.0), np.minimum(dg, 0.0), np.abs(dg)
    sh = (h, x1 - x0, ng, 8)
    lo, hi, M = np.zeros(sh), np.zeros(sh), np.zeros(sh)
    for dy in range(5):
        for dx in range(5):
            sl = g1p[0][dy:dy + h, x0 + dx:x1 + dx].reshape(sh)
            su = g1p[1][dy:dy + h, x0 + dx:x1 + dx].reshape(sh)
            e = lambda v, k: np.einsum("hwgi,goi->hwgo", v, k[:, :, :, dy, dx])      # noqa: E731
            lo += e(sl, kp) + e(su, kn)
            hi += e(su, kp) + e(sl, kn)
            M += e(np.maximum(np.abs(sl), np.abs(su)), ka)
    out = (h, x1 - x0, ng * 8)
    lo, hi = ar.acc(lo.reshape(out), hi.reshape(out), 240 + 8, M.reshape(out))
    return ar.h16(lo, hi)


def second_1x1_gate2(ar: Arith, r, W2, C: int):
    """stage 6 -> ((lo, hi) of b = [b1 | b2'], (lo, hi) of the un-rounded g2, (lo, hi) of g2 in bf16)"""
    lo, hi, M = _imatmul(r[0], r[1], W2)
    lo, hi = ar.acc(lo, hi, C + 8, M)
    with np.errstate(over="ignore"):
        s_lo, s_hi = 1.0 / (1.0 + np.exp2(hi[..., C:])), 1.0 / (1.0 + np.exp2(lo[..., C:]))
    vlo, vhi = _imul(lo[..., :C], hi[..., :C], s_lo, s_hi)
    vlo, vhi = ar.rel(vlo, vhi, RHO_GATE2)
    return (lo, hi), (vlo, vhi), ar.bf(vlo, vhi)


def pool_rows(ar: Arith, v, bounds: Sequence[int], extra_left: int = 0):
    """v (lo, hi) [n][h][w][C] -> pool rows (lo, hi) [n][strips * row blocks][C]: per (strip, block of 8 image rows) the sum over the row's own
    pixels, widened by n u sum |.|.  extra_left: strips after the first also count that many columns left of their own (negative control)."""
    n, h, w, C = v[0].shape
    nbh = -(-h // P1R_RB)
    nsx = len(bounds) - 1
    lo, hi = np.zeros((n, nsx * nbh, C)), np.zeros((n, nsx * nbh, C))
    for s in range(nsx):
        x0, x1 = bounds[s] - (extra_left if s else 0), bounds[s + 1]
        for b in range(nbh):
            y0, y1 = b * P1R_RB, min(b * P1R_RB + P1R_RB, h)
            blo, bhi = v[0][:, y0:y1, x0:x1], v[1][:, y0:y1, x0:x1]
            cnt = (y1 - y0) * (x1 - x0)
            if ar.kind == "point":
                q = blo.reshape(n, cnt, C).astype(F32).sum(1, dtype=F32).astype(F64)
                lo[:, s * nbh + b], hi[:, s * nbh + b] = q, q
            else:
                lo[:, s * nbh + b], hi[:, s * nbh + b] = ar.acc(blo.sum((1, 2)), bhi.sum((1, 2)), cnt, np.maximum(np.abs(blo), np.abs(bhi)).sum((1, 2)))
    return lo, hi


STAGES = ("u", "xn", "a", "F", "g1", "g1s", "r", "b", "v", "g2")


def frame_stages(c: P1Case, ops, fw, ar: Arith, t: int, fault: Optional[str] = None, bounds: Optional[Sequence[int]] = None) -> Dict[str, tuple]:
    """every stage of absolute frame t as (lo, hi): u, xn [h][w][K]; a, F [h][w][2C]; g1 (unscaled), g1s (as the RepConv reads it), r, v (g2 before
    its rounding), g2 [h][w][C]; b [h][w][2C].
    fault (point runs, one each): "tap3" / "rep_corner" (fw already holds the dropped tap), "bias_outside", "g1_row_above", "seam" (bounds: the
    first own column of the second strip sees zeros left of it in the RepConv), "no_eps", "one_pass", "same_frame"."""
    C, h, w = c.C, c.h, c.w
    u = gather(c, ops, t, fault)
    xn = layer_norm(ar, u, fault)
    a = first_1x1(ar, xn, fw, c.K)
    outside = None
    if fault == "bias_outside":
        outside = ar.h16(fw["b_hi"] + fw["b_lo"], fw["b_hi"] + fw["b_lo"])[0]
    Fe = stencil3(ar, a, fw["d3"], outside)
    scale = ops["g1_scale"][t].double().numpy() if ops.get("g1_scale") is not None else None
    g1, g1s = gate(ar, Fe, C, scale, keep_row_above=fault == "g1_row_above")
    r = rep_conv(ar, g1s, fw["dg"])
    if fault == "seam":
        x0 = bounds[1]
        cut = tuple(np.concatenate((np.zeros_like(g[:, :x0 + 2]), g[:, x0 + 2:]), 1) for g in g1s)
        rc = rep_conv(ar, cut, fw["dg"], (x0, x0 + 1))
        r = tuple(np.concatenate((q[:, :x0], qc, q[:, x0 + 1:]), 1) for q, qc in zip(r, rc))
    b, v, g2 = second_1x1_gate2(ar, r, fw["W2"], C)
    crop = lambda p: (p[0][2:-2, 2:-2], p[1][2:-2, 2:-2])      # noqa: E731
    return {"u": (u, u), "xn": xn, "a": a, "F": (Fe[0][1:-1, 1:-1], Fe[1][1:-1, 1:-1]), "g1": crop(g1), "g1s": crop(g1s), "r": r, "b": b, "v": v, "g2": g2}


def reference(c: P1Case, ops, ar: Optional[Arith] = None, fw=None, fault: Optional[str] = None, bounds: Optional[Sequence[int]] = None,
              want=("g2", "v", "g1")) -> Dict[str, tuple]:
    """stage -> (lo, hi) [nt][h][w][...] over c.frames for the stages in `want`.  The default run is the interval reference; it asserts the fp16
    range."""
    ar = ar or Arith("interval")
    fw = fw or folded(ops, rounded=ar.kind != "exact")
    acc: Dict[str, list] = {k: [[], []] for k in want}
    for t in c.frames:
        st = frame_stages(c, ops, fw, ar, t, fault, bounds)
        for k in want:
            acc[k][0].append(st[k][0])
            acc[k][1].append(st[k][1])
    out = {k: (np.stack(v[0]), np.stack(v[1])) for k, v in acc.items()}
    if ar.kind == "interval":
        assert ar.max16 <= MAX16, (c.id, ar.max16)
        assert all(np.isfinite(v[0]).all() and np.isfinite(v[1]).all() for v in out.values()), c.id
    return out


def stage_intervals(c: P1Case, t: int, y: int, x: int, ops=None, keep16: bool = False) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """The debug aid: the interval of every stage at pixel (y, x) of absolute frame t -- which stage did a failing element leave?  `a`, F and b hold
    the gate partners of channel ch at ch and C + ch.  keep16: the intervals that take fp16 subnormals as kept.  No kernel runs."""
    ops = ops or operands(c)
    st = frame_stages(c, ops, folded(ops), Arith("interval", keep16=keep16), t)
    return {k: (st[k][0][y, x], st[k][1][y, x]) for k in STAGES}


def strip_bounds(lib, w: int, ncu: int = 256) -> List[int]:
    """first own column of every strip, and w: sn_p1r_plan / sn_p1r_strip_begin (the strips depend on w alone)"""
    import ctypes
    o = (ctypes.c_int * 7)()
    assert lib.sn_p1r_plan(1, 1, w, ncu, 1, o) == 0
    return [lib.sn_p1r_strip_begin(o, s, w) for s in range(o[0] + 1)]


def width_stats(lo: np.ndarray, hi: np.ndarray) -> Dict[str, float]:
    """median and maximum of (hi - lo) / peak and the share of zero-width elements"""
    peak = max(float(np.abs(lo).max()), float(np.abs(hi).max()), 1e-300)
    wd = (hi - lo) / peak
    return {"peak": peak, "median": float(np.median(wd)), "max": float(wd.max()), "zero_share": float((wd == 0).mean())}


def outside(got: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """elements not inside their interval (NaN is outside)"""
    return ~((got >= lo) & (got <= hi))
