"""The small kernels of csrc/sn_conv.hip that nothing compared with anything directly: the squeeze-excite MLP (ca_mlp_kernel behind sn_ca_mlp), the
closed-form CALayer of a dense CAB (cab_ca_part_kernel<bf16_t> + cab_ca_kernel<bf16_t> behind sn_cab_ca / sn_cab_ca_lines), SkipUpSample's tail
(upsample2_add_kernel, sn_upsample2_add) and the ingest (ingest_kernel, sn_ingest).  Case tables, operand generators, float64 references with a
bound per element, and fp32 point emulations in the kernels' reduction order, shared by tests/test_host_ca_ref.py (CPU) and
tests/test_gpu_ca_kernels.py (-m gpu).

The contract of an entry point is a function of ITS OWN operands (partial, the border pixels of mid as stored, the weights), in float64:

  sn_cab_ca / sn_cab_ca_lines
    tot[ci]  = sum_b partial[t][b][ci]
    row0, row1, col0, col1 [ci] = the sums of row 0, row h-1, column 0, column w-1 of mid; k00, k01, k10, k11 its corners
    S[ci][ky][kx] = tot - rowex[ky] - colex[kx] + cor[ky][kx],  rowex = (row1, 0, row0), colex = (col1, 0, col0),
                    cor = ((k11, 0, k10), (0, 0, 0), (k01, 0, k00))       -- tap (ky, kx) reads mid(p + (ky - 1, kx - 1)): it never sees the far line
    mean[co] = (1 / (h w)) sum_ci sum_tap w2[ci][tap][co] S[ci][tap]
    hid = relu(wa mean), ca = sigmoid(wb hid); ca[c .. cpad) = 0 exactly
  sn_ca_mlp: the same tail from mean = inv_hw sum_b partial[t][b].

Bound per element of ca: the project's convention (n + 8) u M per fp32 accumulation, u = 2^-24, M the sum of the absolute addends and n the DEPTH of
the chain the kernel runs (a thread's serial additions, not the number of addends), each stated below next to the kernel line it comes from:

  total          cab_ca_part_kernel `for (bb = sidx * nsplit + part; bb < nblk; bb += SN_CABCA_NS * nsplit)`: ceil(nblk / (16 nsplit)) additions,
                 `for (q < nsplit) m += acc[...]`: nsplit, cab_ca_kernel `for (q < SN_CABCA_NS) m += sp[...]`: 16.      nsplit = 256 / cpad
                 n_tot = ceil(nblk / (16 nsplit)) + nsplit + 16
  a border line  `for (i = sidx * nseg + seg; i < len; i += SN_CABCA_NS * nseg)`: ceil(len / (16 nseg)), `for (q < nseg)`: nseg, the same 16.
                 n_line = ceil(len / (16 nseg)) + nseg + 16, nseg = 256 / cs, len = w for the rows and h for the columns
  S              `tot - rowex[ky] - colex[kx] + cor[ky][kx]`: three operations on values bounded by Ms = M_tot + M_row + M_col + |corner|:
                 E_S = e_tot + e_rowex + e_colex + 3 u Ms
  tap loop       cab_ca_kernel `for (cin = part; cin < c; cin += nsplit)` x 9 taps, then `for (q < nsplit) m += acc[...]`, nsplit = 1024 / cpad:
                 n_tap = 9 ceil(c / nsplit) + nsplit; the product's rounding and the division by (float) h (float) w sit in the + 8
                 e_mean = (sum |w2| E_S + (n_tap + 8) u sum |w2| Ms) / (h w)
  sn_ca_mlp      ca_mlp_kernel `for (b = part; b < nblk; b += nsplit)`: ceil(nblk / nsplit), `for (q < nsplit)`: nsplit, nsplit = 1024 / cpad; the
                 product with inv_hw in the + 8:  e_mean = (ceil(nblk / nsplit) + nsplit + 8) u inv_hw sum_b |partial|
  hidden layer   `for (j < c) h += wa[tid * c + j] * mean[j]`: e_hid = |wa| e_mean + (c + 8) u |wa| M_mean; ReLU is 1-Lipschitz
  output         `for (j < cr) o += wb[tid * cr + j] * hid[j]`: e_o = |wb| e_hid + (cr + 8) u |wb| |wa| M_mean
  sigmoid        slope <= 1/4; __expf (1 ulp, and the scaling of its argument: |o| ulps), the addition, v_rcp_f32 (1 ulp):
                 tol = e_o / 4 + (3 + |o|) 2^-23      (DESIGN 3.22 derives the last term for the fold's tail)

On dense data this worst case is loose by three orders of magnitude (an fp32 emulation in the kernel's order sits at <= 2e-3 of it), so the bound alone
would let a dropped corner through on anything but the smallest maps.  The discriminating power comes from the operands -- three families per case:
  (a) dense: mid = bf16(PReLU(noise x 2^U(-3, 3) per channel)) (one variant + 8: cancellation in tot - row - col), partial = its exact block sums
      rounded to fp32, weights of a named module through Engine's own Plan.add_cab packing;
  (b) impulse rows: partial zero but for ONE row b* per frame, b* on every seam of the 16 x nsplit split, mid zero: the bound collapses to that
      row's terms and a row skipped or counted twice is a change of 100 %;
  (c) impulse pixels: partial zero, mid zero but for one pixel per frame: each corner, the seams of the lines' 16 x nseg split, one interior pixel
      (which must leave ca at its zero-input value).
A frame whose hidden layer is all zero gives ca = 0.5 under every fault: dense seeds are chosen (by the reference alone) so that at least two hidden
units are positive and no |o| exceeds 8 in every frame, and an impulse's sign is chosen likewise.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

U = 2.0 ** -24
NS = 16                         # SN_CABCA_NS of csrc/sn_conv.hip
EINVAL = -22
F32, F64 = np.float32, np.float64
T = 3                           # frames per launch
CONTROL_RATIO = 8.0             # what a control must leave its bound by (the ratio of the bf16 conv pin)

# (variant, module, c, cs, cpad): the channel configurations of the network's dense CABs; cr comes from the state dict (c / 4, or c where
# the variant forces reduction = 1).  The module of a width is one whose synthetic weights keep |o| <= 8 under the + 8 offset on all nine maps
# (the offset alone puts 8 sum(w2) into the mean: orb1.encoder_level2.0 of gshift_deblur1 and stage1.skip_attn1 of gshift_denoise2 end at
# |o| = 9 .. 11.5 whatever the seed, where the sigmoid's slope is 1e-5 and the scale says nothing)
CONFIGS = [
    ("gshift_deblur2", "feat_extract.1.", 14, 16, 16),
    ("gshift_denoise2", "orb1.encoder_level2.0.", 18, 24, 32),
    ("gshift_deblur2", "orb1.encoder_level3.0.", 22, 24, 32),
    ("gshift_deblur1", "feat_extract.1.", 24, 24, 32),
    ("gshift_deblur1", "orb1.encoder_level2.2.", 36, 40, 48),
    ("gshift_deblur1", "orb1.encoder_level3.0.", 48, 48, 48),
    ("gshift_deblur2", "stage1.skip_attn1.", 64, 64, 64),
    ("gshift_deblur1", "stage1.encoder_level1.", 80, 80, 80),
]
# (h, w, nblk): None = min(h w, 5) rows; "split" = 16 nsplit + 1 rows (the total's strided loop takes a second trip)
MAPS = [(2, 2, None), (2, 3, None), (3, 2, None), (5, 7, None), (17, 2, None), (2, 300, None), (300, 2, None), (13, 70, 40), (37, 33, "split")]


@dataclass(frozen=True)
class CabCase:
    id: str
    variant: str
    pre: str
    c: int
    cs: int
    cpad: int
    h: int
    w: int
    nblk: int
    seed: int

    @property
    def nsplit(self) -> int:        # cab_ca_part_kernel: rows of partial per workgroup and trip
        return 256 // self.cpad

    @property
    def nseg(self) -> int:          # cab_ca_part_kernel: pixels of a border line per workgroup and trip
        return 256 // self.cs


@dataclass(frozen=True)
class MlpCase:
    id: str
    c: int
    cpad: int
    cr: int
    nblk: int
    seed: int

    @property
    def nsplit(self) -> int:        # ca_mlp_kernel
        return 1024 // self.cpad


def _cab_cases() -> List[CabCase]:
    out = []
    for k, (variant, pre, c, cs, cpad) in enumerate(CONFIGS):
        for j, (h, w, nb) in enumerate(MAPS):
            nblk = min(h * w, 5) if nb is None else (16 * (256 // cpad) + 1 if nb == "split" else nb)
            out.append(CabCase(f"cab{c}_{h}x{w}_b{nblk}", variant, pre, c, cs, cpad, h, w, nblk, 1000 * (k + 1) + 10 * j))
    return out


def _mlp_cases() -> List[MlpCase]:
    out = []
    for k, cpad in enumerate((16, 32, 48, 64, 80, 128)):
        for c in (cpad, cpad - 2):
            ns = 1024 // cpad
            for j, nblk in enumerate((1, ns - 1, ns, ns + 1, 1000)):
                out.append(MlpCase(f"mlp{c}of{cpad}_b{nblk}", c, cpad, c // 4, nblk, 50000 + 100 * k + 10 * j + (c != cpad)))
    return out


CAB_CASES = _cab_cases()
MLP_CASES = _mlp_cases()


def cab_by_id(i: str) -> CabCase:
    return next(c for c in CAB_CASES if c.id == i)


# ---- weights -------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _state_dict(variant: str):
    from shiftnet_amd.weights import synth_state_dict
    return synth_state_dict(variant)


def light_plan(variant: str, pres, device=torch.device("cpu")):
    """A Plan that holds only the named CABs, built by Engine's own Plan.add_cab (pack_conv, the CALayer matrices and the fp32 [cin][9][cpad]
    copy of conv2, bf16-rounded): the packing under test, without the seconds a whole checkpoint takes."""
    from shiftnet_amd.engine import Plan, host_f32_copy
    from shiftnet_amd.spec import VARIANTS
    sd = _state_dict(variant)
    P = Plan.__new__(Plan)
    P.V, P.device = VARIANTS[variant], device
    P.sd = host_f32_copy({k: v for k, v in sd.items() if any(k.startswith(p) for p in pres)})
    P.convs, P.cas, P.units = {}, {}, {}
    for pre in pres:
        P.add_cab(pre, sd[pre + "body.0.weight"].shape[0])
    return P


@functools.lru_cache(maxsize=None)
def cab_weights(variant: str, pre: str) -> Dict[str, object]:
    """w2 [c][9][cpad], wa [cr][c], wb [c][cr] (fp32 numpy, exactly the device operands of Engine.cab), the PReLU slope and cr"""
    P = light_plan(variant, (pre,))
    q = P.cas[pre + "CA"]
    return {"w2": q["w2"].numpy().copy(), "wa": q["wa"].numpy().copy(), "wb": q["wb"].numpy().copy(), "c": int(q["c"]), "cr": int(q["cr"]),
            "cpad": int(q["w2"].shape[2]), "cs": int(P.convs[pre + "body.0"]["cs_in"]), "slope": P.scalar(pre + "body.1.weight")}


def mlp_weights(case: MlpCase) -> Dict[str, np.ndarray]:
    g = torch.Generator().manual_seed(case.seed // 10 * 10 + 7)          # one draw per (cpad, c), shared by its nblk rows
    wa = (torch.randn((case.cr, case.c), generator=g) / math.sqrt(case.c)).float().numpy()
    wb = (torch.randn((case.c, case.cr), generator=g) / math.sqrt(case.cr)).float().numpy()
    return {"wa": wa, "wb": wb}


# ---- the float64 contract ------------------------------------------------------------------------------------------------------------------

def _tail(mean, m_mean, e_mean, wa, wb, c, cr, cpad, relu=True):
    """hid = relu(wa mean), ca = sigmoid(wb hid) in float64 with the bound carried through |wa|, the ReLU, |wb| and the sigmoid"""
    A, B = np.asarray(wa, F64), np.asarray(wb, F64)
    pre = mean @ A.T
    m_hid = m_mean @ np.abs(A).T
    e_hid = e_mean @ np.abs(A).T + (c + 8) * U * m_hid                    # for (j < c) h += wa[tid * c + j] * mean[j]: depth c
    hid = np.maximum(pre, 0.0) if relu else pre
    o = hid @ B.T
    e_o = e_hid @ np.abs(B).T + (cr + 8) * U * (m_hid @ np.abs(B).T)      # for (j < cr) o += wb[tid * cr + j] * hid[j]: depth cr
    ca = np.zeros(mean.shape[:-1] + (cpad,), F64)
    tol = np.zeros_like(ca)
    ca[..., :c] = 1.0 / (1.0 + np.exp(-o))
    tol[..., :c] = 0.25 * e_o + (3.0 + np.abs(o)) * 2.0 ** -23
    return {"ca": ca, "tol": tol, "o": o, "hid_pre": pre, "mean": mean, "e_mean": e_mean}


def line_sums(mid):
    """[F][h][w][cs] -> the four border-line sums [F][cs] (row 0, row h-1, column 0, column w-1) and the corners"""
    h, w = mid.shape[1], mid.shape[2]
    return ((mid[:, 0].sum(1), mid[:, h - 1].sum(1), mid[:, :, 0].sum(1), mid[:, :, w - 1].sum(1)),
            (mid[:, 0, 0], mid[:, 0, w - 1], mid[:, h - 1, 0], mid[:, h - 1, w - 1]))


def _s_taps(tot, lines, corners):
    """S[F][c][9] of the closed form from the total, the line sums and the corners (any dtype: float64 here, fp32 in the emulation)"""
    r0, r1, c0, c1 = lines
    k00, k01, k10, k11 = corners
    z = np.zeros_like(tot)
    rowex, colex = (r1, z, r0), (c1, z, c0)
    cor = ((k11, z, k10), (z, z, z), (k01, z, k00))
    return np.stack([((tot - rowex[ky]) - colex[kx]) + cor[ky][kx] for ky in range(3) for kx in range(3)], -1)


def cab_ca_reference(case: CabCase, wts, partial, mid, relu=True, e_tot_extra=None):
    """The contract of sn_cab_ca on operands partial [F][nblk][cpad], mid [F][h][w][cs] (any float dtype; evaluated in float64).
    e_tot_extra [F][c]: a further uncertainty of the total (the chain check: the pool sums fp32 accumulators, mid stores their bf16 roundings)"""
    c, cs, cpad, h, w, nblk = case.c, case.cs, case.cpad, case.h, case.w, case.nblk
    P, Mi = np.asarray(partial, F64)[..., :c], np.asarray(mid, F64)[..., :c]
    W2 = np.asarray(wts["w2"], F64)[:c, :, :c]
    n_tot = -(-nblk // (NS * case.nsplit)) + case.nsplit + NS
    n_row = -(-w // (NS * case.nseg)) + case.nseg + NS
    n_col = -(-h // (NS * case.nseg)) + case.nseg + NS
    tot, m_tot = P.sum(1), np.abs(P).sum(1)
    lines, corners = line_sums(Mi)
    m_lines, m_corners = line_sums(np.abs(Mi))
    S = _s_taps(tot, lines, corners)
    e_tot = (n_tot + 8) * U * m_tot + (0.0 if e_tot_extra is None else np.asarray(e_tot_extra, F64))
    e_lines = tuple((n + 8) * U * m for n, m in zip((n_row, n_row, n_col, n_col), m_lines))
    z = np.zeros_like(tot)
    # sums of absolute values / of the bounds, tap by tap: the same selection as S with every sign positive
    r0, r1, c0, c1 = m_lines
    k00, k01, k10, k11 = m_corners
    rowex, colex, cor = (r1, z, r0), (c1, z, c0), ((k11, z, k10), (z, z, z), (k01, z, k00))
    Ms = np.stack([m_tot + rowex[ky] + colex[kx] + cor[ky][kx] for ky in range(3) for kx in range(3)], -1)
    er0, er1, ec0, ec1 = e_lines
    erow, ecol = (er1, z, er0), (ec1, z, ec0)
    Es = np.stack([e_tot + erow[ky] + ecol[kx] for ky in range(3) for kx in range(3)], -1) + 3 * U * Ms
    ns2 = 1024 // cpad
    n_tap = 9 * -(-c // ns2) + ns2
    mean = np.einsum("fit,ito->fo", S, W2) / (h * w)
    m_mean = np.einsum("fit,ito->fo", Ms, np.abs(W2)) / (h * w)
    e_mean = np.einsum("fit,ito->fo", Es, np.abs(W2)) / (h * w) + (n_tap + 8) * U * m_mean
    return _tail(mean, m_mean, e_mean, wts["wa"], wts["wb"], c, wts["wa"].shape[0], cpad, relu)


def ca_mlp_reference(case: MlpCase, wts, partial, inv_hw):
    """The contract of sn_ca_mlp on partial [F][nblk][cpad] and the fp32 factor inv_hw"""
    P = np.asarray(partial, F64)[..., :case.c]
    inv = float(F32(inv_hw))
    n = -(-case.nblk // case.nsplit) + case.nsplit
    mean, m_mean = P.sum(1) * inv, np.abs(P).sum(1) * inv
    return _tail(mean, m_mean, (n + 8) * U * m_mean, wts["wa"], wts["wb"], case.c, case.cr, case.cpad)


def torch_calayer(case: CabCase, wts, mid):
    """float64 torch: conv2d(mid, w2, padding=1).mean((2, 3)) into the MLP -- what the closed form stands for.  [F][c]"""
    import torch.nn.functional as Fn
    c = case.c
    x = torch.from_numpy(np.asarray(mid, F64)[..., :c]).permute(0, 3, 1, 2)
    w = torch.from_numpy(np.asarray(wts["w2"], F64)[:c, :, :c]).permute(2, 0, 1).reshape(c, c, 3, 3)
    mean = Fn.conv2d(x, w, padding=1).mean((2, 3))
    hid = torch.relu(mean @ torch.from_numpy(np.asarray(wts["wa"], F64)).T)
    return torch.sigmoid(hid @ torch.from_numpy(np.asarray(wts["wb"], F64)).T).numpy()


def condition(ref) -> bool:
    """every frame: at least two hidden units positive, no |o| above 8"""
    return bool(((ref["hid_pre"] > 0).sum(-1) >= 2).all() and (np.abs(ref["o"]) <= 8.0).all())


# ---- operands ------------------------------------------------------------------------------------------------------------------------------

def bf16(x: np.ndarray) -> np.ndarray:
    """round to bf16 (nearest even), returned as float32"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(torch.bfloat16).float().numpy()


def block_of_pixel(case: CabCase) -> np.ndarray:
    """the partial row every pixel (row major) is summed into: nblk contiguous runs"""
    n = case.h * case.w
    return (np.arange(n) * case.nblk) // n


def block_sums(case: CabCase, mid: np.ndarray, dtype=F32) -> np.ndarray:
    """partial [F][nblk][cpad]: the exact per-block sums of mid (float64), rounded to `dtype`; pad channels zero"""
    Fr = mid.shape[0]
    flat = np.asarray(mid, F64).reshape(Fr, case.h * case.w, case.cs)
    out = np.zeros((Fr, case.nblk, case.cpad), F64)
    blk = block_of_pixel(case)
    for b in range(case.nblk):
        out[:, b, :case.c] = flat[:, blk == b, :case.c].sum(1)
    return out.astype(dtype)


def _dense_draw(case: CabCase, wts, seed: int, offset: float):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((T, case.h, case.w, case.cs), generator=g) * torch.exp2(torch.rand((T, 1, 1, case.cs), generator=g) * 6.0 - 3.0)
    x = torch.where(x >= 0, x, x * wts["slope"]) + offset
    x[..., case.c:] = 0.0
    mid = x.to(torch.bfloat16).float().numpy()
    return block_sums(case, mid), mid


MAX_SEED_TRIES = 64


def dense_operands(case: CabCase, offset: float = 0.0):
    """family (a): (partial fp32 [T][nblk][cpad], mid bf16-valued fp32 [T][h][w][cs], tries).  The seed is the first from the case's own at which
    the reference alone says that every frame has two positive hidden units and |o| <= 8 (nothing is skipped; the CPU test bounds the tries)."""
    wts = cab_weights(case.variant, case.pre)
    for k in range(MAX_SEED_TRIES):
        partial, mid = _dense_draw(case, wts, case.seed + 7919 * k + (1 if offset else 0), offset)
        if condition(cab_ca_reference(case, wts, partial, mid)):
            return partial, mid, k + 1
    raise AssertionError(f"{case.id}: no seed meets the condition")


def seam_rows(nblk: int, nsplit: int, outer: int = NS) -> List[int]:
    """the rows of partial at the seams of the outer x nsplit split"""
    s = {0, nsplit - 1, nsplit, outer * nsplit - 1, outer * nsplit, nblk - 1}
    return sorted(b for b in s if 0 <= b < nblk)


def seam_index(n: int, inner: int, outer: int = NS) -> int:
    """the element a seam control drops or doubles: the first of the second trip, else the first of the second workgroup, else the last"""
    return outer * inner if outer * inner < n else (inner if inner < n else n - 1)


def line_points(n: int, nseg: int) -> List[int]:
    """indices along a border line of n pixels: both ends, and both sides of the seams of the 16 x nseg split"""
    s = {0, 1, nseg - 1, nseg, NS * nseg - 1, NS * nseg, n - 2, n - 1}
    return sorted(i for i in s if 0 <= i < n)


def impulse_pixels(case: CabCase) -> List[Tuple[int, int, str]]:
    """(y, x, what) of family (c): every corner, the seam pixels of each border line, one interior pixel where the map has one"""
    h, w = case.h, case.w
    px: Dict[Tuple[int, int], str] = {}
    for (y, x) in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        px[(y, x)] = "corner"
    for i in line_points(w, case.nseg):
        px.setdefault((0, i), "row0")
        px.setdefault((h - 1, i), "row1")
    for i in line_points(h, case.nseg):
        px.setdefault((i, 0), "col0")
        px.setdefault((i, w - 1), "col1")
    if h > 2 and w > 2:
        px[(1, 1)] = "interior"
    return [(y, x, k) for (y, x), k in px.items()]


def _orient(case, wts, partial, mid):
    """flip the sign of every frame with fewer than two positive hidden units (the mean is linear in the impulse: with cr >= 3 one sign has two)"""
    ref = cab_ca_reference(case, wts, partial, mid)
    flip = (ref["hid_pre"] > 0).sum(-1) < 2
    partial[flip] *= -1
    mid[flip] *= -1
    return partial, mid


def impulse_row_operands(case: CabCase):
    """family (b): (partial [F][nblk][cpad], mid zeros [F][h][w][cs], rows): frame f has the single row rows[f], O(h w) per channel"""
    wts = cab_weights(case.variant, case.pre)
    rows = seam_rows(case.nblk, case.nsplit)
    g = torch.Generator().manual_seed(case.seed + 3)
    partial = np.zeros((len(rows), case.nblk, case.cpad), F32)
    for f, b in enumerate(rows):
        partial[f, b, :case.c] = (torch.randn(case.c, generator=g) * float(case.h * case.w)).numpy()
    mid = np.zeros((len(rows), case.h, case.w, case.cs), F32)
    partial, mid = _orient(case, wts, partial, mid)
    return partial, mid, rows


def impulse_pixel_operands(case: CabCase):
    """family (c): (partial zeros, mid [F][h][w][cs], pixels): frame f has the single pixel pixels[f], bf16 values of O(h w) per channel"""
    wts = cab_weights(case.variant, case.pre)
    px = impulse_pixels(case)
    g = torch.Generator().manual_seed(case.seed + 5)
    amp = 2.0 ** math.ceil(math.log2(case.h * case.w))
    mid = np.zeros((len(px), case.h, case.w, case.cs), F32)
    for f, (y, x, _) in enumerate(px):
        mid[f, y, x, :case.c] = bf16((torch.randn(case.c, generator=g) * amp).numpy())
    partial = np.zeros((len(px), case.nblk, case.cpad), F32)
    partial, mid = _orient(case, wts, partial, mid)
    return partial, mid, px


def mlp_operands(case: MlpCase):
    """sn_ca_mlp: dense partial [T][nblk][cpad] (pad channels zero), inv_hw, tries; the seed chosen as for the dense CAB operands"""
    wts = mlp_weights(case)
    inv_hw = F32(1.0 / (4.0 * case.nblk))
    for k in range(MAX_SEED_TRIES):
        g = torch.Generator().manual_seed(case.seed + 7919 * k)
        # rows of 4 sqrt(nblk) x noise x 2^U(-3, 1) per channel: the mean is O(1) and of either sign whatever nblk is
        p = 4.0 * math.sqrt(case.nblk) * torch.randn((T, case.nblk, case.cpad), generator=g) * torch.exp2(torch.rand((T, 1, case.cpad), generator=g) * 4.0 - 3.0)
        p[..., case.c:] = 0.0
        p = p.float().numpy()
        if condition(ca_mlp_reference(case, wts, p, inv_hw)):
            return p, inv_hw, k + 1
    raise AssertionError(f"{case.id}: no seed meets the condition")


def mlp_impulse_operands(case: MlpCase):
    """sn_ca_mlp, impulse rows at the seams of its 1 x nsplit split"""
    wts = mlp_weights(case)
    inv_hw = F32(1.0 / (4.0 * case.nblk))
    rows = seam_rows(case.nblk, case.nsplit, 1)
    g = torch.Generator().manual_seed(case.seed + 3)
    p = np.zeros((len(rows), case.nblk, case.cpad), F32)
    for f, b in enumerate(rows):
        p[f, b, :case.c] = (torch.randn(case.c, generator=g) * 4.0 * case.nblk).numpy()
    flip = (ca_mlp_reference(case, wts, p, inv_hw)["hid_pre"] > 0).sum(-1) < 2
    p[flip] *= -1
    return p, inv_hw, rows


# ---- fp32 point emulations in the kernels' order --------------------------------------------------------------------------------------------

def split_sum(x: np.ndarray, outer: int, inner: int, skip: Optional[int] = None, twice: Optional[int] = None) -> np.ndarray:
    """[F][N][C] fp32 -> [F][C]: element i goes to thread (i / inner % outer, i % inner) of trip i / (outer inner); a thread adds its trips in
    order, then the inner threads are added in order, then the outer groups -- the three loops of cab_ca_part_kernel / cab_ca_kernel (outer = 16)
    or the two of ca_mlp_kernel (outer = 1).  skip / twice: the element a faulty kernel leaves out / counts twice."""
    Fr, N, C = x.shape
    G = outer * inner
    K = -(-N // G)
    pad = np.zeros((Fr, K * G, C), F32)
    pad[:, :N] = x
    if skip is not None:
        pad[:, skip] = 0
    if twice is not None:
        pad[:, twice] = pad[:, twice] * F32(2)
    v = pad.reshape(Fr, K, outer, inner, C)
    s = np.zeros((Fr, outer, inner, C), F32)
    for k in range(K):
        s = s + v[:, k]
    m = np.zeros((Fr, outer, C), F32)
    for q in range(inner):
        m = m + s[:, :, q]
    t = np.zeros((Fr, C), F32)
    for q in range(outer):
        t = t + m[:, q]
    return t


def _mac(r, a, b, fma):
    if fma:
        return (r.astype(F64) + a.astype(F64) * b.astype(F64)).astype(F32)
    return r + a * b


def _emu_tail(mean, wa, wb, c, cr, cpad, fma, relu=True):
    wa, wb = np.asarray(wa, F32), np.asarray(wb, F32)
    hid = np.zeros(mean.shape[:1] + (cr,), F32)
    for j in range(c):
        hid = _mac(hid, wa[None, :, j], mean[:, j:j + 1], fma)
    if relu:
        hid = np.maximum(hid, F32(0))
    o = np.zeros(mean.shape[:1] + (c,), F32)
    for j in range(cr):
        o = _mac(o, wb[None, :, j], hid[:, j:j + 1], fma)
    ca = np.zeros(mean.shape[:1] + (cpad,), F32)
    ca[:, :c] = (1.0 / (1.0 + np.exp(-o.astype(F64)))).astype(F32)
    return ca


CAB_FAULTS = ("rows_swapped", "cols_swapped", "corner_dropped", "corners_swapped", "divisor", "row_skipped", "row_doubled", "pixel_skipped",
              "w2_transposed", "no_relu")
SEAM_FAULTS = {"row_skipped": "rows", "row_doubled": "rows", "pixel_skipped": "pixels"}      # the family that must catch it in EVERY case


def emulate_cab_ca(case: CabCase, wts, partial, mid, fma: bool = False, fault: Optional[str] = None) -> np.ndarray:
    """ca [F][cpad] as the two kernels compute it in fp32, optionally with one fault"""
    assert fault is None or fault in CAB_FAULTS, fault
    c, cs, cpad, h, w = case.c, case.cs, case.cpad, case.h, case.w
    P, Mi = np.asarray(partial, F32), np.asarray(mid, F32)
    sb = seam_index(case.nblk, case.nsplit)
    tot = split_sum(P, NS, case.nsplit, skip=sb if fault == "row_skipped" else None, twice=sb if fault == "row_doubled" else None)[:, :c]
    src = (Mi[:, 0], Mi[:, h - 1], Mi[:, :, 0], Mi[:, :, w - 1])
    lines = [split_sum(np.ascontiguousarray(s), NS, case.nseg, skip=seam_index(s.shape[1], case.nseg) if (fault == "pixel_skipped" and q == 0) else None)[:, :c]
             for q, s in enumerate(src)]
    k00, k01, k10, k11 = (Mi[:, 0, 0, :c], Mi[:, 0, w - 1, :c], Mi[:, h - 1, 0, :c], Mi[:, h - 1, w - 1, :c])
    if fault == "rows_swapped":
        lines[0], lines[1] = lines[1], lines[0]
    if fault == "cols_swapped":
        lines[2], lines[3] = lines[3], lines[2]
    if fault == "corner_dropped":
        k11 = np.zeros_like(k11)
    if fault == "corners_swapped":
        k01, k10 = k10, k01
    S = _s_taps(tot, tuple(lines), (k00, k01, k10, k11))                  # fp32: ((tot - rowex) - colex) + cor, the zeros exact
    W2 = np.asarray(wts["w2"], F32)
    if fault == "w2_transposed":                                           # w2 read as [co][9][ci]
        Wt = np.zeros_like(W2)
        Wt[:, :, :c] = W2[:c, :, :c].transpose(2, 1, 0)
        W2 = Wt
    ns2 = 1024 // cpad
    K2 = -(-c // ns2)
    Sp = np.zeros((S.shape[0], K2 * ns2, 9), F32)
    Sp[:, :c] = S
    Wp = np.zeros((K2 * ns2, 9, cpad), F32)
    Wp[:c] = W2[:c]
    Sp, Wp = Sp.reshape(-1, K2, ns2, 9), Wp.reshape(K2, ns2, 9, cpad)
    r = np.zeros((S.shape[0], ns2, cpad), F32)
    for k in range(K2):                                                    # for (cin = part; cin < c; cin += nsplit), nine taps each
        for tap in range(9):
            r = _mac(r, Wp[None, k, :, tap, :], Sp[:, k, :, tap, None], fma)
    m = np.zeros((S.shape[0], cpad), F32)
    for q in range(ns2):
        m = m + r[:, q]
    div = F32(h) * F32(w) + (F32(1) if fault == "divisor" else F32(0))
    mean = (m / div).astype(F32)
    return _emu_tail(mean, wts["wa"], wts["wb"], c, wts["wa"].shape[0], cpad, fma, relu=fault != "no_relu")


MLP_FAULTS = ("row_skipped", "row_doubled", "no_relu")


def emulate_ca_mlp(case: MlpCase, wts, partial, inv_hw, fma: bool = False, fault: Optional[str] = None) -> np.ndarray:
    assert fault is None or fault in MLP_FAULTS, fault
    sb = seam_index(case.nblk, case.nsplit, 1)
    m = split_sum(np.asarray(partial, F32), 1, case.nsplit, skip=sb if fault == "row_skipped" else None, twice=sb if fault == "row_doubled" else None)
    return _emu_tail((m * F32(inv_hw)).astype(F32), wts["wa"], wts["wb"], case.c, case.cr, case.cpad, fma, relu=fault != "no_relu")


def ratio(got, ref) -> float:
    """max |got - ca| / tol over the logical channels (pad channels must be exactly 0: inf otherwise)"""
    got = np.asarray(got, F64)
    c = ref["o"].shape[-1]
    if not np.isfinite(got).all() or (got[..., c:] != 0).any():
        return float("inf")
    return float((np.abs(got[..., :c] - ref["ca"][..., :c]) / ref["tol"][..., :c]).max())


# ---- sn_upsample2_add ----------------------------------------------------------------------------------------------------------------------

UP_MAPS = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 43)]
UP_CS = [8, 16, 24, 40, 48, 64, 80]
UP_T = 2
UP_FAULTS = ("align_corners", "weights_exchanged", "no_clamp_low", "no_clamp_high")


def up_axis(n: int, fault: Optional[str] = None):
    """nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False) along one axis of n samples: (i0, i1, w0, w1) per output index;
    src = max(o / 2 - 0.25, 0), i1 clamped at n - 1.  A fault reads zero where the missing clamp would have read outside."""
    o = np.arange(2 * n, dtype=F64)
    src = o * 0.5 - 0.25
    if fault == "align_corners":
        src = o * (n - 1) / max(2 * n - 1, 1)
    if fault != "no_clamp_low":
        src = np.maximum(src, 0.0)
    i0 = np.floor(src).astype(np.int64)
    lam = src - i0
    if fault == "weights_exchanged":
        lam = np.where((lam > 0) & (lam < 1), 1.0 - lam, lam)
    i1 = i0 + 1
    w0, w1 = 1.0 - lam, lam
    if fault == "no_clamp_high":
        w1 = np.where(i1 > n - 1, 0.0, w1)
    w0 = np.where(i0 < 0, 0.0, w0)
    return np.clip(i0, 0, n - 1), np.clip(i1, 0, n - 1), w0, w1


def upsample_add_reference(lo, res, fault: Optional[str] = None):
    """float64 bilinear_x2(lo) + res on NHWC [T][hs][ws][cs] / [T][2 hs][2 ws][cs], and the bound 6 u sum |terms|: the kernel rounds the two
    column interpolations' sums (their products are exact: bf16 x 0.25 / 0.75), two row products, their sum and the residual's addition"""
    lo, res = np.asarray(lo, F64), np.asarray(res, F64)
    hs, ws = lo.shape[1], lo.shape[2]
    y0, y1, a0, a1 = up_axis(hs, fault)
    x0, x1, b0, b1 = up_axis(ws, fault)

    def interp(v):
        rows = v[:, y0] * a0[None, :, None, None] + v[:, y1] * a1[None, :, None, None]
        return rows[:, :, x0] * b0[None, None, :, None] + rows[:, :, x1] * b1[None, None, :, None]
    ref = interp(lo) + res
    m = interp(np.abs(lo)) + np.abs(res)
    return ref, 6 * U * m


def round_bf16_f64(x: np.ndarray) -> np.ndarray:
    """float64 x rounded to nearest even at 8 significant bits, exactly (normal range)"""
    m, ex = np.frexp(x)
    ex = np.maximum(ex, -125)
    return np.round(np.ldexp(x, 8 - ex)) * np.exp2((ex - 8).astype(F64))


def upsample_interval(ref, tol):
    """[lo, hi]: every bf16 value the store can produce from an fp32 result within tol of ref (rounding is monotone)"""
    return round_bf16_f64(ref - tol), round_bf16_f64(ref + tol)


def upsample_operands(hs: int, ws: int, cs: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    act = lambda shp: (torch.randn(shp, generator=g) * torch.exp2(torch.rand(shp, generator=g) * 8.0 - 4.0)).to(torch.bfloat16)      # noqa: E731
    return act((UP_T, hs, ws, cs)), act((UP_T, 2 * hs, 2 * ws, cs))


def upsample_impulses(hs: int, ws: int):
    """(y, x) of the one-hot inputs: each corner and one interior pixel (where the map has one)"""
    px = {(0, 0), (0, ws - 1), (hs - 1, 0), (hs - 1, ws - 1)}
    if hs > 2 and ws > 2:
        px.add((1, ws // 2))
    return sorted(px)


# ---- sn_ingest -----------------------------------------------------------------------------------------------------------------------------

INGEST_HW = [1, 255, 257]
INGEST_T = 2
# fp32 values whose bf16 rounding is the point: ties to even downwards (1 + 2^-8 -> 1) and upwards (1 + 3 2^-8 -> 1 + 2^-6), the same negated, +-0,
# just below a tie and just above, a value that rounds up into the next binade (2 - 2^-9 -> 2), the largest fp32 (-> inf) and the largest bf16
INGEST_SPECIALS = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 0.0, -0.0, 1.0 + 2.0 ** -8 - 2.0 ** -23,
                   1.0 + 2.0 ** -8 + 2.0 ** -23, 2.0 - 2.0 ** -9, -(2.0 - 2.0 ** -9), 3.4028234663852886e38, -3.4028234663852886e38,
                   3.3895313892515355e38, 0.99609375 + 2.0 ** -9]


def ingest_operands(dtype: torch.dtype, C: int, HW: int, noise: bool, seed: int):
    """src [T][C][HW] and the noise plane [T][1][HW] (or None) of `dtype`: noise x 2^U(-6, 6) (no subnormals of any format), the fp32 sources with
    the rounding specials spread over channels and pixels"""
    g = torch.Generator().manual_seed(seed)

    def draw(shp):
        x = torch.randn(shp, generator=g) * torch.exp2(torch.rand(shp, generator=g) * 12.0 - 6.0)
        x = torch.where(x.abs() < 2.0 ** -10, torch.full_like(x, 0.5), x)
        if dtype == torch.float32:
            flat = x.reshape(-1)
            sp = torch.tensor(INGEST_SPECIALS, dtype=torch.float32)
            idx = (torch.arange(len(sp)) * 37) % flat.numel()
            flat[idx] = sp                                             # (HW = 1: the later specials overwrite the earlier ones; the larger sizes hold all)
        return x.to(dtype)
    return draw((INGEST_T, C, HW)), (draw((INGEST_T, 1, HW)) if noise else None)


def ingest_reference(src: torch.Tensor, noise: Optional[torch.Tensor]) -> torch.Tensor:
    """[T][HW][8] bf16: torch's own rounding, channel c in lane c, the noise plane in lane C, zero above"""
    Tn, C, HW = src.shape
    out = torch.zeros((Tn, HW, 8), dtype=torch.bfloat16)
    out[..., :C] = src.to(torch.bfloat16).permute(0, 2, 1)
    if noise is not None:
        out[..., C] = noise.to(torch.bfloat16)[:, 0]
    return out
