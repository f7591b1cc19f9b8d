"""The frames the tests of the CLIs' I/O edges run on (csrc/sn_io.hip: ``sn_ingest_u8``, ``sn_egress_u8``, ``sn_ssim_u8``), and their references:
seeded generators, numpy and scipy only, nothing of a GPU.  tests/test_host_io_ref.py asserts the conditions that keep the GPU test honest (the
yardstick's own error, the ties, the pass counts), tests/test_gpu_io_edges.py runs the kernels.

Sizes.  ``egress_u8_kernel`` walks a frame in passes of sn_egress_blocks() * 256 = 16 384 pixels and ``ssim_hpass_kernel`` in passes of sn_ssim_blocks() *
256 = 32 768; ``SIZES`` states how many passes each size makes, and the host test checks the table against the library, so it cannot go stale.

Contents, ``clip(content, T, H, W)`` -> (gt uint8 [T, H, W, 3], out float32 [T, 3, H, W]); the frames of a clip have seeds of their own, so they
differ in content and in error and a wrong frame stride shows:
  texture     random codes, out = gt / 255 + noise of 20 codes: values below 0 and above 1, the clamp matters;
  flat250_s1, flat128_s2, flat2_s1
              one code everywhere in gt, out = gt / 255 + Gaussian noise of that many codes: near-flat areas far from mid-grey (and at it), where
              G(a a) - G(a)^2 is tiny against its terms and is divided by something close to c2 -- sky, walls, night, bars;
  sky         a vertical ramp from 180 to 240, the same in the three channels, noise of 2 codes;
  equal       out == gt / 255 exactly as float32: SSE 0, PSNR inf, SSIM 1.  (Rounded to fp16 or bf16 it is no longer equal; what is exact is asserted
              at float32.)
``egress_clip`` puts ``TIES`` into the first frame of ``texture`` -- float32 x for which float32(x) * float32(255) is exactly k + 0.5, found by search at
import, with 0.5 (exact in all three dtypes), exact 0 and 1, -0.0 and values just inside and outside [0, 1] -- and gives the T = 3 ``equal`` clip
two texture frames as neighbours.

References.
  image  v = float32(clamp(x, 0, 1)) * float32(255), rounded once; the byte is rint(v), ties to even: the kernel's arithmetic, checked byte for byte.
  SSE    per frame sum((float64(v) - gt)^2) in float64.  The kernel's v - gt is exact only if it is formed from the ROUNDED v (|v - gt| <= 255 is a
         multiple of v's last place), so this reference also pins that the product is not fused into the difference.
         ``sse_bound``: |sse_dev - sse_ref| <= (3 ceil(HW / 16384) + 14) 2^-24 sse_ref -- one rounding of v - gt, squared (counts as 2); at most 3 passes
         fused accumulations per lane; at most 10 levels of the wave and LDS tree; 2 spare.  Every term is non-negative, so a relative bound holds.
  SSIM   ``cli.ssim_calculate`` (scipy, the CLI's own formula) is the yardstick, at the project's stated contract of 2e-5; ``ssim_f64`` is the same
         function in float64, printed beside it.  At (1, 1) and (3, 5) only ``texture`` and ``equal`` run: at one pixel the float32 yardstick itself is
         2.7e-5 from float64 on flat bright content."""
from __future__ import annotations

import math
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

Size = namedtuple("Size", "H W egress_passes ssim_passes why")
SIZES = [
    Size(1, 1, 1, 1, "smallest frame"),
    Size(3, 5, 1, 1, "the reflection folds twice"),
    Size(6, 13, 1, 1, "H below the filter radius + 1"),
    Size(9, 300, 1, 1, "two column blocks in the W pass"),
    Size(40, 56, 1, 1, "the size of tests/test_gpu_io.py"),
    Size(130, 127, 2, 1, "egress: a second pass, for 126 pixels of workgroup 0 only"),
    Size(150, 221, 3, 2, "egress: a third pass for some lanes; SSIM H pass: a second pass for 382 pixels"),
]
TS = (1, 3)
SSIM_CONTENTS = ("texture", "flat250_s1", "flat128_s2", "flat2_s1", "sky", "equal")
_FLAT = {"flat250_s1": (250, 1.0), "flat128_s2": (128, 2.0), "flat2_s1": (2, 1.0)}
SSIM_TOL = 2e-5                       # DESIGN.md kernel table, sn_io.hip row: "SSIM within 2e-5" of cli.ssim_calculate
YARDSTICK_TOL = 1e-5                  # half of it: what the float32 yardstick may be away from float64, so that it cannot use up the bound


def ssim_contents(H: int, W: int):
    return ("texture", "equal") if H * W <= 15 else SSIM_CONTENTS


def _rng(content: str, T: int, H: int, W: int, t: int):
    return np.random.default_rng(zlib.crc32(f"{content}/{T}/{H}x{W}/{t}".encode()))


def _frame(content: str, T: int, H: int, W: int, t: int):
    """(gt uint8 [H, W, 3], out float32 [3, H, W]) of frame t."""
    rng = _rng(content, T, H, W, t)
    sigma = 0.0
    if content in ("texture", "equal"):
        gt = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        sigma = 20.0 if content == "texture" else 0.0
    elif content in _FLAT:
        gt = np.full((H, W, 3), _FLAT[content][0], np.uint8)
        sigma = _FLAT[content][1]
    elif content == "sky":
        rows = np.rint(180.0 + 60.0 * np.arange(H) / max(H - 1, 1)).astype(np.uint8)
        gt = np.broadcast_to(rows[:, None, None], (H, W, 3)).copy()
        sigma = 2.0
    else:
        raise KeyError(content)
    out = gt.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    if sigma:
        out = out + (rng.normal(0.0, 1.0, (3, H, W)) * (sigma / 255.0)).astype(np.float32)
    return gt, np.ascontiguousarray(out, np.float32)


@lru_cache(maxsize=None)
def clip(content: str, T: int, H: int, W: int):
    """(gt uint8 [T, H, W, 3], out float32 [T, 3, H, W]), read-only: computed once, shared by every test that asks."""
    frames = [_frame(content, T, H, W, t) for t in range(T)]
    gt, out = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    gt.setflags(write=False)
    out.setflags(write=False)
    return gt, out


def _find_ties():
    """float32 x with float32(x) * float32(255) == k + 0.5 exactly (the product rounded once), one per k where the neighbourhood of (k + 0.5) / 255 has
    one: (x, k) lists."""
    xs, ks = [], []
    for k in range(255):
        want = np.float32(k + 0.5)
        x = np.float32((k + 0.5) / 255.0)
        cands = [x]
        lo = hi = x
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
            cands += [lo, hi]
        for c in cands:
            if np.float32(c) * np.float32(255) == want:
                xs.append(np.float32(c))
                ks.append(k)
                break
    return np.array(xs, np.float32), np.array(ks, np.int64)


TIE_X, TIE_K = _find_ties()
_one, _zero = np.float32(1), np.float32(0)
EDGE_X = np.array([0.5, 0.0, 1.0, -0.0, np.nextafter(_zero, -_one), np.nextafter(_zero, _one), np.nextafter(_one, _zero), np.nextafter(_one, np.float32(2)),
                   -1e-3, 1.001, 1e-30, -1e-30], np.float32)


def _ties():
    """16 ties with k even, 16 with k odd (spread over the range of k), then the edge values."""
    ev, od = TIE_X[TIE_K % 2 == 0], TIE_X[TIE_K % 2 == 1]
    assert len(ev) >= 16 and len(od) >= 16, (len(ev), len(od))
    pick = lambda a: a[np.linspace(0, len(a) - 1, 16).astype(int)]
    return np.concatenate([pick(ev), pick(od), EDGE_X]).astype(np.float32)


TIES = _ties()


@lru_cache(maxsize=None)
def egress_clip(content: str, T: int, H: int, W: int):
    """The clips of the egress tests.  ``texture``: ``clip`` with as many of ``TIES`` as fit at the start of frame 0 (all of them from 6 x 13 upward).
    ``equal``: ``clip`` at T = 1; at T = 3 the equal frame in the middle of two texture frames."""
    if content == "texture":
        gt, out = clip("texture", T, H, W)
        out = out.copy()
        n = min(len(TIES), 3 * H * W)
        out[0].reshape(-1)[:n] = TIES[:n]
    elif content == "equal":
        gt, out = clip("equal", T, H, W)
        if T == 3:
            tg, to = clip("texture", T, H, W)
            gt, out = np.stack([tg[0], gt[1], tg[2]]), np.stack([to[0], out[1], to[2]])
    else:
        raise KeyError(content)
    out.setflags(write=False)
    return gt, out


def egress_ref(x: np.ndarray, gt: np.ndarray):
    """x: float32 [T, 3, H, W], the values the kernel reads (rounded to its dtype, back in float32); gt: uint8 [T, H, W, 3] ->
    (v float32 [T, H, W, 3] = clamp * 255, img uint8 [T, H, W, 3], sse float64 [T])."""
    assert x.dtype == np.float32 and gt.dtype == np.uint8
    v = (np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).transpose(0, 2, 3, 1)
    assert v.dtype == np.float32
    img = np.rint(v).astype(np.uint8)                                  # ties to even
    d = v.astype(np.float64) - gt.astype(np.float64)
    return v, img, np.array([math.fsum((f * f).reshape(-1)) for f in d], np.float64)


def sse_bound(sse_ref: float, H: int, W: int, pass_pixels: int = 16384) -> float:
    return (3 * -(-(H * W) // pass_pixels) + 14) * 2.0 ** -24 * sse_ref


def ssim_f64(img1: np.ndarray, img2: np.ndarray, sd: float = 1.5, c1: float = 0.01 ** 2, c2: float = 0.03 ** 2) -> float:
    """``cli.ssim_calculate`` with float64 volumes: the same formula, the same scipy filter, nothing rounded to float32."""
    from scipy.ndimage import gaussian_filter
    a = np.array(img1, dtype=np.float64).transpose(2, 0, 1) / 255
    b = np.array(img2, dtype=np.float64).transpose(2, 0, 1) / 255
    mu1, mu2 = gaussian_filter(a, sd), gaussian_filter(b, sd)
    s1 = gaussian_filter(a * a, sd) - mu1 * mu1
    s2 = gaussian_filter(b * b, sd) - mu2 * mu2
    s12 = gaussian_filter(a * b, sd) - mu1 * mu2
    return float(np.mean(((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))))


def host_image(x: np.ndarray) -> np.ndarray:
    """x: float32 [3, H, W] -> float32 [H, W, 3], what the CLI hands its metrics: clamp(0, 1) * 255 (inference/test_deblur.py:140-141)."""
    return np.clip(x, np.float32(0), np.float32(1)).transpose(1, 2, 0) * np.float32(255)
