"""Full-reference quality of the video restorer's report: PSNR and SSIM of the input and of the written frames against a ground-truth stream
(``VideoRestorer.restore(..., gt=...)``, ``--gt``).  Host arithmetic only: float64, numpy and math, no torch.

The experiment is the standard one: a clean clip, a degraded copy of it, and a restoration of the copy compared with the clip.  Every written frame
is compared, in the format written; nothing is dropped or cropped, unlike the evaluation harnesses under ``inference/test_*.py``.

PSNR needs no kernel of its own: ``sn_yuv_diff_stats(truth, frames)`` (csrc/sn_yuv_stats.hip) has the exact integer sums of squared differences of all
three planes, and ``psnr_from_sums`` makes ``10 log10(p^2 / (sum d^2 / N))`` of them with p = 2^bits - 1, ``inf`` where the sum is 0 -- upstream's
``calculate_psnr`` on the codes, per plane.

SSIM is upstream's Y-channel SSIM (``_ssim_cly`` of basicsr/metrics/psnr_ssim.py) on the luma codes as stored: an 11 x 11 Gaussian window of sigma 1.5,
the border replicated, all h x w positions counted, C1 = (0.01 p)^2 and C2 = (0.03 p)^2.  At 8 bit that is upstream's formula on its 0 .. 255 scale;
at 10 bit it is the same formula on codes * 255 / 1023, because SSIM does not change when the constants scale with the data.
``sn_yuv_ssim_sums`` (csrc/sn_ssim.hip, include/shiftnet_hip.h) sums the map per 32 x 32 tile on the device, ``ssim_from_tiles`` adds the tiles.

**Luma SSIM only** -- no chroma SSIM, no MS-SSIM, no VMAF, no LPIPS.  **The truth must be in the format written and frame-aligned by the caller**: no
offset is searched.  No threshold and no verdict, and nothing is fed back into ``amount`` or ``sigma``."""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Dict, Iterable, Tuple

import numpy as np

FIELDS = ("psnr_y_in", "psnr_y_out", "psnr_u_in", "psnr_u_out", "psnr_v_in", "psnr_v_out", "ssim_in", "ssim_out")
# per written frame; _in: the input (in the format written) against the truth, _out: the frame written against the truth
FullRef = namedtuple("FullRef", FIELDS)
TAPS = 11
SIGMA = 1.5


def ssim_taps() -> np.ndarray:
    """The 11 float64 taps of the window's separable factor, ``exp(-(i - 5)^2 / (2 * 1.5^2))`` normalised to sum 1 (the device rounds them to float32)."""
    g = np.exp(-((np.arange(TAPS, dtype=np.float64) - TAPS // 2) ** 2) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def ssim_constants(bits: int) -> Tuple[float, float]:
    """(C1, C2) for codes of ``bits`` bits."""
    p = float((1 << int(bits)) - 1)
    return (0.01 * p) ** 2, (0.03 * p) ** 2


def _psnr(sq: int, n: int, bits: int) -> float:
    if n <= 0:
        return float("nan")
    if sq == 0:
        return float("inf")
    p = float((1 << int(bits)) - 1)
    return 10.0 * math.log10(p * p / (sq / n))


def psnr_from_sums(sums16, bits: int) -> Tuple[float, float, float]:
    """One row of ``sn_yuv_diff_stats`` (words 0 and 2: N and the sum of d^2 of the luma; 10: the samples of a chroma plane; 12, 14: the sums of du^2
    and dv^2) -> (psnr_y, psnr_u, psnr_v) in dB: ``10 log10(p^2 / (sum d^2 / N))``, p = 2^bits - 1; ``inf`` where the sum is 0."""
    s = [int(v) for v in np.asarray(sums16).reshape(-1)]
    if len(s) != 16:
        raise ValueError(f"a row of sn_yuv_diff_stats has 16 words, got {len(s)}")
    return _psnr(s[2], s[0], bits), _psnr(s[12], s[10], bits), _psnr(s[14], s[10], bits)


def ssim_from_tiles(tiles, h: int, w: int) -> float:
    """A payload's tile sums of ``sn_yuv_ssim_sums`` (any shape; the picture is h x w) -> its SSIM: their exactly rounded sum over h w."""
    return math.fsum(float(v) for v in np.asarray(tiles, np.float64).reshape(-1)) / (int(h) * int(w))


def frame_fullref(sums_in, sums_out, tiles_in, tiles_out, bits: int, h: int, w: int) -> FullRef:
    """The rows of ``sn_yuv_diff_stats(truth, input)`` and ``(truth, written)`` and the tiles of ``sn_yuv_ssim_sums`` of the same pairs -> a FullRef."""
    pi, po = psnr_from_sums(sums_in, bits), psnr_from_sums(sums_out, bits)
    return FullRef(pi[0], po[0], pi[1], po[1], pi[2], po[2], ssim_from_tiles(tiles_in, h, w), ssim_from_tiles(tiles_out, h, w))


def summarize_fullref(frames: Iterable[FullRef]) -> Dict[str, Dict]:
    """{"mean": per field the mean over the frames with a finite value (what papers quote), "median": per field the median over the frames that are not
    nan (``inf`` counts: the report's last line), "inf": per field the frames left out of the mean because they are ``inf``}; nan where nothing counts."""
    frames = list(frames)
    out = {"mean": {}, "median": {}, "inf": {}}
    for i, name in enumerate(FIELDS):
        v = [float(f[i]) for f in frames if not math.isnan(f[i])]
        fin = [x for x in v if not math.isinf(x)]
        out["mean"][name] = math.fsum(fin) / len(fin) if fin else float("nan")
        out["median"][name] = float(np.median(v)) if v else float("nan")
        out["inf"][name] = len(v) - len(fin)
    return out


def summary_line_fullref(summary: Dict[str, Dict]) -> str:
    """Mean and median PSNR-Y and SSIM of input and output, for a log."""
    mean, med, inf = summary["mean"], summary["median"], summary["inf"]
    words = []
    for k, form in (("psnr_y_in", "%.2f"), ("psnr_y_out", "%.2f"), ("ssim_in", "%.4f"), ("ssim_out", "%.4f")):
        words.append(f"{k} mean {form % mean[k]} median {form % med[k]}" + (f" ({inf[k]} inf left out of the mean)" if inf[k] else ""))
    return ", ".join(words)
