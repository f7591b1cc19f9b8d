"""Device-side I/O edges of the CLIs (csrc/sn_io.hip): uint8 frames in, uint8 frames and PSNR out.

``ingest_u8``  == ``numpy2tensor(frames).to(device).to(dtype)`` of inference/test_deblur.py:191-200,128,134, bit for bit,
               with 3 instead of 12 bytes per pixel crossing PCIe;
``ingest_yuv`` / ``egress_yuv``: planar Y'CbCr payloads as a Y4M stream carries them (csrc/sn_yuv.hip) <-> RGB tensors, for the video
               restorer (shiftnet_amd/restore.py); 1.5 bytes per pixel cross PCIe for 8-bit 4:2:0.  ``egress_yuv`` takes ``dither=(seed, t0)`` to add
               triangular noise of +-1 code before the rounding, and ``mix=`` with ``ref=`` to blend the result with the payloads that came in, or to
               show their difference;
the statistics of the same payloads' luma (csrc/sn_yuv_stats.hip), each for one decision the restorer makes on the host:
``thumb_yuv``  : uint16 sums of the luma codes of every 8 x 8 block, for the scene-cut detector (shiftnet_amd/scenes.py);
``noise_hist_yuv``: uint32 histograms of |a - b - c + d| over the 2 x 2 luma blocks, for the blind noise estimate (shiftnet_amd/noise.py);
``noise_hist_bands_yuv``: that statistic split into 16 bands of brightness, from which noise.py estimates a noise-level function (sigma against the
               luma code);
``noise_hist_pairs_yuv`` / ``noise_hist_pairs_bands_yuv``: the same two statistics of the difference of consecutive payloads, T - 1 pairs, for the
               temporal noise estimate (shiftnet_amd/noise.py);
``block_motion_yuv``: one integer translation within +-7 samples per 16 x 16 luma block of every pair of consecutive payloads, and
``noise_hist_pairs_mv_yuv`` / ``noise_hist_pairs_bands_mv_yuv``: the two pair statistics with the second payload's block taken where the vector
               points, for the motion-compensated temporal estimate (shiftnet_amd/noise.py);
``noise_map_level``: payloads + the 16 knots of such a function -> the denoisers' noise plane;
``degrade_yuv``: clean payloads + the 16 knots of a noise curve -> the payloads with Gaussian noise added to R'G'B' (csrc/sn_degrade.hip), for the
               restorer's ``add_noise`` stage: the degraded copy that the comparison with a ground truth needs;
``blur_yuv``: sharp payloads -> the means of n consecutive ones on R'G'B', in linear light where gamma tables are given (csrc/sn_blur.hip), for the
               restorer's ``add_blur`` stage: the same for the deblurrers;
``grain_yuv``: payloads + the 16 knots of a level curve -> the payloads with spatially correlated Gaussian grain added in the code domain, in place if
               asked (csrc/sn_grain.hip), for the restorer's ``grain`` stage behind the egress;
``code_hist_yuv``: payloads -> the exact histogram of every payload's luma codes, and ``apply_lut_yuv``: payloads + one table for the luma and one for
               the chroma planes per payload -> the payloads looked up, in place if asked (csrc/sn_deflicker.hip), for the restorer's ``deflicker``
               stage (the rule between the two is shiftnet_amd/deflicker.py's);
``despot_vectors``: payloads -> the block vectors of every frame into its previous and into its next frame, and ``despot_yuv``: payloads + those
               vectors -> the payloads with dirt taken out and two counts per frame (csrc/sn_despot.hip), for the restorer's ``despot`` stage;
``rowcol_sums_yuv``: uint32 sums of the luma codes of every row and of every column, for the letterbox rule (shiftnet_amd/picture.py);
``diff_stats_yuv``: int64 sums of the difference of two sets of payloads, what came in and what was written, for the method-noise report
               (shiftnet_amd/report.py);
``diff_stats_mv_yuv``: int64 sums of that difference in consecutive payloads along the vectors of ``block_motion_yuv``, for the report's motion-compensated
               temporal correlation;
``niqe_sums_yuv``: float64 sums of the locally normalised luma and of its neighbour products per 96 x 96 block at two scales (csrc/sn_niqe.hip), for the
               no-reference quality score of the report (shiftnet_amd/niqe.py);
``ssim_sums_yuv``: float64 sums of the SSIM map of the luma of two sets of payloads per 32 x 32 tile (csrc/sn_ssim.hip), for the report's comparison with a
               ground-truth stream (shiftnet_amd/fullref.py);
``tile_accumulate``: one tile's float32 result added into the window's float32 canvas with its feather weights (csrc/sn_tile.hip), for the tiled
               restorer (``VideoRestorer(tile=...)``);
``geo_transform`` / ``geo_accumulate``: a tensor mirrored, transposed and reversed in time, and a float32 result mapped back and added into a float32
               canvas (csrc/sn_geo.hip), for the self-ensemble (shiftnet_amd/ensemble.py);
``time_crossfade``: the frames two overlapping windows share, cross-faded in place, and the exact sum of squares of the two answers' difference
               (csrc/sn_time.hip), for ``VideoRestorer(window_overlap=...)``;
``rect=(x0, y0, w, h)``, where a function takes it (all but ``thumb_yuv`` and ``rowcol_sums_yuv``), restricts it to that picture of the stream, with
               the result of the cropped stream;
``egress_u8``  == the per-frame ``clamp(0,1) * 255`` -> skimage PSNR(data_range=255) against the uint8 ground truth
               (:139-143) and the rounded uint8 frame cv2.imwrite would store (:152).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Tuple

import torch

from . import lib as L

_CODE = {torch.float32: L.SN_F32, torch.float16: L.SN_F16, torch.bfloat16: L.SN_BF16}


def ingest_u8(frames_u8: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """frames_u8: [T,H,W,3] uint8 on a HIP device -> [1,T,3,H,W] of ``dtype`` in [0,1]."""
    assert frames_u8.dtype == torch.uint8 and frames_u8.is_cuda and frames_u8.dim() == 4 and frames_u8.shape[3] == 3
    frames_u8 = frames_u8.contiguous()
    T, H, W, _ = frames_u8.shape
    x = torch.empty((1, T, 3, H, W), dtype=dtype, device=frames_u8.device)
    with torch.cuda.device(frames_u8.device):
        L.check(L.load().sn_ingest_u8(frames_u8.data_ptr(), x.data_ptr(), _CODE[dtype], T, H, W,
                                      torch.cuda.current_stream(frames_u8.device).cuda_stream), "sn_ingest_u8")
    return x


def egress_u8(out: torch.Tensor, gt_u8: Optional[torch.Tensor] = None, want_image: bool = True
              ) -> Tuple[Optional[torch.Tensor], Optional[List[float]]]:
    """out: [T,3,H,W] network output (module dtype) on the device; gt_u8: [T,H,W,3] uint8 on the device or None.

    Returns (uint8 frames [T,H,W,3] on the device or None, per-frame PSNR in dB or None)."""
    assert out.is_cuda and out.dim() == 4 and out.shape[1] == 3 and out.dtype in _CODE
    out = out.contiguous()
    T, _, H, W = out.shape
    lib = L.load()
    img = torch.empty((T, H, W, 3), dtype=torch.uint8, device=out.device) if want_image else None
    sse = None
    if gt_u8 is not None:
        assert gt_u8.dtype == torch.uint8 and tuple(gt_u8.shape) == (T, H, W, 3) and gt_u8.device == out.device
        gt_u8 = gt_u8.contiguous()
        sse = torch.empty((T, lib.sn_egress_blocks()), dtype=torch.float32, device=out.device)
    with torch.cuda.device(out.device):
        L.check(lib.sn_egress_u8(out.data_ptr(), _CODE[out.dtype], gt_u8.data_ptr() if gt_u8 is not None else None,
                                 img.data_ptr() if img is not None else None, sse.data_ptr() if sse is not None else None,
                                 T, H, W, torch.cuda.current_stream(out.device).cuda_stream), "sn_egress_u8")
    psnr = None
    if sse is not None:
        tot = sse.double().cpu().sum(1)             # T x 64 partial sums: summed in float64 on the host
        psnr = [float("inf") if s == 0 else 10.0 * math.log10(255.0 ** 2 / (s / (3 * H * W))) for s in tot.tolist()]
    return img, psnr


def ssim_u8(out: torch.Tensor, gt_u8: torch.Tensor) -> List[float]:
    """The CLIs' SSIM (test_deblur.py:25-49) per frame, on the device.  out: [T,3,H,W] module dtype, gt_u8: [T,H,W,3] uint8."""
    assert out.is_cuda and out.dim() == 4 and out.shape[1] == 3 and out.dtype in _CODE
    out = out.contiguous()
    T, _, H, W = out.shape
    assert gt_u8.dtype == torch.uint8 and tuple(gt_u8.shape) == (T, H, W, 3) and gt_u8.device == out.device
    gt_u8 = gt_u8.contiguous()
    lib = L.load()
    scratch = torch.empty((T, 15, H, W), dtype=torch.float32, device=out.device)
    part = torch.empty((T, lib.sn_ssim_blocks()), dtype=torch.float32, device=out.device)
    with torch.cuda.device(out.device):
        L.check(lib.sn_ssim_u8(out.data_ptr(), _CODE[out.dtype], gt_u8.data_ptr(), scratch.data_ptr(), part.data_ptr(), T, H, W,
                               torch.cuda.current_stream(out.device).cuda_stream), "sn_ssim_u8")
    return (part.double().cpu().sum(1) / (3.0 * H * W)).tolist()


def yuv_fmt(bits: int, chroma: int, matrix: int, range_: int) -> "L.YuvFmt":
    """sn_yuv_fmt from the integer codes of lib.py (SN_YUV_*)."""
    return L.YuvFmt(bits, chroma, matrix, range_)


def _rect(rect, fmt: "L.YuvFmt", H: int, W: int) -> "L.YuvRect":
    from .picture import check_rect
    return L.YuvRect(*check_rect(rect, fmt, H, W, smallest=1))      # the kernels take any rectangle; the restorer has a limit of its own


def _payload(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int) -> Tuple[int, torch.device]:
    """The check every function below makes of its payloads, [T, frame_bytes] uint8 on a HIP device -> (T, the device)."""
    fb = fmt.frame_bytes(H, W)
    assert payload_u8.dtype == torch.uint8 and payload_u8.is_cuda and payload_u8.dim() == 2 and payload_u8.shape[1] == fb and payload_u8.is_contiguous()
    return payload_u8.shape[0], payload_u8.device


def _clip(fmt: "L.YuvFmt", lo: Optional[int], hi: Optional[int]) -> Tuple[int, int]:
    """``lo``, ``hi`` of the noise statistics; None is the format's black / white code (noise.clip_codes)."""
    from .noise import clip_codes
    dlo, dhi = clip_codes(fmt.bits, fmt.range)
    return dlo if lo is None else int(lo), dhi if hi is None else int(hi)


def ingest_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, Hp: int, Wp: int, dtype: torch.dtype,
               out: Optional[torch.Tensor] = None, rect=None) -> torch.Tensor:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device, T planar Y'CbCr frames of H x W -> [1,T,3,Hp,Wp] RGB of ``dtype`` in [0,1];
    pixels outside H x W replicate the edge pixel.  ``out``: a [1,T,3,Hp,Wp] tensor to fill instead of a new one.
    ``rect=(x0, y0, w, h)``: the picture of the stream to ingest, bit for bit as the cropped stream would be: Hp >= h, Wp >= w, the chroma
    neighbours clamp to the picture's chroma planes and the padding repeats its last row and column."""
    T, _ = _payload(payload_u8, fmt, H, W)
    r = None if rect is None else _rect(rect, fmt, H, W)
    assert Hp >= (H if r is None else r.h) and Wp >= (W if r is None else r.w) and dtype in _CODE
    x = out if out is not None else torch.empty((1, T, 3, Hp, Wp), dtype=dtype, device=payload_u8.device)
    assert tuple(x.shape) == (1, T, 3, Hp, Wp) and x.dtype == dtype and x.is_contiguous() and x.device == payload_u8.device
    with torch.cuda.device(payload_u8.device):
        st = torch.cuda.current_stream(payload_u8.device).cuda_stream
        if r is None:
            L.check(L.load().sn_ingest_yuv(payload_u8.data_ptr(), fmt, x.data_ptr(), _CODE[dtype], T, H, W, Hp, Wp, st), "sn_ingest_yuv")
        else:
            L.check(L.load().sn_ingest_yuv_rect(payload_u8.data_ptr(), fmt, r, x.data_ptr(), _CODE[dtype], T, H, W, Hp, Wp, st), "sn_ingest_yuv_rect")
    return x


MIXES = {"amount": L.SN_MIX_AMOUNT, "removed": L.SN_MIX_REMOVED}


def _mix(mix) -> "L.YuvMix":
    """("amount", ay, ac) or ("removed", gy, gc) -> sn_yuv_mix; ValueError for anything sn_egress_yuv_mix would refuse."""
    try:
        word, y, c = mix
        y, c = float(y), float(c)
    except (TypeError, ValueError):
        raise ValueError(f"mix must be ('amount', ay, ac) or ('removed', gy, gc), got {mix!r}") from None
    if not isinstance(word, str) or word not in MIXES or not (math.isfinite(y) and math.isfinite(c)):
        raise ValueError(f"mix must be ('amount', ay, ac) or ('removed', gy, gc) with finite numbers, got {mix!r}")
    if word == "amount" and not (0.0 <= y <= 1.0 and 0.0 <= c <= 1.0):
        raise ValueError(f"mix=('amount', ay, ac): the amounts lie in [0, 1], got {mix!r}")
    return L.YuvMix(MIXES[word], y, c)


def egress_yuv(out: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, dst: Optional[torch.Tensor] = None, rect=None, dither=None, mix=None,
               ref: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out: [T,3,Hp,Wp] network output (float32 or module dtype) on the device -> [T, frame_bytes] uint8 payloads of the H x W crop.
    ``dst``: a [T, frame_bytes] uint8 tensor to fill instead of a new one.
    ``rect=(x0, y0, w, h)``: out holds that picture of the H x W stream (Hp >= h, Wp >= w); only the picture's samples of the payloads, luma and
    chroma, are written, with what the cropped stream's egress writes -- every other byte of ``dst`` stays (a new tensor starts as zeros).
    ``dither=(seed, t0)``: triangular noise of +-1 code is added before the rounding (include/shiftnet_hip.h: sn_egress_yuv_dither), a hash of
    the seed (0 .. 2^32 - 1), the frame number t0 + t and the sample's plane, row and column; None is today's call and today's bytes.
    ``mix=("amount", ay, ac)`` with ``ref``, the [T, frame_bytes] payloads that came in (same format and size as the result, another tensor than
    ``dst``): every code is the input's code moved by that share of the way to the result's, separately for luma and chroma, linear in the code
    domain; amount 0 is ``ref`` byte for byte.  ``mix=("removed", gy, gc)``: input minus result around mid-grey, times the gain
    (include/shiftnet_hip.h: sn_egress_yuv_mix).  ``mix=None`` calls exactly what it called before."""
    assert out.is_cuda and out.dim() == 4 and out.shape[1] == 3 and out.dtype in _CODE and out.is_contiguous()
    T, _, Hp, Wp = out.shape
    r = None if rect is None else _rect(rect, fmt, H, W)
    assert Hp >= (H if r is None else r.h) and Wp >= (W if r is None else r.w)
    fb = fmt.frame_bytes(H, W)
    y = dst if dst is not None else (torch.empty if r is None else torch.zeros)((T, fb), dtype=torch.uint8, device=out.device)
    assert tuple(y.shape) == (T, fb) and y.dtype == torch.uint8 and y.is_contiguous() and y.device == out.device
    d = None
    if dither is not None:
        seed, t0 = (int(v) for v in dither)
        if not (0 <= seed < 2 ** 32) or not (0 <= t0 <= 2 ** 31 - 1 - T):
            raise ValueError(f"dither=(seed, t0): need 0 <= seed < 2^32 and 0 <= t0 <= 2^31 - 1 - T, got {dither!r}")
        d = L.YuvDither(L.SN_DITHER_TPDF, seed, t0)
    if (mix is None) != (ref is None):
        raise ValueError("mix and ref go together: the mix reads the payloads that came in")
    m = None if mix is None else _mix(mix)
    if m is not None:
        assert tuple(ref.shape) == (T, fb) and ref.dtype == torch.uint8 and ref.is_contiguous() and ref.device == out.device
    with torch.cuda.device(out.device):
        st = torch.cuda.current_stream(out.device).cuda_stream
        if m is not None:
            L.check(L.load().sn_egress_yuv_mix(out.data_ptr(), _CODE[out.dtype], fmt, r, d, m, ref.data_ptr(), y.data_ptr(), T, H, W, Hp, Wp, st),
                    "sn_egress_yuv_mix")
        elif d is not None:
            L.check(L.load().sn_egress_yuv_dither(out.data_ptr(), _CODE[out.dtype], fmt, r, d, y.data_ptr(), T, H, W, Hp, Wp, st), "sn_egress_yuv_dither")
        elif r is None:
            L.check(L.load().sn_egress_yuv(out.data_ptr(), _CODE[out.dtype], fmt, y.data_ptr(), T, H, W, Hp, Wp, st), "sn_egress_yuv")
        else:
            L.check(L.load().sn_egress_yuv_rect(out.data_ptr(), _CODE[out.dtype], fmt, r, y.data_ptr(), T, H, W, Hp, Wp, st), "sn_egress_yuv_rect")
    return y


def degrade_yuv(src: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, knots, seed: int, t0: int, gauss: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src: [T, frame_bytes] uint8 on a HIP device, T clean payloads of H x W, frames t0 .. t0 + T - 1 of their stream -> [T, frame_bytes] uint8, the
    same frames with Gaussian noise added to R'G'B' between the two colour edges (include/shiftnet_hip.h: sn_yuv_degrade): ``egress(ingest_float32(src) +
    s * g)``, in one launch and with no float frame in memory.  ``knots``: the 16 sigmas of the noise curve in 8-bit R'G'B' code units, finite and >= 0,
    knot b at luma code lo + (b + 0.5) (hi - lo) / 16 of the format's black and white codes (noise.knot_codes); s is the curve at the pixel's clean luma
    code.  ``seed`` (0 .. 2^32 - 1) picks the noise, a hash of the seed, the frame's number in the stream, the channel, the row and the column.
    ``gauss``: float32 [65536] on the same device, degrade.gauss_table().  ``out``: a [T, frame_bytes] uint8 tensor to fill, another than ``src``."""
    T, dev = _payload(src, fmt, H, W)
    kn = [float(k) for k in knots]
    if len(kn) != L.SN_NLF_BANDS or not all(math.isfinite(k) and k >= 0.0 for k in kn):
        raise ValueError(f"knots: need {L.SN_NLF_BANDS} finite numbers >= 0, got {knots!r}")
    seed, t0 = int(seed), int(t0)
    if not (0 <= seed < 2 ** 32) or not (0 <= t0 <= 2 ** 31 - 1 - T):
        raise ValueError(f"need 0 <= seed < 2^32 and 0 <= t0 <= 2^31 - 1 - T, got seed {seed!r}, t0 {t0!r}")
    assert gauss.dtype == torch.float32 and tuple(gauss.shape) == (1 << 16,) and gauss.is_contiguous() and gauss.device == dev
    y = out if out is not None else torch.empty_like(src)
    assert _payload(y, fmt, H, W) == (T, dev)
    noise = L.YuvDegradeNoise(seed, t0, (C.c_float * L.SN_NLF_BANDS)(*kn))
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_degrade(src.data_ptr(), fmt, noise, gauss.data_ptr(), y.data_ptr(), T, H, W,
                                        torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_degrade")
    return y


def grain_yuv(src: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, knots, taps, chroma: float, seed: int, t0: int, gauss: torch.Tensor, rect=None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src: [T, frame_bytes] uint8 on a HIP device, T payloads of H x W, frames t0 .. t0 + T - 1 of their clip -> [T, frame_bytes] uint8, the same
    frames with spatially correlated Gaussian grain added in the code domain (include/shiftnet_hip.h: sn_yuv_grain), in one launch.  ``knots``: the 16
    levels of the grain in 8-bit R'G'B' code units, finite and >= 0 (the sigma of i.i.d. noise on R'G'B' whose luma part the grain equals; converted
    to luma codes here, grain.luma_knots), knot b at luma code lo + (b + 0.5) (hi - lo) / 16 (noise.knot_codes); the level of a sample is the curve at
    the luma code read.  ``taps``: (w0, w1, w2) of the separable filter, grain.grain_taps(size).  ``chroma``: the share of the level the chroma planes
    get, >= 0; 0 leaves them as they came.  ``seed`` (0 .. 2^32 - 1) picks the grain, a hash of the seed, the frame's number, the plane, the row and the
    column counted from the picture's origin.  ``gauss``: float32 [65536] on the same device, degrade.gauss_table().  ``rect=(x0, y0, w, h)``: only that
    picture is read and written.  ``out``: a [T, frame_bytes] uint8 tensor to fill -- ``src`` itself for in place, or one that does not overlap it; None
    is a new tensor (a copy of ``src`` outside a rectangle)."""
    from .grain import luma_knots
    T, dev = _payload(src, fmt, H, W)
    try:
        kn = luma_knots(knots, fmt)
    except (TypeError, ValueError):
        raise ValueError(f"knots: need {L.SN_NLF_BANDS} finite numbers >= 0, got {knots!r}") from None
    tp = [float(w) for w in taps]
    if len(tp) != 3 or not all(math.isfinite(w) and w >= 0.0 for w in tp) or not tp[0] > 0.0 or abs(tp[0] ** 2 + 2 * tp[1] ** 2 + 2 * tp[2] ** 2 - 1.0) > 1e-3:
        raise ValueError(f"taps: need (w0, w1, w2), finite and >= 0, w0 > 0, of unit energy w0^2 + 2 w1^2 + 2 w2^2, got {taps!r}")
    chroma = float(chroma)
    if not (math.isfinite(chroma) and chroma >= 0.0):
        raise ValueError(f"chroma: need a finite share >= 0, got {chroma!r}")
    seed, t0 = int(seed), int(t0)
    if not (0 <= seed < 2 ** 32) or not (0 <= t0 <= 2 ** 31 - 1 - T):
        raise ValueError(f"need 0 <= seed < 2^32 and 0 <= t0 <= 2^31 - 1 - T, got seed {seed!r}, t0 {t0!r}")
    assert gauss.dtype == torch.float32 and tuple(gauss.shape) == (1 << 16,) and gauss.is_contiguous() and gauss.device == dev
    r = None if rect is None else _rect(rect, fmt, H, W)
    y = out if out is not None else (torch.empty_like(src) if r is None else src.clone())
    assert _payload(y, fmt, H, W) == (T, dev)
    grain = L.YuvGrainNoise(seed, t0, (C.c_float * L.SN_NLF_BANDS)(*kn), chroma, (C.c_float * 3)(*tp))
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_grain(src.data_ptr(), fmt, r, grain, gauss.data_ptr(), y.data_ptr(), T, H, W,
                                      torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_grain")
    return y


def code_hist_yuv(src: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, rect=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src: [T, frame_bytes] uint8 on a HIP device, T payloads of H x W -> [T, 2^bits] int32 (the bits of uint32 counts): how many luma samples of
    every payload have each code, a stored 16-bit word above 2^bits - 1 counted in the last bin (include/shiftnet_hip.h: sn_yuv_code_hist), in one
    launch.  Exact; every row sums to the sample count.  ``rect=(x0, y0, w, h)``: only that picture is counted.  ``out``: a [T, 2^bits] int32 tensor to
    fill -- the call zeroes it itself -- instead of a new one."""
    T, dev = _payload(src, fmt, H, W)
    r = None if rect is None else _rect(rect, fmt, H, W)
    codes = 1 << fmt.bits
    y = out if out is not None else torch.empty((T, codes), dtype=torch.int32, device=dev)
    assert tuple(y.shape) == (T, codes) and y.dtype == torch.int32 and y.is_contiguous() and y.device == dev
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_code_hist(src.data_ptr(), fmt, r, y.data_ptr(), T, H, W, torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_code_hist")
    return y


def apply_lut_yuv(src: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, lut: torch.Tensor, rect=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src: [T, frame_bytes] uint8 on a HIP device, T payloads of H x W; lut: [T, 2, 2^bits] int16 (the bits of uint16 codes) on the same device, per
    payload the table of the luma plane and the table of both chroma planes -> [T, frame_bytes] uint8, every code replaced by its table's entry
    (include/shiftnet_hip.h: sn_yuv_apply_lut), in one launch.  ``rect=(x0, y0, w, h)``: only that picture is read and written.  ``out``: a
    [T, frame_bytes] uint8 tensor to fill -- ``src`` itself for in place, or one that does not overlap it; None is a new tensor (a copy of ``src``
    outside a rectangle)."""
    T, dev = _payload(src, fmt, H, W)
    assert lut.dtype == torch.int16 and tuple(lut.shape) == (T, 2, 1 << fmt.bits) and lut.is_contiguous() and lut.device == dev
    r = None if rect is None else _rect(rect, fmt, H, W)
    y = out if out is not None else (torch.empty_like(src) if r is None else src.clone())
    assert _payload(y, fmt, H, W) == (T, dev)
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_apply_lut(src.data_ptr(), fmt, r, lut.data_ptr(), y.data_ptr(), T, H, W, torch.cuda.current_stream(dev).cuda_stream),
                "sn_yuv_apply_lut")
    return y


def despot_vectors(src: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """src: [S, frame_bytes] uint8 on a HIP device, S >= 2 payloads of H x W -> (mv_prev, mv_next), int8 [S - 1, nby, nbx, 2] each, what
    ``despot_yuv`` takes: mv_next[f] is the vector of every 16 x 16 luma block of frame f into frame f + 1 (``block_motion_yuv`` on the stack), and
    mv_prev[f - 1] that of frame f into frame f - 1 (``block_motion_yuv`` on the time-reversed stack, flipped back along its first axis).  Two
    launches; none for a picture without a vector block."""
    mv_next, _ = block_motion_yuv(src, fmt, H, W)
    mv_rev, _ = block_motion_yuv(src.flip(0), fmt, H, W)
    return mv_rev.flip(0).contiguous(), mv_next


def despot_yuv(src: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, mv_prev: torch.Tensor, mv_next: torch.Tensor, f0: int, n: int, threshold: int,
               support: int, grow: int, chroma: str, out: Optional[torch.Tensor] = None,
               out_counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """src: [S, frame_bytes] uint8 on a HIP device, S payloads of H x W; mv_prev, mv_next: int8 [S - 1, nby, nbx, 2] on the same device, as
    ``despot_vectors`` makes them (ANY int8 contents are memory-safe) -> ([n, frame_bytes] uint8: frames f0 .. f0 + n - 1 with dirt taken out, each
    repaired from the ORIGINAL frames f - 1, f, f + 1 of ``src``; [n, 2] int32, the bits of uint32 counts: the core seeds and the luma samples
    replaced of each), in one launch (include/shiftnet_hip.h: sn_yuv_despot states the rule).  1 <= f0 and f0 + n <= S - 1.  ``threshold``: T in
    8-BIT codes, multiplied here by 2^(bits - 8); ``support``: K in 0 .. 8; ``grow``: G in 0 .. 2; ``chroma``: "follow" or "off".  ``out``: a
    [n, frame_bytes] uint8 tensor to fill that does not overlap ``src``; ``out_counts``: a [n, 2] int32 tensor to overwrite."""
    from .noise import motion_grid
    S, dev = _payload(src, fmt, H, W)
    nby, nbx = motion_grid(H, W)
    for mv in (mv_prev, mv_next):
        assert mv.dtype == torch.int8 and tuple(mv.shape) == (S - 1, nby, nbx, 2) and mv.is_contiguous() and mv.device == dev
    if chroma not in ("follow", "off"):
        raise ValueError(f"sn_yuv_despot: chroma is 'follow' or 'off', got {chroma!r}")
    y = out if out is not None else torch.empty((n, src.shape[1]), dtype=torch.uint8, device=dev)
    assert _payload(y, fmt, H, W) == (n, dev)
    c = out_counts if out_counts is not None else torch.empty((n, 2), dtype=torch.int32, device=dev)
    assert tuple(c.shape) == (n, 2) and c.dtype == torch.int32 and c.is_contiguous() and c.device == dev
    # an empty grid has no storage to point at: the entry point reads no vector then, and wants no null pointer
    mp, mn = (mv.data_ptr() if mv.numel() else src.data_ptr() for mv in (mv_prev, mv_next))
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_despot(src.data_ptr(), fmt, mp, mn, y.data_ptr(), c.data_ptr(), S, int(f0), int(n), int(threshold) << (fmt.bits - 8),
                                       int(support), int(grow), 1 if chroma == "follow" else 0, H, W, torch.cuda.current_stream(dev).cuda_stream),
                "sn_yuv_despot")
    return y, c


def blur_yuv(src: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, n: int, c0: int, lo: int, hi: int, tables, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src: [S, frame_bytes] uint8 on a HIP device, S sharp payloads of H x W; out: [T, frame_bytes] uint8 to fill, another than ``src`` (None: T =
    hi - c0 + 1 fresh payloads) -> output t is the mean of the ``n`` (odd, 1 .. 15) source payloads clamp(c0 + t + j, lo, hi), j = -(n // 2) .. n // 2,
    taken on R'G'B' between the two colour edges (include/shiftnet_hip.h: sn_yuv_blur), in one launch and with no float frame in memory.  [lo, hi], with
    0 <= lo <= hi < S, is the scene the outputs c0 .. c0 + T - 1 lie in: its ends are replicated.  ``tables``: None -- the mean of the R'G'B' values as
    they are (gamma 1); (lin, rinv) -- float32 [4096] and [4095] on the same device, degrade.gamma_tables(g): the mean in linear light."""
    S, dev = _payload(src, fmt, H, W)
    n, c0, lo, hi = int(n), int(c0), int(lo), int(hi)
    if not (1 <= n <= L.SN_BLUR_MAX_TAPS and n % 2 == 1):
        raise ValueError(f"n: need an odd number of taps, 1 .. {L.SN_BLUR_MAX_TAPS}, got {n!r}")
    y = out if out is not None else torch.empty((max(hi - c0 + 1, 1), src.shape[1]), dtype=torch.uint8, device=dev)
    T, ydev = _payload(y, fmt, H, W)
    assert ydev == dev
    if not (0 <= lo <= hi < S) or not (lo <= c0 and c0 + T - 1 <= hi):
        raise ValueError(f"need 0 <= lo <= hi < S and lo <= c0, c0 + T - 1 <= hi, got lo {lo}, hi {hi}, c0 {c0} with S {S}, T {T}")
    lin = rinv = None
    if tables is not None:
        lin, rinv = tables
        for t, k in ((lin, 4096), (rinv, 4095)):
            assert t.dtype == torch.float32 and tuple(t.shape) == (k,) and t.is_contiguous() and t.device == dev
    win = L.YuvBlurWindow(n, c0, lo, hi)
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_blur(src.data_ptr(), S, fmt, win, None if lin is None else lin.data_ptr(), None if rinv is None else rinv.data_ptr(),
                                     y.data_ptr(), T, H, W, torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_blur")
    return y


def thumb_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device (only the luma plane of each payload is read) -> uint16 [T, ceil(H/8), ceil(W/8)]:
    the integer sum of the luma codes of every 8 x 8 block, partial at the right and bottom edge.  ``out``: a tensor of that shape to fill."""
    T, hb, wb = _payload(payload_u8, fmt, H, W)[0], (H + 7) // 8, (W + 7) // 8
    y = out if out is not None else torch.empty((T, hb, wb), dtype=torch.uint16, device=payload_u8.device)
    assert tuple(y.shape) == (T, hb, wb) and y.dtype == torch.uint16 and y.is_contiguous() and y.device == payload_u8.device
    with torch.cuda.device(payload_u8.device):
        L.check(L.load().sn_yuv_thumb(payload_u8.data_ptr(), fmt, y.data_ptr(), T, H, W,
                                      torch.cuda.current_stream(payload_u8.device).cuda_stream), "sn_yuv_thumb")
    return y


def _noise_hist(symbol: str, shape, payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, lo, hi, out, rect, pairs: bool = False,
                vectors: bool = False, mv=None) -> torch.Tensor:
    """What the six histogram functions share: T payloads -> uint32 [T, *shape] from ``symbol``; with ``pairs`` T >= 2 payloads -> [T - 1, *shape];
    with ``vectors`` the entry point takes ``mv`` as well, int8 [T - 1, nby, nbx, 2] on the payloads' device.  Its contents are not looked at: the
    kernel tests every displaced block against the picture."""
    T, dev = _payload(payload_u8, fmt, H, W)
    if pairs and T < 2:
        raise ValueError(f"{symbol}: a pair needs two payloads, got {T}")
    n = T - 1 if pairs else T
    lo, hi = _clip(fmt, lo, hi)
    r = None if rect is None else _rect(rect, fmt, H, W)
    y = out if out is not None else torch.empty((n,) + shape, dtype=torch.uint32, device=dev)
    assert tuple(y.shape) == (n,) + shape and y.dtype == torch.uint32 and y.is_contiguous() and y.device == dev
    args = [payload_u8.data_ptr(), fmt] + ([] if symbol == "sn_yuv_noise_hist" else [r])      # the one entry point without a rectangle
    if vectors:
        from .noise import motion_grid
        nby, nbx = motion_grid(H if r is None else r.h, W if r is None else r.w)
        assert tuple(mv.shape) == (n, nby, nbx, 2) and mv.dtype == torch.int8 and mv.is_contiguous() and mv.device == dev
        if nby * nbx == 0:                                    # no whole block: no vector to point at, and what the entry point writes then
            return y.zero_()
        args.append(mv.data_ptr())
    with torch.cuda.device(dev):
        L.check(getattr(L.load(), symbol)(*args, y.data_ptr(), lo, hi, T, H, W, torch.cuda.current_stream(dev).cuda_stream), symbol)
    return y


def noise_hist_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, lo: Optional[int] = None, hi: Optional[int] = None,
                   out: Optional[torch.Tensor] = None, rect=None) -> torch.Tensor:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device (only the luma plane of each payload is read) -> uint32 [T, 2 (2^bits - 1) + 1]:
    per frame the counts of v = |a - b - c + d| over the non-overlapping 2 x 2 luma blocks whose four codes lie strictly between ``lo`` and
    ``hi`` (default: the format's black and white codes, noise.clip_codes).  ``out``: a tensor of that shape to overwrite.
    ``rect=(x0, y0, w, h)``: the blocks of that picture of the stream alone, the block grid anchored at (x0, y0): the cropped stream's histograms."""
    from .noise import nbins
    return _noise_hist("sn_yuv_noise_hist" if rect is None else "sn_yuv_noise_hist_rect", (nbins(fmt.bits),), payload_u8, fmt, H, W, lo, hi, out, rect)


def noise_hist_bands_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, lo: Optional[int] = None, hi: Optional[int] = None,
                         out: Optional[torch.Tensor] = None, rect=None) -> torch.Tensor:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device (only the luma plane of each payload is read) -> uint32 [T, 16, NBV], NBV = 128 / 512:
    ``noise_hist_yuv``'s counts split by the block's brightness, band = (16 (S - 4 lo)) / (4 (hi - lo)) for the block's sum S, and v saturated to
    NBV - 1 (the last bin means "at least NBV - 1").  ``lo``, ``hi``, ``out``, ``rect`` as there."""
    from .noise import NLF_BANDS, nlf_bins
    return _noise_hist("sn_yuv_noise_hist_bands", (NLF_BANDS, nlf_bins(fmt.bits)), payload_u8, fmt, H, W, lo, hi, out, rect)


def noise_hist_pairs_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, lo: Optional[int] = None, hi: Optional[int] = None,
                         out: Optional[torch.Tensor] = None, rect=None) -> torch.Tensor:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device, T >= 2 (only the luma plane of each payload is read) -> uint32 [T - 1, 4 (2^bits - 1) + 1]:
    per pair of consecutive payloads the counts of v = |HH(p + 1) - HH(p)|, HH = a - b - c + d of the same 2 x 2 luma block in both, over the blocks
    whose eight codes lie strictly between ``lo`` and ``hi``.  ``lo``, ``hi``, ``out``, ``rect`` as ``noise_hist_yuv``."""
    from .noise import pair_bins
    return _noise_hist("sn_yuv_noise_hist_pairs", (pair_bins(fmt.bits),), payload_u8, fmt, H, W, lo, hi, out, rect, pairs=True)


def noise_hist_pairs_bands_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, lo: Optional[int] = None, hi: Optional[int] = None,
                               out: Optional[torch.Tensor] = None, rect=None) -> torch.Tensor:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device, T >= 2 -> uint32 [T - 1, 16, NBV], NBV = 128 / 512: ``noise_hist_pairs_yuv``'s counts split by
    the brightness of the block in both payloads, band = (2 (S - 8 lo)) / (hi - lo) for the sum S of the eight codes, and v saturated to NBV - 1.
    ``lo``, ``hi``, ``out``, ``rect`` as ``noise_hist_yuv``."""
    from .noise import NLF_BANDS, nlf_bins
    return _noise_hist("sn_yuv_noise_hist_pairs_bands", (NLF_BANDS, nlf_bins(fmt.bits)), payload_u8, fmt, H, W, lo, hi, out, rect, pairs=True)


def block_motion_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, rect=None, out_mv: Optional[torch.Tensor] = None,
                     out_sad: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device, T >= 2 (only the luma plane of each payload is read) -> (int8 [T - 1, nby, nbx, 2], uint32
    [T - 1, nby, nbx]) with (nby, nbx) = noise.motion_grid(h, w): per pair of consecutive payloads and per 16 x 16 luma block the vector (dy, dx),
    |dy|, |dx| <= 7, with the smallest sum of absolute differences over the block's matching 2 x 2 blocks ((i + j) even), and that sum
    (include/shiftnet_hip.h: sn_yuv_block_motion states the admissible candidates and the tie order).  ``rect=(x0, y0, w, h)``: the blocks of that
    picture of the stream, the grid anchored at (x0, y0): the cropped stream's vectors.  ``out_mv`` / ``out_sad``: tensors of those shapes to overwrite.
    A picture without a whole 2 x 2 block has empty grids and nothing is launched."""
    from .noise import motion_grid
    T, dev = _payload(payload_u8, fmt, H, W)
    if T < 2:
        raise ValueError(f"sn_yuv_block_motion: a pair needs two payloads, got {T}")
    r = None if rect is None else _rect(rect, fmt, H, W)
    nby, nbx = motion_grid(H if r is None else r.h, W if r is None else r.w)
    mv = out_mv if out_mv is not None else torch.empty((T - 1, nby, nbx, 2), dtype=torch.int8, device=dev)
    sad = out_sad if out_sad is not None else torch.empty((T - 1, nby, nbx), dtype=torch.uint32, device=dev)
    assert tuple(mv.shape) == (T - 1, nby, nbx, 2) and mv.dtype == torch.int8 and mv.is_contiguous() and mv.device == dev
    assert tuple(sad.shape) == (T - 1, nby, nbx) and sad.dtype == torch.uint32 and sad.is_contiguous() and sad.device == dev
    if nby * nbx:
        with torch.cuda.device(dev):
            L.check(L.load().sn_yuv_block_motion(payload_u8.data_ptr(), fmt, r, mv.data_ptr(), sad.data_ptr(), T, H, W,
                                                 torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_block_motion")
    return mv, sad


def noise_hist_pairs_mv_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, mv: torch.Tensor, lo: Optional[int] = None,
                            hi: Optional[int] = None, out: Optional[torch.Tensor] = None, rect=None) -> torch.Tensor:
    """``noise_hist_pairs_yuv`` along the vectors ``mv`` of ``block_motion_yuv`` (same payloads, same ``rect``): only the measuring 2 x 2 blocks ((i + j)
    odd) count, the second payload's four codes are those at (2 i + dy, 2 j + dx) with (dy, dx) the vector of block (i / 8, j / 8), and a block whose
    displaced position is not wholly inside the picture does not count.  Any int8 contents of ``mv`` are safe."""
    from .noise import pair_bins
    return _noise_hist("sn_yuv_noise_hist_pairs_mv", (pair_bins(fmt.bits),), payload_u8, fmt, H, W, lo, hi, out, rect, pairs=True, vectors=True, mv=mv)


def noise_hist_pairs_bands_mv_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, mv: torch.Tensor, lo: Optional[int] = None,
                                  hi: Optional[int] = None, out: Optional[torch.Tensor] = None, rect=None) -> torch.Tensor:
    """``noise_hist_pairs_bands_yuv`` along the vectors ``mv``, with the three differences of ``noise_hist_pairs_mv_yuv``."""
    from .noise import NLF_BANDS, nlf_bins
    return _noise_hist("sn_yuv_noise_hist_pairs_bands_mv", (NLF_BANDS, nlf_bins(fmt.bits)), payload_u8, fmt, H, W, lo, hi, out, rect, pairs=True, vectors=True, mv=mv)


def noise_map_level(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, Hp: int, Wp: int, knots, dtype: torch.dtype,
                    lo: Optional[int] = None, hi: Optional[int] = None, out: Optional[torch.Tensor] = None, rect=None) -> torch.Tensor:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device (only the luma plane of each payload is read) -> [1, T, 1, Hp, Wp] of ``dtype``: the noise
    plane of the denoisers for a noise-level function.  ``knots``: its 16 values as the network takes them (sigma / 255), rounded to float32 here; knot
    b sits at luma code lo + (b + 0.5) (hi - lo) / 16 (default ``lo``, ``hi``: noise.clip_codes).  The value at a pixel is the function, linear between
    the knots and constant beyond the outer ones, at the bilinear interpolation of the means of the 8 x 8 luma blocks -- not at the noisy pixel itself;
    pixels outside H x W replicate the edge pixel.  ``rect=(x0, y0, w, h)``: the plane of that picture of the stream (Hp >= h, Wp >= w), bit for bit the
    cropped stream's.  ``out``: a [1, T, 1, Hp, Wp] tensor to fill.  The knots travel as a kernel argument: no upload, nothing to wait for."""
    import ctypes as C
    from .noise import NLF_BANDS
    T, _ = _payload(payload_u8, fmt, H, W)
    r = None if rect is None else _rect(rect, fmt, H, W)
    assert Hp >= (H if r is None else r.h) and Wp >= (W if r is None else r.w) and dtype in _CODE
    kn = [float(k) for k in knots]
    if len(kn) != NLF_BANDS or not all(math.isfinite(k) for k in kn):
        raise ValueError(f"knots: need {NLF_BANDS} finite numbers, got {knots!r}")
    lo, hi = _clip(fmt, lo, hi)
    y = out if out is not None else torch.empty((1, T, 1, Hp, Wp), dtype=dtype, device=payload_u8.device)
    assert tuple(y.shape) == (1, T, 1, Hp, Wp) and y.dtype == dtype and y.is_contiguous() and y.device == payload_u8.device
    with torch.cuda.device(payload_u8.device):
        L.check(L.load().sn_noise_map_level(payload_u8.data_ptr(), fmt, r, (C.c_float * NLF_BANDS)(*kn), lo, hi, y.data_ptr(), _CODE[dtype], T, H, W, Hp, Wp,
                                            torch.cuda.current_stream(payload_u8.device).cuda_stream), "sn_noise_map_level")
    return y


def rowcol_sums_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, out_rows: Optional[torch.Tensor] = None,
                    out_cols: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device (only the luma plane of each payload is read) -> (uint32 [T, H], uint32 [T, W]): the exact
    sums of the luma codes of every row and of every column of every frame.  ``out_rows`` / ``out_cols``: tensors of those shapes to overwrite."""
    T, dev = _payload(payload_u8, fmt, H, W)
    rows = out_rows if out_rows is not None else torch.empty((T, H), dtype=torch.uint32, device=dev)
    cols = out_cols if out_cols is not None else torch.empty((T, W), dtype=torch.uint32, device=dev)
    for a, n in ((rows, H), (cols, W)):
        assert tuple(a.shape) == (T, n) and a.dtype == torch.uint32 and a.is_contiguous() and a.device == dev
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_rowcol_sums(payload_u8.data_ptr(), fmt, rows.data_ptr(), cols.data_ptr(), T, H, W,
                                            torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_rowcol_sums")
    return rows, cols


def diff_stats_yuv(ref: torch.Tensor, out: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, rect=None, edge: int = 0,
                   out_sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ref (what came in) and out (what was written): [T, frame_bytes] uint8 on a HIP device each, the same format and size; they may be the same
    tensor -> int64 [T, 16]: per payload the exact sums of d = out - ref that include/shiftnet_hip.h lists under sn_yuv_diff_stats (the counts; the sums
    of d and d^2 of the luma; of its products with the right, the lower and the next payload's sample; the count and the sum of d^2 of the pixels whose
    gradient in ``out`` is at least ``edge`` codes; the sums of d and d^2 of both chroma planes).  ``rect=(x0, y0, w, h)``: the sums of that picture of
    the stream.  ``out_sums``: a tensor of that shape to overwrite.  report.frame_measures turns a row into numbers."""
    T, dev = _payload(ref, fmt, H, W)
    assert _payload(out, fmt, H, W) == (T, dev)
    edge = int(edge)
    if edge < 0:
        raise ValueError(f"edge must be >= 0, got {edge!r}")
    y = out_sums if out_sums is not None else torch.empty((T, L.SN_DIFF_STATS), dtype=torch.int64, device=dev)
    assert tuple(y.shape) == (T, L.SN_DIFF_STATS) and y.dtype == torch.int64 and y.is_contiguous() and y.device == dev
    r = None if rect is None else _rect(rect, fmt, H, W)
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_diff_stats(ref.data_ptr(), out.data_ptr(), fmt, r, edge, y.data_ptr(), T, H, W,
                                           torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_diff_stats")
    return y


def diff_stats_mv_yuv(ref: torch.Tensor, out: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, mv: torch.Tensor, rect=None,
                      out_sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ref (what came in) and out (what was written): [T, frame_bytes] uint8 on a HIP device each, T >= 2, the same format and size; ``mv``: int8
    [T - 1, nby, nbx, 2] as ``block_motion_yuv`` makes it for the same picture (of ``out``, by the restorer's use) -> int64 [T - 1, 8]: per pair of
    consecutive payloads the exact sums that include/shiftnet_hip.h lists under sn_yuv_diff_stats_mv, over the measuring 2 x 2 luma blocks ((i + j) odd)
    whose displaced position lies wholly inside the picture: their samples; the sums of d = out - ref and d^2 in the first payload and, where the vector
    points, in the second; the sum of their product; the sum of the squared difference of ``out`` along the vector; the samples whose vector is not
    (0, 0).  Any int8 contents of ``mv`` are safe.  ``rect=(x0, y0, w, h)``: the sums of that picture of the stream.  ``out_sums``: a tensor of that
    shape to overwrite.  report.pair_measures_mv turns a row into numbers."""
    from .noise import motion_grid
    T, dev = _payload(ref, fmt, H, W)
    assert _payload(out, fmt, H, W) == (T, dev)
    if T < 2:
        raise ValueError(f"sn_yuv_diff_stats_mv: a pair needs two payloads, got {T}")
    r = None if rect is None else _rect(rect, fmt, H, W)
    nby, nbx = motion_grid(H if r is None else r.h, W if r is None else r.w)
    assert tuple(mv.shape) == (T - 1, nby, nbx, 2) and mv.dtype == torch.int8 and mv.is_contiguous() and mv.device == dev
    y = out_sums if out_sums is not None else torch.empty((T - 1, L.SN_DIFF_STATS_MV), dtype=torch.int64, device=dev)
    assert tuple(y.shape) == (T - 1, L.SN_DIFF_STATS_MV) and y.dtype == torch.int64 and y.is_contiguous() and y.device == dev
    if nby * nbx == 0:                                        # no whole block: no vector to point at, and what the entry point writes then
        return y.zero_()
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_diff_stats_mv(ref.data_ptr(), out.data_ptr(), fmt, r, mv.data_ptr(), y.data_ptr(), T, H, W,
                                              torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_diff_stats_mv")
    return y


def niqe_sums_yuv(payload_u8: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, win7_dev: torch.Tensor, rect=None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """payload_u8: [T, frame_bytes] uint8 on a HIP device (only the luma plane of each payload is read); ``win7_dev``: the 7 float32 taps of NIQE's
    window on the same device (niqe.load_params) -> float64 [T, 2, nbh, nbw, 5, 5]: per payload, scale (1, 2) and 96 x 96 block of the picture's top-left
    96 nbh x 96 nbw samples, for the normalised luma and its four neighbour products the five sums include/shiftnet_hip.h lists under sn_yuv_niqe_sums
    (the count and the sum of squares of the negative and of the positive values, the sum of the magnitudes).  ``rect=(x0, y0, w, h)``: the sums of
    that picture of the stream.  ``out``: a tensor of that shape to overwrite.  A picture without a whole block is refused (ValueError): the caller
    decides what no number means.  niqe.block_features and niqe.score turn the sums into the score, on the host."""
    T, dev = _payload(payload_u8, fmt, H, W)
    r = None if rect is None else _rect(rect, fmt, H, W)
    nbh, nbw = (H if r is None else r.h) // L.SN_NIQE_BLOCK, (W if r is None else r.w) // L.SN_NIQE_BLOCK
    if nbh * nbw == 0:
        raise ValueError(f"sn_yuv_niqe_sums: the picture holds no whole {L.SN_NIQE_BLOCK} x {L.SN_NIQE_BLOCK} block")
    assert win7_dev.dtype == torch.float32 and tuple(win7_dev.shape) == (7,) and win7_dev.is_contiguous() and win7_dev.device == dev
    shape = (T, 2, nbh, nbw, L.SN_NIQE_MAPS, L.SN_NIQE_SUMS)
    y = out if out is not None else torch.empty(shape, dtype=torch.float64, device=dev)
    assert tuple(y.shape) == shape and y.dtype == torch.float64 and y.is_contiguous() and y.device == dev
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_niqe_sums(payload_u8.data_ptr(), fmt, r, win7_dev.data_ptr(), y.data_ptr(), T, H, W,
                                          torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_niqe_sums")
    return y


def ssim_tiles(h: int, w: int) -> tuple:
    """(nty, ntx): the tiles of ``sn_yuv_ssim_sums`` for a picture of h x w luma samples, the last row and column partial."""
    return (-(-int(h) // L.SN_SSIM_TILE), -(-int(w) // L.SN_SSIM_TILE))


def ssim_sums_yuv(ref: torch.Tensor, out: torch.Tensor, fmt: "L.YuvFmt", H: int, W: int, rect=None, out_sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ref and out: [T, frame_bytes] uint8 on a HIP device each, the same format and size (only the luma plane of each payload is read); they may be the
    same tensor -> float64 [T, nty, ntx]: per payload and 32 x 32 tile of the picture the sum of the SSIM map of the two luma planes that
    include/shiftnet_hip.h states under sn_yuv_ssim_sums (an 11 x 11 Gaussian window, the border replicated at the picture's edge, constants that follow
    2^bits - 1).  ``rect=(x0, y0, w, h)``: the sums of that picture of the stream.  ``out_sums``: a tensor of that shape to overwrite.
    fullref.ssim_from_tiles turns a payload's tiles into its SSIM, on the host."""
    T, dev = _payload(ref, fmt, H, W)
    assert _payload(out, fmt, H, W) == (T, dev)
    r = None if rect is None else _rect(rect, fmt, H, W)
    shape = (T,) + ssim_tiles(H if r is None else r.h, W if r is None else r.w)
    y = out_sums if out_sums is not None else torch.empty(shape, dtype=torch.float64, device=dev)
    assert tuple(y.shape) == shape and y.dtype == torch.float64 and y.is_contiguous() and y.device == dev
    with torch.cuda.device(dev):
        L.check(L.load().sn_yuv_ssim_sums(ref.data_ptr(), out.data_ptr(), fmt, r, y.data_ptr(), T, H, W,
                                          torch.cuda.current_stream(dev).cuda_stream), "sn_yuv_ssim_sums")
    return y


def tile_accumulate(tile: torch.Tensor, canvas: torch.Tensor, wy: torch.Tensor, wx: torch.Tensor, y0: int, x0: int) -> torch.Tensor:
    """tile: [T, C, th, tw] float32 on a HIP device, the result of one tile's forward; canvas: [T, C, Hc, Wc] float32 on the same device; wy: [th] and
    wx: [tw] float32, the tile's feather weights per axis (windows.plan_tiles) -> ``canvas``, whose th x tw rectangle at (y0, x0) of every plane has
    become ``canvas + (wy[y] * wx[x]) * tile``, every product and sum rounded to float32 on its own (include/shiftnet_hip.h: sn_tile_accumulate).
    Nothing else of the canvas is touched; it is added to, so the caller zeroes it before a window's first tile.  All four tensors contiguous."""
    for name, a, nd in (("tile", tile, 4), ("canvas", canvas, 4), ("wy", wy, 1), ("wx", wx, 1)):
        if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.dim() == nd and a.is_contiguous() and a.device == tile.device):
            raise ValueError(f"tile_accumulate: {name} must be a contiguous float32 tensor of {nd} dimensions on the tile's HIP device")
    T, C, th, tw = tile.shape
    Hc, Wc = canvas.shape[2], canvas.shape[3]
    y0, x0 = int(y0), int(x0)
    if tuple(canvas.shape[:2]) != (T, C) or tuple(wy.shape) != (th,) or tuple(wx.shape) != (tw,):
        raise ValueError(f"tile_accumulate: tile {tuple(tile.shape)} goes with canvas [{T}, {C}, Hc, Wc], wy [{th}] and wx [{tw}], got "
                         f"{tuple(canvas.shape)}, {tuple(wy.shape)}, {tuple(wx.shape)}")
    if min(T, C, th, tw) < 1 or T * C > 65535:
        raise ValueError(f"tile_accumulate: need T, C, th, tw >= 1 and T * C <= 65535, got tile {tuple(tile.shape)}")
    if y0 < 0 or x0 < 0 or y0 + th > Hc or x0 + tw > Wc:
        raise ValueError(f"tile_accumulate: the {th} x {tw} tile at (y0, x0) = ({y0}, {x0}) does not lie inside the {Hc} x {Wc} canvas")
    with torch.cuda.device(tile.device):
        L.check(L.load().sn_tile_accumulate(tile.data_ptr(), canvas.data_ptr(), wy.data_ptr(), wx.data_ptr(), T, C, th, tw, Hc, Wc, y0, x0,
                                            torch.cuda.current_stream(tile.device).cuda_stream), "sn_tile_accumulate")
    return canvas


def time_crossfade(prev: torch.Tensor, cur: torch.Tensor, w_prev: torch.Tensor, w_cur: torch.Tensor, h: int, w: int,
                   sq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """prev: [V, C, Hp, Wp] float32 on a HIP device, the last V frames of the older window's result; cur: the same shape, the first V frames of the
    newer window's; w_prev, w_cur: [V] float32, the weights per shared frame (windows.overlap_weights) -> ``cur``, every sample of which has become
    ``(w_prev[j] * prev) + (w_cur[j] * cur)``, the two products and the sum rounded to float32 on their own (include/shiftnet_hip.h:
    sn_time_crossfade).  ``prev`` is not written.  ``sq``: None, or [V, C] int64 that the kernel ADDS to (the caller zeroes it): per plane the sum over
    the h x w picture of ``rint(clamp(prev - cur, +-8) * 65536) ** 2``, taken before the blend.  All tensors contiguous."""
    for name, a, nd in (("prev", prev, 4), ("cur", cur, 4), ("w_prev", w_prev, 1), ("w_cur", w_cur, 1)):
        if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.dim() == nd and a.is_contiguous() and a.device == cur.device):
            raise ValueError(f"time_crossfade: {name} must be a contiguous float32 tensor of {nd} dimensions on cur's HIP device")
    V, C, Hp, Wp = cur.shape
    h, w = int(h), int(w)
    if tuple(prev.shape) != (V, C, Hp, Wp) or tuple(w_prev.shape) != (V,) or tuple(w_cur.shape) != (V,):
        raise ValueError(f"time_crossfade: cur {tuple(cur.shape)} goes with prev of its shape and weights [{V}], got {tuple(prev.shape)}, "
                         f"{tuple(w_prev.shape)}, {tuple(w_cur.shape)}")
    if min(V, C, Hp, Wp) < 1 or V * C > 65535 or not (1 <= h <= Hp and 1 <= w <= Wp):
        raise ValueError(f"time_crossfade: need V, C, Hp, Wp >= 1, V * C <= 65535 and a picture inside the plane, got cur {tuple(cur.shape)}, h {h}, w {w}")
    if sq is not None:
        if not (isinstance(sq, torch.Tensor) and sq.dtype == torch.int64 and tuple(sq.shape) == (V, C) and sq.is_contiguous() and sq.device == cur.device):
            raise ValueError(f"time_crossfade: sq must be a contiguous int64 tensor [{V}, {C}] on cur's HIP device")
        if h * w > 1 << 25:
            raise ValueError(f"time_crossfade: the statistic takes pictures of at most 2^25 samples, got {h} x {w}")
    with torch.cuda.device(cur.device):
        L.check(L.load().sn_time_crossfade(prev.data_ptr(), cur.data_ptr(), w_prev.data_ptr(), w_cur.data_ptr(), None if sq is None else sq.data_ptr(),
                                           V, C, Hp, Wp, h, w, torch.cuda.current_stream(cur.device).cuda_stream), "sn_time_crossfade")
    return cur


def geo_out_shape(shape, op: int) -> Tuple[int, int, int, int]:
    """The shape of ``geo_transform(a, op)`` for ``a`` of ``shape`` [T, C, H, W]: the two sides swapped under ``SN_GEO_TRANSPOSE``."""
    T, C, H, W = (int(v) for v in shape)
    return (T, C, W, H) if op & L.SN_GEO_TRANSPOSE else (T, C, H, W)


def _geo_args(what: str, a: torch.Tensor, b: torch.Tensor, op: int):
    """a: the plain tensor [T, C, H, W], b: the transformed one; both contiguous, of one dtype, on one HIP device."""
    if not (isinstance(op, int) and not isinstance(op, bool) and 0 <= op <= 15):
        raise ValueError(f"{what}: op must be an int of the four SN_GEO_* bits, 0 .. 15, got {op!r}")
    for t in (a, b):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 and t.is_contiguous() and t.device == a.device and t.dtype == a.dtype):
            raise ValueError(f"{what}: both tensors must be contiguous, of 4 dimensions, of one dtype and on one HIP device")
    if min(a.shape) < 1 or tuple(b.shape) != geo_out_shape(a.shape, op):
        raise ValueError(f"{what}: op {op} takes {tuple(a.shape)} to {geo_out_shape(a.shape, op)} (no empty side), got {tuple(b.shape)}")
    return tuple(int(v) for v in a.shape)


def geo_transform(src: torch.Tensor, op: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src: [T, C, H, W] on a HIP device, contiguous, of a 2- or 4-byte dtype -> the tensor mirrored (``SN_GEO_FLIP_X`` columns, ``SN_GEO_FLIP_Y`` rows),
    transposed (``SN_GEO_TRANSPOSE``, before the flips: [T, C, W, H]) and reversed in time (``SN_GEO_REVERSE_T``) as ``op`` says (include/shiftnet_hip.h:
    sn_geo_transform).  Pure data movement.  ``out``: where to write it (contiguous, of the result's shape and src's dtype, not overlapping src)."""
    if isinstance(src, torch.Tensor) and src.dim() == 4 and out is None:
        out = torch.empty(geo_out_shape(src.shape, op), dtype=src.dtype, device=src.device)
    T, C, H, W = _geo_args("geo_transform", src, out, op)
    if src.element_size() not in (2, 4):
        raise ValueError(f"geo_transform: elements of 2 or 4 bytes, got {src.dtype}")
    with torch.cuda.device(src.device):
        L.check(L.load().sn_geo_transform(src.data_ptr(), out.data_ptr(), src.element_size(), op, T, C, H, W,
                                          torch.cuda.current_stream(src.device).cuda_stream), "sn_geo_transform")
    return out


def geo_accumulate(member: torch.Tensor, canvas: torch.Tensor, op: int, init: bool, scale: float = 1.0) -> torch.Tensor:
    """member: float32, ``geo_out_shape(canvas.shape, op)``, a result computed on ``geo_transform(., op)`` of the input; canvas: [T, C, H, W] float32 ->
    ``canvas``, every sample of which has become ``(canvas + member mapped back) * scale`` -- or ``member mapped back * scale`` with ``init``, which
    does not read the canvas -- the sum and the product each rounded to float32 on its own (include/shiftnet_hip.h: sn_geo_accumulate)."""
    T, C, H, W = _geo_args("geo_accumulate", canvas, member, op)
    if canvas.dtype != torch.float32:
        raise ValueError(f"geo_accumulate: float32 tensors, got {canvas.dtype}")
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"geo_accumulate: scale must be finite, got {scale!r}")
    with torch.cuda.device(canvas.device):
        L.check(L.load().sn_geo_accumulate(member.data_ptr(), canvas.data_ptr(), op, 1 if init else 0, scale, T, C, H, W,
                                           torch.cuda.current_stream(canvas.device).cuda_stream), "sn_geo_accumulate")
    return canvas
