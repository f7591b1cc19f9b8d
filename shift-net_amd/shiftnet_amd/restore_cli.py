"""The command line of the video restorer (inference/restore_video.py): Y4M in, Y4M out.  The restorer itself is shiftnet_amd/restore.py, which
hands these names on; nothing here touches the device before the arguments have been judged."""
from __future__ import annotations

import argparse
import sys
import time
from typing import Optional, Sequence

import numpy as np


def sigma_arg(word: str):
    """--sigma: a number stays the float it always was; 'auto'; anything else names a file with one sigma per window."""
    try:
        return float(word)
    except ValueError:
        return word


def picture_arg(word: str):
    """--picture: 'full' -> None; 'auto'; X:Y:W:H -> the rectangle; anything else names a file with one rectangle per window."""
    if word == "full":
        return None
    parts = word.split(":")
    if len(parts) == 4 and all(p.isdigit() for p in parts):
        return tuple(int(p) for p in parts)
    return word


def amount_arg(word: str):
    """--amount: A -> the float; AY,AC -> the pair (luma, chroma)."""
    parts = word.split(",")
    if len(parts) not in (1, 2):
        raise argparse.ArgumentTypeError(f"A or AY,AC, got {word!r}")
    try:
        vals = tuple(float(p) for p in parts)
    except ValueError:
        raise argparse.ArgumentTypeError(f"A or AY,AC with numbers in [0, 1], got {word!r}") from None
    return vals[0] if len(vals) == 1 else vals


def report_edge_arg(word: str) -> float:
    """--report_edge: a finite number >= 0."""
    import math
    try:
        v = float(word)
    except ValueError:
        v = math.nan
    if not (math.isfinite(v) and v >= 0.0):
        raise argparse.ArgumentTypeError(f"a finite number >= 0, got {word!r}")
    return v


def add_noise_arg(word: str):
    """--add_noise: SIGMA or s0,...,s15 -> the 16 knots."""
    from .degrade import parse_add_noise
    try:
        return parse_add_noise(word)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def add_blur_arg(word: str) -> int:
    """--add_blur: N -> the odd number of frames averaged."""
    from .degrade import parse_add_blur
    try:
        return parse_add_blur(word)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def deflicker_arg(word: str) -> int:
    """--deflicker: R, the frames looked at on either side, 1 .. 15."""
    from .deflicker import parse_deflicker
    try:
        return parse_deflicker(word)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def despot_arg(word: str) -> int:
    """--despot: T, the threshold in 8-bit codes, 1 .. 255."""
    from .despot import parse_despot
    try:
        return parse_despot(word)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def grain_arg(word: str):
    """--grain: SIGMA or s0,...,s15 -> the 16 knots; auto / auto:SHARE -> ("auto", share)."""
    from .grain import parse_grain
    try:
        return parse_grain(word)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def tile_arg(word: str):
    """--tile: N -> the int (N x N tiles); HxW -> (H, W)."""
    parts = word.lower().split("x")
    if len(parts) not in (1, 2) or not all(p.isdigit() for p in parts):
        raise argparse.ArgumentTypeError(f"N or HxW in samples, got {word!r}")
    vals = tuple(int(p) for p in parts)
    return vals[0] if len(vals) == 1 else vals


def _modes():
    from .y4m import MODES
    return MODES


def make_parser() -> argparse.ArgumentParser:
    from .restore import VARIANTS
    ap = argparse.ArgumentParser(description="Restore a Y4M video with Shift-Net on the MI355X: same frames and size out, same pixel format unless "
                                             "--out_format names another")
    ap.add_argument("--variant", choices=list(VARIANTS), required=True)
    ap.add_argument("--checkpoint", required=True, help="checkpoint path, or 'synthetic' for the deterministic synthetic weights")
    ap.add_argument("--dtype", choices=["fp32", "fp16", "bf16"], default="bf16")
    ap.add_argument("--one_len", type=int, default=16, help="frames restored per window")
    ap.add_argument("--sigma", type=sigma_arg, default=None, metavar="{NUMBER,auto,FILE}",
                    help="noise level (8-bit code values), required by the denoise variants: a number; 'auto' estimates it per window on the device "
                         "(a heuristic that assumes white Gaussian noise); FILE lists one sigma per window, one per line ('#' comments)")
    ap.add_argument("--sigma_clamp", type=float, nargs=2, default=(0.0, 50.0), metavar=("LO", "HI"), help="auto: the estimate is clamped to this range")
    ap.add_argument("--sigma_estimator", choices=["spatial", "temporal", "min"], default="spatial",
                    help="--sigma auto only: 'temporal' estimates the noise from the difference of consecutive frames, in which texture that does not move "
                         "cancels (temporally correlated noise -- inter-coded or temporally denoised footage -- reads low); 'min' takes the lower of that and "
                         "the spatial estimate; with --noise_model level the curve follows band by band; default spatial: each frame on its own")
    ap.add_argument("--sigma_motion", choices=["none", "blocks"], default="none",
                    help="--sigma_estimator temporal / min only: 'blocks' finds one integer vector (within +-7 px) per 16 x 16 luma block and frame pair on the "
                         "device and lets the temporal estimate follow it, so that a pan does not read as noise (a heuristic, checked on synthetic clips "
                         "only: sub-pixel motion, zoom and rotation still read as noise, and flat content reads a few per cent high); default none: every "
                         "block is compared with the block at the same place")
    ap.add_argument("--sigma_out", default=None, metavar="FILE", help="write the sigma that every window was restored with, in the format --sigma FILE reads")
    ap.add_argument("--noise_model", default="flat", metavar="{flat,level,FILE}",
                    help="denoise variants: 'level' (needs --sigma auto) estimates per window the noise level as a function of brightness on the device and "
                         "gives the network a noise plane that follows it (a heuristic, checked on synthetic clips only); FILE lists one curve per window, "
                         "16 sigmas per line from black to white ('#' comments); default flat: one level per window")
    ap.add_argument("--noise_model_out", default=None, metavar="FILE",
                    help="write the curve every window was restored with, in the format --noise_model FILE reads")
    ap.add_argument("--matrix", choices=["bt601", "bt709"], default=None, help="default: bt709 when H >= 720, else bt601")
    ap.add_argument("--range", choices=["limited", "full"], default=None, help="default: the stream's XCOLORRANGE, else limited")
    ap.add_argument("--no_pipeline", action="store_true", help="run read / copy / forward / write one after the other")
    ap.add_argument("--scene_cuts", default="off", metavar="{off,auto,FILE}",
                    help="restore every scene as a clip of its own: 'auto' finds the cuts on the device (a heuristic, see --cut_threshold / --cut_ratio), "
                         "FILE lists the first frame of every scene but the first, one index per line ('#' comments); default off: the stream is one clip")
    ap.add_argument("--cut_threshold", type=float, default=4.0, help="auto: smallest mean absolute difference of 8x8 block means (8-bit code units) of a cut")
    ap.add_argument("--cut_ratio", type=float, default=2.5, help="auto: ... and at least this many times the median of the six neighbouring frames' differences")
    ap.add_argument("--picture", default="full", metavar="{full,auto,X:Y:W:H,FILE}",
                    help="restore the active picture of a letterboxed / pillarboxed stream only and leave the bars as they are: X:Y:W:H in luma samples; "
                         "'auto' finds the bars per window on the device (a heuristic, see --bar_level); FILE lists 'x0 y0 w h' (or 'full') per window, one "
                         "per line ('#' comments); default full: the whole frame")
    ap.add_argument("--bar_level", type=float, default=1.0, help="auto: a row or column is bar if its mean luma stays within this many 8-bit codes of black")
    ap.add_argument("--picture_out", default=None, metavar="FILE", help="write the picture every window was restored with, in the format --picture FILE reads")
    ap.add_argument("--out_format", choices=list(_modes()), default=None, metavar="TAG",
                    help="write this Y4M C tag instead of the input's (%(choices)s): another bit depth and chroma layout, e.g. 444p10 or 420p10 to keep the "
                         "precision of the result when 8 bit came in; matrix and range stay the input's; default: the input's format")
    ap.add_argument("--dither", choices=["none", "tpdf"], default="none",
                    help="tpdf: add triangular noise of +-1 code before rounding to the output's codes: no banding, about 0.5 code rms of noise instead; "
                         "default none: round to nearest")
    ap.add_argument("--dither_seed", type=int, default=0, metavar="N", help="tpdf: which noise (0 .. 2^32 - 1); the same seed gives the same bytes")
    ap.add_argument("--amount", type=amount_arg, default=None, metavar="{A,AY,AC}",
                    help="how much of the restoration to apply, 0 .. 1: every code written is the input's moved by that share of the way to the result's "
                         "(linear in the code domain, not perceptual; 0 writes the input byte for byte); AY,AC sets luma and chroma separately, e.g. 0.5,1 "
                         "denoises chroma fully and luma at half; default: the full result")
    ap.add_argument("--view", choices=["restored", "removed"], default="restored",
                    help="removed: write what the restoration took out instead of the result, input minus result around mid-grey (see --removed_gain); "
                         "not together with an --amount other than 1; default restored")
    ap.add_argument("--removed_gain", type=float, default=1.0, metavar="G", help="removed: the difference is multiplied by G (finite, >= 0) to make it visible")
    ap.add_argument("--report", default=None, metavar="FILE",
                    help="measure what the run changed and write one line per written frame: written minus input as noise level (removed_sigma, to be read "
                         "beside --sigma_out), its correlation with the right, lower and next-frame neighbour (rho_x, rho_y, rho_t: about 0 if only noise "
                         "left) and its energy on edges over that elsewhere (edge_ratio: about 1 if only noise left); medians in the last line and in the "
                         "log; changes no byte written; the interpretation is unvalidated on real footage; not together with --view removed")
    ap.add_argument("--report_edge", type=report_edge_arg, default=16.0, metavar="E",
                    help="report: a pixel is an edge where the written luma's gradient |right - here| + |below - here| reaches E 8-bit codes (finite, >= 0; "
                         "the default is a guess nobody has tuned)")
    ap.add_argument("--report_motion", choices=["none", "blocks"], default="none",
                    help="--report only: 'blocks' adds the correlation of written minus input with the next frame's ALONG the motion of the written picture "
                         "(rho_t_mv; one integer vector within +-7 px per 16 x 16 luma block and frame pair, found on the device), because removed detail "
                         "that moves with a pan reads rho_t about 0 as noise does; also how well the vectors fit (mv_match_rms), the share that moved and "
                         "the share counted; blocks at the border of a pan read low, zoom and rotation still read as uncorrelated; unvalidated on real "
                         "footage; default none: the report as it is without")
    ap.add_argument("--report_quality", choices=["none", "niqe"], default="none",
                    help="--report only: 'niqe' adds two columns about the pictures themselves, NIQE (a no-reference score, lower is nearer to natural "
                         "pictures) of the luma of every input frame and of the frame written for it (niqe_in, niqe_out); sums on the device, the fit on "
                         "the host; nan below two 96 x 96 blocks; the model was fitted to natural stills and BT.601 luma, the stream's own luma is fed; "
                         "denoising can move it either way; no threshold, no verdict, unvalidated on real footage; default none: the report as it is without")
    ap.add_argument("--niqe_params", default=None, metavar="FILE",
                    help="--report_quality niqe: the pristine model (an .npz with mu_pris_param, cov_pris_param, gaussian_window); default: "
                         "tests/golden/niqe_pris_params.npz of the checkout")
    ap.add_argument("--gt", default=None, metavar="FILE",
                    help="--report only: a ground-truth Y4M of the width, height and C tag of the stream WRITTEN (--out_format if given), frame i the truth "
                         "of written frame i; adds eight columns, PSNR of Y, U and V and SSIM of the luma of every input frame and of the frame written "
                         "for it against the truth (psnr_y_in psnr_y_out ... ssim_in ssim_out; peak and SSIM constants follow 2^bits - 1; SSIM is the "
                         "Y-channel SSIM of the evaluation harnesses: 11 x 11 Gaussian window, replicated border, every frame and every position); sums on "
                         "the device; LUMA SSIM ONLY, no MS-SSIM or VMAF; the streams must be frame-aligned, no offset is searched; no threshold, no "
                         "verdict, nothing fed back; changes no byte written; default: the report as it is without")
    ap.add_argument("--add_noise", type=add_noise_arg, default=None, metavar="{SIGMA,s0,...,s15}",
                    help="IN is a CLEAN stream: add Gaussian noise to it on the device and restore the degraded stream; SIGMA is the standard deviation in "
                         "8-bit R'G'B' code values, 16 comma-separated values are a curve from black to white (the knots --noise_model FILE reads) taken at "
                         "the clean pixel's luma; with --report the clean frames are the truth and the report has the columns of --gt (not together with "
                         "--gt, nor with --report and an --out_format other than the input's).  I.i.d. per R'G'B' channel, added before chroma subsampling: "
                         "what the networks were trained with, not a sensor and a codec; clipped to the legal codes; tails end at about 4.3 sigma; the "
                         "colour conversion round trip runs even at 0, so 0 is not the input byte for byte; bars are noised too; default: IN is the input")
    ap.add_argument("--add_noise_seed", type=int, default=0, metavar="N", help="--add_noise: which noise (0 .. 2^32 - 1); the same seed gives the same bytes")
    ap.add_argument("--degraded_out", default=None, metavar="FILE",
                    help="--add_noise / --add_blur: write the degraded stream, a Y4M with the input's header")
    ap.add_argument("--add_blur", type=add_blur_arg, default=None, metavar="N",
                    help="IN is a SHARP stream: blur it on the device and restore the blurred stream, for the deblur variants; every frame becomes the mean "
                         "of N consecutive frames around it (N odd, 1 .. 15), taken on R'G'B' in linear light (--add_blur_gamma), as the deblur datasets "
                         "(GOPRO, DVD) are made; the window is clamped at the stream's ends and, with a LISTED --scene_cuts, to the frame's scene; with "
                         "--scene_cuts auto the cuts are found afterwards on the blurred stream and the blur crosses them; with --report the sharp frames "
                         "are the truth and the report has the columns of --gt (not together with --gt or --add_noise, nor with --report and an "
                         "--out_format other than the input's).  A box over N frames of the stream as it is: its length in time is N / fps of the input, "
                         "no frame is dropped; a pure power law, not the sRGB curve; not a lens and not a rolling shutter; N = 1 still runs the colour "
                         "conversion round trip, so it is not the input byte for byte; bars are averaged too; default: IN is the input")
    ap.add_argument("--add_blur_gamma", type=float, default=2.2, metavar="G",
                    help="--add_blur: the power law between R'G'B' and the linear light the frames are averaged in, 1 .. 3; 1 averages the R'G'B' values "
                         "as they are (default 2.2)")
    ap.add_argument("--deflicker", type=deflicker_arg, default=None, metavar="R",
                    help="take brightness flicker out of IN on the device, in front of everything else: every frame gets one tone curve that matches "
                         "its luma histogram to the median of the histograms of the R frames on either side (1 .. 15), inside its scene under a listed "
                         "--scene_cuts; payloads to payloads, no colour conversion.  The deflickered stream is THE input of all the rest (--amount 0 "
                         "returns it, not the file).  One curve per frame: local flicker stays; a real flash is pulled towards its neighbours; moving "
                         "content that changes the histogram reads as flicker; computed on codes, not in linear light; bars are in the histogram; "
                         "nobody has judged it on real footage; not together with --add_noise or --add_blur; default: off")
    ap.add_argument("--deflicker_chroma", choices=["gain", "off"], default="gain",
                    help="--deflicker: 'gain' scales Cb and Cr about mid-grey by the factor the frame's mean luma above black changed by, clamped to "
                         "0.5 .. 2 (default); 'off' leaves chroma as it came")
    ap.add_argument("--deflicker_out", default=None, metavar="FILE",
                    help="--deflicker: write one line per frame, 'r mean_in mean_out chroma_gain', and a last line with the rms second difference of "
                         "the frame means before and after")
    ap.add_argument("--despot", type=despot_arg, default=None, metavar="T",
                    help="take dirt, dust, blotches and dropouts -- small regions that are wrong in exactly ONE frame -- out of IN on the device, in "
                         "front of everything else and behind --deflicker: a luma sample that differs from both motion-compensated neighbours "
                         "(frames f - 1 and f + 1 along one integer vector per 16 x 16 block) in the same direction by more than T + |p - n| is a "
                         "seed, T in 8-bit codes (1 .. 255; 24 is a start); seeds with --despot_support seeds around them, grown by --despot_grow, "
                         "become the mean of the two neighbours; inside its scene under a listed --scene_cuts, whose first and last frame leave as "
                         "they came; payloads to payloads, no colour conversion.  The despotted stream is THE input of all the rest.  One threshold "
                         "in codes, not scaled to the footage's noise; dirt that stays for two frames and line scratches are not found; small fast "
                         "objects that are in one place for one frame ARE taken for dirt; the repair is soft; luma alone decides; nobody has judged "
                         "it on real footage; not together with --add_noise or --add_blur; default: off")
    ap.add_argument("--despot_support", type=int, default=2, metavar="K",
                    help="--despot: a seed counts only with at least K seeds among its eight neighbours, 0 .. 8: dirt comes in blobs, noise in single "
                         "samples (default 2)")
    ap.add_argument("--despot_grow", type=int, default=1, metavar="G",
                    help="--despot: the mask is grown by G samples, 0 .. 2: a blotch has a soft edge that stays under T (default 1)")
    ap.add_argument("--despot_chroma", choices=["follow", "off"], default="follow",
                    help="--despot: 'follow' repairs a chroma sample where its luma is repaired (default); 'off' leaves chroma as it came")
    ap.add_argument("--despot_max_share", type=float, default=0.05, metavar="S",
                    help="--despot: a frame of which more than this share would be replaced -- a flash, a frame under uncorrected flicker, a cut the "
                         "motion search could not follow -- is handed on as it came, in (0, 1] (default 0.05)")
    ap.add_argument("--despot_out", default=None, metavar="FILE",
                    help="--despot: write one line per frame, 'seeds replaced share kept', and a last line with the median share and the number of "
                         "frames kept")
    ap.add_argument("--grain", type=grain_arg, default=None, metavar="{SIGMA,s0,...,s15,auto,auto:SHARE}",
                    help="put fine grain back on the stream written, on the device, behind everything else ('denoise, encode, re-grain'): SIGMA is its "
                         "level in the unit of --sigma, the sigma of i.i.d. noise on 8-bit R'G'B' whose luma part the grain equals; 16 comma-separated "
                         "values are a curve from black to white taken at the written luma code; 'auto' is SHARE (0 .. 4, default 0.5) times what the "
                         "window was restored with (the denoise variants).  A Gaussian field of the size --grain_size says, NOT a model fitted to the "
                         "removed noise: no AR fit, no film-grain table for an encoder; independent from frame to frame; rounded to codes and clipped at "
                         "the legal range; under auto it steps at window boundaries; --report, --gt and NIQE describe the stream with the grain; nobody "
                         "has judged it on real footage; not together with --view removed; default: no grain")
    ap.add_argument("--grain_size", type=float, default=0.0, metavar="S",
                    help="--grain: the standard deviation, in samples, of the Gaussian the grain is filtered with (5 taps each way, unit energy), "
                         "0 .. 1.2; 0 is white grain (default); 4:2:0 chroma grain lives at chroma resolution and looks twice the size")
    ap.add_argument("--grain_chroma", type=float, default=0.0, metavar="C",
                    help="--grain: the chroma planes get grain of their own at C times the luma's level (a plain factor, >= 0); default 0: chroma stays")
    ap.add_argument("--grain_seed", type=int, default=0, metavar="N", help="--grain: which grain (0 .. 2^32 - 1); the same seed gives the same bytes")
    ap.add_argument("--grain_out", default=None, metavar="FILE",
                    help="--grain: write the curve of every window's grain, 16 levels per line in the format --noise_model FILE reads")
    ap.add_argument("--tile", type=tile_arg, default=None, metavar="{N,HxW}",
                    help="for frames whose activations do not fit the device: run the network on overlapping tiles of H x W samples (N: N x N) of every "
                         "window, one after the other, and blend their results with feather weights on the device; both sides multiples of 4 (8 for "
                         "the deblur / denoise variants without _small) and at least twice that; everything but the forward still sees the whole "
                         "picture.  A TILED RESULT IS NOT THE FULL-FRAME RESULT: every channel-attention layer pools over the tile it is given and the "
                         "receptive field is cut at tile edges; the feather turns a mismatch into a gradient instead of an edge, it does not remove it; "
                         "nobody has looked at a seam on real footage; default: whole frames")
    ap.add_argument("--tile_overlap", type=int, default=None, metavar="V",
                    help="--tile only: consecutive tiles overlap by at least V samples, 0 <= V <= half the tile's shorter side; default 32, taken from "
                         "upstream's quadrants (which crop 17 to 32 samples per side) and never tuned")
    ap.add_argument("--ensemble", type=int, choices=(1, 2, 4, 8), default=1,
                    help="test-time self-ensemble: run the network on that many copies of every window -- the window, its columns mirrored, its rows "
                         "mirrored and both, at 8 also their transposes -- map every result back and write their mean.  A WINDOW COSTS THAT MANY "
                         "FORWARDS.  The transposed copies have another input signature: the engine builds a plan of its own for them in the first "
                         "window.  NOBODY HAS MEASURED WHAT THIS GAINS ON SHIFT-NET: the +0.05 to +0.2 dB quoted for image super-resolution is a figure "
                         "from the literature for other networks, and no trained checkpoint ships here.  Not with --tile; default 1: one forward")
    ap.add_argument("--ensemble_time", action="store_true",
                    help="double the members of --ensemble: the same copies of the window reversed in time (twice the forwards again)")
    ap.add_argument("--window_overlap", type=int, default=0, metavar="V",
                    help="consecutive windows of a scene share V frames, 0 <= V <= one_len / 2, and the two answers for a shared frame are cross-faded on "
                         "the device with a linear ramp in time, against a step at every window boundary.  A WINDOW STILL COSTS ONE FORWARD AND THERE ARE "
                         "one_len / (one_len - V) TIMES AS MANY.  The cross-fade blends two different answers: a mismatch becomes a ramp over V frames, it "
                         "is not removed; nobody has looked at a seam of a trained network; default 0: window k + 1 starts where window k ends")
    ap.add_argument("--seams_out", default=None, metavar="FILE",
                    help="--window_overlap: write one line per window, '-' or the V rms differences (8-bit R'G'B' code units, oldest shared frame first) "
                         "between the previous window's answer for the shared frames and this window's, measured before the cross-fade")
    ap.add_argument("--cuts_out", default=None, metavar="FILE", help="write the scene starts that were used, in the format --scene_cuts FILE reads")
    ap.add_argument("input", metavar="IN", help="Y4M file, or - for stdin")
    ap.add_argument("output", metavar="OUT", help="Y4M file, or - for stdout")
    return ap


def _text_reader(parse):
    """parse(text) as a reader by path."""
    def read(path):
        with open(path, "r") as fh:
            return parse(fh.read())
    return read


def _text_writer(fmt):
    """fmt(*args) -> text as a writer by path."""
    def write(path, *args):
        with open(path, "w") as fh:
            fh.write(fmt(*args))
    return write


def _listed(ap: argparse.ArgumentParser, flag: str, word: str, read):
    """The FILE form of a {keyword,FILE} option: what ``read(word)`` makes of the file, or the parser's error naming the option and the word."""
    try:
        return read(word)
    except (OSError, ValueError) as e:
        ap.error(f"{flag} {word}: {e}")


def _injected(knots) -> str:
    """The level --add_noise injected, for the log: the number, or the ends of the curve."""
    return "%g" % knots[0] if min(knots) == max(knots) else "a curve, %g at black .. %g at white" % (knots[0], knots[-1])


def _write_out(path: Optional[str], write, *args) -> None:
    """A --*_out option: ``write(path, *args)`` where a path was given."""
    if path is not None:
        write(path, *args)


def main(argv: Optional[Sequence[str]] = None) -> int:
    from . import lib as L
    from . import noise, picture as pic, scenes
    from .deflicker import deflicker_form, format_deflicker, mean_roughness
    from .despot import despot_form, format_despot, frames_kept, median_share
    from .grain import grain_form
    from .io_edges import yuv_fmt
    from .restore import VideoRestorer, load_net
    from . import report as rep
    from .spec import VARIANTS as SPECS
    from .restore import VARIANTS
    from .windows import DEFAULT_TILE_OVERLAP, amount_form, ensemble_form, format_seams, quality_form, report_form, report_motion_form, tile_form, window_overlap_form
    from .y4m import Y4MReader, Y4MWriter, output_header
    ap = make_parser()
    a = ap.parse_args(argv)
    if not (0 <= a.dither_seed < 2 ** 32):
        ap.error("--dither_seed: an integer in 0 .. 2^32 - 1")
    view = None if a.view == "restored" else a.view
    try:
        amount_form(a.amount, view, a.removed_gain)
    except ValueError as e:
        ap.error(f"--amount / --view / --removed_gain: {e}")
    try:
        report_form(a.report is not None, a.report_edge, view)
    except ValueError as e:
        ap.error(f"--report / --report_edge / --view: {e}")
    try:                                                          # as above: before any file is opened
        report_motion = report_motion_form(None if a.report_motion == "none" else a.report_motion, a.report is not None)
    except ValueError:
        ap.error(f"--report_motion {a.report_motion} needs --report")
    report_quality = None if a.report_quality == "none" else a.report_quality
    try:                                                          # as above; the model is read here and again by the restorer
        quality_form(report_quality, a.niqe_params, a.report is not None)
    except ValueError as e:
        ap.error(f"--report_quality / --niqe_params: {str(e).replace('report=True', '--report')}")
    if a.gt is not None and a.report is None:                     # as above: before any file is opened
        ap.error("--gt adds its columns to the report: it needs --report")
    if a.add_noise is not None and a.gt is not None:              # as above: before any file is opened
        ap.error("--add_noise makes the clean input the truth of the report: not together with --gt")
    if a.add_blur is not None and a.gt is not None:
        ap.error("--add_blur makes the sharp input the truth of the report: not together with --gt")
    if a.add_blur is not None and a.add_noise is not None:
        ap.error("--add_blur together with --add_noise: no network here was trained on both, pick one")
    if a.add_noise is None and (a.add_noise_seed != 0 or (a.degraded_out is not None and a.add_blur is None)):
        ap.error("--add_noise_seed / --degraded_out need --add_noise (--degraded_out also goes with --add_blur)")
    if a.add_blur is None and a.add_blur_gamma != 2.2:
        ap.error("--add_blur_gamma needs --add_blur")
    if not (1.0 <= a.add_blur_gamma <= 3.0):
        ap.error("--add_blur_gamma: a number in 1 .. 3")
    if not (0 <= a.add_noise_seed < 2 ** 32):
        ap.error("--add_noise_seed: an integer in 0 .. 2^32 - 1")
    if a.deflicker is None and a.deflicker_out is not None:       # as above: before any file is opened
        ap.error("--deflicker_out needs --deflicker")
    for flag, other in (("--add_noise", a.add_noise), ("--add_blur", a.add_blur)):
        if a.deflicker is not None and other is not None:
            ap.error(f"--deflicker together with {flag}: {flag} makes a degraded copy of a clean stream for an experiment, --deflicker repairs a stream "
                     "that flickers; pick one")
    try:
        deflicker_form(a.deflicker, a.deflicker_chroma)
    except ValueError as e:
        ap.error(f"--deflicker / --deflicker_chroma: {e}")
    if a.despot is None and a.despot_out is not None:             # as above: before any file is opened
        ap.error("--despot_out needs --despot")
    for flag, other in (("--add_noise", a.add_noise), ("--add_blur", a.add_blur)):
        if a.despot is not None and other is not None:
            ap.error(f"--despot together with {flag}: {flag} makes a degraded copy of a clean stream for an experiment, --despot repairs a stream "
                     "that carries dirt; pick one")
    try:
        despot_form(a.despot, a.despot_support, a.despot_grow, a.despot_chroma, a.despot_max_share)
    except ValueError as e:
        ap.error(f"--despot / --despot_support / --despot_grow / --despot_chroma / --despot_max_share: {e}")
    if a.grain is None and a.grain_out is not None:               # as above: before any file is opened
        ap.error("--grain_out needs --grain")
    try:
        grain_mode = grain_form(a.grain, a.grain_size, a.grain_chroma, a.grain_seed)[0]
    except ValueError as e:
        ap.error(f"--grain / --grain_size / --grain_chroma / --grain_seed: {e}")
    if grain_mode is not None and view is not None:
        ap.error(f"--grain together with --view {view}: the view is not the restored stream, there is nothing to put grain back on")
    if grain_mode == "auto" and "denoise" not in a.variant:
        ap.error("--grain auto is a share of the noise level the window was restored with: it is for the denoise variants")
    if a.tile is None and a.tile_overlap is not None:             # as above: before any file is opened
        ap.error("--tile_overlap needs --tile")
    tile_overlap = DEFAULT_TILE_OVERLAP if a.tile_overlap is None else a.tile_overlap
    try:
        tile = tile_form(a.tile, tile_overlap, SPECS[VARIANTS[a.variant]].topo)
    except ValueError as e:
        ap.error(f"--tile / --tile_overlap: {e}")
    try:
        ensemble_form(a.ensemble, a.ensemble_time, tile)
    except ValueError as e:
        ap.error(f"--ensemble / --ensemble_time: {e}")
    try:
        window_overlap_form(a.window_overlap, a.one_len)
    except ValueError as e:
        ap.error(f"--window_overlap: {e}")
    if "denoise" in a.variant and a.sigma is None:
        ap.error("--sigma is required by the denoise variants")
    if a.sigma_estimator != "spatial" and a.sigma != "auto":      # before the file of a --sigma FILE is opened
        ap.error(f"--sigma_estimator {a.sigma_estimator} needs --sigma auto")
    if a.sigma_motion != "none" and a.sigma_estimator == "spatial":      # as above: before any file is opened
        ap.error(f"--sigma_motion {a.sigma_motion} needs --sigma_estimator temporal or min")
    log = lambda s: (sys.stderr.write(s + "\n"), sys.stderr.flush())      # noqa: E731
    sigma, sigma_how = a.sigma, "fixed"
    if isinstance(sigma, str):
        if "denoise" not in a.variant:
            ap.error(f"--sigma {sigma} is for the denoise variants")
        if sigma == "auto":
            sigma_how = "auto"
        else:
            sigma, sigma_how = _listed(ap, "--sigma", sigma, _text_reader(noise.parse_sigmas)), "listed"
    noise_model, nlf_how = None, "flat"
    if a.noise_model != "flat":
        if "denoise" not in a.variant:
            ap.error(f"--noise_model {a.noise_model} is for the denoise variants")
        if a.noise_model == "level":
            if sigma_how != "auto":
                ap.error("--noise_model level needs --sigma auto")
            noise_model, nlf_how = "level", "level"
        else:
            noise_model, nlf_how = _listed(ap, "--noise_model", a.noise_model, _text_reader(noise.parse_curves)), "listed"
    try:
        noise.check_clamp(a.sigma_clamp)
    except ValueError as e:
        ap.error(f"--sigma_clamp: {e}")
    cuts = None if a.scene_cuts == "off" else a.scene_cuts
    if cuts not in (None, "auto"):
        cuts = _listed(ap, "--scene_cuts", cuts, _text_reader(scenes.parse_cuts))
    picture, picture_how = picture_arg(a.picture), "fixed"
    if picture == "auto":
        picture_how = "auto"
    elif isinstance(picture, str):
        picture, picture_how = _listed(ap, "--picture", picture, pic.read_pictures), "listed"
    fin = sys.stdin.buffer if a.input == "-" else open(a.input, "rb")
    fout = sys.stdout.buffer if a.output == "-" else open(a.output, "wb")
    fgt = fdeg = None
    try:
        rd = Y4MReader(fin)
        hd = rd.header
        gt = None
        if a.gt is not None:                                      # judged against the header of the stream written, before the network is loaded
            try:
                fgt = open(a.gt, "rb")
                gt = Y4MReader(fgt)
            except (OSError, ValueError) as e:
                ap.error(f"--gt {a.gt}: {e}")
            want, got = output_header(hd, a.out_format), gt.header
            if (got.width, got.height) != (want.width, want.height):
                ap.error(f"--gt {a.gt}: the truth is {got.width}x{got.height}, the stream written is {want.width}x{want.height}")
            if (got.bits, got.chroma_code) != (want.bits, want.chroma_code):
                ap.error(f"--gt {a.gt}: the truth is C{got.chroma}, the stream written is C{want.chroma}: the truth must be in the format written")
        if (a.add_noise is not None or a.add_blur is not None) and a.report is not None:      # as above: the clean input is the truth, in the format read
            want = output_header(hd, a.out_format)
            if (want.bits, want.chroma_code) != (hd.bits, hd.chroma_code):
                ap.error(f"{'--add_noise' if a.add_noise is not None else '--add_blur'} with --report and --out_format {a.out_format}: the truth is the "
                         f"clean input, C{hd.chroma}, the stream written is C{want.chroma}; it would have to be converted")
        matrix = a.matrix or ("bt709" if hd.height >= 720 else "bt601")
        rng = a.range or (hd.color_range if hd.color_range in ("full", "limited") else "limited")
        log(f"input: {hd.width}x{hd.height} C{hd.chroma} F{hd.fps}; matrix {matrix}{'' if a.matrix else ' (default)'}, range {rng}"
            f"{'' if a.range else (' (stream)' if hd.color_range else ' (default)')}")
        fmt = yuv_fmt(hd.bits, hd.chroma_code, L.SN_YUV_BT709 if matrix == "bt709" else L.SN_YUV_BT601,
                      L.SN_YUV_FULL if rng == "full" else L.SN_YUV_LIMITED)
        net = load_net(a.variant, a.checkpoint, a.dtype)
        vr = VideoRestorer(net, a.one_len, sigma=sigma, pipeline=not a.no_pipeline, scene_cuts=cuts, cut_threshold=a.cut_threshold,
                           cut_ratio=a.cut_ratio, sigma_clamp=a.sigma_clamp, picture=picture, bar_level=a.bar_level, out_format=a.out_format,
                           dither=None if a.dither == "none" else a.dither, dither_seed=a.dither_seed, noise_model=noise_model,
                           amount=a.amount, view=view, removed_gain=a.removed_gain, sigma_estimator=a.sigma_estimator,
                           report=a.report is not None, report_edge=a.report_edge, sigma_motion=None if a.sigma_motion == "none" else a.sigma_motion,
                           report_motion=report_motion, tile=a.tile, tile_overlap=tile_overlap, ensemble=a.ensemble,
                           ensemble_time=a.ensemble_time, window_overlap=a.window_overlap, report_quality=report_quality, niqe_params=a.niqe_params,
                           add_noise=a.add_noise, add_noise_seed=a.add_noise_seed, add_blur=a.add_blur, add_blur_gamma=a.add_blur_gamma,
                           grain=a.grain, grain_size=a.grain_size, grain_chroma=a.grain_chroma, grain_seed=a.grain_seed,
                           deflicker=a.deflicker, deflicker_chroma=a.deflicker_chroma, despot=a.despot, despot_support=a.despot_support,
                           despot_grow=a.despot_grow, despot_chroma=a.despot_chroma, despot_max_share=a.despot_max_share)
        wdeg = None
        if a.deflicker is not None:
            log(f"deflicker: one tone curve per frame from the median of {2 * a.deflicker + 1} luma histograms, chroma {a.deflicker_chroma}; the "
                f"deflickered stream is the input of all the rest{'; the windows cross the cuts --scene_cuts auto finds' if a.scene_cuts == 'auto' else ''}")
        if a.despot is not None:
            log(f"despot: threshold {a.despot} (8-bit codes), support {a.despot_support}, grow {a.despot_grow}, chroma {a.despot_chroma}, at most "
                f"{a.despot_max_share:g} of a frame; {'behind deflicker; ' if a.deflicker is not None else ''}the despotted stream is the input of "
                f"all the rest{'; the windows cross the cuts --scene_cuts auto finds' if a.scene_cuts == 'auto' else ''}")
        if a.add_blur is not None:
            log(f"added blur: the mean of {a.add_blur} frame{'' if a.add_blur == 1 else 's'} (a box of {a.add_blur} frame times at F{hd.fps}), "
                f"{'of the RGB values as they are' if a.add_blur_gamma == 1.0 else 'in linear light through gamma %g' % a.add_blur_gamma}; "
                f"IN is the sharp stream{', and the truth of the report' if a.report is not None else ''}"
                f"{'; the blur crosses the cuts --scene_cuts auto finds' if a.scene_cuts == 'auto' and a.add_blur > 1 else ''}")
        if a.add_noise is not None:
            kn = vr.add_noise
            log(f"added noise: sigma {_injected(kn)} in 8-bit R'G'B' codes, seed "
                f"{a.add_noise_seed}; IN is the clean stream{', and the truth of the report' if a.report is not None else ''}")
        if a.degraded_out is not None:
            fdeg = open(a.degraded_out, "wb")
            wdeg = Y4MWriter(fdeg, hd)
        if vr.ensemble is not None:
            log(f"ensemble: {len(vr.ensemble[2])} forwards per window (ops {vr.ensemble[2]}); what it gains on this network nobody has measured")
        if vr.window_overlap:
            log(f"window overlap: {vr.window_overlap} of {a.one_len} frames shared and cross-faded, {a.one_len / (a.one_len - vr.window_overlap):.2f} times the windows "
                "(a mismatch becomes a ramp, it is not removed)")
        if vr.tile is not None:
            log("tile: %d x %d, overlap %d (a tiled result is not the full-frame result: channel attention sees the tile)" % vr.tile)
        if a.out_format is not None or a.dither != "none":
            log(f"output: C{a.out_format or hd.chroma}{'' if a.out_format else ' (as the input)'}, dither {a.dither}"
                f"{' seed %d' % a.dither_seed if a.dither != 'none' else ''}")
        if vr.mix is not None:
            log("amount: luma %g, chroma %g of the correction (linear in the code domain)" % vr.amount if view is None else
                f"view: removed (input minus result around mid-grey, gain {a.removed_gain:g})")
        wr = Y4MWriter(fout, output_header(hd, a.out_format))
        t0 = time.perf_counter()
        n = 0
        for p in vr.restore(rd, fmt, hd.height, hd.width, gt=gt, degraded=None if wdeg is None else wdeg.write):
            wr.write(p)
            n += 1
            if n % max(a.one_len, 1) == 0:
                log(f"  {n} frames, {time.perf_counter() - t0:.1f} s")
        fout.flush()
        dt = time.perf_counter() - t0
        fwd = vr.stats["forward_s"]
        used = vr.stats.get("cuts", [])
        if vr.stats.get("cuts_ignored"):
            log(f"scene cuts at or beyond the end of the stream ({n} frames) ignored: {vr.stats['cuts_ignored']}")
        _write_out(a.cuts_out, _text_writer(scenes.format_cuts), used)
        log(f"done: {n} frames in {dt:.2f} s, {n / dt if dt > 0 else 0.0:.2f} frames/s end to end, "
            f"{n / fwd if fwd > 0 else 0.0:.2f} frames/s forward only, {len(used) + 1} scene{'s' if used else ''}"
            f"{'' if cuts is None else (' (cuts found)' if cuts == 'auto' else ' (cuts listed)')}")
        if vr.tile is not None:
            wt = vr.stats["window_tiles"]
            log(f"tiles: {min(len(w) for w in wt) if wt else 0} to {max(len(w) for w in wt) if wt else 0} per window, "
                f"{vr.stats['tile_launches']} blended over {len(wt)} window{'' if len(wt) == 1 else 's'}")
        seams = vr.stats.get("seam_rms", [None] * vr.stats["windows"])
        _write_out(a.seams_out, _text_writer(format_seams), seams)
        if vr.window_overlap:
            flat = [v for s in seams if s is not None for v in s]
            log(f"seams: {sum(s is not None for s in seams)} cross-faded over {len(seams)} window{'' if len(seams) == 1 else 's'}"
                f"{', median difference of the two answers %.3f 8-bit codes rms' % float(np.median(flat)) if flat else ''} "
                "(says nothing about a trained network unless the checkpoint is one)")
        wp = vr.stats.get("window_picture", [])
        _write_out(a.picture_out, pic.write_pictures, wp, picture_how)
        if picture is not None:
            kinds = sorted({r for r in wp if r is not None})
            log(f"picture ({picture_how}): {sum(r is not None for r in wp)} of {len(wp)} window{'' if len(wp) == 1 else 's'} restored inside a rectangle"
                f"{': ' + ', '.join('%d:%d:%d:%d' % r for r in kinds[:4]) + (' ...' if len(kinds) > 4 else '') if kinds else ''}")
        ws = vr.stats.get("window_sigma")
        _write_out(a.sigma_out, _text_writer(noise.format_sigmas), ws or [], sigma_how)
        wn = vr.stats.get("window_nlf")
        _write_out(a.noise_model_out, _text_writer(noise.format_curves), wn or [], nlf_how)
        if wn:
            log(f"noise model ({nlf_how}): knots min {min(min(c) for c in wn):.2f} / max {max(max(c) for c in wn):.2f} over {len(wn)} "
                f"window{'' if len(wn) == 1 else 's'}")
        if ws:
            log(f"sigma ({sigma_how}{', ' + a.sigma_estimator if a.sigma_estimator != 'spatial' else ''}{', motion ' + a.sigma_motion if a.sigma_motion != 'none' else ''}{', clamped to [%g, %g]' % tuple(a.sigma_clamp) if sigma_how == 'auto' else ''}): "
                f"min {min(ws):.2f} / median {float(np.median(ws)):.2f} / max {max(ws):.2f} over {len(ws)} window{'' if len(ws) == 1 else 's'}"
                f"{'; injected ' + _injected(vr.add_noise) if vr.add_noise is not None else ''}")
        if vr.deflicker is not None:
            fd = vr.stats["frame_deflicker"]
            _write_out(a.deflicker_out, _text_writer(format_deflicker), fd)
            log(f"deflicker (R {vr.deflicker}, chroma {vr.deflicker_chroma}): rms second difference of the frame means "
                f"{mean_roughness([f[1] for f in fd]):.4f} before, {mean_roughness([f[2] for f in fd]):.4f} after, in luma codes over {len(fd)} "
                f"frame{'' if len(fd) == 1 else 's'} (one curve per frame; unvalidated on real footage)")
        if vr.despot is not None:
            fd = vr.stats["frame_despot"]
            _write_out(a.despot_out, _text_writer(format_despot), fd)
            log(f"despot (T {vr.despot}, K {vr.despot_support}, G {vr.despot_grow}, chroma {vr.despot_chroma}): median share replaced "
                f"{median_share(fd):.6f}, {frames_kept(fd)} frame{'' if frames_kept(fd) == 1 else 's'} kept as they came, over {len(fd)} "
                f"frame{'' if len(fd) == 1 else 's'} (one threshold in codes; unvalidated on real footage)")
        if vr.grain_part is not None:
            wg = vr.stats["window_grain"]
            _write_out(a.grain_out, _text_writer(noise.format_curves), wg, "the grain put back: " + vr.grain_part.how)
            log(f"grain ({vr.grain_part.how}): size {vr.stats['grain_size']:g}, chroma share {vr.stats['grain_chroma']:g}, seed {vr.stats['grain_seed']}, "
                f"median level {float(np.median([k for c in wg for k in c])) if wg else 0.0:.2f} in 8-bit R'G'B' codes over {len(wg)} "
                f"window{'' if len(wg) == 1 else 's'} (a Gaussian field, not a model of the removed noise)")
        if a.report is not None:
            fr = vr.stats["frame_report"]
            _write_out(a.report, _text_writer(rep.format_report), fr, f"edge {a.report_edge:g}", vr.stats.get("frame_report_motion"), vr.stats.get("frame_niqe"),
                       vr.stats.get("frame_fullref"))
            log(f"report (written minus input, medians over {len(fr)} frame{'' if len(fr) == 1 else 's'}, unvalidated on real footage): "
                f"{rep.summary_line(vr.stats['report_summary'])}")
            if report_motion is not None:
                log(f"report along block motion (medians over the pairs inside a window, unvalidated on real footage): "
                    f"{rep.summary_line_motion(vr.stats['report_motion_summary'])}")
            if report_quality is not None:
                log(f"quality (NIQE of the luma, medians over the frames with a score; no verdict, unvalidated on real footage): "
                    f"{rep.summary_line_quality(vr.stats['report_quality_summary'])}")
            if gt is not None or a.add_noise is not None or a.add_blur is not None:
                from .fullref import summary_line_fullref
                log(f"against the ground truth ({a.gt or 'the clean input'}; PSNR in dB, SSIM of the luma; _in the input, _out the frames written; no verdict): "
                    f"{summary_line_fullref(vr.stats['fullref_summary'])}")
    finally:
        if fin is not sys.stdin.buffer:
            fin.close()
        if fout is not sys.stdout.buffer:
            fout.close()
        if fgt is not None:
            fgt.close()
        if fdeg is not None:
            fdeg.close()
    return 0
