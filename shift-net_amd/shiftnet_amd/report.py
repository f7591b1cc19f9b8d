"""Method noise of a run of the video restorer: numbers about what it changed, per written frame (numpy only, no torch).

The classical test of a denoiser is its method noise, input minus output.  If only noise left the picture, that difference is white in space,
independent from frame to frame, no stronger on edges than on flat areas, and as strong as the noise was.  If detail left with it, the difference is
correlated: with its neighbours, with the next frame (static texture is the same in both) and with the edges of the picture.

The sums are what ``sn_yuv_diff_stats`` (csrc/sn_yuv_stats.hip) writes per frame for d = written - input of the luma and of both chroma planes:
``SUMS`` names its 16 integers.  From one row, in float64 on exact integers (so the device's sums and a host restatement give the same floats):

  m = S1 / N;  var = S2 / N - m^2                       luma code units of the format written; the numerator N S2 - S1^2 is formed in integers
  mean_y = m / c;  rms_y = sqrt(S2 / N) / c             c = 2^(bits - 8): in 8-bit code units
  removed_sigma = sqrt(max(var, 0)) / (g s)             g, s of noise.py (``luma_gain``, ``code_scale``): the sigma of i.i.d. noise on 8-bit R'G'B' with
                                                        this much luma variance -- the unit of the restorer's ``sigma``
  rho_x = (Sx / Nx - m^2) / var;  rho_y likewise        the correlation of d with its right and its lower neighbour
  edge_share = Ne / N;  edge_ratio = (S2e / Ne) / ((S2 - S2e) / (N - Ne))        the mean of d^2 on the edge pixels over that on the others
  mean_u, rms_u, mean_v, rms_v                          as mean_y and rms_y, of the chroma planes
  rho_t = (St / N - m_t m_t1) / sqrt(var_t var_t1)      the correlation with the next frame's d (``pair_rho``)

A measure whose denominator is zero is nan.  A noise-only removal reads rho_x ~ rho_y ~ rho_t ~ 0, edge_ratio ~ 1 and removed_sigma ~ the sigma
the window was restored with.  ``removed_sigma`` is not corrected for rounding: the output's rounding to codes adds 1/12 code^2 to var, a TPDF dither
adds its own noise (about 1/4 code^2), and with an ``amount`` below 1 only that share of the correction was written.  **The interpretation is
unvalidated on real footage**: the deblur variants change edges by design; the edge threshold is a guess; at 4:2:0 the luma noise of real footage
need not be white to begin with.

Along block motion (``report_motion="blocks"`` of the restorer): rho_t compares a frame's d with the next frame's AT THE SAME PLACE, so removed detail that
moves with the picture reads rho_t ~ 0 -- what a noise-only removal reads.  ``sn_yuv_diff_stats_mv`` sums d of the pair along the vectors that
``sn_yuv_block_motion`` finds on the WRITTEN frames, on the half of the 2 x 2 blocks the vectors were not chosen on: ``SUMS_MV`` names its 8 integers, and
``pair_measures_mv`` makes of one row

  rho_t_mv = (Nm S01 - S0 S1) / sqrt((Nm S00 - S0^2) (Nm S11 - S1^2))      the correlation of d with the next frame's d where the vector points
  mv_match_rms = sqrt(Sgg / Nm) / c                     how well the vectors fit the written picture, in 8-bit code units
  mv_moved = Nv / Nm                                    the share of the counted samples whose vector is not (0, 0)
  mv_counted = Nm / (h w)                               the share of the picture's samples that were counted (at most about one half)

Its limits: integer-pel vectors within +-7 samples, one per 16 x 16 block; half of the samples; a block at the border whose true vector points outside
the picture has another vector or none, so a pan reads well below 1 even where everything removed was detail; pairs across window boundaries have no
value; zoom, rotation and occlusion still read as uncorrelated.  No threshold, no verdict, and as unvalidated on real footage as the rest.

``format_report`` / ``parse_report`` / ``parse_report_motion`` are the file of one line per written frame.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, fields
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .noise import code_scale, luma_gain

SUMS = ("N", "S1", "S2", "Nx", "Sx", "Ny", "Sy", "St", "Ne", "S2e", "Nc", "Su", "Su2", "Sv", "Sv2", "zero")      # the 16 words of sn_yuv_diff_stats
SUMS_MV = ("Nm", "S0", "S00", "S1", "S11", "S01", "Sgg", "Nv")                  # the 8 words of sn_yuv_diff_stats_mv
NAN = float("nan")


def _same(a, b) -> bool:
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


@dataclass(eq=False)
class FrameReport:
    """One written frame: where it was (``frame`` in the stream, ``window`` in the order restored), the sigma its window was restored with (None: a
    deblur variant) and the measures of the module's docstring.  Equality takes nan for equal to nan: two reports of the same sums are equal."""
    frame: int = 0
    window: int = 0
    sigma: Optional[float] = None
    m: float = NAN
    var: float = NAN
    removed_sigma: float = NAN
    mean_y: float = NAN
    rms_y: float = NAN
    rho_x: float = NAN
    rho_y: float = NAN
    edge_share: float = NAN
    edge_ratio: float = NAN
    mean_u: float = NAN
    rms_u: float = NAN
    mean_v: float = NAN
    rms_v: float = NAN
    rho_t: float = NAN

    def __eq__(self, other) -> bool:
        if not isinstance(other, FrameReport):
            return NotImplemented
        return all(_same(getattr(self, f.name), getattr(other, f.name)) for f in fields(self))

    __hash__ = None


COLUMNS = tuple(f.name for f in fields(FrameReport))
MEASURES = COLUMNS[3:]                                        # every float column


def _ratio(num: int, den: int) -> float:
    """num / den of two integers, correctly rounded; nan for den == 0."""
    return num / den if den else NAN


def _ints(sums) -> List[int]:
    s = [int(v) for v in np.asarray(sums).reshape(-1)]
    if len(s) != len(SUMS):
        raise ValueError(f"a row of sn_yuv_diff_stats has {len(SUMS)} words, got {len(s)}")
    return s


def frame_measures(sums, bits: int, matrix: int, range_: int) -> FrameReport:
    """One row of ``sn_yuv_diff_stats`` (the format written: ``bits``, ``matrix``, ``range_``) -> a FrameReport with frame 0, window 0, no sigma and
    no rho_t.  ``removed_sigma`` is uncorrected: the output's rounding adds 1/12 code^2 to the variance and a TPDF dither its own noise."""
    N, S1, S2, Nx, Sx, Ny, Sy, _, Ne, S2e, Nc, Su, Su2, Sv, Sv2, _ = _ints(sums)
    c = float(1 << (bits - 8))
    r = FrameReport()
    r.m, r.var = _ratio(S1, N), _ratio(N * S2 - S1 * S1, N * N)
    r.mean_y, r.rms_y = r.m / c, math.sqrt(_ratio(S2, N)) / c if N else NAN
    r.removed_sigma = math.sqrt(max(r.var, 0.0)) / (luma_gain(matrix) * code_scale(bits, range_)) if N else NAN
    vnum = N * S2 - S1 * S1                                   # var = vnum / N^2, cov_x = (Sx N^2 - S1^2 Nx) / (Nx N^2): rho_x = that / var
    r.rho_x = _ratio(Sx * N * N - S1 * S1 * Nx, Nx * vnum)
    r.rho_y = _ratio(Sy * N * N - S1 * S1 * Ny, Ny * vnum)
    r.edge_share = _ratio(Ne, N)
    r.edge_ratio = _ratio(S2e * (N - Ne), Ne * (S2 - S2e))
    r.mean_u, r.mean_v = _ratio(Su, Nc) / c, _ratio(Sv, Nc) / c
    r.rms_u, r.rms_v = (math.sqrt(_ratio(Su2, Nc)) / c, math.sqrt(_ratio(Sv2, Nc)) / c) if Nc else (NAN, NAN)
    return r


def pair_rho(sums_t, sums_t1) -> float:
    """The correlation of a frame's d with the next frame's: both rows of one launch, so that ``sums_t`` holds St.  nan when there is no next frame
    (None), the two are of different pictures, or either has no variance."""
    if sums_t is None or sums_t1 is None:
        return NAN
    a, b = _ints(sums_t), _ints(sums_t1)
    N = a[0]
    if N == 0 or b[0] != N:
        return NAN
    va, vb = N * a[2] - a[1] * a[1], N * b[2] - b[1] * b[1]   # N^2 var of each
    if va <= 0 or vb <= 0:
        return NAN
    return (a[7] * N - a[1] * b[1]) / math.sqrt(va * vb)      # (St / N - m_t m_t1) / sqrt(var_t var_t1), the N^2 cancelled


def frames_report(frame_sums: Sequence, windows: Sequence[int], sigmas: Sequence[Optional[float]], bits: int, matrix: int, range_: int
                  ) -> List[FrameReport]:
    """The report of a run: ``frame_sums[i]`` is the row of written frame i, ``windows[i]`` the window it was restored in and ``sigmas[i]`` that
    window's sigma (None: none).  rho_t of a frame is ``pair_rho`` with the next frame where that one lies in the same window -- its St was summed
    in the same launch -- and nan elsewhere."""
    out = []
    n = len(frame_sums)
    for i in range(n):
        r = frame_measures(frame_sums[i], bits, matrix, range_)
        r.frame, r.window, r.sigma = i, int(windows[i]), (None if sigmas[i] is None else float(sigmas[i]))
        r.rho_t = pair_rho(frame_sums[i], frame_sums[i + 1]) if i + 1 < n and windows[i + 1] == windows[i] else NAN
        out.append(r)
    return out


@dataclass(eq=False)
class MotionReport:
    """The motion part of one written frame's report: the measures of ``pair_measures_mv`` for the pair (frame, frame + 1) where both lie in one
    window, nan elsewhere -- exactly where ``rho_t`` has a value.  Equality takes nan for equal to nan."""
    rho_t_mv: float = NAN
    mv_match_rms: float = NAN
    mv_moved: float = NAN
    mv_counted: float = NAN

    def __eq__(self, other) -> bool:
        if not isinstance(other, MotionReport):
            return NotImplemented
        return all(_same(getattr(self, f.name), getattr(other, f.name)) for f in fields(self))

    __hash__ = None


COLUMNS_MV = tuple(f.name for f in fields(MotionReport))
COLUMNS_F = ("psnr_y_in", "psnr_y_out", "psnr_u_in", "psnr_u_out", "psnr_v_in", "psnr_v_out", "ssim_in", "ssim_out")      # gt: fullref.FIELDS, against the truth
COLUMNS_Q = ("niqe_in", "niqe_out")                           # report_quality="niqe": the score of the input and of the written frame (shiftnet_amd/niqe.py)


def pair_measures_mv(sums, bits: int, h: int, w: int) -> MotionReport:
    """One row of ``sn_yuv_diff_stats_mv`` (the format written has ``bits``; the picture is h x w) -> the four measures, float64 expressions of the exact
    integers.  None (no pair) -> all nan.  rho_t_mv is nan if nothing was counted or either frame's d has no variance on the counted samples; the
    other three are nan if nothing was counted (mv_counted: 0.0 then, nan only for an empty picture)."""
    if sums is None:
        return MotionReport()
    s = [int(v) for v in np.asarray(sums).reshape(-1)]
    if len(s) != len(SUMS_MV):
        raise ValueError(f"a row of sn_yuv_diff_stats_mv has {len(SUMS_MV)} words, got {len(s)}")
    Nm, S0, S00, S1, S11, S01, Sgg, Nv = s
    r = MotionReport()
    r.mv_counted = _ratio(Nm, int(h) * int(w))
    if Nm == 0:
        return r
    v0, v1 = Nm * S00 - S0 * S0, Nm * S11 - S1 * S1             # Nm^2 var of each
    if v0 > 0 and v1 > 0:
        r.rho_t_mv = (Nm * S01 - S0 * S1) / math.sqrt(v0 * v1)
    r.mv_match_rms = math.sqrt(Sgg / Nm) / float(1 << (bits - 8))
    r.mv_moved = Nv / Nm
    return r


def frames_report_motion(pair_sums: Sequence, bits: int, sizes: Sequence[Tuple[int, int]]) -> List[MotionReport]:
    """The motion part of a run's report: ``pair_sums[i]`` is the row of the pair (written frame i, i + 1), or None where the two lie in different
    windows or i is the last frame; ``sizes[i]`` the (h, w) of the picture frame i's window was restored in."""
    return [pair_measures_mv(s, bits, *sizes[i]) for i, s in enumerate(pair_sums)]


def summarize_motion(motion: Iterable[MotionReport]) -> Dict[str, float]:
    """The median of every motion measure over the frames that have one (nan where none has)."""
    motion = list(motion)
    out = {}
    for name in COLUMNS_MV:
        v = [x for x in (getattr(m, name) for m in motion) if not math.isnan(x)]
        out[name] = float(np.median(v)) if v else NAN
    return out


def summary_line_motion(summary: Dict[str, float]) -> str:
    """The four motion medians, for a log."""
    return ", ".join(f"{k} {summary[k]:.3f}" for k in COLUMNS_MV)


def summarize(frames: Iterable[FrameReport]) -> Dict[str, float]:
    """The median of every measure over the frames that have one (nan where none has)."""
    frames = list(frames)
    out = {}
    for name in MEASURES:
        v = [getattr(f, name) for f in frames]
        v = [x for x in v if not math.isnan(x)]
        out[name] = float(np.median(v)) if v else NAN
    return out


def summary_line(summary: Dict[str, float]) -> str:
    """The medians a reader looks at first, for a log."""
    return ", ".join(f"{k} {summary[k]:.3f}" for k in ("removed_sigma", "rho_x", "rho_y", "rho_t", "edge_ratio", "edge_share"))


def _word(v) -> str:
    if v is None:
        return "-"
    return repr(float(v)) if isinstance(v, float) else str(int(v))     # repr of a float reads back to the same float; nan reads back as nan


def summarize_quality(pairs: Iterable) -> Dict[str, float]:
    """The medians of the (niqe_in, niqe_out) pairs of the written frames, each over the frames that have a number (nan where none has)."""
    pairs = list(pairs)
    out = {}
    for i, name in enumerate(COLUMNS_Q):
        v = [float(p[i]) for p in pairs if not math.isnan(p[i])]
        out[name] = float(np.median(v)) if v else NAN
    return out


def summary_line_quality(summary: Dict[str, float]) -> str:
    """Both medians, for a log."""
    return ", ".join(f"{k} {summary[k]:.3f}" for k in COLUMNS_Q)


def format_report(frames: Iterable[FrameReport], how: str = "", motion: Optional[Iterable[MotionReport]] = None, quality: Optional[Iterable] = None,
                  fullref: Optional[Iterable] = None) -> str:
    """The report file: '#' header lines that name the columns, one line per written frame (sigma '-' where the window had none), and the medians of
    ``summarize`` as the last line, '# median'.  Floats are written so that ``parse_report`` reads back equal reports.  ``motion``: one MotionReport
    per frame; every line, the median line and the '#' column line then gain its four columns (``parse_report_motion`` reads them back).  ``quality``:
    one (niqe_in, niqe_out) per frame; they gain those two columns (``parse_report_quality``).  ``fullref``: one fullref.FullRef per frame (``gt``); they
    gain its eight columns, after all others (``parse_report_fullref``), ``inf`` where a plane equals the truth's.  Without any of them the text is what
    it was before there was such a part."""
    frames = list(frames)
    med = summarize(frames)
    lines = ["# method noise: written minus input, one line per written frame" + (f" ({how})" if how else ""),
             "# m, var: luma codes of the format written; sigma, removed_sigma: 8-bit R'G'B' codes; mean_*, rms_*: 8-bit codes; rho_t: to the next frame"]
    cols = list(COLUMNS)
    rows = [[_word(getattr(f, c)) for c in COLUMNS] for f in frames]
    meds = [_word(med[c]) for c in MEASURES]
    if motion is not None:
        motion = list(motion)
        if len(motion) != len(frames):
            raise ValueError(f"{len(frames)} frames and {len(motion)} motion reports")
        mmed = summarize_motion(motion)
        lines.append("# rho_t_mv: to the next frame along block motion vectors of the written picture (measuring blocks only); mv_match_rms: 8-bit codes; "
                     "mv_moved, mv_counted: shares")
        cols += COLUMNS_MV
        for r, m in zip(rows, motion):
            r += [_word(getattr(m, c)) for c in COLUMNS_MV]
        meds += [_word(mmed[c]) for c in COLUMNS_MV]
    if quality is not None:
        quality = [(float(a), float(b)) for a, b in quality]
        if len(quality) != len(frames):
            raise ValueError(f"{len(frames)} frames and {len(quality)} quality pairs")
        qmed = summarize_quality(quality)
        lines.append("# niqe_in, niqe_out: NIQE of the luma of the input and of the written frame (no reference; lower is nearer to natural pictures; nan: "
                     "fewer than two 96 x 96 blocks could be fitted)")
        cols += COLUMNS_Q
        for r, q in zip(rows, quality):
            r += [_word(q[0]), _word(q[1])]
        meds += [_word(qmed[c]) for c in COLUMNS_Q]
    if fullref is not None:
        from .fullref import summarize_fullref
        fullref = [tuple(float(v) for v in f) for f in fullref]
        if len(fullref) != len(frames) or any(len(f) != len(COLUMNS_F) for f in fullref):
            raise ValueError(f"{len(frames)} frames and {len(fullref)} full-reference rows of {len(COLUMNS_F)} numbers")
        fmed = summarize_fullref(fullref)["median"]
        lines.append("# psnr_*_in, psnr_*_out: dB, of the input (as written) and of the written frame against the ground truth, p = 2^bits - 1 (inf: the planes "
                     "are equal); ssim_in, ssim_out: SSIM of the luma codes, 11 x 11 Gaussian window, replicated border")
        cols += COLUMNS_F
        for r, f in zip(rows, fullref):
            r += [_word(v) for v in f]
        meds += [_word(fmed[c]) for c in COLUMNS_F]
    lines.append("# " + " ".join(cols))
    lines += [" ".join(r) for r in rows]
    lines.append("# median - - - " + " ".join(meds))
    return "\n".join(lines) + "\n"


def _parse(text: str):
    """(FrameReport, MotionReport or None, (niqe_in, niqe_out) or None, the eight numbers of fullref.FullRef or None) of every line of a report file; a
    line has the columns of a frame, or those and the four of its motion part ('#' lines are comments, the medians among them: ``summarize`` makes them
    again).  Where the '#' line that names the columns ends in the eight names of COLUMNS_F every line has those columns more, last; where what stands
    before them (or the line, without them) ends in ``niqe_in niqe_out``, those two more; a file without either is read as it always was."""
    out = []
    nf, nm, nq, nF = len(COLUMNS), len(COLUMNS_MV), len(COLUMNS_Q), len(COLUMNS_F)
    named = [line.split()[1:] for line in text.splitlines() if line.startswith("# " + COLUMNS[0] + " ")]
    f = nF if any(tuple(n[-nF:]) == COLUMNS_F for n in named) else 0
    q = nq if any(tuple(n[len(n) - f - nq:len(n) - f]) == COLUMNS_Q for n in named) else 0
    widths = (nf + q + f, nf + nm + q + f)
    for ln, line in enumerate(text.splitlines(), 1):
        body = line.split("#", 1)[0].split()
        if not body:
            continue
        if len(body) not in widths:
            raise ValueError(f"line {ln}: {widths[0]} or {widths[1]} columns expected, got {len(body)}")
        try:
            vals = [int(body[0]), int(body[1]), None if body[2] == "-" else float(body[2])] + [float(w) for w in body[3:]]
        except ValueError:
            raise ValueError(f"line {ln}: not a report line: {line!r}") from None
        full = tuple(vals[len(vals) - f:]) if f else None
        vals = vals[:len(vals) - f]
        rest = vals[nf:len(vals) - q]
        out.append((FrameReport(*vals[:nf]), MotionReport(*rest) if rest else None, tuple(vals[-q:]) if q else None, full))
    return out


def parse_report(text: str) -> List[FrameReport]:
    """The frames of a report file, with or without a motion part."""
    return [f for f, _, _, _ in _parse(text)]


def parse_report_motion(text: str) -> List[Optional[MotionReport]]:
    """The motion part of every line of a report file; None for a line without one."""
    return [m for _, m, _, _ in _parse(text)]


def parse_report_quality(text: str) -> List[Optional[tuple]]:
    """The (niqe_in, niqe_out) of every line of a report file; None for a line without them."""
    return [q for _, _, q, _ in _parse(text)]


def parse_report_fullref(text: str) -> List[Optional[tuple]]:
    """The fullref.FullRef of every line of a report file; None for a line without its eight columns."""
    from .fullref import FullRef
    return [None if f is None else FullRef(*f) for _, _, _, f in _parse(text)]
