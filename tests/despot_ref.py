"""The despot rule (``--despot``, include/shiftnet_hip.h: sn_yuv_despot) restated on its own: straightforward numpy on int64 planes, one frame at a
time, every step of the rule a line.  Shares no code with the kernel or the stage it checks; its vectors come from motion_ref.block_motion_ref.

    c = Y_f(y, x); p, n = Y_{f-1}, Y_{f+1} at the places displaced by the vectors of the sample's block (clamped to the plane); a = c - p, b = c - n;
    d = min(|a|, |b|) if a and b have the same sign and neither is 0, else 0; SEED iff d > T + |p - n|, T in 8-bit codes times 2^(bits - 8);
    CORE iff a seed with at least K seeds among its eight neighbours; M = the core seeds dilated by the (2G + 1)^2 square; a sample in M becomes
    (p + n + 1) >> 1; chroma follows the luma or is left alone."""
import numpy as np

import motion_ref as MR
import yuv_ref as R


def _block_vectors(mv, H, W):
    """int8 [nby, nbx, 2] -> (dy, dx) int64 [H, W]: every luma sample the vector of block (min(y / 16, nby - 1), min(x / 16, nbx - 1))."""
    nby, nbx = mv.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    v = np.asarray(mv).astype(np.int64)[np.minimum(y // 16, nby - 1), np.minimum(x // 16, nbx - 1)]
    return v[..., 0], v[..., 1]


def _displaced(P, dy, dx, y, x):
    """P at (y + dy, x + dx), the coordinates clamped to the plane."""
    h, w = P.shape
    return P[np.clip(y + dy, 0, h - 1), np.clip(x + dx, 0, w - 1)]


def _count_around(S):
    """How many of the eight neighbours of every sample are set; outside the picture nothing is."""
    h, w = S.shape
    pad = np.zeros((h + 2, w + 2), np.int64)
    pad[1:-1, 1:-1] = S
    return sum(pad[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)


def _dilate(S, G):
    h, w = S.shape
    pad = np.zeros((h + 2 * G, w + 2 * G), bool)
    pad[G:G + h, G:G + w] = S
    out = np.zeros((h, w), bool)
    for dy in range(2 * G + 1):
        for dx in range(2 * G + 1):
            out |= pad[dy:dy + h, dx:dx + w]
    return out


def despot_frame(prev, cur, nxt, mvp, mvn, fmt, H, W, T, K, G, chroma):
    """Three payloads and the two vector grids of the middle one -> (the middle payload repaired, core seeds, luma samples replaced)."""
    Yp, Up, Vp = R.split_planes(prev, fmt, H, W)
    Yc, Uc, Vc = R.split_planes(cur, fmt, H, W)
    Yn, Un, Vn = R.split_planes(nxt, fmt, H, W)
    if H < 2 or W < 2:                                             # no vector block: no seeds
        return np.array(cur, copy=True), 0, 0
    y, x = np.mgrid[0:H, 0:W]
    dyp, dxp = _block_vectors(mvp, H, W)
    dyn, dxn = _block_vectors(mvn, H, W)
    p, n = _displaced(Yp, dyp, dxp, y, x), _displaced(Yn, dyn, dxn, y, x)
    a, b = Yc - p, Yc - n
    d = np.where(((a > 0) & (b > 0)) | ((a < 0) & (b < 0)), np.minimum(np.abs(a), np.abs(b)), 0)
    seed = d > T * (1 << (fmt.bits - 8)) + np.abs(p - n)
    core = seed & (_count_around(seed.astype(np.int64)) >= K)
    M = _dilate(core, G)
    Y = np.where(M, (p + n + 1) >> 1, Yc)
    U, V = Uc.copy(), Vc.copy()
    if chroma == "follow":
        ch, cw = Uc.shape
        cy, cx = np.mgrid[0:ch, 0:cw]
        if fmt.chroma == R.C444:
            Mc, vy, vx = M, (dyp, dyn), (dxp, dxn)
        else:
            pad = np.zeros((2 * ch, 2 * cw), bool)                 # a luma sample outside the picture is in no mask
            pad[:H, :W] = M
            Mc = pad[0::2, 0::2] | pad[0::2, 1::2] | pad[1::2, 0::2] | pad[1::2, 1::2]
            vy = tuple(v[2 * cy, 2 * cx] >> 1 for v in (dyp, dyn))    # of luma sample (2 cy, 2 cx), halved with an arithmetic shift
            vx = tuple(v[2 * cy, 2 * cx] >> 1 for v in (dxp, dxn))
        U = np.where(Mc, (_displaced(Up, vy[0], vx[0], cy, cx) + _displaced(Un, vy[1], vx[1], cy, cx) + 1) >> 1, Uc)
        V = np.where(Mc, (_displaced(Vp, vy[0], vx[0], cy, cx) + _displaced(Vn, vy[1], vx[1], cy, cx) + 1) >> 1, Vc)
    else:
        assert chroma == "off"
    return R.join_planes(Y, U, V, fmt), int(core.sum()), int(M.sum())


def despot_ref(payloads, mv_prev, mv_next, fmt, H, W, f0, n, T, K, G, chroma):
    """payloads: uint8 [S, frame_bytes]; mv_prev, mv_next: int8 [S - 1, nby, nbx, 2] (mv_next[f]: frame f into f + 1; mv_prev[f - 1]: frame f into
    f - 1) -> (uint8 [n, frame_bytes]: frames f0 .. f0 + n - 1 repaired from the originals, uint32 [n, 2]: core seeds and luma samples replaced)."""
    S = len(payloads)
    assert f0 >= 1 and n >= 1 and f0 + n <= S - 1
    out, counts = [], []
    for f in range(f0, f0 + n):
        q, seeds, replaced = despot_frame(payloads[f - 1], payloads[f], payloads[f + 1], mv_prev[f - 1], mv_next[f], fmt, H, W, T, K, G, chroma)
        out.append(q)
        counts.append((seeds, replaced))
    return np.stack(out), np.array(counts, dtype=np.uint32).reshape(n, 2)


def vectors_ref(payloads, fmt, H, W):
    """(mv_prev, mv_next) of a stack of at least two payloads: the matcher on the time-reversed stack, flipped back, and on the stack."""
    stack = np.stack(list(payloads))
    return MR.block_motion_ref(stack[::-1], fmt, H, W)[0][::-1], MR.block_motion_ref(stack, fmt, H, W)[0]


def despot_stream_ref(payloads, fmt, H, W, cuts=(), T=24, K=2, G=1, chroma="follow", max_share=0.05, chunk=None):
    """The whole stage on a stream: -> (the payloads handed on, [(seeds, replaced, share, kept)] per frame).  Every scene of the LISTED ``cuts`` is a
    clip of its own; a clip's first and last frame leave as they came with the record (0, 0, 0.0, False); a frame whose replaced share exceeds
    ``max_share`` is handed on as the ORIGINAL and marked kept.  ``chunk``: walk every clip in pieces of that many frames, each from the original
    frames around it -- the result does not depend on it."""
    pay = [np.asarray(p) for p in payloads]
    starts = [0] + [c for c in cuts if c < len(pay)] + [len(pay)]
    out, rec = [], []
    for lo, hi in zip(starts[:-1], starts[1:]):
        for f in range(lo, hi):
            out.append(pay[f].copy())
            rec.append((0, 0, 0.0, False))
        step = chunk or max(hi - lo, 1)
        for a in range(lo + 1, hi - 1, step):                       # the frames with two neighbours in the clip
            b = min(a + step, hi - 1)
            stack = np.stack(pay[a - 1:b + 1])
            mvp, mvn = vectors_ref(stack, fmt, H, W)
            got, counts = despot_ref(stack, mvp, mvn, fmt, H, W, 1, b - a, T, K, G, chroma)
            for i, f in enumerate(range(a, b)):
                seeds, replaced = int(counts[i, 0]), int(counts[i, 1])
                share = replaced / (H * W)
                kept = share > max_share
                if not kept:
                    out[f] = got[i]
                rec[f] = (seeds, replaced, share, kept)
    return out, rec
