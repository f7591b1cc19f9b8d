"""The deflicker rule (shiftnet_amd/deflicker.py, ``--deflicker``) restated on its own: plain loops over frames, neighbours and codes, Python
integers for every numerator and denominator, one float division, a sorted median, floor(x + 0.5).  Shares no code with the module it checks.
Also the numpy side of the kernels: the luma histogram of payloads and the application of tables to them."""
import math

import numpy as np

import yuv_ref as R


def tables_ref(hists, lo, hi, radius, bits, full_range, chroma="gain"):
    """hists: [S][2^bits] counts -> ([[lutY, lutC]] and [(r, mean_in, mean_out, chroma_gain)]) of frames lo .. hi - 1, the clip."""
    L = 1 << bits
    H = [[int(v) for v in row] for row in hists]
    run = []                                                       # running sums
    for row in H:
        acc, c = [], 0
        for v in row:
            c += v
            acc.append(c)
        run.append(acc)
    yo = 0 if full_range else 16 << (bits - 8)
    co = 128 << (bits - 8)
    luts, info = [], []
    for t in range(lo, hi):
        r = min(radius, t - lo, hi - 1 - t)
        h, C = H[t], run[t]
        n = C[L - 1]
        lut_y = [None] * L
        at = {s: 0 for s in range(t - r, t + r + 1)}               # a grows with c, so every neighbour's k only moves up: the search resumes where it stood
        for c in range(L):
            if h[c] == 0:
                continue
            a = (C[c - 1] if c else 0) + C[c]
            qs = []
            for s in range(t - r, t + r + 1):
                k = at[s]
                while 2 * run[s][k] < a:
                    k += 1
                at[s] = k
                num = (2 * k - 1) * H[s][k] + a - 2 * (run[s][k - 1] if k else 0)
                den = 2 * H[s][k]
                qs.append(num / den)                               # Python's int / int: the correctly rounded quotient
            qs.sort()
            lut_y[c] = min(max(math.floor(qs[r] + 0.5), 0), L - 1)
        present = [c for c in range(L) if h[c]]
        for c in range(L):
            if lut_y[c] is None:
                below = [p for p in present if p < c]
                lut_y[c] = lut_y[below[-1]] if below else lut_y[present[0]]
        m_in = sum(c * h[c] for c in range(L)) / n
        m_out = sum(lut_y[c] * h[c] for c in range(L)) / n
        k = 1.0
        if chroma == "gain" and m_in - yo >= 1 and any(lut_y[c] != c for c in present):
            k = min(max((m_out - yo) / (m_in - yo), 0.5), 2.0)
        lut_c = [min(max(math.floor(co + k * (c - co) + 0.5), 0), L - 1) for c in range(L)] if chroma == "gain" else list(range(L))
        luts.append([lut_y, lut_c])
        info.append((r, m_in, m_out, k))
    return np.array(luts, dtype=np.uint16), info


def luma_of(payload, fmt, h, w):
    """The luma plane of one payload as integers, [h][w]."""
    return np.asarray(R.split_planes(payload, fmt, h, w)[0]).astype(np.int64)


def hist_ref(payloads, fmt, h, w, rect=None):
    """[T][2^bits] int64: np.bincount of min(code, L - 1) over the luma of every payload, or of the rectangle (x0, y0, w, h)."""
    L = 1 << fmt.bits
    out = []
    for p in payloads:
        Y = luma_of(p, fmt, h, w)
        if rect is not None:
            x0, y0, rw, rh = rect
            Y = Y[y0:y0 + rh, x0:x0 + rw]
        out.append(np.bincount(np.minimum(Y, L - 1).ravel(), minlength=L))
    return np.stack(out)


def apply_ref(payloads, luts, fmt, h, w, rect=None):
    """payloads [T][frame_bytes] uint8, luts [T][2][2^bits] -> the payloads with lut[t][plane ? 1 : 0][min(code, L - 1)] in place of every code, inside
    the rectangle (x0, y0, w, h) of the luma -- and its chroma -- or everywhere."""
    L = 1 << fmt.bits
    sub = fmt.chroma != R.C444
    out = []
    for p, lut in zip(payloads, luts):
        lut = np.asarray(lut).astype(np.int64)
        Y, U, V = (np.asarray(a).astype(np.int64).copy() for a in R.split_planes(p, fmt, h, w))
        if rect is None:
            ys, xs = slice(None), slice(None)
            cys, cxs = ys, xs
        else:
            x0, y0, rw, rh = rect
            ys, xs = slice(y0, y0 + rh), slice(x0, x0 + rw)
            cys, cxs = (slice(y0 >> 1, (y0 + rh + 1) >> 1), slice(x0 >> 1, (x0 + rw + 1) >> 1)) if sub else (ys, xs)
        Y[ys, xs] = lut[0][np.minimum(Y[ys, xs], L - 1)]
        U[cys, cxs] = lut[1][np.minimum(U[cys, cxs], L - 1)]
        V[cys, cxs] = lut[1][np.minimum(V[cys, cxs], L - 1)]
        out.append(R.join_planes(Y, U, V, fmt))
    return np.stack(out)


def roughness(means):
    """The rms of m[t - 1] - 2 m[t] + m[t + 1]."""
    d = [means[i - 1] - 2.0 * means[i] + means[i + 1] for i in range(1, len(means) - 1)]
    return math.sqrt(sum(v * v for v in d) / len(d))
