"""The tiles of the video restorer restated in numpy, for tests/test_host_tiles.py and tests/test_gpu_tiles.py: the plan of one axis written out
position by position (shiftnet_amd/windows.py: tile_axis vectorises it), and the blend ``sn_tile_accumulate`` makes (include/shiftnet_hip.h), every
product and sum rounded to float32 on its own -- numpy's float32 array operations round each result once, and fuse nothing."""
import math

import numpy as np


def origins(L, S, V):
    """The tile origins of an axis of length L for tiles of side S that overlap by at least V."""
    if S >= L:
        return [0]
    step = S - V
    n = math.ceil((L - S) / step) + 1
    return [min(k * step, L - S) for k in range(n)]


def ramp(k, n, o, S, p):
    """t_k(p): the distance to the tile's edges that face a neighbour, counted from 1; a lone tile has 1 everywhere."""
    cands = []
    if k > 0:
        cands.append(p - o + 1)
    if k < n - 1:
        cands.append(o + S - p)
    return min(cands) if cands else 1


def weights64(L, S, V):
    """float64 [n][min(S, L)]: tile k's weight at its own position q (the axis position o_k + q)."""
    os_ = origins(L, S, V)
    n, side = len(os_), min(S, L)
    w = np.zeros((n, side), dtype=np.float64)
    for k, o in enumerate(os_):
        for q in range(side):
            p = o + q
            total = sum(ramp(j, n, oj, side, p) for j, oj in enumerate(os_) if oj <= p < oj + side)
            w[k, q] = ramp(k, n, o, side, p) / total
    return w


def cover(L, S, V):
    """Per axis position, the list of tiles that cover it."""
    os_ = origins(L, S, V)
    side = min(S, L)
    return [[k for k, o in enumerate(os_) if o <= p < o + side] for p in range(L)]


def accumulate(canvas, tile, wy, wx, y0, x0):
    """canvas [T, C, Hc, Wc] float32, changed in place and returned: its th x tw rectangle at (y0, x0) becomes canvas + (wy[y] * wx[x]) * tile."""
    assert canvas.dtype == tile.dtype == wy.dtype == wx.dtype == np.float32
    th, tw = tile.shape[2], tile.shape[3]
    w = wy[:, None] * wx[None, :]                                  # float32 product, rounded
    prod = w[None, None] * tile                                    # float32 product, rounded
    view = canvas[:, :, y0:y0 + th, x0:x0 + tw]
    view[...] = view + prod                                        # float32 sum, rounded
    assert w.dtype == prod.dtype == np.float32
    return canvas


def blend(results, plan, shape):
    """The canvas of one window: ``results[i]`` is the float32 [n, 3, th, tw] result of ``plan.tiles[i]``, accumulated in order into zeros."""
    canvas = np.zeros(shape, dtype=np.float32)
    nx = len(plan.xs)
    for i, ((y0, x0, th, tw), r) in enumerate(zip(plan.tiles, results)):
        accumulate(canvas, np.ascontiguousarray(r, dtype=np.float32), plan.wy[i // nx], plan.wx[i % nx], y0, x0)
    return canvas
