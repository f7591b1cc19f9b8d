"""The index map of sn_geo_transform / sn_geo_accumulate (include/shiftnet_hip.h, csrc/sn_geo.hip) restated in numpy, sample by sample through index
arrays and with no flip or transpose call of numpy's: the kernels equal these bit for bit.  ``op``: bit 1 mirrors the columns, 2 the rows, 4 transposes
(before the flips), 8 reverses time."""
import numpy as np

FLIP_X, FLIP_Y, TRANSPOSE, REVERSE_T = 1, 2, 4, 8


def out_shape(shape, op):
    T, C, H, W = shape
    return (T, C, W, H) if op & TRANSPOSE else (T, C, H, W)


def index_map(shape, op):
    """For the plain tensor's ``shape`` [T, C, H, W]: index arrays (t, y, x), each of the transformed tensor's [T, H', W'], that say which plain sample
    (t, c, y, x) belongs to the transformed sample (t', c, y', x') -- the five steps of the header, in its order."""
    T, C, H, W = shape
    Hp, Wp = out_shape(shape, op)[2:]
    tp, yp, xp = np.meshgrid(np.arange(T), np.arange(Hp), np.arange(Wp), indexing="ij")
    u, v = yp, xp                                      # 1
    if op & FLIP_Y:
        u = Hp - 1 - u                                 # 2
    if op & FLIP_X:
        v = Wp - 1 - v                                 # 3
    y, x = (v, u) if op & TRANSPOSE else (u, v)        # 4
    t = T - 1 - tp if op & REVERSE_T else tp           # 5
    return t, y, x


def transform(a, op):
    """a: [T, C, H, W] of any dtype -> dst [T, C, H', W'] with dst[t'][c][y'][x'] = a[t][c][y][x]."""
    assert a.ndim == 4 and 0 <= op <= 15
    t, y, x = index_map(a.shape, op)
    return np.ascontiguousarray(a[t[:, None], np.arange(a.shape[1])[None, :, None, None], y[:, None], x[:, None]])


def accumulate(canvas, member, op, init, scale):
    """canvas: [T, C, H, W] float32, changed in place and returned; member: float32 of out_shape.  a = member if init else canvas + member (one float32
    sum, rounded); canvas = a * scale (one float32 product, rounded).  With init the canvas is not read."""
    assert canvas.dtype == np.float32 and member.dtype == np.float32 and member.shape == out_shape(canvas.shape, op)
    t, y, x = index_map(canvas.shape, op)
    c = np.arange(canvas.shape[1])[None, :, None, None]
    idx = (t[:, None], c, y[:, None], x[:, None])      # a bijection onto the canvas: every sample is written once
    with np.errstate(all="ignore"):
        a = member if init else (canvas[idx] + member).astype(np.float32)
        canvas[idx] = (a * np.float32(scale)).astype(np.float32)
    return canvas
