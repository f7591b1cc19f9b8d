"""-m gpu: ``sn_yuv_grain`` (csrc/sn_grain.hip) against its numpy restatement (tests/grain_ref.py), which knows no tiles, byte for byte; and the paths
that must give the same bytes: in place, a rectangle, unaligned payloads, one launch or several.  Payloads of random codes over the whole sample
range, illegal ones included: both clamps and both ends of the curve take part.

Shapes (H x W): 38 x 270 crosses two tiles across and three down, has a width that is no multiple of 8 and a tile seam inside the picture; 37 x 269
is odd both ways, so 4:2:0 blocks are clamped; 16 x 256 is exactly one tile; 2 x 3 is the smallest."""
import itertools

import numpy as np
import pytest
import torch

import grain_ref as GR
import yuv_ref as R
from shiftnet_amd import degrade, grain
from shiftnet_amd.io_edges import grain_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

FORMATS = [R.Fmt(8, R.C444, R.BT601, R.FULL), R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED), R.Fmt(8, R.C420_LEFT, R.BT601, R.LIMITED),
           R.Fmt(8, R.C420_LEFT, R.BT709, R.FULL), R.Fmt(10, R.C444, R.BT709, R.LIMITED), R.Fmt(10, R.C420_CENTER, R.BT601, R.FULL),
           R.Fmt(10, R.C420_LEFT, R.BT709, R.FULL), R.Fmt(10, R.C420_LEFT, R.BT601, R.LIMITED)]
SHAPES = [(38, 270), (37, 269), (16, 256), (2, 3)]
T, T0, SEED = 3, 5, 12345
WHITE, SIZED = grain.grain_taps(0.0), grain.grain_taps(0.8)
ids = dict(ids=lambda f: "%d-%d-%d-%d" % f)


def codes(fmt, H, W, seed=0, t=T):
    """uint8 [t, frame_bytes]: random codes over the whole range of a sample."""
    n = R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)
    a = np.random.default_rng(seed).integers(0, 1 << fmt.bits, (t, n))
    return a.astype("<u2").view(np.uint8).reshape(t, -1) if fmt.bits == 10 else a.astype(np.uint8)


@pytest.fixture(scope="module")
def gauss():
    return torch.from_numpy(degrade.gauss_table().copy()).cuda()


def on_device(src, fmt, H, W, knots, taps, chroma, gauss, seed=SEED, t0=T0, **kw):
    return grain_yuv(torch.from_numpy(src).cuda(), yuv_fmt(*fmt), H, W, knots, taps, chroma, seed, t0, gauss, **kw).cpu().numpy()


@pytest.mark.parametrize("fmt", FORMATS, **ids)
def test_the_kernel_is_the_numpy_restatement_byte_for_byte(fmt, gauss):
    for H, W in SHAPES:
        src = codes(fmt, H, W, seed=H * 1000 + W)
        for taps, chroma in itertools.product((WHITE, SIZED), (0.0, 0.5)):
            got = on_device(src, fmt, H, W, GR.BUMPY, taps, chroma, gauss)
            want = GR.grain_ref(src, fmt, H, W, GR.BUMPY, taps, chroma, SEED, T0)
            assert got.shape == want.shape == src.shape
            assert np.array_equal(got, want), (H, W, taps, chroma, int(np.sum(got != want)))
            assert not np.array_equal(got, src)
        # all knots 0: the input byte for byte, illegal codes included, on the general path too
        assert np.array_equal(on_device(src, fmt, H, W, [0.0] * 16, SIZED, 0.5, gauss), src)


@pytest.mark.parametrize("fmt", FORMATS, **ids)
def test_in_place_and_a_rectangle_give_the_same_bytes(fmt, gauss):
    f = yuv_fmt(*fmt)
    H, W = 38, 270
    src = codes(fmt, H, W, seed=9)
    want = GR.grain_ref(src, fmt, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0)
    d = torch.from_numpy(src).cuda()
    assert grain_yuv(d, f, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0, gauss, out=d) is d and np.array_equal(d.cpu().numpy(), want)
    # chroma share 0 in place: the chroma planes are not touched; out of place: they are copied
    d = torch.from_numpy(src).cuda()
    grain_yuv(d, f, H, W, GR.BUMPY, SIZED, 0.0, SEED, T0, gauss, out=d)
    luma_only = GR.grain_ref(src, fmt, H, W, GR.BUMPY, SIZED, 0.0, SEED, T0)
    assert np.array_equal(d.cpu().numpy(), luma_only) and np.array_equal(on_device(src, fmt, H, W, GR.BUMPY, SIZED, 0.0, gauss), luma_only)
    # a rectangle, not tile-aligned, with a tile seam inside: even origin at 4:2:0, odd at 4:4:4; only its samples are written
    rect = (5, 3, 263, 33) if fmt.chroma == R.C444 else (6, 4, 262, 30)
    for taps in (WHITE, SIZED):
        boxed = GR.grain_ref(src, fmt, H, W, GR.BUMPY, taps, 0.5, SEED, T0, rect=rect)
        d = torch.from_numpy(src).cuda()
        grain_yuv(d, f, H, W, GR.BUMPY, taps, 0.5, SEED, T0, gauss, rect=rect, out=d)
        assert np.array_equal(d.cpu().numpy(), boxed)
        other = codes(fmt, H, W, seed=10)                              # out of place: what lies outside the rectangle in dst stays dst's
        o = torch.from_numpy(other).cuda()
        grain_yuv(torch.from_numpy(src).cuda(), f, H, W, GR.BUMPY, taps, 0.5, SEED, T0, gauss, rect=rect, out=o)
        got, x0, y0, w, h = o.cpu().numpy(), *rect
        for t in range(T):
            pg, pb, po = (R.split_planes(a[t], fmt, H, W) for a in (got, boxed, other))
            sub = fmt.chroma != R.C444
            for k, (g, b, q) in enumerate(zip(pg, pb, po)):
                ys, xs = (slice(y0 >> 1, (y0 + h + 1) >> 1), slice(x0 >> 1, (x0 + w + 1) >> 1)) if (k and sub) else (slice(y0, y0 + h), slice(x0, x0 + w))
                assert np.array_equal(g[ys, xs], b[ys, xs])
                g[ys, xs] = q[ys, xs]
                assert np.array_equal(g, q)


def test_an_unaligned_payload_takes_the_element_wise_path_to_the_same_bytes(gauss):
    for fmt in FORMATS[:4]:                                        # 8 bit: a base moved by one sample
        f = yuv_fmt(*fmt)
        for H, W in ((38, 270), (37, 269)):
            src = codes(fmt, H, W, seed=3)
            fb = src.shape[1]
            want = GR.grain_ref(src, fmt, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0)
            for so, do in ((1, 0), (0, 1), (1, 1)):
                a, b = torch.zeros(T * fb + 1, dtype=torch.uint8, device="cuda"), torch.zeros(T * fb + 1, dtype=torch.uint8, device="cuda")
                s, o = a[so:so + T * fb].view(T, fb), b[do:do + T * fb].view(T, fb)
                s.copy_(torch.from_numpy(src))
                assert s.data_ptr() % 2 == so and o.data_ptr() % 2 == do
                grain_yuv(s, f, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0, gauss, out=o)
                assert np.array_equal(o.cpu().numpy(), want), (fmt, H, W, so, do)
                assert int(b[0 if do else T * fb]) == 0             # the byte beside the payloads stays
            a = torch.zeros(T * fb + 2, dtype=torch.uint8, device="cuda")      # in place at an odd address
            s = a[1:1 + T * fb].view(T, fb)
            s.copy_(torch.from_numpy(src))
            grain_yuv(s, f, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0, gauss, out=s)
            assert np.array_equal(s.cpu().numpy(), want) and int(a[0]) == 0 and int(a[-1]) == 0


def test_launches_seeds_and_the_source(gauss):
    fmt, H, W = FORMATS[2], 37, 269
    f = yuv_fmt(*fmt)
    src = codes(fmt, H, W, seed=11)
    d = torch.from_numpy(src).cuda()
    whole = grain_yuv(d, f, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0, gauss).cpu().numpy()
    assert np.array_equal(d.cpu().numpy(), src)                     # out of place: src is not written
    singly = np.concatenate([grain_yuv(d[t:t + 1], f, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0 + t, gauss).cpu().numpy() for t in range(T)])
    assert np.array_equal(whole, singly)                            # frame t of a launch with t0 is frame 0 of a launch with t0 + t
    assert not np.array_equal(grain_yuv(d[:1], f, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0 + 1, gauss).cpu().numpy(), whole[:1])
    assert not np.array_equal(grain_yuv(d, f, H, W, GR.BUMPY, SIZED, 0.5, SEED + 1, T0, gauss).cpu().numpy(), whole)
    with pytest.raises(ValueError, match="knots"):
        grain_yuv(d, f, H, W, [1.0] * 15 + [-1.0], SIZED, 0.5, SEED, 0, gauss)
    with pytest.raises(ValueError, match="taps"):
        grain_yuv(d, f, H, W, GR.FLAT, (0.5, 0.5, 0.5), 0.5, SEED, 0, gauss)
    with pytest.raises(ValueError, match="chroma"):
        grain_yuv(d, f, H, W, GR.FLAT, SIZED, -0.5, SEED, 0, gauss)
    with pytest.raises(ValueError, match="seed"):
        grain_yuv(d, f, H, W, GR.FLAT, SIZED, 0.5, 2 ** 32, 0, gauss)
