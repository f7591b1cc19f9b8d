"""-m gpu: ``sn_yuv_degrade`` (csrc/sn_degrade.hip) against its numpy restatement (tests/degrade_ref.py) byte for byte, against the composition of
the two existing edge kernels around a noise tensor, and the properties that follow from the noise being a pure function of the sample's place in
the stream.  Payloads of random codes over the whole sample range, illegal ones included: both clamps and both ends of the curve take part."""
import numpy as np
import pytest
import torch

import degrade_ref as DR
import yuv_ref as R
from shiftnet_amd import degrade
from shiftnet_amd.io_edges import degrade_yuv, egress_yuv, ingest_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

# all three chroma codes x 8 / 10 bit; every matrix and range with every bit depth
FORMATS = [R.Fmt(8, R.C444, R.BT601, R.FULL), R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED), R.Fmt(8, R.C420_LEFT, R.BT601, R.LIMITED),
           R.Fmt(8, R.C420_LEFT, R.BT709, R.FULL), R.Fmt(10, R.C444, R.BT709, R.LIMITED), R.Fmt(10, R.C420_CENTER, R.BT601, R.FULL),
           R.Fmt(10, R.C420_LEFT, R.BT709, R.FULL), R.Fmt(10, R.C420_LEFT, R.BT601, R.LIMITED)]
# H x W: all-interior wide path; odd, edge threads on both sides; narrower than a thread's span, both ways; one pixel
SIZES = [(16, 64), (37, 53), (2, 5), (5, 2), (1, 1)]
T, T0, SEED = 3, 5, 12345


def clean(fmt, H, W, seed=0, t=T):
    """uint8 [t, frame_bytes]: random codes over the whole range of a sample."""
    n = R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)
    a = np.random.default_rng(seed).integers(0, 1 << fmt.bits, (t, n))
    return a.astype("<u2").view(np.uint8).reshape(t, -1) if fmt.bits == 10 else a.astype(np.uint8)


@pytest.fixture(scope="module")
def gauss():
    return torch.from_numpy(degrade.gauss_table().copy()).cuda()


def on_device(src, fmt, H, W, knots, gauss, seed=SEED, t0=T0):
    return degrade_yuv(torch.from_numpy(src).cuda(), yuv_fmt(*fmt), H, W, knots, seed, t0, gauss).cpu().numpy()


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: "%d-%d-%d-%d" % f)
def test_the_kernel_is_the_numpy_restatement_byte_for_byte(fmt, gauss):
    for H, W in SIZES:
        src = clean(fmt, H, W, seed=H * 100 + W)
        for knots in (DR.FLAT, DR.FALLING):
            got = on_device(src, fmt, H, W, knots, gauss)
            want = DR.degrade_ref(src, fmt, H, W, knots, SEED, T0)
            assert got.shape == want.shape == src.shape and np.array_equal(got, want), (H, W, knots[0])


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: "%d-%d-%d-%d" % f)
def test_the_kernel_is_the_two_edge_kernels_around_a_noise_tensor(fmt, gauss):
    f = yuv_fmt(*fmt)
    for H, W in SIZES:
        src = clean(fmt, H, W, seed=7 + H)
        d = torch.from_numpy(src).cuda()
        x = ingest_yuv(d, f, H, W, H, W, torch.float32)[0]
        g = degrade.noise_field(SEED, T0, T, H, W)
        for knots in (DR.FLAT, DR.FALLING):
            n = torch.from_numpy(DR.sigma_plane(src, fmt, H, W, knots) * g).cuda()
            want = egress_yuv((x + n).contiguous(), f, H, W).cpu().numpy()
            assert np.array_equal(on_device(src, fmt, H, W, knots, gauss), want), (H, W, knots[0])


def test_an_unaligned_payload_takes_the_element_wise_path_to_the_same_bytes(gauss):
    for fmt in FORMATS[:4]:                                        # 8 bit: a base moved by one sample
        f = yuv_fmt(*fmt)
        for H, W in ((16, 64), (37, 53)):
            src = clean(fmt, H, W, seed=3)
            fb = src.shape[1]
            want = on_device(src, fmt, H, W, DR.FALLING, gauss)
            for so, do in ((1, 0), (0, 1), (1, 1)):
                a, b = torch.zeros(T * fb + 1, dtype=torch.uint8, device="cuda"), torch.zeros(T * fb + 1, dtype=torch.uint8, device="cuda")
                s, o = a[so:so + T * fb].view(T, fb), b[do:do + T * fb].view(T, fb)
                s.copy_(torch.from_numpy(src))
                assert s.data_ptr() % 2 == so and o.data_ptr() % 2 == do
                degrade_yuv(s, f, H, W, DR.FALLING, SEED, T0, gauss, out=o)
                assert np.array_equal(o.cpu().numpy(), want), (fmt, H, W, so, do)
                assert int(b[0 if do else T * fb]) == 0             # the byte beside the payloads stays


def test_launches_seeds_and_the_source(gauss):
    fmt, H, W = FORMATS[2], 37, 53
    f = yuv_fmt(*fmt)
    src = clean(fmt, H, W, seed=11)
    d = torch.from_numpy(src).cuda()
    whole = degrade_yuv(d, f, H, W, DR.FALLING, SEED, 0, gauss).cpu().numpy()
    assert np.array_equal(d.cpu().numpy(), src)                     # src is not written
    singly = np.concatenate([degrade_yuv(d[t:t + 1], f, H, W, DR.FALLING, SEED, t, gauss).cpu().numpy() for t in range(T)])
    assert np.array_equal(whole, singly)                            # frames [0:3] in one launch are three launches with t0 = 0, 1, 2
    # the same frame under another frame number, and under another seed, gets other noise
    assert not np.array_equal(degrade_yuv(d[:1], f, H, W, DR.FALLING, SEED, 1, gauss).cpu().numpy(), whole[:1])
    assert not np.array_equal(degrade_yuv(d, f, H, W, DR.FALLING, SEED + 1, 0, gauss).cpu().numpy(), whole)
    # sigma 0 is the conversion round trip, not the input
    zero = degrade_yuv(d, f, H, W, [0.0] * 16, SEED, 0, gauss)
    back = egress_yuv(ingest_yuv(d, f, H, W, H, W, torch.float32)[0], f, H, W)
    assert torch.equal(zero, back)
    with pytest.raises(ValueError, match="knots"):
        degrade_yuv(d, f, H, W, [1.0] * 15 + [-1.0], SEED, 0, gauss)
    with pytest.raises(ValueError, match="seed"):
        degrade_yuv(d, f, H, W, DR.FLAT, 2 ** 32, 0, gauss)
