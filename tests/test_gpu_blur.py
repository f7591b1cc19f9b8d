"""-m gpu: ``sn_yuv_blur`` (csrc/sn_blur.hip) against its numpy restatement (tests/blur_ref.py) byte for byte, against the composition of the two
existing edge kernels at one tap, and the properties that follow from an output being a pure function of the source payloads its window names.
Payloads of random codes over the whole sample range, illegal ones included: both clamps and both ends of the tables take part."""
import numpy as np
import pytest
import torch

import blur_ref as B
from shiftnet_amd import degrade
from shiftnet_amd.io_edges import blur_yuv, egress_yuv, ingest_yuv, yuv_fmt
from test_gpu_degrade import FORMATS, SIZES, clean

pytestmark = pytest.mark.gpu

S, T, GAMMA = 7, 3, 2.2
# (c0, lo, hi, outputs): the window clamps at neither end (at n <= 5), at the low end, at the high end, at both, and at both with lo == hi
WINDOWS = [(2, 0, 6, T), (0, 0, 6, T), (4, 0, 6, T), (2, 2, 4, T), (3, 3, 3, 1)]


@pytest.fixture(scope="module")
def tables():
    return tuple(torch.from_numpy(t.copy()).cuda() for t in degrade.gamma_tables(GAMMA))


def on_device(src, fmt, H, W, n, c0, lo, hi, t, tab):
    d = torch.from_numpy(src).cuda()
    out = torch.empty((t, src.shape[1]), dtype=torch.uint8, device="cuda")
    return blur_yuv(d, yuv_fmt(*fmt), H, W, n, c0, lo, hi, tab, out=out).cpu().numpy()


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: "%d-%d-%d-%d" % f)
def test_the_kernel_is_the_numpy_restatement_byte_for_byte(fmt, tables):
    for H, W in SIZES:
        src = clean(fmt, H, W, seed=H * 100 + W, t=S)
        cases = [(n, w) for n in (1, 3, 5) for w in WINDOWS] + ([(15, WINDOWS[0])] if (H, W) == (37, 53) else [])
        for n, (c0, lo, hi, t) in cases:
            for tab, gamma in ((tables, GAMMA), (None, 1.0)):
                got = on_device(src, fmt, H, W, n, c0, lo, hi, t, tab)
                want = B.blur_ref(src, fmt, H, W, n, c0, t, lo, hi, gamma)
                assert got.shape == want.shape == (t, src.shape[1]) and np.array_equal(got, want), (H, W, n, c0, lo, hi, gamma)


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: "%d-%d-%d-%d" % f)
def test_one_tap_without_tables_is_the_two_edge_kernels(fmt):
    f = yuv_fmt(*fmt)
    for H, W in SIZES:
        src = clean(fmt, H, W, seed=7 + H, t=S)
        d = torch.from_numpy(src).cuda()
        want = egress_yuv(ingest_yuv(d, f, H, W, H, W, torch.float32)[0], f, H, W)
        assert torch.equal(blur_yuv(d, f, H, W, 1, 0, 0, S - 1, None), want), (H, W)


def test_an_unaligned_payload_takes_the_element_wise_path_to_the_same_bytes(tables):
    for fmt in FORMATS[:4]:                                        # 8 bit: a base moved by one sample
        f = yuv_fmt(*fmt)
        for H, W in ((16, 64), (37, 53)):
            src = clean(fmt, H, W, seed=3, t=S)
            fb = src.shape[1]
            want = on_device(src, fmt, H, W, 5, 2, 0, 6, T, tables)
            for so, do in ((1, 0), (0, 1), (1, 1)):
                a, b = torch.zeros(S * fb + 1, dtype=torch.uint8, device="cuda"), torch.zeros(T * fb + 1, dtype=torch.uint8, device="cuda")
                s, o = a[so:so + S * fb].view(S, fb), b[do:do + T * fb].view(T, fb)
                s.copy_(torch.from_numpy(src))
                assert s.data_ptr() % 2 == so and o.data_ptr() % 2 == do
                blur_yuv(s, f, H, W, 5, 2, 0, 6, tables, out=o)
                assert np.array_equal(o.cpu().numpy(), want), (fmt, H, W, so, do)
                assert int(b[0 if do else T * fb]) == 0             # the byte beside the payloads stays


def test_launches_the_source_and_the_wrappers_refusals(tables):
    fmt, H, W = FORMATS[2], 37, 53
    f = yuv_fmt(*fmt)
    src = clean(fmt, H, W, seed=11, t=S)
    d = torch.from_numpy(src).cuda()
    whole = blur_yuv(d, f, H, W, 5, 1, 0, 6, tables, out=torch.empty((5, src.shape[1]), dtype=torch.uint8, device="cuda"))
    assert np.array_equal(d.cpu().numpy(), src)                     # src is not written
    one = torch.empty((1, src.shape[1]), dtype=torch.uint8, device="cuda")
    singly = torch.cat([blur_yuv(d, f, H, W, 5, c, 0, 6, tables, out=one).clone() for c in range(1, 6)])
    assert torch.equal(whole, singly)                               # five outputs in one launch are five launches of one
    assert torch.equal(blur_yuv(d, f, H, W, 5, 2, 0, 6, tables)[:4], whole[1:])    # out=None: outputs c0 .. hi, here 2 .. 6
    # a window clamped to a scene is the blur of the scene alone
    assert torch.equal(blur_yuv(d, f, H, W, 5, 2, 2, 4, tables), blur_yuv(d[2:5].contiguous(), f, H, W, 5, 0, 0, 2, tables))
    # linear light is not gamma 1
    assert not torch.equal(blur_yuv(d, f, H, W, 5, 1, 0, 6, None), whole)
    for n in (0, 4, 17):
        with pytest.raises(ValueError, match="taps"):
            blur_yuv(d, f, H, W, n, 1, 0, 6, tables)
    for c0, lo, hi in ((1, 0, 7), (1, -1, 6), (1, 2, 6), (5, 0, 4), (3, 4, 3)):
        with pytest.raises(ValueError, match="lo"):
            blur_yuv(d, f, H, W, 5, c0, lo, hi, tables, out=one)
    with pytest.raises(ValueError, match="lo"):
        blur_yuv(d, f, H, W, 5, 5, 0, 6, tables, out=torch.empty((3, src.shape[1]), dtype=torch.uint8, device="cuda"))      # c0 + T - 1 > hi
