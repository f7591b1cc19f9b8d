"""-m gpu: the two kernels of ``--deflicker`` (csrc/sn_deflicker.hip) against numpy, exactly: ``sn_yuv_code_hist`` equals np.bincount of
min(code, L - 1) over the luma, ``sn_yuv_apply_lut`` equals lut[plane][min(code, L - 1)] byte for byte; and the paths that must agree: a second call
on a used destination, in place, a rectangle.

Shapes (H x W): 37 x 83 is odd both ways with rows at no alignment (the element-wise loads and stores, clamped 4:2:0 blocks); 40 x 96 at 10 bit holds
words up to 0xFFFF, which both kernels count and look up as code 1023; 64 x 256 FLAT is the histogram's worst case, every sample in one bin; 270 x 480
is several workgroups a frame in both kernels (more than 2048 histogram units, 5 x 2 table tiles); 2 x 3 is the smallest."""
import numpy as np
import pytest
import torch

import deflicker_ref as DR
import yuv_ref as R
from shiftnet_amd.io_edges import apply_lut_yuv, code_hist_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

F420 = R.Fmt(8, R.C420_LEFT, R.BT601, R.LIMITED)
F444_10 = R.Fmt(10, R.C444, R.BT709, R.LIMITED)
F420_10 = R.Fmt(10, R.C420_CENTER, R.BT709, R.FULL)
F444 = R.Fmt(8, R.C444, R.BT601, R.FULL)
RECT = (8, 6, 40, 20)
CASES = {"37x83 420p8": (F420, 37, 83, 3, None), "40x96 444p10 any word": (F444_10, 40, 96, 2, None), "270x480 420p8": (F420, 270, 480, 2, None),
         "270x480 420p10": (F420_10, 270, 480, 1, None), "38x270 444p8": (F444, 38, 270, 2, None), "2x3 420p8": (F420, 2, 3, 2, None),
         "37x83 420p8 rect": (F420, 37, 83, 3, RECT), "37x83 420p10 rect to the edge": (F420_10, 37, 83, 2, (8, 6, 75, 31))}


def words(fmt, H, W, t, seed=0):
    """uint8 [t, frame_bytes]: random bytes at 8 bit, random 16-bit words -- up to 0xFFFF, far above the format's codes -- at 10."""
    n = R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)
    a = np.random.default_rng(seed).integers(0, 256 if fmt.bits == 8 else 65536, (t, n))
    return a.astype("<u2").view(np.uint8).reshape(t, -1) if fmt.bits == 10 else a.astype(np.uint8)


def hist_on_device(src, fmt, H, W, **kw):
    return code_hist_yuv(torch.from_numpy(src).cuda(), yuv_fmt(*fmt), H, W, **kw).cpu().numpy().view(np.uint32).astype(np.int64)


def random_luts(fmt, t, seed=1):
    """[t][2][L] uint16: random codes, no order in them, other ones for every frame."""
    L = 1 << fmt.bits
    return np.random.default_rng(seed).integers(0, L, (t, 2, L)).astype(np.uint16)


def lut_on_device(lut):
    return torch.from_numpy(lut.view(np.int16)).cuda()


@pytest.mark.parametrize("case", list(CASES))
def test_the_histogram_is_bincount_exactly(case):
    fmt, H, W, t, rect = CASES[case]
    src = words(fmt, H, W, t, seed=H + W)
    got = hist_on_device(src, fmt, H, W, rect=rect)
    want = DR.hist_ref(src, fmt, H, W, rect=rect)
    assert got.shape == (t, 1 << fmt.bits) and np.array_equal(got, want), int(np.sum(got != want))
    assert np.all(got.sum(axis=1) == (H * W if rect is None else rect[2] * rect[3]))      # every frame's bins sum to its sample count
    if fmt.bits == 10:
        assert np.all(got[:, 1023] > got[:, :1023].max(axis=1))       # nearly every random word lies above 1023 and is counted there


@pytest.mark.parametrize("code", [0, 16, 255])
def test_a_flat_frame_is_one_bin(code):
    H, W = 64, 256
    src = np.full((2, R.frame_bytes(F420, H, W)), 128, dtype=np.uint8)
    src[:, :H * W] = code
    src[1, 5 * W + 7] = 77                                            # ... and the second frame one sample apart from flat
    got = hist_on_device(src, F420, H, W)
    want = np.zeros((2, 256), dtype=np.int64)
    want[0, code], want[1, code], want[1, 77] = H * W, H * W - 1, 1
    assert np.array_equal(got, want)


def test_a_second_call_on_a_used_destination_gives_the_same_counts():
    fmt, H, W = F420, 37, 83
    f = yuv_fmt(*fmt)
    a, b = (torch.from_numpy(words(fmt, H, W, 3, seed=s)).cuda() for s in (1, 2))
    out = torch.full((3, 256), 12345, dtype=torch.int32, device="cuda")      # zeroed by the call, whatever it held
    assert code_hist_yuv(a, f, H, W, out=out) is out
    first = out.cpu().numpy().copy()
    code_hist_yuv(b, f, H, W, out=out)
    code_hist_yuv(a, f, H, W, out=out)
    assert np.array_equal(out.cpu().numpy(), first) and np.array_equal(first.astype(np.int64), DR.hist_ref(a.cpu().numpy(), fmt, H, W))


@pytest.mark.parametrize("case", list(CASES))
def test_the_tables_are_applied_byte_for_byte_in_place_and_inside_a_rectangle(case):
    fmt, H, W, t, rect = CASES[case]
    f = yuv_fmt(*fmt)
    src = words(fmt, H, W, t, seed=H * W)
    lut = random_luts(fmt, t)
    want = DR.apply_ref(src, lut, fmt, H, W, rect=rect)
    d, dl = torch.from_numpy(src).cuda(), lut_on_device(lut)
    got = apply_lut_yuv(d, f, H, W, dl, rect=rect).cpu().numpy()
    assert got.shape == src.shape and np.array_equal(got, want), int(np.sum(got != want))
    assert np.array_equal(d.cpu().numpy(), src) and not np.array_equal(got, src)
    if rect is not None:                                              # every byte outside the rectangle is the source's, on a destination of its own too
        out = torch.full_like(d, 0xA5)
        apply_lut_yuv(d, f, H, W, dl, rect=rect, out=out)
        inside = DR.apply_ref(np.zeros_like(src), np.full_like(lut, 0xFFFF), fmt, H, W, rect=rect) != 0      # the bytes of the rectangle's samples
        o = out.cpu().numpy()
        assert inside.any() and not inside.all() and np.all(o[~inside] == 0xA5) and np.array_equal(o[inside], want[inside])
    assert apply_lut_yuv(d, f, H, W, dl, rect=rect, out=d) is d and np.array_equal(d.cpu().numpy(), want)      # in place equals out of place


@pytest.mark.parametrize("fmt", [F420, F444, F420_10, F444_10], ids=lambda f: "%d-%d-%d-%d" % f)
def test_identity_tables_return_the_input_illegal_codes_included(fmt):
    H, W, t = 37, 83, 2
    L = 1 << fmt.bits
    a = np.random.default_rng(4).integers(0, L, (t, R.frame_bytes(fmt, H, W) // (1 if fmt.bits == 8 else 2)))      # every code of the format: 0, 255, 1023
    src = a.astype("<u2").view(np.uint8).reshape(t, -1) if fmt.bits == 10 else a.astype(np.uint8)
    ident = np.tile(np.arange(L, dtype=np.uint16), (t, 2, 1))
    got = apply_lut_yuv(torch.from_numpy(src).cuda(), yuv_fmt(*fmt), H, W, lut_on_device(ident)).cpu().numpy()
    assert np.array_equal(got, src)
