"""-m gpu: ``sn_yuv_niqe_sums`` against its restatement and against the plain long-double reference (tests/niqe_ref.py) on the frames of
tests/niqe_cases.py, the score made of the kernel's sums against what the reference implementation recorded for those frames
(tests/golden/niqe_cases.npz), and the equalities that must be exact.

The kernel computes in float64 from the codes on and the restatement repeats it rounding for rounding, with the kernel's taps (the float32 taps
widened, over their own sum), so the coefficients are the same bits (the test prints every figure before it asserts; DESIGN.md 3.33 has the list):
  * counts: equal, COUNT_TOL = 0;
  * the three sums of a map: the two differ only in the order in which at most 9 216 doubles are added, 9 216 x 2^-53 = 1e-12 at most; measured
    4.4e-16, asserted at SUM_RTOL = 1e-10;
  * against the plain long-double reference with the model's float64 taps -- the right answer: what is left is the rounding of the taps to float32,
    3e-8 relative each.  Largest relative difference of a sum 3.0e-8 (2.4e-8 .. 3.0e-8 on every case, textured or near-flat), every count equal;
    asserted at PLAIN_RTOL = 3e-7, ten times that;
  * the score against the reference implementation's: largest relative difference 1.55e-8, asserted at SCORE_RTOL = 1.55e-7.
The float32 kernel this one replaced was asserted at 2 counts, 2e-5 and 5e-4, measured on textured frames only; on the near-flat frames it missed
this restatement by up to 8.1e-3 of a sum, 3 counts and 3.2e-3 of a score, and a flat frame of code 49, 98, 125 or 196 (10 bit: 98, 125) came out as
9 216 values of one sign (DESIGN.md 3.33 has what the device gave, case by case)."""
import os
import warnings

import numpy as np
import pytest
import torch

import niqe_cases as K
import niqe_ref as NR
from shiftnet_amd import niqe as N
from shiftnet_amd.io_edges import niqe_sums_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_TOL = 0
SUM_RTOL = 1e-10
PLAIN_RTOL = 3e-7
SCORE_RTOL = 1.55e-7
GARBAGE = -1.2345e300      # what dst holds before a call


@pytest.fixture(scope="module")
def model():
    return N.load_params(N.default_params_path())


@pytest.fixture(scope="module")
def taps(model):
    """(the 7 taps as float32 on the device, the model's float64 taps for the references)."""
    return torch.from_numpy(model[2].astype(np.float32)).cuda(), model[2]


@pytest.fixture(scope="module")
def results(taps):
    """case name -> (the payloads on the device, the kernel's sums, the restatement's sums with the kernel's taps), each [T, 2, nbh, nbw, 5, 5]
    float64: computed once, read by every test below."""
    dev, g = taps
    out = {}
    for c in K.CASES + K.PARTLY_FLAT:
        pay = K.payloads(c)
        d = torch.from_numpy(pay).cuda()
        got = niqe_sums_yuv(d, yuv_fmt(*c.fmt), c.H, c.W, dev, rect=c.rect).cpu().numpy()
        out[c.name] = (d, got, NR.niqe_sums_ref(pay, c.fmt, c.H, c.W, NR.kernel_taps(g), rect=c.rect))
    return out


def _differences(got, want):
    """(largest difference of a count, largest relative difference of a sum; a sum that is zero in ``want`` and not in ``got`` counts as inf)."""
    g, w = got[..., [1, 3, 4]], want[..., [1, 3, 4]]
    ds = float((np.abs(g - w)[w > 0] / w[w > 0]).max())
    return float(np.abs(got[..., [0, 2]] - want[..., [0, 2]]).max()), ds if (g[w == 0] == 0).all() else np.inf


def test_counts_equal_the_float64_restatements_and_sums_differ_by_their_order_only(results):
    worst_count, worst_sum = 0.0, 0.0
    for c in K.CASES + K.PARTLY_FLAT:
        _, got, want = results[c.name]
        assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(got).all(), c.name
        dc, ds = _differences(got, want)
        print(f"{c.name}: largest difference of a count {dc:g}, largest relative difference of a sum {ds:.3g}")
        worst_count, worst_sum = max(worst_count, dc), max(worst_sum, ds)
    print(f"largest difference of a count: {worst_count:g}; largest relative difference of a sum: {worst_sum:.3g}")
    assert worst_count <= COUNT_TOL and worst_sum <= SUM_RTOL
    for c in K.CASES + K.PARTLY_FLAT:
        _, got, _ = results[c.name]
        if c.flat:
            assert (got[:, :, 0, 0] == 0).all(), got[:, :, 0, 0]                       # exactly zero counts, and sums, on all five maps at both scales
        # every sample is on one side or is zero: the two counts add up to the block's samples at most, and -- an exact zero being rare -- nearly to
        # all of them, except in the flat case
        B2 = np.array([96 * 96, 48 * 48], np.float64)[None, :, None, None, None] * np.ones(got.shape[:5])
        assert (got[..., 0] + got[..., 2] <= B2).all() and (c.flat or (got[..., 0] + got[..., 2] >= B2 - 2).all())
        assert (got[..., [0, 2]] == np.rint(got[..., [0, 2]])).all()


def test_counts_and_sums_are_those_of_the_plain_long_double_reference_but_for_the_float32_taps(results, taps):
    """What the kernel is for: the header's formula on the values themselves, in long double, with the model's unrounded taps.  In the two partly flat
    cases only the blocks no window of which touches the flat square are compared (zero there, a residue of 1e-17 in the reference)."""
    worst_count, worst_sum = 0.0, 0.0
    for c in K.CASES + K.PARTLY_FLAT:
        _, got, _ = results[c.name]
        want = NR.niqe_sums_ref(K.payloads(c), c.fmt, c.H, c.W, taps[1], rect=c.rect, sums=NR.plain_sums_of_luma)
        if c.flat:
            got, want = got[:, :, :, 2:], want[:, :, :, 2:]
        dc, ds = _differences(got, want)
        print(f"{c.name}: largest difference of a count {dc:g}, largest relative difference of a sum {ds:.3g}")
        worst_count, worst_sum = max(worst_count, dc), max(worst_sum, ds)
    print(f"largest difference of a count: {worst_count:g}; largest relative difference of a sum: {worst_sum:.3g}")
    assert worst_count == 0 and worst_sum <= PLAIN_RTOL <= 2e-5


def test_the_score_of_the_kernels_sums_is_the_references_score(results, model):
    mu, cov, _ = model
    with np.load(os.path.join(ROOT, "tests", "golden", "niqe_cases.npz")) as z:
        recorded = {k: z[k] for k in z.files}
    worst = 0.0
    for c in K.CASES:
        _, got, _ = results[c.name]
        for t in range(len(c.seeds)):
            want = recorded["score/" + c.name][t]
            rel = abs(N.frame_score(got[t], mu, cov) - want) / want
            print(f"{c.name}[{t}]: reference {want:.6f}, relative difference {rel:.3g}")
            worst = max(worst, rel)
    print(f"largest relative difference of a score: {worst:.3g}")
    assert worst <= SCORE_RTOL <= 5e-4


def test_a_flat_picture_gives_zeros_at_every_code_and_no_score(taps, model):
    """All 50 doubles of every block of a picture of one code are exactly 0 -- both scales, both ranges, both bit depths, the codes included at which
    a filter of the values themselves leaves a residue -- and such a frame has no score."""
    mu, cov, _ = model
    bad = []
    for c in K.FLAT_CASES:
        d = torch.from_numpy(K.payloads(c)).cuda()
        got = niqe_sums_yuv(d, yuv_fmt(*c.fmt), c.H, c.W, taps[0]).cpu().numpy()
        assert got.shape == (1, 2, 1, 2, 5, 5)
        if (got != 0).any():
            bad.append(c.name)
            print(f"{c.name}: counts {got[0, :, 0, :, 0, [0, 2]].ravel()}, largest sum {np.abs(got[..., [1, 3, 4]]).max():.3g}")
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            assert np.isnan(N.frame_score(got[0], mu, cov)), c.name
    assert not bad, bad


def test_a_rectangle_gives_the_sums_of_the_cropped_stream_exactly(results, taps):
    import picture_ref as P
    c = K.BY_NAME["rect-of-240x400-420"]
    _, got, _ = results[c.name]
    x0, y0, w, h = c.rect
    cropped = torch.from_numpy(P.crop_payloads(K.payloads(c), c.fmt, c.H, c.W, c.rect)).cuda()
    alone = niqe_sums_yuv(cropped, yuv_fmt(*c.fmt), h, w, taps[0]).cpu().numpy()
    assert got.shape == (1, 2, 2, 3, 5, 5) and np.array_equal(got, alone)


def test_a_rectangle_of_a_10_bit_left_sited_stream_gives_the_sums_of_the_cropped_stream_exactly(results, taps):
    """x0 = 10 is no multiple of 16: every row of the rectangle starts 20 bytes into the 2-byte pitch and the loads go element by element."""
    import picture_ref as P
    c = K.BY_NAME["rect-of-240x400-420-left-10bit"]
    _, got, _ = results[c.name]
    x0, y0, w, h = c.rect
    assert x0 % 16 != 0 and c.fmt.bits == 10 and c.fmt.chroma == 2
    cropped = torch.from_numpy(P.crop_payloads(K.payloads(c), c.fmt, c.H, c.W, c.rect)).cuda()
    alone = niqe_sums_yuv(cropped, yuv_fmt(*c.fmt), h, w, taps[0]).cpu().numpy()
    assert got.shape == (1, 2, 2, 3, 5, 5) and np.array_equal(got, alone)


def test_every_frame_of_a_launch_equals_the_frame_alone_and_a_second_launch_gives_the_same_doubles(results, taps):
    c = K.BY_NAME["T3"]
    d, got, _ = results[c.name]
    f = yuv_fmt(*c.fmt)
    assert got.shape[0] == 3 and not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    for t in range(3):
        assert np.array_equal(niqe_sums_yuv(d[t:t + 1].contiguous(), f, c.H, c.W, taps[0]).cpu().numpy(), got[t:t + 1]), t
    # into garbage between guard words: every word of dst is overwritten, nothing else is written, and the doubles are those of the first launch
    n = got.size
    buf = torch.full((n + 16,), GARBAGE, dtype=torch.float64, device="cuda")
    out = buf[8:8 + n].view(got.shape)
    for _ in range(2):
        assert niqe_sums_yuv(d, f, c.H, c.W, taps[0], out=out) is out
        assert np.array_equal(out.cpu().numpy(), got)
    ends = buf.cpu().numpy()
    assert (ends[:8] == GARBAGE).all() and (ends[8 + n:] == GARBAGE).all()


def test_payloads_at_odd_addresses_give_the_same_sums(results, taps):
    """The wide loads test the address: an 8-bit stream one byte past a 16-byte boundary takes the element-wise path and gives the same doubles."""
    c = K.BY_NAME["200x300-crop"]
    d, got, _ = results[c.name]
    T, fb = d.shape
    buf = torch.zeros(T * fb + 32, dtype=torch.uint8, device="cuda")
    base = (-buf.data_ptr()) % 16 + 1
    moved = buf[base:base + T * fb].view(T, fb)
    moved.copy_(d)
    assert moved.data_ptr() % 16 == 1
    assert np.array_equal(niqe_sums_yuv(moved, yuv_fmt(*c.fmt), c.H, c.W, taps[0]).cpu().numpy(), got)


def test_a_picture_without_a_block_is_refused_by_the_binding():
    d = torch.zeros((1, 95 * 192 * 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="no whole"):
        niqe_sums_yuv(d, yuv_fmt(8, 0, 1, 0), 95, 192, torch.zeros(7, device="cuda"))
