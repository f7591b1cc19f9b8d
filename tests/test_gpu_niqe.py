"""-m gpu: ``sn_yuv_niqe_sums`` against its float64 restatement (tests/niqe_ref.py) on the frames of tests/niqe_cases.py, the score made of the kernel's
sums against what the reference implementation recorded for those frames (tests/golden/niqe_cases.npz), and the equalities that must be exact.

The kernel forms the map values in float32 and the restatement in float64, so the comparison has tolerances; they were measured on these cases (the
test prints them before it asserts; DESIGN.md 3.33 has the list):
  * counts: a value and its float64 twin can lie on both sides of zero.  Largest difference of a count: 0 -- none of the 1.1 million values of
    these cases does -- asserted at COUNT_TOL = 2;
  * the three sums of a map: largest relative difference 6.0e-6 (the rectangle case), asserted at SUM_RTOL = 2e-5;
  * the score: largest relative difference to the reference's 1.8e-4 (192x288-sigma10: one shape lands a step of the grid away; every other
    case is below 2e-6), asserted at SCORE_RTOL = 5e-4 -- the host test's tolerance, 2e-9, is lost in it.
The restatement filters with the model's float64 taps, the kernel with their float32 roundings: that is part of what float32 costs.  With either a
flat area filters to exactly itself (tests/niqe_cases.py: FLAT), so in the flat case both have coefficients and sums of exactly zero in block (0, 0) and
in the 3 (at scale 2: 1 or 2) columns and rows beside it, and are compared there as everywhere: zero against zero."""
import os

import numpy as np
import pytest
import torch

import niqe_cases as K
import niqe_ref as NR
from shiftnet_amd import niqe as N
from shiftnet_amd.io_edges import niqe_sums_yuv, yuv_fmt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_TOL = 2
SUM_RTOL = 2e-5
SCORE_RTOL = 5e-4
GARBAGE = -1.2345e300      # what dst holds before a call


@pytest.fixture(scope="module")
def model():
    return N.load_params(N.default_params_path())


@pytest.fixture(scope="module")
def taps(model):
    """(the 7 taps as float32 on the device, the model's float64 taps for the restatement)."""
    return torch.from_numpy(model[2].astype(np.float32)).cuda(), model[2]


@pytest.fixture(scope="module")
def results(taps):
    """case name -> (the payloads on the device, the kernel's sums, the restatement's sums), each [T, 2, nbh, nbw, 5, 5] float64: computed once, read
    by every test below."""
    dev, g = taps
    out = {}
    for c in K.CASES:
        pay = K.payloads(c)
        d = torch.from_numpy(pay).cuda()
        got = niqe_sums_yuv(d, yuv_fmt(*c.fmt), c.H, c.W, dev, rect=c.rect).cpu().numpy()
        out[c.name] = (d, got, NR.niqe_sums_ref(pay, c.fmt, c.H, c.W, g, rect=c.rect))
    return out


def test_counts_and_sums_equal_the_float64_restatement_within_what_float32_costs(results):
    worst_count, worst_sum = 0.0, 0.0
    for c in K.CASES:
        _, got, want = results[c.name]
        assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(got).all(), c.name
        if c.flat:
            assert (got[:, :, 0, 0] == 0).all(), got[:, :, 0, 0]                       # exactly zero counts, and sums, on all five maps at both scales
        # every sample is on one side or is zero: the two counts add up to the block's samples at most, and -- an exact zero being rare in either
        # precision -- nearly to all of them, except in the flat case
        B2 = np.array([96 * 96, 48 * 48], np.float64)[None, :, None, None, None] * np.ones(got.shape[:5])
        assert (got[..., 0] + got[..., 2] <= B2).all() and (c.flat or (got[..., 0] + got[..., 2] >= B2 - COUNT_TOL).all())
        assert (got[..., [0, 2]] == np.rint(got[..., [0, 2]])).all()
        dc = float(np.abs(got[..., [0, 2]] - want[..., [0, 2]]).max())
        g, w = got[..., [1, 3, 4]], want[..., [1, 3, 4]]
        assert (g[w == 0] == 0).all()
        ds = float((np.abs(g - w)[w > 0] / w[w > 0]).max())
        print(f"{c.name}: largest difference of a count {dc:g}, largest relative difference of a sum {ds:.3g}")
        worst_count, worst_sum = max(worst_count, dc), max(worst_sum, ds)
    print(f"largest difference of a count: {worst_count:g}; largest relative difference of a sum: {worst_sum:.3g}")
    assert worst_count <= COUNT_TOL and worst_sum <= SUM_RTOL


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
    assert worst <= SCORE_RTOL


def test_a_rectangle_gives_the_sums_of_the_cropped_stream_exactly(results, taps):
    import picture_ref as P
    c = K.BY_NAME["rect-of-240x400-420"]
    _, got, _ = results[c.name]
    x0, y0, w, h = c.rect
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
