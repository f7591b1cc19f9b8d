"""What tests/test_gpu_payload_wide.py relies on, checked without a GPU: that its two shapes provide what they are chosen for, that the references it
compares with run at the top of the seed and frame range, that the two statements of the noise hash name one hash on a frame wider than a tile, and
that the noise of the second tile column is not that of the first.

The geometry every payload kernel launches with (the kernels that include csrc/sn_yuv.h: sn_yuv.hip, sn_degrade.hip, sn_blur.hip, sn_grain.hip,
sn_deflicker.hip): a thread owns SPAN_W x SPAN_H luma samples starting at x0 = (blockIdx.x * 32 + threadIdx.x) * 8, y0 = (blockIdx.y * 8 +
threadIdx.y) * 2; a workgroup of 32 x 8 threads owns a tile of TILE_W x TILE_H.  A thread reads and writes its 8 luma samples of a row with one
8 * esz byte access where the address is a multiple of that (``ldn`` / ``stn``), its 4 samples of a 4:2:0 chroma row with one of 4 * esz bytes, and
element by element otherwise."""
import warnings

import numpy as np
import pytest

import degrade_ref as DR
import dither_ref as D
import grain_ref as GR
import yuv_ref as R
from shiftnet_amd import degrade, grain

TILE_W, TILE_H, SPAN_W, SPAN_H = 256, 16, 8, 2
# all three chroma codes x 8 / 10 bit; every matrix and range with every bit depth (the list of tests/test_gpu_degrade.py; the device file asserts they are equal)
FORMATS = [R.Fmt(8, R.C444, R.BT601, R.FULL), R.Fmt(8, R.C420_CENTER, R.BT709, R.LIMITED), R.Fmt(8, R.C420_LEFT, R.BT601, R.LIMITED),
           R.Fmt(8, R.C420_LEFT, R.BT709, R.FULL), R.Fmt(10, R.C444, R.BT709, R.LIMITED), R.Fmt(10, R.C420_CENTER, R.BT601, R.FULL),
           R.Fmt(10, R.C420_LEFT, R.BT709, R.FULL), R.Fmt(10, R.C420_LEFT, R.BT601, R.LIMITED)]
WIDE, ODD = (40, 272), (37, 269)                                  # H x W: every access wide, across a tile seam; odd both ways
T = 3
SEED, T0 = 12345, 5                                               # what the older tests run with
SEED_MAX, T0_MAX = 2 ** 32 - 1, 2 ** 31 - 1 - T                   # the top of what the wrappers accept for T frames
ids = dict(ids=lambda f: "%d-%d-%d-%d" % f)


def esz(fmt):
    return 1 if fmt.bits == 8 else 2


def row_starts(fmt, H, W, base=0, t=T):
    """(luma, chroma): the byte address of the first sample of every row of the luma plane and of the two chroma planes of ``t`` payloads laid out
    one after the other from address ``base``.  The first entry of each plane is the plane's offset."""
    e, (ch, cw), fb = esz(fmt), R.chroma_shape(fmt, H, W), R.frame_bytes(fmt, H, W)
    luma = [base + k * fb + r * W * e for k in range(t) for r in range(H)]
    chroma = [base + k * fb + (H * W + p * ch * cw + r * cw) * e for k in range(t) for p in range(2) for r in range(ch)]
    return np.array(luma), np.array(chroma)


def chroma_span(fmt):
    """The samples of a chroma row a thread loads at once: its 8 at 4:4:4, the 4 under its luma span at 4:2:0."""
    return SPAN_W if fmt.chroma == R.C444 else SPAN_W // 2


# ---- what the two shapes are claimed to provide -----------------------------------------------------------------------------------------------
def test_the_wide_shape_crosses_a_tile_seam_both_ways_with_interior_threads_behind_it():
    H, W = WIDE
    assert -(-W // TILE_W) >= 2 and -(-H // TILE_H) >= 2
    # the first two threads of the second tile column own whole spans: x0 = 256 reads pixel 255 of the neighbouring workgroup, x0 = 264 does not
    assert TILE_W + 2 * SPAN_W <= W and H % SPAN_H == 0 and W % SPAN_W == 0


@pytest.mark.parametrize("fmt", FORMATS, **ids)
def test_at_the_wide_shape_every_access_of_every_thread_is_aligned(fmt):
    """Payloads at a 16 B aligned base.  Every plane offset, payload start and luma row start is a multiple of 16 B, and so is every chroma row start
    but that of 8-bit 4:2:0, whose pitch is 136 B: a multiple of 8 B, twice the 4 B its chroma load takes.  So no ``ldn`` / ``stn`` falls back."""
    H, W = WIDE
    e = esz(fmt)
    luma, chroma = row_starts(fmt, H, W)
    ch, cw = R.chroma_shape(fmt, H, W)
    assert R.frame_bytes(fmt, H, W) % 16 == 0 and (H * W * e) % 16 == 0 and ((H * W + ch * cw) * e) % 16 == 0
    assert np.all(luma % 16 == 0)
    assert np.all(chroma % (8 if (fmt.bits == 8 and fmt.chroma != R.C444) else 16) == 0)
    # every thread's own accesses, span by span
    assert all((a + x0 * e) % (SPAN_W * e) == 0 for a in luma for x0 in range(0, W, SPAN_W))
    n = chroma_span(fmt)
    assert cw % n == 0 and all((a + c0 * e) % (n * e) == 0 for a in chroma for c0 in range(0, cw, n))


@pytest.mark.parametrize("fmt", FORMATS, **ids)
def test_the_odd_shape_has_a_partial_span_a_one_row_thread_row_and_rows_at_many_alignments(fmt):
    H, W = ODD
    assert -(-W // TILE_W) >= 2 and -(-H // TILE_H) >= 2
    assert 0 < W % SPAN_W < SPAN_W and W - W // SPAN_W * SPAN_W == 5 and W // SPAN_W * SPAN_W >= TILE_W      # the last thread of column 2 owns 5 pixels
    assert H % SPAN_H == 1                                                                                  # the bottom row of threads owns one row
    if fmt.chroma != R.C444:
        assert R.chroma_shape(fmt, H, W) == (19, 135) and 2 * 135 > W and 2 * 19 > H                         # the last chroma sample's block is clamped
    luma, chroma = row_starts(fmt, H, W)
    assert len(set(luma % 16)) > 1 and len(set(chroma % 16)) > 1
    # some spans are aligned and some are not: both paths of ldn / stn run in one launch
    e = esz(fmt)
    al = [(a + x0 * e) % (SPAN_W * e) == 0 for a in luma for x0 in range(0, W - SPAN_W + 1, SPAN_W)]
    assert any(al) and not all(al)


@pytest.mark.parametrize("fmt", FORMATS, **ids)
def test_a_base_moved_by_one_sample_leaves_no_access_aligned_at_the_wide_shape(fmt):
    """A view from byte 2 (10 bit) or byte 1 (8 bit) of a 16 B aligned buffer: no row start is 16 B aligned, and no span of any thread is aligned to
    its own access, so every ``ldn`` / ``stn`` of the launch goes element by element -- at 10 bit in 16-bit words."""
    H, W = WIDE
    e = esz(fmt)
    luma, chroma = row_starts(fmt, H, W, base=e)
    assert np.all(luma % 16 == e) and np.all(chroma % (8 if (fmt.bits == 8 and fmt.chroma != R.C444) else 16) == e)
    assert not any((a + x0 * e) % (SPAN_W * e) == 0 for a in luma for x0 in range(0, W, SPAN_W))
    n = chroma_span(fmt)
    assert not any((a + c0 * e) % (n * e) == 0 for a in chroma for c0 in range(0, R.chroma_shape(fmt, H, W)[1], n))
    assert np.all(luma % e == 0) and np.all(chroma % e == 0)        # ... while every 16-bit word stays 2 B aligned, as the entry points demand


# ---- the references at the top of the seed and frame range ------------------------------------------------------------------------------------
def codes(fmt, H, W, seed=0, t=T):
    """uint8 [t, frame_bytes]: random codes over the whole range of a sample (``clean`` of tests/test_gpu_degrade.py)."""
    n = R.frame_bytes(fmt, H, W) // esz(fmt)
    a = np.random.default_rng(seed).integers(0, 1 << fmt.bits, (t, n))
    return a.astype("<u2").view(np.uint8).reshape(t, -1) if fmt.bits == 10 else a.astype(np.uint8)


def test_the_references_run_warning_free_at_the_extreme_seed_and_frame_and_give_other_noise():
    sized = grain.grain_taps(0.8)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert T0_MAX == 2 ** 31 - 4
        far, near = degrade.noise_field(SEED_MAX, T0_MAX, T, 4, 300), degrade.noise_field(SEED, T0, T, 4, 300)
        assert far.shape == near.shape == (T, 3, 4, 300) and far.dtype == np.float32 and np.isfinite(far).all()
        assert not np.array_equal(far, near) and np.count_nonzero(far) > far.size // 2
        for fmt in (FORMATS[2], FORMATS[5]):                         # one 8-bit and one 10-bit 4:2:0 format, as the device test
            for H, W in (WIDE, ODD):
                src = codes(fmt, H, W, seed=H)
                for ref in (lambda s, f: GR.grain_ref(src, fmt, H, W, GR.BUMPY, sized, 0.5, s, f),
                            lambda s, f: GR.grain_ref(src, fmt, H, W, GR.BUMPY, grain.grain_taps(0.0), 0.5, s, f),
                            lambda s, f: DR.degrade_ref(src, fmt, H, W, DR.FALLING, s, f)):
                    a, b = ref(SEED_MAX, T0_MAX), ref(SEED, T0)
                    assert a.shape == src.shape and not np.array_equal(a, b) and not np.array_equal(a, src) and not np.array_equal(b, src)
            H, W = ODD
            x = np.random.default_rng(1).random((T, 3, H, W), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)
            a, b, plain = D.egress(x, fmt, H, W, SEED_MAX, T0_MAX), D.egress(x, fmt, H, W, SEED, T0), R.egress_emu(x, fmt, H, W)
            assert not np.array_equal(a, b) and not np.array_equal(a, plain) and not np.array_equal(b, plain)


# ---- two statements of one hash ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,t0", [(SEED, T0), (SEED_MAX, T0_MAX)], ids=["default", "extreme"])
def test_the_packages_noise_field_is_the_tests_own_hash_on_a_frame_wider_than_two_tiles(seed, t0):
    """``degrade.noise_field`` is the package's statement (uint32 arithmetic); ``grain_ref.white_field`` (uint32, Python integers for the frame and
    plane terms) and ``dither_ref.key`` (uint64 masked after every product) are the tests' own.  Channel c of the noise is plane 3 + c."""
    H, W = 4, 520
    field = degrade.noise_field(seed, t0, T, H, W)
    gauss = degrade.gauss_table()
    for t in range(T):
        for c in range(3):
            key = D.key(seed, t0 + t, 3 + c, H, W)
            assert key.dtype == np.uint64 and int(key.max()) < 2 ** 32
            assert np.array_equal(field[t, c], gauss[(key >> np.uint64(16)).astype(np.int64)])
            assert np.array_equal(field[t, c], GR.white_field(seed, t0 + t, 3 + c, np.arange(H), np.arange(W)))
    # ... and the columns of the third tile column are not those of the first two
    assert not np.array_equal(field[..., 512:520], field[..., 0:8]) and not np.array_equal(field[..., 512:520], field[..., 256:264])


# ---- the second tile column is not a repeat of the first ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [FORMATS[0], FORMATS[2], FORMATS[5]], **ids)
def test_the_noise_of_the_second_tile_column_is_not_that_of_the_first(fmt):
    """A flat source: every difference between two columns of the result is the noise's.  A kernel that hashed threadIdx.x * 8 + k in place of the
    pixel's column would repeat columns 0 .. 15 in columns 256 .. 271; the restatement does not, so such a kernel cannot equal it."""
    H, W = WIDE
    n = R.frame_bytes(fmt, H, W) // esz(fmt)
    mid = np.full((T, n), 128 << (fmt.bits - 8))
    src = mid.astype("<u2").view(np.uint8).reshape(T, -1) if fmt.bits == 10 else mid.astype(np.uint8)
    out = DR.degrade_ref(src, fmt, H, W, DR.FLAT, SEED, T0)
    back = DR.degrade_ref(src, fmt, H, W, [0.0] * 16, SEED, T0)         # all knots 0: the conversion round trip, the same in every column
    for t in range(T):
        Y, Y0 = R.split_planes(out[t], fmt, H, W)[0], R.split_planes(back[t], fmt, H, W)[0]
        assert len(np.unique(Y0)) == 1
        added = Y - Y0
        assert np.any(added[:, TILE_W:] != 0)
        assert not np.array_equal(added[:, TILE_W:TILE_W + 16], added[:, 0:16])
    field = degrade.noise_field(SEED, T0, T, H, W)
    assert not np.array_equal(field[..., TILE_W:TILE_W + 16], field[..., 0:16])
