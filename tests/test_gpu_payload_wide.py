"""-m gpu: the kernels that read and write planar Y'CbCr payloads on frames wider than one workgroup, at bases moved by one sample at both bit depths,
and at the top of the seed and frame range -- each against the numpy restatement the kernel's own test uses, byte for byte.

Shapes (H x W; tests/test_host_payload_wide.py asserts what each provides): 40 x 272 is two tile columns by three tile rows with every row and
plane aligned, so every thread takes the wide loads and stores and the thread at x0 = 256 reads pixel 255 of the neighbouring workgroup; 37 x 269 is
odd both ways, the last thread of the second column owns 5 pixels, the bottom row of threads one row, the 135-wide chroma plane is clamped and rows
sit at every alignment.  Payloads are random codes over the whole sample range (random 16-bit words for the two deflicker kernels)."""
import itertools

import numpy as np
import pytest
import torch

import blur_ref as B
import deflicker_ref as FR
import degrade_ref as DR
import dither_ref as D
import grain_ref as GR
import mix_ref as M
import test_host_payload_wide as HW
import yuv_ref as R
from shiftnet_amd import degrade, grain
from shiftnet_amd.io_edges import apply_lut_yuv, blur_yuv, code_hist_yuv, degrade_yuv, egress_yuv, grain_yuv, yuv_fmt
from test_gpu_deflicker import random_luts, words
from test_gpu_degrade import FORMATS, clean

pytestmark = pytest.mark.gpu

WIDE, ODD, T = HW.WIDE, HW.ODD, HW.T
SHAPES = [WIDE, ODD]
SEED, T0, SEED_MAX, T0_MAX = HW.SEED, HW.T0, HW.SEED_MAX, HW.T0_MAX
S, GAMMA = 7, 2.2                                                 # source payloads of a blur, and its gamma
SIZED, WHITE = grain.grain_taps(0.8), grain.grain_taps(0.0)
MIXES = [("amount", 0.25, 1.0), ("removed", 4.0, 2.0)]
DITHERS = [None, (0xDEADBEEF, 5)]
DTYPES = [torch.float32, torch.bfloat16]
GUARD, FILL = 64, 0xA5
ids = dict(ids=lambda f: "%d-%d-%d-%d" % f)
by_fmt = pytest.mark.parametrize("fmt", FORMATS, **ids)


def test_the_formats_are_the_eight_the_host_file_makes_its_claims_for():
    assert FORMATS == HW.FORMATS and len(set(FORMATS)) == 8
    assert {(f.bits, f.chroma) for f in FORMATS} == set(itertools.product((8, 10), (R.C444, R.C420_CENTER, R.C420_LEFT)))


@pytest.fixture(scope="module")
def gauss():
    return torch.from_numpy(degrade.gauss_table().copy()).cuda()


@pytest.fixture(scope="module")
def tables():
    return tuple(torch.from_numpy(t.copy()).cuda() for t in degrade.gamma_tables(GAMMA))


def dev(a):
    return torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy()


def padded(H, W):
    """The tensor an egress reads: the wide shape as it is, the odd one inside a plane whose rows are at no alignment either."""
    return (H, W) if (H, W) == WIDE else (40, 275)


def tensor(t, Hp, Wp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(t, 3, Hp, Wp, generator=g) * 1.4 - 0.2                         # drawn from [-0.2, 1.2]: the clamp matters


# ---- 1 .. 3: the three kernels that had never run with gridDim.x > 1 ------------------------------------------------------------------------------
@by_fmt
def test_degrade_wide_is_the_restatement_byte_for_byte(fmt, gauss):
    f = yuv_fmt(*fmt)
    for H, W in SHAPES:
        src = clean(fmt, H, W, seed=H * 1000 + W)
        d = dev(src)
        for knots in (DR.FLAT, DR.FALLING):
            got = host(degrade_yuv(d, f, H, W, knots, SEED, T0, gauss))
            want = DR.degrade_ref(src, fmt, H, W, knots, SEED, T0)
            assert got.shape == want.shape == src.shape
            assert np.array_equal(got, want), (H, W, knots[0], int(np.sum(got != want)), int(np.flatnonzero((got != want).ravel())[0]))
            if (H, W) == WIDE:                                     # noise reached the second tile column: all knots 0 is the conversion round trip
                back = host(degrade_yuv(d, f, H, W, [0.0] * 16, SEED, T0, gauss))
                for t in range(T):
                    for a, b in zip(R.split_planes(got[t], fmt, H, W), R.split_planes(back[t], fmt, H, W)):
                        c = HW.TILE_W if a.shape[1] == W else HW.TILE_W // 2
                        assert np.any(a[:, c:] != b[:, c:])


@by_fmt
def test_blur_wide_is_the_restatement_byte_for_byte(fmt, tables):
    f = yuv_fmt(*fmt)
    for H, W in SHAPES:
        src = clean(fmt, H, W, seed=H * 1000 + W, t=S)
        d = dev(src)
        cases = [(n, w) for n in (1, 5) for w in ((2, 0, 6), (2, 2, 4))] + ([(15, (2, 0, 6))] if (H, W) == ODD else [])
        for n, (c0, lo, hi) in cases:
            for tab, gamma in ((tables, GAMMA), (None, 1.0)):
                out = torch.empty((T, src.shape[1]), dtype=torch.uint8, device="cuda")
                got = host(blur_yuv(d, f, H, W, n, c0, lo, hi, tab, out=out))
                want = B.blur_ref(src, fmt, H, W, n, c0, T, lo, hi, gamma)
                assert got.shape == want.shape == (T, src.shape[1])
                assert np.array_equal(got, want), (H, W, n, c0, lo, hi, gamma, int(np.sum(got != want)), int(np.flatnonzero((got != want).ravel())[0]))


@by_fmt
def test_mixed_egress_wide_is_the_restatement_byte_for_byte_and_writes_nothing_else(fmt):
    f = yuv_fmt(*fmt)
    for H, W in SHAPES:
        fb = R.frame_bytes(fmt, H, W)
        inp = M.random_payloads(fmt, T, H, W, seed=H + W)
        ref = dev(inp)
        x32 = tensor(T, *padded(H, W), seed=H * 1000 + W)
        for dt in DTYPES:
            x = x32.to(dt)
            xd, xh = x.cuda(), x.float().numpy()
            for mix, dither in itertools.product(MIXES, DITHERS):
                buf = torch.full((T * fb + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
                got = host(egress_yuv(xd, f, H, W, dst=buf[GUARD:GUARD + T * fb].view(T, fb), dither=dither, mix=mix, ref=ref))
                want = M.egress(xh, fmt, H, W, mix, inp, dither)
                assert np.array_equal(got, want), (H, W, dt, mix, dither, int(np.sum(got != want)), int(np.flatnonzero((got != want).ravel())[0]))
                b = host(buf)
                assert (b[:GUARD] == FILL).all() and (b[GUARD + T * fb:] == FILL).all()


# ---- 4: a payload moved by one sample, both bit depths ----------------------------------------------------------------------------------------------
PAD = 16
MOVES = [(True, False), (False, True), (True, True)]              # (src moved, dst moved)


class Moved:
    """``t`` payloads of ``fb`` bytes inside a buffer of t * fb + 16 bytes filled with FILL: viewed from byte 2 at 10 bit, byte 1 at 8 bit (a base
    moved by one sample) or from byte 0.  ``stays()``: every byte beside the payloads still holds FILL."""

    def __init__(self, fmt, t, fb, moved, data=None):
        self.off, self.n = (HW.esz(fmt) if moved else 0), t * fb
        self.buf = torch.full((self.n + PAD,), FILL, dtype=torch.uint8, device="cuda")
        self.view = self.buf[self.off:self.off + self.n].view(t, fb)
        assert self.view.data_ptr() % 16 == self.off and self.view.is_contiguous()
        if data is not None:
            self.view.copy_(torch.from_numpy(data))

    def stays(self):
        b = host(self.buf)
        return bool((b[:self.off] == FILL).all() and (b[self.off + self.n:] == FILL).all())


def each_move(fmt, src, t_out, call, want, in_place=False):
    """``call(s, o)`` fills o from s: with src, dst and both moved by one sample it must give ``want`` and leave the bytes beside both payloads;
    ``in_place``: also with o = s, moved."""
    fb = src.shape[1]
    for sm, dm in MOVES:
        s, o = Moved(fmt, len(src), fb, sm, src), Moved(fmt, t_out, fb, dm)
        call(s.view, o.view)
        got = host(o.view)
        assert np.array_equal(got, want), (fmt, sm, dm, int(np.sum(got != want)), int(np.flatnonzero((got != want).ravel())[0]))
        assert np.array_equal(host(s.view), src) and s.stays() and o.stays(), (fmt, sm, dm)
    if in_place:
        s = Moved(fmt, len(src), fb, True, src)
        call(s.view, s.view)
        assert np.array_equal(host(s.view), want) and s.stays(), fmt


@by_fmt
def test_degrade_of_payloads_moved_by_one_sample(fmt, gauss):
    f = yuv_fmt(*fmt)
    for H, W in SHAPES:
        src = clean(fmt, H, W, seed=3)
        want = DR.degrade_ref(src, fmt, H, W, DR.FALLING, SEED, T0)
        each_move(fmt, src, T, lambda s, o: degrade_yuv(s, f, H, W, DR.FALLING, SEED, T0, gauss, out=o), want)


@by_fmt
def test_blur_of_payloads_moved_by_one_sample(fmt, tables):
    f = yuv_fmt(*fmt)
    for H, W in SHAPES:
        src = clean(fmt, H, W, seed=3, t=S)
        want = B.blur_ref(src, fmt, H, W, 5, 2, T, 0, 6, GAMMA)
        each_move(fmt, src, T, lambda s, o: blur_yuv(s, f, H, W, 5, 2, 0, 6, tables, out=o), want)


@by_fmt
def test_grain_of_payloads_moved_by_one_sample_also_in_place(fmt, gauss):
    f = yuv_fmt(*fmt)
    for H, W in SHAPES:
        src = clean(fmt, H, W, seed=3)
        want = GR.grain_ref(src, fmt, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0)
        each_move(fmt, src, T, lambda s, o: grain_yuv(s, f, H, W, GR.BUMPY, SIZED, 0.5, SEED, T0, gauss, out=o), want, in_place=True)


@by_fmt
def test_tables_and_histogram_of_payloads_moved_by_one_sample(fmt):
    f = yuv_fmt(*fmt)
    for H, W in SHAPES:
        src = words(fmt, H, W, T, seed=H + W)
        lut = random_luts(fmt, T)
        dl = dev(lut.view(np.int16))
        each_move(fmt, src, T, lambda s, o: apply_lut_yuv(s, f, H, W, dl, out=o), FR.apply_ref(src, lut, fmt, H, W), in_place=True)
        s = Moved(fmt, T, src.shape[1], True, src)                  # the histogram: src moved
        got = host(code_hist_yuv(s.view, f, H, W)).view(np.uint32).astype(np.int64)
        want = FR.hist_ref(src, fmt, H, W)
        assert got.shape == (T, 1 << fmt.bits) and np.array_equal(got, want), int(np.sum(got != want))
        assert np.array_equal(host(s.view), src) and s.stays()


@by_fmt
def test_mixed_egress_with_ref_and_dst_at_different_alignments(fmt):
    f = yuv_fmt(*fmt)
    for H, W in SHAPES:
        fb = R.frame_bytes(fmt, H, W)
        inp = M.random_payloads(fmt, T, H, W, seed=7 + H)
        x = tensor(T, *padded(H, W), seed=W)
        xd, xh = x.cuda(), x.numpy()
        for mix in MIXES:
            want = M.egress(xh, fmt, H, W, mix, inp, DITHERS[1])
            for rm, dm in ((True, False), (False, True)):           # ref moved and dst not; dst moved and ref not
                r, o = Moved(fmt, T, fb, rm, inp), Moved(fmt, T, fb, dm)
                egress_yuv(xd, f, H, W, dst=o.view, dither=DITHERS[1], mix=mix, ref=r.view)
                got = host(o.view)
                assert np.array_equal(got, want), (H, W, mix, rm, dm, int(np.sum(got != want)), int(np.flatnonzero((got != want).ravel())[0]))
                assert np.array_equal(host(r.view), inp) and r.stays() and o.stays()


# ---- 5: seed and frame number at the top of their range ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [FORMATS[2], FORMATS[5]], **ids)   # 8-bit 4:2:0 left, 10-bit 4:2:0 centre
def test_the_largest_seed_and_frame_number_give_the_references_bytes_and_other_noise(fmt, gauss):
    """``egress_yuv``'s dither takes the same range as the two noise wrappers, 0 <= seed < 2^32 and 0 <= t0 <= 2^31 - 1 - T: all three run at its top.
    The kernels form t0 + (uint32_t)t on the device, the references (f0 & 0xFFFFFFFF) + t on the host."""
    f = yuv_fmt(*fmt)
    H, W = ODD
    assert (SEED_MAX, T0_MAX) == (2 ** 32 - 1, 2 ** 31 - 1 - T)
    src = clean(fmt, H, W, seed=21)
    d = dev(src)
    x = tensor(T, *padded(H, W), seed=5)
    xd, xh = x.cuda(), x.numpy()
    runs = [("degrade", lambda s, t0: host(degrade_yuv(d, f, H, W, DR.FALLING, s, t0, gauss)), lambda s, t0: DR.degrade_ref(src, fmt, H, W, DR.FALLING, s, t0))]
    for name, taps in (("grain sized", SIZED), ("grain white", WHITE)):
        runs.append((name, lambda s, t0, taps=taps: host(grain_yuv(d, f, H, W, GR.BUMPY, taps, 0.5, s, t0, gauss)),
                     lambda s, t0, taps=taps: GR.grain_ref(src, fmt, H, W, GR.BUMPY, taps, 0.5, s, t0)))
    runs.append(("dither", lambda s, t0: host(egress_yuv(xd, f, H, W, dither=(s, t0))), lambda s, t0: D.egress(xh, fmt, H, W, s, t0)))
    for name, on_device, ref in runs:
        far, near = on_device(SEED_MAX, T0_MAX), on_device(SEED, T0)
        want = ref(SEED_MAX, T0_MAX)
        assert np.array_equal(far, want), (name, int(np.sum(far != want)))
        assert np.array_equal(near, ref(SEED, T0)), name
        assert not np.array_equal(far, near), name
    for call in (lambda: degrade_yuv(d, f, H, W, DR.FALLING, SEED_MAX, T0_MAX + 1, gauss), lambda: egress_yuv(xd, f, H, W, dither=(SEED_MAX, T0_MAX + 1)),
                 lambda: grain_yuv(d, f, H, W, GR.BUMPY, SIZED, 0.5, SEED_MAX, T0_MAX + 1, gauss)):
        with pytest.raises(ValueError, match="t0"):                 # one past the top is refused on the host
            call()


# ---- 6: one launch or several, across the tile seam -------------------------------------------------------------------------------------------------
@by_fmt
def test_degrade_in_one_launch_is_three_launches_of_one_frame_at_the_wide_shape(fmt, gauss):
    f = yuv_fmt(*fmt)
    H, W = WIDE
    d = dev(clean(fmt, H, W, seed=11))
    whole = degrade_yuv(d, f, H, W, DR.FALLING, SEED, T0, gauss)
    singly = torch.cat([degrade_yuv(d[t:t + 1], f, H, W, DR.FALLING, SEED, T0 + t, gauss) for t in range(T)])
    assert torch.equal(whole, singly)
    assert not torch.equal(whole[:1], degrade_yuv(d[:1], f, H, W, DR.FALLING, SEED, T0 + 1, gauss))      # ... and the frame number matters
