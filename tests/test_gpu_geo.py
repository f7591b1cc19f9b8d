"""-m gpu: the two kernels of the self-ensemble (csrc/sn_geo.hip) against the numpy restatement of tests/geo_ref.py, bit for bit: every op, both element
sizes, shapes for every path of the kernels, guard bands around what is written."""
import numpy as np
import pytest
import torch

import geo_ref as G
from shiftnet_amd import lib as L
from shiftnet_amd.io_edges import geo_accumulate, geo_out_shape, geo_transform

pytestmark = pytest.mark.gpu

GUARD = 64                               # elements kept on either side of what is written: 64 keep a 16-byte alignment for both element sizes
SHAPES = [(3, 3, 5, 7),                  # everything on the element path
          (2, 3, 64, 64),                # whole tiles, the wide path
          (2, 1, 66, 130),               # partial tiles on both axes; W * 2 is no multiple of 16, so the mirrored chunk is misaligned
          (1, 2, 1, 40), (1, 2, 40, 1)]  # a side of one
NP = {2: np.int16, 4: np.int32}
TORCH = {2: torch.int16, 4: torch.int32}


def ramp(shape, esz):
    """Distinct values (the largest shape has 24576 elements: they fit 15 bits), so that a misplaced element cannot pass."""
    n = int(np.prod(shape))
    assert n < 2 ** 15
    return (np.arange(n) + 1).reshape(shape).astype(NP[esz])


class Banded:
    """``n`` elements inside a larger device buffer, ``shift`` elements off 16-byte alignment, with a sentinel around and under them."""

    def __init__(self, n, dtype, sentinel, shift=0):
        self.n, self.lo = n, GUARD + shift
        self.dev = torch.full((n + 2 * GUARD + 8,), sentinel, dtype=dtype, device="cuda")
        assert self.dev.data_ptr() % 16 == 0
        self.sentinel = self.dev.cpu().numpy().copy()

    def view(self, shape):
        return self.dev[self.lo:self.lo + self.n].view(*shape)

    def check(self, want, what):
        got = self.dev.cpu().numpy()
        inner = got[self.lo:self.lo + self.n]
        assert np.array_equal(inner.view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)), what
        assert np.array_equal(got[:self.lo].view(np.uint8), self.sentinel[:self.lo].view(np.uint8)), what                  # the bytes around dst are untouched
        assert np.array_equal(got[self.lo + self.n:].view(np.uint8), self.sentinel[self.lo + self.n:].view(np.uint8)), what


@pytest.mark.parametrize("esz", [2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_transform_equals_the_restatement_for_all_16_ops(shape, esz):
    a = ramp(shape, esz)
    n = a.size
    for shift in ((0, 1) if shape == (2, 3, 64, 64) else (0,)):                      # one case: src and dst one element off an aligned base
        src = Banded(n, TORCH[esz], 0, shift)
        src.view(shape).copy_(torch.from_numpy(a))
        for op in range(16):
            dst = Banded(n, TORCH[esz], -7, shift)
            out = dst.view(geo_out_shape(shape, op))
            assert geo_transform(src.view(shape), op, out=out) is out
            dst.check(G.transform(a, op), (shape, esz, op, shift))
        src.check(a, (shape, esz, "src"))                                            # and the source is only read


def test_transform_moves_bf16_and_float32_and_allocates_its_result():
    rng = np.random.default_rng(5)
    a32 = rng.standard_normal((2, 3, 12, 20)).astype(np.float32)
    for op in (0, 3, 5, 14):
        got = geo_transform(torch.from_numpy(a32).cuda(), op)
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy().view(np.uint32), G.transform(a32, op).view(np.uint32))
        b = torch.from_numpy(a32).cuda().to(torch.bfloat16)
        got = geo_transform(b, op)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == G.out_shape(a32.shape, op)
        assert np.array_equal(got.view(torch.int16).cpu().numpy(), G.transform(b.view(torch.int16).cpu().numpy(), op))


def values(rng, shape):
    """float32 of both signs: most of magnitude about 1, one in eight up to 1e4, exact +0.0 and -0.0 among them."""
    v = rng.standard_normal(shape)
    v = np.where(rng.random(shape) < 0.125, rng.uniform(-1e4, 1e4, shape), v)
    v = np.where(rng.random(shape) < 0.04, 0.0, v)
    v = np.where((v == 0.0) & (rng.random(shape) < 0.5), -0.0, v).astype(np.float32)
    v.reshape(-1)[0] = -0.0
    return v


@pytest.mark.parametrize("shape", SHAPES)
def test_accumulate_equals_the_restatement_for_all_16_ops(shape):
    rng = np.random.default_rng(sum(shape))
    n = int(np.prod(shape))
    for op in range(16):
        for init in (0, 1):
            for scale in (1.0, 0.125):
                member = values(rng, G.out_shape(shape, op))
                if init:
                    start = np.full(shape, np.nan, np.float32)                       # a canvas that must not be read: NaN would leak
                else:
                    start = values(rng, shape)
                    start.reshape(-1)[0] = -0.0                                      # -0 + -0 = -0 where the member's -0 lands on it (op 0)
                canvas = Banded(n, torch.float32, 1234.5)
                view = canvas.view(shape)
                view.copy_(torch.from_numpy(start))
                mdev = torch.from_numpy(member).cuda()
                assert geo_accumulate(mdev, view, op, bool(init), scale) is view
                want = G.accumulate(start.copy(), member, op, init, scale)
                assert not np.isnan(want).any()
                canvas.check(want, (shape, op, init, scale))
                assert np.array_equal(mdev.cpu().numpy().view(np.uint32), member.view(np.uint32))


def test_accumulate_off_alignment_and_a_sequence_of_members_is_the_sequential_sum():
    rng = np.random.default_rng(11)
    shape = (2, 3, 64, 64)
    for shift in (1, 2):
        canvas = Banded(int(np.prod(shape)), torch.float32, 1234.5, shift)
        view = canvas.view(shape)
        want = np.full(shape, np.nan, np.float32)
        ops = [0, 1, 6, 13]
        for i, op in enumerate(ops):
            member = values(rng, G.out_shape(shape, op))
            store = torch.zeros(member.size + 4, dtype=torch.float32, device="cuda")
            mdev = store[shift:shift + member.size].view(*member.shape)
            mdev.copy_(torch.from_numpy(member))
            scale = 0.25 if i == len(ops) - 1 else 1.0
            geo_accumulate(mdev, view, op, i == 0, scale)
            G.accumulate(want, member, op, i == 0, scale)
        canvas.check(want, shift)


def test_illegal_arguments_are_refused_before_anything_is_launched():
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    GARBAGE = 1234.5
    dst = torch.full((2, 3, 8, 8), GARBAGE, device="cuda")
    src = torch.ones((2, 3, 8, 8), device="cuda")
    a, b = src.data_ptr(), dst.data_ptr()

    def tr(sp=a, dp=b, esz=4, op=0, T=2, C=3, H=8, W=8):
        return lib.sn_geo_transform(sp, dp, esz, op, T, C, H, W, s)

    def ac(mp=a, cp=b, op=0, init=0, scale=1.0, T=2, C=3, H=8, W=8):
        return lib.sn_geo_accumulate(mp, cp, op, init, scale, T, C, H, W, s)
    for kw in ({"sp": None}, {"dp": None}, {"esz": 3}, {"esz": 8}, {"op": 16}, {"op": -1}, {"H": 0}, {"W": 0}, {"T": 0}, {"C": -1}, {"sp": a + 2}, {"dp": b + 1},
               {"dp": a}, {"sp": b + 4 * 191, "T": 1}, {"T": 2 ** 31 - 1, "C": 2 ** 31 - 1, "H": 2 ** 31 - 1, "W": 2 ** 31 - 1}):
        assert tr(**kw) == -22, kw
    for kw in ({"mp": None}, {"cp": None}, {"op": 16}, {"H": 0}, {"mp": a + 2}, {"cp": b + 2}, {"mp": b}, {"scale": float("inf")}, {"scale": float("nan")}):
        assert ac(**kw) == -22, kw
    torch.cuda.synchronize()
    assert bool((dst == GARBAGE).all())                                              # nothing was launched
    assert tr(op=15) == 0 and ac(op=7, init=1, scale=0.5) == 0                       # legal
    torch.cuda.synchronize()
    assert bool((dst == 0.5).all())
    with pytest.raises(ValueError, match="op"):
        geo_transform(src, 16)
    with pytest.raises(ValueError, match="contiguous"):
        geo_transform(src[..., ::2], 0)
    with pytest.raises(ValueError, match="takes"):
        geo_transform(src, 4, out=dst[:1])
    with pytest.raises(ValueError, match="float32"):
        geo_accumulate(src.half(), dst.half(), 0, True)
    with pytest.raises(ValueError, match="finite"):
        geo_accumulate(src, dst, 0, True, float("inf"))
