"""-m gpu: ``sn_time_crossfade`` (csrc/sn_time.hip), the cross-fade of the frames two overlapping windows share and the exact sum of squares of the
two answers' difference, against the numpy / Python-integer restatement of tests/time_ref.py bit for bit; what it must leave alone; its argument checks."""
import numpy as np
import pytest
import torch

import time_ref as TR
from shiftnet_amd import lib as L
from shiftnet_amd.io_edges import time_crossfade

pytestmark = pytest.mark.gpu

GUARD = 64                               # floats kept on either side of cur (64 floats keep its 16-byte alignment), and int64 words around sq
SENTINEL = -0x0123456789ABCDEF


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def operands(rng, shape):
    """(prev, cur) float32 [V, C, Hp, Wp], all finite: pictures in [0, 1] with an overshoot below 0 and above 1, differences of about a code and of a
    good part of the range; one sample in 16 with a difference beyond +-8, which the statistic clamps; one in 8 with ``(prev - cur) * 65536`` exactly
    on k + 0.5, k of both signs and both parities, which the statistic rounds to the even neighbour."""
    V, C, Hp, Wp = shape
    cur = rng.uniform(-0.25, 1.25, shape)
    prev = cur + np.where(rng.random(shape) < 0.5, rng.normal(0.0, 1.0 / 255.0, shape), rng.normal(0.0, 0.2, shape))
    prev, cur = prev.astype(np.float32), cur.astype(np.float32)
    far = rng.random(shape) < 1.0 / 16.0
    prev = np.where(far, (cur + rng.choice([-1.0, 1.0], shape) * rng.uniform(8.0, 40.0, shape)).astype(np.float32), prev)
    tie = (rng.random(shape) < 0.125) & ~far
    grid = rng.integers(-(1 << 15), 1 << 17, shape)                                  # cur on the grid of 2^-17, inside (-0.25, 1]: exact in float32
    k = rng.integers(-70000, 70000, shape)                                           # |d| up to about 1.07: prev stays below 2^7 * 2^-17 * 2^24
    cur = np.where(tie, (grid / 131072.0), cur).astype(np.float32)
    prev = np.where(tie, ((grid + 2 * k + 1) / 131072.0), prev).astype(np.float32)
    d = (prev - cur).astype(np.float32)
    frac = (d.astype(np.float64) * 65536.0) % 1.0
    assert np.isfinite(prev).all() and np.isfinite(cur).all()
    assert (frac[tie] == 0.5).all()                                                  # the ties are exact ties in float32
    return prev, cur, int(tie.sum()), int((np.abs(d) > 8).sum())


class Case:
    """prev, cur and sq inside larger device buffers -- cur ``cur_shift`` floats and prev ``prev_shift`` floats off 16-byte alignment -- with host twins."""

    def __init__(self, rng, shape, cur_shift=0, prev_shift=0, weights=None):
        V, C, Hp, Wp = shape
        self.shape, self.n = shape, V * C * Hp * Wp
        self.prev, cur, self.ties, self.far = operands(rng, shape)
        self.lo = GUARD + cur_shift
        self.host = rng.standard_normal(self.n + 2 * GUARD + 4).astype(np.float32)
        self.host[self.lo:self.lo + self.n] = cur.ravel()
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.cur = self.dev[self.lo:self.lo + self.n].view(shape)
        assert self.cur.data_ptr() % 16 == 4 * cur_shift
        pstore = torch.zeros(self.n + 4, dtype=torch.float32, device="cuda")
        self.pdev = pstore[prev_shift:prev_shift + self.n].view(shape)
        self.pdev.copy_(torch.from_numpy(self.prev))
        assert self.pdev.data_ptr() % 16 == 4 * prev_shift
        if weights is None:                                                          # any float32 is legal: above 1, below 0, exact 0 and 1
            weights = rng.uniform(-0.5, 1.5, V).astype(np.float32), rng.uniform(-0.5, 1.5, V).astype(np.float32)
        self.w_prev, self.w_cur = weights
        self.wp, self.wc = torch.from_numpy(self.w_prev.copy()).cuda(), torch.from_numpy(self.w_cur.copy()).cuda()
        self.sq_all = torch.full((V * C + 2 * GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
        self.sq = self.sq_all[GUARD:GUARD + V * C].view(V, C)
        self.sq.zero_()
        self.want_sq = [[0] * C for _ in range(V)]

    def want(self):
        return self.host[self.lo:self.lo + self.n].reshape(self.shape)                # a view of the host twin

    def step(self, h, w, stat=True):
        """One launch and its restatement on the host twin."""
        cur = self.want()
        if stat:
            add = TR.seam_sq(self.prev, cur, h, w)
            self.want_sq = [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(self.want_sq, add)]
        cur[...] = TR.crossfade(self.prev, cur, self.w_prev, self.w_cur)
        assert time_crossfade(self.pdev, self.cur, self.wp, self.wc, h, w, sq=self.sq if stat else None) is self.cur

    def check(self, what):
        got = self.dev.cpu().numpy()
        assert np.array_equal(bits(got[self.lo:self.lo + self.n]), bits(self.host[self.lo:self.lo + self.n])), what
        assert np.array_equal(bits(got[:self.lo]), bits(self.host[:self.lo])) and np.array_equal(bits(got[self.lo + self.n:]), bits(self.host[self.lo + self.n:])), what
        assert np.array_equal(bits(self.pdev.cpu().numpy()), bits(self.prev)), what                      # prev is read only
        sq = self.sq_all.cpu().numpy()
        V, C = self.shape[:2]
        assert (sq[:GUARD] == SENTINEL).all() and (sq[GUARD + V * C:] == SENTINEL).all(), what
        assert [[int(v) for v in row] for row in sq[GUARD:GUARD + V * C].reshape(V, C)] == self.want_sq, what


# (V, C, Hp, Wp, h, w), cur's and prev's offset from 16-byte alignment in floats
CASES = [((1, 3, 4, 4, 4, 4), 0, 0),
         ((2, 3, 8, 12, 5, 9), 0, 0),                 # padding, which the statistic leaves out
         ((3, 1, 7, 13, 7, 13), 0, 0),                # odd planes: the later planes and rows are off 16-byte alignment
         ((2, 3, 68, 260, 67, 257), 0, 0),            # more than one workgroup per row and per plane; a row's last thread owns fewer than 4 samples
         ((2, 3, 8, 12, 5, 9), 1, 0),                 # cur starts one element past a 16-byte boundary: the element path everywhere
         ((2, 2, 9, 16, 9, 14), 0, 3),                # ... and prev alone off it
         ((2, 3, 68, 260, 67, 257), 1, 1)]


@pytest.mark.parametrize("shape,cur_shift,prev_shift", CASES)
def test_the_kernel_equals_the_restatement_bit_for_bit_and_touches_nothing_else(shape, cur_shift, prev_shift):
    V, C, Hp, Wp, h, w = shape
    rng = np.random.default_rng(sum(shape) + 7 * cur_shift + 11 * prev_shift)
    c = Case(rng, (V, C, Hp, Wp), cur_shift, prev_shift, weights=TR.weights(V) if cur_shift == prev_shift else None)
    if c.n >= 64:
        assert c.ties >= 1 and c.far >= 1
    c.step(h, w)
    c.check(("first", shape))
    assert any(v > 0 for row in c.want_sq for v in row)
    c.step(h, w)                                     # sq is added to, not overwritten: the second launch's sums (of the blended cur) come on top
    c.check(("second", shape))
    first = c.want().copy()
    c.step(h, w, stat=False)                         # without sq: the same arithmetic, and sq stays
    c.check(("no sq", shape))
    assert not np.array_equal(first, c.want())


def test_without_the_statistic_cur_is_the_same():
    shape = (2, 3, 68, 260)
    a = Case(np.random.default_rng(5), shape)
    b = Case(np.random.default_rng(5), shape)
    a.step(67, 257, stat=True)
    b.step(67, 257, stat=False)
    assert np.array_equal(bits(a.cur.cpu().numpy()), bits(b.cur.cpu().numpy()))
    a.check("with sq")
    b.check("without sq")
    assert b.want_sq == [[0] * 3] * 2


def test_the_clamp_and_the_tie_rule_on_hand_picked_values():
    """d * 65536 = 0.5, 1.5, 2.5, -0.5, -1.5, -2.5 round to 0, 2, 2, 0, -2, -2; differences of 8, 9 and -1000 all count as 8."""
    d = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5], dtype=np.float64) / 65536.0
    cur = np.zeros((1, 1, 2, 6), dtype=np.float32)
    prev = np.zeros((1, 1, 2, 6), dtype=np.float32)
    prev[0, 0, 0] = d
    prev[0, 0, 1, :3] = [8.0, 9.0, -1000.0]
    want = 0 + 4 + 4 + 0 + 4 + 4 + 3 * (8 * 65536) ** 2
    assert TR.seam_sq(prev, cur, 2, 6) == [[want]]
    sq = torch.zeros((1, 1), dtype=torch.int64, device="cuda")
    one = torch.ones(1, device="cuda")
    time_crossfade(torch.from_numpy(prev).cuda(), torch.from_numpy(cur).cuda(), one, one, 2, 6, sq=sq)
    assert int(sq[0, 0]) == want


def test_illegal_arguments_are_refused_before_anything_is_launched():
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    GARBAGE = 1234.5
    V, C, Hp, Wp = 2, 3, 8, 12
    cur = torch.full((V, C, Hp, Wp), GARBAGE, device="cuda")
    prev = torch.ones((V, C, Hp, Wp), device="cuda")
    w = torch.ones(V + 2, device="cuda")
    sq = torch.full((V * C + 1,), 77, dtype=torch.int64, device="cuda")
    p, c, a, q = prev.data_ptr(), cur.data_ptr(), w.data_ptr(), sq.data_ptr()

    def call(pp=p, cp=c, ap=a, bp=a, sp=q, V=V, C=C, Hp=Hp, Wp=Wp, h=Hp, w=Wp):
        return lib.sn_time_crossfade(pp, cp, ap, bp, sp, V, C, Hp, Wp, h, w, s)
    for kw in ({"pp": None}, {"cp": None}, {"ap": None}, {"bp": None},                                   # a null pointer
               {"pp": p + 2}, {"cp": c + 1}, {"ap": a + 2}, {"bp": a + 3}, {"sp": q + 4}, {"sp": q + 2},     # 4-byte alignment, 8 for sq
               {"V": 0}, {"C": 0}, {"Hp": 0}, {"Wp": 0}, {"V": -1}, {"Hp": -8},                              # a size below 1
               {"h": 0}, {"w": 0}, {"h": Hp + 1}, {"w": Wp + 1}, {"h": -1}, {"w": 2 ** 31 - 1},              # a picture outside the plane
               {"V": 21846, "C": 3}, {"V": 65536, "C": 1}, {"V": 2 ** 16, "C": 2 ** 16},                   # V * C > 65535 (the last: a product past 2^31)
               {"Hp": 8192, "Wp": 4097, "h": 8192, "w": 4097}):                                            # with sq: h * w > 2^25
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert bool((cur == GARBAGE).all()) and bool((sq == 77).all())                   # nothing was launched
    assert call(pp=p + 4, cp=c + 4, ap=a + 4, bp=a + 8, sp=q + 8, V=1, Hp=Hp - 1, h=1, w=1) == 0      # legal: 4-byte alignment, 8 for sq, the smallest picture
    assert call(sp=None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="float32"):
        time_crossfade(prev.half(), cur, w[:V], w[:V], Hp, Wp)
    with pytest.raises(ValueError, match="prev of its shape"):
        time_crossfade(prev[:1], cur, w[:V], w[:V], Hp, Wp)
    with pytest.raises(ValueError, match="weights"):
        time_crossfade(prev, cur, w[:V], w[:V + 1], Hp, Wp)
    with pytest.raises(ValueError, match="contiguous"):
        time_crossfade(prev, cur[..., ::2], w[:V], w[:V], Hp, Wp // 2)
    with pytest.raises(ValueError, match="inside the plane"):
        time_crossfade(prev, cur, w[:V], w[:V], Hp + 1, Wp)
    with pytest.raises(ValueError, match="sq"):
        time_crossfade(prev, cur, w[:V], w[:V], Hp, Wp, sq=sq[:V * C].view(V, C).int())
